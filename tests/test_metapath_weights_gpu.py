"""Weighted meta-path graphs on the GPU (K0: han_spgemm_values, han_csr_pathsim, han_csr_row_topk_*), all by exact
equality against the NumPy / scipy references of tests/metapath_weights_ref.py computed from the GPU-generated
relations copied to the host: the counted product on the operand pairs of tests/test_metapath_gpu.py (both row bins
and their boundary, the bit-map tiles, repeated entries, operand counts up to 2^20), instance counts / PathSim / top-k
of APA, APCPA and APTPA on the DBLP-like relations (the H Hᵀ plan and the full chain agree), PAP at 3 M papers, and
the model on the weighted graphs."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from han_amd import metapath, ops, synth
from han_amd.graph import CSRGraph
from tests import metapath_weights_ref as ref

pytestmark = pytest.mark.gpu

MPS = ("APA", "APCPA", "APTPA")


def _sp(g: CSRGraph, data=None):
    """scipy CSR of a graph as stored (repeats kept: scipy sums them in a product, as the kernels count them)."""
    data = np.ones(g.nnz, dtype=np.int64) if data is None else data
    return sp.csr_matrix((data, g.colidx.cpu().numpy(), g.rowptr.cpu().numpy()), shape=(g.n_rows, g.n_cols))


def _same_structure(a: CSRGraph, b: CSRGraph):
    return (a.n_rows, a.n_cols) == (b.n_rows, b.n_cols) and torch.equal(a.rowptr, b.rowptr) and \
        torch.equal(a.colidx, b.colidx)


def _graph(rows, n_cols, dev):
    """CSRGraph of per-row column lists taken AS GIVEN (unsorted, repeats kept)."""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rowptr[-1] else np.zeros(0, np.int32)
    return CSRGraph.from_arrays(rowptr, colidx, n_cols, device=dev)


def _pair(seed, n_rows, n_mid, n_cols, S, dev, n_random=300):
    """The operand pair of tests/test_metapath_gpu.py: B rows of 0, 1, S - 1, S, S + 1 and 5 S candidates (with
    repeats), A rows with bounds 0 (empty, and non-empty over empty B rows), S - 1, S, S + 1, long, and random unsorted
    rows with repeated entries; the other A rows are empty."""
    rng = np.random.default_rng(seed)
    deg = {0: 0, 1: 1, 2: S - 1, 3: S, 4: S + 1, 5: 5 * S}
    b_rows = []
    for l in range(n_mid):
        d = deg.get(l, int(rng.integers(0, 40)))
        b_rows.append(rng.integers(0, n_cols, d))
    a_rows = [[] for _ in range(n_rows)]
    a_rows[1] = [0, 0]
    a_rows[2], a_rows[3], a_rows[4], a_rows[5] = [2], [3], [4], [1, 3]
    a_rows[6] = [5, 2, 5]
    a_rows[n_rows - 1] = [1, 2]
    for i in rng.choice(np.arange(7, n_rows - 1), size=min(n_random, n_rows - 8), replace=False):
        a_rows[i] = rng.integers(0, n_mid, int(rng.integers(1, 30)))
    return _graph(a_rows, n_mid, dev), _graph(b_rows, n_cols, dev)


@pytest.mark.parametrize("S,tile", [(None, None), (64, 64), (4096, 1 << 19)])
@pytest.mark.parametrize("shape", ["rect", "square_diag", "wide"])
@pytest.mark.parametrize("operands", ["binary", "counts", "counts_2p20"])
def test_count_matmul_matches_scipy(dev, monkeypatch, S, tile, shape, operands):
    if S is not None:
        monkeypatch.setattr(ops, "SPGEMM_SHORT", S)
        monkeypatch.setattr(ops, "SPGEMM_TILE", tile)
    S, T = ops.SPGEMM_SHORT, ops.SPGEMM_TILE
    n_rows, n_mid, n_cols, diag = {"rect": (400, 60, 700, False), "square_diag": (900, 60, 900, True),
                                   "wide": (300, 40, 2 * T + 77, False)}[shape]    # wide: three bit-map tiles
    A, B = _pair(7, n_rows, n_mid, n_cols, S, dev)
    rng = np.random.default_rng(11)
    ac = bc = None
    if operands != "binary":        # positive, so that no stored sum cancels to 0 and the structure is the boolean one
        lo, hi = (1, 1000) if operands == "counts" else ((1 << 20) - 1000, (1 << 20) + 1000)
        ac, bc = rng.integers(lo, hi, A.nnz, dtype=np.int64), rng.integers(lo, hi, B.nnz, dtype=np.int64)
    dv = lambda x: None if x is None else torch.as_tensor(x).to(dev)
    C, counts = ops.csr_count_matmul(A, B, a_counts=dv(ac), b_counts=dv(bc), diag=diag)
    assert counts.dtype == torch.int64 and counts.shape == (C.nnz,) and counts.device == C.device
    assert C.values is None and _same_structure(C, ops.csr_bool_matmul(A, B, diag=diag))
    want = ref.counted(_sp(A, ac) @ _sp(B, bc), diag)
    np.testing.assert_array_equal(C.rowptr.cpu().numpy(), want.indptr.astype(np.int64))
    np.testing.assert_array_equal(C.colidx.cpu().numpy(), want.indices.astype(np.int32))
    np.testing.assert_array_equal(counts.cpu().numpy(), want.data)
    if operands == "counts_2p20":
        assert int(counts.max()) > 1 << 40          # beyond any 32-bit or fp32 accumulation
    C2, again = ops.csr_count_matmul(A, B, a_counts=dv(ac), b_counts=dv(bc), diag=diag)
    assert _same_structure(C, C2) and torch.equal(counts, again)


def test_count_matmul_degenerate_inputs_and_errors(dev):
    e = lambda r, c: CSRGraph(torch.zeros(r + 1, dtype=torch.int64, device=dev),
                              torch.zeros(0, dtype=torch.int32, device=dev), c)
    B = _graph([[0, 3], [], [2, 2, 1]], 4, dev)
    C, counts = ops.csr_count_matmul(e(5, 3), B)
    assert C.nnz == 0 and counts.numel() == 0 and counts.dtype == torch.int64
    C, counts = ops.csr_count_matmul(e(4, 3), B, diag=True)      # the diagonal alone, without instances
    assert C.colidx.tolist() == [0, 1, 2, 3] and counts.tolist() == [0, 0, 0, 0]
    C, counts = ops.csr_count_matmul(e(0, 3), B)
    assert C.n_rows == 0 and counts.numel() == 0
    A = _graph([[2, 2], [0, 2], []], 3, dev)                     # a repeated stored entry counts per repetition
    C, counts = ops.csr_count_matmul(A, B)
    assert C.rowptr.tolist() == [0, 2, 6, 6] and C.colidx.tolist() == [1, 2, 0, 1, 2, 3]
    assert counts.tolist() == [2, 4, 1, 1, 2, 1]
    np.testing.assert_array_equal(counts.cpu().numpy(), ref.counted(_sp(A) @ _sp(B)).data)
    with pytest.raises(ValueError, match="columns"):
        ops.csr_count_matmul(A, e(4, 2))
    with pytest.raises(ValueError, match="a_counts"):
        ops.csr_count_matmul(A, B, a_counts=torch.ones(A.nnz + 1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="b_counts"):
        ops.csr_count_matmul(A, B, b_counts=torch.ones(B.nnz, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="a_counts"):
        ops.csr_count_matmul(A, B, a_counts=torch.ones(A.nnz, dtype=torch.int64))
    g = CSRGraph(C.rowptr, C.colidx, C.n_cols, values=counts.float())
    with pytest.raises(ValueError, match="k ="):
        ops.csr_row_topk(g, 0)
    with pytest.raises(ValueError, match="counts"):
        ops.csr_pathsim(e(3, 3), torch.zeros(2, dtype=torch.int64, device=dev))


@pytest.fixture(scope="module")
def dblp():
    dev = torch.device("cuda:0")
    rel, sizes = synth.hetero_relations("dblp-like", device=dev)
    return rel, {k: _sp(g) for k, g in rel.items()}, sizes


_chains = {}


def _chain(host, rel, mp):
    """The counted scipy chain of `mp` with the diagonal (cached per meta-path: APTPA takes seconds)."""
    if mp not in _chains:
        hops = metapath.plan(rel, mp)["hops"]
        _chains[mp] = ref.count_chain([sp.csr_matrix(host[k].T) if t else host[k] for k, t in hops], diag=True)
    return _chains[mp]


def _assert_graph(g: CSRGraph, indptr, indices, values):
    np.testing.assert_array_equal(g.rowptr.cpu().numpy(), np.asarray(indptr, dtype=np.int64))
    np.testing.assert_array_equal(g.colidx.cpu().numpy(), np.asarray(indices, dtype=np.int32))
    got = g.values.cpu().numpy()
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), np.asarray(values, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("mp", MPS)
def test_dblp_like_counts(dev, dblp, mp):
    rel, host, sizes = dblp
    m = _chain(host, rel, mp)
    g = metapath.metapath_graph(rel, mp, weights="count")
    assert _same_structure(g, metapath.metapath_graph(rel, mp))                 # bitwise the boolean graph
    assert int(m.data.max()) < 1 << 24                                          # fp32 holds every count exactly
    _assert_graph(g, m.indptr, m.indices, m.data.astype(np.float32))
    p = metapath.plan(rel, mp)
    assert p["split"] == len(mp) // 2                                           # g came from H Hᵀ; the chain agrees:
    full = metapath.compose([rel[k].transpose() if t else rel[k] for k, t in p["hops"]], self_loops=True,
                            weights="count")
    _assert_graph(full, m.indptr, m.indices, m.data.astype(np.float32))
    again = metapath.metapath_graph(rel, mp, weights="count")
    assert _same_structure(g, again) and torch.equal(g.values, again.values)


@pytest.mark.parametrize("mp", MPS)
def test_dblp_like_pathsim(dev, dblp, mp):
    rel, host, sizes = dblp
    m = _chain(host, rel, mp)
    g = metapath.metapath_graph(rel, mp, weights="pathsim")
    rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
    d = m.diagonal()
    assert (d > 0).all()                                                        # every author of the preset writes
    want = (2.0 * m.data / (d[rows] + d[m.indices])).astype(np.float32)
    _assert_graph(g, m.indptr, m.indices, want)
    np.testing.assert_array_equal(want, ref.pathsim(m.indptr, m.indices, m.data))
    vals = g.values.cpu().numpy()
    assert (vals[m.indices == rows] == 1.0).all() and (m.indices == rows).sum() == sizes["A"]
    assert vals.min() > 0.0 and vals.max() <= 1.0
    hops = [rel[k].transpose() if t else rel[k] for k, t in metapath.plan(rel, mp)["hops"]]
    _assert_graph(metapath.compose(hops, self_loops=True, weights="pathsim"), m.indptr, m.indices, want)


def test_pathsim_of_an_isolated_author(dev):
    # author 2 has no paper: no instance, so the self-loop alone, count 0 and PathSim exactly 1
    rel = {"AP": metapath.relation([0, 0, 1, 3, 3], [0, 1, 1, 2, 0], 4, 3, device=dev),
           "PC": metapath.relation([0, 1, 2], [0, 0, 1], 3, 2, device=dev)}
    for mp in ("APA", "APCPA"):
        c = metapath.metapath_graph(rel, mp, weights="count")
        g = metapath.metapath_graph(rel, mp, weights="pathsim")
        assert _same_structure(c, g)
        s, e = g.rowptr[2:4].tolist()
        assert e - s == 1 and g.colidx[s].item() == 2
        assert c.values[s].item() == 0.0 and g.values[s].item() == 1.0
        assert not bool((g.colidx[:s] == 2).any()) and not bool((g.colidx[e:] == 2).any())
        host = {k: _sp(v) for k, v in rel.items()}
        m = ref.count_chain([sp.csr_matrix(host[k].T) if t else host[k] for k, t in metapath.plan(rel, mp)["hops"]],
                            diag=True)
        _assert_graph(c, m.indptr, m.indices, m.data.astype(np.float32))
        _assert_graph(g, m.indptr, m.indices, ref.pathsim(m.indptr, m.indices, m.data))
    loose = metapath.metapath_graph(rel, "APA", self_loops=False, weights="pathsim")     # row 2 stays empty
    assert loose.rowptr[2].item() == loose.rowptr[3].item()


@pytest.mark.parametrize("k", [1, 8, 32, 10 ** 6])
@pytest.mark.parametrize("mp", MPS)
def test_dblp_like_top_k(dev, dblp, mp, k):
    rel, host, sizes = dblp
    m = _chain(host, rel, mp)
    w = ref.pathsim(m.indptr, m.indices, m.data)
    ptr, cols, vals = ref.topk(m.indptr, m.indices, w, k)
    g = metapath.metapath_graph(rel, mp, weights="pathsim", top_k=k)
    _assert_graph(g, ptr, cols, vals)
    # the properties, on the output itself
    n = sizes["A"]
    rp, ci = g.rowptr.cpu().numpy(), g.colidx.cpu().numpy()
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert ((ci == rows).sum() == n) and (np.diff(rp) <= k + 1).all()           # the diagonal kept, at most k besides
    assert ((ci[1:] > ci[:-1]) | (rows[1:] != rows[:-1])).all()                 # columns ascending
    whole = np.diff(m.indptr) - 1 <= k                                          # rows with at most k off-diagonal entries
    np.testing.assert_array_equal(np.diff(rp)[whole], np.diff(m.indptr)[whole])
    if k == 10 ** 6:
        assert whole.all()
    # counts rank the same way through ops.csr_row_topk, without the diagonal too
    gc = CSRGraph(torch.as_tensor(m.indptr.astype(np.int64)).to(dev), torch.as_tensor(m.indices.astype(np.int32)).to(dev),
                  n, values=torch.as_tensor(m.data.astype(np.float32)).to(dev))
    cut = ops.csr_row_topk(gc, k, keep_diag=False)
    _assert_graph(cut, *ref.topk(m.indptr, m.indices, m.data.astype(np.float32), k, keep_diag=False))


def test_pap_3m_counts_and_top_k(dev):
    rel, sizes = synth.hetero_relations("pap-3m", device=dev)
    pa = rel["PA"]
    n, n_a = sizes["P"], sizes["A"]
    g = metapath.metapath_graph(rel, "PAP", weights="count")
    assert g.n_rows == g.n_cols == n and g.values.dtype == torch.float32
    counts = g.values.to(torch.int64)
    deg_a = torch.bincount(pa.colidx.long(), minlength=n_a)
    assert int(counts.sum()) == int((deg_a * deg_a).sum())          # every (paper, author, paper) instance, int64
    del counts
    pa_rp, pa_ci = pa.rowptr.cpu().numpy(), pa.colidx.cpu().numpy()
    ap = sp.csr_matrix((np.ones(pa.nnz, dtype=bool), pa_ci, pa_rp), shape=(n, n_a)).T.tocsr()
    rp_h = g.rowptr.cpu().numpy()
    longest = int(torch.argmax(g.degrees()))
    rng = np.random.default_rng(3)
    sample = sorted({0, n - 1, longest} | set(rng.integers(0, n, 61).tolist()))
    assert rp_h[longest + 1] - rp_h[longest] > ops.SPGEMM_SHORT     # the bit-map bin is sampled too

    def row_ref(p):
        authors = pa_ci[pa_rp[p]:pa_rp[p + 1]]
        cols, cnt = np.unique(np.concatenate([ap.indices[ap.indptr[a]:ap.indptr[a + 1]] for a in authors]),
                              return_counts=True)
        assert p in cols                                            # every paper of the preset has an author
        return cols.astype(np.int32), cnt.astype(np.float32)

    for p in sample:
        cols, cnt = row_ref(p)
        s, e = rp_h[p], rp_h[p + 1]
        np.testing.assert_array_equal(g.colidx[s:e].cpu().numpy(), cols, err_msg=f"row {p}")
        np.testing.assert_array_equal(g.values[s:e].cpu().numpy(), cnt, err_msg=f"row {p}")
    del g
    torch.cuda.empty_cache()
    t = metapath.metapath_graph(rel, "PAP", weights="count", top_k=32)
    assert int(t.degrees().max()) <= 33 and int(t.degrees().min()) >= 1
    row_of = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), t.degrees())
    assert int((t.colidx == row_of).sum()) == n                     # every row holds its diagonal (once)
    del row_of
    tp = t.rowptr.cpu().numpy()
    for p in sample:
        cols, cnt = row_ref(p)
        keep = ref.topk_row(cols, cnt, p, 32)
        s, e = tp[p], tp[p + 1]
        np.testing.assert_array_equal(t.colidx[s:e].cpu().numpy(), cols[keep], err_msg=f"row {p}")
        np.testing.assert_array_equal(t.values[s:e].cpu().numpy(), cnt[keep], err_msg=f"row {p}")


def _model(sizes, dev):
    from han_amd.gat import HeteGAT_multi
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(sizes["A"], 64, generator=gen, device=dev)
    model = HeteGAT_multi().build(len(MPS), 64, 4, device=dev, generator=torch.Generator().manual_seed(5))
    return model, x, gen


def test_inference_on_pathsim_graphs_is_bitwise_the_host_built_graphs(dev, dblp):
    rel, host, sizes = dblp
    built = [metapath.metapath_graph(rel, mp, weights="pathsim") for mp in MPS]
    hosted = []
    for mp in MPS:
        m = _chain(host, rel, mp)
        g = CSRGraph.from_arrays(m.indptr, m.indices, sizes["A"], device=dev)
        hosted.append(CSRGraph(g.rowptr, g.colidx, g.n_cols,
                               values=torch.as_tensor(ref.pathsim(m.indptr, m.indices, m.data)).to(dev)))
    model, x, _ = _model(sizes, dev)
    with torch.no_grad():
        la, ea, aa = model.inference([x] * 3, 4, sizes["A"], False, 0.0, 0.0, built, [8], [8, 1])
        lb, eb, ab = model.inference([x] * 3, 4, sizes["A"], False, 0.0, 0.0, hosted, [8], [8, 1])
    assert torch.equal(la, lb) and torch.equal(ea, eb) and torch.equal(aa, ab)
    assert bool(torch.isfinite(la).all())


def test_forward_on_pathsim_top_k_graphs_matches_the_float64_oracle(dev, dblp):
    """One forward on the pathsim + top_k = 32 graphs against the float64 oracle fed the same stored values
    (sp_attn_head with adj_vals per head, SimpleAttLayer, the classifier): the 1e-4 bar of the parity tests."""
    from oracle import han_oracle as ho
    from tests.helpers import build_model
    rel, _, sizes = dblp
    n = sizes["A"]
    graphs = [metapath.metapath_graph(rel, mp, weights="pathsim", top_k=32) for mp in MPS]
    rng = np.random.default_rng(21)
    prob = dict(params=ho.init_params(rng, len(MPS), 64, 4), p=len(MPS), f=64, c=4)
    x = rng.standard_normal((1, n, 64))
    model, _ = build_model(prob, dev)
    xt = torch.tensor(x[0], dtype=torch.float32, device=dev)
    with torch.no_grad():
        logits, embed, att = model.inference([xt] * 3, 4, n, False, 0.0, 0.0, graphs, [8], [8, 1])
    x32 = x.astype(np.float32).astype(np.float64)
    embeds = []
    for p, g in enumerate(graphs):
        rp, ci = g.rowptr.cpu().numpy(), g.colidx.cpu().numpy()
        v = g.values.cpu().numpy().astype(np.float64)
        heads = [ho.sp_attn_head(x32, h, rp, ci, adj_vals=v)[0] for h in prob["params"]["heads"][p]]
        embeds.append(np.concatenate(heads, axis=1)[:, None, :])
    pr = prob["params"]
    final, alphas = ho.simple_att_layer(np.concatenate(embeds, axis=1), pr["w_omega"], pr["b_omega"], pr["u_omega"],
                                        return_alphas=True)
    want = sum(final @ c["W"] + c["b"] for c in pr["cls"]) / len(pr["cls"])
    for name, got, exp in (("embed", embed, final), ("att", att, alphas), ("logits", logits.reshape(n, -1), want)):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - exp).max())
        print(f"{name}: max abs error {err:.3e}")
        assert err < 1e-4, name


def test_trainer_on_pathsim_top_k_graphs(dev, dblp):
    from han_amd.trainer import HANTrainer
    rel, _, sizes = dblp
    graphs = [metapath.metapath_graph(rel, mp, weights="pathsim", top_k=32) for mp in MPS]
    model, x, gen = _model(sizes, dev)
    n = sizes["A"]
    labels = torch.randint(0, 4, (n,), generator=gen, device=dev, dtype=torch.int32)
    u = torch.rand(n, generator=gen, device=dev)
    tr = HANTrainer(model, [x] * 3, graphs, labels, (u < 0.2).to(torch.uint8), ((u >= 0.2) & (u < 0.3)).to(torch.uint8))
    for _ in range(3):
        tl, ta, vl, va = tr.epoch()
        assert np.isfinite(float(tl)) and np.isfinite(float(vl))
