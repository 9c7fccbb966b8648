"""K0 on the GPU: the boolean sparse-sparse product (han_spgemm_*) and the meta-path builder, all by exact integer
equality against scipy's (A @ B) != 0 with sorted indices: both row bins and their boundary, the bit-map tiles,
the diagonal flag, degenerate inputs; APA / APCPA / APTPA on the DBLP-like relations (palindromic form, full chain
and scipy agree); PAP at 3 M papers; and the model on builder graphs."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from han_amd import metapath, ops, synth
from han_amd.graph import CSRGraph

pytestmark = pytest.mark.gpu


def _sp(g: CSRGraph):
    return sp.csr_matrix((np.ones(g.nnz, dtype=bool), g.colidx.cpu().numpy(), g.rowptr.cpu().numpy()),
                         shape=(g.n_rows, g.n_cols))


def _canon(m, diag=False):
    m = sp.csr_matrix(m, dtype=bool)
    if diag:
        m = sp.csr_matrix(m + sp.identity(m.shape[0], dtype=bool, format="csr"))
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


def _assert_same(g: CSRGraph, ref):
    assert g.values is None and (g.n_rows, g.n_cols) == ref.shape
    np.testing.assert_array_equal(g.rowptr.cpu().numpy(), ref.indptr.astype(np.int64))
    np.testing.assert_array_equal(g.colidx.cpu().numpy(), ref.indices.astype(np.int32))


def _graph(rows, n_cols, dev):
    """CSRGraph of per-row column lists taken AS GIVEN (unsorted, repeats kept)."""
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rowptr[-1] else np.zeros(0, np.int32)
    return CSRGraph.from_arrays(rowptr, colidx, n_cols, device=dev)


def _pair(seed, n_rows, n_mid, n_cols, S, dev, n_random=300):
    """A (n_rows x n_mid) and B (n_mid x n_cols) whose rows hit the bins' boundaries: B rows of 0, 1, S - 1, S, S + 1
    and 5 S candidates (with repeats), A rows with bounds 0 (empty, and non-empty over empty B rows), S - 1, S, S + 1,
    long, and random unsorted rows with repeated entries; the other A rows are empty."""
    rng = np.random.default_rng(seed)
    deg = {0: 0, 1: 1, 2: S - 1, 3: S, 4: S + 1, 5: 5 * S}
    b_rows = []
    for l in range(n_mid):
        d = deg.get(l, int(rng.integers(0, 40)))
        b_rows.append(rng.integers(0, n_cols, d))                  # repeats within the row, no order
    a_rows = [[] for _ in range(n_rows)]
    a_rows[1] = [0, 0]                                             # non-empty, bound 0
    a_rows[2], a_rows[3], a_rows[4], a_rows[5] = [2], [3], [4], [1, 3]   # S - 1, S, S + 1, S + 1
    a_rows[6] = [5, 2, 5]                                          # long, a repeated entry
    a_rows[n_rows - 1] = [1, 2]                                    # S: the last row
    for i in rng.choice(np.arange(7, n_rows - 1), size=min(n_random, n_rows - 8), replace=False):
        a_rows[i] = rng.integers(0, n_mid, int(rng.integers(1, 30)))
    return _graph(a_rows, n_mid, dev), _graph(b_rows, n_cols, dev)


@pytest.mark.parametrize("S,tile", [(None, None), (64, 64), (4096, 1 << 19)])
@pytest.mark.parametrize("shape", ["rect", "square_diag", "wide"])
def test_bool_matmul_matches_scipy(dev, monkeypatch, S, tile, shape):
    if S is not None:
        monkeypatch.setattr(ops, "SPGEMM_SHORT", S)
        monkeypatch.setattr(ops, "SPGEMM_TILE", tile)
    S, T = ops.SPGEMM_SHORT, ops.SPGEMM_TILE
    n_rows, n_mid, n_cols, diag = {"rect": (400, 60, 700, False), "square_diag": (900, 60, 900, True),
                                   "wide": (300, 40, 2 * T + 77, False)}[shape]    # wide: three bit-map tiles
    A, B = _pair(7, n_rows, n_mid, n_cols, S, dev)
    C = ops.csr_bool_matmul(A, B, diag=diag)
    ref = _canon(_sp(A) @ _sp(B), diag)
    _assert_same(C, ref)
    again = ops.csr_bool_matmul(A, B, diag=diag)
    assert torch.equal(C.rowptr, again.rowptr) and torch.equal(C.colidx, again.colidx)


def test_bool_matmul_degenerate_inputs(dev):
    e = lambda r, c: CSRGraph(torch.zeros(r + 1, dtype=torch.int64, device=dev),
                              torch.zeros(0, dtype=torch.int32, device=dev), c)
    B = _graph([[0, 3], [], [2, 2, 1]], 4, dev)
    C = ops.csr_bool_matmul(e(5, 3), B)                            # empty A
    assert C.nnz == 0 and C.rowptr.tolist() == [0] * 6 and C.n_cols == 4
    C = ops.csr_bool_matmul(e(4, 3), B, diag=True)                 # empty A, square: the diagonal alone
    _assert_same(C, _canon(sp.csr_matrix((4, 4), dtype=bool), True))
    A = _graph([[1], [0, 2], []], 3, dev)
    _assert_same(ops.csr_bool_matmul(A, e(3, 6)), _canon(sp.csr_matrix((3, 6), dtype=bool)))   # empty B
    C = ops.csr_bool_matmul(e(0, 3), B)                            # no rows
    assert C.n_rows == 0 and C.rowptr.tolist() == [0]
    with pytest.raises(ValueError, match="columns"):
        ops.csr_bool_matmul(A, e(4, 2))
    with pytest.raises(ValueError, match="square"):
        ops.csr_bool_matmul(A, B, diag=True)


def test_two_pass_builders_without_entries(dev):
    """The count / scan / fill builders (csr.two_pass) on results without entries: no fill launch, empty arrays of the
    dtypes a full result has, an all-zero row pointer."""
    def check(g, n_rows, n_cols, *more):
        assert (g.n_rows, g.n_cols, g.nnz) == (n_rows, n_cols, 0)
        assert g.rowptr.dtype == torch.int64 and g.rowptr.tolist() == [0] * (n_rows + 1)
        assert g.colidx.dtype == torch.int32 and g.colidx.shape == (0,)
        for t, dtype in more:
            assert t.dtype == dtype and t.shape == (0,) and t.device == g.device
        assert g.rowptr.device == g.colidx.device == torch.device(dev)

    g = CSRGraph.from_bias(torch.full((4, 4), -1e9, device=dev))
    check(g, 4, 4)
    assert g.values is None
    A = CSRGraph(torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 2)
    B = _graph([[0, 3], [1]], 4, dev)
    C = ops.csr_bool_matmul(A, B)
    check(C, 3, 4)
    assert C.values is None
    C, counts = ops.csr_count_matmul(A, B)
    check(C, 3, 4, (counts, torch.int64))
    V = CSRGraph(torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 3,
                 values=torch.zeros(0, dtype=torch.float32, device=dev))
    T = ops.csr_row_topk(V, 2)
    check(T, 3, 3, (T.values, torch.float32))
    hop = CSRGraph(torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 3)
    g, visits = ops.metapath_walk([hop], 8, 2)
    check(g, 3, 3, (visits, torch.int32))
    g, visits = ops.metapath_walk([hop], 8, 2, diag=True)          # the lone (i, i), never visited
    assert g.rowptr.tolist() == [0, 1, 2, 3] and g.colidx.tolist() == [0, 1, 2] and g.colidx.dtype == torch.int32
    assert visits.dtype == torch.int32 and visits.tolist() == [0, 0, 0]


@pytest.fixture(scope="module")
def dblp():
    dev = torch.device("cuda:0")
    rel, sizes = synth.hetero_relations("dblp-like", device=dev)
    return rel, {k: _sp(g) for k, g in rel.items()}, sizes


def _scipy_chain(host, plan, diag):
    m = None
    for key, t in plan["hops"]:
        r = sp.csr_matrix(host[key].T) if t else host[key]
        m = r if m is None else sp.csr_matrix(m @ r)
    return _canon(m, diag)


@pytest.mark.parametrize("mp", ["APA", "APCPA", "APTPA"])
def test_dblp_like_palindromes(dev, dblp, mp):
    rel, host, sizes = dblp
    p = metapath.plan(rel, mp)
    assert p["split"] == len(mp) // 2
    g = metapath.metapath_graph(rel, mp)
    hops = [rel[k].transpose() if t else rel[k] for k, t in p["hops"]]
    full = metapath.compose(hops, self_loops=True)
    ref = _scipy_chain(host, p, diag=True)
    _assert_same(g, ref)
    _assert_same(full, ref)
    again = metapath.metapath_graph(rel, mp)
    assert torch.equal(g.rowptr, again.rowptr) and torch.equal(g.colidx, again.colidx)
    assert g.n_rows == g.n_cols == sizes["A"]


@pytest.mark.parametrize("mp,loops", [("APC", False), ("APT", False), ("CPAPC", True), ("PAP", True), ("CP", False)])
def test_dblp_like_left_to_right_paths(dev, dblp, mp, loops):
    rel, host, _ = dblp
    p = metapath.plan(rel, mp)
    assert p["split"] is None
    _assert_same(metapath.metapath_graph(rel, mp, self_loops=loops), _scipy_chain(host, p, loops))


def test_pap_3m_full_size(dev):
    rel, sizes = synth.hetero_relations("pap-3m", device=dev)
    pa = rel["PA"]
    n, n_a = sizes["P"], sizes["A"]
    assert metapath.plan(rel, "PAP")["split"] == 1
    g = metapath.metapath_graph(rel, "PAP")
    rp, ci = g.rowptr, g.colidx
    assert g.n_rows == g.n_cols == n
    assert 2e8 < g.nnz < 4e8, g.nnz
    # global invariants, on the device
    assert int(rp[0]) == 0 and int(rp[-1]) == g.nnz and bool((rp[1:] >= rp[:-1]).all())
    assert int(ci.min()) >= 0 and int(ci.max()) < n
    inc = ci[1:] > ci[:-1]
    starts = rp[1:-1]
    inc[starts[(starts > 0) & (starts < g.nnz)] - 1] = True        # a new row may start lower
    assert bool(inc.all())
    del inc
    row_of = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), g.degrees())
    assert int((ci == row_of).sum()) == n                          # every row holds its diagonal (once)
    del row_of
    # sampled rows against a NumPy union of the papers of the row's authors
    pa_rp, pa_ci = pa.rowptr.cpu().numpy(), pa.colidx.cpu().numpy()
    ap = sp.csr_matrix((np.ones(pa.nnz, dtype=bool), pa_ci, pa_rp), shape=(n, n_a)).T.tocsr()
    rp_h = rp.cpu().numpy()
    longest = int(torch.argmax(g.degrees()))
    rng = np.random.default_rng(3)
    sample = sorted({0, n - 1, longest} | set(rng.integers(0, n, 61).tolist()))
    assert rp_h[longest + 1] - rp_h[longest] > ops.SPGEMM_SHORT     # the bit-map bin is sampled too
    for p in sample:
        authors = pa_ci[pa_rp[p]:pa_rp[p + 1]]
        ref = np.unique(np.concatenate([ap.indices[ap.indptr[a]:ap.indptr[a + 1]] for a in authors] + [[p]]))
        np.testing.assert_array_equal(ci[rp_h[p]:rp_h[p + 1]].cpu().numpy(), ref.astype(np.int32), err_msg=f"row {p}")


MPS = ("APA", "APCPA", "APTPA")


def _model(sizes, dev):
    from han_amd.gat import HeteGAT_multi
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(sizes["A"], 64, generator=gen, device=dev)
    model = HeteGAT_multi().build(len(MPS), 64, 4, device=dev, generator=torch.Generator().manual_seed(5))
    return model, x, gen


def test_inference_on_builder_graphs_is_bitwise_the_scipy_graphs(dev, dblp):
    from han_amd import process
    rel, host, sizes = dblp
    built = [metapath.metapath_graph(rel, mp) for mp in MPS]
    ref = [process.adj_to_graph(_scipy_chain(host, metapath.plan(rel, mp), diag=False), device=dev) for mp in MPS]
    model, x, _ = _model(sizes, dev)
    with torch.no_grad():
        la, ea, aa = model.inference([x] * 3, 4, sizes["A"], False, 0.0, 0.0, built, [8], [8, 1])
        lb, eb, ab = model.inference([x] * 3, 4, sizes["A"], False, 0.0, 0.0, ref, [8], [8, 1])
    assert torch.equal(la, lb) and torch.equal(ea, eb) and torch.equal(aa, ab)


def test_trainer_on_builder_graphs(dev, dblp):
    from han_amd.trainer import HANTrainer
    rel, _, sizes = dblp
    graphs = [metapath.metapath_graph(rel, mp) for mp in MPS]
    model, x, gen = _model(sizes, dev)
    n = sizes["A"]
    labels = torch.randint(0, 4, (n,), generator=gen, device=dev, dtype=torch.int32)
    u = torch.rand(n, generator=gen, device=dev)
    tr = HANTrainer(model, [x] * 3, graphs, labels, (u < 0.2).to(torch.uint8), ((u >= 0.2) & (u < 0.3)).to(torch.uint8))
    for _ in range(3):
        tl, ta, vl, va = tr.epoch()
        assert np.isfinite(float(tl)) and np.isfinite(float(vl))
