"""Sampled meta-path neighbours on the GPU (K0: han_metapath_walk_count / _fill): graph and visit counts bit for bit
the NumPy restatement of tests/metapath_walk_ref.py, on chains of 60-300 rows built to reach every place where the
kernel can go wrong (the x / y word of odd chain lengths, walk counts around the wave and the sort sizes, the fanout
cut with ties across the threshold, dead ends at every hop, a hub row, parallel and unsorted entries, the diagonal
visited or not, degenerate inputs, the widest column space); row ranges, reproducibility, the stored values; the
DBLP-like relations against the exact product; and the model on sampled graphs."""
import numpy as np
import pytest
import torch

from han_amd import metapath, ops, synth
from han_amd.graph import CSRGraph
from tests import metapath_walk_ref as ref

pytestmark = pytest.mark.gpu


def _csr(rows):
    rowptr = np.zeros(len(rows) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    colidx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rowptr[-1] else np.zeros(0, np.int32)
    return rowptr, colidx


def _dev_hops(hops, sizes, dev):
    """CSRGraphs of host (rowptr, colidx) pairs taken AS GIVEN (unsorted, repeats kept)."""
    return [CSRGraph(torch.as_tensor(rp).to(dev), torch.as_tensor(ci).to(dev), n, validate=False)
            for (rp, ci), n in zip(hops, sizes[1:])]


def _host(g: CSRGraph):
    return g.rowptr.cpu().numpy(), g.colidx.cpu().numpy()


def _chain(seed, sizes, empty=0.1, most=6):
    """A random chain over the node counts `sizes`: about `empty` of the rows of every hop have no entry (dead ends at
    the first, the middle and the last hop), the others 1 .. most entries with repeats, in no order."""
    rng = np.random.default_rng(seed)
    hops = []
    for n_rows, n_cols in zip(sizes, sizes[1:]):
        deg = np.where(rng.random(n_rows) < empty, 0, rng.integers(1, most + 1, n_rows))
        hops.append(_csr([rng.integers(0, n_cols, d) for d in deg]))
    return hops


def _assert_walk(dev, hops, sizes, walks, fanout, seed=0, diag=False, rows=None, graphs=None, ends=None):
    graphs = _dev_hops(hops, sizes, dev) if graphs is None else graphs
    g, visits = ops.metapath_walk(graphs, walks, fanout, seed=seed, diag=diag, rows=rows)
    rowptr, colidx, want = ref.sample(hops, walks, fanout, seed=seed, diag=diag, rows=rows, ends=ends)
    r0, r1 = (0, sizes[0]) if rows is None else rows
    assert g.values is None and (g.n_rows, g.n_cols, g.row_base) == (r1 - r0, sizes[-1], r0)
    assert visits.dtype == torch.int32 and visits.shape == (g.nnz,) and g.colidx.dtype == torch.int32
    what = f"walks {walks} fanout {fanout} seed {seed} diag {diag} rows {rows}"
    np.testing.assert_array_equal(g.rowptr.cpu().numpy(), rowptr, err_msg=what)
    np.testing.assert_array_equal(g.colidx.cpu().numpy(), colidx, err_msg=what)
    np.testing.assert_array_equal(visits.cpu().numpy(), want, err_msg=what)
    return g, visits


SIZES = {1: [96, 96], 2: [96, 40, 96], 3: [96, 150, 7, 96], 4: [96, 150, 5, 150, 96],
         8: [96, 30, 96, 12, 70, 9, 50, 20, 96]}


@pytest.mark.parametrize("walks", [1, 63, 64, 65, 1000, 4096])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 8])
def test_random_chains_match_the_restatement(dev, L, walks):
    sizes = SIZES[L]
    hops = _chain(10 * L + 1, sizes)
    assert any((np.diff(rp) == 0).any() for rp, _ in hops)
    graphs = _dev_hops(hops, sizes, dev)
    ends = ref.endpoints(hops, walks, walks + L)
    for fanout in sorted({1, min(5, walks), walks}):
        for diag in (False, True):
            _assert_walk(dev, hops, sizes, walks, fanout, seed=walks + L, diag=diag, graphs=graphs, ends=ends)


def test_rectangular_chain_without_self_loops(dev):
    sizes = [130, 200, 9]                                                     # APC
    hops = _chain(3, sizes)
    for walks, fanout in ((64, 3), (300, 9), (300, 2)):
        g, _ = _assert_walk(dev, hops, sizes, walks, fanout, seed=5)
    assert g.n_cols == 9 and g.n_rows == 130
    with pytest.raises(ValueError, match="square"):
        ops.metapath_walk(_dev_hops(hops, sizes, dev), 8, diag=True)


def test_hub_row_ties_across_the_threshold(dev):
    """Every start node leads to one of three venues; venue 0 holds 5000 entries over 6000 columns (degree >> walks:
    most end points are visited once, so the cut runs through a long run of equal counts), venue 1 two, venue 2
    none."""
    rng = np.random.default_rng(8)
    first = [[0]] * 50 + [[1]] * 4 + [[2]] * 3 + [[0, 1, 0, 0]] * 3 + [[0, 2]] * 3 + [[]]
    hub = [rng.integers(0, 6000, 5000), [5999, 0], []]
    hops, sizes = [_csr(first), _csr(hub)], [len(first), 3, 6000]
    graphs = _dev_hops(hops, sizes, dev)
    for walks, fanout in ((256, 32), (256, 1), (4096, 5), (1000, 999), (65, 65)):
        g, visits = _assert_walk(dev, hops, sizes, walks, fanout, seed=2, graphs=graphs)
    g, visits = ops.metapath_walk(graphs, 256, 32, seed=2)
    deg, v = g.degrees().cpu().numpy(), visits.cpu().numpy()
    assert deg[0] == 32 and deg[50] == 2 and deg[54] == 0 and deg[-1] == 0
    assert (v[:32] == 1).sum() > 8                                            # the cut really runs through ties


def test_every_walk_ends_in_one_node(dev):
    n = 70
    hops, sizes = [_csr([[7]] * n), _csr([[3, 3]] * n), _csr([[7]] * n)], [n, n, n, n]
    for walks in (1, 65, 4096):
        for diag in (False, True):
            g, visits = _assert_walk(dev, hops, sizes, walks, 1, seed=1, diag=diag)
    # (diag, walks 4096) row 7 is (7, 7) alone with every walk; any other row holds (i, i) with 0 and (i, 7)
    assert g.nnz == 2 * n - 1 and int(visits.max()) == 4096 and int((visits == 0).sum()) == n - 1
    s = int(g.rowptr[7])
    assert g.colidx[s].item() == 7 and visits[s].item() == 4096 and int(g.rowptr[8]) == s + 1


def test_diagonal_dead_rows_and_the_last_row(dev):
    # row 0 never reaches itself; row 1 may; row 2 only reaches itself; row 3: every walk dies at the second hop;
    # row 4 has no entry; the last row is an ordinary one
    a = [[1], [0, 1, 2, 1], [2, 2], [4], [], [5, 0, 3]]
    b = [[1, 2], [1, 0], [2], [3, 5, 5], [], [5, 4, 0]]
    hops, sizes = [_csr(a), _csr(b)], [6, 6, 6]
    for walks, fanout in ((64, 1), (64, 64), (200, 2), (1, 1)):
        for diag in (False, True):
            g, visits = _assert_walk(dev, hops, sizes, walks, fanout, seed=4, diag=diag)
    rp = g.rowptr.tolist()                                                    # (walks 1, diag): a row of (i, i) + one
    assert rp[4] - rp[3] == 1 and rp[5] - rp[4] == 1 and g.colidx[rp[3]].item() == 3 and visits[rp[3]].item() == 0
    g, visits = ops.metapath_walk(_dev_hops(hops, sizes, dev), 64, 1, seed=4)
    rp = g.rowptr.tolist()
    assert rp[4] == rp[3] and rp[5] == rp[4] and rp[6] - rp[5] == 1           # dead rows are empty without diag


def test_zero_rows_and_an_empty_relation(dev):
    hops, sizes = _chain(2, [60, 30, 60]), [60, 30, 60]
    graphs = _dev_hops(hops, sizes, dev)
    g, visits = ops.metapath_walk(graphs, 64, 4, rows=(17, 17))
    assert g.n_rows == 0 and g.nnz == 0 and g.rowptr.tolist() == [0] and visits.numel() == 0 and g.row_base == 17
    none = CSRGraph(torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 30)
    g, visits = ops.metapath_walk([none, graphs[1]], 64, 4)
    assert g.n_rows == 0 and g.n_cols == 60 and visits.numel() == 0
    empty = (np.zeros(31, dtype=np.int64), np.zeros(0, np.int32))             # a relation without entries: all die
    for diag in (False, True):
        g, visits = _assert_walk(dev, [hops[0], empty], sizes, 100, 5, diag=diag)
        assert g.nnz == (60 if diag else 0) and int(visits.sum()) == 0
    _assert_walk(dev, [(np.zeros(61, dtype=np.int64), np.zeros(0, np.int32)), hops[1]], sizes, 100, 5, diag=True)


def test_widest_column_space(dev):
    """A last hop of 2^31 - 1 columns with entries in column 2^31 - 2: a dead walk must sort above it."""
    top = 2 ** 31 - 2
    first = [[0], [1], [2], [3, 0, 3], [1, 2]] * 12
    last = [[top, 5, top], [0, top - 1], [], [top]]
    hops, sizes = [_csr(first), _csr(last)], [60, 4, top + 1]
    for walks, fanout in ((64, 64), (100, 1), (63, 2)):
        g, visits = _assert_walk(dev, hops, sizes, walks, fanout, seed=6)
    assert int(g.colidx.max()) == top and g.n_cols == 2 ** 31 - 1
    assert int(g.rowptr[3]) == int(g.rowptr[2])                               # rows 2, 7, ...: every walk died


def test_row_ranges_repeats_and_seeds(dev):
    sizes = [300, 120, 11, 120, 300]
    hops = _chain(9, sizes)
    graphs = _dev_hops(hops, sizes, dev)
    whole, vw = _assert_walk(dev, hops, sizes, 256, 8, seed=77, diag=True, graphs=graphs)
    a, va = _assert_walk(dev, hops, sizes, 256, 8, seed=77, diag=True, rows=(0, 131), graphs=graphs)
    b, vb = _assert_walk(dev, hops, sizes, 256, 8, seed=77, diag=True, rows=(131, 300), graphs=graphs)
    assert torch.equal(torch.cat([a.rowptr, a.rowptr[-1] + b.rowptr[1:]]), whole.rowptr)
    assert torch.equal(torch.cat([a.colidx, b.colidx]), whole.colidx) and torch.equal(torch.cat([va, vb]), vw)
    again, v2 = ops.metapath_walk(graphs, 256, 8, seed=77, diag=True)
    assert torch.equal(again.rowptr, whole.rowptr) and torch.equal(again.colidx, whole.colidx) and torch.equal(v2, vw)
    other, v3 = ops.metapath_walk(graphs, 256, 8, seed=78, diag=True)
    assert not (other.nnz == whole.nnz and torch.equal(other.colidx, whole.colidx) and torch.equal(v3, vw))
    big, v4 = _assert_walk(dev, hops, sizes, 256, 8, seed=(1 << 64) - 3, diag=True, rows=(290, 300), graphs=graphs)
    assert big.row_base == 290


def _small_relations(dev, n_a=300, n_p=500, n_c=6, seed=13):
    rng = np.random.default_rng(seed)
    n_auth = rng.integers(1, 4, n_p)
    pid = np.repeat(np.arange(n_p), n_auth)
    aid = rng.integers(0, n_a - 10, pid.size)                                 # the last ten authors have no paper
    return {"AP": metapath.relation(aid, pid, n_a, n_p, device=dev),
            "PC": metapath.relation(np.arange(n_p), rng.integers(0, n_c, n_p), n_p, n_c, device=dev)}


def _plan_hops(rel, mp):
    return [rel[k].transpose() if t else rel[k] for k, t in metapath.plan(rel, mp)["hops"]]


def test_sample_values_are_exact(dev):
    rel = _small_relations(dev)
    for mp, loops, rows in (("APCPA", True, None), ("APA", True, (100, 300)), ("APC", False, None)):
        hops = [_host(g) for g in _plan_hops(rel, mp)]
        for walks, fanout in ((256, 32), (100, None)):
            rp, ci, visits = ref.sample(hops, walks, fanout, seed=9, diag=loops, rows=rows)
            for weights in (None, "count", "prob"):
                g = metapath.metapath_sample(rel, mp, walks=walks, fanout=fanout, seed=9, self_loops=loops,
                                             weights=weights, rows=rows)
                np.testing.assert_array_equal(g.rowptr.cpu().numpy(), rp)
                np.testing.assert_array_equal(g.colidx.cpu().numpy(), ci)
                assert g.row_base == (rows[0] if rows else 0)
                if weights is None:
                    assert g.values is None
                    continue
                got = g.values.cpu().numpy()
                assert got.dtype == np.float32
                np.testing.assert_array_equal(got.view(np.uint32), ref.values(visits, walks, weights).view(np.uint32))
                assert got.min() >= 0.0 and (weights == "count" or got.max() <= 1.0)
    deg = g.degrees()
    assert int(deg.max()) <= 6 and int(deg[-10:].sum()) == 0                  # (APC) authors without papers: empty


@pytest.fixture(scope="module")
def dblp():
    dev = torch.device("cuda:0")
    return synth.hetero_relations("dblp-like", device=dev)


@pytest.mark.parametrize("mp", ["APCPA", "APTPA"])
def test_dblp_like_samples_lie_in_the_product(dev, dblp, mp):
    rel, sizes = dblp
    n = sizes["A"]
    g = metapath.metapath_sample(rel, mp, walks=256, fanout=32, seed=1, weights="count")
    full = metapath.metapath_graph(rel, mp)
    rows = lambda x: torch.repeat_interleave(torch.arange(n, device=dev), x.degrees())
    key_full = rows(full) * n + full.colidx.long()                            # ascending: sorted rows, sorted columns
    key = rows(g) * n + g.colidx.long()
    at = torch.searchsorted(key_full, key).clamp_(max=key_full.numel() - 1)
    assert bool((key_full[at] == key).all())                                  # (the diagonal is in both)
    assert bool((key[1:] > key[:-1]).all())                                   # columns strictly ascending
    deg = g.degrees()
    assert int(deg.max()) == 33 and int(deg.min()) >= 1
    per_row = torch.zeros(n, device=dev).index_add_(0, rows(g), g.values)
    assert float(per_row.max()) <= 256.0
    on_diag = g.colidx.long() == rows(g)
    assert int(on_diag.sum()) == n
    rp, ci, visits = ref.sample([_host(h) for h in _plan_hops(rel, mp)], 256, 32, seed=1, diag=True)
    np.testing.assert_array_equal(g.rowptr.cpu().numpy(), rp)
    np.testing.assert_array_equal(g.colidx.cpu().numpy(), ci)
    np.testing.assert_array_equal(g.values.cpu().numpy(), visits.astype(np.float32))


def test_forward_on_sampled_graphs_matches_the_float64_oracle(dev):
    """One forward on a sampled boolean graph (APA) and a sampled "prob" graph (APCPA) of 300 authors against the
    float64 oracle fed the same structure and stored values: the 1e-4 bar of the parity tests."""
    from oracle import han_oracle as ho
    from tests.helpers import build_model
    rel = _small_relations(dev)
    n = 300
    graphs = [metapath.metapath_sample(rel, "APA", walks=64, fanout=8, seed=3),
              metapath.metapath_sample(rel, "APCPA", walks=256, fanout=32, seed=3, weights="prob")]
    assert graphs[0].values is None and graphs[1].values is not None
    rng = np.random.default_rng(22)
    prob = dict(params=ho.init_params(rng, 2, 64, 4), p=2, f=64, c=4)
    x = rng.standard_normal((1, n, 64))
    model, _ = build_model(prob, dev)
    xt = torch.tensor(x[0], dtype=torch.float32, device=dev)
    with torch.no_grad():
        logits, embed, att = model.inference([xt] * 2, 4, n, False, 0.0, 0.0, graphs, [8], [8, 1])
    x32 = x.astype(np.float32).astype(np.float64)
    embeds = []
    for p, g in enumerate(graphs):
        rp, ci = _host(g)
        v = None if g.values is None else g.values.cpu().numpy().astype(np.float64)
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


def test_trainer_on_sampled_graphs(dev):
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    rel = _small_relations(dev)
    n = 300
    graphs = [metapath.metapath_sample(rel, "APA", walks=64, fanout=8),
              metapath.metapath_sample(rel, "APCPA", weights="prob")]
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(n, 64, generator=gen, device=dev)
    model = HeteGAT_multi().build(2, 64, 4, device=dev, generator=torch.Generator().manual_seed(5))
    labels = torch.randint(0, 4, (n,), generator=gen, device=dev, dtype=torch.int32)
    u = torch.rand(n, generator=gen, device=dev)
    tr = HANTrainer(model, [x] * 2, graphs, labels, (u < 0.2).to(torch.uint8), ((u >= 0.2) & (u < 0.3)).to(torch.uint8))
    for _ in range(2):
        tl, ta, vl, va = tr.epoch()
        assert np.isfinite(float(tl)) and np.isfinite(float(vl))
