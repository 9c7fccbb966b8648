"""han_node_attn_bwd_cols_scores: the backward gather that also takes the score-parameter gradients.

dH and df2 must be the BYTES of ops.node_attn_bwd_cols.  da1, da2, db1, db2 are compared with float64 sums of the same H
(as stored: keep bits included, not masked, not scaled), df1 and df2 taken on the host.  The bound is per element

    (roundings on the longest path of the kernel's summation tree) x 2^-24 x sum |terms|

with the path counted from the launch geometry (_depth): the product, the lane's chain over the rows it writes in its
grid-stride loop, the block's 16 lane groups, the fold of the slab (beyond 1024 slab rows) and han_reduce_slabs.

The graph: 1027 source rows against a 600-row table, row lengths cycling through 0 .. 20, so the lengths 0, 15, 16 and 17
(the short / wave-per-row bin boundary) occur; df1 is non-zero on every row, the empty ones included.  The gs table is
written through ops.gs_views: finite statistics records (f1, lse, s, z) and g rows, a quarter of the heads all zero
with z set (what HAN_FLAG_K2_ZERO_ROWS leaves out)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NS, NT = 1027, 600
U = 2.0 ** -24
HEADS = ((8, 8), (4, 16), (1, 64))
RATIOS = {}      # kernel form -> largest err / bound seen (printed by the last test)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _graph_t(dev, ns, nt, lengths):
    """Transposed graph: source row j lists lengths[j] destinations, (7 j + 13 e) % nt -- distinct within a row."""
    from han_amd.graph import CSRGraph
    lens = torch.tensor(lengths, dtype=torch.int64)
    rowptr = torch.zeros(ns + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(lens, 0)
    j = torch.repeat_interleave(torch.arange(ns), lens)
    e = torch.arange(int(rowptr[-1])) - rowptr[:-1][j]
    col = ((7 * j + 13 * e) % nt).to(torch.int32)
    return CSRGraph(rowptr.to(dev), col.to(dev), n_cols=nt)


_cache = {}


def _inputs(dev, ns, nt, K, FP, tdt, seed=0):
    """H, f2, df1, a1, a2 of the sources and the gs table of the destinations: made once per shape, never written."""
    key = (ns, nt, K, FP, tdt, seed)
    if key not in _cache:
        from han_amd import ops
        g = torch.Generator(device=dev).manual_seed(17 + 1000 * K + ns + seed)
        rnd = lambda *s: torch.randn(s, device=dev, generator=g)
        H = rnd(ns, 64).to(tdt)
        f2 = rnd(ns, K) * 0.5
        df1 = rnd(ns, K)
        df1 = torch.where(df1.abs() < 0.05, torch.full_like(df1, 0.25), df1)      # non-zero on every row
        a1, a2 = rnd(K, FP) * 0.3, rnd(K, FP) * 0.3
        gs = torch.zeros((nt, ops.gs_row_bytes(K, FP, tdt)), dtype=torch.uint8, device=dev)
        gv, st = ops.gs_views(gs, K, FP, tdt)
        gval = rnd(nt, K, FP)
        zero = torch.rand((nt, K), device=dev, generator=g) < 0.25
        gval[zero] = 0.0
        gv.copy_(gval.reshape(nt, 64).to(tdt))
        st[:, :, 0] = rnd(nt, K) * 0.5                        # f1
        st[:, :, 1] = 2.0 + torch.rand((nt, K), device=dev, generator=g)      # lse: alpha = exp(lrelu(f1 + f2) - lse) stays small
        st[:, :, 2] = rnd(nt, K) * 0.1                        # s
        st[:, :, 3] = zero.to(torch.float32)                  # z: non-zero bits = the head's g values are all zero
        _cache[key] = (H, f2, df1, a1, a2, gs)
    return _cache[key]


def _cleared(H):
    """H with EVERY keep bit (bit 0 of each stored element) cleared."""
    out = H.clone()
    _bits(out).bitwise_and_(-2)
    return out


def _depth(launches):
    """Roundings on the longest path from a term to its sum; launches = [(rows of the launch, rows per wave)]."""
    slab_rows = lane = 0
    for n_work, rpw in launches:
        units = -(-n_work // rpw)
        grid = min(max(-(-units // 4), 1), 8192)
        lane = max(lane, -(-units // (4 * grid)))      # one row per lane group and unit of its wave
        slab_rows += grid
    d = 1 + lane + 16                                   # product; the lane's chain; the block's 16 groups through LDS
    if slab_rows > 1024:
        d += -(-slab_rows // 256)                       # the fold: block j adds rows j, j + 256, ...
        slab_rows = 256
    return d + -(-slab_rows // 64) + 1 + 2 + 16         # han_reduce_slabs: an accumulator's chain, the four accumulators, 16 slices


def _launches(gt, binned):
    deg = (gt.rowptr[1:] - gt.rowptr[:-1]).cpu()
    if binned:
        n_short = int((deg < 16).sum())
        return [(n, r) for n, r in ((n_short, 4), (gt.n_rows - n_short, 1)) if n > 0]
    return [(gt.n_rows, 4 if gt.nnz < 12 * gt.n_rows else 1)]


def _check_scores(form, got, H, df1, df2, K, FP, depth):
    Hd = H.float().double().cpu().reshape(-1, K, FP)
    worst = 0.0
    for name, d, out in (("da1", df1, got[0]), ("da2", df2, got[1])):
        dd = d.double().cpu()
        ref = torch.einsum("jk,jkf->kf", dd, Hd)
        mag = torch.einsum("jk,jkf->kf", dd.abs(), Hd.abs())
        err, bound = (out.double().cpu() - ref).abs(), depth * U * mag
        assert bool((err <= bound).all()), f"{name}: err {float(err.max()):.3e} bound {float(bound.max()):.3e} ({form})"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    for name, d, out in (("db1", df1, got[2]), ("db2", df2, got[3])):
        dd = d.double().cpu()
        err, bound = (out.double().cpu() - dd.sum(0)).abs(), depth * U * dd.abs().sum(0)
        assert bool((err <= bound).all()), f"{name}: err {float(err.max()):.3e} bound {float(bound.max()):.3e} ({form})"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    RATIOS[form] = max(RATIOS.get(form, 0.0), worst)


def _run_case(dev, gt, K, FP, tdt, coef_drop, zero_rows, fts, binned, seed=0):
    from han_amd import ops
    H, f2, df1, a1, a2, gs = _inputs(dev, gt.n_rows, gt.n_cols, K, FP, tdt, seed)
    if fts == "cleared":
        H, fts_drop = _cleared(H), 0.6
    else:
        fts_drop = fts
    kw = dict(coef_drop=coef_drop, fts_drop=fts_drop, seed=11, zero_rows=zero_rows)
    rdH, rdf2 = ops.node_attn_bwd_cols(gt, gs, H, f2, df1, a1, a2, **kw)
    outs = [torch.full(s, 7.25, device=dev) for s in ((K, FP), (K, FP), (K,), (K,))]
    got = ops.node_attn_bwd_cols_scores(gt, gs, H, f2, df1, a1, a2, out=outs, **kw)
    assert got is not None, "eligible call declined"
    assert _same(got[0], rdH), "dH differs from node_attn_bwd_cols"
    assert _same(got[1], rdf2), "df2 differs from node_attn_bwd_cols"
    mode = 0 if (tdt == torch.bfloat16 or coef_drop == 0.0) else (3 if zero_rows else 1)
    form = f"{'binned' if binned else 'unbinned'} {K}x{FP} {'bf16' if tdt == torch.bfloat16 else 'f32'} mode{mode}"
    _check_scores(form, outs, H, df1, rdf2, K, FP, _depth(_launches(gt, binned)))
    if fts == "cleared":      # every projected row is dropped: a kernel that summed the DROPPED row would return zeros
        assert float(outs[0].abs().min()) > 0.0 and float(outs[1].abs().max()) > 0.0
    outs2 = [torch.full_like(o, -3.5) for o in outs]
    again = ops.node_attn_bwd_cols_scores(gt, gs, H, f2, df1, a1, a2, out=outs2, **kw)
    assert all(_same(a, b) for a, b in zip(outs + list(got), outs2 + list(again))), "a second call gives other bytes"


@pytest.mark.parametrize("fts", [0.0, 0.6, "cleared"], ids=["fts0", "fts06", "fts06_all_dropped"])
@pytest.mark.parametrize("coef_drop,zero_rows", [(0.0, False), (0.6, False), (0.6, True)], ids=["mode0", "mode1", "mode3"])
@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", HEADS)
@pytest.mark.parametrize("binned", [True, False], ids=["binned", "unbinned"])
def test_fused_gather_matches_the_two_calls(dev, monkeypatch, binned, K, FP, tdt, coef_drop, zero_rows, fts):
    from han_amd import ops
    monkeypatch.setattr(ops, "BINNED", binned)
    gt = _graph_t(dev, NS, NT, [j % 21 for j in range(NS)])
    assert set(_launches(gt, binned)) == ({(784, 4), (243, 1)} if binned else {(1027, 4)})
    _run_case(dev, gt, K, FP, tdt, coef_drop, zero_rows, fts, binned)


def test_grid_stride_more_rows_than_one_pass_covers(dev):
    """NS = 140 000 rows of two entries: 35 000 wave units on 8192 blocks x 4 waves, so lane groups write two rows, and
    8192 slab rows go through the fold."""
    ns = 140_000
    gt = _graph_t(dev, ns, NT, [2] * ns)
    assert _launches(gt, True) == [(ns, 4)] and ns > 8192 * 16
    _run_case(dev, gt, 8, 8, torch.float32, 0.6, False, 0.6, True)


def _patterned(dev, K, FP):
    return [torch.full(s, 7.25, device=dev) for s in ((K, FP), (K, FP), (K,), (K,))]


@pytest.mark.parametrize("route", ["lean", "masked", "long_row"])
def test_declined_routes_return_none_and_write_nothing(dev, monkeypatch, route):
    from han_amd import ops
    K, FP = 8, 8
    if route == "lean":      # a small table with long rows: node_attn_bwd_cols runs the one-lane-per-head kernel
        gt = _graph_t(dev, 64, 64, [64] * 64)
    elif route == "masked":
        full = _graph_t(dev, NS, NT, [j % 21 for j in range(NS)])
        gt = full.with_masked_columns(torch.arange(NT, device=dev) % 3 == 0)
        assert gt.masked
    else:                    # one row beyond the split length
        monkeypatch.setattr(ops, "SPLIT_DEG", 48)
        monkeypatch.setattr(ops, "SPLIT_CHUNK", 16)
        gt = _graph_t(dev, NS, NT, [60 if j == 500 else j % 21 for j in range(NS)])
    H, f2, df1, a1, a2, gs = _inputs(dev, gt.n_rows, gt.n_cols, K, FP, torch.float32, seed=1)
    if route == "lean":
        assert ops._use_lean(gt, H)
    outs = _patterned(dev, K, FP)
    assert ops.node_attn_bwd_cols_scores(gt, gs, H, f2, df1, a1, a2, coef_drop=0.6, fts_drop=0.6, seed=11, out=outs) is None
    torch.cuda.synchronize()
    assert all(bool((o == 7.25).all()) for o in outs)
    dH, df2 = ops.node_attn_bwd_cols(gt, gs, H, f2, df1, a1, a2, coef_drop=0.6, fts_drop=0.6, seed=11)      # the route the caller takes
    assert bool(torch.isfinite(dH).all()) and bool(torch.isfinite(df2).all())


# ------------------------------------------------------------------------------------------------ the training step
def _step(dev, fused, monkeypatch):
    """One trainer epoch from a fixed state -> (gradient of every parameter, what the score-gradient calls saw)."""
    from han_amd import ops, synth
    from han_amd import rng as hrng
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    n, P = 8192, 2
    wl = synth.planted_partition(n, 4, P, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=dev)
    u = torch.rand(n, generator=torch.Generator().manual_seed(1))
    masks = ((u < 0.1).to(torch.uint8).to(dev), ((u >= 0.1) & (u < 0.2)).to(torch.uint8).to(dev))
    torch.manual_seed(0)
    hrng.manual_seed(5)
    model = HeteGAT_multi().build(P, 64, 4, (8,), (8, 1), 128, device=dev, generator=torch.Generator().manual_seed(11))
    assert model.fused_scores == "auto"
    model.fused_scores = fused
    seen = []
    # which meta-path a call works for: its da1 is a slice of the model's a1 gradient (the trainer's direct gradients)
    path_of = lambda out: (out[0].data_ptr() - model._views["a1"].grad.data_ptr()) // (64 * 4)
    fused_call, pair_call = ops.node_attn_bwd_cols_scores, ops.score_param_bwd

    def spy_fused(graph_t, *a, **kw):
        got = fused_call(graph_t, *a, **kw)
        seen.append(("fused", path_of(kw["out"]), graph_t, got is not None))
        return got

    def spy_pair(H, df1, df2, **kw):
        seen.append(("pair", path_of(kw["out"]), H.clone(), df1.clone(), df2.clone()))
        return pair_call(H, df1, df2, **kw)

    monkeypatch.setattr(ops, "node_attn_bwd_cols_scores", spy_fused)
    monkeypatch.setattr(ops, "score_param_bwd", spy_pair)
    tr = HANTrainer(model, [wl["x"]] * P, wl["graphs"], wl["labels"], masks[0], masks[1], use_graph=False)
    tr.epoch()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "node_attn_bwd_cols_scores", fused_call)
    monkeypatch.setattr(ops, "score_param_bwd", pair_call)
    return {k: v.grad.clone() for k, v in model._views.items()}, seen


def test_training_step_with_and_without_the_fused_scores(dev, monkeypatch):
    from han_amd import ops
    g_on, seen_on = _step(dev, "auto", monkeypatch)
    g_off, seen_off = _step(dev, False, monkeypatch)
    assert sorted(s[:2] for s in seen_on) == [("fused", 0), ("fused", 1)] and all(s[3] for s in seen_on), "auto: the fused call, taken"
    assert sorted(s[:2] for s in seen_off) == [("pair", 0), ("pair", 1)]
    scores = ("a1", "a2", "b1", "b2")
    for k in g_off:
        if k not in scores:
            assert _same(g_on[k], g_off[k]), f"d{k} differs"
    # the four score gradients: both runs round the same sums, each within its own tree's bound of the exact value
    for p in range(2):
        H, df1, df2 = [s for s in seen_off if s[1] == p][0][2:]
        gt = [s for s in seen_on if s[1] == p][0][2]
        rb = gt.row_bins(ops.SHORT_DEG, ops.SPLIT_DEG)
        d_on = _depth([(n, r) for n, r in ((rb["n_short"], 4), (rb["n_mid"], 1)) if n > 0])
        n = H.shape[0]
        grid = min(-(-n // 16), 1024)
        d_off = 1 + -(-n // (16 * grid)) + 16 + -(-grid // 64) + 1 + 2 + 16      # score_param_bwd_kernel and its reduction
        Hd = H.double().cpu().reshape(n, 8, 8)
        for name, d in (("a1", df1), ("a2", df2)):
            mag = torch.einsum("jk,jkf->kf", d.double().cpu().abs(), Hd.abs())
            err = (g_on[name][p].double() - g_off[name][p].double()).abs().cpu()
            assert bool((err <= (d_on + d_off) * U * mag).all()), f"d{name}[{p}]: {float(err.max()):.3e}"
        for name, d in (("b1", df1), ("b2", df2)):
            mag = d.double().cpu().abs().sum(0)
            err = (g_on[name][p].double() - g_off[name][p].double()).abs().cpu()
            assert bool((err <= (d_on + d_off) * U * mag).all()), f"d{name}[{p}]: {float(err.max()):.3e}"


def test_report_largest_ratio_per_form():
    """Not a check: prints the largest err / bound ratio of every kernel form the cases above reached (run with -s)."""
    for form in sorted(RATIOS):
        print(f"err/bound {form}: {RATIOS[form]:.4f}")
