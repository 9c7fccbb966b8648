"""The backward over the rows the loss reaches: ops.sem_attn_bwd_rows(live=...) (han_sem_attn_bwd_rows_live) against the
full entry on inputs whose dead dZ rows are zero, the backward gather on CSRGraph.with_live_columns against the gather
on the full transposed graph, and HANTrainer(live_backward=True) against live_backward=False."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sem_attn_ref as sr
from tests.test_k3_fold_gpu import _dc_depth, _inputs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# N * P >= 65 536 (the full entry is the reference) and N * P no multiple of 16: n_live = N leaves a partial last tile
# and a last pass with one tile; n_live = 1, 5, N / 10 give fewer tiles than waves, so every pass's second tile lies
# past the end, and (n_live * P mod 16 != 0) a partial last tile as well
FOLD_N = {4: 16387, 2: 32771, 1: 65541}
N_LIVE = ["1", "5", "N/10", "N"]
PATTERN = 0xA5


def _live_ids(N, which, seed):
    k = {"1": 1, "5": 5, "N/10": N // 10, "N": N}[which]
    ids = np.sort(np.random.default_rng(seed).permutation(N)[:k])
    if which == "5":
        ids[0], ids[-1] = 0, N - 1          # the first and the last row of the tables
    return np.unique(ids)


def _run_fold(ops, t, P, N, dev, code, live=None, fill=None):
    rb = ops.gs_row_bytes(8, 8)
    if fill is None:
        gs_buf = df_buf = None
    else:
        gs_buf = [torch.full((N, rb), fill, dtype=torch.uint8, device=dev) for _ in range(P)]
        df_buf = [torch.full((N, 32), fill, dtype=torch.uint8, device=dev).view(torch.float32) for _ in range(P)]
    dc = torch.full((P, 64), float("nan"), device=dev)
    r = ops.sem_attn_bwd_rows(t["M"], t["w"], t["b"], t["u"], t["beta"], t["dZ"],
                              [(t["aggp"][p], t["tsum"][p], t["f1"][p], t["lse"][p]) for p in range(P)], t["c"], dc,
                              activation=code, gs_out=gs_buf, df1_out=df_buf, live=live)
    assert r is not None, "the library refused an eligible shape"
    torch.cuda.synchronize()
    return r + (dc,)


@pytest.mark.parametrize("which", N_LIVE)
@pytest.mark.parametrize("A", [64, 128])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_fold_over_a_row_list_matches_the_full_entry(dev, P, A, which):
    """Tables pre-filled with a byte pattern: rows outside `live` keep it; live rows of g, f1, lse, z are the bits of
    han_sem_attn_bwd_rows on the same inputs with the dead dZ rows zeroed, s and df1 within the rounding bounds of
    tests/test_k3_fold_gpu.py; dw / db / du against the float64 sums over the live rows with the bounds of
    tests/sem_attn_ref.py; dc against the float64 column sum of g with _dc_depth of the live geometry."""
    from han_amd import ops
    N = FOLD_N[P]
    t = _inputs(P, N, A, dev, 2000 * P + A)
    ids = _live_ids(N, which, 10 * P + len(which))
    n_live = ids.size
    assert (n_live * P) % 16 != 0
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    mask[torch.from_numpy(ids).to(dev)] = True
    t["dZ"] = t["dZ"] * mask[:, None]
    live = torch.from_numpy(ids.astype(np.int32)).to(dev)
    code = ops.ACT_ELU
    gs0, df0, dw0, db0, du0, dc0 = _run_fold(ops, t, P, N, dev, code)                       # reference: the full entry
    gs, df1, dw, db, du, dc = _run_fold(ops, t, P, N, dev, code, live=live, fill=PATTERN)
    pat_f = torch.full((4,), PATTERN, dtype=torch.uint8, device=dev).view(torch.int32)
    n_s = n_df = 0
    for p in range(P):
        assert bool((gs[p][~mask] == PATTERN).all()), f"gs rows outside the list, meta-path {p}"
        assert bool((df1[p][~mask].view(torch.int32) == pat_f).all()), f"df1 rows outside the list, meta-path {p}"
        g, st = ops.gs_views(gs[p][mask])
        g0, st0 = ops.gs_views(gs0[p][mask])
        assert torch.equal(g.contiguous().view(torch.int32), g0.contiguous().view(torch.int32)), f"g bytes, meta-path {p}"
        for word, name in ((0, "f1"), (1, "lse"), (3, "z")):
            assert torch.equal(st[..., word].contiguous().view(torch.int32),
                               st0[..., word].contiguous().view(torch.int32)), f"{name}, meta-path {p}"
        # the bounds of tests/test_k3_fold_gpu.py for s and df1 (11 roundings on sum |g| (|pre| + |c|); 8 + 2 and s's)
        g64 = g.double()
        o = t["M"][mask][:, p, :].double()
        neg = o <= 0
        da = o + 1
        pre = torch.where(neg, torch.where(da > 0, torch.log(da.clamp_min(1e-300)), torch.zeros_like(o)), o)
        t_s = (g64.abs() * (pre.abs() + t["c"][p].double().abs())).view(n_live, 8, 8).sum(2)
        t_d = (g64.abs() * t["aggp"][p][mask].double().abs()).view(n_live, 8, 8).sum(2)
        s, s0 = st[..., 2].double(), st0[..., 2].double()
        ts_abs = t["tsum"][p][mask].double().abs()
        bound_s = 11 * U * t_s
        bound_d = U * (8 * t_d + 2 * (t_d + s0.abs() * ts_abs)) + ts_abs * bound_s
        assert bool(((s - s0).abs() <= bound_s).all()), f"s, meta-path {p}"
        d, d0 = df1[p][mask].double(), df0[p][mask].double()
        assert bool(((d - d0).abs() <= bound_d).all()), f"df1, meta-path {p}"
        n_s += int((st[..., 2].contiguous().view(torch.int32) != st0[..., 2].contiguous().view(torch.int32)).sum())
        n_df += int((df1[p][mask].view(torch.int32) != df0[p][mask].view(torch.int32)).sum())
        # dc: the float64 column sum of the (bit-equal) g rows of the list, chain depth of a grid over n_live * P rows
        depth = _dc_depth(n_live, P)
        want = g64.sum(0)
        bound_c = depth * U * g64.abs().sum(0)
        err = (dc[p].double() - want).abs()
        assert bool((err <= bound_c).all()), f"dc, meta-path {p}: {float((err / bound_c.clamp_min(1e-300)).max())} of the bound"
    # dw, db, du: float64 sums over the live rows from the kernel's own beta (tests/sem_attn_ref.py: T = n_live)
    case = {k: t[k].cpu().numpy() for k in ("M", "w", "b", "u", "dZ")}
    ref = sr.sem_ref(case, beta_in=t["beta"].cpu().numpy(), nodes=ids)
    ratios = {"dW": sr.ratio(dw.cpu().numpy(), ref.dW, ref.e_dW), "db": sr.ratio(db.cpu().numpy(), ref.db, ref.e_db),
              "du": sr.ratio(du.cpu().numpy(), ref.du, ref.e_du)}
    full = {"dW": sr.ratio(dw0.cpu().numpy(), ref.dW, ref.e_dW), "db": sr.ratio(db0.cpu().numpy(), ref.db, ref.e_db),
            "du": sr.ratio(du0.cpu().numpy(), ref.du, ref.e_du)}
    print(f"P={P} A={A} n_live={n_live}: err / bound live {ratios}, full entry {full}; s not bit-equal {n_s}, df1 {n_df}")
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_the_identity_list_gives_the_bytes_of_the_full_entry(dev):
    """live = 0 .. N - 1 at the existing entry's smallest size, 4 x 16384: every output byte-equal."""
    from han_amd import ops
    P, N, A = 4, 16384, 128
    t = _inputs(P, N, A, dev, 4321)
    live = torch.arange(N, dtype=torch.int32, device=dev)
    a = _run_fold(ops, t, P, N, dev, ops.ACT_ELU, fill=PATTERN)
    b = _run_fold(ops, t, P, N, dev, ops.ACT_ELU, live=live, fill=PATTERN)
    for p in range(P):
        assert torch.equal(a[0][p], b[0][p]), f"gs, meta-path {p}"
        assert torch.equal(a[1][p].view(torch.int32), b[1][p].view(torch.int32)), f"df1, meta-path {p}"
    for x, y, name in zip(a[2:], b[2:], ("dw", "db", "du", "dc")):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


def test_an_empty_list_launches_nothing_and_writes_zeros(dev):
    from han_amd import ops
    P, N, A = 4, 16384, 128
    t = _inputs(P, N, A, dev, 99)
    gs, df1, dw, db, du, dc = _run_fold(ops, t, P, N, dev, ops.ACT_ELU,
                                        live=torch.empty(0, dtype=torch.int32, device=dev), fill=PATTERN)
    assert all(bool((x == PATTERN).all()) for x in gs) and all(bool((x.view(torch.uint8) == PATTERN).all()) for x in df1)
    assert all(bool((x == 0).all()) for x in (dw, db, du, dc))


@pytest.mark.parametrize("why,P,N,D,A,kw", [
    ("P = 8", 8, 8192, 64, 128, {}),
    ("A = 256", 4, 16384, 64, 256, {}),
    ("D = 128", 4, 16384, 128, 128, {}),
    ("exact-pipe flag", 4, 16384, 64, 128, {"flags": 8}),
    ("pairs flag", 4, 16384, 64, 128, {"flags": 16}),
    ("fp32 G3 flag", 4, 16384, 64, 128, {"flags": 32}),
    ("bf16 tables", 4, 16384, 64, 128, {"table_dtype": torch.bfloat16}),
    ("4 x 16 heads", 4, 16384, 64, 128, {"K": 4, "FP": 16}),
])
def test_other_shapes_are_refused_before_any_launch(dev, why, P, N, D, A, kw):
    """The refusals of han_sem_attn_bwd_rows hold for the row-list entry -- but for the one on the row count."""
    from han_amd import _lib, ops
    lib = _lib.load()
    K, FP = kw.get("K", 8), kw.get("FP", 8)
    z = lambda *sh: torch.zeros(sh, device=dev)
    M, w, b, u, beta, dZ, c = z(N, P, D), z(D, A), z(A), z(A), z(N, P), z(N, D), z(P, 64)
    tabs = [[z(N, 64) for _ in range(P)], [z(N, K) for _ in range(P)], [z(N, K) for _ in range(P)], [z(N, K) for _ in range(P)]]
    gs = [torch.full((N, 384), 7, dtype=torch.uint8, device=dev) for _ in range(P)]
    df1 = [torch.full((N, K), 7.0, device=dev) for _ in range(P)]
    outs = [torch.full(sh, 7.0, device=dev) for sh in ((D, A), (A,), (A,), (P, 64))]
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=dev)
    live = torch.arange(0, N, 10, dtype=torch.int32, device=dev)
    arr = lambda ts: (ctypes.c_void_p * P)(*[x.data_ptr() for x in ts])
    code = lib.han_sem_attn_bwd_rows_live(M.data_ptr(), w.data_ptr(), b.data_ptr(), u.data_ptr(), beta.data_ptr(), dZ.data_ptr(),
                                          arr(tabs[0]), arr(tabs[1]), arr(tabs[2]), arr(tabs[3]), c.data_ptr(), arr(gs), arr(df1),
                                          *[o.data_ptr() for o in outs], ws.data_ptr(), ws.numel(), live.data_ptr(),
                                          live.numel(), N, P, D, A, K, FP,
                                          ops.DTYPE_CODE[kw.get("table_dtype", torch.float32)], 1, kw.get("flags", 0), None)
    torch.cuda.synchronize()
    assert code == _lib.E_UNSUPPORTED, why
    assert all(bool((x == 7).all()) for x in gs + df1 + outs), why


# ---------------------------------------------------------------------------------------------------------- gather
GN = 700                                       # sources = destinations
PLANTED = list(range(0, 21)) + [3, 4, 5, 15, 16, 17]      # live-row lengths 0 .. 20, the 4 and 16 boundaries twice
MID, LONG = 31, 75                             # a mid row (16 .. split_deg), a row beyond the test's split_deg of 48
_gather_cache = {}


def _gather_graph(dev):
    """Forward graph (rows = destinations) built from its sources: source j has live_len[j] live and dead_len[j] dead
    destinations, distinct; 30 % of the destinations are live.  -> (graph, values, live mask, live_len)."""
    if "g" not in _gather_cache:
        from han_amd.graph import CSRGraph
        rng = np.random.default_rng(77)
        live = rng.random(GN) < 0.3
        L, Dd = np.flatnonzero(live), np.flatnonzero(~live)
        live_len = rng.integers(0, 13, GN)
        live_len[:len(PLANTED)] = PLANTED
        live_len[len(PLANTED)], live_len[len(PLANTED) + 1] = MID, LONG
        dead_len = rng.integers(0, 31, GN)
        dead_len[[0, 5, len(PLANTED) + 1]] = [0, 40, 90]
        src, dst = [], []
        for j in range(GN):
            d = np.concatenate([rng.choice(L, int(live_len[j]), replace=False), rng.choice(Dd, int(dead_len[j]), replace=False)])
            dst.append(d)
            src.append(np.full(d.size, j))
        src, dst = np.concatenate(src), np.concatenate(dst)
        order = np.lexsort((src, dst))
        rowptr = np.zeros(GN + 1, dtype=np.int64)
        np.cumsum(np.bincount(dst, minlength=GN), out=rowptr[1:])
        g = CSRGraph.from_arrays(rowptr, src[order].astype(np.int32), GN, device=dev)
        vals = torch.tensor(rng.uniform(0.5, 1.5, g.nnz), dtype=torch.float32, device=dev)
        _gather_cache["g"] = (g, vals, torch.tensor(live, device=dev), live_len)
    return _gather_cache["g"]


@pytest.mark.parametrize("coef_drop", [0.0, 0.6])
@pytest.mark.parametrize("valued", [False, True])
def test_gather_on_the_live_graph(dev, monkeypatch, valued, coef_drop):
    """dH and df2 from the transposed graph with only the live destinations against those from the full transposed
    graph on the same table (whose dead rows hold g = 0): the same terms in another order -- within 1e-5 of the largest
    value, the tolerance of test_masked_edges_backward_is_bit_identical for the same comparison.  With the dead table
    rows filled with 0xFF bytes the live graph gives the same bits: they are never read.  A source without a live
    entry gets dH = df1 a1 exactly."""
    from han_amd import ops
    from han_amd.graph import CSRGraph
    monkeypatch.setattr(ops, "SPLIT_DEG", 48)
    monkeypatch.setattr(ops, "SPLIT_CHUNK", 16)
    g0, vals, live, live_len = _gather_graph(dev)
    K = FP = 8
    rng = np.random.default_rng(5 + int(valued))
    gens = lambda *sh: torch.tensor(rng.standard_normal(sh), dtype=torch.float32, device=dev)
    a1, a2, b1, b2, c = gens(K, FP) * 0.3, gens(K, FP) * 0.3, gens(K) * 0.1, gens(K) * 0.1, gens(64) * 0.1
    gg = CSRGraph(g0.rowptr, g0.colidx, GN, validate=False, values=vals if valued else None)
    gt = gg.transpose()
    gl = gt.with_live_columns(live)
    assert np.array_equal(gl.degrees().cpu().numpy(), live_len)
    assert not ops._use_lean(gt, a1) and not ops._use_lean(gl, a1)
    assert gl.row_split(ops.SPLIT_DEG, ops.SPLIT_CHUNK)["n_long"] == 1 and gl.row_bins(ops.SHORT_DEG, ops.SPLIT_DEG)["n_mid"] >= 1
    H, f1, f2 = ops.project_fwd(gens(GN, 64), torch.eye(64, device=dev), a1, a2, b1, b2, fts_drop=0.6, seed=9)
    kw = dict(coef_drop=coef_drop, fts_drop=0.6, seed=77)
    _, (o, lse, aggp, tsum) = ops.node_attn_fwd(gg, H, f1, a2, b2, c, train=True, **kw)
    dOut = gens(GN, 64) * live[:, None]
    gs, df1, _ = ops.node_attn_bwd_rows(dOut, o, aggp, tsum, f1, lse, c)
    assert bool((ops.gs_views(gs)[0][~live] == 0).all()) and bool((df1[~live] == 0).all())
    dH_f, df2_f = ops.node_attn_bwd_cols(gt, gs, H, f2, df1, a1, a2, **kw)
    dH_l, df2_l = ops.node_attn_bwd_cols(gl, gs, H, f2, df1, a1, a2, **kw)
    torch.cuda.synchronize()
    e_h, e_f = float((dH_l - dH_f).abs().max()), float((df2_l - df2_f).abs().max())
    print(f"valued={valued} coef_drop={coef_drop}: max |dH diff| {e_h:.3e} of {float(dH_f.abs().max()):.3e}, "
          f"max |df2 diff| {e_f:.3e} of {float(df2_f.abs().max()):.3e}")
    assert bool(torch.isfinite(dH_l).all()) and bool(torch.isfinite(df2_l).all())
    assert e_h < 1e-5 * max(1.0, float(dH_f.abs().max()))
    assert e_f < 1e-5 * max(1.0, float(df2_f.abs().max()))
    poisoned = gs.clone()
    poisoned[~live] = 0xFF
    dH_p, df2_p = ops.node_attn_bwd_cols(gl, poisoned, H, f2, df1, a1, a2, **kw)
    assert torch.equal(dH_p.view(torch.int32), dH_l.view(torch.int32))
    assert torch.equal(df2_p.view(torch.int32), df2_l.view(torch.int32))
    none = torch.tensor(live_len == 0, device=dev)
    assert int(none.sum()) >= 2
    assert bool((df2_l[none] == 0).all())
    assert torch.equal(dH_l[none].view(-1, K, FP), df1[none][:, :, None] * a1[None])


def test_a_small_dense_live_graph_keeps_off_the_lean_kernels(dev):
    """A live graph that is lean-eligible by size (256 table rows, >= 64 live entries per row: an ACM-like meta-path
    under live_backward=True).  The lean kernels read the whole table row 0 for every slot past the end of a row piece,
    and node 0 is dead here, so the live graph must run the row kernels: with the dead table rows filled with 0xFF bytes
    dH / df2 are finite, have the bits of the unpoisoned run, and agree with the full graph (which does run the lean
    kernel) to the 5e-5 of the largest value that test_gpu_parity.py allows between the lean and the row kernels."""
    from han_amd import ops
    from han_amd.graph import CSRGraph
    n, K, FP = 256, 8, 8
    rng = np.random.default_rng(123)
    live = np.zeros(n, dtype=bool)
    live[rng.permutation(np.arange(1, n))[:128]] = True            # node 0 is dead
    L, Dd = np.flatnonzero(live), np.flatnonzero(~live)
    src, dst = [], []
    for j in range(n):
        d = np.concatenate([rng.choice(L, int(rng.integers(70, 100)), replace=False), rng.choice(Dd, int(rng.integers(40, 90)), replace=False)])
        dst.append(d)
        src.append(np.full(d.size, j))
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = np.lexsort((src, dst))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    gg = CSRGraph.from_arrays(rowptr, src[order].astype(np.int32), n, device=dev)
    gt = gg.transpose()
    live_t = torch.tensor(live, device=dev)
    gl = gt.with_live_columns(live_t)
    gens = lambda *sh: torch.tensor(rng.standard_normal(sh), dtype=torch.float32, device=dev)
    a1, a2, b1, b2, c = gens(K, FP) * 0.3, gens(K, FP) * 0.3, gens(K) * 0.1, gens(K) * 0.1, gens(64) * 0.1
    H, f1, f2 = ops.project_fwd(gens(n, 64), torch.eye(64, device=dev), a1, a2, b1, b2, fts_drop=0.6, seed=9)
    assert ops.LEAN and ops._use_lean(gt, H) and ops._use_lean(gl, H)      # by size both would take the lean kernels
    kw = dict(coef_drop=0.6, fts_drop=0.6, seed=77)
    _, (o, lse, aggp, tsum) = ops.node_attn_fwd(gg, H, f1, a2, b2, c, train=True, f2=f2, **kw)
    gs, df1, _ = ops.node_attn_bwd_rows(gens(n, 64) * live_t[:, None], o, aggp, tsum, f1, lse, c)
    dH_f, df2_f = ops.node_attn_bwd_cols(gt, gs, H, f2, df1, a1, a2, **kw)
    dH_l, df2_l = ops.node_attn_bwd_cols(gl, gs, H, f2, df1, a1, a2, **kw)
    poisoned = gs.clone()
    poisoned[~live_t] = 0xFF
    dH_p, df2_p = ops.node_attn_bwd_cols(gl, poisoned, H, f2, df1, a1, a2, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dH_p).all()) and bool(torch.isfinite(df2_p).all())
    assert torch.equal(dH_p.view(torch.int32), dH_l.view(torch.int32)) and torch.equal(df2_p.view(torch.int32), df2_l.view(torch.int32))
    e_h, e_f = float((dH_l - dH_f).abs().max()), float((df2_l - df2_f).abs().max())
    print(f"lean-eligible live graph: max |dH diff| {e_h:.3e} of {float(dH_f.abs().max()):.3e}, max |df2 diff| {e_f:.3e} of {float(df2_f.abs().max()):.3e}")
    assert e_h < 5e-5 * (float(dH_f.abs().max()) + 1.0) and e_f < 5e-5 * (float(df2_f.abs().max()) + 1.0)


# ---------------------------------------------------------------------------------------------------------- trainer
def _trainer(dev, wl, masks, **kw):
    from han_amd import rng as hrng
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    torch.manual_seed(0)
    hrng.manual_seed(5)
    model = HeteGAT_multi().build(4, 64, 4, kw.pop("hid", (8,)), kw.pop("heads", (8, 1)), 128, device=dev,
                                  generator=torch.Generator().manual_seed(11))
    return model, HANTrainer(model, [wl["x"]] * 4, wl["graphs"], wl["labels"], masks[0], masks[1], **kw)


def _workload(dev):
    if "wl" not in _gather_cache:
        from han_amd import synth
        N = 16384
        wl = synth.planted_partition(N, 4, 4, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=dev)
        u = torch.rand(N, generator=torch.Generator().manual_seed(1))
        _gather_cache["wl"] = (wl, u)
    return _gather_cache["wl"]


def _masks(u, frac, dev):
    return (u < frac).to(torch.uint8).to(dev), ((u >= frac) & (u < frac + 0.1)).to(torch.uint8).to(dev)


@pytest.mark.parametrize("use_graph", [False, True])
def test_three_epochs_live_against_full(dev, monkeypatch, use_graph):
    """N = 16384, P = 4, 10 % train mask, three epochs from the same seeds with live_backward on and off.  The two
    runs add the same non-zero terms in another order, so they agree to rounding and not to the bit: parameters within
    2e-4 (the three-train-step tolerance of DESIGN.md section 6), each gradient slice within 2e-4 of its largest entry
    (the gradients of the third step are taken at parameters that already differ by the first bound).  This departs from
    the wording "the tolerance test_trainer_step_with_the_fold uses": that test asserts bit-equality (and the dc chain
    bound for c), which two summation orders cannot meet over three Adam steps.  The live run
    goes through the row-list entry and gives no zero-rows hint; the other run is today's path.  With use_graph=True
    the meta-paths run on streams of their own, where the K3 backward does not fold at all: that case covers the live
    graph over tables the row kernel wrote in full, not the row-list kernel (the eager case and the fold tests do).
    (live_backward=True: `auto` needs trainer.LIVE_BACKWARD_MIN_ROWS rows, which the small-graph parity tests of the
    default trainer make necessary.)"""
    from han_amd import ops
    wl, u = _workload(dev)
    seen = {"live": [], "hint": [], "nnz": []}
    fused, cols = ops.sem_attn_bwd_rows, ops.node_attn_bwd_cols

    def keep_fused(*a, **k):
        r = fused(*a, **k)
        seen["live"].append((k.get("live") is not None, r is not None))
        return r

    def keep_cols(graph_t, *a, **k):
        seen["hint"].append(bool(k.get("zero_rows", False)))
        seen["nnz"].append(graph_t.nnz)
        return cols(graph_t, *a, **k)

    monkeypatch.setattr(ops, "sem_attn_bwd_rows", keep_fused)
    monkeypatch.setattr(ops, "node_attn_bwd_cols", keep_cols)
    runs = {}
    for mode in (True, False):
        for v in seen.values():
            v.clear()
        model, tr = _trainer(dev, wl, _masks(u, 0.1, dev), live_backward=mode, use_graph=use_graph)
        assert tr.live_backward == (mode is True)
        for _ in range(3):
            tr.epoch()
        torch.cuda.synchronize()
        runs[mode] = (model.flat.clone(), model.flat_grad.clone(), model)
        full_nnz = sum(g.nnz for g in tr.graphs_t)
        # (a captured epoch runs its meta-paths on streams of their own, where the K3 backward does not fold: the row
        # kernel then writes every row, and the live graph reads the live ones)
        assert len(seen["live"]) == (0 if use_graph else 3) and all(s == (mode is True, True) for s in seen["live"])
        assert len(seen["hint"]) >= 4 and all(h == (mode is False) for h in seen["hint"])
        if mode is True:
            assert sum(seen["nnz"][:4]) < 0.2 * full_nnz
            assert all(bool((d[~tr.train_mask.bool()] == 0).all()) for d in tr._live_plan.df1(8))
        else:
            assert sum(seen["nnz"][:4]) == full_nnz
    (pa, ga, model), (pf, gf, _) = runs[True], runs[False]
    assert bool(torch.isfinite(pa).all()) and bool(ga.abs().max() > 0)
    dp = float((pa - pf).abs().max())
    print(f"use_graph={use_graph}: max |param diff| {dp:.3e} of {float(pf.abs().max()):.3e}")
    off = 0
    worst = 0.0
    for name, shp in model.param_shapes():
        n = int(np.prod(shp))
        a, b = ga[off:off + n], gf[off:off + n]
        off += n
        d, m = float((a - b).abs().max()), float(b.abs().max())
        print(f"  grad {name}: max diff {d:.3e} of {m:.3e}")
        worst = max(worst, d / max(m, 1e-30))
    assert dp < 2e-4
    assert worst < 2e-4


def test_auto_is_off_where_the_plan_does_not_hold(dev, monkeypatch):
    """`auto` needs LIVE_BACKWARD_MIN_ROWS rows (16384 are too few: the default there is the full backward); from that
    size on it is off for a train mask above half of the rows, a second node-attention layer and masked_backward=True.
    True switches it on at any size and refuses what `auto` would leave off for good."""
    from han_amd import trainer
    wl, u = _workload(dev)
    assert trainer.LIVE_BACKWARD_MIN_ROWS > 16384
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev))
    assert not tr.live_backward and tr.model.live_bwd is None
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev), live_backward=True)
    assert tr.live_backward and tr.model.live_bwd is not None
    with pytest.raises(ValueError, match="live_backward"):
        _trainer(dev, wl, _masks(u, 0.6, dev), live_backward=True)
    with pytest.raises(ValueError, match="live_backward"):
        _trainer(dev, wl, _masks(u, 0.1, dev), live_backward=True, hid=(8, 8), heads=(8, 8, 1))
    monkeypatch.setattr(trainer, "LIVE_BACKWARD_MIN_ROWS", 16384)      # these graphs are now large enough
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev))
    assert tr.live_backward and tr.model.live_bwd is not None
    _, tr = _trainer(dev, wl, _masks(u, 0.6, dev))
    assert not tr.live_backward and tr.model.live_bwd is None
    model, tr = _trainer(dev, wl, _masks(u, 0.1, dev), hid=(8, 8), heads=(8, 8, 1))
    assert model.extra and not tr.live_backward
    model, tr = _trainer(dev, wl, _masks(u, 0.1, dev), masked_backward=True)
    assert not tr.live_backward and model.masked_bwd is not None
    tr.set_masked_backward(False)
    assert tr.live_backward and model.masked_bwd is None
    tr.set_masked_backward(True)
    assert not tr.live_backward
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev), live_backward=False)
    assert not tr.live_backward
