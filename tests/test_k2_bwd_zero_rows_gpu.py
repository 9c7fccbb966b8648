"""K2 backward: the fourth word of a head's statistics record, z, says that all g values of the head in that row are
+-0 (han_hip.h: HAN_GS_Z_ALL_ZERO; 0 = they may be anything), and the predicated backward gather, told that most rows
are zero (zero_rows=True: HAN_FLAG_K2_ZERO_ROWS), does not request the g piece of such a head.  Both producers (the row
kernel, the K3 backward's epilogue) must write z exactly where the stored g values are all zero; the gather's sums must
be BIT-EQUAL to the full gather's (ops.K2_FULL_GATHER, which ignores z) and to those of the form without the hint, what
sits in a left-out piece must not reach them, and clearing z must change nothing.  HANTrainer gives the hint for a
one-layer model whose train mask covers at most half of the rows."""
import numpy as np
import pytest
import torch

from tests.test_k2_bwd_skip_gpu import HEADS, N1, _both_forms, _ragged_graph, _t, classic_kernels  # noqa: F401
from tests.test_k3_fold_gpu import _inputs as _fold_inputs

pytestmark = pytest.mark.gpu

FOLD_CASES = [(4, 16384), (4, 16387), (1, 65541)]


def _z_bits(stats):
    return stats[..., 3].contiguous().view(torch.int32)


def _want_z(ops, gs, K, FP, tdt=torch.float32):
    """(N, K) bool from the stored g values: every one of the head's FP values is +0 or -0."""
    g, _ = ops.gs_views(gs, K, FP, tdt)
    return (g.float().view(g.shape[0], K, FP) == 0).all(2)


def _assert_z(ops, gs, K, FP, tdt=torch.float32):
    want = _want_z(ops, gs, K, FP, tdt)
    _, stats = ops.gs_views(gs, K, FP, tdt)
    exp = torch.where(want, torch.full_like(_z_bits(stats), ops.GS_Z_ALL_ZERO), torch.zeros_like(_z_bits(stats)))
    assert torch.equal(_z_bits(stats), exp)
    return want


def _row_inputs(n, K, rng, dev):
    """What node_attn_bwd_rows reads besides dOut: ELU outputs (some 0, some -1: derivative 0), random tables."""
    out = rng.standard_normal((n, 64))
    out = np.where(out < 0, np.expm1(out), out)
    kind = rng.integers(0, 40, (n, 64))
    out[kind == 0] = 0.0
    out[kind == 1] = -1.0
    return [_t(a, dev) for a in (out, rng.standard_normal((n, 64)), rng.standard_normal((n, K)),
                                 rng.standard_normal((n, K)), rng.standard_normal((n, K)), 0.1 * rng.standard_normal(64))]


def _sparse_dout(n, K, FP, dead_frac, rng):
    """dOut (n, 64) float32 with `dead_frac` of its rows zero, single heads of live rows zero, -0.0 in a third of the
    zeroed slots, and in dead row `lone` one head whose only non-zero value sits in its last column."""
    d = rng.standard_normal((n, K, FP)).astype(np.float32)
    d[d == 0] = 1.0
    dead = rng.random(n) < dead_frac
    d[dead] = 0.0
    d[(rng.random((n, K)) < 0.15) & ~dead[:, None]] = 0.0
    d[(d == 0) & (rng.random((n, K, FP)) < 1 / 3)] = -0.0
    lone = int(np.flatnonzero(dead)[7])
    d[lone, K // 2, FP - 1] = 0.375
    return d.reshape(n, 64), dead, lone


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,FP", HEADS)
def test_row_kernel_sets_z_exactly_where_a_head_is_zero(dev, K, FP, tdt):
    """30 % and 90 % of the rows zero, single zero heads, -0.0 among the zeros, a lone value in a head's last column;
    outputs of -1 (derivative 0) add zero g values under a non-zero dOut.  z is compared with the stored g."""
    from han_amd import ops
    rng = np.random.default_rng(7 * K + FP)
    n = N1
    out, aggp, tsum, f1, lse, c = _row_inputs(n, K, rng, dev)
    for frac in (0.3, 0.9):
        d, dead, lone = _sparse_dout(n, K, FP, frac, rng)
        o = out.clone()
        o.view(n, K, FP)[5, K - 1] = -1.0                      # a head whose derivative is 0 throughout, dOut or no
        gs, _, _ = ops.node_attn_bwd_rows(_t(d, dev), o, aggp, tsum, f1, lse, c, K=K, FP=FP, table_dtype=tdt)
        want = _assert_z(ops, gs, K, FP, tdt)
        dead_t = _t(dead, dev, torch.bool)
        assert bool(want[dead_t].sum() == int(dead.sum()) * K - 1) and not bool(want[lone, K // 2])
        assert bool(want[5, K - 1]) and bool(want[~dead_t].any()) and bool((~want[~dead_t]).any())
        g, _ = ops.gs_views(gs, K, FP, tdt)
        assert bool((g.float() == 0).logical_and(torch.signbit(g.float())).any())      # -0 is among the stored zeros


@pytest.mark.parametrize("P,N", FOLD_CASES)
def test_fold_epilogue_writes_the_row_kernels_z(dev, P, N):
    """ops.sem_attn_bwd_rows with 90 % of the dZ rows zero and, in live rows, M = -1 across one head: word 3 of its
    tables is bit-equal to word 3 of node_attn_bwd_rows on the same dM, and set exactly where its own g is zero."""
    from han_amd import ops
    t = _fold_inputs(P, N, 128, dev, 77 + P)
    gen = torch.Generator(device="cpu").manual_seed(N)
    live = (torch.rand(N, generator=gen) < 0.1).to(dev)
    t["dZ"] = t["dZ"] * live[:, None]
    M = t["M"]
    pick = (torch.rand(N, P, generator=gen) < 0.25).to(dev)
    head = torch.randint(0, 8, (N, P), generator=gen).to(dev)
    sel = pick[:, :, None] & (torch.arange(8, device=dev)[None, None, :] == head[:, :, None])      # (N, P, 8 heads)
    M.view(N, P, 8, 8)[sel] = -1.0
    _, t["beta"] = ops.sem_attn_fwd(M, t["w"], t["b"], t["u"])
    dM = ops.sem_attn_bwd(M, t["w"], t["b"], t["u"], t["beta"], t["dZ"])[0]
    dc = torch.empty((P, 64), device=dev)
    r = ops.sem_attn_bwd_rows(M, t["w"], t["b"], t["u"], t["beta"], t["dZ"],
                              [(t["aggp"][p], t["tsum"][p], t["f1"][p], t["lse"][p]) for p in range(P)], t["c"], dc)
    assert r is not None, "the library refused an eligible shape"
    for p in range(P):
        ref = ops.node_attn_bwd_rows(dM[:, p, :], M[:, p, :], t["aggp"][p], t["tsum"][p], t["f1"][p], t["lse"][p], t["c"][p])[0]
        want = _assert_z(ops, r[0][p], 8, 8)
        assert torch.equal(_z_bits(ops.gs_views(r[0][p])[1]), _z_bits(ops.gs_views(ref)[1])), p
        assert bool(want[~live].all()) and bool(want[live][sel[live, p]].all())
        assert bool((~want[live]).sum() > 4 * int(live.sum()))


def _k2_case(ops, dev, K, FP, seed):
    """Forward tensors on the ragged graph shared by the consumer tests."""
    rng = np.random.default_rng(seed)
    gens = lambda *sh: _t(rng.standard_normal(sh), dev)
    a1, a2, b1, b2, c = gens(K, FP) * 0.3, gens(K, FP) * 0.3, gens(K) * 0.1, gens(K) * 0.1, gens(64) * 0.1
    return rng, dict(a1=a1, a2=a2, b1=b1, b2=b2, c=c, X=gens(N1, 64), dOut=gens(N1, 64))


def _douts(t, K, FP, rng, dev):
    """dOut at live fractions 0, 0.1, 0.3 and 1, and one with single zero heads in every row."""
    u = _t(rng.random(N1), dev)
    out = {f: t["dOut"] * (u < f)[:, None] for f in (0.0, 0.1, 0.3, 1.0)}
    keep = _t(rng.random((N1, K)) < 0.5, dev, torch.bool)
    out["heads"] = (t["dOut"].view(N1, K, FP) * keep[:, :, None]).reshape(N1, 64)
    return out


@pytest.mark.parametrize("K,FP", HEADS)
def test_gather_with_zero_heads_equals_full_gather(dev, classic_kernels, K, FP):
    """dH and df2 of the zero_rows form (which honours z), of the full gather and of the default form (which do not) are torch.equal on the
    ragged graph -- all row lengths around the step and batch boundaries, a row beyond the split degree -- at live
    fractions 0, 0.1, 0.3, 1 and with single zero heads, attention dropout 0.6 / 0.95, projected-row dropout off / on,
    with and without edge values."""
    from han_amd.graph import CSRGraph
    ops = classic_kernels
    g0, vals, _ = _ragged_graph(dev)
    rng, t = _k2_case(ops, dev, K, FP, 300 * K + FP)
    douts = _douts(t, K, FP, rng, dev)
    eye = torch.eye(64, device=dev)
    for v in (None, vals):
        gg = CSRGraph(g0.rowptr, g0.colidx, N1, validate=False, values=v)
        gt = gg.transpose()
        assert gt.row_split(ops.SPLIT_DEG, ops.SPLIT_CHUNK)["n_long"] == 1
        for fts_drop in (0.0, 0.6):
            H, f1, f2 = ops.project_fwd(t["X"], eye, t["a1"], t["a2"], t["b1"], t["b2"], fts_drop=fts_drop, seed=9)
            for coef_drop in (0.6, 0.95):
                kw = dict(coef_drop=coef_drop, fts_drop=fts_drop, seed=77)
                _, (o, lse, aggp, tsum) = ops.node_attn_fwd(gg, H, f1, t["a2"], t["b2"], t["c"], train=True, **kw)
                kz = dict(kw, zero_rows=True)
                for name, d in douts.items():
                    gs, df1, _ = ops.node_attn_bwd_rows(d, o, aggp, tsum, f1, lse, t["c"], K=K, FP=FP)
                    nz = int((_z_bits(ops.gs_views(gs, K, FP)[1]) != 0).sum())
                    assert (nz == N1 * K) if name == 0.0 else (nz > 0) if name != 1.0 else (nz < N1 * K // 100), (name, nz)
                    (dH_s, df2_s), (dH_f, df2_f) = _both_forms(ops, gt, gs, H, f2, df1, t["a1"], t["a2"], **kz)
                    dH_d, df2_d = ops.node_attn_bwd_cols(gt, gs, H, f2, df1, t["a1"], t["a2"], **kw)
                    case = (v is not None, fts_drop, coef_drop, name)
                    assert bool(torch.isfinite(dH_f).all()), case
                    assert torch.equal(dH_s, dH_f) and torch.equal(dH_d, dH_f), case
                    assert torch.equal(df2_s, df2_f) and torch.equal(df2_d, df2_f), case


def _poison_setup(dev, ops, fts_drop, coef_drop=0.6):
    from han_amd.graph import CSRGraph
    K = FP = 8
    g0, vals, _ = _ragged_graph(dev)
    rng, t = _k2_case(ops, dev, K, FP, 4242)
    gg = CSRGraph(g0.rowptr, g0.colidx, N1, validate=False, values=vals)
    gt = gg.transpose()
    H, f1, f2 = ops.project_fwd(t["X"], torch.eye(64, device=dev), t["a1"], t["a2"], t["b1"], t["b2"], fts_drop=fts_drop, seed=9)
    kw = dict(coef_drop=coef_drop, fts_drop=fts_drop, seed=77)
    _, (o, lse, aggp, tsum) = ops.node_attn_fwd(gg, H, f1, t["a2"], t["b2"], t["c"], train=True, **kw)
    # 30 % live rows, and single zero heads in the live ones
    d = t["dOut"].view(N1, K, FP) * _t(rng.random(N1) < 0.3, dev, torch.bool)[:, None, None]
    d = (d * _t(rng.random((N1, K)) < 0.7, dev, torch.bool)[:, :, None]).reshape(N1, 64)
    gs, df1, _ = ops.node_attn_bwd_rows(d, o, aggp, tsum, f1, lse, t["c"])
    return gt, gs, (H, f2, df1, t["a1"], t["a2"]), kw


@pytest.mark.parametrize("fts_drop", [0.0, 0.6])
def test_pieces_under_a_set_z_are_not_read(dev, classic_kernels, fts_drop):
    """NaN in every g piece whose z is set: dH / df2 of the zero_rows form are the bits of the unpoisoned run and finite;
    the full gather shows NaN at every (source, head) with a poisoned incoming edge, and so does the form without the
    hint at some (it leaves out dropped heads only)."""
    ops = classic_kernels
    K = FP = 8
    gt, gs, rest, kw = _poison_setup(dev, ops, fts_drop)
    zset = _z_bits(ops.gs_views(gs)[1]) != 0                              # (N1, K), row = destination
    assert bool(zset.all(1).sum() > N1 // 2) and bool((zset.any(1) & ~zset.all(1)).sum() > 100)
    poisoned = gs.clone()
    ops.gs_views(poisoned)[0].view(N1, K, FP)[zset] = float("nan")
    src_of = torch.repeat_interleave(torch.arange(N1, device=dev), gt.degrees().long())
    hit = torch.zeros((N1, K), dtype=torch.int32, device=dev)
    hit = hit.index_add_(0, src_of, zset[gt.colidx.long()].to(torch.int32)) > 0
    assert bool(hit.sum() > N1)
    dH_ref, df2_ref = ops.node_attn_bwd_cols(gt, gs, *rest, **kw)
    (dH_s, df2_s), (dH_f, df2_f) = _both_forms(ops, gt, poisoned, *rest, zero_rows=True, **kw)
    assert bool(torch.isfinite(dH_ref).all()) and bool(torch.isfinite(df2_ref).all())
    assert torch.equal(dH_s, dH_ref) and torch.equal(df2_s, df2_ref)
    assert bool(torch.isnan(df2_f[hit]).all()) and bool(torch.isnan(dH_f.view(N1, K, FP)[hit]).all())
    df2_d = ops.node_attn_bwd_cols(gt, poisoned, *rest, **kw)[1]      # no hint: z is not looked at
    assert bool(torch.isnan(df2_d[hit]).any()) and not bool(torch.isnan(df2_d[~hit]).any())


@pytest.mark.parametrize("fts_drop", [0.0, 0.6])
def test_z_is_an_optimisation_only(dev, classic_kernels, fts_drop):
    """The same tables with word 3 cleared to 0 everywhere give bit-equal dH / df2."""
    ops = classic_kernels
    gt, gs, rest, kw = _poison_setup(dev, ops, fts_drop)
    cleared = gs.clone()
    ops.gs_views(cleared)[1][..., 3] = 0.0
    assert bool((_z_bits(ops.gs_views(cleared)[1]) == 0).all()) and bool((_z_bits(ops.gs_views(gs)[1]) != 0).any())
    dH, df2 = ops.node_attn_bwd_cols(gt, gs, *rest, zero_rows=True, **kw)
    dH_c, df2_c = ops.node_attn_bwd_cols(gt, cleared, *rest, zero_rows=True, **kw)
    assert torch.equal(dH, dH_c) and torch.equal(df2, df2_c)


def test_three_epochs_equal_the_full_gather(dev, monkeypatch):
    """HANTrainer, N = 16384, P = 4, 10 % train mask, three epochs from the same seeds: parameters and gradients of the
    default run and of a run with ops.K2_FULL_GATHER are torch.equal; the K3 backward writes the tables (fold path), and
    the trainer tells every backward gather that most rows are zero (with a 60 % mask it does not)."""
    from han_amd import ops
    from han_amd import rng as hrng
    from han_amd import synth
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    N = 16384
    fused_calls = []
    fused = ops.sem_attn_bwd_rows

    def keep_fused(*a, **k):
        r = fused(*a, **k)
        fused_calls.append(r is not None)
        return r

    monkeypatch.setattr(ops, "sem_attn_bwd_rows", keep_fused)
    hints = []
    cols = ops.node_attn_bwd_cols

    def keep_hint(*a, **k):
        hints.append(bool(k.get("zero_rows", False)))
        return cols(*a, **k)

    monkeypatch.setattr(ops, "node_attn_bwd_cols", keep_hint)
    wl = synth.planted_partition(N, 4, 4, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=dev)
    u = torch.rand(N, generator=torch.Generator().manual_seed(1))
    train_mask, val_mask = (u < 0.1).to(torch.uint8).to(dev), ((u >= 0.1) & (u < 0.2)).to(torch.uint8).to(dev)
    runs = []
    try:
        for full in (False, True):
            ops.K2_FULL_GATHER = full
            torch.manual_seed(0)
            hrng.manual_seed(5)
            model = HeteGAT_multi().build(4, 64, 4, (8,), (8, 1), 128, device=dev, generator=torch.Generator().manual_seed(11))
            tr = HANTrainer(model, [wl["x"]] * 4, wl["graphs"], wl["labels"], train_mask, val_mask)
            for _ in range(3):
                tr.epoch()
            torch.cuda.synchronize()
            runs.append((model.flat.clone(), model.flat_grad.clone()))
    finally:
        ops.K2_FULL_GATHER = False
    assert len(fused_calls) == 6 and all(fused_calls)
    assert len(hints) == 2 * 3 * 4 and all(hints)
    model = HeteGAT_multi().build(4, 64, 4, (8,), (8, 1), 128, device=dev, generator=torch.Generator().manual_seed(11))
    wide = HANTrainer(model, [wl["x"]] * 4, wl["graphs"], wl["labels"], (u < 0.6).to(torch.uint8).to(dev), val_mask)
    wide.epoch()
    assert len(hints) == 2 * 3 * 4 + 4 and not any(hints[-4:]) and not model.zero_rows
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(runs[0][1].abs().max() > 0)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
