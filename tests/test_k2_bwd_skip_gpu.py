"""K2 backward gather: the row and chunk kernels leave out the g values of (edge, head) pairs whose attention-dropout
draw fell (bwd_consume in node_attn.hip).  A dropped head contributes exact zeros, so the sums must be BIT-EQUAL to the
full gather (HAN_FLAG_K2_FULL_GATHER, ops.K2_FULL_GATHER), and what sits in the left-out pieces must not reach them."""
import numpy as np
import pytest
import torch

from tests import rng_ref

pytestmark = pytest.mark.gpu

HEADS = [(8, 8), (4, 16), (1, 64), (16, 4)]
PLANTED = [0, 1, 3, 4, 15, 16, 17, 63, 64, 65]     # 4-edge tail step, 16-edge full step, 64-id batch, short-row bin
N1, LONG = 3000, 2500                              # LONG > ops.SPLIT_DEG: the chunk and finish kernels run

_graph_cache = {}


def _t(a, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)


def _graph_from_sources(n, lens, rng, dev):
    """Forward CSR graph (rows = destinations) whose source j has lens[j] distinct random destinations."""
    from han_amd.graph import CSRGraph
    src = np.repeat(np.arange(n), lens)
    dst = np.concatenate([rng.choice(n, size=int(l), replace=False) for l in lens]) if src.size else src
    order = np.lexsort((src, dst))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return CSRGraph.from_arrays(rowptr, src[order].astype(np.int32), n, device=dev)


def _ragged_graph(dev):
    """3000 rows; transposed-row lengths random in 0..140 with the boundary lengths planted and one row of 2500."""
    if "g" not in _graph_cache:
        rng = np.random.default_rng(2024)
        lens = rng.integers(0, 141, N1)
        lens[:len(PLANTED)] = PLANTED
        lens[len(PLANTED)] = LONG
        g = _graph_from_sources(N1, lens, rng, dev)
        deg_t = g.transpose().degrees().cpu().numpy()
        assert np.array_equal(deg_t, lens)
        _graph_cache["g"] = (g, _t(rng.uniform(0.5, 1.5, g.nnz), dev), _t((rng.random(N1) < 0.3).astype(np.float32), dev) > 0)
    return _graph_cache["g"]


@pytest.fixture
def classic_kernels():
    """The row / chunk kernels also where a small graph would take the lean ones (which gather whole rows)."""
    from han_amd import ops
    old = ops.LEAN
    ops.LEAN = False
    yield ops
    ops.LEAN = old
    ops.K2_FULL_GATHER = False


def _both_forms(ops, *args, **kw):
    try:
        ops.K2_FULL_GATHER = False
        skip = ops.node_attn_bwd_cols(*args, **kw)
        ops.K2_FULL_GATHER = True
        full = ops.node_attn_bwd_cols(*args, **kw)
    finally:
        ops.K2_FULL_GATHER = False
    return skip, full


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("K,FP", HEADS)
def test_predicated_gather_equals_full_gather(dev, classic_kernels, K, FP, tdt):
    """dH and df2 of the default form and of the full gather are torch.equal: every row length around the step, batch
    and bin boundaries, a row beyond the split degree, attention dropout 0 / 0.6 / 0.95, projected-row dropout off /
    on, with and without table_gid, edge values, masked columns.
    What the library predicates today (bwd_gather_mode in node_attn.hip): fp32 tables, attention dropout > 0, no
    table_gid, unmasked graph -- the FAST row kernels and the chunk kernel; those combinations compare the predicated
    gather with its full-gather twin.  In the others (bf16, table_gid, masked columns, attention dropout 0) the flag
    changes nothing and both sides run the same kernel: they guard the launch rule, should it be relaxed."""
    from han_amd.graph import CSRGraph
    ops = classic_kernels
    g0, vals, live = _ragged_graph(dev)
    n = N1
    rng = np.random.default_rng(100 * K + FP)
    gens = lambda *sh: _t(rng.standard_normal(sh), dev)
    a1, a2, b1, b2, c = gens(K, FP) * 0.3, gens(K, FP) * 0.3, gens(K) * 0.1, gens(K) * 0.1, gens(64) * 0.1
    X, dOut = gens(n, 64), gens(n, 64)
    ident = torch.arange(n, dtype=torch.int32, device=dev)
    eye = torch.eye(64, device=dev)
    for v in (None, vals):
        gg = CSRGraph(g0.rowptr, g0.colidx, n, validate=False, values=v)
        gt = gg.transpose()
        assert gt.row_split(ops.SPLIT_DEG, ops.SPLIT_CHUNK)["n_long"] == 1
        gm = gt.with_masked_columns(live)
        for fts_drop in (0.0, 0.6):
            H, f1, f2 = ops.project_fwd(X, eye, a1, a2, b1, b2, fts_drop=fts_drop, seed=9, table_dtype=tdt)
            for coef_drop in (0.0, 0.6, 0.95):
                kw = dict(coef_drop=coef_drop, fts_drop=fts_drop, seed=77)
                _, sv = ops.node_attn_fwd(gg, H, f1, a2, b2, c, train=True, **kw)
                pre, lse, aggp, tsum = sv
                for masked in (False, True):
                    d = dOut * live[:, None] if masked else dOut      # masked columns: g == 0 outside the mask
                    gs, df1, _ = ops.node_attn_bwd_rows(d, pre, aggp, tsum, f1, lse, c, K=K, FP=FP, table_dtype=tdt)
                    for gid in (None, ident):
                        (dH_s, df2_s), (dH_f, df2_f) = _both_forms(ops, gm if masked else gt, gs, H, f2, df1, a1, a2,
                                                                   table_gid=gid, **kw)
                        case = (v is not None, fts_drop, coef_drop, masked, gid is not None)
                        assert bool(torch.isfinite(dH_f).all()), case
                        assert torch.equal(dH_s, dH_f), case
                        assert torch.equal(df2_s, df2_f), case


def test_dropped_pieces_do_not_reach_the_result(dev, classic_kernels):
    """900 destinations with one incoming edge each: NaN written into the g columns of every dropped (edge, head) must
    not change dH / df2 of the default form by a bit, and must show in the full gather -- the poison sits where the old
    kernel reads."""
    from han_amd.graph import CSRGraph
    ops = classic_kernels
    n, K, FP, drop, seed = 900, 8, 8, 0.6, 77
    rng = np.random.default_rng(31)
    src = rng.integers(0, n, n)
    dst = np.arange(n)
    keep = rng_ref.coef_draws(seed, dst, src, K, drop) > 0            # (E, K): edge e is dst e <- src[e]
    for half in (keep[:, :4], keep[:, 4:]):                          # one hash, one 128-byte line of the fp32 g row
        assert int((~half).all(1).sum()) >= 50
    gg = CSRGraph.from_arrays(np.arange(n + 1), src.astype(np.int32), n, device=dev)
    gt = gg.transpose()
    gens = lambda *sh: _t(rng.standard_normal(sh), dev)
    a1, a2, b1, b2, c = gens(K, FP) * 0.3, gens(K, FP) * 0.3, gens(K) * 0.1, gens(K) * 0.1, gens(64) * 0.1
    H, f1, f2 = ops.project_fwd(gens(n, 64), torch.eye(64, device=dev), a1, a2, b1, b2, fts_drop=drop, seed=9)
    kw = dict(coef_drop=drop, fts_drop=drop, seed=seed)
    _, sv = ops.node_attn_fwd(gg, H, f1, a2, b2, c, train=True, **kw)
    pre, lse, aggp, tsum = sv
    gs, df1, _ = ops.node_attn_bwd_rows(gens(n, 64), pre, aggp, tsum, f1, lse, c)
    poisoned = gs.clone()
    g_view, _ = ops.gs_views(poisoned)
    dropped = _t(~keep, dev, torch.bool)                             # (n, K), row = destination
    g_view.view(n, K, FP)[dropped] = float("nan")
    hit = torch.zeros((n, K), dtype=torch.int32, device=dev)          # (source, head) pairs with a poisoned edge
    hit = hit.index_add_(0, _t(src, dev, torch.long), dropped.to(torch.int32)) > 0
    assert bool(hit.any(1).sum() > 100)
    # (launches with table_gid stay on the full gather: no general instantiation here)
    dH_ref, df2_ref = ops.node_attn_bwd_cols(gt, gs, H, f2, df1, a1, a2, **kw)
    (dH_s, df2_s), (dH_f, df2_f) = _both_forms(ops, gt, poisoned, H, f2, df1, a1, a2, **kw)
    assert bool(torch.isfinite(dH_ref).all()) and bool(torch.isfinite(df2_ref).all())
    assert torch.equal(dH_s, dH_ref) and torch.equal(df2_s, df2_ref)
    assert bool(torch.isnan(df2_f[hit]).all()) and bool(torch.isnan(dH_f.view(n, K, FP)[hit]).all())
