"""GPU tests of the K2 backward kernels (han_amd/csrc/node_attn.hip) through han_amd.ops.node_attn_bwd_rows,
node_attn_bwd_cols, node_attn_bwd_cols_scores and score_param_bwd: per row and per element, |gpu - float64| <= e with the
reference and the bound e of tests/node_attn_ref.py (counts of fp32 roundings, derived there;
tests/test_node_attn_ref_host.py checks reference, bounds and cases without a GPU).  No forward error is counted twice:
the row-local pass runs on synthetic saved state, the transposed-graph pass on a synthetic gs table written through
ops.gs_views and on the table the row-local kernel itself wrote, s / df1 / z against the g values the kernel stored.

bwd_rows   every head shape x fp32 / bf16 g table x ELU / identity x with / without res, 403 rows in strided views, outputs
           exactly -1, 0, just below 0 and just above -1, heads whose dOut is all +-0: the stored g inside
           [RN(g - e), RN(g + e)], f1 and lse copied bit for bit, z exactly, s, df1, dc; the padding bytes of a row keep
           their bits.
bwd_cols   the edge graph of the forward file as the transposed graph (397 source rows, 2579 destinations: short rows,
           wave rows, chunk and finish kernels in one call) x every head shape x table x binary / edge values x
           {no dropout (MODE 0), both dropouts with table_gid and seed_dev (MODE 0, not FAST), both dropouts with
           src_offset / dst_offset != 0 (MODE 1; bf16: MODE 0 FAST), K2_FULL_GATHER (MODE 2), zero_rows (MODE 3), a masked
           graph (with_masked_columns), a live graph (with_live_columns)}; the unbinned launches; SPLIT_DEG = 48 /
           SPLIT_CHUNK = 16 (157 chunks: the finish kernel's loop turns).
scores     the same variants on the graph without rows beyond SPLIT_DEG through node_attn_bwd_cols_scores -- table_gid
           and graph.values included, which tests/test_bwd_cols_scores_gpu.py does not run: dH / df2 the bytes of the
           two-call path, da / db against depth x u x sum |terms|; score_param_bwd alone on 403 rows.

Past the loops, 8 x 8, fp32 with both dropouts and bf16 without: the wave, short and chunk graphs of the forward file as
transposed graphs (the first two through the fused score form as well: 16 384 slab rows and their fold), 2 x 16 x 1024 + 5
rows for bwd_rows and score_param_bwd.

The lean gathers (a 1031-row gs table, mean degree 89): every head shape x binary / edge values x {no dropout, both with
table_gid, both with offsets}; 8 x 8 at 2 x 32768 + 5 source rows of 64 entries, compared on the first and last 256 rows
of each grid pass and 4096 random rows, the rest checked finite.

The dense backward: density 0.82 at (130, 130) and (1000, 777), without dropout and with both.

Largest err / bound measured on an MI355X (gfx950), per kernel over all of its instances and cases (the number of
instances in brackets, MODE as launch_bwd_rows passes it: 4 + the gather mode for the fused score forms;
profiles/r26_k2_parity_ratios.json holds the table per instance, named by template arguments as in node_attn_ref.CELLS:
all 374 backward entries of CELLS ran).  One call launches several kernels (short rows, wave rows, chunk, finish) and its
ratios are recorded for each of them:

    backward kernel (instances)   dH      df2     s       df1     dc      da1     da2     db1     db2
    bwd_chunk MODE=0 (20)         0.68    0.33    -       -       -       -       -       -       -
    bwd_chunk MODE=1 (10)         0.63    0.32    -       -       -       -       -       -       -
    bwd_chunk MODE=2 (10)         0.63    0.31    -       -       -       -       -       -       -
    bwd_chunk MODE=3 (10)         0.63    0.31    -       -       -       -       -       -       -
    bwd_cols RPW=1 DEDUP (10)     0.59    0.31    -       -       -       -       -       -       -
    bwd_cols RPW=1 MASKED (20)    0.64    0.31    -       -       -       -       -       -       -
    bwd_cols RPW=1 MODE=0 (30)    0.68    0.34    -       -       -       -       -       -       -
    bwd_cols RPW=1 MODE=1 (10)    0.63    0.34    -       -       -       -       -       -       -
    bwd_cols RPW=1 MODE=2 (10)    0.63    0.34    -       -       -       -       -       -       -
    bwd_cols RPW=1 MODE=3 (10)    0.63    0.34    -       -       -       -       -       -       -
    bwd_cols RPW=1 MODE=4 (30)    -       -       -       -       -       0.019   0.032   0.0084  0.013
    bwd_cols RPW=1 MODE=5 (10)    -       -       -       -       -       0.015   0.035   0.0084  0.0095
    bwd_cols RPW=1 MODE=6 (10)    -       -       -       -       -       0.015   0.026   0.0076  0.014
    bwd_cols RPW=1 MODE=7 (10)    -       -       -       -       -       0.015   0.026   0.0076  0.014
    bwd_cols RPW=4 MASKED (20)    0.64    0.31    -       -       -       -       -       -       -
    bwd_cols RPW=4 MODE=0 (30)    0.84    0.38    -       -       -       -       -       -       -
    bwd_cols RPW=4 MODE=1 (10)    0.76    0.4     -       -       -       -       -       -       -
    bwd_cols RPW=4 MODE=2 (10)    0.63    0.34    -       -       -       -       -       -       -
    bwd_cols RPW=4 MODE=3 (10)    0.63    0.34    -       -       -       -       -       -       -
    bwd_cols RPW=4 MODE=4 (30)    -       -       -       -       -       0.022   0.036   0.0076  0.017
    bwd_cols RPW=4 MODE=5 (10)    -       -       -       -       -       0.018   0.035   0.0076  0.015
    bwd_cols RPW=4 MODE=6 (10)    -       -       -       -       -       0.015   0.026   0.0076  0.014
    bwd_cols RPW=4 MODE=7 (10)    -       -       -       -       -       0.015   0.026   0.0076  0.014
    bwd_dense (1)                 0.29    0.013   -       -       -       -       -       -       -
    bwd_dense_finish (1)          0.29    0.013   -       -       -       -       -       -       -
    bwd_finish (10)               0.68    0.33    -       -       -       -       -       -       -
    bwd_h8 (2)                    0.53    0.24    -       -       -       -       -       -       -
    bwd_rows (10)                 -       -       0.43    0.34    0.016   -       -       -       -
    score_param (10)              -       -       -       -       -       0.021   0.02    0.0072  0.0054

Every ratio is <= 1, every stored g lies in its rounding interval, f1, lse and z are exact, dH / df2 of the fused form are the
bytes of the two-call path in every variant (table_gid and graph.values included): no kernel bug was found, and
node_attn.hip is unchanged.  dH is the tightest: on a source row with few or no entries it is df1 a1 alone, two roundings
against the three the bound counts per term.  What the bounds still exclude is asserted in the host file.  The 336 cases of
this file take 16 s with 16 host threads, the slowest 2.1 s (2 x 131072 + 7 source rows), nearly all of it the float64
reference.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import node_attn_ref as R

pytestmark = pytest.mark.gpu

_SEEN = {}
CD, FD = 0.6, 0.5
N_ROWS = 403


def _note(cells, ratios):
    for tag in cells:
        for k, v in ratios.items():
            _SEEN[(tag, k)] = max(_SEEN.get((tag, k), 0.0), v)
    print(cells, {k: f"{v:.3g}" for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the largest err / bound per kernel instance and output when the module is done (pytest -s); HAN_RATIO_JSON
    names a file that receives the same table (merged with what the file already holds)."""
    yield
    for (tag, k), v in sorted(_SEEN.items()):
        print(f"{tag:70s} {k:6s} {v:.3g}")
    path = os.environ.get("HAN_RATIO_JSON")
    if path:
        table = {}
        if os.path.exists(path):
            with open(path) as f:
                table = json.load(f)
        table.update({f"{tag} | {k}": v for (tag, k), v in sorted(_SEEN.items())})
        with open(path, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)


def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a)).to(dev)


def _tdt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _table(H, bf16, dev):
    t = _t(H, dev)
    return t.to(torch.bfloat16) if bf16 else t      # exact: the values are bf16 numbers


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ------------------------------------------------------------------------------------------------ row-local pass
def _check_rows(dev, K, FP, bf16, elu, res, inp, strided=True):
    from han_amd import ops
    N = inp["out"].shape[0]
    tdt = _tdt(bf16)
    if strided:
        M = torch.zeros((N, 3, 64), device=dev)
        G = torch.zeros((N, 3, 64), device=dev)
        M[:, 1, :] = _t(inp["out"], dev)
        G[:, 1, :] = _t(inp["dOut"], dev)
        out_v, dout_v = M[:, 1, :], G[:, 1, :]
    else:
        out_v, dout_v = _t(inp["out"], dev), _t(inp["dOut"], dev)
    rb = ops.gs_row_bytes(K, FP, tdt)
    gs = torch.full((N, rb), 0xA5, dtype=torch.uint8, device=dev)
    dc = torch.full((64,), float("nan"), device=dev)
    got_gs, df1, got_dc = ops.node_attn_bwd_rows(dout_v, out_v, _t(inp["aggp"], dev), _t(inp["tsum"], dev), _t(inp["f1"], dev),
                                                 _t(inp["lse"], dev), _t(inp["c"], dev), R.ACT_ELU if elu else R.ACT_IDENTITY,
                                                 K, FP, tdt, res=_t(inp["res"], dev) if res else None, dc_out=dc, gs_out=gs)
    torch.cuda.synchronize()
    assert got_gs.data_ptr() == gs.data_ptr() and got_dc.data_ptr() == dc.data_ptr()
    gv, st = ops.gs_views(gs, K, FP, tdt)
    g_st = gv.float().cpu().numpy()
    st = st.cpu().numpy()
    used = 64 * (2 if bf16 else 4) + 16 * K
    assert bool((gs[:, used:] == 0xA5).all()), "padding bytes written"
    r = R.bwd_rows_ref(inp["dOut"], inp["out"], inp["aggp"], inp["tsum"], inp["f1"], inp["lse"], inp["c"], K, FP,
                       res=inp["res"] if res else None, elu=elu, bf16=bf16, g_stored=g_st)
    assert ((r.g_lo <= g_st) & (g_st <= r.g_hi)).all(), "stored g outside [RN(g - e), RN(g + e)]"
    assert np.array_equal(st[:, :, 0].view(np.uint32), inp["f1"].view(np.uint32)), "f1 not copied bit for bit"
    assert np.array_equal(st[:, :, 1].view(np.uint32), inp["lse"].view(np.uint32)), "lse not copied bit for bit"
    assert np.array_equal(st[:, :, 3].view(np.uint32), r.z), "z word"
    assert (r.z[inp["zero"]] == R.GS_Z_ALL_ZERO).all() and (r.z == 0).any()
    ratios = dict(s=R.ratio(st[:, :, 2], r.s, r.e_s), df1=R.ratio(df1.cpu().numpy(), r.df1, r.e_df1),
                  dc=R.ratio(dc.cpu().numpy(), r.dc, r.e_dc))
    _note([f"bwd_rows<FP={FP},BF={int(bf16)}>"], ratios)
    return gs, df1


@pytest.mark.parametrize("elu,res", [(True, False), (True, True), (False, True)], ids=["elu", "elu-res", "identity-res"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_bwd_rows(dev, K, FP, bf16, elu, res):
    inp = R.bwd_rows_inputs(K, FP, N_ROWS)
    o = inp["out"]
    assert (o == -1).any() and (o == 0).any() and (o == -np.float32(2.0 ** -24)).any() and inp["zero"].any()
    _check_rows(dev, K, FP, bf16, elu, res, inp)


# ------------------------------------------------------------------------------------------------ transposed-graph pass
VARIANTS = {      # name -> (coef_drop, fts_drop, table_gid, full_gather, zero_rows, graph form)
    "plain": (0.0, 0.0, False, False, False, None), "gid": (CD, FD, True, False, False, None),
    "drop": (CD, FD, False, False, False, None), "full": (CD, FD, False, True, False, None),
    "zero": (CD, FD, False, False, True, None), "masked": (CD, FD, False, False, False, "masked"),
    "live": (CD, FD, False, False, False, "live"),
}
F32_ONLY = ("full", "zero")      # the predicated gather (MODE 1-3) exists for fp32 tables only; bf16 runs MODE 0 in "drop"


def _cases(variants, vals=(False, True)):
    return [pytest.param(K, FP, bf, val, v, id=f"{K}x{FP}-{'bf16' if bf else 'f32'}-{'val' if val else 'bin'}-{v}")
            for K, FP in R.HEADS for bf in (False, True) for val in vals for v in variants if not (bf and v in F32_ONLY)]


@pytest.fixture(scope="module")
def score_graph():
    """The edge graph with its two rows beyond SPLIT_DEG shortened: the fused form takes it."""
    rowptr, _ = R.edge_graph()
    lens = np.diff(rowptr)
    lens = np.where(lens == 1025, 513, np.where(lens == 2500, 777, lens))
    return R.graph_from_lengths(lens, R.EDGE_NT)


def _gs_table(dev, K, FP, bf16, g, stats):
    from han_amd import ops
    gs = torch.zeros((g.shape[0], ops.gs_row_bytes(K, FP, _tdt(bf16))), dtype=torch.uint8, device=dev)
    gv, st = ops.gs_views(gs, K, FP, _tdt(bf16))
    gv.copy_(_table(g, bf16, dev))
    st.copy_(_t(stats, dev))
    return gs


def _run_cols(dev, monkeypatch, colptr, rowidx, nt, K, FP, bf16, val, variant, *, binned=True,
              split=(R.SPLIT_DEG, R.SPLIT_CHUNK), score=False, table=None, lean=False, dense=False):
    """One node_attn_bwd_cols call (and, score=True, the fused call) against the reference."""
    from han_amd import ops
    from han_amd.graph import CSRGraph
    cd, fd, gid, full, zero_rows, form = VARIANTS[variant]
    if full:
        monkeypatch.setattr(ops, "K2_FULL_GATHER", True)
    ns = len(colptr) - 1
    b = R.bwd_cols_inputs(K, FP, bf16, ns, nt, fd)
    g_np, stats_np, gs = (b["g"], b["stats"], None) if table is None else table
    if gs is None:
        gs = _gs_table(dev, K, FP, bf16, g_np, stats_np)
    values = R.edge_values(len(rowidx), 1) if val else None
    gt = CSRGraph(_t(colptr, dev), _t(rowidx, dev), n_cols=nt, values=None if values is None else _t(values, dev))
    r_colptr, r_rowidx, r_values, empty_mid = colptr, rowidx.astype(np.int64), values, False
    live = np.arange(nt) % 3 != 0
    if form == "masked":
        gt = gt.with_masked_columns(_t(live, dev))
        r_rowidx = np.where(live[rowidx], rowidx, -1)
        assert gt.masked
    elif form == "live":
        gt = gt.with_live_columns(_t(live.astype(np.uint8), dev))
        keep = live[rowidx]
        r_rowidx = rowidx[keep].astype(np.int64)
        r_colptr = np.zeros(ns + 1, dtype=np.int64)
        r_colptr[1:] = np.cumsum(np.bincount(np.repeat(np.arange(ns), np.diff(colptr))[keep], minlength=ns))
        r_values = values[keep] if val else None
        empty_mid = True
        assert np.array_equal(gt.rowptr.cpu().numpy(), r_colptr) and not gt.masked
    gid_np = ((np.arange(nt, dtype=np.int64) * 5 + 17) % 100_003).astype(np.int32) if gid else None
    kw = dict(coef_drop=cd, fts_drop=fd, seed=11, zero_rows=zero_rows)
    rkw = dict(bf16=bf16, values=r_values, coef_drop=cd, fts_drop=fd, seed=11, binned=binned, split=split, empty_mid=empty_mid)
    if gid:
        kw.update(table_gid=_t(gid_np, dev), seed_dev=torch.tensor([R.SEED_DEV], dtype=torch.int64, device=dev))
        rkw.update(gid=gid_np, seed_dev=R.SEED_DEV)
    if variant == "drop":
        kw.update(src_offset=7, dst_offset=1_000_003)
        rkw.update(src_offset=7, dst_offset=1_000_003)
    args = (gt, gs, _table(b["H"], bf16, dev), _t(b["f2"], dev), _t(b["df1"], dev), _t(b["a1"], dev), _t(b["a2"], dev))
    assert ops._use_lean(gt, args[2]) == lean and (not lean or ops._use_dense(gt, args[2], K, FP) == dense)
    assert not dense or R.dense_applies(b["f2"])
    rkw.update(lean=lean, dense=dense)
    dH, df2 = ops.node_attn_bwd_cols(*args, **kw)
    torch.cuda.synchronize()
    r = R.bwd_cols_ref(r_colptr, r_rowidx, g_np, stats_np, b["H"], b["f2"], b["df1"], b["a1"], b["a2"], **rkw)
    assert r.flushed <= 0.01 * max(r.entries, 1)
    deg = np.diff(r_colptr)
    forms = tuple(np.unique(R.row_forms(deg, binned, split[0], empty_mid)))
    ckw = dict(gid=gid, masked=form == "masked", full_gather=full, zero_rows=zero_rows)
    _note(["bwd_dense", "bwd_dense_finish"] if dense else R.lean_bwd_cells(K, FP, val, gid) if lean else R.bwd_cells(K, FP, bf16, val, cd, forms=forms, **ckw),
          dict(dH=R.ratio(dH.cpu().numpy(), r.dH, r.e_dH), df2=R.ratio(df2.cpu().numpy(), r.df2, r.e_df2)))
    if not score:
        return
    outs = [torch.full(s, float("nan"), device=dev) for s in ((K, FP), (K, FP), (K,), (K,))]
    got = ops.node_attn_bwd_cols_scores(*args, out=outs, **kw)
    torch.cuda.synchronize()
    assert got is not None, "eligible call declined"
    assert torch.equal(_bits(got[0]), _bits(dH)) and torch.equal(_bits(got[1]), _bits(df2)), "not the bytes of the two calls"
    launches = [(int((R.row_forms(deg, binned, split[0], empty_mid) == f).sum()), rpw) for f, rpw in ((R.SHORT, 4), (R.WAVE, 1))]
    sr = R.score_ref(b["H"], b["df1"], df2.cpu().numpy(), K, FP, R.score_depth([x for x in launches if x[0]]))
    _note(R.bwd_cells(K, FP, bf16, val, cd, forms=forms, score=True, **ckw), R.score_ratios(sr, [o.cpu().numpy() for o in outs]))


@pytest.mark.parametrize("K,FP,bf16,val,variant", _cases(list(VARIANTS)))
def test_bwd_cols_edge_graph(dev, monkeypatch, K, FP, bf16, val, variant):
    colptr, rowidx = R.edge_graph()
    _run_cols(dev, monkeypatch, colptr, rowidx, R.EDGE_NT, K, FP, bf16, val, variant)


@pytest.mark.parametrize("K,FP,bf16,val,variant", _cases(["plain", "gid", "drop", "full", "zero"]))
def test_fused_scores_gid_and_values(dev, monkeypatch, score_graph, K, FP, bf16, val, variant):
    colptr, rowidx = score_graph
    assert np.diff(colptr).max() == R.SPLIT_DEG
    _run_cols(dev, monkeypatch, colptr, rowidx, R.EDGE_NT, K, FP, bf16, val, variant, score=True)


@pytest.mark.parametrize("variant", ["plain", "gid", "drop"])
@pytest.mark.parametrize("val", [False, True], ids=["bin", "val"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_lean_gathers(dev, monkeypatch, K, FP, val, variant):
    """131 source rows of 0 .. 333 entries against a 1031-row gs table: the one-lane-per-head kernel at 8 x 8 without an id
    table, the DEDUP gather otherwise."""
    colptr, rowidx = R.lean_graph()
    _run_cols(dev, monkeypatch, colptr, rowidx, R.LEAN_NT, K, FP, False, val, variant, lean=True)


@pytest.mark.parametrize("variant", ["plain", "drop"])
@pytest.mark.parametrize("n,nt", [(130, 130), (1000, 777)])
def test_dense_backward(dev, monkeypatch, n, nt, variant):
    """Density 0.82 (>= 0.65), 8 x 8, binary, no id table: the matrix-pipe form over the transposed bit mask."""
    colptr, rowidx = R.dense_graph(n, nt)
    _run_cols(dev, monkeypatch, colptr, rowidx, nt, 8, 8, False, False, variant, lean=True, dense=True)


def test_lean_gather_past_the_grid_cap(dev):
    """2 x 32768 + 5 source rows of 64 entries against a 4099-row gs table, 8 x 8, both dropouts: the float64 comparison on
    the first and the last 256 rows of each grid pass and 4096 random rows, every other element finite."""
    from han_amd import ops
    from han_amd.graph import CSRGraph
    K, FP, n, nt = 8, 8, R.LEAN_LOOP_ROWS, R.LOOP_NT
    colptr, rowidx = R.graph_from_lengths(np.full(n, 64), nt)
    b = R.bwd_cols_inputs(K, FP, False, n, nt, FD)
    gt = CSRGraph(_t(colptr, dev), _t(rowidx, dev), n_cols=nt)
    H = _t(b["H"], dev)
    assert ops._use_lean(gt, H) and not ops._use_dense(gt, H, K, FP)
    gs = _gs_table(dev, K, FP, False, b["g"], b["stats"])
    dH, df2 = ops.node_attn_bwd_cols(gt, gs, H, _t(b["f2"], dev), _t(b["df1"], dev), _t(b["a1"], dev), _t(b["a2"], dev),
                                     coef_drop=CD, fts_drop=FD, seed=11, src_offset=7, dst_offset=1_000_003)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dH).all()) and bool(torch.isfinite(df2).all())
    pick = R.lean_loop_sample()
    cp, ri = R.sample_rows(colptr, rowidx, pick)
    r = R.bwd_cols_ref(cp, ri, b["g"], b["stats"], b["H"][pick], b["f2"][pick], b["df1"][pick], b["a1"], b["a2"],
                       coef_drop=CD, fts_drop=FD, seed=11, src_offset=7, dst_offset=1_000_003, lean=True, row_ids=pick)
    _note(R.lean_bwd_cells(K, FP, False), dict(dH=R.ratio(dH.cpu().numpy()[pick], r.dH, r.e_dH),
                                               df2=R.ratio(df2.cpu().numpy()[pick], r.df2, r.e_df2)))


LOW_LENGTHS = (1, 0, 3, 4, 5, 15, 16, 17, 33, 2, 1, 4, 3, 5, 1, 2)


@pytest.mark.parametrize("shape", ["low", "high"])
@pytest.mark.parametrize("variant", ["plain", "drop"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", [(8, 8), (2, 32)])
def test_unbinned_row_shapes(dev, monkeypatch, score_graph, K, FP, bf16, variant, shape):
    from han_amd import ops
    monkeypatch.setattr(ops, "BINNED", False)
    if shape == "low":
        (colptr, rowidx), nt = R.graph_from_lengths([LOW_LENGTHS[i % 16] for i in range(203)], 257), 257
    else:
        (colptr, rowidx), nt = score_graph, R.EDGE_NT
    assert set(R.row_forms(np.diff(colptr), False)) == ({R.SHORT} if shape == "low" else {R.WAVE})
    _run_cols(dev, monkeypatch, colptr, rowidx, nt, K, FP, bf16, False, variant, binned=False, score=True)


@pytest.mark.parametrize("variant", ["plain", "drop", "masked"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_many_chunks_finish_loop(dev, monkeypatch, K, FP, bf16, variant):
    from han_amd import ops
    monkeypatch.setattr(ops, "SPLIT_DEG", 48)
    monkeypatch.setattr(ops, "SPLIT_CHUNK", 16)
    colptr, rowidx = R.edge_graph()
    _run_cols(dev, monkeypatch, colptr, rowidx, R.EDGE_NT, K, FP, bf16, False, variant, split=(48, 16))


@pytest.mark.parametrize("bf16,variant", [(False, "drop"), (True, "plain")], ids=["f32-both", "bf16-plain"])
@pytest.mark.parametrize("kind", ["wave", "short", "chunk"])
def test_bwd_cols_past_the_grid_cap(dev, monkeypatch, kind, bf16, variant):
    """Every block goes round its grid-stride loop twice, a few a third time (node_attn_ref.loop_graph)."""
    from han_amd import ops
    split = (R.SPLIT_DEG, R.SPLIT_CHUNK)
    if kind == "chunk":
        split = R.LOOP_SPLIT
        monkeypatch.setattr(ops, "SPLIT_DEG", split[0])
        monkeypatch.setattr(ops, "SPLIT_CHUNK", split[1])
    colptr, rowidx = R.loop_graph(kind)
    assert all(p[2] == 3 for p in R.grid_passes(np.diff(colptr), True, *split).values())
    _run_cols(dev, monkeypatch, colptr, rowidx, R.LOOP_NT, 8, 8, bf16, False, variant, split=split, score=kind != "chunk")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_bwd_rows_and_score_param_past_their_row_loops(dev, bf16):
    """2 x 16 x 1024 + 5 rows: every lane group of the 1024 blocks takes two rows, five take a third."""
    from han_amd import ops
    K, FP, N = 8, 8, R.LOOP_ROWS
    _check_rows(dev, K, FP, bf16, True, True, R.bwd_rows_inputs(K, FP, N, seed=2))
    b = R.bwd_cols_inputs(K, FP, bf16, N, 17, FD)
    df2 = np.random.default_rng([K, N]).standard_normal((N, K)).astype(np.float32)
    got = ops.score_param_bwd(_table(b["H"], bf16, dev), _t(b["df1"], dev), _t(df2, dev), K, FP)
    torch.cuda.synchronize()
    sr = R.score_ref(b["H"], b["df1"], df2, K, FP, R.depth_rows(N))
    _note([f"score_param<FP={FP},BF={int(bf16)}>"], R.score_ratios(sr, [o.cpu().numpy() for o in got]))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", [(8, 8), (1, 64), (16, 4)])
def test_bwd_cols_on_the_table_bwd_rows_wrote(dev, monkeypatch, K, FP, bf16):
    """The [g | f1, lse, s, z] table straight from node_attn_bwd_rows (2579 destination rows) into the gather."""
    from han_amd import ops
    inp = R.bwd_rows_inputs(K, FP, R.EDGE_NT, seed=1)
    gs, _ = _check_rows(dev, K, FP, bf16, True, True, inp, strided=False)
    gv, st = ops.gs_views(gs, K, FP, _tdt(bf16))
    colptr, rowidx = R.edge_graph()
    table = (gv.float().cpu().numpy(), st.cpu().numpy(), gs)
    for variant in ("drop", "zero" if not bf16 else "plain"):
        _run_cols(dev, monkeypatch, colptr, rowidx, R.EDGE_NT, K, FP, bf16, False, variant, table=table)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_score_param_bwd(dev, K, FP, bf16):
    from han_amd import ops
    b = R.bwd_cols_inputs(K, FP, bf16, N_ROWS, 17, FD)
    df2 = np.random.default_rng([K, 4]).standard_normal((N_ROWS, K)).astype(np.float32)
    outs = [torch.full(s, float("nan"), device=dev) for s in ((K, FP), (K, FP), (K,), (K,))]
    got = ops.score_param_bwd(_table(b["H"], bf16, dev), _t(b["df1"], dev), _t(df2, dev), K, FP, out=outs)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == o.data_ptr() for a, o in zip(got, outs))
    sr = R.score_ref(b["H"], b["df1"], df2, K, FP, R.depth_rows(N_ROWS))
    _note([f"score_param<FP={FP},BF={int(bf16)}>"], R.score_ratios(sr, [o.cpu().numpy() for o in outs]))


def test_every_backward_cell_was_reached(dev):
    want = [c for c in R.CELLS if c.startswith(("bwd", "score"))]
    seen = {tag for tag, _ in _SEEN}
    assert [c for c in want if c not in seen] == []
    assert all(v <= 1.0 for v in _SEEN.values())
