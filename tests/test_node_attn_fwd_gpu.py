"""GPU tests of the K2 forward gather kernels (han_amd/csrc/node_attn.hip) through han_amd.ops.node_attn_fwd and
node_attn_coefs: per row and per element, |gpu - float64| <= e with the reference and the bound e of
tests/node_attn_ref.py (counts of fp32 roundings, derived there; tests/test_node_attn_ref_host.py checks reference, bounds
and cases without a GPU).  Checked: out, and of a training call lse, aggp and tsum; node_attn_coefs against p am / l.

The edge graph (node_attn_ref.edge_graph): 397 rows whose lengths cycle through 0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63,
64, 65, 127, 128, 129, with single rows of 1023, 1024, 1025 and 2500 entries (the SPLIT_DEG / SPLIT_CHUNK boundary of
han_amd.ops, no monkeypatch), columns distinct within a row, against a 2579-row table: one call runs the short-row, the
wave-per-row, the chunk and the finish kernel.  Cases: every head shape x fp32 / bf16 table x binary / edge values x
{eval, train without dropout, attention dropout only, row dropout only, both (FAST)}; both dropouts with table_gid; the
shared hash (8 x 8); K2_DEEP (bf16 eval); f2_src (1 x 64); res, the identity activation, row_offset != 0 and seed_dev;
scores spread over more than 80 with the maximum arriving last; the unbinned launches (ops.BINNED = False) with the low
and the high row shape; SPLIT_DEG = 48 / SPLIT_CHUNK = 16, where the 2500-entry row has 157 chunks and the finish kernel's
own loop turns; rows=RowSubset into a strided out=M[:, p, :] with every other byte checked unchanged.

Past the grid cap (attn_grid: 8192 blocks of 4 waves), 8 x 8, fp32 both dropouts and bf16 eval: 2 x 32768 + 5 wave rows of
16 .. 24 entries, 2 x 131072 + 7 short rows of 1 .. 15 entries, 2 x 32768 + 5 chunks (SPLIT_DEG = SPLIT_CHUNK = 16), against
a 4099-row table.

The lean kernels (f2 passed; a 1031-row table, mean degree 89, rows of 0 .. 333 entries): every head shape x binary / edge
values x the five modes; 8 x 8 with both dropouts at 2 x 32768 + 5 rows of 64 entries (a 4099-row table), compared on the
first and last 256 rows of each grid pass and 4096 random rows, the rest checked finite.

The dense matrix-pipe form: density 0.82 at (130, 130) and (1000, 777), the five modes, and its device-side fallback
to the lean kernel on scores that range over more than 80.

Largest err / bound measured on an MI355X (gfx950), per kernel over all of its instances and cases (the number of
instances in brackets; profiles/r26_k2_parity_ratios.json holds the table per instance, named by template arguments as in
node_attn_ref.CELLS: all 211 forward entries of CELLS ran).  One call launches several kernels (short rows, wave rows,
chunk, finish) and its ratios are recorded for each of them:

    forward kernel (instances)    out     lse     aggp    tsum    coef
    coef (5)                      -       -       -       -       0.066
    fwd RPW=1 (72)                0.51    0.22    1       1       -
    fwd RPW=4 (60)                0.51    0.21    0.51    0.12    -
    fwd_chunk (40)                0.51    0.21    0.51    0.12    -
    fwd_dense (2)                 0.43    0.062   0.012   0.014   -
    fwd_dense_finish (2)          0.43    0.062   0.012   0.014   -
    fwd_finish (10)               0.51    0.21    0.51    0.12    -
    fwd_h8 (4)                    0.49    0.18    0.055   0.049   -
    fwd_lean (16)                 0.5     0.16    0.061   0.059   -

Every ratio is <= 1: no kernel bug was found, and node_attn.hip is unchanged.  The 0.5 of `out` is an empty row or a
fully dropped one, out = act(c + res): one rounding against the two the bound counts.  The 1 (0.999997) of aggp / tsum is
the fp32 both-dropouts case past the grid cap: 8 of its 10.5 million (entry, head) scores lie within their own rounding
error of 0, the kernel took the other branch of LeakyReLU's slope for one of them, and the bound of such an entry is that
difference itself; everywhere else aggp and tsum stay below 0.52.  What the bounds still exclude is asserted in the host
file.  The 281 cases of this file take 18 s with 16 host threads, the slowest 2.2 s (2 x 131072 + 7 rows), nearly all of it
the float64 reference.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import node_attn_ref as R

pytestmark = pytest.mark.gpu

_SEEN = {}
BF = {False: "f32", True: "bf16"}
OFFSET = 1_000_003


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


def _table(H, bf16, dev):
    t = _t(H, dev)
    return t.to(torch.bfloat16) if bf16 else t      # exact: the values are bf16 numbers


def _graph(rowptr, colidx, nt, dev, values=None):
    from han_amd.graph import CSRGraph
    return CSRGraph(_t(rowptr, dev), _t(colidx, dev), n_cols=nt, values=None if values is None else _t(values, dev))


MODES = {      # name -> (train, coef_drop, fts_drop)
    "eval": (False, 0.0, 0.0), "train": (True, 0.0, 0.0), "coef": (True, 0.6, 0.0), "fts": (True, 0.0, 0.5),
    "both": (True, 0.6, 0.5),
}


def _run(dev, rowptr, colidx, nt, K, FP, bf16, mode, *, val=False, gid=False, extras=False, elu=True, kind="plain",
         f2_src=False, binned=True, split=(R.SPLIT_DEG, R.SPLIT_CHUNK), shared_hash=False, deep=False, sort=False,
         lean=False, dense=None):
    """One node_attn_fwd call against the reference; returns nothing, notes and asserts the ratios."""
    from han_amd import ops
    train, cd, fd = MODES[mode]
    n = len(rowptr) - 1
    d = R.fwd_inputs(K, FP, bf16, n, nt, kind, fd)
    if sort:
        colidx = R.sort_rows_by_score(rowptr, colidx, d["f2"])
    values = R.edge_values(len(colidx)) if val else None
    g = _graph(rowptr, colidx, nt, dev, values)
    gid_np = ((np.arange(nt, dtype=np.int64) * 5 + 17) % 100_003).astype(np.int32) if gid else None
    kw = dict(train=train, coef_drop=cd, fts_drop=fd, seed=11, activation=R.ACT_ELU if elu else R.ACT_IDENTITY)
    rkw = dict(bf16=bf16, values=values, train=train, coef_drop=cd, fts_drop=fd, seed=11, elu=elu, binned=binned,
               split=split, gid=gid_np)
    if extras:
        sd = torch.tensor([R.SEED_DEV], dtype=torch.int64, device=dev)
        kw.update(res=_t(d["res"], dev), row_offset=OFFSET, seed_dev=sd)
        rkw.update(res=d["res"], row_offset=OFFSET, seed_dev=R.SEED_DEV)
    if gid:
        kw.update(table_gid=_t(gid_np, dev))
    if f2_src:
        kw.update(f2_src=_t(d["f2"], dev))
        rkw.update(f2=d["f2"])
    if lean:      # f2 given, a small fp32 table, long rows: the lean kernels (han_amd.ops._use_lean), not the dense form
        kw.update(f2=_t(d["f2"], dev))
        rkw.update(f2=d["f2"], lean=True)
        assert ops._use_lean(g, _t(d["H"], dev)) and not bf16 and not gid
        assert ops._use_dense(g, _t(d["H"], dev), K, FP) == (dense is not None)
        if dense is not None:      # "applies": the fixed-shift form; "fallback": the device finds the range too wide: lean kernel
            assert R.dense_applies(d["f2"]) == (dense == "applies")
            rkw.update(dense=dense == "applies")
    out = torch.full((n, 64), float("nan"), device=dev)
    got, saved = ops.node_attn_fwd(g, _table(d["H"], bf16, dev), _t(d["f1"], dev), _t(d["a2"], dev), _t(d["b2"], dev),
                                   _t(d["c"], dev), out=out, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    r = R.fwd_ref(rowptr, colidx, d["H"], d["f1"], d["a2"], d["b2"], d["c"], **rkw)
    assert r.undecided <= 0.01 * max(len(colidx) * K, 1)
    sv = None
    if train:
        assert saved[0].data_ptr() == out.data_ptr()
        sv = [t.cpu().numpy() for t in saved[1:]]
        empty = np.diff(rowptr) == 0
        assert (sv[0][empty].view(np.uint32) == np.float32(R.NEG_BIG).view(np.uint32)).all()
    else:
        assert saved is None
    forms = tuple(np.unique(R.row_forms(np.diff(rowptr), binned, split[0])))
    cells = R.fwd_cells(K, FP, bf16, val, train, cd, fd, gid=gid, f2_src=f2_src, shared_hash=shared_hash, deep=deep,
                        forms=forms)
    if lean:
        cells = R.lean_fwd_cells(K, FP, val, train)
    if dense == "applies":
        cells = [f"fwd_dense<TRAIN={int(train)}>", f"fwd_dense_finish<TRAIN={int(train)}>"]
    _note(cells, R.fwd_ratios(r, out.cpu().numpy(), sv))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("val", [False, True], ids=["bin", "val"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_edge_graph(dev, K, FP, bf16, val, mode):
    rowptr, colidx = R.edge_graph()
    _run(dev, rowptr, colidx, R.EDGE_NT, K, FP, bf16, mode, val=val)


@pytest.mark.parametrize("mode", ["eval", "both"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_res_offset_seed_dev_and_identity(dev, K, FP, bf16, mode):
    rowptr, colidx = R.edge_graph()
    _run(dev, rowptr, colidx, R.EDGE_NT, K, FP, bf16, mode, extras=True, elu=(K, FP) not in ((8, 8), (2, 32)))
    if (K, FP) == (8, 8):
        _run(dev, rowptr, colidx, R.EDGE_NT, K, FP, bf16, mode, extras=True, elu=True)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_table_gid_is_not_the_fast_kernel(dev, K, FP, bf16):
    rowptr, colidx = R.edge_graph()
    _run(dev, rowptr, colidx, R.EDGE_NT, K, FP, bf16, "both", gid=True)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_shared_hash(dev, monkeypatch, bf16):
    from han_amd import ops
    monkeypatch.setattr(ops, "K2_SHARED_HASH", True)
    rowptr, colidx = R.edge_graph()
    _run(dev, rowptr, colidx, R.EDGE_NT, 8, 8, bf16, "both", shared_hash=True)


@pytest.mark.parametrize("val", [False, True], ids=["bin", "val"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_deep_bf16_eval(dev, monkeypatch, K, FP, val):
    from han_amd import ops
    monkeypatch.setattr(ops, "K2_DEEP", True)
    rowptr, colidx = R.edge_graph()
    _run(dev, rowptr, colidx, R.EDGE_NT, K, FP, True, "eval", val=val, deep=True)


@pytest.mark.parametrize("mode", ["eval", "coef"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_f2_src_one_head(dev, bf16, mode):
    rowptr, colidx = R.edge_graph()
    _run(dev, rowptr, colidx, R.EDGE_NT, 1, 64, bf16, mode, f2_src=True)


@pytest.mark.parametrize("mode", ["eval", "both"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", [(8, 8), (2, 32), (1, 64)])
def test_wide_scores_maximum_last(dev, K, FP, bf16, mode):
    rowptr, colidx = R.edge_graph()
    d = R.fwd_inputs(K, FP, bf16, len(rowptr) - 1, R.EDGE_NT, "wide", MODES[mode][2])
    x = R.up(d["f2"])[:, 0]
    x = np.where(x > 0, x, R.SLOPE * x)
    assert x.max() - x.min() > 80
    _run(dev, rowptr, colidx, R.EDGE_NT, K, FP, bf16, mode, kind="wide", sort=True)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("val", [False, True], ids=["bin", "val"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_lean_kernels(dev, K, FP, val, mode):
    """f2 passed, 131 rows of 0 .. 333 entries against a 1031-row table: the one-lane-per-head kernel at 8 x 8, the lean
    16-lane kernel at every other head shape; res, row_offset and seed_dev in the "both" and "eval" cases."""
    rowptr, colidx = R.lean_graph()
    _run(dev, rowptr, colidx, R.LEAN_NT, K, FP, False, mode, val=val, lean=True, extras=mode in ("both", "eval"))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n,nt", [(130, 130), (1000, 777)])
def test_dense_form(dev, n, nt, mode):
    """Density 0.82 (>= 0.65), 8 x 8, binary: the matrix-pipe form with its fixed shift per row; res, row_offset and
    seed_dev in the "both" and "eval" cases."""
    rowptr, colidx = R.dense_graph(n, nt)
    _run(dev, rowptr, colidx, nt, 8, 8, False, mode, lean=True, dense="applies", extras=mode in ("both", "eval"))


@pytest.mark.parametrize("mode", ["eval", "both"])
def test_dense_form_falls_back_on_a_wide_score_range(dev, mode):
    """Scores ranging over more than 80: the dense launches return at once and the lean kernel behind them does the work."""
    rowptr, colidx = R.dense_graph(130, 130)
    _run(dev, rowptr, colidx, 130, 8, 8, False, mode, lean=True, dense="fallback", kind="wide")


def test_lean_kernel_past_the_grid_cap(dev):
    """2 x 32768 + 5 rows of 64 entries against a 4099-row table, 8 x 8, both dropouts: the float64 comparison on the first
    and the last 256 rows of each grid pass and 4096 random rows, every other element finite."""
    from han_amd import ops
    K, FP, n, nt = 8, 8, R.LEAN_LOOP_ROWS, R.LOOP_NT
    rowptr, colidx = R.graph_from_lengths(np.full(n, 64), nt)
    d = R.fwd_inputs(K, FP, False, n, nt, "plain", 0.5)
    g = _graph(rowptr, colidx, nt, dev)
    H = _t(d["H"], dev)
    assert ops._use_lean(g, H) and not ops._use_dense(g, H, K, FP) and -(-n // (4 * R.GRID_CAP)) == 3
    out = torch.full((n, 64), float("nan"), device=dev)
    _, saved = ops.node_attn_fwd(g, H, _t(d["f1"], dev), _t(d["a2"], dev), _t(d["b2"], dev), _t(d["c"], dev), out=out,
                                 train=True, coef_drop=0.6, fts_drop=0.5, seed=11, f2=_t(d["f2"], dev))
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in saved)
    pick = R.lean_loop_sample()
    assert {0, 32767, 32768, 65535, 65536, n - 1} <= set(pick.tolist())
    rp, ci = R.sample_rows(rowptr, colidx, pick)
    r = R.fwd_ref(rp, ci, d["H"], d["f1"][pick], d["a2"], d["b2"], d["c"], f2=d["f2"], train=True, coef_drop=0.6,
                  fts_drop=0.5, seed=11, lean=True, row_ids=pick)
    _note(R.lean_fwd_cells(K, FP, False, True), R.fwd_ratios(r, out.cpu().numpy()[pick], [t.cpu().numpy()[pick] for t in saved[1:]]))


LOW_LENGTHS = (1, 0, 3, 4, 5, 15, 16, 17, 33, 2, 1, 4, 3, 5, 1, 2)


@pytest.mark.parametrize("shape", ["low", "high"])
@pytest.mark.parametrize("mode", ["eval", "both"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", [(8, 8), (2, 32)])
def test_unbinned_row_shapes(dev, monkeypatch, K, FP, bf16, mode, shape):
    from han_amd import ops
    monkeypatch.setattr(ops, "BINNED", False)
    if shape == "low":
        rowptr, colidx = R.graph_from_lengths([LOW_LENGTHS[i % 16] for i in range(203)], 257)
        nt = 257
    else:
        (rowptr, colidx), nt = R.edge_graph(), R.EDGE_NT
    forms = R.row_forms(np.diff(rowptr), False)
    assert set(forms[np.diff(rowptr) <= R.SPLIT_DEG]) == ({R.SHORT} if shape == "low" else {R.WAVE})
    _run(dev, rowptr, colidx, nt, K, FP, bf16, mode, binned=False)


@pytest.mark.parametrize("mode", ["eval", "both"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_many_chunks_finish_loop(dev, monkeypatch, K, FP, bf16, mode):
    from han_amd import ops
    monkeypatch.setattr(ops, "SPLIT_DEG", 48)
    monkeypatch.setattr(ops, "SPLIT_CHUNK", 16)
    rowptr, colidx = R.edge_graph()
    assert -(-2500 // 16) > 64
    _run(dev, rowptr, colidx, R.EDGE_NT, K, FP, bf16, mode, split=(48, 16))


@pytest.mark.parametrize("bf16,mode", [(False, "both"), (True, "eval")], ids=["f32-both", "bf16-eval"])
@pytest.mark.parametrize("kind", ["wave", "short", "chunk"])
def test_past_the_grid_cap(dev, monkeypatch, kind, bf16, mode):
    """Every block goes round its grid-stride loop twice, a few a third time (node_attn_ref.loop_graph)."""
    from han_amd import ops
    split = (R.SPLIT_DEG, R.SPLIT_CHUNK)
    if kind == "chunk":
        split = R.LOOP_SPLIT
        monkeypatch.setattr(ops, "SPLIT_DEG", split[0])
        monkeypatch.setattr(ops, "SPLIT_CHUNK", split[1])
    rowptr, colidx = R.loop_graph(kind)
    assert all(p[2] == 3 for p in R.grid_passes(np.diff(rowptr), True, *split).values())
    _run(dev, rowptr, colidx, R.LOOP_NT, 8, 8, bf16, mode, split=split)


@pytest.mark.parametrize("bf16,mode", [(False, "both"), (True, "eval")], ids=["f32-both", "bf16-eval"])
def test_row_subset_into_a_strided_view(dev, bf16, mode):
    """rows=RowSubset, out=M[:, 1, :]: the listed rows lie within the bound, every other byte of M keeps its bits."""
    from han_amd import ops
    K, FP = 8, 8
    train, cd, fd = MODES[mode]
    rowptr, colidx = R.edge_graph()
    n = len(rowptr) - 1
    d = R.fwd_inputs(K, FP, bf16, n, R.EDGE_NT, "plain", fd)
    g = _graph(rowptr, colidx, R.EDGE_NT, dev)
    listed = (np.arange(n) % 3 == 1) | (np.diff(rowptr) > 1000)
    M = torch.full((n, 3, 64), float("nan"), device=dev)
    M.view(torch.int32).copy_(torch.arange(n * 192, device=dev).view(n, 3, 64) | 0x7FC00000)      # NaNs with distinct payloads
    before = M.clone()
    got, saved = ops.node_attn_fwd(g, _table(d["H"], bf16, dev), _t(d["f1"], dev), _t(d["a2"], dev), _t(d["b2"], dev),
                                   _t(d["c"], dev), out=M[:, 1, :], train=train, coef_drop=cd, fts_drop=fd, seed=11,
                                   rows=ops.RowSubset(g, _t(listed, dev)))
    torch.cuda.synchronize()
    r = R.fwd_ref(rowptr, colidx, d["H"], d["f1"], d["a2"], d["b2"], d["c"], bf16=bf16, train=train, coef_drop=cd,
                  fts_drop=fd, seed=11)
    keep = torch.ones((n, 3, 64), dtype=torch.bool, device=dev)
    keep[_t(listed, dev), 1, :] = False
    assert torch.equal(M.view(torch.int32)[keep], before.view(torch.int32)[keep])
    o = M[:, 1, :].cpu().numpy()
    ratios = {"out": R.ratio(o[listed], r.out[listed], r.e_out[listed])}
    if train:
        for name, t in zip(("lse", "aggp", "tsum"), saved[1:]):
            ratios[name] = R.ratio(t.cpu().numpy()[listed], getattr(r, name)[listed], getattr(r, "e_" + name)[listed])
    _note(R.fwd_cells(K, FP, bf16, False, train, cd, fd), ratios)


@pytest.mark.parametrize("variant", ["plain", "drop", "drop_gid_val"])
@pytest.mark.parametrize("K,FP", R.HEADS)
def test_coefs(dev, K, FP, variant):
    from han_amd import ops
    rowptr, colidx = R.edge_graph()
    n, nt = len(rowptr) - 1, R.EDGE_NT
    d = R.fwd_inputs(K, FP, False, n, nt, "plain", 0.0)
    cd = 0.0 if variant == "plain" else 0.6
    values = R.edge_values(len(colidx)) if variant == "drop_gid_val" else None
    gid_np = ((np.arange(nt, dtype=np.int64) * 5 + 17) % 100_003).astype(np.int32) if variant == "drop_gid_val" else None
    g = _graph(rowptr, colidx, nt, dev, values)
    coef = ops.node_attn_coefs(g, _t(d["f1"], dev), _t(d["f2"], dev), coef_drop=cd, seed=11, row_offset=OFFSET,
                               table_gid=None if gid_np is None else _t(gid_np, dev))
    torch.cuda.synchronize()
    r = R.fwd_ref(rowptr, colidx, d["H"], d["f1"], d["a2"], d["b2"], d["c"], f2=d["f2"], values=values, train=True,
                  coef_drop=cd, seed=11, row_offset=OFFSET, gid=gid_np, path=R.coef_path(np.diff(rowptr)), want_coef=True)
    _note([f"coef<K={K}>"], {"coef": R.ratio(coef.cpu().numpy(), r.coef, r.e_coef)})


def test_every_forward_cell_was_reached(dev):
    want = [c for c in R.CELLS if c.startswith(("fwd", "coef"))]
    seen = {tag for tag, _ in _SEEN}
    assert [c for c in want if c not in seen] == []
    assert all(v <= 1.0 for v in _SEEN.values())
