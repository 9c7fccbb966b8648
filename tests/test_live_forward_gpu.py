"""Forward passes over the rows the loss and the metrics read: han_node_attn_fwd with HAN_FLAG_K2_ROW_SUBSET against the
full launch (bit for bit on the listed rows, a NaN pattern kept everywhere else), han_sem_attn_fwd_live against
han_sem_attn_fwd and the float64 reference of tests/sem_attn_ref.py, han_classifier_loss_live against the
full entry and the float64 reference of tests/loss_opt_ref.py, and HANTrainer(live_forward=True) against
live_forward=False."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import live_forward_cases as lc
from tests import loss_opt_ref as R
from tests import sem_attn_ref as sr

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0A5A5      # a quiet NaN with a recognisable payload
E_UNSUPPORTED = -2


def _pattern(shape, dev):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def _is_pattern(t):
    return bool((t.contiguous().view(torch.int32) == NAN_BITS).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------------------- K2 subset
@functools.lru_cache(maxsize=None)
def _k2_inputs(dev_str, bf16, valued):
    from han_amd.graph import CSRGraph
    dev = torch.device(dev_str)
    rowptr, colidx, vals = lc.k2_graph(dev, valued=valued)
    g = CSRGraph(rowptr, colidx, lc.K2_N, values=vals)
    gen = torch.Generator().manual_seed(7)
    H = (torch.randn((lc.K2_N, 64), generator=gen) * 0.5).to(dev)
    if bf16:
        H = H.to(torch.bfloat16)
    f1 = (torch.randn((lc.K2_N, 8), generator=gen) * 0.5).to(dev)
    a2 = (torch.randn((8, 8), generator=gen) * 0.3).to(dev)
    b2 = (torch.randn((8,), generator=gen) * 0.1).to(dev)
    c = (torch.randn((64,), generator=gen) * 0.1).to(dev)
    return g, H, f1, a2, b2, c


def _k2_call(g, H, f1, a2, b2, c, train, split, flags, f2=None, dense=None):
    """han_node_attn_fwd on outputs pre-filled with the NaN pattern; returns (code, out, lse, aggp, tsum)."""
    from han_amd import _lib, ops
    lib = _lib.load()
    dev, N = H.device, g.n_rows
    out, aggp = _pattern((N, 64), dev), _pattern((N, 64), dev)
    lse, tsum = _pattern((N, 8), dev), _pattern((N, 8), dev)
    tr = (None, lse.data_ptr(), aggp.data_ptr(), tsum.data_ptr()) if train else (None,) * 4
    drop = 0.6 if train else 0.0
    code = lib.han_node_attn_fwd(
        g.rowptr.data_ptr(), g.colidx.data_ptr(), ops._ptr(g.values), H.data_ptr(), ops.DTYPE_CODE[H.dtype], None,
        f1.data_ptr(), ops._ptr(f2), a2.data_ptr(), b2.data_ptr(), c.data_ptr(), None, out.data_ptr(), 64,
        tr[0], tr[1], tr[2], tr[3], N, g.nnz, 8, 8, ops.LEAKY_SLOPE, drop, drop, 1234, None, 0, ops.ACT_ELU,
        flags | (ops.FLAG_XCD_ORDER if g.has_locality() else 0),
        ctypes.byref(split) if split is not None else None, ctypes.byref(dense) if dense is not None else None,
        ops._stream())
    torch.cuda.synchronize()
    return code, out, lse, aggp, tsum


@functools.lru_cache(maxsize=None)
def _k2_full(dev_str, bf16, valued, train):
    """The full launch with the graph's own bins and chunks: computed once per configuration, never modified."""
    from han_amd import ops
    g, H, f1, a2, b2, c = _k2_inputs(dev_str, bf16, valued)
    split, keep = ops._row_split_arg(g, "f")
    assert split.n_short > 0 and split.n_mid > 0 and split.n_long == 2 and split.n_chunks == 8      # all three sets
    r = _k2_call(g, H, f1, a2, b2, c, train, split, 0)
    assert r[0] == 0
    return r[1:]


@pytest.fixture
def k2_split(monkeypatch):
    from han_amd import ops
    monkeypatch.setattr(ops, "SPLIT_DEG", lc.SPLIT_DEG)
    monkeypatch.setattr(ops, "SPLIT_CHUNK", lc.SPLIT_CHUNK)


@pytest.mark.parametrize("which", lc.SUBSETS)
@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("train", [False, True])
def test_k2_subset_rows_have_the_bits_of_the_full_launch(dev, k2_split, train, bf16, valued, which):
    """Listed rows of out (and lse, aggp, tsum in training, both dropouts 0.6) equal the full launch's as int32; every
    other row still holds the NaN pattern the outputs were filled with."""
    from han_amd import ops
    g, H, f1, a2, b2, c = _k2_inputs(str(dev), bf16, valued)
    full = _k2_full(str(dev), bf16, valued, train)
    mask_np = lc.k2_subset(which)
    mask = torch.from_numpy(mask_np).to(dev)
    sub = ops.RowSubset(g, mask)
    split, keep = sub.arg("f")
    short, mid, long = lc.brute_force_sets(lc.k2_degrees(), mask_np, 16, lc.SPLIT_DEG)
    assert (split.n_short, split.n_mid, split.n_long) == (len(short), len(mid), len(long))
    code, *got = _k2_call(g, H, f1, a2, b2, c, train, split, ops.FLAG_K2_ROW_SUBSET)
    assert code == 0
    names = ("out", "lse", "aggp", "tsum") if train else ("out",)
    for name, a, b in zip(names, got, full):
        assert torch.equal(_bits(a[mask]), _bits(b[mask])), f"{name}: listed rows differ from the full launch"
        assert _is_pattern(a[~mask]), f"{name}: a row outside the list was written"
        assert which == "empty" or not bool(torch.isnan(a[mask]).any()), name
    if not train:
        assert all(_is_pattern(t) for t in got[1:])


@pytest.mark.parametrize("train", [False, True])
def test_ops_subset_call_on_a_lean_eligible_graph(dev, monkeypatch, train):
    """256 rows of 80 entries over a 256-row fp32 table: the full call would take the lean (or dense) form; a subset
    call never does, and equals the full call made with ops.LEAN = False.  ops.K2_TIMING prices the listed rows."""
    from han_amd import ops
    from han_amd.graph import CSRGraph
    N, deg = 256, 80
    rng = np.random.default_rng(3)
    cols = np.concatenate([np.sort(rng.choice(N, size=deg, replace=False)) for _ in range(N)]).astype(np.int32)
    g = CSRGraph(torch.arange(0, N * deg + 1, deg, dtype=torch.int64, device=dev), torch.from_numpy(cols).to(dev), N)
    gen = torch.Generator().manual_seed(9)
    H = (torch.randn((N, 64), generator=gen) * 0.5).to(dev)
    f1 = (torch.randn((N, 8), generator=gen) * 0.5).to(dev)
    a2 = (torch.randn((8, 8), generator=gen) * 0.3).to(dev)
    b2 = (torch.randn((8,), generator=gen) * 0.1).to(dev)
    c = (torch.randn((64,), generator=gen) * 0.1).to(dev)
    f2 = ((H.view(N, 8, 8) * a2).sum(-1) + b2).contiguous()
    assert ops._use_lean(g, H)
    drop = 0.6 if train else 0.0
    kw = dict(train=train, coef_drop=drop, fts_drop=drop, seed=77, f2=f2)
    monkeypatch.setattr(ops, "LEAN", False)
    out_full, sv_full = ops.node_attn_fwd(g, H, f1, a2, b2, c, **kw)
    monkeypatch.setattr(ops, "LEAN", True)
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    mask[torch.from_numpy(rng.permutation(N)[:26]).to(dev)] = True
    sub = ops.RowSubset(g, mask)
    out = _pattern((N, 64), dev)
    monkeypatch.setattr(ops, "K2_TIMING", [])
    _, sv = ops.node_attn_fwd(g, H, f1, a2, b2, c, out=out, rows=sub, **kw)
    torch.cuda.synchronize()
    rec = ops.K2_TIMING[0]
    assert rec[0] == ("train" if train else "eval") and rec[3:] == (26, 26 * deg)
    assert torch.equal(_bits(out[mask]), _bits(out_full[mask])) and _is_pattern(out[~mask])
    if train:
        for a, b in zip(sv[1:], sv_full[1:]):
            assert torch.equal(_bits(a[mask]), _bits(b[mask]))
    with pytest.raises(ValueError, match="another graph"):
        ops.node_attn_fwd(g.transpose(), H, f1, a2, b2, c, rows=sub, **kw)


def test_k2_subset_refusals_leave_the_outputs_untouched(dev, k2_split):
    """The flag with HAN_FLAG_LEAN, with a han_dense_t, or with a non-empty bin whose list is NULL: HAN_E_UNSUPPORTED
    before any launch."""
    from han_amd import _lib, ops
    g, H, f1, a2, b2, c = _k2_inputs(str(dev), False, False)
    sub = ops.RowSubset(g, torch.from_numpy(lc.k2_subset("random")).to(dev))
    f2 = ((H.view(-1, 8, 8) * a2).sum(-1) + b2).contiguous()
    split, keep = sub.arg("f")
    bits = torch.zeros((g.n_rows, (g.n_cols + 31) // 32), dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    dense = _lib.HanDense(bits.data_ptr(), bits.shape[1], g.n_cols, ws.data_ptr(), ws.numel())
    no_short, _k1 = sub.arg("f")
    no_short.short_rows = None
    no_mid, _k2 = sub.arg("f")
    no_mid.mid_rows = None
    cases = [("lean", split, ops.FLAG_K2_ROW_SUBSET | ops.FLAG_LEAN, None),
             ("dense", split, ops.FLAG_K2_ROW_SUBSET, dense),
             ("short list NULL", no_short, ops.FLAG_K2_ROW_SUBSET, None),
             ("mid list NULL", no_mid, ops.FLAG_K2_ROW_SUBSET, None)]
    for why, sp, flags, d in cases:
        for train in (False, True):
            code, *outs = _k2_call(g, H, f1, a2, b2, c, train, sp, flags, f2=f2, dense=d)
            assert code == E_UNSUPPORTED, why
            assert all(_is_pattern(t) for t in outs), why
    code, *outs = _k2_call(g, H, f1, a2, b2, c, False, None, ops.FLAG_K2_ROW_SUBSET)      # the flag needs a split
    assert code != 0 and all(_is_pattern(t) for t in outs)


# ------------------------------------------------------------------------------------------------------------ K3 list
K3_N = {4: 16384, 2: 32768, 1: 65536}      # N * P = 65 536: the full entry runs the bf16-pipe kernel, the reference
K3_LISTS = ["0", "1", "16/P-1", "16/P", "16/P+1", "N/10", "N"]


def _k3_ids(N, P, which):
    k = {"0": 0, "1": 1, "16/P-1": 16 // P - 1, "16/P": 16 // P, "16/P+1": 16 // P + 1, "N/10": N // 10, "N": N}[which]
    ids = np.sort(np.random.default_rng(1000 * P + k).permutation(N)[:k])
    if k >= 3:
        ids[0], ids[-1] = 0, N - 1          # the first and the last node
    return np.unique(ids)


@functools.lru_cache(maxsize=None)
def _k3_full(dev_str, N, P, A):
    """Inputs on the device and Z / beta of han_sem_attn_fwd, computed once per shape and never modified."""
    from han_amd import ops
    case = sr.dense_case(N, P, 64, A)
    t = {k: torch.from_numpy(case[k]).to(dev_str) for k in ("M", "w", "b", "u")}
    Z, beta = ops.sem_attn_fwd(t["M"], t["w"], t["b"], t["u"])
    torch.cuda.synchronize()
    return case, t, Z, beta


def _k3_live(t, ids, M=None):
    """han_sem_attn_fwd_live (through ops, which falls back nowhere here) on outputs pre-filled with the NaN pattern."""
    from han_amd import ops
    M = t["M"] if M is None else M
    dev, (N, P, _) = M.device, M.shape
    live = torch.from_numpy(ids.astype(np.int32)).to(dev)
    Z, beta = _pattern((N, 64), dev), _pattern((N, P), dev)
    ops.sem_attn_fwd(M, t["w"], t["b"], t["u"], live=live, out=(Z, beta))
    torch.cuda.synchronize()
    return Z, beta


@pytest.mark.parametrize("which", K3_LISTS)
@pytest.mark.parametrize("A", [64, 128])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_k3_list_rows_have_the_bits_of_the_full_entry(dev, monkeypatch, P, A, which):
    """M holds NaN at every unlisted node.  Listed Z / beta rows are bit-equal to han_sem_attn_fwd on the finite M, and
    unlisted rows keep the pattern.  (The call must reach the row-list entry: the full entry is made unreachable.)"""
    from han_amd import _lib
    N = K3_N[P]
    case, t, Z0, beta0 = _k3_full(str(dev), N, P, A)
    ids = _k3_ids(N, P, which)
    listed = torch.zeros(N, dtype=torch.bool, device=dev)
    listed[torch.from_numpy(ids).to(dev)] = True
    M = torch.where(listed[:, None, None], t["M"], torch.full_like(t["M"], float("nan")))
    lib = _lib.load()

    class NoFull:
        def __getattr__(self, name):
            assert name != "han_sem_attn_fwd", "the row-list entry refused an eligible shape"
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: NoFull())
    Z, beta = _k3_live(t, ids, M)
    assert torch.equal(_bits(Z[listed]), _bits(Z0[listed])) and torch.equal(_bits(beta[listed]), _bits(beta0[listed]))
    assert _is_pattern(Z[~listed]) and _is_pattern(beta[~listed])
    assert not bool(torch.isnan(Z[listed]).any()) and not bool(torch.isnan(beta[listed]).any())


@pytest.mark.parametrize("A", [64, 128])
def test_k3_list_below_the_pipe_bound_against_float64(dev, A):
    """N = 1000, P = 4: the full entry would take the fp32 kernels here, so the reference is tests/sem_attn_ref.py with
    its own bounds.  Two different lists that share rows give those rows the same bits."""
    N, P = 1000, 4
    case = sr.dense_case(N, P, 64, A)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("M", "w", "b", "u")}
    rng = np.random.default_rng(5)
    ids_a = np.sort(rng.permutation(N)[:100])
    ids_b = np.unique(np.concatenate([ids_a[::3], rng.permutation(N)[:37], [0, N - 1]]))      # other neighbours, other tiles
    Za, ba = _k3_live(t, ids_a)
    Zb, bb = _k3_live(t, ids_b)
    W, b, uo = sr._f64(case)
    for ids, Z, beta in ((ids_a, Za, ba), (ids_b, Zb, bb)):
        r = sr._fwd(sr.up(case["M"][ids]), W, b, uo)
        idx = torch.from_numpy(ids).to(dev)
        ratios = {"Z": sr.ratio(Z[idx].cpu().numpy(), r.Z, r.e_Z), "beta": sr.ratio(beta[idx].cpu().numpy(), r.beta, r.e_beta)}
        print(f"A={A} list of {ids.size}:", {k: f"{v:.3g}" for k, v in ratios.items()})
        assert max(ratios.values()) <= 1.0, ratios
        rest = torch.ones(N, dtype=torch.bool, device=dev)
        rest[idx] = False
        assert _is_pattern(Z[rest]) and _is_pattern(beta[rest])
    shared = torch.from_numpy(np.intersect1d(ids_a, ids_b)).to(dev)
    assert shared.numel() >= 30
    assert torch.equal(_bits(Za[shared]), _bits(Zb[shared])) and torch.equal(_bits(ba[shared]), _bits(bb[shared]))


@pytest.mark.parametrize("why,P,D,A,flags", [("P = 3", 3, 64, 128, 0), ("P = 8", 8, 64, 64, 0), ("D = 128", 4, 128, 128, 0),
                                            ("A = 192", 4, 64, 192, 0), ("HAN_FLAG_K3_EXACT_PIPE", 4, 64, 128, 8)])
def test_k3_list_refusals_happen_before_any_launch(dev, why, P, D, A, flags):
    from han_amd import _lib, ops
    lib = _lib.load()
    N = 64
    M = torch.zeros((N, P, D), device=dev)
    w, b, u = torch.zeros((D, A), device=dev), torch.zeros(A, device=dev), torch.zeros(A, device=dev)
    Z, beta = _pattern((N, D), dev), _pattern((N, P), dev)
    live = torch.arange(0, N, 2, dtype=torch.int32, device=dev)
    code = lib.han_sem_attn_fwd_live(M.data_ptr(), w.data_ptr(), b.data_ptr(), u.data_ptr(), Z.data_ptr(), beta.data_ptr(),
                                     live.data_ptr(), live.numel(), N, P, D, A, flags, ops._stream())
    torch.cuda.synchronize()
    assert code == E_UNSUPPORTED, why
    assert _is_pattern(Z) and _is_pattern(beta), why
    assert ops.FLAG_K3_EXACT_PIPE == 8


# ---------------------------------------------------------------------------------------------------- classifier list
CLS_N = 4099
CLS_CELLS = [(64, 3, 2), (64, 4, 1), (128, 7, 3)]      # (D, C, HC)
CLS_LISTS = ["0", "1", "15", "16", "17", "N/10", "N"]


def _cls_ids(which):
    k = {"0": 0, "1": 1, "15": 15, "16": 16, "17": 17, "N/10": CLS_N // 10, "N": CLS_N}[which]
    ids = np.sort(np.random.default_rng(100 + k).permutation(CLS_N)[:k])
    if k >= 15:
        ids[0], ids[-1] = 0, CLS_N - 1      # the first and the last row
    return np.unique(ids)


@functools.lru_cache(maxsize=None)
def _cls_case(D, C, HC):
    return R.dense_case(D, C, HC, CLS_N)


@functools.lru_cache(maxsize=None)
def _cls_full(dev_str, D, C, HC):
    """The full entry on a Z that is finite everywhere: logits and dZ, computed once."""
    from han_amd import ops
    case = _cls_case(D, C, HC)
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev_str) for k in ("Z", "Wc", "bc", "labels", "mask")}
    logits, _, grads = ops.classifier_loss(t["Z"], t["Wc"], t["bc"], t["labels"], t["mask"], case["row_weight"], backward=True)
    torch.cuda.synchronize()
    return t, logits, grads[0]


@pytest.mark.parametrize("which", CLS_LISTS)
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("D,C,HC", CLS_CELLS)
def test_classifier_over_a_row_list(dev, D, C, HC, backward, which):
    """Z holds NaN at every unlisted row.  logits / dZ of the listed rows are the bits of the full entry on the finite Z,
    the other rows keep the pattern; loss, accuracy, dWc and dbc against the float64 reference over the listed rows
    (mask still applied per row) within the bounds of tests/loss_opt_ref.py; everything finite."""
    from han_amd import _lib, ops
    lib = _lib.load()
    case = _cls_case(D, C, HC)
    t, logits_full, dZ_full = _cls_full(str(dev), D, C, HC)
    ids = _cls_ids(which)
    listed_np = np.zeros(CLS_N, dtype=bool)
    listed_np[ids] = True
    listed = torch.from_numpy(listed_np).to(dev)
    live = torch.from_numpy(ids.astype(np.int32)).to(dev)
    Z = torch.where(listed[:, None], t["Z"], torch.full_like(t["Z"], float("nan")))
    logits, dZ = _pattern((CLS_N, C), dev), _pattern((CLS_N, D), dev)
    loss_acc = _pattern((2,), dev)
    dWc, dbc = _pattern((HC, D, C), dev), _pattern((HC, C), dev)
    ws = torch.empty(lib.han_classifier_workspace(CLS_N, D, C, HC), dtype=torch.uint8, device=dev)
    ws.view(torch.int32)[:ws.numel() // 4].fill_(NAN_BITS)
    code = lib.han_classifier_loss_live(
        Z.data_ptr(), t["Wc"].data_ptr(), t["bc"].data_ptr(), t["labels"].data_ptr(), t["mask"].data_ptr(),
        float(case["row_weight"]), logits.data_ptr(), loss_acc.data_ptr(), dZ.data_ptr() if backward else None,
        dWc.data_ptr() if backward else None, dbc.data_ptr() if backward else None, ws.data_ptr(), ws.numel(),
        ops._ptr_nonempty(live), live.numel(), CLS_N, D, C, HC, ops._stream())
    torch.cuda.synchronize()
    assert code == 0
    assert torch.equal(_bits(logits[listed]), _bits(logits_full[listed])) and _is_pattern(logits[~listed])
    if backward:
        assert torch.equal(_bits(dZ[listed]), _bits(dZ_full[listed])) and _is_pattern(dZ[~listed])
    else:
        assert _is_pattern(dZ) and _is_pattern(dWc) and _is_pattern(dbc)
    ref = R.classifier_ref(case["Z"], case["Wc"], case["bc"], case["labels"],
                           (case["mask"] != 0) & listed_np, case["row_weight"])
    la = loss_acc.cpu().numpy()
    ratios = {"loss": R.ratio(float(la[0]), ref.loss, ref.e_loss)}
    a = float(la[1])
    ratios["acc"] = R.ratio(a, min(max(a, ref.acc_lo), ref.acc_hi), ref.e_acc)
    if backward:
        ratios["dWc"] = R.ratio(dWc.cpu().numpy(), ref.dWc, ref.e_dWc)
        ratios["dbc"] = R.ratio(dbc.cpu().numpy(), ref.dbc, ref.e_dbc)
        assert bool(torch.isfinite(dWc).all()) and bool(torch.isfinite(dbc).all()) and bool(torch.isfinite(dZ[listed]).all())
    print(f"D={D} C={C} HC={HC} backward={backward} list={which}:", {k: f"{v:.3g}" for k, v in ratios.items()})
    assert np.isfinite(la).all() and bool(torch.isfinite(logits[listed]).all())
    assert max(ratios.values()) <= 1.0, ratios
    if which == "0":
        assert la[0] == 0.0 and la[1] == 0.0
        assert not backward or (not bool(dWc.any()) and not bool(dbc.any()))


def test_classifier_list_through_ops_and_its_refusals(dev):
    """ops.classifier_loss(live=...) gives what the entry gives; the three-kernel shapes are refused before any launch."""
    from han_amd import _lib, ops
    D, C, HC = 64, 3, 2
    case = _cls_case(D, C, HC)
    t, logits_full, dZ_full = _cls_full(str(dev), D, C, HC)
    live = torch.from_numpy(_cls_ids("N/10").astype(np.int32)).to(dev)
    idx = live.long()
    logits, la, grads = ops.classifier_loss(t["Z"], t["Wc"], t["bc"], t["labels"], t["mask"], case["row_weight"],
                                            backward=True, live=live)
    assert torch.equal(_bits(logits[idx]), _bits(logits_full[idx])) and torch.equal(_bits(grads[0][idx]), _bits(dZ_full[idx]))
    assert bool(torch.isfinite(la).all())
    lib = _lib.load()
    for Dx, Cx in ((192, 3), (64, 65)):
        Z = _pattern((CLS_N, Dx), dev)
        Wc, bc = torch.zeros((1, Dx, Cx), device=dev), torch.zeros((1, Cx), device=dev)
        lg, la2 = _pattern((CLS_N, Cx), dev), _pattern((2,), dev)
        ws = torch.empty(max(lib.han_classifier_workspace(CLS_N, Dx, Cx, 1), 4), dtype=torch.uint8, device=dev)
        code = lib.han_classifier_loss_live(Z.data_ptr(), Wc.data_ptr(), bc.data_ptr(), t["labels"].data_ptr(),
                                            t["mask"].data_ptr(), 1.0, lg.data_ptr(), la2.data_ptr(), None, None, None,
                                            ws.data_ptr(), ws.numel(), live.data_ptr(), live.numel(), CLS_N, Dx, Cx, 1,
                                            ops._stream())
        torch.cuda.synchronize()
        assert code == E_UNSUPPORTED and _is_pattern(lg) and _is_pattern(la2)


# ------------------------------------------------------------------------------------------------------------ trainer
_cache = {}


def _workload(dev):
    if "wl" not in _cache:
        from han_amd import synth
        N = 16384
        wl = synth.planted_partition(N, 4, 4, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=dev)
        _cache["wl"] = (wl, torch.rand(N, generator=torch.Generator().manual_seed(1)))
    return _cache["wl"]


def _masks(u, frac, dev):
    return (u < frac).to(torch.uint8).to(dev), ((u >= frac) & (u < frac + 0.1)).to(torch.uint8).to(dev)


def _trainer(dev, wl, masks, **kw):
    from han_amd import rng as hrng
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    torch.manual_seed(0)
    hrng.manual_seed(5)
    model = HeteGAT_multi().build(4, 64, 4, kw.pop("hid", (8,)), kw.pop("heads", (8, 1)), 128,
                                  device=kw.pop("model_dev", dev), generator=torch.Generator().manual_seed(11))
    return model, HANTrainer(model, [wl["x"]] * 4, wl["graphs"], wl["labels"], masks[0], masks[1], **kw)


def _three_epochs(dev, monkeypatch, seen, **kw):
    """Three epochs from the seeds every run shares; `seen` receives (train, listed row count or None) per K2 launch."""
    wl, u = _workload(dev)
    seen.clear()
    seen.k3.clear()
    model, tr = _trainer(dev, wl, _masks(u, 0.1, dev), **kw)
    for _ in range(3):
        out = tr.epoch()
    torch.cuda.synchronize()
    return model, tr, model.flat.clone(), model.flat_grad.clone(), [float(v) for v in out]


@pytest.fixture
def k2_launches(monkeypatch):
    from han_amd import ops
    class Seen(list):      # the K2 launches; .k3: the listed row count (or None) of every K3 forward
        k3 = []

    seen, fwd = Seen(), ops.node_attn_fwd
    seen.k3 = []

    def keep(graph, *a, **k):
        rows = k.get("rows")
        seen.append((bool(k.get("train")), None if rows is None else rows.subset(graph).n_rows))
        return fwd(graph, *a, **k)

    monkeypatch.setattr(ops, "node_attn_fwd", keep)
    k3 = ops.sem_attn_fwd

    def keep_k3(M, *a, **k):
        live = k.get("live")
        seen.k3.append(None if live is None else int(live.numel()))
        return k3(M, *a, **k)

    monkeypatch.setattr(ops, "sem_attn_fwd", keep_k3)
    return seen


def _param_and_grad_gap(model, a, b):
    (pa, ga), (pf, gf) = a, b
    dp = float((pa - pf).abs().max())
    off, worst = 0, 0.0
    for name, shp in model.param_shapes():
        n = int(np.prod(shp))
        d, m = float((ga[off:off + n] - gf[off:off + n]).abs().max()), float(gf[off:off + n].abs().max())
        off += n
        print(f"  grad {name}: max diff {d:.3e} of {m:.3e}")
        worst = max(worst, d / max(m, 1e-30))
    print(f"max |param diff| {dp:.3e} of {float(pf.abs().max()):.3e}; worst gradient slice {worst:.3e}")
    return dp, worst


def test_three_epochs_live_forward_against_the_full_forward(dev, monkeypatch, k2_launches):
    """The r21 workload (N = 16384, P = 4, masks 10 % / 10 %), three epochs from equal seeds, live_backward on in both
    runs.  Parameters within 2e-4 and each gradient slice within 2e-4 of its largest entry (the three-step tolerance of
    DESIGN.md section 6, as test_three_epochs_live_against_full); all four scalars finite, the validation pair to 1e-5
    relative.  Every K2 launch of the live run covers exactly the listed rows of its pass.  Then the fall-backs: with
    use_graph=True, masked_backward=True and after set_masked_backward(True) the training forward computes every row
    and the eval forward stays on the val list."""
    seen = k2_launches
    model, tr, p0, g0, s0 = _three_epochs(dev, monkeypatch, seen, live_forward=False, live_backward=True)
    assert not tr.live_forward and all(n is None for _, n in seen) and len(seen) == 24
    assert seen.k3 == [None] * 6
    model, tr, p1, g1, s1 = _three_epochs(dev, monkeypatch, seen, live_forward=True, live_backward=True)
    n_train, n_val = int(tr.train_mask.sum()), int(tr.val_mask.sum())
    assert tr.live_forward and len(seen) == 24
    assert all(n == (n_train if train else n_val) for train, n in seen), seen
    assert seen.k3 == [n_train, n_val] * 3      # K3 runs over the list of its pass
    assert all(np.isfinite(s1)) and all(np.isfinite(s0))
    print("scalars", s0, s1)
    dp, worst = _param_and_grad_gap(model, (p1, g1), (p0, g0))
    assert bool(torch.isfinite(p1).all()) and bool(g1.abs().max() > 0)
    assert dp < 2e-4 and worst < 2e-4
    assert abs(s1[2] - s0[2]) <= 1e-5 * abs(s0[2]) and abs(s1[3] - s0[3]) <= 1e-5 * abs(s0[3])
    # eval_step with another mask: the full forward
    seen.clear()
    tr.eval_step(mask=tr.train_mask, weight=tr.w_train)
    assert [n for _, n in seen] == [None] * 4
    # the masked backward, switched on afterwards: the training forward goes back to every row
    seen.clear()
    tr.set_masked_backward(True)
    tr.epoch()
    assert [n for t, n in seen if t] == [None] * 4 and [n for t, n in seen if not t] == [n_val] * 4
    for kw in (dict(use_graph=True), dict(masked_backward=True)):
        # (a captured epoch draws its dropout from the device seed word: the full run of the same kind is the reference)
        _, tr, pf, _, _ = _three_epochs(dev, monkeypatch, seen, live_forward=False, live_backward=True, **kw)
        assert not tr.live_forward and all(n is None for _, n in seen)
        model, tr, p2, g2, s2 = _three_epochs(dev, monkeypatch, seen, live_forward=True, live_backward=True, **kw)
        assert tr.live_forward
        if not kw.get("use_graph"):
            assert len(seen) == 24
        assert seen and all(n == (None if train else n_val) for train, n in seen), (kw, seen)
        assert seen.k3 and seen.k3[::2] == [None] * (len(seen.k3) // 2) and seen.k3[1::2] == [n_val] * (len(seen.k3) // 2)
        dp2 = float((p2 - pf).abs().max())
        print(kw, f"max |param diff| against the full run {dp2:.3e}")
        assert dp2 < 2e-4 and all(np.isfinite(s2))


def test_auto_and_the_conditions_of_the_live_forward(dev, monkeypatch):
    """`auto` is off at 16384 rows and on once LIVE_FORWARD_MIN_ROWS is patched down (patching the backward's bound does
    not switch it on); off for a 60 % mask, a second layer or a CPU model, for each of which True raises."""
    from han_amd import trainer
    wl, u = _workload(dev)
    assert trainer.LIVE_FORWARD_MIN_ROWS > 16384
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev))
    assert not tr.live_forward and tr._live_fwd_train is None
    monkeypatch.setattr(trainer, "LIVE_BACKWARD_MIN_ROWS", 16384)
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev))
    assert tr.live_backward and not tr.live_forward and tr._live_fwd_train is None
    monkeypatch.setattr(trainer, "LIVE_FORWARD_MIN_ROWS", 16384)
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev))
    assert tr.live_forward and tr._live_fwd_train is not None
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev), live_backward=False)      # no row-list fold: the eval forward only
    assert tr.live_forward and tr._live_fwd_train is None
    _, tr = _trainer(dev, wl, _masks(u, 0.1, dev), live_forward=False)
    assert not tr.live_forward and tr._live_fwd_train is None
    m = _masks(u, 0.1, dev)
    _, tr = _trainer(dev, wl, (m[0], m[0]))      # one tensor for both masks: one set of row lists
    assert tr.live_forward and tr._live_fwd_train._subsets is tr._live_fwd[id(tr.val_mask)][1]._subsets
    wide = ((u < 0.1).to(torch.uint8).to(dev), (u >= 0.4).to(torch.uint8).to(dev))      # a 60 % val mask
    _, tr = _trainer(dev, wl, wide)
    assert not tr.live_forward
    model, tr = _trainer(dev, wl, _masks(u, 0.1, dev), hid=(8, 8), heads=(8, 8, 1))
    assert model.extra and not tr.live_forward
    with pytest.raises(ValueError, match="live_forward"):
        _trainer(dev, wl, wide, live_forward=True)
    with pytest.raises(ValueError, match="live_forward"):
        _trainer(dev, wl, _masks(u, 0.1, dev), live_forward=True, hid=(8, 8), heads=(8, 8, 1))
    with pytest.raises(ValueError, match="live_forward"):
        _trainer(dev, wl, _masks(u, 0.1, dev), live_forward="yes")


def test_a_cpu_model_keeps_the_full_forward(dev, monkeypatch):
    """A model on the host (the CPU stand-in backend of the host tests): `auto` stays off at any size, True raises."""
    from han_amd import synth, trainer
    monkeypatch.setattr(trainer, "LIVE_FORWARD_MIN_ROWS", 1)
    cpu = torch.device("cpu")
    wl = synth.planted_partition(256, 4, 4, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=cpu)
    u = torch.rand(256, generator=torch.Generator().manual_seed(1))
    _, tr = _trainer(cpu, wl, _masks(u, 0.1, cpu), live_backward=False)
    assert not tr.live_forward and tr._live_fwd_train is None
    with pytest.raises(ValueError, match="live_forward"):
        _trainer(cpu, wl, _masks(u, 0.1, cpu), live_backward=False, live_forward=True)
