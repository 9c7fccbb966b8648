"""GPU tests of han_classifier_multilabel (han_amd/csrc/loss_opt.hip, multilabel_body.h) through han_amd.ops: the fused
classifier + masked sigmoid cross-entropy + micro-F1 in its three kernel forms -- 16 lanes per row (C <= 16, unrolled
to 4 / 8 / 16), class per lane (C <= 64), the any-shape row kernel followed by cls_dw_kernel -- and the row-list form
of the fused ones.

Every comparison is elementwise |gpu - float64| <= e with the bound e of tests/multilabel_ref.py (counts of fp32
roundings, derived there; tests/test_multilabel_host.py checks the reference and the inputs without a GPU), exact
where the arithmetic is exact: the counts tp / fp / fn always (the shared inputs hold no undecided prediction), dZ
outside the mask, the bits of a row between the full and the row-list form.

The last section drives the objective through the model: HANTrainer(objective="sigmoid") against the torch-autograd
oracle the way tests/test_gpu_parity.py drives the softmax trainer, live forward on / off, a captured epoch against
the eager one, and MiniBatchTrainer against the full graph on the seeds of a block.

Largest err / bound measured on an MI355X (gfx950), per kernel instance over all of its cases in this file (the counts
and micro-F1 were equal everywhere); the planted cases alone are in profiles/r27_multilabel_parity_ratios.json:

    kernel                                   logits   loss     dZ       dWc      dbc
    multilabel_kernel<CM=4,NV=1>             0.027    0.0016   0.070    0.0064   0.0014
    multilabel_kernel<CM=8,NV=1>             0.020    0.0013   0.014    0.012    0.0049
    multilabel_kernel<CM=16,NV=2>            0.0065   0.00001  0.0027   0.0018   0.0016
    multilabel_wide_kernel<NV=1>             0.066    0.0008   0.033    0.0077   0.0034
    multilabel_wide_kernel<NV=2>             0.036    0.0010   0.0080   0.045    0.032
    multilabel_live_kernel<CM=4|8|16>        0.012    0.0015   0.039    0.0054   0.0018
    multilabel_wide_live_kernel<NV=1|2>      0.040    0.0007   0.014    0.0094   0.0044
    ml_gen_kernel<NV=4>+cls_dw_kernel        0.030    0.0016   0.081    0.011    0.0045
    ml_gen_kernel<NV=8>+cls_dw_kernel        0.0017   0.0002   0.0009   0.0039   0.0009
    ml_gen_kernel<NV=0>+cls_dw_kernel        0.0004   0.00003  0.0011   0.0001   0.00007

One check is stated more narrowly than "sigma saturates to exactly 0 or 1 at +-80 and +-1e4": at -80 fp32 holds
exp(-80) = 2^-115.4 as a normal number and sigma = e / (1 + e) returns it, so test_saturated_logits demands exactly 1
at +80 and +1e4, exactly 0 at -1e4, and at -80 a gradient of at most 2^-115 per class.
"""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import multilabel_ref as R

pytestmark = pytest.mark.gpu

_SEEN = {}


def _note(tag, ratios):
    for k, v in ratios.items():
        _SEEN[(tag, k)] = max(_SEEN.get((tag, k), 0.0), v)
    print(tag, {k: f"{v:.3g}" for k, v in ratios.items()})


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the largest err / bound per kernel and quantity when the module is done (pytest -s); HAN_RATIO_JSON names
    a file that receives the same table."""
    yield
    for (tag, k), v in sorted(_SEEN.items()):
        print(f"{tag:50s} {k:7s} {v:.3g}")
    path = os.environ.get("HAN_RATIO_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({f"{tag} | {k}": v for (tag, k), v in sorted(_SEEN.items())}, f, indent=1)


def _gpu(case, dev, Z=None):
    from han_amd import ops
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("Z", "Wc", "bc", "mask")}
    if Z is not None:
        t["Z"] = torch.from_numpy(np.ascontiguousarray(Z)).to(dev)
    t["bits"] = ops.pack_label_bits(torch.from_numpy(case["y"]).to(dev))
    assert np.array_equal(t["bits"].cpu().numpy().view(np.uint64), R.pack_bits(case["y"]))
    return t


def _poison_workspace(dev):
    """NaN bytes over the scratch buffer of the entry (ops._ws tag "clsml"), when it exists already."""
    from han_amd import ops
    ws = ops._workspaces.get((str(dev), "clsml"))
    if ws is not None:
        ws.fill_(0xFF)


def _run(t, row_weight, backward, live=None, poison=True):
    from han_amd import ops
    if poison:
        _poison_workspace(t["Z"].device)
    return ops.classifier_multilabel(t["Z"], t["Wc"], t["bc"], t["bits"], t["mask"], row_weight, backward=backward,
                                     live=live)


def _raw_call(t, case, D, C, HC, ws=None, poison_ws=False):
    """han_classifier_multilabel with the backward, every row, through ctypes: logits, loss_acc, counts, dZ, dWc and dbc
    are filled with NaN bytes before the call (ops hands out fresh tensors, which cannot be poisoned), the workspace too
    when asked.  Returns (logits, loss_acc, counts, (dZ, dWc, dbc), workspace)."""
    from han_amd import _lib
    lib = _lib.load()
    dev, N = t["Z"].device, t["Z"].shape[0]

    def nan_bytes(shape, dtype=torch.float32):
        x = torch.empty(shape, dtype=dtype, device=dev)
        x.view(torch.uint8).fill_(0xFF)
        return x
    logits, la, counts = nan_bytes((N, C)), nan_bytes((2,)), nan_bytes((3,), torch.int64)
    dZ, dWc, dbc = nan_bytes((N, D)), nan_bytes(tuple(t["Wc"].shape)), nan_bytes(tuple(t["bc"].shape))
    if ws is None:
        ws = torch.empty(lib.han_classifier_multilabel_workspace(N, D, C, HC), dtype=torch.uint8, device=dev)
    if poison_ws:
        ws.fill_(0xFF)
    _lib.check(lib.han_classifier_multilabel(
        t["Z"].data_ptr(), t["Wc"].data_ptr(), t["bc"].data_ptr(), t["bits"].data_ptr(), t["mask"].data_ptr(),
        float(case["row_weight"]), logits.data_ptr(), la.data_ptr(), counts.data_ptr(), dZ.data_ptr(), dWc.data_ptr(),
        dbc.data_ptr(), ws.data_ptr(), ws.numel(), None, 0, N, D, C, HC, torch.cuda.current_stream().cuda_stream))
    return logits, la, counts, (dZ, dWc, dbc), ws


def _np(out):
    logits, la, counts, grads = out
    return (logits.cpu().numpy(), la.cpu().numpy(), counts.cpu().numpy(),
            None if grads is None else tuple(g.cpu().numpy() for g in grads))


def _check(ref, out, tag, rows=None):
    logits, la, counts, grads = _np(out)
    ratios = R.multilabel_ratios(ref, logits, la, grads, rows=rows)
    _note(tag, ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert ref.undecided == 0
    assert counts.dtype == np.int64 and np.array_equal(counts, ref.counts), (counts, ref.counts)
    assert R.f1_matches(la[1], ref), (la[1], ref.f1)
    if grads is not None and rows is None:
        assert not grads[0][~ref.live].any(), "dZ of a row outside the mask must be exactly 0"
    return logits, la, counts, grads


@functools.lru_cache(maxsize=2)
def _planted(D, C, HC):
    case = R.planted_case(D, C, HC)
    return case, R.multilabel_ref(**case)


@functools.lru_cache(maxsize=4)
def _dense(D, C, HC, N):
    case = R.dense_case(D, C, HC, N)
    return case, R.multilabel_ref(**case)


# ------------------------------------------------------------------------------------------------ 1, 2: parity
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("D,C,HC", R.CELLS)
def test_planted_rows_past_the_loop(dev, D, C, HC, backward):
    """One grid-stride pass plus 77 rows: logits on every row, loss / dZ / dWc / dbc within bounds over the 48 planted
    rows (first, last, second pass), dZ exactly 0 elsewhere (large finite junk there), counts exact."""
    case, ref = _planted(D, C, HC)
    _check(ref, _run(_gpu(case, dev), case["row_weight"], backward), R.kernel_name(D, C))


@pytest.mark.parametrize("N", R.SMALL_N)
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("D,C,HC", R.SMALL_CELLS)
def test_small_n_dense_mask(dev, D, C, HC, backward, N):
    """Partial blocks, partial groups, a single row; half of the rows live."""
    case, ref = _dense(D, C, HC, N)
    _check(ref, _run(_gpu(case, dev), case["row_weight"], backward), R.kernel_name(D, C))


# ------------------------------------------------------------------------------------------------ 3: the row list
@pytest.mark.parametrize("backward", [False, True])
@pytest.mark.parametrize("D,C,HC", R.FUSED)
def test_row_list_form(dev, D, C, HC, backward):
    """Z is NaN outside the list: listed logits / dZ rows carry the bits of the full call on the defined Z, unlisted rows
    keep the poison they held, the sums are within bounds and the counts exact."""
    from han_amd import _lib, ops
    case, _ = _planted(D, C, HC)
    rows, Zn = R.live_list(case)
    ref = R.multilabel_ref(**{**case, "Z": Zn}, rows=rows)
    full = _np(_run(_gpu(case, dev), case["row_weight"], backward))
    t = _gpu(case, dev, Z=Zn)
    live = torch.from_numpy(rows).to(dev)
    # the entry through ctypes, so that the outputs can be poisoned beforehand (ops hands out fresh tensors)
    lib = _lib.load()
    N = Zn.shape[0]
    poison = 123456.0
    logits = torch.full((N, C), poison, device=dev)
    dZ = torch.full((N, D), poison, device=dev)
    la = torch.full((2,), float("nan"), device=dev)
    counts = torch.full((3,), -1, dtype=torch.int64, device=dev)
    dWc, dbc = torch.full_like(t["Wc"], float("nan")), torch.full_like(t["bc"], float("nan"))
    ws = torch.full((lib.han_classifier_multilabel_workspace(N, D, C, HC),), 0xFF, dtype=torch.uint8, device=dev)
    g = (dZ.data_ptr(), dWc.data_ptr(), dbc.data_ptr()) if backward else (None, None, None)
    _lib.check(lib.han_classifier_multilabel(
        t["Z"].data_ptr(), t["Wc"].data_ptr(), t["bc"].data_ptr(), t["bits"].data_ptr(), t["mask"].data_ptr(),
        float(case["row_weight"]), logits.data_ptr(), la.data_ptr(), counts.data_ptr(), g[0], g[1], g[2], ws.data_ptr(),
        ws.numel(), live.data_ptr(), rows.size, N, D, C, HC, torch.cuda.current_stream().cuda_stream))
    out = (logits, la, counts, (dZ, dWc, dbc) if backward else None)
    logits, la, counts, grads = _check(ref, out, R.kernel_name(D, C).replace("_kernel", "_live_kernel", 1), rows=rows)
    off = np.ones(N, dtype=bool)
    off[rows] = False
    assert np.array_equal(logits[rows].view(np.uint32), full[0][rows].view(np.uint32))
    assert (logits[off] == poison).all()
    if backward:
        assert np.array_equal(grads[0][rows].view(np.uint32), full[3][0][rows].view(np.uint32))
        assert (grads[0][off] == poison).all()
        assert not grads[0][rows][case["mask"][rows] == 0].any()
    # the same through ops (fresh outputs): identical results
    again = _np(ops.classifier_multilabel(t["Z"], t["Wc"], t["bc"], t["bits"], t["mask"], case["row_weight"],
                                          backward=backward, live=live))
    assert np.array_equal(again[1].view(np.uint32), la.view(np.uint32)) and np.array_equal(again[2], counts)


@pytest.mark.parametrize("backward", [False, True])
def test_empty_row_list(dev, backward):
    """n_live == 0: zeros for the loss, the counts and the parameter gradients, NaN for micro-F1, nothing else touched."""
    case, _ = _dense(64, 8, 2, 17)
    t = _gpu(case, dev, Z=np.full_like(case["Z"], np.nan))
    logits, la, counts, grads = _np(_run(t, case["row_weight"], backward, live=torch.empty(0, dtype=torch.int32, device=dev)))
    assert la[0] == 0 and math.isnan(la[1]) and not counts.any()
    if backward:
        assert not grads[1].any() and not grads[2].any()


# ------------------------------------------------------------------------------------------------ 4: edges
@pytest.mark.parametrize("D,C,HC", [(64, 4, 1), (64, 32, 2), (192, 4, 1)])
def test_zero_row_gives_log2(dev, D, C, HC):
    case = R.zero_case(D, C, HC)
    ref = R.multilabel_ref(**case)
    for backward in (False, True):
        logits, la, counts, _ = _check(ref, _run(_gpu(case, dev), 1.0, backward), R.kernel_name(D, C))
        assert not logits[0].any(), "a row of zeros with zero bias: logits exactly 0"
        assert abs(float(la[0]) - math.log(2.0)) <= ref.e_loss
        assert counts[0] == 0 and counts[1] == 0 and counts[2] == int(case["y"][0].sum()), "sigma(0) = 1/2 predicts 0"
        assert math.isnan(la[1]), "tp == 0: micro-F1 is the reference's 0 / 0"


@pytest.mark.parametrize("s", [80.0, 1.0e4])
@pytest.mark.parametrize("D,C", [(64, 4), (128, 32), (192, 4)])
def test_saturated_logits(dev, D, C, s):
    """Logits of exactly +-s: nothing overflows; sigma is exactly 1 on the positive side and exactly 0 at -1e4.  At -80
    fp32 holds exp(-80) = 2^-115.4, a normal number, and sigma = e / (1 + e) returns it: there the gradient is
    bounded by it instead (a form that returned 0 would be the less accurate one)."""
    case = R.saturation_case(D, C, s)
    ref = R.multilabel_ref(**case)
    logits, la, counts, grads = _check(ref, _run(_gpu(case, dev), case["row_weight"], True), R.kernel_name(D, C))
    assert np.array_equal(np.abs(logits), np.full_like(logits, s))
    assert np.isfinite(la[0]) and all(np.isfinite(g).all() for g in grads)
    dz0 = grads[0][:, 0].astype(np.float64)
    wc = 0.125 / C
    # labels == predictions: sigma - y is 0 (positive logits; negative ones at 1e4) or exp(-80)
    assert np.abs(dz0[0::4]).max() <= (0.0 if s > 100 else C * wc * 2.0 ** -115)
    # the opposite labels: sigma - y is exactly +-1 on both sides, C terms of w / C, all exact
    assert np.array_equal(dz0[1::4], np.full(dz0[1::4].shape, C * wc))
    assert not grads[0][:, 1:].any()
    # all-zero label rows predict C / 2 classes falsely, all-one rows miss C / 2
    n = logits.shape[0] // 4 * C      # two of the four kinds of row add C / 2 to each count
    assert np.array_equal(counts, [n, n, n])


@pytest.mark.parametrize("D,C,HC", [(64, 8, 2), (128, 33, 1), (320, 17, 3)])
def test_no_label_set_gives_nan_f1(dev, D, C, HC):
    case, _ = _dense(D, C, HC, 65)
    case = {**case, "y": np.zeros_like(case["y"])}
    ref = R.multilabel_ref(**case)
    assert ref.tp == 0 and ref.fn == 0 and ref.fp > 0 and ref.undecided == 0
    _, la, _, _ = _check(ref, _run(_gpu(case, dev), case["row_weight"], True), R.kernel_name(D, C))
    assert math.isnan(la[1])


# ------------------------------------------------------------------------------------------------ 5: exact counts
def test_counts_are_exact_past_2_24(dev):
    """tp = 266 401 * 63 = 16 783 263: odd and above 2^24, which no fp32 accumulation can produce."""
    from han_amd import ops
    N, C = R.BIG_N, R.BIG_C
    Z = torch.zeros((N, 64), device=dev)
    Wc = torch.zeros((1, 64, C), device=dev)
    bc = torch.full((1, C), 0.5, device=dev)
    bits = ops.pack_label_bits(torch.ones((N, C), dtype=torch.uint8, device=dev))
    mask = torch.ones(N, dtype=torch.uint8, device=dev)
    for backward in (False, True):
        _, la, counts, _ = ops.classifier_multilabel(Z, Wc, bc, bits, mask, 1.0 / N, backward=backward)
        assert counts.tolist() == [R.BIG_TP, 0, 0]
        assert float(la[1]) == 1.0
        assert abs(float(la[0]) - math.log1p(math.exp(-0.5))) < 1e-4


# ------------------------------------------------------------------------------------------------ 6: determinism, scratch
@pytest.mark.parametrize("D,C,HC", R.SMALL_CELLS)
def test_deterministic_and_scratch_independent(dev, D, C, HC):
    """The entry through ctypes with every output and the workspace full of NaN bytes beforehand, twice, and once more on
    the scratch the call before left: bit-equal outputs, within the bounds, nothing of the poison left."""
    case, ref = _planted(D, C, HC)
    t = _gpu(case, dev)
    a = _raw_call(t, case, D, C, HC, poison_ws=True)
    b = _raw_call(t, case, D, C, HC, poison_ws=True)
    ws = a[4]
    c = _raw_call(t, case, D, C, HC, ws=ws)            # the scratch now holds the first call's slabs
    _check(ref, a[:4], R.kernel_name(D, C))
    for other in (b, c):
        for x, y in zip((a[0], a[1], a[2]) + a[3], (other[0], other[1], other[2]) + other[3]):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert all(bool(torch.isfinite(x).all()) for x in (a[0], a[1]) + a[3])


@pytest.mark.parametrize("D,C,HC", R.SMALL_CELLS)
def test_error_codes(dev, D, C, HC):
    from han_amd import _lib
    lib = _lib.load()
    case, _ = _dense(D, C, HC, 17)
    t = _gpu(case, dev)
    N = 17
    need = lib.han_classifier_multilabel_workspace(N, D, C, HC)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    logits = torch.full((N, C), 7.0, device=dev)
    la = torch.full((2,), 7.0, device=dev)
    counts = torch.full((3,), 7, dtype=torch.int64, device=dev)
    live = torch.arange(N, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(D_=D, ws_bytes=need, dZ=None, live_=None, n_live=0, bits=t["bits"].data_ptr()):
        return lib.han_classifier_multilabel(
            t["Z"].data_ptr(), t["Wc"].data_ptr(), t["bc"].data_ptr(), bits, t["mask"].data_ptr(), 1.0,
            logits.data_ptr(), la.data_ptr(), counts.data_ptr(), dZ, None, None, ws.data_ptr(), ws_bytes, live_, n_live,
            N, D_, C, HC, st)
    assert call(ws_bytes=need - 1) == -3                       # HAN_E_WORKSPACE
    assert call(D_=D + 32) == -2                               # HAN_E_UNSUPPORTED
    assert call(bits=None) == -1                               # HAN_E_BADARG
    assert call(dZ=ws.data_ptr()) == -1                        # dZ without dWc / dbc
    assert call(live_=live.data_ptr(), n_live=N + 1) == -1
    assert call(live_=live.data_ptr(), n_live=-1) == -1
    if R.family(D, C) == "gen":
        assert call(live_=live.data_ptr(), n_live=N) == -2     # the row list: the fused shapes only
    torch.cuda.synchronize()
    assert (logits == 7.0).all() and (la == 7.0).all() and (counts == 7).all(), "a refused call writes nothing"
    assert call() == 0


# ------------------------------------------------------------------------------------------------ 7: through the model
def _model_problem(seed=27, n=2000, f=16, c=5):
    """N = 2000, P = 2, 8 x 8 heads, C = 5: the suite's seeded problem with multi-hot labels drawn beside it."""
    from tests.helpers import make_problem
    prob = make_problem(seed, n, f, 2, c, [0.002, 0.01])
    prob["y"] = (np.random.default_rng([seed, 5]).random((n, c)) < 0.4).astype(np.uint8)
    return prob


def _oracle_epoch(xs, graphs, bp, state, y, train_mask, val_mask, keep, masks):
    """oracle.han_oracle_torch.train_epoch with the multi-label pair of han_amd.base_gattn (float64 torch)."""
    from han_amd.base_gattn import BaseGAttN
    from oracle import han_oracle_torch as ht
    for k in ht.PARAM_ORDER:
        bp[k].requires_grad_(True)
        bp[k].grad = None
    logits, _, _ = ht.hetegat_forward(xs, graphs, bp, keep_in=keep, keep_coef=keep, masks=masks)
    data_loss = BaseGAttN.masked_sigmoid_cross_entropy(logits, y, train_mask)
    loss = data_loss + ht.l2_all(bp, 0.001)
    loss.backward()
    grads = {k: bp[k].grad for k in ht.PARAM_ORDER}
    for k in ht.PARAM_ORDER:
        bp[k].requires_grad_(False)
    ht.adam_step_tf_(bp, grads, state, lr=0.005)
    with torch.no_grad():
        vlogits, _, _ = ht.hetegat_forward(xs, graphs, bp)
        vloss = BaseGAttN.masked_sigmoid_cross_entropy(vlogits, y, val_mask)
        vf1 = BaseGAttN.micro_f1(vlogits, y, val_mask)
        # a prediction can differ from the oracle's only where the oracle's logit is nearer to zero than the logits
        # can differ: 2e-4, to which this test holds the parameters (twice the 1e-4 of the suite's logits).  Each
        # such entry moves tp, fp or fn by one, so 2 tp and b = 2 tp + fp + fn by at most 2 each, and F1 = 2 tp / b <= 1
        # by at most 4 k / (b - 2 k) for k of them.
        k = int((vlogits[val_mask].abs() < 2e-4).sum())
        pred, lab = vlogits[val_mask] > 0, y[val_mask] > 0
        b = 2 * int((pred & lab).sum()) + int((pred & ~lab).sum()) + int((~pred & lab).sum())
    return float(data_loss.detach()), float(vloss), float(vf1), 4.0 * k / (b - 2 * k)


def test_three_training_steps_match_oracle(dev):
    """HANTrainer(objective="sigmoid"), dropout 0.6 / 0.6, three epochs against the float64 autograd oracle fed the
    regenerated hash masks: training and validation loss within 5e-4 (the suite's bound under dropout), micro-F1 within
    what the validation logits inside 2e-4 of zero can move it (_oracle_epoch; 1e-5 on top, the suite's bound for the accuracy),
    parameters within 2e-4."""
    from han_amd import rng as hrng
    from han_amd.trainer import HANTrainer
    from oracle import han_oracle as ho
    from oracle import han_oracle_torch as ht
    from tests import rng_ref
    from tests.helpers import build_model, gpu_inputs
    prob = _model_problem()
    n, f, drop = prob["n"], prob["f"], 0.6
    model, bp = build_model(prob, dev)
    x, graphs = gpu_inputs(prob, dev)
    tm, vm = torch.tensor(prob["mask"]), torch.tensor(~prob["mask"])
    hrng.manual_seed(99)
    seeds = [hrng.next_seed() for _ in range(6)]
    hrng.manual_seed(99)                       # the trainer draws the same seeds: two per training step
    tr = HANTrainer(model, [x] * 2, graphs, torch.from_numpy(prob["y"]), tm.to(torch.uint8), vm.to(torch.uint8),
                    lr=0.005, l2_coef=0.001, attn_drop=drop, ffd_drop=drop, objective="sigmoid")
    assert tr.labels.dtype == torch.int64 and tuple(tr.labels.shape) == (n, 1)
    bpo = {k: v.clone() for k, v in bp.items()}
    state = ht.new_adam_state(bpo)
    xt, y = torch.tensor(prob["x"][0]), torch.tensor(prob["y"].astype(np.float64))
    csr = [ho.bias_to_csr(b) for b in prob["biases"]]
    og = [tuple(torch.tensor(t) for t in g) for g in csr]
    keep = rng_ref.keep_prob32(drop)
    for step in range(3):
        tl, tf1, vl, vf1 = (float(v) for v in tr.epoch())
        masks = [{"seq": torch.tensor(rng_ref.seq_mask(seeds[2 * step + q], n, f, 8, drop)),
                  "coef": torch.tensor(rng_ref.coef_mask_csr(seeds[2 * step + q], csr[q][0], csr[q][1], 8, drop)),
                  "fts": torch.tensor(rng_ref.fts_mask(seeds[2 * step + q], n, 64, drop))} for q in range(2)]
        tl_ref, vl_ref, vf1_ref, e_f1 = _oracle_epoch([xt] * 2, og, bpo, state, y, tm, vm, keep, masks)
        print(f"step {step}: train loss {tl:.6f} / {tl_ref:.6f}  val loss {vl:.6f} / {vl_ref:.6f}  "
              f"val F1 {vf1:.6f} / {vf1_ref:.6f} (bound {e_f1:.2e})")
        assert abs(tl - tl_ref) < 5e-4 and abs(vl - vl_ref) < 5e-4
        assert e_f1 < 1e-2, "the bound must stay a check: few validation logits so close to zero"
        assert abs(vf1 - vf1_ref) <= e_f1 + 1e-5
        assert 0.0 < tf1 <= 1.0
    for k in ht.PARAM_ORDER:
        assert np.abs(getattr(model, k).detach().cpu().numpy() - bpo[k].numpy()).max() < 2e-4, k


def _planted_trainer(dev, **kw):
    from han_amd import rng as hrng, synth
    from han_amd.gat import HeteGAT_multi
    from han_amd.trainer import HANTrainer
    wl = synth.planted_partition(2048, 4, 2, 64, deg_in=6, deg_out=2, noise=1.0, seed=3, device=dev)
    y = synth.multilabel_labels(wl["labels"], 5, seed=3)
    u = torch.rand(2048, generator=torch.Generator().manual_seed(1))
    tm, vm = (u < 0.1).to(torch.uint8).to(dev), ((u >= 0.1) & (u < 0.2)).to(torch.uint8).to(dev)
    torch.manual_seed(0)
    hrng.manual_seed(5)
    model = HeteGAT_multi().build(2, 64, 5, (8,), (8, 1), 128, device=dev, generator=torch.Generator().manual_seed(11))
    return model, HANTrainer(model, [wl["x"]] * 2, wl["graphs"], y, tm, vm, objective="sigmoid", **kw)


def test_live_forward_on_and_off(dev):
    """The same parameters through eval_step with the row-list forward and with the full one: the listed rows carry
    the same logits, so the counts and with them micro-F1 are equal to the bit; the loss is the same terms added in
    another order (1e-5 relative, what the softmax trainer's live-forward test asserts).  Then three epochs each:
    parameters within 2e-4."""
    runs = []
    for on in (False, True):          # one after the other: each run starts the dropout seed stream afresh
        model, tr = _planted_trainer(dev, live_forward=on, live_backward=True)
        assert tr.live_forward == on
        first = model.flat.clone()
        l, f = tr.eval_step()
        l, f = l.clone(), f.clone()
        for _ in range(3):
            s = [float(v) for v in tr.epoch()]
        assert all(np.isfinite(s))
        runs.append((first, l, f, s, model.flat.clone()))
    (p0, l0, f0, s0, q0), (p1, l1, f1, s1, q1) = runs
    assert torch.equal(p0, p1)
    assert torch.equal(f0.view(1).view(torch.int32), f1.view(1).view(torch.int32)) and 0.0 < float(f0) < 1.0
    assert abs(float(l0) - float(l1)) <= 1e-5 * abs(float(l0))
    assert float((q0 - q1).abs().max()) < 2e-4
    assert abs(s1[2] - s0[2]) <= 1e-5 * abs(s0[2])


def test_captured_epoch_equals_the_eager_flow(dev):
    """use_graph=True: the captured and replayed epoch against the identical device-state flow launched eagerly --
    the four scalars and the parameters to the bit (the multi-label entry is capturable: nothing on the host)."""
    from han_amd import rng as hrng
    trainers = []
    for capture in (True, False):
        model, tr = _planted_trainer(dev, use_graph=True)
        tr._capture = capture
        trainers.append(tr)
    for ep in range(1, 5):
        outs = []
        for tr in trainers:
            if ep == 1:
                hrng.manual_seed(77)
            outs.append([float(v) for v in tr.epoch()])
        assert outs[0] == outs[1], (ep, outs)
        assert all(np.isfinite(outs[0]))
    assert trainers[0]._graph is not None and trainers[1]._graph is None
    assert torch.equal(trainers[0].model.flat, trainers[1].model.flat)


def test_early_stopping_and_checkpoint_on_micro_f1(dev, tmp_path):
    """early_stopping keeps the best micro-F1 / loss pair; a checkpoint restores the bookkeeping and the run goes on
    bit for bit."""
    model, tr = _planted_trainer(dev)
    for _ in range(3):
        tl, tf1, vl, vf1 = (float(v) for v in tr.epoch())
        assert not tr.early_stopping(vl, vf1)
    assert 0.0 < tr.vacc_mx <= 1.0 and tr.best_state is not None
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    nxt = [float(v) for v in tr.epoch()]
    model2, tr2 = _planted_trainer(dev)
    tr2.load_checkpoint(path)
    assert tr2.vacc_mx == tr.vacc_mx and tr2.vlss_mn == tr.vlss_mn
    assert [float(v) for v in tr2.epoch()] == nxt and torch.equal(model.flat, model2.flat)


def test_minibatch_trainer_on_the_seeds_of_a_block(dev):
    """Dropout 0, one batch = all training nodes: MiniBatchTrainer(objective="sigmoid") against HANTrainer on the same
    rows -- loss within 2e-4, micro-F1 within 1e-5, parameters within 2e-4 after three steps (the bounds of
    tests/test_ego_block_gpu.py) -- and evaluate() against eval_step."""
    from han_amd import minibatch
    from han_amd.trainer import HANTrainer
    from oracle import han_oracle_torch as ht
    from tests.helpers import build_model, gpu_inputs
    prob = _model_problem(seed=11, n=80, f=16, c=5)
    x, graphs = gpu_inputs(prob, dev)
    y = torch.from_numpy(prob["y"]).to(dev)
    tm = torch.tensor(prob["mask"].astype(np.uint8))
    full_model, _ = build_model(prob, dev)
    mini_model, _ = build_model(prob, dev)
    kw = dict(lr=0.005, l2_coef=0.001, attn_drop=0.0, ffd_drop=0.0, objective="sigmoid")
    full = HANTrainer(full_model, [x] * 2, graphs, y, tm, **kw)
    mini = minibatch.MiniBatchTrainer(mini_model, [x] * 2, graphs, y, tm, batch_size=80, seed=1, **kw)
    assert len(mini.batches()) == 1
    for _ in range(3):
        fl, ff = full.train_step()
        (b,) = mini.batches()
        ml, mf = mini.train_step(b)
        mini.epochs_done += 1
        assert abs(float(fl) - float(ml)) < 2e-4 and abs(float(ff) - float(mf)) < 1e-5
    for k in ht.PARAM_ORDER:
        assert float((getattr(full_model, k) - getattr(mini_model, k)).detach().abs().max()) < 2e-4, k
    vl, vf = mini.evaluate(tm)
    same = HANTrainer(mini_model, [x] * 2, graphs, y, tm, **kw)
    fl, ff = same.eval_step(same.train_mask, same.w_train)
    assert abs(float(vl) - float(fl)) < 2e-4 and abs(float(vf) - float(ff)) < 1e-5


def test_minibatch_epoch_forms_micro_f1_from_summed_counts(dev):
    """Several batches, dropout 0 and lr 0 (the parameters stay put): the training micro-F1 of epoch() is the micro-F1 of
    ALL training nodes -- what eval_step of the full-graph trainer gives on the train mask -- not the mean of the
    batches' values, which differs from it on this problem by more than the tolerance."""
    from han_amd import layers, minibatch
    from han_amd.trainer import HANTrainer
    from tests.helpers import build_model, gpu_inputs
    prob = _model_problem(seed=11, n=80, f=16, c=5)
    x, graphs = gpu_inputs(prob, dev)
    y = torch.from_numpy(prob["y"]).to(dev)
    tm = torch.tensor(prob["mask"].astype(np.uint8))
    model, _ = build_model(prob, dev)
    kw = dict(lr=0.0, l2_coef=0.0, attn_drop=0.0, ffd_drop=0.0, objective="sigmoid")
    mini = minibatch.MiniBatchTrainer(model, [x] * 2, graphs, y, tm, batch_size=7, seed=1, **kw)
    batches = mini.batches()
    assert len(batches) >= 4
    start = model.flat.clone()
    per, counts = [], torch.zeros(3, dtype=torch.int64, device=dev)
    for b in batches:
        _, f1 = mini.train_step(b)
        per.append(float(f1) * b.size / mini.train_ids.size)
        counts += mini.last_counts
    tl, tf1, vl, vf1 = mini.epoch()
    assert torch.equal(model.flat, start)
    full = HANTrainer(model, [x] * 2, graphs, y, tm, **kw)
    fl, ff = full.eval_step(full.train_mask, full.w_train)
    assert abs(float(tf1) - float(ff)) < 1e-5 and abs(float(tl) - float(fl)) < 2e-4
    assert float(tf1) == float(layers.micro_f1_of_counts(counts))
    assert int(counts[0] + counts[2]) == int(prob["y"][prob["mask"]].sum())      # tp + fn: every set label of the nodes
    assert abs(sum(per) - float(ff)) > 1e-4, "the mean of the batch values is another number here"
