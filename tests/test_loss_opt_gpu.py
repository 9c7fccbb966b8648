"""GPU tests of han_amd/csrc/loss_opt.hip and the shared slab reduction (han_reduce_slabs): the fused classifier +
masked softmax cross-entropy + accuracy in its three kernel families, the backward for given dlogits, fused L2 + Adam,
han_l2_half_sumsq and the bias-matrix -> CSR kernels, through han_amd.ops.

Every comparison is elementwise |gpu - float64| <= e with the bound e of tests/loss_opt_ref.py (counts of fp32
roundings, derived there; tests/test_loss_opt_ref_host.py checks reference and bounds without a GPU), or exact where the
arithmetic is exact.  One case per cell of the dispatch of han_classifier_loss (loss_opt_ref.CELLS), forward-only and
with the backward:
  (a) N past the row loops (2 * 32768 + 37 rows for the 16-rows-per-block kernel, 2 * 8192 + 9 for the two wave-per-row
      families, so every group / wave takes 2 or 3 rows and the slab reduction sees 2048 slab rows), 64 planted live rows;
  (b) small-integer inputs at the same N: logits, and dZ / dWc / dbc of classifier_bwd, equal float64 bit for bit;
  (c) N in {1, 15, 16, 17, 63, 65, 257} with half of the rows live.
Further: argmax ties (first maximum wins), logits up to +-80, NaN-poisoned scratch and outputs, determinism; Adam per
element on p, m, v through the grid-stride loop and with the device step count; l2_half_sumsq; from_bias on a column
slice of a wider matrix (ld > N).

Largest err / bound measured on an MI355X (gfx950), per kernel instance over all of its cases -- (a), (c), ties, wide
range -- next to the plain fp32 restatement of the host file (torch CPU, the same inputs, per family).  The rows are
also the list of dispatch cells that ran:

    kernel (cells D,C)                                    logits   loss     acc      dZ       dWc      dbc
    classifier_kernel<CM=4,NV=1>   (64,1) (64,3)          0.024    0.0013   0.13     0.024    0.0028   0.0009
    classifier_kernel<CM=4,NV=2>   (128,3) (128,4)        0.0073   0.0004   0.0072   0.0030   0.0027   0.0009
    classifier_kernel<CM=8,NV=1>   (64,5) [(64,8) tie]    0.017    0.0011   0.0083   0.0023   0.0034   0.0019
    classifier_kernel<CM=8,NV=2>   (128,8)                0.0091   0.0007   0.0039   0.015    0.0032   0.0008
    classifier_kernel<CM=16,NV=1>  (64,9) (64,16)         0.026    0.0035   0.0025   0.016    0.036    0.0070
    classifier_kernel<CM=16,NV=2>  (128,16)               0.0075   0.0009   0.0007   0.0018   0.0065   0.0023
      fp32 restatement, tuned cells                       0.081    0.0027   0.031    0.024    0.036    0.0070
    classifier_wide_kernel<NV=1>   (64,17) (64,64)        0.074    0.0021   0        0.0078   0.19     0.049
    classifier_wide_kernel<NV=2>   (128,33) (128,64)      0.068    0.0010   0.0002   0.0062   0.069    0.036
      fp32 restatement, wide cells                        0.074    0.0018   0.0001   0.0078   0.19     0.049
    cls_gen_kernel<NV=4>+cls_dw    (192,3) (256,7) (64,65) (128,200) (192,65) [(192,7) (256,40) ties]
                                                          0.020    0.0025   0.010    0.019    0.090    0.016
    cls_gen_kernel<NV=8>+cls_dw    (320,17)               0.0017   0.0002   0        0.0006   0.0044   0.0028
    cls_gen_kernel<NV=16>+cls_dw   (1024,5)               0.0004   0.00002  0.0096   0.0002   0.0001   0.00003
    cls_gen_kernel<NV=0>+cls_dw    (1088,100)             0.0005   0.0001   0        0.0044   0.018    0.0024
      fp32 restatement, general cells                     0.046    0.0025   0.010    0.018    0.090    0.016
    cls_dz_kernel+cls_dw_kernel (classifier_bwd, real dlogits on 64 rows)            0.35     0.025    0.011

    adam_kernel: p 0.999, m 0.65, v 0.66 (restatement 0.999 / 0.66 / 0.69) -- where the step is far below p the whole
      error of p is the one rounding of the subtraction, half an ulp of p' against u |p|: the ratio reaches 1 for p just
      above a power of two and cannot exceed it;  with step_dev p 0.999, m 0.65, v 0.65;  TFAdam chain 0.95 / 0.58 / 0.63
    sumsq_kernel, 64 planted entries: 0.0097

(The accuracy column is the rounding of the weighted sum; 0 means every addition was exact.)  The 402 cases of this file
take 8 s on the GPU, the slowest 0.4 s.

Found by these tests and fixed in classifier_kernel: the 16-lane sum of the logits ended in two row rotations, after which
the four quads of a group hold differently associated totals.  Lane c stores logit c, lane 0 takes argmax and loss from its
own copies, so two classes with identical weights got stored logits an ulp apart (test_argmax_ties_first_maximum_wins
[64-8-1-2-5]) and the argmax of the stored row could differ from the class the accuracy counted.  The sum is now a butterfly
(cls_row16_sum): all lanes hold the same bits.
"""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import han_oracle as ho
from tests import loss_opt_ref as R

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


def _gpu(case, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("Z", "Wc", "bc", "labels", "mask")}


def _loss(t, row_weight, backward, grad_out=None):
    from han_amd import ops
    return ops.classifier_loss(t["Z"], t["Wc"], t["bc"], t["labels"], t["mask"], row_weight, backward=backward,
                               grad_out=grad_out)


def _np(out):
    logits, la, grads = out
    return logits.cpu().numpy(), la.cpu().numpy(), None if grads is None else tuple(g.cpu().numpy() for g in grads)


def _check(case, ref, out, tag):
    logits, la, grads = _np(out)
    ratios = R.classifier_ratios(ref, logits, la, grads)
    _note(tag, ratios)
    assert max(ratios.values()) <= 1.0, ratios
    if grads is not None:
        assert not grads[0][~ref.live].any(), "dZ of a row outside the mask must be exactly 0"
    return ratios


@functools.lru_cache(maxsize=2)
def _planted(D, C, HC):
    case = R.planted_case(D, C, HC)
    return case, R.classifier_ref(**case)


@functools.lru_cache(maxsize=4)
def _dense(D, C, HC, N):
    case = R.dense_case(D, C, HC, N)
    return case, R.classifier_ref(**case)


CELL_BWD = [(D, C, HC, b) for (D, C, HC) in R.CELLS for b in (False, True)]


# ------------------------------------------------------------------------------------------------ classifier
@pytest.mark.parametrize("D,C,HC,backward", CELL_BWD)
def test_planted_rows_past_the_loop(dev, D, C, HC, backward):
    """(a): every row loop runs 2-3 times, the block reductions and han_reduce_slabs add 2048 slab rows."""
    case, ref = _planted(D, C, HC)
    _check(case, ref, _loss(_gpu(case, dev), case["row_weight"], backward), R.kernel_name(D, C))


@pytest.mark.parametrize("D,C,HC", R.CELLS)
def test_integer_inputs_exact(dev, D, C, HC):
    """(b): every row of the logits, and dZ / dWc / dbc of classifier_bwd (cls_dz_kernel + cls_dw_kernel without a mask),
    equal the float64 result bit for bit: all partial sums are multiples of 1/4 below 2^22."""
    from han_amd import ops
    case = R.integer_case(D, C, HC)
    t = _gpu(case, dev)
    Z, Wm, bm, dl = R.up(case["Z"]), R.up(case["Wc"]).mean(0), R.up(case["bc"]).mean(0), R.up(case["dlogits"])
    hc = case["Wc"].shape[0]
    lg = Z @ Wm + bm
    assert np.abs(lg).max() < 2 ** 22 and np.array_equal(lg * 4, np.round(lg * 4))
    for backward in (False, True):
        logits, la, _ = _np(_loss(t, case["row_weight"], backward))
        bad = np.nonzero((logits.astype(np.float64) != lg).any(1))[0]
        assert bad.size == 0, f"backward={backward}: {bad.size} rows differ, first {bad[:8]}"
        assert np.isfinite(la).all()
    dZ, dWc, dbc = (g.cpu().numpy().astype(np.float64) for g in
                    ops.classifier_bwd(t["Z"], t["Wc"], t["bc"], torch.from_numpy(case["dlogits"]).to(dev)))
    bad = np.nonzero((dZ != dl @ Wm.T).any(1))[0]
    assert bad.size == 0, f"dZ: {bad.size} rows differ, first {bad[:8]}"
    dWm = Z.T @ dl
    assert np.abs(dWm).max() < 2 ** 22
    assert np.array_equal(dWc, np.broadcast_to(dWm / hc, dWc.shape))
    assert np.array_equal(dbc, np.broadcast_to(dl.sum(0) / hc, dbc.shape))


@pytest.mark.parametrize("N", R.SMALL_N)
@pytest.mark.parametrize("D,C,HC,backward", CELL_BWD)
def test_small_n_dense_mask(dev, D, C, HC, backward, N):
    """(c): partial blocks, partial groups, a single row."""
    case, ref = _dense(D, C, HC, N)
    _check(case, ref, _loss(_gpu(case, dev), case["row_weight"], backward), R.kernel_name(D, C))


@pytest.mark.parametrize("D,C,HC", [(64, 3, 1), (128, 16, 3), (64, 64, 2), (1088, 100, 1)])
def test_classifier_bwd_planted_rows(dev, D, C, HC):
    """classifier_bwd with real-valued dlogits that are nonzero on the planted rows only, against its bound."""
    from han_amd import ops
    case, _ = _planted(D, C, HC)
    live = case["mask"] != 0
    dl = np.zeros((live.size, C), dtype=np.float32)
    dl[live] = np.random.default_rng(C).standard_normal((int(live.sum()), C)).astype(np.float32)
    ref = R.classifier_bwd_ref(case["Z"], case["Wc"], case["bc"], dl)
    assert ref.T == R.N_LIVE
    t = _gpu(case, dev)
    grads = tuple(g.cpu().numpy() for g in ops.classifier_bwd(t["Z"], t["Wc"], t["bc"], torch.from_numpy(dl).to(dev)))
    ratios = R.bwd_ratios(ref, grads)
    _note("cls_dz_kernel+cls_dw_kernel (classifier_bwd)", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("D,C,HC,j1,j2", R.TIES)
def test_argmax_ties_first_maximum_wins(dev, D, C, HC, j1, j2):
    case = R.tie_case(D, C, HC, j1, j2)
    acc, e_acc, pair_is_max = R.tie_expected_acc(case, j1, j2)
    assert pair_is_max
    ref = R.classifier_ref(**case)
    for backward in (False, True):
        out = _loss(_gpu(case, dev), case["row_weight"], backward)
        logits, la, _ = _np(out)
        assert np.array_equal(logits[:, j1], logits[:, j2]), "identical class columns must give bit-equal logits"
        assert abs(float(la[1]) - acc) <= e_acc, (float(la[1]), acc)
        _check(case, ref, out, R.kernel_name(D, C))


@pytest.mark.parametrize("D,C,HC", R.WIDE_RANGE)
def test_wide_logit_range(dev, D, C, HC):
    case = R.wide_range_case(D, C, HC)
    ref = R.classifier_ref(**case)
    out = _loss(_gpu(case, dev), case["row_weight"], True)
    logits, la, grads = _np(out)
    assert np.isfinite(la).all() and all(np.isfinite(g).all() for g in grads)
    _check(case, ref, out, R.kernel_name(D, C))


FAMILY_CELLS = [(64, 5, 3), (128, 16, 1), (128, 33, 2), (320, 17, 3), (1088, 100, 1)]


def _poison(dev, case):
    """0xFF bytes (NaN as fp32) in the cached classifier workspaces and in the blocks the next outputs are carved from."""
    from han_amd import ops
    for (_, tag), ws in ops._workspaces.items():
        if tag in ("cls", "clsb"):
            ws.fill_(0xFF)
    junk = [torch.full(s, float("nan"), device=dev) for s in
            (case["Z"].shape, (case["Z"].shape[0], case["Wc"].shape[2]), (2,))]
    del junk
    return (torch.full(case["Wc"].shape, float("nan"), device=dev), torch.full(case["bc"].shape, float("nan"), device=dev))


@pytest.mark.parametrize("D,C,HC", FAMILY_CELLS)
def test_poisoned_scratch_and_outputs(dev, D, C, HC):
    """No kernel reads scratch or output memory it has not written: NaN there changes nothing."""
    from han_amd import ops
    case, _ = _dense(D, C, HC, 257)
    t = _gpu(case, dev)
    dl = torch.from_numpy(np.random.default_rng(1).standard_normal((257, C)).astype(np.float32)).to(dev)
    clean = _loss(t, case["row_weight"], True)
    clean_fwd = _loss(t, case["row_weight"], False)
    clean_bwd = ops.classifier_bwd(t["Z"], t["Wc"], t["bc"], dl)
    go = _poison(dev, case)
    out = _loss(t, case["row_weight"], True, grad_out=go)
    assert torch.equal(out[0], clean[0]) and torch.equal(out[1], clean[1])
    assert all(torch.equal(a, b) for a, b in zip(out[2], clean[2]))
    assert out[2][1] is go[0] and out[2][2] is go[1]
    _poison(dev, case)
    out = _loss(t, case["row_weight"], False)
    assert torch.equal(out[0], clean_fwd[0]) and torch.equal(out[1], clean_fwd[1])
    _poison(dev, case)
    assert all(torch.equal(a, b) for a, b in zip(ops.classifier_bwd(t["Z"], t["Wc"], t["bc"], dl), clean_bwd))
    # nobody is in the mask: loss, accuracy and every gradient are zero, the logits stay
    dead = dict(t, mask=torch.zeros_like(t["mask"]))
    go = _poison(dev, case)
    logits, la, (dZ, dWc, dbc) = _loss(dead, case["row_weight"], True, grad_out=go)
    assert torch.equal(logits, clean[0])
    assert not la.any() and not dZ.any() and not dWc.any() and not dbc.any()
    assert not any(torch.isnan(x).any() for x in (la, dZ, dWc, dbc))


@pytest.mark.parametrize("D,C,HC", [(128, 16, 3), (64, 64, 2), (320, 17, 3)])
def test_planted_rows_deterministic(dev, D, C, HC):
    case, _ = _planted(D, C, HC)
    t = _gpu(case, dev)
    a, b = _loss(t, case["row_weight"], True), _loss(t, case["row_weight"], True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


# ------------------------------------------------------------------------------------------------ Adam
ADAM_N = [1, 255, 257, 2 * 524288 + 77]        # 2048 blocks of 256: the last size runs the grid-stride loop three times


def _adam_gpu(dev, state, lr, l2, step_dev=None):
    from han_amd import ops
    p, g, m, v = (torch.from_numpy(a.copy()).to(dev) for a in state)
    ops.adam_step(p, g, m, v, lr, 0.9, 0.999, 1e-8, l2, step_dev=step_dev)
    return p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("l2", [0.0, 0.001])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_single_step(dev, n, l2):
    p, g, m, v, zero = R.adam_state(n)
    ref = R.adam_ref(p, g, m, v, lr=0.005, t=3, l2=l2)
    got = _adam_gpu(dev, (p, g, m, v), ref.lr_t, l2)
    ratios = R.adam_ratios(ref, *got)
    _note("adam_kernel", ratios)
    assert max(ratios.values()) <= 1.0, ratios
    if l2 == 0.0:
        assert np.array_equal(got[0][zero].view(np.uint32), p[zero].view(np.uint32)), "g = m = v = 0 must leave p alone"
        assert not got[1][zero].any() and not got[2][zero].any()


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 10 ** 6])
def test_adam_device_step_count(dev, t):
    """step_dev: lr_t formed on the device in double from the fp32 lr, beta1, beta2 -- the step equals the one with the
    same lr_t formed on the host, within the bound of p and one fp32 ulp of the rate (2u |step|)."""
    n = 2 * 524288 + 77 if t == 10 else 4099
    p, g, m, v, _ = R.adam_state(n, seed=t)
    ref = R.adam_ref(p, g, m, v, lr=0.005, t=t, l2=0.001)
    extra = 2 * R.U * np.abs(ref.step)
    host = _adam_gpu(dev, (p, g, m, v), R.adam_lr_t(0.005, t), 0.001)
    devc = _adam_gpu(dev, (p, g, m, v), 0.005, 0.001, step_dev=torch.tensor([t], dtype=torch.int64, device=dev))
    ratios = R.adam_ratios(ref, *devc, extra_p=extra)
    _note("adam_kernel step_dev", ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert np.array_equal(devc[1], host[1]) and np.array_equal(devc[2], host[2])
    assert (np.abs(devc[0].astype(np.float64) - host[0]) <= ref.e_p + extra).all()


@pytest.mark.parametrize("device_count", [False, True])
def test_tfadam_five_step_chain(dev, device_count):
    """TFAdam over five steps, each step checked from the state the GPU held before it: the step count, the in-place
    m / v and (host path) lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) as TFAdam states it."""
    from han_amd.base_gattn import TFAdam
    n, lr, l2 = 1500, 0.005, 0.001
    rng = np.random.default_rng(11)
    p = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    g = torch.zeros_like(p)
    opt = TFAdam(p, g, lr=lr, l2_coef=l2)
    if device_count:
        opt.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    for t in range(1, 6):
        g.copy_(torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)))
        before = tuple(x.cpu().numpy() for x in (p, g, opt.m, opt.v))
        if device_count:
            opt.step_dev.fill_(t)
            ref = R.adam_ref(*before, lr=lr, t=t, l2=l2)
            extra = 2 * R.U * np.abs(ref.step)
        else:
            ref = R.adam_ref(*before, lr_t=lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t), l2=l2)
            extra = 0.0
        opt.step()
        assert opt.t == t
        ratios = R.adam_ratios(ref, p.cpu().numpy(), opt.m.cpu().numpy(), opt.v.cpu().numpy(), extra_p=extra)
        _note("adam_kernel TFAdam chain", ratios)
        assert max(ratios.values()) <= 1.0, (t, ratios)


# ------------------------------------------------------------------------------------------------ l2_half_sumsq
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 262144 + 5, 2 * 262144 + 77])
def test_l2_half_sumsq(dev, n):
    """Entries in {0..3}: every partial sum is an integer below 2^24, the result is exact in any order (1024 blocks of
    256: the last size loops three times).  Then 64 planted random entries among zeros against (64 + 3) u sum p^2."""
    from han_amd import ops
    rng = np.random.default_rng(n)
    p = rng.integers(0, 4, n).astype(np.float32)
    s, _ = R.half_sumsq_ref(p)
    assert 2 * s < 2 ** 24
    assert float(ops.l2_half_sumsq(torch.from_numpy(p).to(dev))[0]) == s
    q = np.zeros(n, dtype=np.float32)
    idx = rng.permutation(n)[:63]
    q[idx] = (rng.standard_normal(idx.size) * 10.0 ** rng.uniform(-2, 2, idx.size)).astype(np.float32)
    q[n - 1] = 3.5                                   # the last element is among the (at most) 64
    s, e = R.half_sumsq_ref(q)
    assert e <= 67 * R.U * float((R.up(q) ** 2).sum())
    r = R.ratio(float(ops.l2_half_sumsq(torch.from_numpy(q).to(dev))[0]), s, e)
    _note("sumsq_kernel", {"sumsq": r})
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ from_bias, ld > N
@pytest.mark.parametrize("N", [5, 64, 65, 130])
def test_from_bias_column_slice(dev, N):
    """bias = wide[:, 3:3+N]: rows are ld = N + 11 floats apart.  An all-masked row, an entry exactly at -1e8 (no edge),
    one just above it (an edge), and edges in the columns outside the slice that must not be seen."""
    from han_amd.graph import CSRGraph
    rng = np.random.default_rng(N)
    wide = np.where(rng.random((N, N + 11)) < 0.3, 0.0, -1e9).astype(np.float32)
    wide[:, :3] = np.where(np.arange(N)[:, None] % 2 == 0, 0.0, -1e9)
    wide[:, 3 + N:] = np.where(np.arange(8)[None, :] % 3 == 0, -1e9, 0.0)
    wide[2, 3:3 + N] = -1e9
    wide[0, 3 + 1] = np.float32(-1e8)
    wide[0, 3 + 2] = np.nextafter(np.float32(-1e8), np.float32(0))
    wide[N - 1, 3 + N - 1] = np.nextafter(np.float32(-1e8), np.float32(0))
    wide[N - 1, 3 + N - 2] = np.float32(-1e8)
    tw = torch.from_numpy(wide).to(dev)
    bias = tw[:, 3:3 + N]
    assert bias.stride(0) == N + 11 and not bias.is_contiguous()
    g = CSRGraph.from_bias(bias)
    rp, ci = ho.bias_to_csr(wide[:, 3:3 + N])
    assert rp[3] == rp[2] and rp[-1] > 0
    assert np.array_equal(g.rowptr.cpu().numpy(), rp)
    assert np.array_equal(g.colidx.cpu().numpy(), ci)
    g2 = CSRGraph.from_bias(bias.contiguous())
    assert torch.equal(g2.rowptr, g.rowptr) and torch.equal(g2.colidx, g.colidx)
