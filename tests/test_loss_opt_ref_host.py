"""Host tests of tests/loss_opt_ref.py, the float64 reference with error bounds that tests/test_loss_opt_gpu.py holds
the classifier / loss / Adam kernels to.  No GPU.

  * the reference agrees with float64 autograd of the oracle (1e-12 relative);
  * a plain fp32 restatement (torch CPU: matmul, softmax, the Adam formula) stays inside every bound on the inputs of the
    GPU tests -- largest err / bound seen (test_zz_report prints them per family): logits 0.08, loss 0.003, accuracy
    0.03, dZ 0.02, dWc 0.19 (a single live row; 0.009 with the 64 planted rows), dbc 0.05, Adam p / m / v
    0.999 / 0.66 / 0.69 (p: one rounding of the subtraction against u |p|, which reaches 1 just above a power of two);
  * the bounds have teeth: the same comparison FAILS for the restatement after each planted mutation;
  * the preconditions of the GPU inputs hold for the committed seeds: every planted live row is decided, at most 0.5 % of
    the live rows of a dense-mask case are undecided, the duplicated pair of a tie case is the maximum of every live row.
"""
import numpy as np
import pytest
import torch

from oracle import han_oracle as ho
from oracle import han_oracle_torch as ht
from tests import loss_opt_ref as R

_SEEN = {}


def _note(tag, ratios):
    for k, v in ratios.items():
        _SEEN[(tag, k)] = max(_SEEN.get((tag, k), 0.0), v)
    print(tag, {k: f"{v:.3g}" for k, v in ratios.items()})


def restate32(case, mutation=None, columnwise=False):
    """The classifier + masked loss in plain fp32 (torch CPU).  Returns logits, (loss, acc), (dZ, dWc, dbc) as NumPy.
    `mutation` plants one of the faults the bounds must catch.  `columnwise` forms the logits one rounded product and
    one rounded addition per term, the same sequence for every class: two classes with identical weights then get
    identical bits on any host (a BLAS may treat the columns of a 7-wide matrix differently by position)."""
    Z, Wc, bc = (torch.from_numpy(case[k]) for k in ("Z", "Wc", "bc"))
    lab = torch.from_numpy(case["labels"].astype(np.int64))
    live = torch.from_numpy(case["mask"] != 0)
    N, HC, C = Z.shape[0], Wc.shape[0], Wc.shape[2]
    invh = torch.tensor(1.0 / HC, dtype=torch.float32)
    Wm, bm = Wc.sum(0) * invh, bc.sum(0) * invh
    if columnwise:
        lg = torch.zeros((N, C), dtype=torch.float32)
        for d in range(Z.shape[1]):
            lg = lg + Z[:, d:d + 1] * Wm[d]
        lg = lg + bm
    else:
        lg = Z @ Wm + bm
    rows = torch.arange(N)
    w = torch.where(live, torch.tensor(case["row_weight"], dtype=torch.float32), torch.tensor(0.0))
    if mutation == "skip_32768":
        w = torch.where(rows >= 32768, torch.tensor(0.0), w)
    am = torch.from_numpy(lg.numpy().argmax(1))               # first maximum
    if mutation == "argmax_last":
        am = C - 1 - torch.from_numpy(lg.numpy()[:, ::-1].argmax(1))
    p = torch.softmax(lg, 1)
    y = torch.zeros_like(p)
    y[rows, lab] = 1.0
    dl = w[:, None] * (p - y)
    loss = (w * (torch.logsumexp(lg, 1) - lg[rows, lab])).sum()
    acc = (w * (am == lab).to(torch.float32)).sum()
    dZ = dl @ Wm.T
    dl_w = dl.clone()
    if mutation == "dw_drop_row":
        dl_w[int(np.nonzero(case["mask"])[0][17])] = 0.0
    dWc = ((Z.T @ dl_w) * invh).expand(HC, -1, -1)
    dbc = (dl.sum(0) * (1.0 if mutation == "db_no_hc" else invh)).expand(HC, -1)
    lg = lg.clone()
    if mutation == "tail_logits":
        lg[N - N % 16:] = 0.0
    if mutation == "skip_32768":
        lg[32768:] = 0.0
    return lg.numpy(), (float(loss), float(acc)), (dZ.numpy(), dWc.numpy(), dbc.numpy())


def _ratios32(case, ref, mutation=None):
    lg, la, grads = restate32(case, mutation)
    return R.classifier_ratios(ref, lg, la, grads)


def adam32(p, g, m, v, lr_t, b1, b2, eps, l2, mutation=None):
    p, g, m, v = (torch.from_numpy(a.copy()) for a in (p, g, m, v))
    lr_t, b1, b2, eps, l2 = (torch.tensor(s, dtype=torch.float32) for s in (lr_t, b1, b2, eps, l2))
    gi = g + l2 * p
    mi = (b2 if mutation == "m_with_b2" else b1) * m + (1 - b1) * gi
    vi = b2 * v + (1 - b2) * gi * gi
    return (p - lr_t * mi / (torch.sqrt(vi) + eps)).numpy(), mi.numpy(), vi.numpy()


# ------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("D,C,HC,N", [(64, 3, 1, 65), (128, 16, 3, 63), (64, 64, 2, 17), (192, 65, 2, 257), (1088, 100, 1, 15)])
def test_reference_matches_float64_autograd(D, C, HC, N):
    case = R.dense_case(D, C, HC, N)
    ref = R.classifier_ref(**case)
    tZ, tW, tb = (torch.tensor(R.up(case[k]), requires_grad=True) for k in ("Z", "Wc", "bc"))
    logits = sum(tZ @ tW[i] + tb[i] for i in range(HC)) / HC
    onehot = torch.tensor(np.eye(C)[case["labels"]])
    mask = torch.tensor(case["mask"] != 0)
    T = int(mask.sum())
    # the oracle normalises the mask itself (mean over all rows of mask / mean(mask)): row_weight = 1 / T, up to the
    # fp32 rounding of the scalar the ABI takes
    scale = R.f32s(case["row_weight"]) * T
    loss = ht.masked_softmax_cross_entropy(logits, onehot, mask) * scale
    acc = ht.masked_accuracy(logits, onehot, mask) * scale
    loss.backward()

    def rel(a, b):
        return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))
    assert rel(ref.logits, logits.detach().numpy()) < 1e-12
    assert rel(ref.loss, loss.item()) < 1e-12 and rel(ref.acc, acc.item()) < 1e-12
    assert rel(ref.dZ, tZ.grad.numpy()) < 1e-12
    assert rel(ref.dWc, tW.grad.numpy()) < 1e-12
    assert rel(ref.dbc, tb.grad.numpy()) < 1e-12
    assert abs(ref.loss - ho.masked_softmax_cross_entropy(ref.logits, np.eye(C)[case["labels"]], case["mask"] != 0) * scale) \
        < 1e-12 * abs(ref.loss)
    # the linear part alone
    dl = np.random.default_rng(N).standard_normal((N, C)).astype(np.float32)
    tZ.grad = tW.grad = tb.grad = None
    (sum(tZ @ tW[i] + tb[i] for i in range(HC)) / HC * torch.tensor(R.up(dl))).sum().backward()
    b = R.classifier_bwd_ref(case["Z"], case["Wc"], case["bc"], dl)
    assert rel(b.dZ, tZ.grad.numpy()) < 1e-12 and rel(b.dWc, tW.grad.numpy()) < 1e-12 and rel(b.dbc, tb.grad.numpy()) < 1e-12


def test_adam_reference_matches_oracle():
    p, g, m, v, _ = R.adam_state(257)
    lr, b1, b2, eps, l2 = (R.f32s(s) for s in (0.005, 0.9, 0.999, 1e-8, 0.001))
    for t in (1, 2, 10, 1000):
        ref = R.adam_ref(p, g, m, v, lr=lr, t=t, l2=l2)
        # the oracle with the same (fp32) scalars; its lr_t is not rounded to fp32, which moves the step by u at most
        po, mo, vo = ho.adam_step_tf(R.up(p), R.up(g) + l2 * R.up(p), R.up(m), R.up(v), t, lr, b1, b2, eps)
        assert np.abs(ref.m - mo).max() <= 1e-12 * np.abs(mo).max()
        assert np.abs(ref.v - vo).max() <= 1e-12 * np.abs(vo).max()
        assert (np.abs(ref.p - po) <= R.U * np.abs(ref.step) + 1e-12 * np.abs(po)).all()
    s, e = R.half_sumsq_ref(p)
    assert abs(s - 0.5 * float((R.up(p) ** 2).sum())) <= 1e-12 * s and e > 0


# ------------------------------------------------------------------------------ fp32 restatement inside the bounds
@pytest.mark.parametrize("D,C,HC", R.CELLS)
def test_planted_rows_decided_and_fp32_inside_bounds(D, C, HC):
    case = R.planted_case(D, C, HC)
    assert int((case["mask"] != 0).sum()) == R.N_LIVE and case["mask"].max() == 255
    ref = R.classifier_ref(**case)
    assert ref.decided[ref.live].all(), f"{int((~ref.decided[ref.live]).sum())} undecided live rows: bump the seed"
    ratios = _ratios32(case, ref)
    _note("planted " + R.family(D, C), ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("D,C,HC", R.CELLS)
def test_dense_rows_decided_and_fp32_inside_bounds(D, C, HC):
    for N in R.SMALL_N:
        case = R.dense_case(D, C, HC, N)
        ref = R.classifier_ref(**case)
        und = int((~ref.decided[ref.live]).sum())
        assert und <= 0.005 * ref.T, f"N={N}: {und} of {ref.T} live rows undecided: bump the seed"
        ratios = _ratios32(case, ref)
        _note("dense " + R.family(D, C), ratios)
        assert max(ratios.values()) <= 1.0, (N, ratios)


@pytest.mark.parametrize("D,C,HC", R.WIDE_RANGE)
def test_wide_range_fp32_inside_bounds(D, C, HC):
    case = R.wide_range_case(D, C, HC)
    ref = R.classifier_ref(**case)
    assert 79.9 < np.abs(ref.logits).max() < 80.1 and np.isfinite(ref.loss)
    ratios = _ratios32(case, ref)
    _note("wide range", ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("D,C,HC,j1,j2", R.TIES)
def test_tie_cases_pair_is_maximum(D, C, HC, j1, j2):
    case = R.tie_case(D, C, HC, j1, j2)
    acc, e_acc, ok = R.tie_expected_acc(case, j1, j2)
    assert ok and 0.55 < acc < 0.8
    lg, la, _ = restate32(case, columnwise=True)
    assert np.array_equal(lg[:, j1], lg[:, j2])
    assert abs(la[1] - acc) <= e_acc
    assert max(R.classifier_ratios(R.classifier_ref(**case), lg, la).values()) <= 1.0
    _, la_last, _ = restate32(case, "argmax_last", columnwise=True)     # the last maximum: every j1 row is lost
    assert abs(la_last[1] - acc) > 0.1 > 1000 * e_acc


# ------------------------------------------------------------------------------------------------ teeth
def test_mutations_are_caught():
    D, C, HC = 128, 16, 3
    case = R.planted_case(D, C, HC)
    assert case["Z"].shape[0] > 2 * 32768 and (case["mask"][32768:] != 0).any()
    ref = R.classifier_ref(**case)
    base = _ratios32(case, ref)
    assert max(base.values()) <= 1.0
    r = _ratios32(case, ref, "dw_drop_row")
    print("one live row left out of dW: err / bound =", r["dWc"])
    assert r["dWc"] > 1.0 and r["logits"] <= 1.0 and r["dZ"] <= 1.0
    r = _ratios32(case, ref, "tail_logits")
    assert r["logits"] > 1.0
    r = _ratios32(case, ref, "db_no_hc")
    assert r["dbc"] > 1.0 and r["dWc"] <= 1.0
    r = _ratios32(case, ref, "skip_32768")
    assert r["logits"] > 1.0 and r["loss"] > 1.0 and r["dWc"] > 1.0 and r["dbc"] > 1.0
    # a dropped row is caught in every family's shapes, also where dW has many columns and T is 64
    for cell in [(64, 3, 1), (64, 64, 2), (1088, 100, 1), (192, 65, 2)]:
        case = R.planted_case(*cell)
        ref = R.classifier_ref(**case)
        r = _ratios32(case, ref, "dw_drop_row")
        print(cell, "one live row left out of dW: err / bound =", r["dWc"])
        assert r["dWc"] > 1.0
        if case["Z"].shape[0] % 16:
            assert _ratios32(case, ref, "tail_logits")["logits"] > 1.0
    # the last maximum on a planted tie (accuracy)
    D, C, HC, j1, j2 = R.TIES[0]
    case = R.tie_case(D, C, HC, j1, j2)
    acc, e_acc, _ = R.tie_expected_acc(case, j1, j2)
    assert abs(restate32(case, "argmax_last")[1][1] - acc) > e_acc


@pytest.mark.parametrize("n", [1, 255, 257, 2 * 524288 + 77])
def test_adam_fp32_inside_bounds_and_mutation_caught(n):
    p, g, m, v, zero = R.adam_state(n)
    for l2 in (0.0, 0.001):
        for t in (1, 1000):
            ref = R.adam_ref(p, g, m, v, lr=0.005, t=t, l2=l2)
            got = adam32(p, g, m, v, ref.lr_t, 0.9, 0.999, 1e-8, l2)
            ratios = R.adam_ratios(ref, *got)
            _note("adam", ratios)
            assert max(ratios.values()) <= 1.0, ratios
            if l2 == 0.0:
                assert np.array_equal(ref.p[zero], R.up(p)[zero]) and np.array_equal(got[0][zero], p[zero])
            if n > 1:
                bad = R.adam_ratios(ref, *adam32(p, g, m, v, ref.lr_t, 0.9, 0.999, 1e-8, l2, "m_with_b2"))
                assert bad["m"] > 1.0 and bad["p"] > 1.0 and bad["v"] <= 1.0


def test_adam_lr_t_forms():
    """adam_lr_t rounds the fp32 scalars first, as the device path does; the trainer's host path forms lr_t from the
    Python doubles.  The two differ by (1 - 0.999f) / 0.001 - 1 = -1.3e-5 in 1 - b2^t at small t, 6e-6 in the rate."""
    import math
    for t in (1, 2, 10, 1000, 10 ** 6):
        host = 0.005 * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        assert abs(R.adam_lr_t(0.005, t) - host) <= 1e-5 * host
    assert abs(R.adam_lr_t(0.005, 10 ** 6) - R.f32s(0.005)) <= R.U * 0.005


def test_zz_report():
    """Prints the largest err / bound of the fp32 restatement per input kind and quantity (run with -s)."""
    for (tag, k), v in sorted(_SEEN.items()):
        print(f"{tag:16s} {k:7s} {v:.3g}")
