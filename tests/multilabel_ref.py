"""float64 reference of the multi-label classifier kernels (han_classifier_multilabel, han_amd/csrc/loss_opt.hip and
multilabel_body.h) with a running fp32 error bound, and the seeded inputs the host and the GPU tests share (test
infrastructure, NumPy only; the style and the helpers of tests/loss_opt_ref.py).

The arithmetic (include/han_hip.h): logits x = Z Wm + bm as han_classifier_loss forms them; per class, e = exp(-|x|),

    term   t = max(x, 0) - x y + log(1 + e)          row = (1/C) sum_c t_c        loss = sum_i w_i row_i
    sigma  s = 1 / (1 + e) (x >= 0), e / (1 + e) (x < 0)                          dl = (w / C) (s - y)
    pred   p = (x > 0);   tp, fp, fn over the live rows;   micro_f1 = 2 tp / (2 tp + fp + fn), NaN for tp == 0

Bounds, every constant a count of roundings of u = 2^-24 (none measured); e_lg is loss_opt_ref's bound of the logits:

    t      the derivative of t in x is s - y, at most 1 in magnitude, so the error of the logit costs e_lg.  At the
           fp32 logit: exp(-|x|) is off by (4 + 2|x|) u relative (the fast __expf, as in loss_opt_ref), which reaches
           log(1 + e) as e (4 + 2|x|) u;  1 + e rounds: an absolute u;  the fast log of a value in [1, 2]: 4 u;  the two
           additions 3 u (|max(x,0) - x y| + log1p(e)):
                                            e_t = e_lg + (e (4 + 2|x|) + 5) u + 3 u mag,  mag = |max(x,0) - x y| + log1p(e)
    row    C terms in any order (a lane's loop or a butterfly) and the rounded 1/C:
                                            e_row = (sum_c e_t + (C + 3) u sum_c mag) / C
    loss   the product with w and the T-row summation (T live rows; the others add exact zeros):
                                            e_loss = |w| sum_i e_row + (T + 4) u |w| sum_i (sum_c mag / C)
    sigma  through the logit: s (1 - s) e_lg;  through e, 1 + e and the division: s ((4 + 2|x|) + 3) u;  TINY for a
           flushed subnormal:               e_s = s (1 - s) e_lg + s (7 + 2|x|) u + TINY
    dl     w / C is two roundings, the subtraction and the product two more:
                                            e_dl = (|w| / C) (e_s + 4 u |s - y|)
    dZ, dWc, dbc   from dl and e_dl exactly as loss_opt_ref.classifier_ref forms them.
    counts an entry is DECIDED when |x_c| > e_lg[c] (or e_lg[c] == 0: an exact logit): no fp32 evaluation inside the
           bound changes its prediction.  With no undecided entry on a live row the counts are exact integers and
           the kernel must return them; `undecided` counts the others (the shared inputs have none:
           tests/test_multilabel_host.py asserts it, so the GPU file may demand equality).
"""
import math
import types

import numpy as np

from tests.loss_opt_ref import TINY, U, f32s, ratio, up  # noqa: F401  (re-exported for the tests)


def pack_bits(y):
    """(N, C) 0/1 -> (N, ceil(C/64)) uint64 words, class c at bit c % 64 of word c / 64 (NumPy restatement)."""
    y = np.asarray(y).astype(np.uint64)
    N, C = y.shape
    nw = (C + 63) // 64
    b = np.zeros((N, nw * 64), dtype=np.uint64)
    b[:, :C] = y
    return (b.reshape(N, nw, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def multilabel_ref(Z, Wc, bc, y, mask, row_weight, rows=None):
    """rows: the row list of the live form (None: every row) -- a row outside it is dead whatever its mask, and its Z
    may hold anything (its logits here are then meaningless and the caller leaves them out)."""
    Z, Wc, bc = up(Z), up(Wc), up(bc)
    N, D = Z.shape
    HC, _, C = Wc.shape
    y = np.asarray(y).astype(np.float64)
    assert y.shape == (N, C)
    live = np.asarray(mask) != 0
    if rows is not None:
        listed = np.zeros(N, dtype=bool)
        listed[np.asarray(rows, dtype=np.int64)] = True
        live = live & listed
    T = int(live.sum())
    wv = f32s(row_weight)
    Wm, Wa = Wc.mean(0), np.abs(Wc).mean(0)
    bm, ba = bc.mean(0), np.abs(bc).mean(0)
    r = types.SimpleNamespace(N=N, D=D, C=C, HC=HC, T=T, live=live)
    with np.errstate(invalid="ignore", over="ignore"):
        r.logits = Z @ Wm + bm
        r.e_logits = (D + HC + 3) * U * (np.abs(Z) @ Wa + ba)
    L = np.nonzero(live)[0]
    x, e_lg, yl, aZ = r.logits[L], r.e_logits[L], y[L], np.abs(Z[L])
    ax = np.abs(x)
    e = np.exp(-ax)
    l1p = np.log1p(e)
    lin = np.maximum(x, 0.0) - x * yl
    mag = np.abs(lin) + l1p
    e_t = e_lg + (e * (4 + 2 * ax) + 5) * U + 3 * U * mag
    rowmag = mag.sum(1) / C
    r.row = (lin + l1p).sum(1) / C
    r.e_row = (e_t.sum(1) + (C + 3) * U * mag.sum(1)) / C
    r.loss = float(wv * r.row.sum())
    r.e_loss = float(abs(wv) * r.e_row.sum() + (T + 4) * U * abs(wv) * rowmag.sum())
    s = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    e_s = s * (1 - s) * e_lg + s * (7 + 2 * ax) * U + TINY
    wc = wv / C
    dl, e_dl = wc * (s - yl), abs(wc) * (e_s + 4 * U * np.abs(s - yl))
    r.sigma = s
    r.dl = np.zeros((N, C))
    r.e_dl = np.zeros((N, C))
    r.dl[L], r.e_dl[L] = dl, e_dl
    r.dZ = np.zeros((N, D))
    r.e_dZ = np.zeros((N, D))
    r.dZ[L] = dl @ Wm.T
    r.e_dZ[L] = e_dl @ Wa.T + (C + HC + 2) * U * (np.abs(dl) @ Wa.T)
    r.dWc = np.broadcast_to(Z[L].T @ dl / HC, (HC, D, C))
    r.e_dWc = np.broadcast_to((aZ.T @ e_dl + (T + 3) * U * (aZ.T @ np.abs(dl))) / HC, (HC, D, C))
    r.dbc = np.broadcast_to(dl.sum(0) / HC, (HC, C))
    r.e_dbc = np.broadcast_to((e_dl.sum(0) + (T + 3) * U * np.abs(dl).sum(0)) / HC, (HC, C))
    pred, lab = x > 0, yl != 0
    r.undecided = int((~((ax > e_lg) | (e_lg == 0))).sum())
    r.tp, r.fp, r.fn = int((pred & lab).sum()), int((pred & ~lab).sum()), int((~pred & lab).sum())
    r.counts = np.array([r.tp, r.fp, r.fn], dtype=np.int64)
    r.f1 = 2.0 * r.tp / (2.0 * r.tp + r.fp + r.fn) if r.tp else math.nan
    return r


def f1_matches(got, ref):
    """micro-F1 is formed in double from exact counts and rounded to fp32 once."""
    got = float(got)
    return math.isnan(got) if math.isnan(ref.f1) else got == float(np.float32(ref.f1))


def multilabel_ratios(ref, logits, loss_acc, grads=None, rows=None):
    """err / bound per quantity of one classifier_multilabel call (NumPy arrays): every value must be <= 1.  rows: compare
    the logits on these rows only (the row list of the live form)."""
    sel = slice(None) if rows is None else np.asarray(rows, dtype=np.int64)
    out = {"logits": ratio(logits[sel], ref.logits[sel], ref.e_logits[sel]),
           "loss": ratio(float(loss_acc[0]), ref.loss, ref.e_loss)}
    if grads is not None:
        out["dZ"] = ratio(grads[0][sel], ref.dZ[sel], ref.e_dZ[sel])
        out["dWc"] = ratio(grads[1], ref.dWc, ref.e_dWc)
        out["dbc"] = ratio(grads[2], ref.dbc, ref.e_dbc)
    return out


# ------------------------------------------------------------------------------------------------ inputs
# (D, C, HC) per kernel form: 16 lanes per row at each unroll (4, 8, 16); class per lane; the any-shape row kernel
# (C = 100 crosses a label word)
ROW16 = [(64, 3, 1), (64, 8, 2), (128, 16, 3)]
WIDE = [(64, 17, 1), (64, 64, 2), (128, 33, 1)]
GEN = [(320, 17, 3), (64, 100, 1), (1088, 5, 1)]
FUSED = ROW16 + WIDE
CELLS = FUSED + GEN
SMALL_N = [1, 15, 16, 17, 63, 65, 257]
SMALL_CELLS = [(64, 8, 2), (128, 33, 1), (320, 17, 3)]      # one per form
N_LIVE = 48
GRID_CAP = 2048             # kClsBlocks, kClsGenBlocks


def family(D, C):
    if D in (64, 128) and C <= 16:
        return "row16"
    return "wide" if D in (64, 128) and C <= 64 else "gen"


def kernel_name(D, C):
    fam = family(D, C)
    if fam == "row16":
        return f"multilabel_kernel<CM={4 if C <= 4 else 8 if C <= 8 else 16},NV={D // 64}>"
    if fam == "wide":
        return f"multilabel_wide_kernel<NV={D // 64}>"
    return f"ml_gen_kernel<NV={4 if D <= 256 else 8 if D <= 512 else 16 if D <= 1024 else 0}>+cls_dw_kernel"


def rows_per_block(D, C):
    return 16 if family(D, C) == "row16" else 4


def loop_n(D, C):
    """One grid-stride pass of the capped grid plus 77 rows: some groups / waves take a second row."""
    return GRID_CAP * rows_per_block(D, C) + 77


def _weights(rng, D, C, HC, scale=2.0):
    Wc = (rng.standard_normal((HC, D, C)) * (scale / math.sqrt(D))).astype(np.float32)
    bc = (rng.standard_normal((HC, C)) * 0.1 * scale).astype(np.float32)
    return Wc, bc


def _decided(make, key):
    """The first draw of `make(rng)` (seeds key + [0], key + [1], ...) whose live rows hold no undecided entry."""
    for bump in range(64):
        case = make(np.random.default_rng(list(key) + [bump]))
        if multilabel_ref(**case).undecided == 0:
            return case
    raise AssertionError(f"no decided draw for {key}")


def planted_case(D, C, HC):
    """N past the row loop; 48 live rows -- row 0, row N - 1, the 77 rows of the second pass among them, both sides of
    a block boundary, one row with mask byte 255, an all-zero and an all-one label row; every other Z row holds large
    finite junk (logits of a few thousand)."""
    N, rpb = loop_n(D, C), rows_per_block(D, C)

    def make(rng):
        Z = (rng.standard_normal((N, D)) * 1.0e3).astype(np.float32)
        Wc, bc = _weights(rng, D, C, HC)
        y = (rng.random((N, C)) < 0.4).astype(np.uint8)
        first = GRID_CAP * rpb                       # the first row of the second pass
        rows = [0, N - 1, first, first + 5, N - 2, rpb - 1, rpb, 777]
        rest = np.setdiff1d(rng.permutation(N)[:N_LIVE * 2], rows)
        rows = np.array(rows + list(rng.permutation(rest)[:N_LIVE - len(rows)]))
        assert len(np.unique(rows)) == N_LIVE
        Z[rows] = rng.standard_normal((N_LIVE, D)).astype(np.float32)
        y[rows[2]] = 0
        y[rows[3]] = 1
        mask = np.zeros(N, dtype=np.uint8)
        mask[rows] = 1
        mask[777] = 255
        return dict(Z=Z, Wc=Wc, bc=bc, y=y, mask=mask, row_weight=1.0 / N_LIVE)
    return _decided(make, [D, C, HC, N, 0])


def dense_case(D, C, HC, N):
    """Small N, about half of the rows live (row 0 always)."""
    def make(rng):
        Z = rng.standard_normal((N, D)).astype(np.float32)
        Wc, bc = _weights(rng, D, C, HC)
        y = (rng.random((N, C)) < 0.4).astype(np.uint8)
        mask = (rng.random(N) < 0.5).astype(np.uint8)
        mask[0] = 1
        return dict(Z=Z, Wc=Wc, bc=bc, y=y, mask=mask, row_weight=1.0 / int(mask.sum()))
    return _decided(make, [D, C, HC, N, 1])


def live_list(case):
    """The row list of the live-form tests of a planted case: every masked row, as many unmasked ones, ascending -- it
    skips most rows -- and the Z the live call sees: NaN outside the list."""
    mask = case["mask"]
    N = mask.size
    on = np.nonzero(mask)[0]
    rng = np.random.default_rng([N, 7])
    off = np.setdiff1d(rng.permutation(N)[:3 * on.size], on)[:on.size]
    rows = np.sort(np.concatenate([on, off])).astype(np.int32)
    Zn = np.full_like(case["Z"], np.nan)
    Zn[rows] = case["Z"][rows]
    return rows, Zn


def saturation_case(D, C, s, N=16):
    """Logits of exactly +-s: HC = 1, zero bias, Wc[0, 0, c] = +1 for even c and -1 for odd c, zero elsewhere, and
    Z[i] = (s, 0, ...).  Rows i % 4: labels equal to the prediction, the opposite, all zero, all one.  C a power of two
    and row_weight = 1 / 8 make w / C and every sum of dl exact.  Full mask."""
    Z = np.zeros((N, D), dtype=np.float32)
    Z[:, 0] = s
    Wc = np.zeros((1, D, C), dtype=np.float32)
    Wc[0, 0, :] = np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    bc = np.zeros((1, C), dtype=np.float32)
    pred = (np.arange(C) % 2 == 0).astype(np.uint8)
    y = np.zeros((N, C), dtype=np.uint8)
    y[0::4] = pred
    y[1::4] = 1 - pred
    y[3::4] = 1
    return dict(Z=Z, Wc=Wc, bc=bc, y=y, mask=np.ones(N, dtype=np.uint8), row_weight=0.125)


def zero_case(D, C, HC, N=5):
    """Row 0: zeros with zero bias -- logits exactly 0 --, the only live row, weight 1: loss = log 2, nothing predicted."""
    rng = np.random.default_rng([D, C, HC, 9])
    Z = rng.standard_normal((N, D)).astype(np.float32)
    Z[0] = 0
    Wc, _ = _weights(rng, D, C, HC)
    bc = np.zeros((HC, C), dtype=np.float32)
    y = (rng.random((N, C)) < 0.5).astype(np.uint8)
    y[0, 0] = 1
    mask = np.zeros(N, dtype=np.uint8)
    mask[0] = 1
    return dict(Z=Z, Wc=Wc, bc=bc, y=y, mask=mask, row_weight=1.0)


# exact counts past 2^24: tp = N * C is odd and above 2^24
BIG_N, BIG_C, BIG_TP = 266_401, 63, 16_783_263
