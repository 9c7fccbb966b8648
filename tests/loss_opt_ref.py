"""float64 reference of the classifier / loss / Adam kernels (han_amd/csrc/loss_opt.hip) with a running fp32
error bound, and the seeded inputs the host and the GPU tests share (test infrastructure, NumPy only).

Every function takes the fp32 values the kernel sees and promotes them to float64; the scalars of the C ABI
(row_weight, lr_t, beta1/2, eps, l2_coef) are `float` there, so they go through np.float32 first.  Next to each
result `x` stands an elementwise bound `e_x` on |fp32 kernel - float64|, built from u = 2^-24 (the relative
rounding error of one fp32 operation) alone: the constants are counts of roundings, not measurements.

    logits   lg = Z Wm + bm, Wm = mean_h Wc, Wa = mean_h |Wc|:   the head sum and the 1/HC scaling (HC + 1 roundings of
             Wm), a dot product of D terms, the bias:             e_lg = (D + HC + 3) u (|Z| Wa + mean_h |bc|)
    softmax  x = lg - max.  Relative error of exp(x_c):           rho_c = e_lg[c] + e_lg[argmax] + (4 + 2|x_c|) u
             (both logits move, the subtraction, the fast __expf: its argument is scaled by log2(e) in fp32, which
             costs |x| u, and v_exp_f32 is good to an ulp);  of p_c = exp(x_c) / sum:
                                                                  r_c = rho_c + max_c rho + (C + 2) u
             An fp32 value below the smallest normal may be flushed to zero, hence the absolute TINY = 2^-126 on p.
    dl       dl = w (p - y):                                      e_dl = |w| (p r + TINY + 2u |p - y|)
    dZ       dl Wm^T, C terms against the rounded Wm:             e_dZ = e_dl Wa^T + (C + HC + 2) u (|dl| Wa^T)
    dW, db   T = number of live rows (mask != 0).  Dead rows add exact zeros, so at most T - 1 additions round
             whatever the order (lane, group, block, slab):       e_dW = (|Z|^T e_dl + (T + 3) u |Z|^T |dl|) / HC
             and e_db the same with |Z| replaced by ones.
    loss     per row  |w| (e_lg[am] + e_lg[lab] + max rho + C u + 4u max(1, |log se|) + 3u (|mx| + |log se| + |lg_lab|))
             plus (T + 3) u sum |w| (|mx| + |log se| + |lg_lab|) for the summation.
    accuracy a row is DECIDED when its float64 top-2 gap exceeds 2 max_c e_lg (no fp32 evaluation inside e_lg can
             change its argmax); the kernel's figure lies in [acc_lo, acc_hi] widened by (T + 3) u sum w, where the
             undecided live rows count for 0 in acc_lo and for w in acc_hi.
"""
import math
import types

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126


def up(a):
    """The fp32 values a kernel sees, as float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def f32s(x):
    """A scalar of the C ABI (`float`), as a Python float."""
    return float(np.float32(x))


def ratio(got, ref, e):
    """max |got - ref| / e.  Where the bound is 0 the values must be equal (ratio 0, else inf); a NaN counts as inf."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    e = np.broadcast_to(np.asarray(e, dtype=np.float64), d.shape)
    if d.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(e > 0, d / e, np.where(d == 0, 0.0, np.inf))
    r = np.where(np.isnan(d), np.inf, r)
    return float(r.max())


# ------------------------------------------------------------------------------------------------ classifier
def classifier_ref(Z, Wc, bc, labels, mask, row_weight):
    Z, Wc, bc = up(Z), up(Wc), up(bc)
    N, D = Z.shape
    HC, _, C = Wc.shape
    labels = np.asarray(labels).astype(np.int64)
    live = np.asarray(mask) != 0
    T = int(live.sum())
    w = np.where(live, f32s(row_weight), 0.0)
    rows = np.arange(N)
    Wm, Wa = Wc.mean(0), np.abs(Wc).mean(0)
    bm, ba = bc.mean(0), np.abs(bc).mean(0)
    r = types.SimpleNamespace(N=N, D=D, C=C, HC=HC, T=T, live=live, w=w)
    r.logits = lg = Z @ Wm + bm
    r.e_logits = e_lg = (D + HC + 3) * U * (np.abs(Z) @ Wa + ba)
    am = lg.argmax(1)                        # first maximum
    mx = lg[rows, am]
    x = lg - mx[:, None]
    ex = np.exp(x)
    se = ex.sum(1)
    p = ex / se[:, None]
    lse = np.log(se)
    rho = e_lg + e_lg[rows, am][:, None] + (4 + 2 * np.abs(x)) * U
    rmax = rho.max(1)
    rr = rho + rmax[:, None] + (C + 2) * U
    y = np.zeros((N, C))
    y[rows, labels] = 1.0
    lg_lab = lg[rows, labels]
    mag = np.abs(mx) + np.abs(lse) + np.abs(lg_lab)
    r.ce = mx + lse - lg_lab
    r.e_ce = (e_lg[rows, am] + e_lg[rows, labels] + rmax + C * U + 4 * U * np.maximum(1.0, np.abs(lse)) + 3 * U * mag)
    r.loss = float((w * r.ce).sum())
    r.e_loss = float((np.abs(w) * r.e_ce).sum() + (T + 3) * U * (np.abs(w) * mag).sum())
    if C > 1:
        top = np.partition(lg, C - 2, axis=1)
        gap = top[:, C - 1] - top[:, C - 2]
    else:
        gap = np.full(N, np.inf)
    r.decided = gap > 2 * e_lg.max(1)
    correct = am == labels
    r.acc = float((w * correct).sum())
    r.acc_lo = float((w * (correct & r.decided)).sum())
    r.acc_hi = r.acc_lo + float((w * ~r.decided).sum())
    r.e_acc = (T + 3) * U * float(w.sum()) if T else 0.0
    # backward: dead rows have dl == 0 and bound 0, only the live ones are formed
    L = np.nonzero(live)[0]
    r.dl = np.zeros((N, C))
    r.e_dl = np.zeros((N, C))
    r.dl[L] = w[L, None] * (p[L] - y[L])
    r.e_dl[L] = np.abs(w[L, None]) * (p[L] * rr[L] + TINY + 2 * U * np.abs(p[L] - y[L]))
    dl, e_dl, aZ = r.dl[L], r.e_dl[L], np.abs(Z[L])
    r.dZ = np.zeros((N, D))
    r.e_dZ = np.zeros((N, D))
    r.dZ[L] = dl @ Wm.T
    r.e_dZ[L] = e_dl @ Wa.T + (C + HC + 2) * U * (np.abs(dl) @ Wa.T)
    r.dWc = np.broadcast_to(Z[L].T @ dl / HC, (HC, D, C))
    r.e_dWc = np.broadcast_to((aZ.T @ e_dl + (T + 3) * U * (aZ.T @ np.abs(dl))) / HC, (HC, D, C))
    r.dbc = np.broadcast_to(dl.sum(0) / HC, (HC, C))
    r.e_dbc = np.broadcast_to((e_dl.sum(0) + (T + 3) * U * np.abs(dl).sum(0)) / HC, (HC, C))
    return r


def classifier_ratios(ref, logits, loss_acc, grads=None):
    """err / bound per quantity of one classifier_loss call (NumPy arrays): every value must be <= 1."""
    out = {"logits": ratio(logits, ref.logits, ref.e_logits),
           "loss": ratio(float(loss_acc[0]), ref.loss, ref.e_loss)}
    a = float(loss_acc[1])
    out["acc"] = ratio(a, min(max(a, ref.acc_lo), ref.acc_hi), ref.e_acc)
    if grads is not None:
        out["dZ"] = ratio(grads[0], ref.dZ, ref.e_dZ)
        out["dWc"] = ratio(grads[1], ref.dWc, ref.e_dWc)
        out["dbc"] = ratio(grads[2], ref.dbc, ref.e_dbc)
    return out


def classifier_bwd_ref(Z, Wc, bc, dlogits):
    """The linear part alone: the gradients of logits = (1/HC) sum_h (Z Wc[h] + bc[h]) for a given dlogits.
    T counts the rows with a nonzero dlogits entry (the others add exact zeros)."""
    Z, Wc, dl = up(Z), up(Wc), up(dlogits)
    N, D = Z.shape
    HC, _, C = Wc.shape
    Wm, Wa = Wc.mean(0), np.abs(Wc).mean(0)
    T = int((dl != 0).any(1).sum())
    adl, aZ = np.abs(dl), np.abs(Z)
    r = types.SimpleNamespace(N=N, D=D, C=C, HC=HC, T=T)
    r.dZ = dl @ Wm.T
    r.e_dZ = (C + HC + 2) * U * (adl @ Wa.T)
    r.dWc = np.broadcast_to(Z.T @ dl / HC, (HC, D, C))
    r.e_dWc = np.broadcast_to((T + 3) * U * (aZ.T @ adl) / HC, (HC, D, C))
    r.dbc = np.broadcast_to(dl.sum(0) / HC, (HC, C))
    r.e_dbc = np.broadcast_to((T + 3) * U * adl.sum(0) / HC, (HC, C))
    return r


def bwd_ratios(ref, grads):
    return {"dZ": ratio(grads[0], ref.dZ, ref.e_dZ), "dWc": ratio(grads[1], ref.dWc, ref.e_dWc),
            "dbc": ratio(grads[2], ref.dbc, ref.e_dbc)}


# ------------------------------------------------------------------------------------------------ optimiser
def adam_lr_t(lr, t, b1=0.9, b2=0.999):
    """The bias-corrected rate as adam_kernel forms it from a device step count: float64 arithmetic on the fp32
    lr, beta1, beta2, rounded to fp32."""
    lr, b1, b2 = f32s(lr), f32s(b1), f32s(b2)
    return float(np.float32(lr * math.sqrt(1.0 - math.pow(b2, float(t))) / (1.0 - math.pow(b1, float(t)))))


def adam_ref(p, g, m, v, lr_t=None, lr=None, t=None, b1=0.9, b2=0.999, eps=1e-8, l2=0.0):
    """One fused L2 + Adam step (tf.train.AdamOptimizer form) in float64, with bounds:
        g' = g + l2 p                      e_g = 2u (|g| + |l2 p|)
        m' = b1 m + (1 - b1) g'            e_m = (1 - b1) e_g + 3u (|b1 m| + |(1 - b1) g'|)
        v' = b2 v + (1 - b2) g'^2          e_v = (1 - b2) 2|g'| e_g + 3u (|b2 v| + |(1 - b2) g'^2|)
        p' = p - lr_t m' / (sqrt v' + eps) e_p = u |p| + |step| (6u + e_m / |m'| + e_v / (2 v'))
    (|step| e_m / |m'| is written lr_t e_m / (sqrt v' + eps), which also holds at m' = 0; the e_v term is 0 at
    v' = 0, where g' = 0 and v = 0 are exact).  1 - b is the fp32 difference the kernel forms."""
    p, g, m, v = up(p), up(g), up(m), up(v)
    if lr_t is None:
        lr_t = adam_lr_t(lr, t, b1, b2)
    lr_t, eps, l2 = f32s(lr_t), f32s(eps), f32s(l2)
    c1, c2 = float(np.float32(1) - np.float32(b1)), float(np.float32(1) - np.float32(b2))
    b1, b2 = f32s(b1), f32s(b2)
    gp = g + l2 * p
    e_g = 2 * U * (np.abs(g) + np.abs(l2 * p))
    r = types.SimpleNamespace(lr_t=lr_t)
    r.m = b1 * m + c1 * gp
    r.e_m = c1 * e_g + 3 * U * (np.abs(b1 * m) + np.abs(c1 * gp))
    r.v = b2 * v + c2 * gp * gp
    r.e_v = c2 * 2 * np.abs(gp) * e_g + 3 * U * (np.abs(b2 * v) + np.abs(c2 * gp * gp))
    den = np.sqrt(r.v) + eps
    r.step = lr_t * r.m / den
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_v = np.where(r.v > 0, r.e_v / (2 * r.v), 0.0)
    r.p = p - r.step
    r.e_p = U * np.abs(p) + lr_t * r.e_m / den + np.abs(r.step) * (6 * U + rel_v)
    return r


def adam_ratios(ref, p, m, v, extra_p=0.0):
    return {"p": ratio(p, ref.p, ref.e_p + extra_p), "m": ratio(m, ref.m, ref.e_m), "v": ratio(v, ref.v, ref.e_v)}


def half_sumsq_ref(p):
    """0.5 sum p^2 and its bound (T + 3) u sum p^2, T = number of nonzero entries."""
    p = up(p)
    s = float((p * p).sum())
    return 0.5 * s, (int(np.count_nonzero(p)) + 3) * U * s


# ------------------------------------------------------------------------------------------------ inputs
# One entry per cell of the dispatch of han_classifier_loss: (D, C, HC).  The tuned small-C kernel takes 16 rows
# per block iteration (CM = class bound 4 / 8 / 16, NV = D / 64), the other two one wave per row, all on at most
# 2048 blocks.
TUNED = [(64, 1, 2), (64, 3, 1), (128, 3, 2), (128, 4, 3), (64, 5, 3), (128, 8, 1), (64, 9, 2), (64, 16, 1), (128, 16, 3)]
WIDE = [(64, 17, 2), (128, 33, 3), (64, 64, 2), (128, 64, 1)]
GEN = [(192, 3, 1), (256, 7, 2), (320, 17, 3), (1024, 5, 2), (1088, 100, 1), (64, 65, 3), (128, 200, 1), (192, 65, 2)]
CELLS = TUNED + WIDE + GEN
SMALL_N = [1, 15, 16, 17, 63, 65, 257]
N_LIVE = 64


def family(D, C):
    if D in (64, 128) and C <= 16:
        return "tuned"
    return "wide" if D in (64, 128) and C <= 64 else "gen"


def kernel_name(D, C):
    """The template instance han_classifier_loss launches for (D, C)."""
    fam = family(D, C)
    if fam == "tuned":
        return f"classifier_kernel<CM={4 if C <= 4 else 8 if C <= 8 else 16},NV={D // 64}>"
    if fam == "wide":
        return f"classifier_wide_kernel<NV={D // 64}>"
    return f"cls_gen_kernel<NV={4 if D <= 256 else 8 if D <= 512 else 16 if D <= 1024 else 0}>+cls_dw_kernel"


def rows_per_block(D, C):
    return 16 if family(D, C) == "tuned" else 4


def loop_n(D, C):
    """Rows that make every group / wave of the 2048 blocks loop at least twice and some three times."""
    return 2 * 2048 * rows_per_block(D, C) + (37 if family(D, C) == "tuned" else 9)


# seeds whose draw misses a precondition (tests/test_loss_opt_ref_host.py asserts them) are bumped here
SEED_BUMP = {(320, 17, 3, 16393, 0): 1, (1088, 100, 1, 63, 1): 1, (1088, 100, 1, 65, 1): 2, (1088, 100, 1, 257, 1): 1}


def _rng(D, C, HC, N, kind):
    key = (D, C, HC, N, kind)
    return np.random.default_rng([D, C, HC, N, kind, SEED_BUMP.get(key, 0)])


def _weights(rng, D, C, HC, scale=2.0):
    Wc = (rng.standard_normal((HC, D, C)) * (scale / math.sqrt(D))).astype(np.float32)
    bc = (rng.standard_normal((HC, C)) * 0.1 * scale).astype(np.float32)
    return Wc, bc


def planted_case(D, C, HC):
    """Case (a): N past the row loop, 64 live rows -- row 0 and N - 1, the three rows one group / wave visits in its
    1st, 2nd and 3rd iteration, both sides of a block boundary, one row with mask byte 255, the rest random."""
    N, rpb = loop_n(D, C), rows_per_block(D, C)
    rng = _rng(D, C, HC, N, 0)
    Z = rng.standard_normal((N, D), dtype=np.float32)
    Wc, bc = _weights(rng, D, C, HC)
    labels = rng.integers(0, C, N).astype(np.int32)
    stride = 2048 * rpb
    rows = [0, N - 1, 5, 5 + stride, 5 + 2 * stride, rpb - 1, rpb, 777]
    rest = np.setdiff1d(rng.permutation(N)[:N_LIVE * 2], rows, assume_unique=False)
    rows = np.array(rows + list(rng.permutation(rest)[:N_LIVE - len(rows)]))
    assert len(np.unique(rows)) == N_LIVE
    mask = np.zeros(N, dtype=np.uint8)
    mask[rows] = 1
    mask[777] = 255
    return dict(Z=Z, Wc=Wc, bc=bc, labels=labels, mask=mask, row_weight=1.0 / N_LIVE)


def dense_case(D, C, HC, N):
    """Case (c): small N, half of the rows live (row 0 always)."""
    rng = _rng(D, C, HC, N, 1)
    Z = rng.standard_normal((N, D), dtype=np.float32)
    Wc, bc = _weights(rng, D, C, HC)
    labels = rng.integers(0, C, N).astype(np.int32)
    mask = (rng.random(N) < 0.5).astype(np.uint8)
    mask[0] = 1
    return dict(Z=Z, Wc=Wc, bc=bc, labels=labels, mask=mask, row_weight=1.0 / int(mask.sum()))


def integer_case(D, C, HC):
    """Case (b): small integers, HC in {1, 2, 4} (a head count of 3 maps to 4), dense mask, integer dlogits.  Every
    product and partial sum of logits, dZ, dWc, dbc is a multiple of 1/4 below 2^22 in magnitude: exact in fp32 in
    any order."""
    N, HC = loop_n(D, C), {1: 1, 2: 2, 3: 4}[HC]
    rng = _rng(D, C, HC, N, 2)
    Z = rng.integers(-2, 3, (N, D)).astype(np.float32)
    Wc = rng.integers(-2, 3, (HC, D, C)).astype(np.float32)
    bc = rng.integers(-2, 3, (HC, C)).astype(np.float32)
    dl = rng.integers(-2, 3, (N, C)).astype(np.float32)
    labels = rng.integers(0, C, N).astype(np.int32)
    return dict(Z=Z, Wc=Wc, bc=bc, labels=labels, mask=np.ones(N, dtype=np.uint8), row_weight=1.0 / N, dlogits=dl)


# (D, C, HC, j1, j2): one tie per kernel family, and a pair that straddles classes 15 / 16 (two cls_dw_kernel tiles)
TIES = [(64, 8, 1, 2, 5), (128, 33, 2, 7, 20), (192, 7, 3, 0, 6), (256, 40, 2, 15, 16)]
WIDE_RANGE = [(64, 5, 3), (128, 33, 2), (1088, 100, 1)]


def tie_case(D, C, HC, j1, j2, N=257):
    """Classes j1 < j2 share their column of Wc and bc (bit-equal logits) and carry a bias that makes the pair the
    maximum of every row; two thirds of the rows are labelled j1 (correct: the first maximum wins), the others j2."""
    rng = _rng(D, C, HC, N, 3)
    Z = rng.standard_normal((N, D), dtype=np.float32)
    Wc, bc = _weights(rng, D, C, HC, scale=1.0)
    Wc[:, :, j2] = Wc[:, :, j1]
    bc[:, j1] = 12.0
    bc[:, j2] = 12.0
    labels = np.where(np.arange(N) % 3 != 0, j1, j2).astype(np.int32)
    mask = (rng.random(N) < 0.5).astype(np.uint8)
    mask[:2] = 1
    return dict(Z=Z, Wc=Wc, bc=bc, labels=labels, mask=mask, row_weight=1.0 / int(mask.sum()))


def tie_expected_acc(case, j1, j2):
    """(accuracy, bound, pair_is_max) of a tie case under "first maximum wins"; pair_is_max: the margin of the pair
    over every other class exceeds twice the logit bound on every live row."""
    ref = classifier_ref(**case)
    others = np.delete(ref.logits, [j1, j2], axis=1)
    margin = ref.logits[:, j1] - (others.max(1) if others.shape[1] else -np.inf)
    ok = bool((margin[ref.live] > 2 * ref.e_logits.max(1)[ref.live]).all())
    acc = float((ref.w * (case["labels"] == j1)).sum())
    return acc, ref.e_acc, ok


def wide_range_case(D, C, HC, N=257):
    """Wc and bc scaled so that the largest |logit| is 80: exp(x - max) of the losing classes underflows."""
    rng = _rng(D, C, HC, N, 4)
    Z = rng.standard_normal((N, D), dtype=np.float32)
    Wc, bc = _weights(rng, D, C, HC)
    f = np.float32(80.0 / np.abs(up(Z) @ up(Wc).mean(0) + up(bc).mean(0)).max())
    Wc, bc = Wc * f, bc * f
    labels = rng.integers(0, C, N).astype(np.int32)
    mask = (rng.random(N) < 0.5).astype(np.uint8)
    mask[0] = 1
    return dict(Z=Z, Wc=Wc, bc=bc, labels=labels, mask=mask, row_weight=1.0 / int(mask.sum()))


def adam_state(n, seed=0):
    """A random fp32 state (p, g, m, v): magnitudes 1e-6 .. 1e3, v >= 0, every 7th element g = m = v = 0."""
    rng = np.random.default_rng([n, seed, 5])

    def mags():
        return (10.0 ** rng.uniform(-6, 3, n)).astype(np.float32)

    def signs():
        return rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)
    p, g, m, v = mags() * signs(), mags() * signs(), mags() * signs(), mags()
    z = np.arange(n) % 7 == 3
    g[z] = 0
    m[z] = 0
    v[z] = 0
    return p, g, m, v, z
