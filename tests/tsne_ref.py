"""NumPy float64 reference of the t-SNE kernels (han_tsne_calibrate, han_tsne_step) and the derived bounds of the
calibration outputs.  It restates scikit-learn's TSNE(method="exact"): _utils._binary_search_perplexity,
_joint_probabilities, _kl_divergence (one degree of freedom, two components) and _gradient_descent;
tests/test_tsne_host.py holds it against those functions themselves.

Everything works on a subset `rows` of the rows against all N columns, so a large case can be checked on a sample:
d2 is (R, N), by direct differences in float64.  With the kernel's own (beta, dmin, zsum) of every row,
    c_ij = exp(-beta_i (d2_ij - dmin_i)) / zsum_i,   p_ij = max((c_ij + c_ji) / (2 N), 2^-52),   p_ii = 0,
    dy = y_i - y_j,  w = 1 / (1 + |dy|^2),  w_ii = 0,  Z_q = sum_ij w,
    grad_i = 4 (sum_j e p w dy - sum_j w^2 dy / Z_q),   KL = sum_ij e p (log(e p) - log w + log Z_q).

Bounds (u = 2^-24), from the pair bound of tests/test_evaluate_gpu.py and tests/silhouette_ref.py: the kernel's
d2 = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) in fp32 is within tau_ij = 2 (D + 3) u (|x_i|^2 + |x_j|^2) of d2_ij.
  dmin:  |min_j a_j - min_j b_j| <= max_j |a_j - b_j|, so |dmin_i - min_j d2_ij| <= max_j tau_ij.
  zsum:  given the kernel's beta_i and dmin_i, Z_i = sum_j t_j with t_j = exp(-a_j), a_j = beta_i (d2_ij - dmin_i).  The
         kernel's term differs by the factor exp(-beta_i (d2^_ij - d2_ij)), within expm1(beta_i tau_ij) of 1; its
         exponent (a difference, the product with beta log2 e, itself rounded) carries a relative 3 u, an absolute
         3 u a_j, and the hardware exp2 one more u: 4 u (1 + a_j) t_j.  A tile's fp32 sum of at most 16 terms, the
         double sums and the store as fp32 are covered by 20 u Z_i; terms below 2^-126 may be flushed:
             e_Z(i) = sum_j t_j (expm1(beta_i tau_ij) + 4 u (1 + a_j)) + 20 u Z_i + N 2^-126.
"""
import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -52           # MACHINE_EPSILON of sklearn.manifold._t_sne


def d2_rows(x, rows=None, block=32):
    """(R, N) float64 squared distances of the rows `rows` (all by default) to every row, by direct differences"""
    x = np.asarray(x, dtype=np.float64)
    rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    out = np.empty((len(rows), x.shape[0]))
    for s in range(0, len(rows), block):
        diff = x[rows[s:s + block], None, :] - x[None, :, :]
        np.einsum("ijk,ijk->ij", diff, diff, out=out[s:s + block])
    return out


def tau_rows(x, rows=None):
    """(R, N) bound of the kernel's fp32 d2 against d2_rows"""
    x = np.asarray(x, dtype=np.float64)
    rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    nrm = (x ** 2).sum(1)
    return 2 * (x.shape[1] + 3) * U * (nrm[rows, None] + nrm[None, :])


def _others(rows, n):
    """(R, N) mask of the pairs j != i"""
    m = np.ones((len(rows), n), dtype=bool)
    m[np.arange(len(rows)), rows] = False
    return m


def entropy(d2, rows, beta):
    """(H, Z, m) of the rows' conditional distributions at beta (R,): distances shifted by the row minimum m"""
    other = _others(rows, d2.shape[1])
    m = np.where(other, d2, np.inf).min(1)
    a = np.asarray(beta, dtype=np.float64)[:, None] * (d2 - m[:, None])
    t = np.where(other, np.exp(-a), 0.0)
    z = t.sum(1)
    return np.log(z) + (a * t).sum(1) / z, z, m


def bisect(d2, perplexity, tol=1e-5, max_passes=100):
    """_binary_search_perplexity for all rows of a square d2 in float64: (beta, passes until every row closed)"""
    n = d2.shape[0]
    rows = np.arange(n)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    open_ = np.ones(n, dtype=bool)
    target = np.log(perplexity)
    passes = 0
    while open_.any() and passes < max_passes:
        passes += 1
        diff = entropy(d2, rows, beta)[0] - target
        open_ &= np.abs(diff) > tol
        up, down = open_ & (diff > 0), open_ & ~(diff > 0)
        lo[up] = beta[up]
        hi[down] = beta[down]
        with np.errstate(invalid="ignore"):
            beta = np.where(up, np.where(np.isinf(hi), beta * 2, (beta + hi) / 2), beta)
            beta = np.where(down, np.where(np.isinf(lo), beta / 2, (beta + lo) / 2), beta)
    return beta, passes


def joint_rows(d2, rows, beta, dmin, zsum):
    """(R, N) p_ij of the rows from the per-row (beta, dmin, zsum) of ALL rows; p_ii = 0"""
    beta, dmin, zsum = (np.asarray(v, dtype=np.float64) for v in (beta, dmin, zsum))
    n = d2.shape[1]
    ci = np.exp(-beta[rows, None] * (d2 - dmin[rows, None])) / zsum[rows, None]
    cj = np.exp(-beta[None, :] * (d2 - dmin[None, :])) / zsum[None, :]
    return np.where(_others(rows, n), np.maximum((ci + cj) / (2 * n), EPS), 0.0)


def joint(d2, perplexity):
    """the float64 joint probabilities of a square d2: bisection, then joint_rows; (P, beta, passes)"""
    rows = np.arange(d2.shape[0])
    beta, passes = bisect(d2, perplexity)
    _, z, m = entropy(d2, rows, beta)
    return joint_rows(d2, rows, beta, m, z), beta, passes


def step_rows(p, y, rows=None, exaggeration=1.0, zq=None):
    """(grad (R, 2), W (R,), KL terms (R,), Z_q) of _kl_divergence for the rows `rows` given their p (R, N) and all of y.
    zq=None: the rows are all rows and Z_q is their sum of W."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    other = _others(rows, n)
    dy = y[rows, None, :] - y[None, :, :]
    w = np.where(other, 1.0 / (1.0 + (dy ** 2).sum(2)), 0.0)
    big_w = w.sum(1)
    if zq is None:
        assert len(rows) == n
        zq = big_w.sum()
    ep = exaggeration * p
    grad = 4.0 * (((ep * w)[:, :, None] * dy).sum(1) - ((w * w)[:, :, None] * dy).sum(1) / zq)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(other, ep * (np.log(ep) - np.log(w) + np.log(zq)), 0.0).sum(1)
    return grad, big_w, kl, zq


def zq_blocked(y, block=1024):
    """Z_q = sum over i != j of 1 / (1 + |y_i - y_j|^2) in float64, a block of rows against the rows after it"""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    total = 0.0
    for s in range(0, n, block):
        a, b = y[s:s + block], y[s:]
        q = 1.0 / (1.0 + np.subtract.outer(a[:, 0], b[:, 0]) ** 2 + np.subtract.outer(a[:, 1], b[:, 1]) ** 2)
        inner = q[:, :len(a)]
        total += 2.0 * (q[:, len(a):].sum() + np.triu(inner, 1).sum())
    return total


def zq_lattice(y, size):
    """Z_q of INTEGER points y in [0, size)^2, exactly: the number of ordered pairs at every offset (dx, dy) is the
    autocorrelation of the occupancy histogram (integers, via a zero-padded FFT and rounding), each pair weighs
    1 / (1 + dx^2 + dy^2), and the N pairs (i, i) at offset (0, 0) are taken out.  O(size^2 log size) where zq_blocked
    costs O(N^2); tests/test_tsne_host.py holds the two against each other."""
    yi = np.asarray(y).astype(np.int64)
    assert (yi == np.asarray(y)).all() and yi.min() >= 0 and yi.max() < size
    hist = np.zeros((2 * size, 2 * size))
    np.add.at(hist, (yi[:, 0], yi[:, 1]), 1.0)
    f = np.fft.rfft2(hist)
    corr = np.rint(np.fft.irfft2(f * np.conj(f), s=hist.shape))            # corr[dx mod 2 size, dy mod 2 size]
    off = np.fft.fftfreq(2 * size, 1.0 / (2 * size))                       # 0 .. size - 1, -size .. -1
    w = 1.0 / (1.0 + off[:, None] ** 2 + off[None, :] ** 2)
    assert corr.sum() == float(len(yi)) ** 2
    return float((corr * w).sum() - len(yi))


def update_rule(y, update, gains, grad, momentum, lr, min_gain=0.01, dtype=np.float64):
    """_gradient_descent's update, elementwise in `dtype` (float32: every product and sum rounded on its own, the form
    the kernel must equal bit for bit).  Returns (y, update, gains, gains * grad) as new arrays."""
    f = dtype
    y, update, gains, grad = (np.array(v, dtype=f) for v in (y, update, gains, grad))
    inc = update * grad < 0
    gains = np.where(inc, gains + f(0.2), gains * f(0.8)).astype(f)
    gains = np.maximum(gains, f(min_gain))
    gg = gains * grad
    update = f(momentum) * update - f(lr) * gg
    return y + update, update, gains, gg


def descend(p, y, n_iter, exaggeration, momentum, lr, min_gain=0.01):
    """n_iter iterations of _gradient_descent in float64 from y with update = 0 and gains = 1; (y, KL at the last
    iterate the loop evaluated -- the one BEFORE the last update, as scikit-learn reports it)"""
    y = np.array(y, dtype=np.float64)
    update, gains = np.zeros_like(y), np.ones_like(y)
    kl = np.nan
    for _ in range(n_iter):
        grad, _, kl_rows, _ = step_rows(p, y, None, exaggeration)
        kl = kl_rows.sum()
        y, update, gains, _ = update_rule(y, update, gains, grad, momentum, lr, min_gain)
    return y, kl


def tsne(p, y, max_iter=1000, early_exaggeration=12.0, lr=None, exploration=250):
    """scikit-learn's schedule without its stopping rules: `exploration` exaggerated iterations at momentum 0.5, the
    rest at 0.8 with update and gains reset; returns the final y"""
    n = p.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if lr is None else lr
    y, _ = descend(p, y, min(exploration, max_iter), early_exaggeration, 0.5, lr)
    if max_iter > exploration:
        y, _ = descend(p, y, max_iter - exploration, 1.0, 0.8, lr)
    return y


def kl_of(p, y):
    """KL(P || Q(y)) under the given float64 P"""
    return float(step_rows(p, y)[2].sum())


def calib_bounds(d2, tau, rows, beta, dmin):
    """For the rows `rows`, their d2_rows / tau_rows and the kernel's beta, dmin (of all rows): dict(dmin -- the float64
    row minimum --, e_dmin, zsum -- the float64 Z at the kernel's beta and dmin --, e_zsum, perplexity -- exp of the
    entropy the kernel's beta realises on the float64 distances)."""
    rows = np.asarray(rows)
    n = d2.shape[1]
    other = _others(rows, n)
    b = np.asarray(beta, dtype=np.float64)[rows]
    a = b[:, None] * (d2 - np.asarray(dmin, dtype=np.float64)[rows, None])
    t = np.where(other, np.exp(-a), 0.0)
    z = t.sum(1)
    e_z = (t * (np.expm1(b[:, None] * tau) + 4 * U * (1 + np.abs(a)))).sum(1) + 20 * U * z + n * 2.0 ** -126
    h = entropy(d2, rows, b)[0]
    return dict(dmin=np.where(other, d2, np.inf).min(1), e_dmin=np.where(other, tau, 0.0).max(1), zsum=z,
                e_zsum=e_z, perplexity=np.exp(h))


def blobs(seed, n, dim, centres=4, spread=3.0):
    """n fp32 rows around `centres` Gaussian centres (drawn with `spread`, unit noise), and their labels"""
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, centres, n)
    c = spread * rs.standard_normal((centres, dim))
    return (c[labels] + rs.standard_normal((n, dim))).astype(np.float32), labels.astype(np.int64)


def trustworthiness(x, y, n_neighbors=5):
    """sklearn.manifold.trustworthiness(x, y, n_neighbors=k), Euclidean: 1 - 2 / (n k (2 n - 3 k - 1)) times the sum,
    over the k nearest neighbours j of i in y, of max(0, rank of j among the neighbours of i in x - k)"""
    n, k = len(x), n_neighbors
    dx, dy = d2_rows(x), d2_rows(y)
    np.fill_diagonal(dx, np.inf)
    np.fill_diagonal(dy, np.inf)
    order_x = np.argsort(dx, axis=1, kind="stable")
    rank_x = np.empty((n, n), dtype=np.int64)
    rank_x[np.arange(n)[:, None], order_x] = np.arange(1, n + 1)[None, :]      # 1 = the nearest
    near_y = np.argsort(dy, axis=1, kind="stable")[:, :k]
    t = np.maximum(rank_x[np.arange(n)[:, None], near_y] - k, 0).sum()
    return 1.0 - t * 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))
