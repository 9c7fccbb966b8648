"""NumPy float64 reference of the silhouette kernel (han_silhouette) and the derived rounding bound of its outputs.

Reference: direct differences d_ij = sqrt(sum (x_i - x_j)^2) in float64, then, with n_c the size of cluster c and L the
cluster of row i,  S(i, c) = sum_{j in c} d_ij,  a = S(i, L) / (n_L - 1),  b = min_{c != L, n_c > 0} S(i, c) / n_c,
s = (b - a) / max(a, b);  s = 0 (and a = 0) for a cluster of one row, s = 0 when max(a, b) = 0.

Bound (u = 2^-24), from the pair bound of tests/test_evaluate_gpu.py: the kernel's d2 = |x_i|^2 + |x_j|^2 - 2 x_i.x_j in
fp32 is within tau_ij = 2 (D + 3) u (|x_i|^2 + |x_j|^2) of d_ij^2, so its square root is within
    e_ij = min(sqrt(tau_ij), tau_ij / d_ij) + 2 u d_ij                       (e_ii = 0: the kernel tests the index)
of d_ij;  e_S(i, c) = sum_{j in c} e_ij + (n_c + 3) u S(i, c) covers an fp32 sum in any order;  e_a = e_S(i, L) / (n_L - 1),
e_b = max_{c != L} e_S(i, c) / n_c, and with m = max(a, b):  |s^ - s| <= (e_a + e_b) / (m - max(e_a, e_b)).
A row with m <= 2 max(e_a, e_b) is undecided.  The score (mean of s) is within the mean of the row bounds + (N + 3) u.
"""
import numpy as np

U = 2.0 ** -24


def pair_distances(x):
    """(N, N) float64 distances by direct differences: eight rows at a time against the rows from there on (the
    temporaries stay in cache), the lower triangle mirrored from the upper one."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    d2 = np.zeros((n, n))
    for i in range(0, n, 8):
        diff = x[i:i + 8, None, :] - x[None, i:, :]
        np.einsum("ijk,ijk->ij", diff, diff, out=d2[i:i + 8, i:])
    d2 = np.triu(d2, 1)
    d2 += d2.T
    return np.sqrt(d2, out=d2)


def reference(x, codes, k=None):
    """dict(a, b, s, e_a, e_b, bound, undecided, score, score_bound) for fp32 rows x and cluster codes in [0, k);
    a code without rows is an empty cluster."""
    x32 = np.asarray(x, dtype=np.float32)
    codes = np.asarray(codes).astype(np.int64)
    n, dim = x32.shape
    k = int(codes.max()) + 1 if k is None else k
    d = pair_distances(x32)
    nrm = (x32.astype(np.float64) ** 2).sum(1)
    tau = 2 * (dim + 3) * U * (nrm[:, None] + nrm[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.minimum(np.sqrt(tau), np.where(d > 0, tau / d, np.inf)) + 2 * U * d
    e[np.arange(n), np.arange(n)] = 0.0
    counts = np.bincount(codes, minlength=k)
    onehot = np.zeros((n, k))
    onehot[np.arange(n), codes] = 1.0
    S = d @ onehot                                           # (N, k): a float64 sum per (row, cluster)
    eS = e @ onehot + (counts + 3)[None, :] * U * S
    rows = np.arange(n)
    n_own = counts[codes]
    a = np.where(n_own > 1, S[rows, codes] / np.maximum(n_own - 1, 1), 0.0)
    e_a = np.where(n_own > 1, eS[rows, codes] / np.maximum(n_own - 1, 1), 0.0)
    other = (counts[None, :] > 0) & (np.arange(k)[None, :] != codes[:, None])
    safe = np.maximum(counts, 1)[None, :]
    b = np.where(other, S / safe, np.inf).min(1)
    e_b = np.where(other, eS / safe, 0.0).max(1)
    m = np.maximum(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where((n_own > 1) & (m > 0), (b - a) / m, 0.0)
    worst = np.maximum(e_a, e_b)
    undecided = (m <= 2 * worst) & (n_own > 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(undecided, 2.0, (e_a + e_b) / (m - worst))
    bound = np.where(n_own > 1, bound, 0.0)                  # a cluster of one row: s = 0 exactly
    out = dict(a=a, b=b, s=s, e_a=e_a, e_b=e_b, bound=bound, undecided=undecided, score=float(s.mean()),
               score_bound=float(bound.mean() + (n + 3) * U))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def blobs(seed, sizes, dim, spread):
    """Gaussian blobs GROUPED BY CLUSTER: sizes[c] rows around centre c (centres drawn with `spread`, unit noise).
    Returns (x fp32, codes int64, seg_ptr int64 (k + 1))."""
    rs = np.random.RandomState(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    codes = np.repeat(np.arange(len(sizes)), sizes)
    centres = spread * rs.standard_normal((len(sizes), dim))
    x = (centres[codes] + rs.standard_normal((len(codes), dim))).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return x, codes, seg


def line_sums(v, codes, k):
    """S(i, c) = sum_{j in c} |v_i - v_j| for points v on a line, exactly (integers), by sorting and prefix sums."""
    v = np.asarray(v, dtype=np.int64)
    S = np.zeros((len(v), k), dtype=np.int64)
    for c in range(k):
        w = np.sort(v[codes == c])
        pre = np.concatenate([[0], np.cumsum(w)])
        le = np.searchsorted(w, v, side="right")
        S[:, c] = v * (2 * le - len(w)) - 2 * pre[le] + pre[-1]
    return S
