"""NumPy / scipy references of the weighted meta-path graphs (K0 counts, PathSim, per-row top-k), shared by
tests/test_metapath_weights_host.py (which checks them against brute-force dense computations) and
tests/test_metapath_weights_gpu.py (which checks the kernels against them)."""
import numpy as np
import scipy.sparse as sp


def counted(m, diag=False):
    """Canonical CSR (int64 data, sorted unique indices) of the integer matrix `m` with positive stored sums; with diag
    every (i, i) is stored, with value 0 where `m` has none -- the layout of ops.csr_count_matmul."""
    m = sp.csr_matrix(m, dtype=np.int64)
    m.sum_duplicates()
    m.eliminate_zeros()
    if diag:
        m = sp.csr_matrix(m + sp.identity(m.shape[0], dtype=np.int64, format="csr"))     # no stored sum becomes 0
        m.sort_indices()
        rows = np.repeat(np.arange(m.shape[0]), np.diff(m.indptr))
        m.data = m.data - (m.indices == rows)
    m.sort_indices()
    return m


def count_chain(mats, diag=False):
    """The int64 product of the chain `mats` (scipy matrices, left to right), as counted()."""
    m = sp.csr_matrix(mats[0], dtype=np.int64)
    for r in mats[1:]:
        m = sp.csr_matrix(m @ sp.csr_matrix(r, dtype=np.int64))
    return counted(m, diag)


def pathsim(indptr, indices, counts):
    """fp32 PathSim of a square counted CSR: (2.0 * c / (d[i] + d[j])).astype(float32), 1 on the diagonal."""
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    on_diag = indices == rows
    d = np.zeros(n, dtype=np.int64)
    d[rows[on_diag]] = counts[on_diag]
    with np.errstate(invalid="ignore", divide="ignore"):
        w = (2.0 * counts / (d[rows] + d[indices])).astype(np.float32)
    w[on_diag] = 1.0
    return w


def topk_row(cols, w, i, k, keep_diag=True):
    """Positions (ascending) of the entries of row i that a top-k cut keeps: the first k of np.lexsort((col, -w)) over
    the entries off the diagonal -- largest value first, ties to the smaller column -- and (i, i) with keep_diag."""
    cols, w = np.asarray(cols), np.asarray(w)
    off = np.nonzero(cols != i)[0]
    order = np.lexsort((cols[off], -w[off].astype(np.float64)))
    keep = off[order[:k]]
    if keep_diag:
        keep = np.concatenate([keep, np.nonzero(cols == i)[0]])
    return np.sort(keep)


def topk(indptr, indices, w, k, keep_diag=True):
    """(indptr, indices, values) of the top-k cut of every row."""
    keeps = [indptr[i] + topk_row(indices[indptr[i]:indptr[i + 1]], w[indptr[i]:indptr[i + 1]], i, k, keep_diag)
             for i in range(len(indptr) - 1)]
    out_ptr = np.zeros(len(indptr), dtype=np.int64)
    out_ptr[1:] = np.cumsum([len(x) for x in keeps])
    sel = np.concatenate(keeps) if keeps else np.zeros(0, dtype=np.int64)
    return out_ptr, indices[sel], w[sel]
