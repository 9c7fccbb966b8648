"""Sparse node features: an immutable (N, F) CSR matrix on one device, the input of the first-layer projection.

The features heterogeneous-graph data sets carry are bag-of-words rows (ACM 1870 columns, DBLP 334, IMDB about
1.2 k), almost all zero.  A :class:`SparseFeatures` is accepted wherever a dense feature tensor is
(``HeteGAT_multi.inference`` / ``forward``, ``HANTrainer(xs=...)``, the single-head functions of ``layers``) and
runs the projection on the stored entries only (``csrc/project_sparse.hip``), with the dropout draws of the dense
kernels.  Nothing else in the model reads the features.
"""
from __future__ import annotations

import numpy as np
import torch

from . import csr

_LIM = 1 << 31


class SparseFeatures:
    """rowptr (N+1,) int64, colidx (nnz,) int32, values (nnz,) fp32 or None (every stored entry is 1: binary
    bag-of-words, 4 bytes per entry less).  Canonical: columns ascending within a row, no repeated entry (the
    constructors sum duplicates); stored zeros are kept -- they contribute nothing.  Build one with from_dense /
    from_torch_sparse / from_scipy / from_arrays."""

    dtype = torch.float32

    def __init__(self, rowptr: torch.Tensor, colidx: torch.Tensor, values: torch.Tensor | None, n_cols: int):
        """Takes canonical, validated arrays as they are (the constructors below produce them)."""
        self.rowptr, self.colidx, self.values = rowptr, colidx, values
        self.n_rows, self.n_cols = rowptr.numel() - 1, int(n_cols)
        self.nnz = colidx.numel()
        self._t = {}

    # ---- tensor-like surface ------------------------------------------------------
    @property
    def shape(self):
        return (self.n_rows, self.n_cols)

    @property
    def device(self):
        return self.rowptr.device

    @property
    def is_cuda(self) -> bool:
        return self.rowptr.is_cuda

    def to(self, device) -> "SparseFeatures":
        device = torch.device(device)
        if device == self.device:
            return self
        return SparseFeatures(self.rowptr.to(device), self.colidx.to(device),
                              self.values.to(device) if self.values is not None else None, self.n_cols)

    def __repr__(self):
        return (f"SparseFeatures(shape={self.shape}, nnz={self.nnz}, "
                f"{'binary' if self.values is None else 'float32'}, device={self.device})")

    def to_dense(self) -> torch.Tensor:
        """(N, F) fp32 -- for tests."""
        out = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
        vals = self.values if self.values is not None else torch.ones(self.nnz, dtype=torch.float32, device=self.device)
        out[csr.row_ids(self.rowptr), self.colidx.long()] = vals
        return out

    def rows(self, r0: int, r1: int) -> "SparseFeatures":
        """Rows [r0, r1): views of colidx / values with a rebased rowptr."""
        r0, r1 = int(r0), int(r1)
        if not (0 <= r0 <= r1 <= self.n_rows):
            raise ValueError(f"rows ({r0}, {r1}) outside [0, {self.n_rows}]")
        b, e = int(self.rowptr[r0]), int(self.rowptr[r1])
        return SparseFeatures(self.rowptr[r0:r1 + 1] - b, self.colidx[b:e],
                              self.values[b:e] if self.values is not None else None, self.n_cols)

    def take(self, ids) -> "SparseFeatures":
        """The rows `ids` (1-D integer tensor or array; any order, repeats allowed) as a new matrix, in the given
        order: the features of the nodes of an ego block (minibatch.EgoBlock.take).  GPU only: the count / fill
        kernels of the block graphs with every row kept and no column map (han_ego_count / han_ego_fill), one host
        read for the new nnz (csr.two_pass) and one for the range of `ids`."""
        from . import ops
        ops.require_gpu(self.rowptr, "SparseFeatures.take")
        ids = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
            raise ValueError(f"ids: expected a 1-D integer array of row ids, got {tuple(ids.shape)} {ids.dtype}")
        ids = ids.to(device=self.device, dtype=torch.int64).contiguous()
        if ids.numel():
            lo, hi = torch.stack([ids.min(), ids.max()]).tolist()
            if lo < 0 or hi >= self.n_rows:
                raise ValueError(f"ids outside [0, {self.n_rows}): [{lo}, {hi}]")
        dtypes = (torch.int32,) if self.values is None else (torch.int32, torch.float32)
        out = csr.two_pass(
            ids.numel(), self.device, dtypes,
            lambda counts: ops.ego_count(self.rowptr, ids, counts),
            lambda rowptr, colidx, values=None: ops.ego_fill(self.rowptr, self.colidx, self.values, ids, self.n_cols,
                                                             rowptr, colidx, values))
        return SparseFeatures(out[0], out[1], out[2] if self.values is not None else None, self.n_cols)

    # ---- the transposed image of the backward ------------------------------------
    def transposed(self) -> dict:
        """The CSC image dW gathers through (ops.project_bwd), built once with torch ops on the first backward and
        cached: colptr (F+1,) int64, rowidx (nnz,) int32 ascending within a column, values_t (or None), and the
        chunk table of the columns longer than ops.SPARSE_COL_CHUNK entries, in the manner of CSRGraph.row_split:
        long_cols (n_long,) int32, long_ptr (n_long+1,) int64, chunk_col (n_chunks,) int32, chunk_start / chunk_end
        (n_chunks,) int64 -- chunk c covers the entries [chunk_start[c], chunk_end[c]) of column chunk_col[c]."""
        from . import ops
        chunk = int(ops.SPARSE_COL_CHUNK)
        hit = self._t.get(chunk)
        if hit is not None:
            return hit
        # the rows are stored in ascending order, so a stable sort by column leaves every column's rows ascending
        colptr, order = csr.group_by(self.colidx.long(), self.n_cols)
        rowidx = csr.row_ids(self.rowptr)[order].to(torch.int32).contiguous()
        values_t = self.values[order].contiguous() if self.values is not None else None
        t = dict(colptr=colptr, rowidx=rowidx, values_t=values_t, col_chunk=chunk, n_long=0, n_chunks=0,
                 long_cols=None, long_ptr=None, chunk_col=None, chunk_start=None, chunk_end=None)
        c = csr.chunk_table(colptr, chunk, chunk)
        if c is not None:       # the index arrays in the int32 that han_project_sparse_bwd reads
            t.update(n_long=c["n_long"], n_chunks=c["n_chunks"], long_cols=c["long"].to(torch.int32),
                     long_ptr=c["long_ptr"], chunk_col=c["long"][c["chunk_long"]].to(torch.int32),
                     chunk_start=c["chunk_start"], chunk_end=c["chunk_end"])
        if self.is_cuda:
            # the image is shared by every later launch, whichever stream it runs on (one stream per meta-path in a
            # captured epoch): it is complete before anybody sees it.  (Built outside a capture: the warm-up epoch.)
            torch.cuda.current_stream(self.device).synchronize()
        self._t[chunk] = t
        return t

    # ---- constructors ---------------------------------------------------------------
    @staticmethod
    def _from_coo(rows, cols, vals, n_rows, n_cols) -> "SparseFeatures":
        """Canonical matrix of the entries (rows[e], cols[e], vals[e] or 1): int64 index tensors on one device."""
        n_rows, n_cols = int(n_rows), int(n_cols)
        if n_rows < 0 or n_cols < 1 or n_rows >= _LIM or n_cols >= _LIM:
            raise ValueError(f"shape ({n_rows}, {n_cols}): N must be in [0, 2^31) and F in [1, 2^31)")
        dev = rows.device
        nnz = rows.numel()
        if cols.numel() != nnz:
            raise ValueError(f"{rows.numel()} row indices for {cols.numel()} column indices")
        if vals is not None:
            if vals.shape != (nnz,):
                raise ValueError(f"values: shape {tuple(vals.shape)}, expected ({nnz},)")
            vals = vals.to(device=dev, dtype=torch.float32)
            if nnz and not bool(torch.isfinite(vals).all()):
                bad = int(torch.nonzero(~torch.isfinite(vals)).flatten()[0])
                raise ValueError(f"values must be finite: entry {bad} is {float(vals[bad])}")
        if nnz:
            lo, hi = int(cols.min()), int(cols.max())
            if lo < 0 or hi >= n_cols:
                raise ValueError(f"column index out of range [0,{n_cols}): [{lo},{hi}]")
            lo, hi = int(rows.min()), int(rows.max())
            if lo < 0 or hi >= n_rows:
                raise ValueError(f"row index out of range [0,{n_rows}): [{lo},{hi}]")
        key = rows * n_cols + cols                          # < 2^62
        if nnz > 1 and not bool((key[1:] > key[:-1]).all()):      # unsorted columns and / or repeated entries
            key, order = torch.sort(key, stable=True)
            uniq, inverse = torch.unique_consecutive(key, return_inverse=True)
            if uniq.numel() != nnz:                         # duplicates are summed (a repeated binary entry counts twice)
                src = vals[order] if vals is not None else torch.ones(nnz, dtype=torch.float32, device=dev)
                vals = torch.zeros(uniq.numel(), dtype=torch.float32, device=dev).index_add_(0, inverse, src)
            elif vals is not None:
                vals = vals[order]
            rows, cols = torch.div(uniq, n_cols, rounding_mode="floor"), uniq % n_cols
        return SparseFeatures(csr.scan(torch.bincount(rows, minlength=n_rows)), cols.to(torch.int32).contiguous(),
                              vals.contiguous() if vals is not None else None, n_cols)

    @staticmethod
    def from_arrays(rowptr, colidx, values, n_cols, device=None) -> "SparseFeatures":
        """From CSR arrays (tensors, NumPy arrays or sequences); values None = all ones.  Validates like CSRGraph:
        rowptr starts at 0, ends at nnz and never decreases, 0 <= col < n_cols, N and F below 2^31, finite values."""
        def as_t(a, dtype):
            if isinstance(a, torch.Tensor):
                return a.to(device=device if device is not None else a.device, dtype=dtype)
            return torch.as_tensor(np.asarray(a), device=device).to(dtype)
        rp, ci = as_t(rowptr, torch.int64), as_t(colidx, torch.int64)
        if rp.dim() != 1 or ci.dim() != 1 or rp.numel() < 1:
            raise ValueError(f"rowptr / colidx must be 1-D with len(rowptr) >= 1; got {tuple(rp.shape)}, {tuple(ci.shape)}")
        if rp.device != ci.device:
            raise ValueError(f"rowptr on {rp.device}, colidx on {ci.device}")
        if int(rp[0]) != 0 or int(rp[-1]) != ci.numel():
            raise ValueError(f"rowptr[0] must be 0 and rowptr[-1] == nnz; got {int(rp[0])}, {int(rp[-1])} for {ci.numel()} entries")
        deg = rp[1:] - rp[:-1]
        if deg.numel() and bool((deg < 0).any()):
            bad = int(torch.nonzero(deg < 0).flatten()[0])
            raise ValueError(f"rowptr must be non-decreasing: rowptr[{bad + 1}] = {int(rp[bad + 1])} < rowptr[{bad}] = {int(rp[bad])}")
        rows = csr.row_ids(rp)
        vals = as_t(values, torch.float32) if values is not None else None
        return SparseFeatures._from_coo(rows, ci, vals, deg.numel(), n_cols)

    @staticmethod
    def from_dense(t: torch.Tensor) -> "SparseFeatures":
        """The non-zero elements of a dense (N,F) or (1,N,F) tensor, on its device."""
        if t.dim() == 3 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 2:
            raise ValueError(f"expected (N,F) or (1,N,F), got {tuple(t.shape)}")
        idx = torch.nonzero(t)                # row-major order: canonical already
        return SparseFeatures._from_coo(idx[:, 0], idx[:, 1], t[idx[:, 0], idx[:, 1]], t.shape[0], t.shape[1])

    @staticmethod
    def from_torch_sparse(t: torch.Tensor) -> "SparseFeatures":
        """From a torch sparse COO or CSR tensor of shape (N,F) or (1,N,F)."""
        if t.dim() == 3 and t.shape[0] != 1:
            raise ValueError(f"batch size must be 1, got shape {tuple(t.shape)}")
        if t.dim() not in (2, 3):
            raise ValueError(f"expected (N,F) or (1,N,F), got {tuple(t.shape)}")
        n_rows, n_cols = t.shape[-2], t.shape[-1]
        if t.layout == torch.sparse_coo:
            idx = t.indices() if t.is_coalesced() else t._indices()
            vals = t.values() if t.is_coalesced() else t._values()
            return SparseFeatures._from_coo(idx[-2], idx[-1], vals, n_rows, n_cols)
        if t.layout == torch.sparse_csr:
            crow, col, vals = t.crow_indices(), t.col_indices(), t.values()
            if t.dim() == 3:
                crow, col, vals = crow[0], col[0], vals[0]
            return SparseFeatures.from_arrays(crow, col, vals, n_cols)
        raise ValueError(f"expected a sparse COO or CSR tensor, got layout {t.layout}")

    @staticmethod
    def from_scipy(m, device=None) -> "SparseFeatures":
        """From a scipy.sparse matrix (any format)."""
        m = m.tocsr()
        return SparseFeatures.from_arrays(m.indptr, m.indices, np.asarray(m.data, dtype=np.float32), m.shape[1],
                                          device=device)


_converted: dict = {}      # id(sparse tensor) -> (the tensor, its SparseFeatures): converted once per tensor identity
_CONVERTED_MAX = 16


def is_sparse_input(x) -> bool:
    """True for what the sparse projection serves: a SparseFeatures or a torch sparse COO / CSR tensor."""
    return isinstance(x, SparseFeatures) or (isinstance(x, torch.Tensor)
                                             and x.layout in (torch.sparse_coo, torch.sparse_csr))


def as_features(x):
    """A feature argument as the layers use it: a SparseFeatures as it is, a torch sparse COO / CSR tensor of shape
    (N,F) / (1,N,F) converted once and cached by identity (the way HeteGAT_multi._graphs caches masks), anything else
    (a dense tensor) unchanged."""
    if not (isinstance(x, torch.Tensor) and is_sparse_input(x)):
        return x
    hit = _converted.get(id(x))
    if hit is None or hit[0] is not x:
        if len(_converted) >= _CONVERTED_MAX:
            _converted.pop(next(iter(_converted)))
        hit = (x, SparseFeatures.from_torch_sparse(x))
        _converted[id(x)] = hit
    return hit[1]
