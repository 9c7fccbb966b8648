"""Host-side CSR plumbing shared by the graphs, the sparse features, the node partition and K0: plain functions on
tensors, torch only, on the device of their arguments.  A row pointer is (n + 1,) int64 with ptr[0] = 0; index
tensors come back int64 unless a dtype is asked for -- the callers cast to the widths their C entry points read."""
from __future__ import annotations

import torch


def scan(counts: torch.Tensor) -> torch.Tensor:
    """(n + 1,) int64 row pointer of the (n,) per-row counts: ptr[i + 1] - ptr[i] = counts[i]."""
    ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    if counts.numel():
        torch.cumsum(counts, 0, out=ptr[1:])
    return ptr


def row_ids(rowptr: torch.Tensor, dtype=torch.int64, base: int = 0) -> torch.Tensor:
    """(nnz,) the row of every entry, counted from `base`."""
    return torch.repeat_interleave(torch.arange(base, base + rowptr.numel() - 1, device=rowptr.device, dtype=dtype),
                                   rowptr[1:] - rowptr[:-1])


def group_by(keys: torch.Tensor, n_groups: int):
    """(ptr, order) of the int64 keys in [0, n_groups): `order` sorts them stably (the input order is kept inside a
    group), group k is order[ptr[k]:ptr[k + 1]].  Keys = the columns of a CSR matrix: its transposed image."""
    order = torch.sort(keys, stable=True).indices
    return scan(torch.bincount(keys, minlength=n_groups)), order


def chunk_table(ptr: torch.Tensor, longer_than: int, chunk: int, only: torch.Tensor | None = None):
    """The segments of `ptr` with more than `longer_than` entries (`only` (n,) bool: among the segments it marks) cut into
    chunks of `chunk` entries (a segment's last may be shorter, none is empty): None without such a segment, else dict(n_long, n_chunks, long (n_long,) segment
    ids, long_ptr (n_long + 1,) first chunk of each, chunk_long (n_chunks,) index into `long`, chunk_start / chunk_end
    (n_chunks,): chunk c covers entries [chunk_start[c], chunk_end[c])), int64.  One host read (n_chunks)."""
    lens = ptr[1:] - ptr[:-1]
    long = torch.nonzero(lens > longer_than if only is None else (lens > longer_than) & only).flatten()
    if long.numel() == 0:
        return None
    nch = (lens[long] + chunk - 1) // chunk
    long_ptr = scan(nch)
    n_chunks = int(long_ptr[-1])
    chunk_long = torch.repeat_interleave(torch.arange(long.numel(), device=ptr.device), nch)
    within = torch.arange(n_chunks, device=ptr.device) - long_ptr[:-1][chunk_long]
    chunk_start = (ptr[long][chunk_long] + within * chunk).contiguous()
    chunk_end = torch.minimum(chunk_start + chunk, ptr[long + 1][chunk_long]).contiguous()
    return dict(n_long=int(long.numel()), n_chunks=n_chunks, long=long, long_ptr=long_ptr, chunk_long=chunk_long,
                chunk_start=chunk_start, chunk_end=chunk_end)


def ragged_index(starts: torch.Tensor, lens: torch.Tensor) -> torch.Tensor:
    """Positions [starts[i], starts[i] + lens[i]) for every i, concatenated."""
    total = int(lens.sum())
    out_ptr = scan(lens)
    seg = torch.repeat_interleave(starts - out_ptr[:-1], lens)
    return seg + torch.arange(total, device=lens.device)


def from_sorted_keys(keys: torch.Tensor, n_rows: int, n_cols: int):
    """(rowptr, cols) of the ascending int64 entry keys row * n_cols + col; cols int64."""
    rows = keys // n_cols if keys.numel() else keys
    return scan(torch.bincount(rows, minlength=n_rows)), keys - rows * n_cols


def two_pass(n_rows: int, device, dtypes, count, fill):
    """Count / scan / fill construction of a CSR result, (rowptr, *entry arrays): `count(counts)` launches the kernel
    that writes the (n_rows,) int64 entry counts, the ONE host read takes nnz off the scanned row pointer, and
    `fill(rowptr, *arrays)` the kernel that writes the (nnz,) entry arrays, one per dtype of `dtypes`.  A result
    without entries needs no fill (and without rows neither count nor the host read): its arrays are empty."""
    counts = torch.empty(n_rows, dtype=torch.int64, device=device)
    if n_rows:
        count(counts)
    rowptr = scan(counts)
    nnz = int(rowptr[-1]) if n_rows else 0
    arrays = [torch.empty(nnz, dtype=d, device=device) for d in dtypes]
    if nnz:
        fill(rowptr, *arrays)
    return (rowptr, *arrays)
