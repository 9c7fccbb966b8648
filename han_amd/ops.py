"""Thin, validating Python wrappers over the C ABI (one per entry point).

Tensors are plumbing: device memory + the current HIP stream.  Every wrapper
checks device / dtype / contiguity / shape and raises ``ValueError`` before the
kernel sees the pointers (the kernels assume validated input).
"""
from __future__ import annotations

import contextlib
import ctypes

import torch

from . import _lib, csr
from .features import SparseFeatures
from .graph import CSRGraph

ACT_IDENTITY = 0
ACT_ELU = 1
FLAG_XCD_ORDER = 1         # HAN_FLAG_XCD_ORDER: XCD-aware work order for graphs with locality
FLAG_LEAN = 256            # HAN_FLAG_LEAN: the lean K2 kernels of small graphs (scores read from the table, shared dropout hash, one lane per head at 8 x 8)
FLAG_K2_DEEP = 512         # HAN_FLAG_K2_DEEP (measurements: bf16 eval forward with 8 steps in flight)
K2_DEEP = False            # set by tools/k2_regimes.py --deep
K2_SHARED_HASH = False     # tests / measurements: FLAG_K2_SHARED_HASH on every node_attn_fwd call
K2_FULL_GATHER = False     # tests / measurements: FLAG_K2_FULL_GATHER on every node_attn_bwd_cols call
FLAG_K2_FULL_GATHER = 2048 # HAN_FLAG_K2_FULL_GATHER: measurements only (the backward gather requests g rows whole, dropped heads included)
FLAG_K2_ZERO_ROWS = 4096   # HAN_FLAG_K2_ZERO_ROWS: most rows of the gs table hold a zero gradient; the predicated backward gather honours z
GS_Z_ALL_ZERO = 0x3F800000 # HAN_GS_Z_ALL_ZERO: fourth word of a head's statistics record when all g values of the head are +-0 (else 0)
FLAG_K2_ROW_SUBSET = 8192  # HAN_FLAG_K2_ROW_SUBSET: the row lists of the split are all the rows han_node_attn_fwd computes
FLAG_MASKED_EDGES = 64     # HAN_FLAG_MASKED_EDGES: negative entries of the transposed graph are skipped in place
FLAG_K1_EXACT_PIPE = 2     # HAN_FLAG_K1_EXACT_PIPE / _MATRIX_PIPE: force one of the two K1 forward kernels (tests, measurements)
FLAG_K1_MATRIX_PIPE = 4
FLAG_K1_4WAVE = 16         # HAN_FLAG_K1_4WAVE (measurements: the two-waves-per-SIMD form of the bf16 x 6 kernel)
FLAG_K1_PAIRS = 32         # HAN_FLAG_K1_PAIRS (measurements: project_fwd_multi fuses 2 meta-paths per block, not 4)
FLAG_K3_EXACT_PIPE = 8     # HAN_FLAG_K3_EXACT_PIPE: fp32 MFMA K3 kernels also for large inputs
FLAG_K2_SHARED_HASH = 1024 # HAN_FLAG_K2_SHARED_HASH: measurements only (one attention-dropout hash per edge and four heads)
FLAG_K3_PAIRS = 16         # HAN_FLAG_K3_PAIRS: measurements only (two waves share a tile in the K3 backward)
FLAG_K3_G3_F32 = 32        # HAN_FLAG_K3_G3_F32: measurements only (dW product of the K3 backward on the fp32 pipe)


def flag_fts_slice(s: int) -> int:
    """HAN_FLAG_FTS_SLICE(s): column slice s of a head wider than 64 columns (project_fwd: the projected-row
    dropout of slice s draws from stream 2 + 4 s; everything else is keyed as for slice 0)."""
    if not 0 <= s < 256:
        raise ValueError("at most 256 slices of 64 columns per head")
    return (int(s) & 0xFF) << 8


LEAKY_SLOPE = 0.2          # tf.nn.leaky_relu default (utils/layers.py:27)
D = 64                     # K * F' of this build
STATS_ROW_BYTES = 128      # per destination row: the (f1, lse, s, z) records of the K = 8 heads inside the fused gs row (bench.py byte model)

_workspaces: dict = {}
_retired_workspaces: list = []      # superseded buffers stay alive: a captured hipGraph may have baked their pointers in

# Optional timing hook (bench.py): a list to which node_attn_fwd / node_attn_bwd_cols
# append (tag, start_event, end_event, N, E) recorded on the launch stream.
K2_TIMING: list | None = None


def _ptr(t):
    """Device pointer of an optional tensor (NULL for None)."""
    return t.data_ptr() if t is not None else None


def _ptr_nonempty(t):
    """Device pointer of an optional tensor that may be empty, as the graphs K0 takes (NULL for None or no elements)."""
    return t.data_ptr() if t is not None and t.numel() else None


class _k2_timed:
    """Bracket a K2 launch with the timing events of K2_TIMING (nothing when it is None)."""

    def __init__(self, tag, n_rows, nnz):
        self.sink, self.rec = K2_TIMING, (tag, n_rows, nnz)

    def __enter__(self):
        if self.sink is not None:
            self.ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.ev[0].record()

    def __exit__(self, *exc):
        if self.sink is not None:
            self.ev[1].record()
            self.sink.append((self.rec[0],) + self.ev + self.rec[1:])


def _dev_word(t):
    """Device pointer of a 1-element int64 tensor (seed_dev / step_dev of the C ABI), or None."""
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.numel() == 1):
        raise ValueError("seed_dev / step_dev must be a 1-element int64 GPU tensor")
    return t.data_ptr()


def _out(t, name, shape, dev):
    """A caller-provided destination (e.g. a slice of the flat gradient buffer) or a fresh tensor."""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=dev)
    _chk(t, name, tuple(shape), device=dev)
    return t


def _stream():
    return torch.cuda.current_stream().cuda_stream


WS_SUFFIX = ""             # set by branch(): kernels that run concurrently (one stream per meta-path inside a captured epoch,
                           # the side stream, the eval branch) must not share a scratch buffer


@contextlib.contextmanager
def branch(stream, suffix=""):
    """Run the enclosed launches on `stream` (None: in place) with scratch buffers of their own: `suffix` is appended
    to every workspace tag (_ws).  Scopes nest, suffixes in nesting order.  The caller orders the streams (fork before,
    join after); the suffix is the caller's too, since an in-place branch may still need its own buffers."""
    global WS_SUFFIX
    prev, WS_SUFFIX = WS_SUFFIX, WS_SUFFIX + suffix
    try:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            yield
    finally:
        WS_SUFFIX = prev


def _ws(nbytes: int, device, tag: str = "") -> torch.Tensor:
    """Grow-only scratch buffer per (device, tag).  A buffer that has to grow is REPLACED, and the old
    one is kept alive for the life of the process (never returned to the caching allocator): an epoch
    captured into a hipGraph (HANTrainer(use_graph=True)) replays with the raw pointers it saw, and a
    later, larger request for the same tag must not free memory such a graph still reads and writes.
    Growth is geometric, so the retired buffers of a tag add up to less than its current one."""
    key = (str(device), tag + WS_SUFFIX)
    t = _workspaces.get(key)
    if t is None or t.numel() < nbytes:
        if t is not None:
            _retired_workspaces.append(t)
        t = torch.empty(max(int(nbytes), 1 << 20, 2 * (t.numel() if t is not None else 0)), dtype=torch.uint8,
                        device=device)
        _workspaces[key] = t
    return t


def require_gpu(t: torch.Tensor, name: str) -> torch.Tensor:
    """Guard of the (few) torch-level paths around the kernels: no CPU path there either."""
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a GPU tensor (han_amd has no CPU path); got {t.device}")
    return t


def _chk(t: torch.Tensor, name: str, shape=None, dtype=torch.float32, device=None, contiguous=True):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a GPU tensor (han_amd has no CPU path); got {t.device}")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None:
        if t.dim() != len(shape) or any(s is not None and int(a) != int(s)
                                        for a, s in zip(t.shape, shape)):
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1}      # HAN_DTYPE_F32 / HAN_DTYPE_BF16


def _dtype_code(t: torch.Tensor, name: str) -> int:
    if t.dtype not in DTYPE_CODE:
        raise ValueError(f"{name}: dtype {t.dtype}, expected float32 or bfloat16")
    return DTYPE_CODE[t.dtype]


# rows longer than SPLIT_DEG are cut into chunks of SPLIT_CHUNK edges, a wave per chunk (round 4: 1024 / 512, from 8192 /
# 4096 -- a wave walking an 8192-entry row alone was the tail of the whole launch on power-law graphs; the finishing
# launch now merges a row's chunks with a block instead of one lane group: profiles/r04_k2_skew_split_sweep.jsonl)
SPLIT_DEG = 1024
SPLIT_CHUNK = 512


SHORT_DEG = 16         # HAN_SHORT_DEG: rows below this many entries run four to a wave in a degree-binned launch
BINNED = True          # tests / measurements: False = one row shape per launch, chosen from E / N (rounds 1-3)


def _row_split_arg(graph: CSRGraph, tag: str, bins: bool = True, split: bool = True):
    """ctypes han_row_split_t for `graph`: its degree bins (short / mid row lists) and the chunks of its rows beyond
    SPLIT_DEG (None when the graph has neither: every row in one bin and no long row still passes the bin counts,
    so that the library uses that bin's row shape).  Returns (byref-able struct or None, keepalive tuple)."""
    sp = graph.row_split(SPLIT_DEG, SPLIT_CHUNK) if split else None      # (the lean kernels walk whole rows)
    rb = graph.row_bins(SHORT_DEG, SPLIT_DEG) if (bins and BINNED and graph.n_rows > 0) else None
    if sp is None and rb is None:
        return None, None
    lib = _lib.load()
    if sp is not None:
        ws = _ws(lib.han_row_split_workspace(sp["n_chunks"]), graph.device, "split" + tag)
        st = _lib.HanRowSplit(sp["split_deg"], sp["n_long"], sp["n_chunks"], sp["long_rows"].data_ptr(),
                              sp["long_ptr"].data_ptr(), sp["chunk_long"].data_ptr(),
                              sp["chunk_start"].data_ptr(), sp["chunk_end"].data_ptr(), ws.data_ptr(),
                              ws.numel(), 0, 0, None, None)
    else:
        ws = None
        st = _lib.HanRowSplit(SPLIT_DEG, 0, 0, None, None, None, None, None, None, 0, 0, 0, None, None)
    if rb is not None:
        st.n_short, st.n_mid = rb["n_short"], rb["n_mid"]
        st.short_rows, st.mid_rows = _ptr(rb["short_rows"]), _ptr(rb["mid_rows"])
    return st, (sp, rb, ws)


class RowSubset:
    """The rows of `graph` a forward is to compute (node_attn_fwd(rows=...), HAN_FLAG_K2_ROW_SUBSET): `mask` (n_rows,)
    bool / uint8, non-zero = listed.  `live`: the ascending int32 ids; n_rows / nnz: the listed rows and their entries
    (what a launch over them is priced by).  The bins and the split restricted to the rows (CSRGraph.row_subset) are
    computed once per (SHORT_DEG, SPLIT_DEG, SPLIT_CHUNK) and kept."""

    def __init__(self, graph: CSRGraph, mask: torch.Tensor, live: torch.Tensor | None = None):
        self.graph = graph
        self.mask = (mask != 0).to(graph.device)
        self.live = live if live is not None else torch.nonzero(self.mask).flatten().to(torch.int32).contiguous()
        self._parts = {}

    def parts(self):
        key = (SHORT_DEG, SPLIT_DEG, SPLIT_CHUNK)
        if key not in self._parts:
            self._parts[key] = self.graph.row_subset(self.mask, *key)
        return self._parts[key]

    @property
    def n_rows(self) -> int:
        return self.parts()["n_rows"]

    @property
    def nnz(self) -> int:
        return self.parts()["nnz"]

    def arg(self, tag: str):
        """ctypes han_row_split_t of the listed rows (+ keepalive)."""
        pt = self.parts()
        sp, rb = pt["split"], pt["bins"]
        ws = None
        if sp is not None:
            ws = _ws(_lib.load().han_row_split_workspace(sp["n_chunks"]), self.graph.device, "split" + tag)
            st = _lib.HanRowSplit(sp["split_deg"], sp["n_long"], sp["n_chunks"], sp["long_rows"].data_ptr(),
                                  sp["long_ptr"].data_ptr(), sp["chunk_long"].data_ptr(),
                                  sp["chunk_start"].data_ptr(), sp["chunk_end"].data_ptr(), ws.data_ptr(),
                                  ws.numel(), 0, 0, None, None)
        else:
            st = _lib.HanRowSplit(SPLIT_DEG, 0, 0, None, None, None, None, None, None, 0, 0, 0, None, None)
        st.n_short, st.n_mid = rb["n_short"], rb["n_mid"]
        st.short_rows, st.mid_rows = _ptr_nonempty(rb["short_rows"]), _ptr_nonempty(rb["mid_rows"])
        return st, (pt, ws)


LEAN = True                # tests / measurements: False keeps the classic gather kernels


def _use_lean(graph: CSRGraph, table) -> bool:
    """The lean K2 forward (HAN_FLAG_LEAN): tables that live in the L2s (<= 16384 rows: 4 MB) with long rows (mean
    degree >= 64), where the classic gather kernels are bound by vector-instruction issue, not by memory."""
    return (LEAN and table.dtype == torch.float32 and 0 < graph.n_cols <= 16384
            and graph.nnz >= 64 * graph.n_rows)


DENSE = True               # tests / measurements: False keeps small dense graphs on the lean CSR kernels
DENSE_MIN_DENSITY = 0.65   # stored entries / (rows x table rows) from which the matrix-pipe form wins over a whole training step (eval + training forward + backward: 0.47 ms at any density against 0.59 ms for the lean CSR kernels at 78 %, ~0.40 ms at 50 %; profiles/r04_k2_dense_vs_lean.jsonl)


def _use_dense(graph: CSRGraph, table, K: int, FP: int) -> bool:
    """The dense (bit mask + fp32 MFMA) K2 path: a lean-eligible graph (_use_lean) of the reference shape whose rows
    are dense enough that computing every (i, j) pair beats walking the stored entries, binary, without repeated
    entries."""
    if not (DENSE and K == 8 and FP == 8 and graph.values is None and not graph.masked and _use_lean(graph, table)):
        return False
    if graph.nnz < DENSE_MIN_DENSITY * graph.n_rows * graph.n_cols:
        return False
    return graph.bitmask() is not None


def _dense_arg(graph: CSRGraph, train: bool, tag: str):
    """ctypes han_dense_t of `graph` (+ keepalive)."""
    lib = _lib.load()
    bits = graph.bitmask()
    ws = _ws(lib.han_node_attn_dense_workspace(graph.n_rows, graph.n_cols, int(train)), graph.device, "dense" + tag)
    return _lib.HanDense(bits.data_ptr(), bits.shape[1], graph.n_cols, ws.data_ptr(), ws.numel()), (bits, ws)


def _ld(t: torch.Tensor, width: int) -> int:
    """Leading dimension of the (N, width) view t, in elements.  The stride of a dimension of size <= 1 means nothing
    (torch leaves it arbitrary, and no second row is addressed): such a view passes at least `width`, which is all
    the library asks of a leading dimension."""
    return t.stride(0) if t.shape[0] > 1 else max(width, t.stride(0))


def _check_heads(K: int, FP: int):
    if K * FP != D or FP not in (4, 8, 16, 32, 64):
        raise NotImplementedError(
            f"this build supports n_heads*hid_units == 64 with hid_units in "
            f"{{4,8,16,32,64}}; got n_heads={K}, hid_units={FP}")


def _check_drop(p: float, name: str):
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise ValueError(f"{name} must be in [0, 1), got {p}")
    return p


# --------------------------------------------------------------------------- K1
def project_fwd(X, W, a1, a2, b1, b2, in_drop=0.0, fts_drop=0.0, seed=0, row_offset=0,
                table_dtype=torch.float32, seed_dev=None, flags=0, want_keep=False):
    """utils/layers.py:18-24,31-32 for the K heads of one meta-path.
    X (N,F) fp32 or bf16 [row stride >= F]; W (F,D); a1,a2 (K,F'); b1,b2 (K,).
    H is stored in `table_dtype` (float32 or bfloat16; f1/f2 come from the stored rows).
    Returns H (N,D), f1 (N,K), f2 (N,K).  With fts_drop > 0 the keep bit of the
    projected-row dropout rides in mantissa bit 0 of every H element.
    want_keep=True returns a 4th value: the keep table of the per-head input dropout for
    project_bwd (uint8, han_project_keep_bytes() long), or None when this shape has none
    (small inputs, in_drop == 0, head shapes other than 8 x 8): dW then regenerates the draws.
    X may be a SparseFeatures: the projection then visits the stored entries only (han_project_sparse_fwd), with the
    same draws; there is no keep table."""
    lib = _lib.load()
    if isinstance(X, SparseFeatures):
        out = _project_sparse_fwd(X, W, a1, a2, b1, b2, (), in_drop, fts_drop, [seed], row_offset, table_dtype,
                                  seed_dev, flags)
        return out + (None,) if want_keep else out
    if X.dim() != 2:
        raise ValueError(f"X: expected (N,F), got {tuple(X.shape)}")
    xcode, ldx, N, F, K, FP, in_drop, fts_drop, H, f1, f2, ws, keep = _project_fwd_setup(
        X, W, a1, a2, b1, b2, (), in_drop, fts_drop, table_dtype, flags, want_keep, lib.han_project_fwd_workspace)
    _lib.check(lib.han_project_fwd(
        X.data_ptr(), xcode, ldx, W.data_ptr(), a1.data_ptr(),
        a2.data_ptr(), b1.data_ptr(), b2.data_ptr(), H.data_ptr(), DTYPE_CODE[table_dtype],
        f1.data_ptr(), f2.data_ptr(), _ptr(ws), ws.numel() if ws is not None else 0, N, F, K, FP,
        in_drop, fts_drop, int(seed), _dev_word(seed_dev), int(row_offset),
        _ptr(keep), int(flags), _stream()), "han_project_fwd")
    if want_keep:
        return H, f1, f2, keep
    return H, f1, f2


def _project_fwd_outputs(N, F, dev, W, a1, a2, b1, b2, lead, in_drop, fts_drop, table_dtype):
    """What every K1 forward shares once its input has given (N, F) and the device: the parameter checks, in their
    order, and the outputs H lead + (N,D), f1 / f2 lead + (N,K)."""
    K, FP = a1.shape[len(lead):]
    if table_dtype not in DTYPE_CODE:
        raise ValueError(f"table_dtype {table_dtype}: expected float32 or bfloat16")
    _check_heads(K, FP)
    _chk(W, "W", lead + (F, D), device=dev)
    _chk(a1, "a1", lead + (K, FP), device=dev)
    _chk(a2, "a2", lead + (K, FP), device=dev)
    _chk(b1, "b1", lead + (K,), device=dev)
    _chk(b2, "b2", lead + (K,), device=dev)
    in_drop = _check_drop(in_drop, "in_drop")
    fts_drop = _check_drop(fts_drop, "fts_drop")
    H = torch.empty(lead + (N, D), dtype=table_dtype, device=dev)
    f1 = torch.empty(lead + (N, K), dtype=torch.float32, device=dev)
    f2 = torch.empty(lead + (N, K), dtype=torch.float32, device=dev)
    return K, FP, in_drop, fts_drop, H, f1, f2


def _project_fwd_setup(X, W, a1, a2, b1, b2, lead, in_drop, fts_drop, table_dtype, flags, want_keep, ws_bytes):
    """The dense project_fwd (lead = ()) and project_fwd_multi (lead = (P,)): the checks of X, _project_fwd_outputs,
    the workspace of ws_bytes(N, F, K, FP, *lead) bytes (> 0 only for short inputs: split-F) and the keep table
    lead + (han_project_keep_bytes(),), or None when this call has none."""
    _chk(X, "X", contiguous=False, dtype=X.dtype)
    xcode = _dtype_code(X, "X")
    if X.stride(1) != 1:
        raise ValueError("X: rows must be contiguous")
    N, F = X.shape
    dev = X.device
    K, FP, in_drop, fts_drop, H, f1, f2 = _project_fwd_outputs(N, F, dev, W, a1, a2, b1, b2, lead, in_drop, fts_drop,
                                                               table_dtype)
    nbytes = ws_bytes(N, F, K, FP, *lead)
    ws = _ws(nbytes, dev, "projf") if nbytes else None
    ldx = _ld(X, F)
    keep = None
    if want_keep and in_drop > 0 and not (flags & FLAG_K1_EXACT_PIPE) and X.data_ptr() % 16 == 0:
        kb = _lib.load().han_project_keep_bytes(N, F, ldx, K, FP)
        if kb:
            keep = torch.empty(lead + (kb,), dtype=torch.uint8, device=dev)
    return xcode, ldx, N, F, K, FP, in_drop, fts_drop, H, f1, f2, ws, keep


def _project_sparse_fwd(X, W, a1, a2, b1, b2, lead, in_drop, fts_drop, seeds, row_offset, table_dtype, seed_dev, flags):
    """project_fwd (lead = ()) / project_fwd_multi (lead = (P,): a loop over the meta-paths with their seeds -- fusing
    them would save only the index stream) of a SparseFeatures: H lead + (N,D), f1 / f2 lead + (N,K)."""
    lib = _lib.load()
    if not X.is_cuda:
        raise ValueError(f"X: must be on a GPU (han_amd has no CPU path); got {X.device}")
    N, F = X.shape
    K, FP, in_drop, fts_drop, H, f1, f2 = _project_fwd_outputs(N, F, X.device, W, a1, a2, b1, b2, lead, in_drop,
                                                               fts_drop, table_dtype)
    sel = (lambda t, p: t[p]) if lead else (lambda t, p: t)
    for p in range(lead[0] if lead else 1):
        _lib.check(lib.han_project_sparse_fwd(
            X.rowptr.data_ptr(), X.colidx.data_ptr(), _ptr(X.values), sel(W, p).data_ptr(), sel(a1, p).data_ptr(),
            sel(a2, p).data_ptr(), sel(b1, p).data_ptr(), sel(b2, p).data_ptr(), sel(H, p).data_ptr(),
            DTYPE_CODE[table_dtype], sel(f1, p).data_ptr(), sel(f2, p).data_ptr(), N, F, K, FP, in_drop, fts_drop,
            int(seeds[p]) & ((1 << 64) - 1), _dev_word(seed_dev), int(row_offset), int(flags), _stream()),
            "han_project_sparse_fwd")
    return H, f1, f2


# columns of a SparseFeatures longer than this many entries are cut into chunks of it for dW, a wave per chunk
# (SparseFeatures.transposed builds the table; han_project_sparse_bwd merges the chunks' partial rows in order): the
# split rule of SPLIT_CHUNK -- a wave walking a column as long as N alone would be the tail of the launch.  A chunk is
# 4 batches of 64 entries, about 20 dependent memory round trips: short enough that the longest wave does not set the
# time of the 3025-row data sets' dW, long enough that a column of 262 144 rows merges 1024 partial rows, not 4096
# (tools/k1_sparse_bench.py --chunks sweeps it: profiles/r12_k1_sparse_bench.jsonl, dw_sparse_by_chunk)
SPARSE_COL_CHUNK = 256


def _project_sparse_bwd(X, dH, K, FP, in_drop, seed, row_offset, seed_dev, out):
    """project_bwd of a SparseFeatures: a gather of dH rows per feature through X.transposed()."""
    lib = _lib.load()
    N, F = X.shape
    _chk(dH, "dH", (N, D), device=X.device)
    _check_heads(K, FP)
    dW = _out(out, "out", (F, D), X.device)
    t = X.transposed()
    nbytes = lib.han_project_sparse_bwd_workspace(t["n_chunks"])
    ws = _ws(nbytes, X.device, "projs") if nbytes else None
    _lib.check(lib.han_project_sparse_bwd(
        t["colptr"].data_ptr(), t["rowidx"].data_ptr(), _ptr(t["values_t"]), t["col_chunk"], t["n_long"], t["n_chunks"],
        _ptr(t["long_cols"]), _ptr(t["long_ptr"]), _ptr(t["chunk_col"]), _ptr(t["chunk_start"]), _ptr(t["chunk_end"]),
        dH.data_ptr(), dW.data_ptr(), _ptr(ws), ws.numel() if ws is not None else 0, N, F, K, FP,
        _check_drop(in_drop, "in_drop"), int(seed) & ((1 << 64) - 1), _dev_word(seed_dev), int(row_offset), _stream()),
        "han_project_sparse_bwd")
    return dW


def keep_bytes(N, F, ldx, K=8, FP=8) -> int:
    """han_project_keep_bytes: size of the keep table of an (N, F) input, 0 when the shape has none."""
    return int(_lib.load().han_project_keep_bytes(int(N), int(F), int(ldx), int(K), int(FP)))


def project_fwd_multi(X, W, a1, a2, b1, b2, in_drop=0.0, fts_drop=0.0, seeds=None, row_offset=0,
                      table_dtype=torch.float32, seed_dev=None, flags=0, want_keep=False):
    """project_fwd for all P meta-paths of ONE shared feature matrix (the reference feeds the same matrix to
    every meta-path: ex_acm3025.py:86, models/gat.py:39).  W (P,F,D), a1/a2 (P,K,F'), b1/b2 (P,K) -- the
    model's own parameter tensors.  Returns H (P,N,D), f1, f2 (P,N,K) and, with want_keep, a list of P keep
    tables (or Nones).  The eval forward of long inputs runs as ONE fused launch (X read, split and staged
    once for 4 meta-paths per block); every other case is the per-meta-path kernel, P times.
    X may be a SparseFeatures (a loop over the meta-paths; no keep tables)."""
    lib = _lib.load()
    if isinstance(X, SparseFeatures):
        P = a1.shape[0]
        if (float(in_drop) > 0 or float(fts_drop) > 0) and (seeds is None or len(seeds) != P):
            raise ValueError("dropout needs one seed per meta-path")
        out = _project_sparse_fwd(X, W, a1, a2, b1, b2, (P,), in_drop, fts_drop, seeds if seeds is not None else [0] * P,
                                  row_offset, table_dtype, seed_dev, flags)
        return out + ([None] * P,) if want_keep else out
    if X.dim() != 2 or W.dim() != 3:
        raise ValueError(f"X: expected (N,F) and W (P,F,D), got {tuple(X.shape)}, {tuple(W.shape)}")
    P = a1.shape[0]
    xcode, ldx, N, F, K, FP, in_drop, fts_drop, H, f1, f2, ws, keep = _project_fwd_setup(
        X, W, a1, a2, b1, b2, (P,), in_drop, fts_drop, table_dtype, flags, want_keep,
        lib.han_project_fwd_multi_workspace)
    if (in_drop > 0 or fts_drop > 0) and (seeds is None or len(seeds) != P):
        raise ValueError("dropout needs one seed per meta-path")
    seed_arr = (ctypes.c_uint64 * P)(*[int(x) & ((1 << 64) - 1) for x in (seeds if seeds is not None else [0] * P)])
    _lib.check(lib.han_project_fwd_multi(
        X.data_ptr(), xcode, ldx, W.data_ptr(), a1.data_ptr(), a2.data_ptr(), b1.data_ptr(), b2.data_ptr(),
        H.data_ptr(), DTYPE_CODE[table_dtype], f1.data_ptr(), f2.data_ptr(),
        _ptr(ws), ws.numel() if ws is not None else 0, N, F, K, FP, P,
        in_drop, fts_drop, seed_arr, _dev_word(seed_dev), int(row_offset),
        _ptr(keep), int(flags), _stream()), "han_project_fwd_multi")
    if want_keep:
        return H, f1, f2, [keep[p] if keep is not None else None for p in range(P)]
    return H, f1, f2


def project_fwd_both(X, W, a1, a2, b1, b2, in_drop, fts_drop, seeds, row_offset=0, table_dtype=torch.float32,
                     seed_dev=None, flags=0):
    """han_project_fwd_both: the TRAINING forward (in_drop / fts_drop / seeds, keep tables) and the EVAL forward (no
    dropout) of all P meta-paths of one dense feature matrix in one pass over X per meta-path.  Returns
    ((H, f1, f2, [keep tables]), (H_eval, f1_eval, f2_eval)) -- byte for byte what project_fwd_multi(..., in_drop,
    fts_drop, seeds, want_keep=True) and project_fwd_multi(...) without dropout return -- or None, with nothing
    launched, where the library's one combined kernel does not apply (han_hip.h lists the conditions: fp32 X and
    tables, input dropout with a keep table, P even, ...): the caller then makes those two calls.  X must be finite."""
    lib = _lib.load()
    if isinstance(X, SparseFeatures) or X.dim() != 2 or W.dim() != 3:
        return None
    P = a1.shape[0]
    xcode, ldx, N, F, K, FP, in_drop, fts_drop, H, f1, f2, ws, keep = _project_fwd_setup(
        X, W, a1, a2, b1, b2, (P,), in_drop, fts_drop, table_dtype, flags, True, lib.han_project_fwd_both_workspace)
    if seeds is None or len(seeds) != P:
        raise ValueError("one seed per meta-path")
    He, f1e, f2e = torch.empty_like(H), torch.empty_like(f1), torch.empty_like(f2)
    seed_arr = (ctypes.c_uint64 * P)(*[int(x) & ((1 << 64) - 1) for x in seeds])
    code = lib.han_project_fwd_both(
        X.data_ptr(), xcode, ldx, W.data_ptr(), a1.data_ptr(), a2.data_ptr(), b1.data_ptr(), b2.data_ptr(),
        H.data_ptr(), DTYPE_CODE[table_dtype], f1.data_ptr(), f2.data_ptr(), He.data_ptr(), f1e.data_ptr(), f2e.data_ptr(),
        _ptr(ws), ws.numel() if ws is not None else 0, N, F, K, FP, P, in_drop, fts_drop, seed_arr, _dev_word(seed_dev),
        int(row_offset), _ptr(keep), int(flags), _stream())
    if code == _lib.E_NOT_ELIGIBLE:
        return None
    _lib.check(code, "han_project_fwd_both")
    return (H, f1, f2, [keep[p] for p in range(P)]), (He, f1e, f2e)


def project_bwd(X, dH, K, FP, in_drop=0.0, seed=0, row_offset=0, seed_dev=None, out=None, keep=None):
    """dW (F,D) = dropout_k(X)^T dH (written to `out` when given).  keep: the table project_fwd(want_keep=True)
    returned for the same X / seed (the draws are then read, not regenerated), or None.
    X may be a SparseFeatures (han_project_sparse_bwd through X.transposed(); the draws are regenerated)."""
    lib = _lib.load()
    if isinstance(X, SparseFeatures):
        if keep is not None:
            raise ValueError("keep: sparse features have no keep table")
        return _project_sparse_bwd(X, dH, K, FP, in_drop, seed, row_offset, seed_dev, out)
    _chk(X, "X", contiguous=False, dtype=X.dtype)
    xcode = _dtype_code(X, "X")
    N, F = X.shape
    _chk(dH, "dH", (N, D), device=X.device)
    _check_heads(K, FP)
    dW = _out(out, "out", (F, D), X.device)
    nbytes = lib.han_project_bwd_workspace(N, F, K, FP)
    ws = _ws(nbytes, X.device, "proj")
    ldx = _ld(X, F)
    if keep is not None:
        _chk(keep, "keep", (lib.han_project_keep_bytes(N, F, ldx, K, FP),), dtype=torch.uint8, device=X.device)
    _lib.check(lib.han_project_bwd(
        X.data_ptr(), xcode, ldx, dH.data_ptr(), dW.data_ptr(),
        ws.data_ptr(), ws.numel(), N, F, K, FP, _check_drop(in_drop, "in_drop"), int(seed), _dev_word(seed_dev),
        int(row_offset), _ptr(keep), _stream()), "han_project_bwd")
    return dW


def project_bwd_input(dH, W, K, FP, out=None, in_drop=0.0, seed=0, row_offset=0, seed_dev=None):
    """dX (N,F) = sum_k mask_k/keep * (dH_k @ W_k^T): gradient w.r.t. the layer input
    (only layers >= 1 of a multi-layer stack need it).  `out`: optional (N,F) view
    with unit inner stride (e.g. dM_prev[:, p, :])."""
    lib = _lib.load()
    _check_heads(K, FP)
    N = dH.shape[0]
    F = W.shape[0]
    dev = dH.device
    _chk(dH, "dH", (N, D))
    _chk(W, "W", (F, D), device=dev)
    if out is None:
        out = torch.empty((N, F), dtype=torch.float32, device=dev)
    else:
        _chk(out, "out", (N, F), device=dev, contiguous=False)
        if out.stride(1) != 1:
            raise ValueError("out: rows must be contiguous")
    _lib.check(lib.han_project_bwd_input(
        dH.data_ptr(), W.data_ptr(), out.data_ptr(), _ld(out, F),
        N, F, K, FP, _check_drop(in_drop, "in_drop"), int(seed), _dev_word(seed_dev), int(row_offset), _stream()),
        "han_project_bwd_input")
    return out


# --------------------------------------------------------------------------- K2
def node_attn_fwd(graph: CSRGraph, H_tab, f1, a2, b2, c, out=None, train=False, coef_drop=0.0,
                  fts_drop=0.0, seed=0, row_offset=0, activation=ACT_ELU, table_gid=None, res=None,
                  seed_dev=None, f2_src=None, f2=None, rows=None):
    """utils/layers.py:26-35,46.  H_tab (NT,D): gather table of UNDROPPED projected
    rows indexed by graph.colidx (f2_j is recomputed from the gathered row with
    a2 (K,F'), b2 (K,)); with fts_drop > 0 bit 0 of each element is its keep bit
    (as project_fwd stamped it); f1 (N,K) local rows; c (D,).  table_gid (NT,)
    int32: global id of each table row when H_tab is a [local | halo] table.
    res (N,D) fp32: residual term added before the activation (layers.py:38-40).  `out`: optional (N,D) view with unit inner
    stride (e.g. M[:,p,:]).  f2_src (NT,1): one head of 64 columns only -- the neighbour scores are gathered from
    this table instead of being recomputed (slices of a head wider than 64 columns: f1 / f2_src hold the head's
    totals).  f2 (NT,K): the table rows' scores as project_fwd returned them -- with them a small graph with long rows
    (_use_lean) runs on the lean kernels, which read the scores instead of recomputing them.
    rows: None, or the rows to compute -- a RowSubset of `graph`, or a plan whose subset(graph) gives one
    (layers.LiveForwardPlan).  Only the listed rows of out (and lse, aggp, tsum) are written, with the bits the full
    call gives them; every other row keeps what the (full-size) tensors held.  Such a call never takes the lean or
    dense form and records the listed rows and their entries in K2_TIMING.
    Returns out, saved where saved = (out, lse, aggp, tsum) if train else None: saved[0] is the OUTPUT view itself,
    which node_attn_bwd_rows reads (it must stay unmodified until then); the pre-activation is not stored."""
    lib = _lib.load()
    if rows is not None and not isinstance(rows, RowSubset):
        rows = rows.subset(graph)
    if rows is not None and rows.graph is not graph:
        raise ValueError("rows: the row subset was built for another graph")
    K, FP = a2.shape
    _check_heads(K, FP)
    N = graph.n_rows
    dev = H_tab.device
    _chk(H_tab, "H", (graph.n_cols, D), dtype=H_tab.dtype)
    tcode = _dtype_code(H_tab, "H")
    _chk(f1, "f1", (N, K), device=dev)
    _chk(a2, "a2", (K, FP), device=dev)
    _chk(b2, "b2", (K,), device=dev)
    _chk(c, "c", (D,), device=dev)
    if table_gid is not None:
        _chk(table_gid, "table_gid", (graph.n_cols,), dtype=torch.int32, device=dev)
    if res is not None:
        _chk(res, "res", (N, D), device=dev)
    if f2_src is not None:
        if FP != D:
            raise ValueError("f2_src: only for one head of 64 columns (K = 1, F' = 64)")
        _chk(f2_src, "f2_src", (graph.n_cols, 1), device=dev)
        f2 = f2_src
    lean = rows is None and f2 is not None and table_gid is None and _use_lean(graph, H_tab)
    if lean:
        _chk(f2, "f2", (graph.n_cols, K), device=dev)
    if graph.device != dev:
        raise ValueError("graph and tables must be on the same device")
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=dev)
    else:
        _chk(out, "out", (N, D), device=dev, contiguous=False)
        if out.stride(1) != 1 or (N > 1 and out.stride(0) < D):
            raise ValueError("out: rows must be contiguous with row stride >= 64")
    coef_drop = _check_drop(coef_drop, "coef_drop")
    fts_drop = _check_drop(fts_drop, "fts_drop")
    if (coef_drop > 0 or fts_drop > 0) and not train:
        raise ValueError("dropout > 0 requires train=True")
    saved = None
    ptrs = [None, None, None, None]
    if train:
        # the pre-activation is not stored (round 3): the backward inverts the activation on `out`, which the
        # caller keeps anyway (it is a slice of M, the input of K3) -- 256 B per row less to write, keep and read
        aggp = torch.empty((N, D), dtype=torch.float32, device=dev)
        lse = torch.empty((N, K), dtype=torch.float32, device=dev)
        tsum = torch.empty((N, K), dtype=torch.float32, device=dev)
        saved = (out, lse, aggp, tsum)
        ptrs = [None, lse.data_ptr(), aggp.data_ptr(), tsum.data_ptr()]
    split, _keep = _row_split_arg(graph, "f", bins=not lean, split=not lean) if rows is None else rows.arg("f")
    dense, _keep_d = _dense_arg(graph, train, "f") if (lean and f2_src is None and _use_dense(graph, H_tab, K, FP)) else (None, None)
    with _k2_timed("train" if train else "eval", *((N, graph.nnz) if rows is None else (rows.n_rows, rows.nnz))):
        _lib.check(lib.han_node_attn_fwd(
            graph.rowptr.data_ptr(), graph.colidx.data_ptr(),
            _ptr(graph.values), H_tab.data_ptr(), tcode, _ptr(table_gid), f1.data_ptr(),
            f2.data_ptr() if (lean or f2_src is not None) else None,
            a2.data_ptr(), b2.data_ptr(), c.data_ptr(), _ptr(res),
            out.data_ptr(), _ld(out, D),
            ptrs[0], ptrs[1], ptrs[2], ptrs[3], N, graph.nnz, K, FP, LEAKY_SLOPE, coef_drop, fts_drop,
            int(seed), _dev_word(seed_dev), int(row_offset), int(activation),
            (FLAG_XCD_ORDER if graph.has_locality() else 0) | (FLAG_LEAN if lean else 0) | (FLAG_K2_DEEP if K2_DEEP else 0)
            | (FLAG_K2_SHARED_HASH if K2_SHARED_HASH else 0) | (FLAG_K2_ROW_SUBSET if rows is not None else 0),
            ctypes.byref(split) if split is not None else None,
            ctypes.byref(dense) if dense is not None else None, _stream()), "han_node_attn_fwd")
    return out, saved


def node_attn_coefs(graph: CSRGraph, f1, f2, coef_drop=0.0, seed=0, row_offset=0, mean_heads=False,
                    table_gid=None, seed_dev=None):
    """The attention coefficients as data (attn_head(..., return_coef=True),
    utils/layers.py:27-30,43-44): (E,K) values in the CSR order of `graph`, or their
    head mean (E,) (models/gat.py:171-172).  f1 (N,K), f2 (NT,K) from project_fwd."""
    lib = _lib.load()
    _chk(f1, "f1", None)
    K = f1.shape[1]
    FP = D // K
    _check_heads(K, FP)
    dev = f1.device
    _chk(f1, "f1", (graph.n_rows, K))
    _chk(f2, "f2", (graph.n_cols, K), device=dev)
    if graph.device != dev:
        raise ValueError("graph and f1 live on different devices")
    if table_gid is not None:
        _chk(table_gid, "table_gid", (graph.n_cols,), dtype=torch.int32, device=dev)
    coef = torch.empty((graph.nnz,) if mean_heads else (graph.nnz, K), dtype=torch.float32, device=dev)
    _lib.check(lib.han_node_attn_coefs(
        graph.rowptr.data_ptr(), graph.colidx.data_ptr(),
        _ptr(graph.values), _ptr(table_gid), f1.data_ptr(), f2.data_ptr(),
        coef.data_ptr(), int(bool(mean_heads)), graph.n_rows, graph.nnz, K, FP, LEAKY_SLOPE,
        _check_drop(coef_drop, "coef_drop"), int(seed), _dev_word(seed_dev), int(row_offset), _stream()), "han_node_attn_coefs")
    return coef


def gs_row_bytes(K=8, FP=8, table_dtype=torch.float32) -> int:
    """Bytes of one fused backward row [g | (f1, lse, s, z) x K] (han_gs_row_bytes)."""
    n = int(_lib.load().han_gs_row_bytes(K, FP, DTYPE_CODE[table_dtype]))
    if n == 0:
        raise NotImplementedError(f"no fused backward row for K={K}, FP={FP}, {table_dtype}")
    return n


def gs_views(gs, K=8, FP=8, table_dtype=torch.float32):
    """(g (N,D) table_dtype, stats (N,K,4) fp32) views of a fused backward table (N, row_bytes) uint8."""
    gb = D * (2 if table_dtype == torch.bfloat16 else 4)
    g = gs[:, :gb].view(table_dtype)
    stats = gs[:, gb:gb + 16 * K].view(torch.float32).unflatten(1, (K, 4))
    return g, stats


def node_attn_bwd_rows(dOut, out, aggp, tsum, f1, lse, c, activation=ACT_ELU, K=8, FP=8,
                       table_dtype=torch.float32, res=None, dc_out=None, gs_out=None):
    """Row-local half of the K2 backward.  dOut (N,D) view (unit inner stride); out (N,D) view: the forward's
    output rows (saved[0] of node_attn_fwd), from which the pre-activation is recovered.
    Returns gs (N, row_bytes) uint8 -- the fused table [g | (f1, lse, s, z) x K] the transposed-graph
    pass gathers from (gs_views() splits it) --, df1 (N,K), dc (D,) [written to dc_out when given].
    gs_out: optional preallocated destination (e.g. the local block of an exchange table)."""
    lib = _lib.load()
    _check_heads(K, FP)
    N = out.shape[0]
    dev = out.device
    _chk(dOut, "dOut", (N, D), device=dev, contiguous=False)
    _chk(out, "out", (N, D), device=dev, contiguous=False)
    if dOut.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("dOut / out: rows must be contiguous")
    for t, n, s in ((aggp, "aggp", (N, D)), (tsum, "tsum", (N, K)),
                    (f1, "f1", (N, K)), (lse, "lse", (N, K)), (c, "c", (D,))):
        _chk(t, n, s, device=dev)
    rb = gs_row_bytes(K, FP, table_dtype)
    if gs_out is None:      # rows padded to whole lines: keep the padding bytes defined
        padded = rb != D * (2 if table_dtype == torch.bfloat16 else 4) + 16 * K
        gs = (torch.zeros if padded else torch.empty)((N, rb), dtype=torch.uint8, device=dev)
    else:
        gs = _chk(gs_out, "gs_out", (N, rb), dtype=torch.uint8, device=dev)
    df1 = torch.empty((N, K), dtype=torch.float32, device=dev)
    dc = _out(dc_out, "dc_out", (D,), dev)
    ws = _ws(lib.han_node_attn_bwd_workspace(N, K, FP), dev, "rows")
    _lib.check(lib.han_node_attn_bwd_rows(
        dOut.data_ptr(), _ld(dOut, D), out.data_ptr(), _ld(out, D), aggp.data_ptr(),
        tsum.data_ptr(), f1.data_ptr(), lse.data_ptr(), c.data_ptr(),
        _ptr(res), gs.data_ptr(),
        DTYPE_CODE[table_dtype], df1.data_ptr(), dc.data_ptr(), ws.data_ptr(), ws.numel(), N, K, FP,
        int(activation), _stream()), "han_node_attn_bwd_rows")
    return gs, df1, dc


def node_attn_bwd_cols(graph_t: CSRGraph, gs_tab, H, f2, df1, a1, a2, coef_drop=0.0,
                       fts_drop=0.0, seed=0, src_offset=0, dst_offset=0, table_gid=None, seed_dev=None, zero_rows=False,
                       scores_out=None):
    """Transposed-graph half of the K2 backward.  graph_t rows = local sources j,
    its colidx = destinations i indexing the fused table gs_tab (NT, row_bytes) uint8.
    H (NS,D) undropped local rows (keep bits in bit 0 when fts_drop > 0),
    f2/df1 (NS,K).  zero_rows: a hint that most rows of gs_tab hold a zero gradient (HAN_FLAG_K2_ZERO_ROWS: the
    g piece of a head whose record says so is not requested; same bits).  Returns dH (NS,D), df2 (NS,K).
    scores_out = (da1, da2, db1, db2): the call goes through node_attn_bwd_cols_scores where the library has that form,
    and returns (dH, df2, done) -- done False: the four tensors are untouched, score_param_bwd is still to be called."""
    if scores_out is not None:
        got = node_attn_bwd_cols_scores(graph_t, gs_tab, H, f2, df1, a1, a2, coef_drop, fts_drop, seed, src_offset,
                                        dst_offset, table_gid, seed_dev, zero_rows, out=scores_out)
        if got is not None:
            return got + (True,)
    lib = _lib.load()
    K, FP = a1.shape
    _check_heads(K, FP)
    NS = graph_t.n_rows
    dev = H.device
    _chk(H, "H", (NS, D), dtype=H.dtype)
    tcode = _dtype_code(H, "H")
    _chk(gs_tab, "gs", (graph_t.n_cols, gs_row_bytes(K, FP, H.dtype)), device=dev, dtype=torch.uint8)
    if table_gid is not None:
        _chk(table_gid, "table_gid", (graph_t.n_cols,), dtype=torch.int32, device=dev)
    _chk(f2, "f2", (NS, K), device=dev)
    _chk(df1, "df1", (NS, K), device=dev)
    _chk(a1, "a1", (K, FP), device=dev)
    _chk(a2, "a2", (K, FP), device=dev)
    fts_drop = _check_drop(fts_drop, "fts_drop")
    dH = torch.empty((NS, D), dtype=torch.float32, device=dev)
    df2 = torch.empty((NS, K), dtype=torch.float32, device=dev)
    # (a live graph, CSRGraph.with_live_columns, stays on the row / chunk kernels: the lean kernels read the whole row 0 of
    # the table for every slot past the end of a row piece, and row 0 may be a row nobody has written there)
    lean_b = not graph_t.masked and not graph_t.empty_rows_mid and _use_lean(graph_t, H)
    split, _keep = _row_split_arg(graph_t, "b", bins=not lean_b, split=not lean_b)
    dense, _keep_d = _dense_arg(graph_t, False, "b") if (lean_b and table_gid is None and _use_dense(graph_t, H, K, FP)) else (None, None)
    with _k2_timed("bwd_cols", NS, graph_t.nnz):
        _lib.check(lib.han_node_attn_bwd_cols(
            graph_t.rowptr.data_ptr(), graph_t.colidx.data_ptr(),
            _ptr(graph_t.values), gs_tab.data_ptr(), _ptr(table_gid), H.data_ptr(),
            tcode, f2.data_ptr(), df1.data_ptr(), a1.data_ptr(), a2.data_ptr(), dH.data_ptr(), df2.data_ptr(),
            NS, graph_t.nnz, K, FP, LEAKY_SLOPE, _check_drop(coef_drop, "coef_drop"), fts_drop,
            int(seed), _dev_word(seed_dev), int(src_offset), int(dst_offset),
            (FLAG_XCD_ORDER if graph_t.has_locality() else 0) | (FLAG_MASKED_EDGES if graph_t.masked else 0)
            | (FLAG_LEAN if lean_b else 0) | (FLAG_K2_FULL_GATHER if K2_FULL_GATHER else 0)
            | (FLAG_K2_ZERO_ROWS if zero_rows else 0),
            ctypes.byref(split) if split is not None else None,
            ctypes.byref(dense) if dense is not None else None, _stream()), "han_node_attn_bwd_cols")
    return (dH, df2, False) if scores_out is not None else (dH, df2)


def node_attn_bwd_cols_scores(graph_t: CSRGraph, gs_tab, H, f2, df1, a1, a2, coef_drop=0.0, fts_drop=0.0, seed=0,
                              src_offset=0, dst_offset=0, table_gid=None, seed_dev=None, zero_rows=False, *, out):
    """node_attn_bwd_cols and score_param_bwd in one pass (han_node_attn_bwd_cols_scores): the gather also sums
    da1, da2 (K,F'), db1, db2 (K,) over all source rows, into the 4 tensors of `out`, from the H rows, df1 and df2 it
    holds anyway.  Returns (dH, df2) -- the bytes of node_attn_bwd_cols -- or None, with nothing launched and
    `out` untouched, where the library has no such form (small graphs on the lean / dense kernels, the masked backward,
    graphs with rows beyond the split length; han_hip.h): the caller then makes the two calls."""
    lib = _lib.load()
    K, FP = a1.shape
    _check_heads(K, FP)
    NS = graph_t.n_rows
    dev = H.device
    _chk(H, "H", (NS, D), dtype=H.dtype)
    tcode = _dtype_code(H, "H")
    _chk(gs_tab, "gs", (graph_t.n_cols, gs_row_bytes(K, FP, H.dtype)), device=dev, dtype=torch.uint8)
    if table_gid is not None:
        _chk(table_gid, "table_gid", (graph_t.n_cols,), dtype=torch.int32, device=dev)
    _chk(f2, "f2", (NS, K), device=dev)
    _chk(df1, "df1", (NS, K), device=dev)
    _chk(a1, "a1", (K, FP), device=dev)
    _chk(a2, "a2", (K, FP), device=dev)
    fts_drop = _check_drop(fts_drop, "fts_drop")
    coef_drop = _check_drop(coef_drop, "coef_drop")
    da1 = _out(out[0], "da1", (K, FP), dev)
    da2 = _out(out[1], "da2", (K, FP), dev)
    db1 = _out(out[2], "db1", (K,), dev)
    db2 = _out(out[3], "db2", (K,), dev)
    lean_b = not graph_t.masked and not graph_t.empty_rows_mid and _use_lean(graph_t, H)      # as node_attn_bwd_cols: declined
    split, _keep = _row_split_arg(graph_t, "b", bins=not lean_b, split=not lean_b)
    dH = torch.empty((NS, D), dtype=torch.float32, device=dev)
    df2 = torch.empty((NS, K), dtype=torch.float32, device=dev)
    ws = _ws(lib.han_node_attn_bwd_cols_scores_workspace(NS, K, FP), dev, "score_cols")
    with _k2_timed("bwd_cols", NS, graph_t.nnz):
        code = lib.han_node_attn_bwd_cols_scores(
            graph_t.rowptr.data_ptr(), graph_t.colidx.data_ptr(),
            _ptr(graph_t.values), gs_tab.data_ptr(), _ptr(table_gid), H.data_ptr(),
            tcode, f2.data_ptr(), df1.data_ptr(), a1.data_ptr(), a2.data_ptr(), dH.data_ptr(), df2.data_ptr(),
            NS, graph_t.nnz, K, FP, LEAKY_SLOPE, coef_drop, fts_drop,
            int(seed), _dev_word(seed_dev), int(src_offset), int(dst_offset),
            (FLAG_XCD_ORDER if graph_t.has_locality() else 0) | (FLAG_MASKED_EDGES if graph_t.masked else 0)
            | (FLAG_LEAN if lean_b else 0) | (FLAG_K2_FULL_GATHER if K2_FULL_GATHER else 0)
            | (FLAG_K2_ZERO_ROWS if zero_rows else 0),
            ctypes.byref(split) if split is not None else None, None,
            da1.data_ptr(), da2.data_ptr(), db1.data_ptr(), db2.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    if code == _lib.E_NOT_ELIGIBLE:
        return None
    _lib.check(code, "han_node_attn_bwd_cols_scores")
    return dH, df2


def score_param_bwd(H, df1, df2, K=8, FP=8, out=None):
    """da1, da2 (K,F'), db1, db2 (K,) [written to the 4 tensors of `out` when given]."""
    lib = _lib.load()
    _check_heads(K, FP)
    N = H.shape[0]
    dev = H.device
    _chk(H, "H", (N, D), dtype=H.dtype)
    tcode = _dtype_code(H, "H")
    _chk(df1, "df1", (N, K), device=dev)
    _chk(df2, "df2", (N, K), device=dev)
    o = out if out is not None else (None,) * 4
    da1 = _out(o[0], "da1", (K, FP), dev)
    da2 = _out(o[1], "da2", (K, FP), dev)
    db1 = _out(o[2], "db1", (K,), dev)
    db2 = _out(o[3], "db2", (K,), dev)
    ws = _ws(lib.han_score_param_bwd_workspace(N, K, FP), dev, "score")
    _lib.check(lib.han_score_param_bwd(
        H.data_ptr(), tcode, df1.data_ptr(), df2.data_ptr(), da1.data_ptr(), da2.data_ptr(),
        db1.data_ptr(), db2.data_ptr(), ws.data_ptr(), ws.numel(), N, K, FP, _stream()),
        "han_score_param_bwd")
    return da1, da2, db1, db2


# --------------------------------------------------------------------------- K3
def sem_attn_fwd(M, w_omega, b_omega, u_omega, flags=0, live=None, out=None):
    """utils/layers.py:152-159.  M (N,P,D) -> Z (N,D), beta (N,P).
    live: (n_live,) int32 ascending node ids (han_sem_attn_fwd_live): only the rows of these nodes of M are read and only
    their rows of Z and beta are written -- the listed rows get the bits of the full call from 65 536 rows of M on --;
    the other rows of the full-size outputs are uninitialised memory (or what `out` = (Z, beta) held).  Where the
    library does not take the shape over a list (han_hip.h), the full entry runs: every row of M is then read."""
    lib = _lib.load()
    _chk(M, "M")
    if M.dim() != 3 or M.shape[2] % 64 != 0 or M.shape[2] == 0:
        raise ValueError(f"M: expected (N,P,D) with D a multiple of 64, got {tuple(M.shape)}")
    N, P, Dm = M.shape
    A = w_omega.shape[1]
    dev = M.device
    _chk(w_omega, "w_omega", (Dm, A), device=dev)
    _chk(b_omega, "b_omega", (A,), device=dev)
    _chk(u_omega, "u_omega", (A,), device=dev)
    Z = _out(None if out is None else out[0], "Z", (N, Dm), dev)
    beta = _out(None if out is None else out[1], "beta", (N, P), dev)
    if live is not None:
        if live.dim() != 1 or live.numel() > N:
            raise ValueError(f"live: expected at most {N} node ids, got {tuple(live.shape)}")
        _chk(live, "live", (live.numel(),), dtype=torch.int32, device=dev)
        code = lib.han_sem_attn_fwd_live(M.data_ptr(), w_omega.data_ptr(), b_omega.data_ptr(), u_omega.data_ptr(),
                                         Z.data_ptr(), beta.data_ptr(), _ptr_nonempty(live), live.numel(), N, P, Dm, A,
                                         int(flags), _stream())
        if code != _lib.E_UNSUPPORTED:
            _lib.check(code, "han_sem_attn_fwd_live")
            return Z, beta
    _lib.check(lib.han_sem_attn_fwd(M.data_ptr(), w_omega.data_ptr(), b_omega.data_ptr(),
                                    u_omega.data_ptr(), Z.data_ptr(), beta.data_ptr(), N, P, Dm, A,
                                    int(flags), _stream()), "han_sem_attn_fwd")
    return Z, beta


def sem_attn_bwd(M, w_omega, b_omega, u_omega, beta, dZ, out=None, flags=0):
    """dM, dw, db, du [the last three written to the tensors of `out` when given]."""
    lib = _lib.load()
    N, P, Dm = M.shape
    A = w_omega.shape[1]
    dev = M.device
    _chk(M, "M", (N, P, Dm))
    _chk(beta, "beta", (N, P), device=dev)
    _chk(dZ, "dZ", (N, Dm), device=dev)
    dM = torch.empty_like(M)
    o = out if out is not None else (None,) * 3
    dw = _out(o[0], "dw", tuple(w_omega.shape), dev)
    db = _out(o[1], "db", tuple(b_omega.shape), dev)
    du = _out(o[2], "du", tuple(u_omega.shape), dev)
    ws = _ws(lib.han_sem_attn_bwd_workspace(N, P, Dm, A), dev, "sem")
    _lib.check(lib.han_sem_attn_bwd(
        M.data_ptr(), w_omega.data_ptr(), b_omega.data_ptr(), u_omega.data_ptr(), beta.data_ptr(),
        dZ.data_ptr(), dM.data_ptr(), dw.data_ptr(), db.data_ptr(), du.data_ptr(), ws.data_ptr(),
        ws.numel(), N, P, Dm, A, int(flags), _stream()), "han_sem_attn_bwd")
    return dM, dw, db, du


SEM_MEAN_GRID_CAP = 1024        # most blocks of any kernel of sem_attn_mean.hip (kMeanStreamBlocks)
SEM_MEAN_ROWS_PER_BLOCK = 64    # rows of M per block iteration (ROWS there); the combine kernel takes 16 or 8 NODES
SEM_MEAN_D = (64, 128)          # shapes of han_sem_attn_mean_fwd / _bwd (after zero-padding to multiples of 64)
SEM_MEAN_A = (64, 128, 192, 256)
SEM_MEAN_MAX_P = 64


def _sem_mean_args(M, w_omega, b_omega, u_omega):
    _chk(M, "M")
    if M.dim() != 3 or M.shape[2] % 64 != 0 or M.shape[2] == 0:
        raise ValueError(f"M: expected (N,P,D) with D a multiple of 64, got {tuple(M.shape)}")
    N, P, Dm = M.shape
    dev = M.device
    if w_omega.dim() != 2:
        raise ValueError(f"w_omega: expected (D,A), got {tuple(w_omega.shape)}")
    A = w_omega.shape[1]
    _chk(w_omega, "w_omega", (Dm, A), device=dev)
    _chk(b_omega, "b_omega", (A,), device=dev)
    _chk(u_omega, "u_omega", (A,), device=dev)
    return N, P, Dm, A, dev


def sem_attn_mean_fwd(M, w_omega, b_omega, u_omega, flags=0, out=None, want_mean=False):
    """han.pdf eq. 7-9: one weight per meta-path.  M (N,P,D) -> Z (N,D), beta (P,) [, the node means of the scores
    (P,) float64].  out = (Z, beta) destinations.  D in SEM_MEAN_D, A in SEM_MEAN_A, P <= SEM_MEAN_MAX_P."""
    lib = _lib.load()
    N, P, Dm, A, dev = _sem_mean_args(M, w_omega, b_omega, u_omega)
    Z = _out(None if out is None else out[0], "Z", (N, Dm), dev)
    beta = _out(None if out is None else out[1], "beta", (P,), dev)
    wmean = torch.empty((P,), dtype=torch.float64, device=dev) if want_mean else None
    ws = _ws(lib.han_sem_attn_mean_workspace(N, P, Dm, A), dev, "semmean")
    _lib.check(lib.han_sem_attn_mean_fwd(
        M.data_ptr(), w_omega.data_ptr(), b_omega.data_ptr(), u_omega.data_ptr(), Z.data_ptr(), beta.data_ptr(),
        None if wmean is None else wmean.data_ptr(), ws.data_ptr(), ws.numel(), N, P, Dm, A, int(flags), _stream()),
        "han_sem_attn_mean_fwd")
    return (Z, beta, wmean) if want_mean else (Z, beta)


def sem_attn_mean_bwd(M, w_omega, b_omega, u_omega, beta, dZ, out=None, flags=0):
    """dM, dw, db, du of sem_attn_mean_fwd [the last three written to the tensors of `out` when given]."""
    lib = _lib.load()
    N, P, Dm, A, dev = _sem_mean_args(M, w_omega, b_omega, u_omega)
    _chk(beta, "beta", (P,), device=dev)
    _chk(dZ, "dZ", (N, Dm), device=dev)
    dM = torch.empty_like(M)
    o = out if out is not None else (None,) * 3
    dw = _out(o[0], "dw", tuple(w_omega.shape), dev)
    db = _out(o[1], "db", tuple(b_omega.shape), dev)
    du = _out(o[2], "du", tuple(u_omega.shape), dev)
    if N == 0:      # the entry launches nothing
        for g in (dw, db, du):
            g.zero_()
        return dM, dw, db, du
    ws = _ws(lib.han_sem_attn_mean_workspace(N, P, Dm, A), dev, "semmean")
    _lib.check(lib.han_sem_attn_mean_bwd(
        M.data_ptr(), w_omega.data_ptr(), b_omega.data_ptr(), u_omega.data_ptr(), beta.data_ptr(),
        dZ.data_ptr(), dM.data_ptr(), dw.data_ptr(), db.data_ptr(), du.data_ptr(), ws.data_ptr(),
        ws.numel(), N, P, Dm, A, int(flags), _stream()), "han_sem_attn_mean_bwd")
    return dM, dw, db, du


def sem_attn_bwd_rows(M, w_omega, b_omega, u_omega, beta, dZ, paths, c, dc, activation=ACT_ELU, K=8, FP=8,
                      table_dtype=torch.float32, out=None, flags=0, gs_out=None, df1_out=None, live=None):
    """sem_attn_bwd with node_attn_bwd_rows of every meta-path in its epilogue, for an M (N,P,D) that is the K2 output
    of P node_attn_fwd calls and has no other consumer: no dM.  paths: per meta-path (aggp, tsum, f1, lse) as
    node_attn_bwd_rows takes them; c (P,D).  Returns (gs list, df1 list, dw, db, du) [dw, db, du written to the tensors
    of `out` when given] and writes dc (P,D) -- or None, with nothing launched, when the library does not take the shape
    (han_hip.h: han_sem_attn_bwd_rows decides, before any launch; the rule is written down there and nowhere else); the
    caller then runs the two ops.  gs_out / df1_out: optional lists of P
    preallocated destinations (N, row_bytes) uint8 / (N,K).
    live: (n_live,) int32 ascending node ids (han_sem_attn_bwd_rows_live): only the rows of these nodes are read, and
    only their rows of gs / df1 are written -- every other row of the destinations keeps what it held (pass df1_out
    whose other rows are zero: the gather and score_param_bwd read df1 of every source row) --, and dw, db, du, dc are
    the sums over them: what the full call gives when dZ is zero in every other row."""
    lib = _lib.load()
    N, P, Dm = M.shape
    A = w_omega.shape[1]
    dev = M.device
    _chk(M, "M", (N, P, Dm))
    _chk(beta, "beta", (N, P), device=dev)
    _chk(dZ, "dZ", (N, Dm), device=dev)
    _chk(c, "c", (P, D), device=dev)
    _chk(dc, "dc", (P, D), device=dev)
    if len(paths) != P:
        raise ValueError(f"paths: expected {P} entries, got {len(paths)}")
    for aggp, tsum, f1, lse in paths:
        for t, n, s in ((aggp, "aggp", (N, D)), (tsum, "tsum", (N, K)), (f1, "f1", (N, K)), (lse, "lse", (N, K))):
            _chk(t, n, s, device=dev)
    o = out if out is not None else (None,) * 3
    dw = _out(o[0], "dw", tuple(w_omega.shape), dev)
    db = _out(o[1], "db", tuple(b_omega.shape), dev)
    du = _out(o[2], "du", tuple(u_omega.shape), dev)
    _check_heads(K, FP)
    rb = gs_row_bytes(K, FP, table_dtype)
    gs = [torch.empty((N, rb), dtype=torch.uint8, device=dev) if gs_out is None else
          _chk(gs_out[p], "gs_out", (N, rb), dtype=torch.uint8, device=dev) for p in range(P)]
    df1 = [_out(None if df1_out is None else df1_out[p], "df1_out", (N, K), dev) for p in range(P)]
    ws = _ws(lib.han_sem_attn_bwd_rows_workspace(N, P, Dm, A), dev, "semrows")
    arr = lambda ts: (ctypes.c_void_p * P)(*[t.data_ptr() for t in ts])
    head = (M.data_ptr(), w_omega.data_ptr(), b_omega.data_ptr(), u_omega.data_ptr(), beta.data_ptr(), dZ.data_ptr(),
            arr([p[0] for p in paths]), arr([p[1] for p in paths]), arr([p[2] for p in paths]), arr([p[3] for p in paths]),
            c.data_ptr(), arr(gs), arr(df1), dw.data_ptr(), db.data_ptr(), du.data_ptr(), dc.data_ptr(), ws.data_ptr(),
            ws.numel())
    tail = (N, P, Dm, A, K, FP, DTYPE_CODE[table_dtype], int(activation), int(flags), _stream())
    if live is None:
        name = "han_sem_attn_bwd_rows"
        code = lib.han_sem_attn_bwd_rows(*head, *tail)
    else:
        if live.dim() != 1 or live.numel() > N:
            raise ValueError(f"live: expected at most {N} node ids, got {tuple(live.shape)}")
        _chk(live, "live", (live.numel(),), dtype=torch.int32, device=dev)
        name = "han_sem_attn_bwd_rows_live"
        code = lib.han_sem_attn_bwd_rows_live(*head, _ptr_nonempty(live), live.numel(), *tail)
    if code == _lib.E_UNSUPPORTED:
        return None
    _lib.check(code, name)
    return gs, df1, dw, db, du


# ------------------------------------------------------------- classifier + loss
def _classifier_args(Z, Wc, bc):
    """The checks classifier_loss and classifier_bwd share; returns (N, device, HC, D, C)."""
    _chk(Z, "Z")
    N, dev = Z.shape[0], Z.device
    HC, Dm, C = Wc.shape
    if Dm % 64 != 0 or Dm == 0:
        raise ValueError(f"Wc: the embedding width must be a multiple of 64 (zero-pad it), got {Dm}")
    _chk(Z, "Z", (N, Dm))
    _chk(Wc, "Wc", (HC, Dm, C), device=dev)
    _chk(bc, "bc", (HC, C), device=dev)
    return N, dev, HC, Dm, C


def classifier_loss(Z, Wc, bc, labels, mask, row_weight, backward=False, grad_out=None, live=None):
    """models/gat.py:65-72 + models/base_gattn.py:41-48,61-69.
    Z (N,D); Wc (HC,D,C); bc (HC,C); labels int32 (N,); mask uint8 (N,).
    Returns logits (N,C), loss_acc (2,) [masked CE, masked accuracy] and, if
    backward, (dZ, dWc, dbc) [dWc, dbc written to the tensors of grad_out when given].
    live: (n_live,) int32 ascending node ids (han_classifier_loss_live): only these rows of Z are read -- the others may
    hold anything --, only their rows of logits and dZ are written (the full call's bits; the other rows are
    uninitialised memory), and the loss, the accuracy, dWc and dbc are sums over them, mask still applied per row.
    The fused shapes only (D in {64, 128}, C <= 64): anything else raises."""
    lib = _lib.load()
    N, dev, HC, Dm, C = _classifier_args(Z, Wc, bc)
    _chk(labels, "labels", (N,), dtype=torch.int32, device=dev)
    _chk(mask, "mask", (N,), dtype=torch.uint8, device=dev)
    logits = torch.empty((N, C), dtype=torch.float32, device=dev)
    loss_acc = torch.empty((2,), dtype=torch.float32, device=dev)
    grads = None
    ptrs = (None, None, None)
    if backward:
        dZ = torch.empty((N, Dm), dtype=torch.float32, device=dev)
        go = grad_out if grad_out is not None else (None, None)
        dWc = _out(go[0], "dWc", tuple(Wc.shape), dev)
        dbc = _out(go[1], "dbc", tuple(bc.shape), dev)
        grads = (dZ, dWc, dbc)
        ptrs = (dZ.data_ptr(), dWc.data_ptr(), dbc.data_ptr())
    ws = _ws(lib.han_classifier_workspace(N, Dm, C, HC), dev, "cls")
    if live is not None:
        if live.dim() != 1 or live.numel() > N:
            raise ValueError(f"live: expected at most {N} node ids, got {tuple(live.shape)}")
        _chk(live, "live", (live.numel(),), dtype=torch.int32, device=dev)
        _lib.check(lib.han_classifier_loss_live(
            Z.data_ptr(), Wc.data_ptr(), bc.data_ptr(), labels.data_ptr(), mask.data_ptr(),
            float(row_weight), logits.data_ptr(), loss_acc.data_ptr(), ptrs[0], ptrs[1], ptrs[2],
            ws.data_ptr(), ws.numel(), _ptr_nonempty(live), live.numel(), N, Dm, C, HC, _stream()),
            "han_classifier_loss_live")
        return logits, loss_acc, grads
    _lib.check(lib.han_classifier_loss(
        Z.data_ptr(), Wc.data_ptr(), bc.data_ptr(), labels.data_ptr(), mask.data_ptr(),
        float(row_weight), logits.data_ptr(), loss_acc.data_ptr(), ptrs[0], ptrs[1], ptrs[2],
        ws.data_ptr(), ws.numel(), N, Dm, C, HC, _stream()), "han_classifier_loss")
    return logits, loss_acc, grads


def label_words(C: int) -> int:
    """64-bit words per row of a packed (N, C) multi-hot label matrix."""
    return (int(C) + 63) // 64


PACK_ROWS = 65536      # rows per step of pack_label_bits


def pack_label_bits(y):
    """(N, C) bool / 0-1 labels -> (N, ceil(C/64)) packed words, class c of a row at bit c % 64 of word c / 64: the
    `label_bits` of han_classifier_multilabel.  The words are stored as int64 (torch has no arithmetic on uint64); the
    kernels read the same 8 bytes as uint64.  Plain torch on the device of `y`: it runs once per data set."""
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError(f"labels: expected an (N, C) multi-hot tensor, got {type(y).__name__} "
                         f"{tuple(y.shape) if isinstance(y, torch.Tensor) else ''}")
    N, C = y.shape
    if C < 1:
        raise ValueError("labels: at least one class")
    if not bool(((y == 0) | (y == 1)).all()):
        raise ValueError("labels: a multi-hot matrix holds only 0 and 1")
    nw = label_words(C)
    out = torch.empty((N, nw), dtype=torch.int64, device=y.device)
    # bit 63 is the sign bit of the stored word: 1 << 63 wraps to the most negative int64, which is that bit pattern
    shifts = torch.arange(64, dtype=torch.int64, device=y.device)
    # in row chunks, so that the transient (rows, nw * 64) int64 image stays at about 32 MB per word whatever N is
    for r0 in range(0, N, PACK_ROWS):
        yc = y[r0:r0 + PACK_ROWS]
        b = torch.zeros((yc.shape[0], nw * 64), dtype=torch.int64, device=y.device)
        b[:, :C] = yc.to(torch.int64)
        out[r0:r0 + PACK_ROWS] = b.view(-1, nw, 64).bitwise_left_shift_(shifts).sum(-1)
    return out


def unpack_label_bits(words, C: int):
    """The (N, C) uint8 multi-hot matrix of packed label words (pack_label_bits)."""
    N, nw = words.shape
    shifts = torch.arange(64, dtype=torch.int64, device=words.device)
    return ((words.view(N, nw, 1) >> shifts) & 1).view(N, nw * 64)[:, :C].to(torch.uint8)


def classifier_multilabel(Z, Wc, bc, label_bits, mask, row_weight, backward=False, grad_out=None, live=None):
    """models/gat.py:65-72 + models/base_gattn.py:50-59,71-94: the multi-label objective (han_classifier_multilabel).
    Z (N,D); Wc (HC,D,C); bc (HC,C); label_bits int64 (N, ceil(C/64)) from pack_label_bits; mask uint8 (N,).
    Returns logits (N,C), loss_acc (2,) [masked sigmoid cross-entropy, micro-F1], counts (3,) int64 [tp, fp, fn] and, if
    backward, (dZ, dWc, dbc) [dWc, dbc written to the tensors of grad_out when given].  live: as classifier_loss --
    only these rows are read and written, the sums and counts run over them; the fused shapes only."""
    lib = _lib.load()
    N, dev, HC, Dm, C = _classifier_args(Z, Wc, bc)
    _chk(label_bits, "label_bits", (N, label_words(C)), dtype=torch.int64, device=dev)
    _chk(mask, "mask", (N,), dtype=torch.uint8, device=dev)
    logits = torch.empty((N, C), dtype=torch.float32, device=dev)
    loss_acc = torch.empty((2,), dtype=torch.float32, device=dev)
    counts = torch.empty((3,), dtype=torch.int64, device=dev)
    grads = None
    ptrs = (None, None, None)
    if backward:
        dZ = torch.empty((N, Dm), dtype=torch.float32, device=dev)
        go = grad_out if grad_out is not None else (None, None)
        dWc = _out(go[0], "dWc", tuple(Wc.shape), dev)
        dbc = _out(go[1], "dbc", tuple(bc.shape), dev)
        grads = (dZ, dWc, dbc)
        ptrs = (dZ.data_ptr(), dWc.data_ptr(), dbc.data_ptr())
    ws = _ws(lib.han_classifier_multilabel_workspace(N, Dm, C, HC), dev, "clsml")
    live_ptr, n_live = None, 0
    if live is not None:
        if live.dim() != 1 or live.numel() > N:
            raise ValueError(f"live: expected at most {N} node ids, got {tuple(live.shape)}")
        _chk(live, "live", (live.numel(),), dtype=torch.int32, device=dev)
        # an empty list still means "no row": the C ABI tells a list from "every row" by the pointer
        live_ptr, n_live = (live.data_ptr() if live.numel() else ws.data_ptr()), live.numel()
    _lib.check(lib.han_classifier_multilabel(
        Z.data_ptr(), Wc.data_ptr(), bc.data_ptr(), label_bits.data_ptr(), mask.data_ptr(), float(row_weight),
        logits.data_ptr(), loss_acc.data_ptr(), counts.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ws.data_ptr(), ws.numel(),
        live_ptr, n_live, N, Dm, C, HC, _stream()), "han_classifier_multilabel")
    return logits, loss_acc, counts, grads


def classifier_bwd(Z, Wc, bc, dlogits):
    """Backward of logits = (1/HC) sum_h (Z Wc[h] + bc[h]) (models/gat.py:65-72) for a given dlogits (N,C):
    returns (dZ, dWc, dbc)."""
    lib = _lib.load()
    N, dev, HC, Dm, C = _classifier_args(Z, Wc, bc)
    _chk(dlogits, "dlogits", (N, C), device=dev)
    dZ = torch.empty((N, Dm), dtype=torch.float32, device=dev)
    dWc, dbc = torch.empty_like(Wc), torch.empty_like(bc)
    ws = _ws(lib.han_classifier_bwd_workspace(N, Dm, C, HC), dev, "clsb")
    _lib.check(lib.han_classifier_bwd(Z.data_ptr(), Wc.data_ptr(), bc.data_ptr(), dlogits.data_ptr(), dZ.data_ptr(),
                                      dWc.data_ptr(), dbc.data_ptr(), ws.data_ptr(), ws.numel(), N, Dm, C, HC,
                                      _stream()), "han_classifier_bwd")
    return dZ, dWc, dbc


# ------------------------------------------------------------------- optimiser
def adam_step(param, grad, m, v, lr_t, beta1=0.9, beta2=0.999, eps=1e-8, l2_coef=0.0, step_dev=None):
    """lr_t = lr*sqrt(1-b2^t)/(1-b1^t) from the caller, or -- with step_dev (device step
    count t) -- the base rate lr, the correction then being computed on the device."""
    lib = _lib.load()
    n = param.numel()
    for t, nme in ((param, "param"), (grad, "grad"), (m, "m"), (v, "v")):
        _chk(t, nme, (n,), device=param.device)
    _lib.check(lib.han_adam_step(param.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n,
                                 float(lr_t), float(beta1), float(beta2), float(eps),
                                 float(l2_coef), _dev_word(step_dev), _stream()), "han_adam_step")


def l2_half_sumsq(param):
    lib = _lib.load()
    _chk(param, "param", (param.numel(),))
    out = torch.empty((1,), dtype=torch.float32, device=param.device)
    ws = _ws(4096 * 4, param.device, "l2")
    _lib.check(lib.han_l2_half_sumsq(param.data_ptr(), param.numel(), out.data_ptr(),
                                     ws.data_ptr(), ws.numel(), _stream()), "han_l2_half_sumsq")
    return out


# ------------------------------------------------------- K0: meta-path graphs
SPGEMM_DIAG = 1            # HAN_SPGEMM_DIAG
SPGEMM_MAX_SHORT = 4096    # HAN_SPGEMM_MAX_SHORT
SPGEMM_MAX_TILE = 1 << 19  # HAN_SPGEMM_MAX_TILE
# rows with at most SPGEMM_SHORT candidates are sorted in LDS by one wave, the others marked in an LDS bit map of
# SPGEMM_TILE columns by a workgroup (profiles/r05_metapath_sweep.jsonl)
SPGEMM_SHORT = 1024
SPGEMM_TILE = 1 << 17
SPGEMM_STATS: list | None = None   # tools/metapath_bench.py: csr_bool_matmul appends one dict of counts per product


def _spgemm_check(A: CSRGraph, B: CSRGraph, diag: bool):
    for g, name in ((A, "A"), (B, "B")):
        if not isinstance(g, CSRGraph):
            raise ValueError(f"{name}: expected a CSRGraph, got {type(g)}")
        require_gpu(g.rowptr, name)
    if A.device != B.device:
        raise ValueError(f"A on {A.device}, B on {B.device}")
    if A.n_cols != B.n_rows:
        raise ValueError(f"A has {A.n_cols} columns, B has {B.n_rows} rows")
    if diag and A.n_rows != B.n_cols:
        raise ValueError(f"diag needs a square product, got {A.n_rows} x {B.n_cols}")


def _spgemm_structure(A: CSRGraph, B: CSRGraph, diag: bool):
    """The launches of csr_bool_matmul: (C, the arguments count / fill / values share), the latter None for a product
    without rows."""
    _spgemm_check(A, B, diag)
    lib = _lib.load()
    n, dev = A.n_rows, A.device
    if n == 0:
        return CSRGraph(torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                        B.n_cols, validate=False), None
    flags = SPGEMM_DIAG if diag else 0
    st, ptr = _stream(), _ptr_nonempty
    ub = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(lib.han_spgemm_row_bounds(A.rowptr.data_ptr(), ptr(A.colidx), B.rowptr.data_ptr(), n, A.n_cols, flags,
                                         ub.data_ptr(), st), "han_spgemm_row_bounds")
    # the bins, on the device: rows by decreasing bound -- the long rows first, and the heaviest rows of each bin
    # are the first ones its persistent blocks take
    rows = torch.sort(ub, descending=True, stable=True).indices.to(torch.int32)
    n_long = (ub > SPGEMM_SHORT).sum().reshape(1)
    args = (A.rowptr.data_ptr(), ptr(A.colidx), B.rowptr.data_ptr(), ptr(B.colidx), n, A.n_cols, B.n_cols,
            rows.data_ptr(), n_long.data_ptr(), SPGEMM_SHORT, SPGEMM_TILE, flags)
    rowptr, colidx = csr.two_pass(
        n, dev, (torch.int32,),
        lambda counts: _lib.check(lib.han_spgemm_count(*args, counts.data_ptr(), st), "han_spgemm_count"),
        lambda rowptr, colidx: _lib.check(lib.han_spgemm_fill(*args, rowptr.data_ptr(), colidx.data_ptr(), st),
                                          "han_spgemm_fill"))
    if SPGEMM_STATS is not None:
        SPGEMM_STATS.append(dict(rows=n, cols=B.n_cols, nnz_a=A.nnz, nnz=colidx.numel(), candidates=ub.sum(),
                                 n_long=n_long))
    return CSRGraph(rowptr, colidx, B.n_cols, validate=False), (rows, n_long, SPGEMM_SHORT, SPGEMM_TILE, flags)


def csr_bool_matmul(A: CSRGraph, B: CSRGraph, diag: bool = False) -> CSRGraph:
    """Boolean product C = A B (han_spgemm_*): entry (i, j) iff some l has (i, l) in A and (l, j) in B, and with
    diag=True also (i, i) (square products).  A and B may hold unsorted or repeated columns; their values are
    ignored.  C has strictly increasing columns in every row and values None.  Row bounds, count and fill launches,
    the rows binned by their bound on the device; the one host sync reads nnz(C)."""
    return _spgemm_structure(A, B, diag)[0]


def _entry_counts(t, name, graph: CSRGraph):
    if t is None:
        return None
    _chk(t, name, (graph.nnz,), dtype=torch.int64, device=graph.device)
    return t


def csr_count_matmul(A: CSRGraph, B: CSRGraph, a_counts=None, b_counts=None, diag: bool = False):
    """Counted product C = A B over the integers (han_spgemm_values after the launches of csr_bool_matmul):
    (graph, counts) with the graph bitwise that of csr_bool_matmul(A, B, diag) and counts (nnz,) int64 on the device,
    counts[e] = sum over l of a_il b_lj for the entry e = (i, j).  a_counts / b_counts: (nnz,) int64 per stored entry
    of A / B, None = every stored entry is 1; a repeated stored entry counts once per repetition.  An (i, i) that only
    diag=True added has count 0.  Sums are int64 (no check for wrap-around beyond 2^63) and integer adds only, so the
    result is bitwise reproducible."""
    _spgemm_check(A, B, diag)
    a_counts, b_counts = _entry_counts(a_counts, "a_counts", A), _entry_counts(b_counts, "b_counts", B)
    C, bins = _spgemm_structure(A, B, diag)
    counts = torch.empty(C.nnz, dtype=torch.int64, device=C.device)
    if C.nnz:
        (rows, n_long, short_max, tile_cols, flags), ptr = bins, _ptr_nonempty
        _lib.check(_lib.load().han_spgemm_values(
            A.rowptr.data_ptr(), ptr(A.colidx), ptr(a_counts), B.rowptr.data_ptr(), ptr(B.colidx), ptr(b_counts),
            A.n_rows, A.n_cols, B.n_cols, rows.data_ptr(), n_long.data_ptr(), short_max, tile_cols, flags,
            C.rowptr.data_ptr(), C.colidx.data_ptr(), C.nnz, counts.data_ptr(), _stream()), "han_spgemm_values")
    return C, counts


def csr_pathsim(graph: CSRGraph, counts: torch.Tensor) -> torch.Tensor:
    """PathSim values (nnz,) fp32 of a square counted graph with strictly increasing columns per row (a K0 product):
    w_ij = 2 c_ij / (c_ii + c_jj), evaluated in double and rounded once; w_ii = 1 exactly, also when c_ii = 0; a row
    that does not store its diagonal has c_ii = 0 (han_csr_pathsim)."""
    if not isinstance(graph, CSRGraph):
        raise ValueError(f"graph: expected a CSRGraph, got {type(graph)}")
    if graph.n_rows != graph.n_cols:
        raise ValueError(f"PathSim needs a square graph, got {graph.n_rows} x {graph.n_cols}")
    require_gpu(graph.rowptr, "graph")
    _chk(counts, "counts", (graph.nnz,), dtype=torch.int64, device=graph.device)
    w = torch.empty(graph.nnz, dtype=torch.float32, device=graph.device)
    if graph.nnz:
        diag = torch.empty(graph.n_rows, dtype=torch.int64, device=graph.device)
        _lib.check(_lib.load().han_csr_pathsim(graph.rowptr.data_ptr(), graph.colidx.data_ptr(), counts.data_ptr(),
                                               graph.n_rows, diag.data_ptr(), w.data_ptr(), _stream()),
                   "han_csr_pathsim")
    return w


def csr_row_topk(graph: CSRGraph, k: int, keep_diag: bool = True) -> CSRGraph:
    """Per row of a graph with values, the k entries of largest value that are not (i, i) -- ties go to the smaller
    column --, and with keep_diag also (i, i) if present; a row with at most k such entries is kept whole.  Columns
    stay ascending and values travel with them.  Rows must hold strictly increasing columns (every K0 product does).
    Values are ordered as finite floats (-0 below +0); where a NaN sorts is unspecified.  Count and fill launches
    (han_csr_row_topk_*), one host sync for the new nnz."""
    if not isinstance(graph, CSRGraph):
        raise ValueError(f"graph: expected a CSRGraph, got {type(graph)}")
    if isinstance(k, bool) or int(k) != k or k < 1:
        raise ValueError(f"k = {k!r}: expected an integer >= 1")
    if graph.values is None:
        raise ValueError("csr_row_topk: the graph has no values to rank")
    if graph.row_base:
        raise ValueError("csr_row_topk: the diagonal of a row shard (row_base != 0) is not supported")
    require_gpu(graph.rowptr, "graph")
    lib, k, n, dev, st = _lib.load(), int(k), graph.n_rows, graph.device, _stream()
    rowptr, colidx, values = csr.two_pass(
        n, dev, (torch.int32, torch.float32),
        lambda counts: _lib.check(lib.han_csr_row_topk_count(
            graph.rowptr.data_ptr(), _ptr_nonempty(graph.colidx), n, k, int(keep_diag), counts.data_ptr(), st),
            "han_csr_row_topk_count"),
        lambda rowptr, colidx, values: _lib.check(lib.han_csr_row_topk_fill(
            graph.rowptr.data_ptr(), graph.colidx.data_ptr(), graph.values.data_ptr(), n, k, int(keep_diag),
            rowptr.data_ptr(), colidx.data_ptr(), values.data_ptr(), st), "han_csr_row_topk_fill"))
    return CSRGraph(rowptr, colidx, graph.n_cols, validate=False, values=values)


WALK_MAX_HOPS = 8          # HAN_WALK_MAX_HOPS
WALK_MAX_WALKS = 4096      # HAN_WALK_MAX_WALKS


def _walk_limits(walks, fanout, seed):
    """(walks, fanout, seed) as ints, fanout None = walks; ValueError outside 1 <= fanout <= walks <= WALK_MAX_WALKS
    or a seed that is not 64 bits."""
    _chk_int(walks, "walks", 1, WALK_MAX_WALKS)
    if fanout is None:
        fanout = walks
    _chk_int(fanout, "fanout", 1, int(walks))
    _chk_int(seed, "seed", 0, (1 << 64) - 1)
    return int(walks), int(fanout), int(seed)


def _walk_rows(rows, n):
    """The start-row range (r0, r1) of `rows` (None: all n)."""
    if rows is None:
        return 0, n
    try:
        r0, r1 = rows
        ok = all(not isinstance(r, bool) and int(r) == r for r in (r0, r1))
    except (TypeError, ValueError):
        ok = False
    if not ok or not 0 <= r0 <= r1 <= n:
        raise ValueError(f"rows = {rows!r}: expected a range (r0, r1) with 0 <= r0 <= r1 <= {n}")
    return int(r0), int(r1)


def metapath_walk(hops, walks: int, fanout=None, seed: int = 0, diag: bool = False, rows=None):
    """Sampled meta-path neighbours (han_metapath_walk_*): from every start node of `rows` = (r0, r1) (default: every
    row of hops[0]) `walks` random walks along the chain `hops` (1 to 8 CSRGraphs, hops[k].n_cols == hops[k+1].n_rows;
    a repeated stored entry is as many parallel edges, a node without entries ends the walk), and per start row the
    `fanout` (None = walks) most visited end points, ties to the smaller column.  diag=True (square chains): (i, i) is
    always kept, with its own visit count (possibly 0), beside the fanout best of the others.  Returns (graph, visits):
    a CSRGraph of r1 - r0 rows (row_base = r0, global columns, strictly increasing per row, values None) and the visit
    count of every entry, int32.  The draws depend on (seed, global start node, walk, hop) only -- include/han_hip.h
    states them --, so a row range returns exactly its rows of the whole result.  Count and fill launches; the one
    host sync reads nnz."""
    hops = list(hops)
    if not 1 <= len(hops) <= WALK_MAX_HOPS:
        raise ValueError(f"metapath_walk: {len(hops)} hops, expected 1 to {WALK_MAX_HOPS}")
    for k, g in enumerate(hops):
        if not isinstance(g, CSRGraph):
            raise ValueError(f"hops[{k}]: expected a CSRGraph, got {type(g)}")
    for k in range(len(hops) - 1):
        if hops[k].n_cols != hops[k + 1].n_rows:
            raise ValueError(f"hops[{k}] has {hops[k].n_cols} columns, hops[{k + 1}] has {hops[k + 1].n_rows} rows")
    walks, fanout, seed = _walk_limits(walks, fanout, seed)
    n, n_cols = hops[0].n_rows, hops[-1].n_cols
    if diag and n != n_cols:
        raise ValueError(f"diag needs a square result, got {n} x {n_cols}")
    r0, r1 = _walk_rows(rows, n)
    for k, g in enumerate(hops):
        require_gpu(g.rowptr, f"hops[{k}]")
        if g.device != hops[0].device:
            raise ValueError(f"hops[{k}] on {g.device}, hops[0] on {hops[0].device}")
        if g.nnz >= 1 << 32 and int(g.degrees().max()) >= 1 << 32:      # (only such a graph costs a sync of its own)
            raise ValueError(f"hops[{k}] has a row of 2^32 entries or more: the draw is a 32-bit word")
    lib, dev, st, L, m = _lib.load(), hops[0].device, _stream(), len(hops), r1 - r0
    rps = (ctypes.c_void_p * L)(*[g.rowptr.data_ptr() for g in hops])
    cis = (ctypes.c_void_p * L)(*[g.colidx.data_ptr() if g.nnz else None for g in hops])
    nrs = (ctypes.c_int64 * L)(*[g.n_rows for g in hops])
    args = (ctypes.cast(rps, ctypes.c_void_p), ctypes.cast(cis, ctypes.c_void_p), ctypes.cast(nrs, ctypes.c_void_p),
            L, n_cols, r0, m, walks, fanout, seed, int(bool(diag)))
    rowptr, colidx, visits = csr.two_pass(
        m, dev, (torch.int32, torch.int32),
        lambda counts: _lib.check(lib.han_metapath_walk_count(*args, counts.data_ptr(), st), "han_metapath_walk_count"),
        lambda rowptr, colidx, visits: _lib.check(lib.han_metapath_walk_fill(
            *args, rowptr.data_ptr(), colidx.data_ptr(), visits.data_ptr(), st), "han_metapath_walk_fill"))
    return CSRGraph(rowptr, colidx, n_cols, validate=False, row_base=r0), visits


# ------------------------------------------------- K0: ego blocks (han_ego_*, csrc/ego_block.hip)
def _long_rows_arg(split):
    """The chunk-table arguments of han_ego_expand / han_ego_fill from CSRGraph.row_split's dict (None: no long row)."""
    if split is None:
        return (0, 0, None, None, None, None)
    return (split["split_deg"], split["n_chunks"], split["long_rows"].data_ptr(), split["chunk_long"].data_ptr(),
            split["chunk_start"].data_ptr(), split["chunk_end"].data_ptr())


def ego_expand(graph: CSRGraph, level: torch.Tensor, h: int, split=None):
    """One breadth-first hop over `graph`, in place: every row with level == h writes h + 1 into the level of its
    unvisited (-1) columns.  level: (n,) int32 on the graph's device; split: graph.row_split(...) or None."""
    _chk(level, "level", (graph.n_rows,), dtype=torch.int32, device=graph.device)
    _lib.check(_lib.load().han_ego_expand(graph.rowptr.data_ptr(), _ptr_nonempty(graph.colidx), graph.n_rows, int(h),
                                          *_long_rows_arg(split), level.data_ptr(), _stream()), "han_ego_expand")


def ego_count(rowptr: torch.Tensor, rows: torch.Tensor, counts: torch.Tensor, level=None, hops: int = 1):
    """counts[r] = the entries of output row r: those of row rows[r] of `rowptr` where it is kept (level None: always;
    else 0 <= level[rows[r]] < hops), 1 on the rim.  rows (n_out,) int64, counts (n_out,) int64, written in place."""
    _chk(rows, "rows", dtype=torch.int64, device=rowptr.device)
    _chk(counts, "counts", (rows.numel(),), dtype=torch.int64, device=rowptr.device)
    _lib.check(_lib.load().han_ego_count(rowptr.data_ptr(), _ptr_nonempty(rows), _ptr(level), int(hops),
                                         rowptr.numel() - 1, rows.numel(), _ptr_nonempty(counts), _stream()),
               "han_ego_count")


def ego_fill(rowptr, colidx, values, rows, n_cols, out_rowptr, out_colidx, out_values, level=None, hops: int = 1,
             local=None, split=None):
    """The output rows counted by ego_count: row rows[r] as stored (columns through `local` when given), (r, r) on the
    rim; out_values None or (nnz,) fp32 (1.0 where `values` is None or on the rim)."""
    _lib.check(_lib.load().han_ego_fill(
        rowptr.data_ptr(), _ptr_nonempty(colidx), _ptr_nonempty(values), _ptr_nonempty(rows), _ptr(level), int(hops),
        _ptr(local), rowptr.numel() - 1, int(n_cols), rows.numel(), *_long_rows_arg(split), out_rowptr.data_ptr(),
        _ptr_nonempty(out_colidx), _ptr_nonempty(out_values), _stream()), "han_ego_fill")


def _long_list_arg(split):
    """The long-row list of the han_ego_sample_* entry points from CSRGraph.row_split's dict (None: no long row)."""
    if split is None:
        return (0, 0, None)
    return (split["split_deg"], split["n_long"], split["long_rows"].data_ptr())


def ego_sample_decision(graph: CSRGraph):
    """(thr uint32 as int32 storage, need int32, kept int64), each (n,): the per-row decisions han_ego_sample_expand
    writes for the rows it expands.  Uninitialised -- but kept is zeroed for a graph without entries, which the entry
    point leaves alone."""
    n, dev = graph.n_rows, graph.device
    kept = (torch.zeros if graph.nnz == 0 else torch.empty)(n, dtype=torch.int64, device=dev)
    return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev), kept)


def ego_sample_expand(graph: CSRGraph, level: torch.Tensor, h: int, fanout: int, seed: int, p: int, decision,
                      split=None):
    """ego_expand over the sampled entries of graph number `p`: every row with level == h keeps its self entries and
    the `fanout` other entries of smallest (key, stored position) (include/han_hip.h), stores that decision and writes
    h + 1 into the level of the unvisited columns it kept."""
    _chk(level, "level", (graph.n_rows,), dtype=torch.int32, device=graph.device)
    thr, need, kept = decision
    _lib.check(_lib.load().han_ego_sample_expand(
        graph.rowptr.data_ptr(), _ptr_nonempty(graph.colidx), graph.n_rows, int(h), int(fanout),
        int(seed) & ((1 << 64) - 1), int(p), *_long_list_arg(split), level.data_ptr(), thr.data_ptr(), need.data_ptr(),
        kept.data_ptr(), _stream()), "han_ego_sample_expand")


def ego_sample_count(rows: torch.Tensor, counts: torch.Tensor, level: torch.Tensor, hops: int, decision):
    """counts[r] = the entries of sampled block row r: the stored kept count where level[rows[r]] < hops, else 1."""
    _chk(rows, "rows", dtype=torch.int64, device=level.device)
    _chk(counts, "counts", (rows.numel(),), dtype=torch.int64, device=level.device)
    _lib.check(_lib.load().han_ego_sample_count(_ptr_nonempty(rows), level.data_ptr(), int(hops),
                                                decision[2].data_ptr(), level.numel(), rows.numel(),
                                                _ptr_nonempty(counts), _stream()), "han_ego_sample_count")


def ego_sample_fill(graph: CSRGraph, rows, out_rowptr, out_colidx, out_values, level, hops: int, local, seed: int,
                    p: int, decision, split=None):
    """The rows counted by ego_sample_count: the kept entries of row rows[r] in stored order, columns through `local`;
    (r, r) on the rim; out_values None or (nnz,) fp32."""
    thr, need, _ = decision
    _lib.check(_lib.load().han_ego_sample_fill(
        graph.rowptr.data_ptr(), _ptr_nonempty(graph.colidx), _ptr_nonempty(graph.values), _ptr_nonempty(rows),
        level.data_ptr(), int(hops), local.data_ptr(), graph.n_rows, rows.numel(), int(seed) & ((1 << 64) - 1), int(p),
        *_long_list_arg(split), thr.data_ptr(), need.data_ptr(), out_rowptr.data_ptr(), _ptr_nonempty(out_colidx),
        _ptr_nonempty(out_values), _stream()), "han_ego_sample_fill")


# ------------------------------------------------- evaluation of the embeddings
KNN_MAX_K = 16             # neighbours per query of han_knn_topk
EVAL_MAX_D = 512           # embedding width of han_knn_topk / han_kmeans_step
KMEANS_MAX_K = 64          # centres of han_kmeans_step
SILHOUETTE_MAX_K = 64      # clusters of han_silhouette
CONTINGENCY_MAX_CELLS = 4096


def _chk_int(v, name, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, int) and int(v) != v or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} = {v!r}: expected an integer in [{lo}, {hi if hi is not None else 'inf'}]")
    return int(v)


def _chk_rows(t, name, device=None):
    """A 2-D fp32 GPU matrix whose rows are contiguous (a row slice or column slice of a larger one is fine);
    returns its leading dimension in elements."""
    _chk(t, name, (None, None), device=device, contiguous=False)
    if t.shape[1] < 1 or t.shape[1] > EVAL_MAX_D:
        raise ValueError(f"{name}: width {t.shape[1]}, expected 1 .. {EVAL_MAX_D}")
    if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < t.shape[1]):
        raise ValueError(f"{name}: rows must be contiguous, got strides {t.stride()}")
    if t.shape[0] <= 1 and t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must be contiguous, got strides {t.stride()}")
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def knn_topk(queries, train, k: int):
    """(idx (Nq, k) int32, d2 (Nq, k) fp32): per query row the k nearest train rows by squared Euclidean distance,
    ascending under the total order (d2, train index) -- equal distances go to the smaller index (han_knn_topk:
    brute force on the fp32 matrix pipe, the distance matrix is never stored)."""
    k = _chk_int(k, "k", 1, KNN_MAX_K)
    ldt = _chk_rows(train, "train")
    ldq = _chk_rows(queries, "queries", device=train.device)
    nq, nt, d = queries.shape[0], train.shape[0], train.shape[1]
    if queries.shape[1] != d:
        raise ValueError(f"queries have width {queries.shape[1]}, train rows {d}")
    if k > nt:
        raise ValueError(f"k = {k} neighbours of {nt} train rows")
    if nt >= 2 ** 31:
        raise ValueError("train: at most 2^31 - 1 rows")
    lib, dev = _lib.load(), train.device
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if nq:
        ws = _ws(lib.han_knn_topk_workspace(nq, nt, d, k), dev, "knn")
        _lib.check(lib.han_knn_topk(queries.data_ptr(), ldq, train.data_ptr(), ldt, idx.data_ptr(), d2.data_ptr(),
                                    ws.data_ptr(), ws.numel(), nq, nt, d, k, _stream()), "han_knn_topk")
    return idx, d2


def knn_vote(idx, labels_train):
    """pred (Nq,) int32: the most frequent of labels_train[idx[q, :]], ties to the smallest class id
    (han_knn_vote; KNeighborsClassifier(weights="uniform").predict)."""
    _chk(idx, "idx", (None, None), dtype=torch.int32)
    k = _chk_int(idx.shape[1], "k", 1, KNN_MAX_K)
    _chk(labels_train, "labels_train", (None,), dtype=torch.int32, device=idx.device)
    pred = torch.empty(idx.shape[0], dtype=torch.int32, device=idx.device)
    if idx.shape[0]:
        _lib.check(_lib.load().han_knn_vote(idx.data_ptr(), labels_train.data_ptr(), pred.data_ptr(), idx.shape[0], k,
                                            labels_train.shape[0], _stream()), "han_knn_vote")
    return pred


def contingency(a, b, ca: int, cb: int):
    """The (ca, cb) int64 count table of two int32 label vectors, table[x, y] = #{i: a[i] == x and b[i] == y}, as a
    HOST tensor (han_contingency; the one copy to the host also carries the kernel's flag word: a label outside
    [0, ca) / [0, cb) raises ValueError)."""
    ca, cb = _chk_int(ca, "ca", 1), _chk_int(cb, "cb", 1)
    if ca * cb > CONTINGENCY_MAX_CELLS:
        raise ValueError(f"contingency: {ca} x {cb} cells, at most {CONTINGENCY_MAX_CELLS}")
    _chk(a, "a", (None,), dtype=torch.int32)
    _chk(b, "b", (a.shape[0],), dtype=torch.int32, device=a.device)
    table = torch.empty(ca * cb + 1, dtype=torch.int64, device=a.device)
    _lib.check(_lib.load().han_contingency(_ptr(a) if a.numel() else None, _ptr(b) if b.numel() else None, a.shape[0],
                                           ca, cb, table.data_ptr(), _stream()), "han_contingency")
    host = table.cpu()
    if int(host[-1]) != 0:
        raise ValueError(f"contingency: a label outside [0, {ca}) x [0, {cb})")
    return host[:-1].reshape(ca, cb)


def kmeans_step(x, centres, prev=None, want_d2=True):
    """One Lloyd iteration (han_kmeans_step): dict(labels (N,) int32 -- the nearest centre, ties to the smaller
    index --, d2 (N,) fp32 or None, counts (k,) int64, centres (k, D) fp32 -- the mean of each cluster's rows, a
    cluster without rows keeps its centre --, inertia (1,) float64, changed (1,) int64 -- rows whose label differs
    from prev, N when prev is None).  Everything stays on the device."""
    ldx = _chk_rows(x, "x")
    n, d = x.shape
    _chk(centres, "centres", (None, d), device=x.device)
    k = _chk_int(centres.shape[0], "k", 1, KMEANS_MAX_K)
    if prev is not None:
        _chk(prev, "prev", (n,), dtype=torch.int32, device=x.device)
    lib, dev = _lib.load(), x.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, dtype=torch.float32, device=dev) if want_d2 else None
    counts = torch.empty(k, dtype=torch.int64, device=dev)
    new = torch.empty((k, d), dtype=torch.float32, device=dev)
    inertia = torch.empty(1, dtype=torch.float64, device=dev)
    changed = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _ws(lib.han_kmeans_step_workspace(n, d, k), dev, "kmeans")
    _lib.check(lib.han_kmeans_step(x.data_ptr() if n else None, ldx, centres.data_ptr(), _ptr(prev), labels.data_ptr() if n else None,
                                   _ptr(d2), counts.data_ptr(), new.data_ptr(), inertia.data_ptr(), changed.data_ptr(),
                                   ws.data_ptr(), ws.numel(), n, d, k, _stream()), "han_kmeans_step")
    return dict(labels=labels, d2=d2, counts=counts, centres=new, inertia=inertia, changed=changed)


def silhouette(x, seg_ptr):
    """scikit-learn's silhouette_samples (Euclidean) of rows GROUPED BY CLUSTER (han_silhouette): rows
    [seg_ptr[c], seg_ptr[c + 1]) of x are cluster c, seg_ptr a (k + 1,) int64 GPU tensor with seg_ptr[0] = 0 and
    seg_ptr[k] = N, 2 <= k <= 64; a cluster may be empty.  Returns dict(a (N,) fp32 -- the mean distance to the other
    rows of the own cluster, 0 for a cluster of one row --, b (N,) fp32 -- the smallest mean distance to another
    non-empty cluster --, s (N,) fp32 = (b - a) / max(a, b), 0 for a cluster of one row, sum (1,) float64 -- the sum
    of s).  Everything stays on the device; the pair distances are never stored."""
    ldx = _chk_rows(x, "x")
    n, d = x.shape
    _chk(seg_ptr, "seg_ptr", (None,), dtype=torch.int64, device=x.device)
    k = _chk_int(seg_ptr.shape[0] - 1, "k", 2, SILHOUETTE_MAX_K)
    if n >= 2 ** 31:
        raise ValueError("x: at most 2^31 - 1 rows")
    lib, dev = _lib.load(), x.device
    a, b, s = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))
    total = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _ws(lib.han_silhouette_workspace(n, d, k), dev, "silhouette")
    _lib.check(lib.han_silhouette(x.data_ptr() if n else None, ldx, seg_ptr.data_ptr(), n, d, k, _ptr_nonempty(a),
                                  _ptr_nonempty(b), _ptr_nonempty(s), total.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _stream()), "han_silhouette")
    return dict(a=a, b=b, s=s, sum=total)


def tsne_calibrate(x, perplexity, tol=1e-5, max_passes=100, check_every=8):
    """scikit-learn's _binary_search_perplexity for TSNE(method="exact") (han_tsne_calibrate): per row of x the beta
    whose conditional distribution has entropy log(perplexity).  All rows bisect together, one pass over all pairs per
    step; the passes run in batches of `check_every` and the count of open rows is read between batches (the one
    synchronisation), until no row is open or max_passes have run.  Returns dict(beta (N,), dmin (N,) -- the smallest
    d2 to another row --, zsum (N,) -- the sum of exp(-beta (d2 - dmin)) --, all fp32; state (3, N) float64 -- the
    bisection's next beta (negative: closed), lower and upper bound --; passes, a 0-d int64 host tensor; open_rows (1,)
    int64 on the device).  Nothing of N x N is stored."""
    ldx = _chk_rows(x, "x")
    n, d = x.shape
    perplexity, tol = float(perplexity), float(tol)
    max_passes, check_every = _chk_int(max_passes, "max_passes", 1), _chk_int(check_every, "check_every", 1)
    if n >= 2 ** 31:
        raise ValueError("x: at most 2^31 - 1 rows")
    if n > 1 and not 1.0 <= perplexity < n:
        raise ValueError(f"perplexity = {perplexity}: expected 1 <= perplexity < {n} rows")
    if not tol >= 0.0:
        raise ValueError(f"tol = {tol}: expected a tolerance >= 0")
    lib, dev = _lib.load(), x.device
    beta, dmin, zsum = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(3))
    state = torch.zeros((3, n), dtype=torch.float64, device=dev)
    open_rows = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _ws(lib.han_tsne_workspace(n, d), dev, "tsne")
    passes = 0
    while n > 1 and passes < max_passes:
        steps = min(check_every, max_passes - passes)
        _lib.check(lib.han_tsne_calibrate(x.data_ptr(), ldx, n, d, perplexity, tol, steps, int(passes == 0), beta.data_ptr(),
                                          dmin.data_ptr(), zsum.data_ptr(), state.data_ptr(), open_rows.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _stream()), "han_tsne_calibrate")
        passes += steps
        if int(open_rows.cpu()[0]) == 0:
            break
    return dict(beta=beta, dmin=dmin, zsum=zsum, state=state, passes=torch.tensor(passes, dtype=torch.int64),
                open_rows=open_rows)


def tsne_step(x, calib, y, update, gains, exaggeration, momentum, lr, min_gain=0.01, want_grad=False, want_kl=False):
    """One iteration of scikit-learn's exact t-SNE in two dimensions (han_tsne_step): the gradient of _kl_divergence
    at y with the joint probabilities formed again per pair from calib (tsne_calibrate's dict), times `exaggeration`,
    then _gradient_descent's update rule IN PLACE on y, update and gains ((N, 2) fp32 each).  Returns dict(stats (3,)
    float64 on the device: Z_q, the squared norm of gains * grad, the KL divergence at the y that came in -- NaN
    without want_kl --; grad (N, 2) fp32, the gradient before the gains, or None without want_grad)."""
    ldx = _chk_rows(x, "x")
    n, d = x.shape
    dev = x.device
    for name in ("beta", "dmin", "zsum"):
        _chk(calib[name], "calib." + name, (n,), device=dev)
    for t, name in ((y, "y"), (update, "update"), (gains, "gains")):
        _chk(t, name, (n, 2), device=dev)
    if n >= 2 ** 31:
        raise ValueError("x: at most 2^31 - 1 rows")
    exaggeration = float(exaggeration)
    if not 0.0 < exaggeration < float("inf"):
        raise ValueError(f"exaggeration = {exaggeration}: expected a positive number")
    lib = _lib.load()
    stats = torch.full((3,), float("nan") if n > 1 else 0.0, dtype=torch.float64, device=dev)      # [2] stays NaN without want_kl
    grad = torch.zeros((n, 2), dtype=torch.float32, device=dev) if want_grad else None
    ws = _ws(lib.han_tsne_workspace(n, d), dev, "tsne")
    _lib.check(lib.han_tsne_step(x.data_ptr() if n else None, ldx, _ptr_nonempty(calib["beta"]), _ptr_nonempty(calib["dmin"]),
                                 _ptr_nonempty(calib["zsum"]), _ptr_nonempty(y), _ptr_nonempty(update), _ptr_nonempty(gains),
                                 _ptr_nonempty(grad), stats.data_ptr(), n, d, exaggeration, float(momentum), float(lr),
                                 float(min_gain), int(bool(want_kl)), ws.data_ptr(), ws.numel(), _stream()), "han_tsne_step")
    return dict(stats=stats, grad=grad)
