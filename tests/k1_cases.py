"""Cases, inputs, float64 references and checks for the K1 projection (han_amd/csrc/project.hip).

Test infrastructure shared by tests/test_project_gpu.py (the checks run against ``han_amd.ops`` on the GPU) and
tests/test_project_cases_cpu.py (the same checks against ``tests.cpu_backend``, plus the dispatch assertions).

Every case declares the forward path it is meant for ("plain": whole-F exact-fp32 kernel, "split": 64-row exact-fp32
kernel + project_finish_kernel, "pipe": a shape on which the bf16 x 6 matrix-pipe kernels may run); forward_path()
reads the path a shape takes from the library's own size queries, so a case that reaches another kernel fails
instead of passing for the wrong reason.

Two kinds of input:

* exact grid -- every tensor holds small integers times a power of two, drawn so that for every output element the
  sum of the absolute values of its terms stays below 2^24 grid units.  Every product and every partial sum, in any
  order, is then an integer below 2^24 and exact in fp32: for the fp32 MFMA kernels, the slab / partial reductions,
  the 4x4x1 block kernel and the bf16 x 6 split alike (a split term never has the opposite sign of its value, so
  the absolute values of the split products add up to |x w|).  The kernels' results must EQUAL the float64
  reference cast to the storage type.  The precondition is asserted here, in float64, from the inputs alone.
* random -- standard normals with rows of very different scale, against the per-element bound
  |got - ref| <= 1.01 * (L + 1) * 2^-24 * S, S the same contraction over absolute values, L the reduction length
  (any fp32 summation order, with or without FMA; L + 7 on the matrix pipe: han_b6.h leaves out three terms of
  under 2^-23 |x w| each; + 2 with the 1/keep factor of a dropout rate that is no power of two).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

from tests import rng_ref

D = 64
HEADS = ((16, 4), (8, 8), (4, 16), (2, 32), (1, 64))
TWO24 = 1 << 24
U = 2.0 ** -24
# han_amd.ops.FLAG_K1_* (restated: this module must import without the library)
FLAG_EXACT_PIPE, FLAG_MATRIX_PIPE, FLAG_4WAVE, FLAG_PAIRS = 2, 4, 16, 32
BIG_OFFSET = 3_000_000_011          # a row offset beyond 2^31: the RNG row key wraps to 32 bits
SEED_DEV = 0x0123456789ABCDEF       # the device seed word of the seed_dev cases
SENTINEL = 777.0

# grid units of the exact-grid tensors (values = integers times these)
GX, GW, GD, GA = 2.0 ** -3, 2.0 ** -5, 2.0 ** -4, 2.0 ** -1
A_MAX, B_MAX = 2, 3                 # |a1|, |a2| <= A_MAX GA; |b1|, |b2| <= B_MAX (GX GW GA)


# --------------------------------------------------------------------------------------------- dispatch
def forward_path(N, F, P=1):
    """The forward path of an (N, F) input with P meta-paths, read from the library's host-side size queries:
    no workspace = "plain" (N < 16384); a workspace that grows with P is the W image of the matrix pipe
    (ceil(F/32) * P * 3*64*64 bytes) = "pipe"; one that does not is the split-F partial tiles (nsplit * N * 64 * 4
    bytes) = "split"."""
    from han_amd import _lib
    lib = _lib.load()
    one = int(lib.han_project_fwd_workspace(N, F, 8, 8))
    assert one == int(lib.han_project_fwd_multi_workspace(N, F, 8, 8, 1))
    ws = int(lib.han_project_fwd_multi_workspace(N, F, 8, 8, P))
    keep = int(lib.han_project_keep_bytes(N, 8, 8, 8, 8))        # a keep table exists for whole-F shapes only
    if one == 0:
        assert ws == 0 and keep == 0 and N < 16384, (N, F, P, ws, keep)
        return "plain"
    two = int(lib.han_project_fwd_multi_workspace(N, F, 8, 8, 2))
    if two == 2 * one:
        img = -(-F // 32) * 3 * 64 * 64
        assert one == img and ws == P * img, (N, F, P, one, ws)
        return "pipe"
    assert two == one == ws and one % (N * D * 4) == 0 and one // (N * D * 4) >= 2 and keep == 0, (N, F, P, one, ws)
    return "split"


# --------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    kind: str               # "fwd" | "multi" | "dw" | "dx"
    n: int
    f: int
    path: str = ""          # forward cases: the declared forward_path()
    K: int = 8
    FP: int = 8
    drop: float = 0.0       # input dropout
    fts: float = 0.0        # projected-row dropout (forward)
    bf16_table: bool = False
    xbf: bool = False       # bf16 features
    flags: int = 0
    view: str = ""          # X layout: "" contiguous | "slice" buf[:, 4:4+F] of F+8 columns (strided, still 16-byte
                            # aligned) | "odd" buf[:, 3:3+F], odd row stride (misaligned) | "off1" buf[:, 1:1+F] of
                            # F+4 columns (pointer off by one element only)
    row_offset: int = 0
    seed_dev: bool = False
    keep_table: bool = False    # forward: ask for the keep table; dW: go through it (N >= 32768 only)
    out_slice: bool = False     # dW: out = buf[1] of (3, F, 64); dX: out = buf[:, 1, :] of (N, 3, F)
    random: bool = False
    P: int = 1

    @property
    def id(self):
        s = f"{self.kind}-{self.n}x{self.f}"
        if self.kind == "multi":
            s += f"-P{self.P}"
        if self.path:
            s += "-" + self.path
        if (self.K, self.FP) != (8, 8):
            s += f"-{self.K}x{self.FP}"
        if self.drop:
            s += f"-drop{self.drop}"
        if self.fts:
            s += f"-fts{self.fts}"
        for flag, name in ((self.bf16_table, "bf16tab"), (self.xbf, "bf16x"), (self.flags, f"flags{self.flags}"),
                           (self.view, self.view), (self.row_offset, "rowoff"), (self.seed_dev, "seeddev"),
                           (self.keep_table, "keep"), (self.out_slice, "out"), (self.random, "random")):
            if flag:
                s += "-" + name
        return s

    @property
    def seed(self):
        return 0x1234ABCD5678 + 131 * self.n + self.f

    @property
    def eff_seed(self):
        return rng_ref.resolve_seed(self.seed, SEED_DEV if self.seed_dev else None)


def _fwd(n, f, path, **kw):
    return Case("fwd", n, f, path, **kw)


def _head_sweep(make, tables=(False, True)):
    return [make(K=K, FP=FP, drop=dr, bf16_table=bt) for K, FP in HEADS for dr in (0.0, 0.5) for bt in tables]


FWD_PLAIN = [
    _fwd(1, 5, "plain"), _fwd(7, 13, "plain"), _fwd(130, 77, "plain"),            # scalar loads
    _fwd(70, 124, "plain"),                                                       # vector loads
    _fwd(130, 77, "plain", random=True),
    _fwd(130, 64, "plain", view="slice"), _fwd(130, 61, "plain", view="odd"),
    _fwd(130, 64, "plain", xbf=True, view="off1"), _fwd(70, 124, "plain", xbf=True),
    _fwd(130, 77, "plain", drop=0.5, fts=0.5), _fwd(130, 77, "plain", drop=0.5, fts=0.5, bf16_table=True),
    _fwd(130, 77, "plain", drop=0.5, fts=0.5, row_offset=BIG_OFFSET),
    _fwd(130, 77, "plain", drop=0.5, fts=0.5, seed_dev=True),
    _fwd(130, 77, "plain", drop=0.6, fts=0.6, random=True),
    _fwd(16383, 64, "plain", flags=FLAG_MATRIX_PIPE),                             # one row short of the matrix pipe
] + _head_sweep(lambda **kw: _fwd(130, 77, "plain", **kw))

FWD_SPLIT = [
    _fwd(7, 128, "split"), _fwd(7, 128, "split", xbf=True),                       # two chunks
    _fwd(130, 300, "split"), _fwd(130, 300, "split", random=True),                # five chunks, a short last one
    _fwd(130, 300, "split", drop=0.6, random=True, bf16_table=True),
    _fwd(700, 129, "split"),                                                      # scalar loads and split
    _fwd(32640, 128, "split"),                                                    # the last split N at F >= 128
    _fwd(130, 300, "split", drop=0.5, fts=0.5), _fwd(130, 300, "split", drop=0.5, fts=0.5, bf16_table=True),
    _fwd(130, 300, "split", drop=0.5, seed_dev=True, row_offset=BIG_OFFSET),
] + _head_sweep(lambda **kw: _fwd(130, 300, "split", **kw))

_MP = FLAG_MATRIX_PIPE
FWD_PIPE = [
    _fwd(16384, 36, "pipe", flags=_MP), _fwd(16384 + 77, 124, "pipe", flags=_MP),
    _fwd(32641, 128, "pipe", flags=_MP),                                          # the first whole-F N at F >= 128
    _fwd(32641, 128, "pipe"),                                                     # ... on the exact-fp32 kernel (MT = 2)
    _fwd(32641 + 77, 136, "pipe", flags=_MP), _fwd(32641 + 77, 136, "pipe", flags=_MP, random=True),
    _fwd(32641 + 77, 264, "pipe", xbf=True), _fwd(32641 + 77, 264, "pipe", xbf=True, random=True),
    _fwd(16384 + 77, 124, "pipe", drop=0.5), _fwd(16384 + 77, 124, "pipe", drop=0.5, xbf=True),   # no keep table
    _fwd(16384 + 77, 124, "pipe", drop=0.5, fts=0.5, bf16_table=True, seed_dev=True, row_offset=BIG_OFFSET),
    _fwd(16384 + 77, 124, "pipe", drop=0.5, flags=FLAG_EXACT_PIPE),               # MT = 2 with dropout
    _fwd(16384 + 77, 124, "pipe", flags=_MP | FLAG_4WAVE),
    _fwd(16384 + 77, 64, "pipe", flags=_MP, view="slice"),
] + [_fwd(n, f, "pipe", drop=0.5, keep_table=True, fts=0.5 if f == 72 else 0.0)
     for n in (32768, 32768 + 77) for f in (8, 72, 136)
] + [_fwd(16384 + 77, 36, "pipe", flags=_MP, K=K, FP=FP, bf16_table=bt) for K, FP in HEADS for bt in (False, True)]


def _multi(P, n, f, **kw):
    return Case("multi", n, f, "pipe", P=P, **kw)


FWD_MULTI = [
    _multi(4, 16384 + 200, 64),                                                   # four per block, fused scores
    _multi(4, 32641 + 7, 256), _multi(4, 32641 + 7, 256, random=True),
    _multi(3, 16384 + 200, 72),                                                   # a pair plus a single
    _multi(6, 16384 + 200, 64),                                                   # four, then two
    _multi(8, 16384 + 200, 36),                                                   # two groups in grid.y
    _multi(5, 16384 + 200, 64, flags=FLAG_PAIRS),
    _multi(2, 16384 + 5, 72, xbf=True, bf16_table=True),
    _multi(4, 16384 + 200, 72, xbf=True),
    _multi(4, 16384 + 200, 64, K=4, FP=16),
]

DW = ([Case("dw", n, f, drop=dr) for n in (1, 31, 32, 33, 3025) for f in (13, 128, 129, 260) for dr in (0.0, 0.5)] + [
    Case("dw", 600, 130, random=True), Case("dw", 600, 130, drop=0.6, random=True),
    Case("dw", 33, 128, xbf=True), Case("dw", 33, 13, xbf=True, drop=0.5),
    Case("dw", 33, 64, view="slice"), Case("dw", 33, 61, view="odd", drop=0.5), Case("dw", 33, 64, xbf=True, view="off1"),
    Case("dw", 33, 77, drop=0.5, seed_dev=True, row_offset=BIG_OFFSET),
    Case("dw", 33, 77, drop=0.5, out_slice=True),
] + [Case("dw", 33, 77, K=K, FP=FP, drop=dr) for K, FP in HEADS for dr in (0.0, 0.5)])

DW_KEEP = [Case("dw", n, f, drop=0.5, keep_table=True, xbf=(f == 264))
           for n in (32768, 32768 + 77) for f in (8, 136, 264)]

DX = ([Case("dx", n, f, drop=dr) for n in (1, 15, 16, 17, 1000) for f in (5, 16, 17, 77) for dr in (0.0, 0.5)] + [
    Case("dx", 300, 77, drop=0.6, random=True), Case("dx", 300, 77, random=True),
    Case("dx", 17, 77, drop=0.5, out_slice=True), Case("dx", 1000, 17, out_slice=True),
    Case("dx", 17, 77, drop=0.5, row_offset=BIG_OFFSET), Case("dx", 17, 77, drop=0.5, seed_dev=True),
] + [Case("dx", 17, 77, K=K, FP=FP, drop=dr) for K, FP in HEADS for dr in (0.0, 0.5)])

FWD_PLAIN, FWD_SPLIT, FWD_PIPE, FWD_MULTI, DW, DW_KEEP, DX = (
    list(dict.fromkeys(v)) for v in (FWD_PLAIN, FWD_SPLIT, FWD_PIPE, FWD_MULTI, DW, DW_KEEP, DX))      # a sweep may repeat a listed case
FWD_ALL = FWD_PLAIN + FWD_SPLIT + FWD_PIPE + FWD_MULTI
ALL = FWD_ALL + DW + DW_KEEP + DX
CPU_MAX_ROWS = 3025       # the cases the CPU stand-ins run


def ids(cases):
    return [c.id for c in cases]


# --------------------------------------------------------------------------------------------- inputs
def _ints(rng, shape, amax):
    return rng.integers(-amax, amax + 1, size=shape).astype(np.float64)


def _odd_ints(rng, shape, lo, hi):
    """odd integers with lo <= |v| <= hi (lo odd): their significand spans from bit 0 to the top bit"""
    m = rng.integers(lo // 2, (hi + 1) // 2, size=shape) * 2 + 1
    return (m * rng.choice([-1, 1], size=shape)).astype(np.float64)


def _scale(c):
    """the exact 1/keep factor of the exact-grid cases (drop is 0 or 0.5)"""
    assert c.drop in (0.0, 0.5) and c.fts in (0.0, 0.5)
    return 2 if c.drop else 1


def _rng(c):
    return np.random.default_rng([c.n, c.f, c.K, c.P, int(c.drop * 10), int(c.random), int(c.xbf)])


def _score_params(rng, c, exact):
    shp = (c.P, c.K, c.FP)
    if exact:
        return (_ints(rng, shp, A_MAX) * GA, _ints(rng, shp, A_MAX) * GA,
                _ints(rng, shp[:2], B_MAX) * (GX * GW * GA), _ints(rng, shp[:2], B_MAX) * (GX * GW * GA))
    return tuple(_as_f32(rng.standard_normal(s)) for s in (shp, shp, shp[:2], shp[:2]))


def _as_f32(a, bf16=False):
    """the float64 values of `a` after storage in fp32 / bf16 (the truth the references start from)"""
    t = torch.tensor(np.asarray(a), dtype=torch.float32)
    if bf16:
        t = t.to(torch.bfloat16)
    return t.to(torch.float64).numpy()


def fwd_inputs(c):
    """x (n, f), W (P, f, 64), a1, a2 (P, K, FP), b1, b2 (P, K): float64 arrays holding exactly the values the
    kernels are given.  Exact-grid cases assert their precondition here."""
    rng = _rng(c)
    n, f, P = c.n, c.f, c.P
    if c.random:
        x = _as_f32(rng.standard_normal((n, f)) * np.exp(rng.standard_normal((n, 1))), c.xbf)
        W = _as_f32(rng.standard_normal((P, f, D)) * 0.2)
        return (x, W) + _score_params(rng, c, False)
    scale = _scale(c)
    # bound on sum_k |x_k w_k| in grid units under which H and the scores are exact: FP A_MAX (scale S) + B_MAX < 2^24,
    # less 1/128 for a bf16 table's rounding of the stored rows
    B = (TWO24 - 1 - B_MAX) // (scale * c.FP * A_MAX)
    B -= B // 128
    if c.path == "pipe":
        # fp32 X: odd integers of 9 .. 12 bits in EVERY element (non-zero mid term of the split); W: small integers
        # and, where the budget allows, one 9-bit entry per column (W's mid term); bf16 X: |x| <= 256
        if c.xbf:
            xb = 256
        else:
            cands = (4095, 2047, 1023, 511)
            xb = next((b for b in cands if B // b >= 511 + 2 * f), None) or next((b for b in cands if B // b >= 2 * f), 511)
        x = _ints(rng, (n, f), 256) if c.xbf else _odd_ints(rng, (n, f), 257, xb)
        room = B // xb
        nbig = 1 if room >= 511 + f else 0
        sw = min(7, (room - 511 * nbig) // f)
        assert sw >= 1, (c.id, B, xb)
        W = _ints(rng, (P, f, D), sw)
        if nbig:
            rows = rng.integers(0, f, size=(P, D))
            for p in range(P):
                W[p, rows[p], np.arange(D)] = _odd_ints(rng, D, 257, 511)
    else:
        xmax = min(math.isqrt(B // f), 256 if c.xbf else 1023)
        wmax = min(B // (f * xmax), 1023)
        assert xmax >= 1 and wmax >= 1, (c.id, B)
        x, W = _ints(rng, (n, f), xmax), _ints(rng, (P, f, D), wmax)
    x, W = x * GX, W * GW
    a1, a2, b1, b2 = _score_params(rng, c, True)
    # the precondition, from the inputs alone (all keep draws taken as "kept")
    assert np.array_equal(x, _as_f32(x, c.xbf)) and np.array_equal(W, _as_f32(W))
    for p in range(P):
        S = scale * (np.abs(x) @ np.abs(W[p])) / (GX * GW)
        assert S.max() < TWO24, (c.id, S.max())
        Sst = S * (1 + 2.0 ** -8) if c.bf16_table else S
        for a, b in ((a1, b1), (a2, b2)):
            sc = (Sst.reshape(n, c.K, c.FP) * np.abs(a[p] / GA)).sum(-1) + np.abs(b[p]) / (GX * GW * GA)
            assert sc.max() < TWO24, (c.id, sc.max())
    return x, W, a1, a2, b1, b2


def _pair_inputs(c, rng, L, shape_a, shape_b, ga, gb, a_bf16=False):
    """two operands whose contraction over L terms is exact (or random): integers up to ~sqrt(2^24 / (scale L))"""
    if c.random:
        a = _as_f32(rng.standard_normal(shape_a) * np.exp(rng.standard_normal((shape_a[0], 1))), a_bf16)
        return a, _as_f32(rng.standard_normal(shape_b) * 0.2)
    B = (TWO24 - 1) // _scale(c)
    amax = min(math.isqrt(B // L), 256 if a_bf16 else 1023)
    bmax = min(B // (L * amax), 1023)
    assert amax >= 1 and bmax >= 1
    return _ints(rng, shape_a, amax) * ga, _ints(rng, shape_b, bmax) * gb


def dw_inputs(c):
    """x (n, f), dH (n, 64)"""
    x, dH = _pair_inputs(c, _rng(c), c.n, (c.n, c.f), (c.n, D), GX, GD, c.xbf)
    if not c.random:
        S = _scale(c) * (np.abs(x).T @ np.abs(dH)) / (GX * GD)
        assert S.max() < TWO24, (c.id, S.max())
        assert np.array_equal(x, _as_f32(x, c.xbf))
    return x, dH


def dx_inputs(c):
    """dH (n, 64), W (f, 64)"""
    dH, W = _pair_inputs(c, _rng(c), D, (c.n, D), (c.f, D), GD, GW)
    if not c.random:
        S = _scale(c) * (np.abs(dH) @ np.abs(W).T) / (GD * GW)
        assert S.max() < TWO24, (c.id, S.max())
    return dH, W


def make_inputs(c):
    return {"fwd": fwd_inputs, "multi": fwd_inputs, "dw": dw_inputs, "dx": dx_inputs}[c.kind](c)


# --------------------------------------------------------------------------------------------- float64 references
def seq_masks(seed, r0, r1, f, K, drop, row_offset=0):
    """rng_ref.seq_mask for the rows [r0, r1): (K, r1 - r0, f) bool.  One hash per (row, feature, four heads), as
    the kernels draw it (rng_ref.seq_mask hashes once per head)."""
    KQ = (K + 3) // 4
    rows = (np.arange(r0, r1, dtype=np.int64) + int(row_offset))[:, None]
    fs = np.arange(f, dtype=np.int64)[None, :]
    thr = rng_ref._thr(drop)
    out = np.empty((K, r1 - r0, f), dtype=bool)
    for q in range(KQ):
        xw, yw = rng_ref.han_rand64(seed, rng_ref.STREAM_SEQ, rows, fs * KQ + q)
        for k in range(4 * q, min(K, 4 * q + 4)):
            out[k] = rng_ref.field(xw, yw, k % 4) < thr
    return out


def _row_blocks(n, f):
    step = max(1, (1 << 20) // max(1, f))       # ~1M draws per block: a 32768-row case stays within megabytes
    return [(r0, min(n, r0 + step)) for r0 in range(0, n, step)]


def _inv_keep(drop):
    return 1.0 / rng_ref.keep_prob32(drop) if drop > 0 else 1.0


def fwd_reference(x, W, K, FP, drop, seed, row_offset):
    """H = per-head masked product x~ W_k (float64) and S, the same contraction over absolute values"""
    if drop == 0:
        return x @ W, np.abs(x) @ np.abs(W)
    n, f = x.shape
    H, S, aW = np.empty((n, D)), np.empty((n, D)), np.abs(W)
    for r0, r1 in _row_blocks(n, f):
        m = seq_masks(seed, r0, r1, f, K, drop, row_offset)
        for k in range(K):
            cs = slice(k * FP, (k + 1) * FP)
            xm = x[r0:r1] * m[k]
            H[r0:r1, cs] = xm @ W[:, cs]
            S[r0:r1, cs] = np.abs(xm) @ aW[:, cs]
    return H * _inv_keep(drop), S * _inv_keep(drop)


def dw_reference(x, dH, K, FP, drop, seed, row_offset):
    """dW = x~^T dH per head, and S"""
    if drop == 0:
        return x.T @ dH, np.abs(x).T @ np.abs(dH)
    n, f = x.shape
    dW, S, aD = np.zeros((f, D)), np.zeros((f, D)), np.abs(dH)
    for r0, r1 in _row_blocks(n, f):
        m = seq_masks(seed, r0, r1, f, K, drop, row_offset)
        for k in range(K):
            cs = slice(k * FP, (k + 1) * FP)
            xm = x[r0:r1] * m[k]
            dW[:, cs] += xm.T @ dH[r0:r1, cs]
            S[:, cs] += np.abs(xm).T @ aD[r0:r1, cs]
    return dW * _inv_keep(drop), S * _inv_keep(drop)


def dx_reference(dH, W, K, FP, drop, seed, row_offset):
    """dX = sum_k m_k / keep * dH_k W_k^T, and S"""
    if drop == 0:
        return dH @ W.T, np.abs(dH) @ np.abs(W).T
    n, f = dH.shape[0], W.shape[0]
    dX, S = np.zeros((n, f)), np.zeros((n, f))
    for r0, r1 in _row_blocks(n, f):
        m = seq_masks(seed, r0, r1, f, K, drop, row_offset)
        for k in range(K):
            cs = slice(k * FP, (k + 1) * FP)
            dX[r0:r1] += m[k] * (dH[r0:r1, cs] @ W[:, cs].T)
            S[r0:r1] += m[k] * (np.abs(dH[r0:r1, cs]) @ np.abs(W[:, cs]).T)
    return dX * _inv_keep(drop), S * _inv_keep(drop)


def bound(L, S, c, pipe=False):
    """the random-input bound; c.drop adds the two roundings of the 1/keep factor"""
    return 1.01 * (L + (7 if pipe else 1) + (2 if c.drop else 0)) * U * S


# --------------------------------------------------------------------------------------------- tensors
def _t(a, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(dtype).to(dev)


def x_tensor(x, dev, c):
    """the (n, f) feature tensor in the layout the case asks for; the rest of a wider buffer holds a sentinel"""
    dt = torch.bfloat16 if c.xbf else torch.float32
    xt = _t(x, dev, dt)
    if not c.view:
        return xt
    n, f = xt.shape
    lead, width = {"slice": (4, f + 8), "odd": (3, f + 6 + (f % 2 == 0)), "off1": (1, f + 4)}[c.view]
    buf = torch.full((n, width), SENTINEL, dtype=dt, device=dev)
    buf[:, lead:lead + f] = xt
    v = buf[:, lead:lead + f]
    assert v.stride(1) == 1 and (n == 1 or v.stride(0) == width)
    return v


def _seed_dev(dev, c):
    return torch.tensor([SEED_DEV], dtype=torch.int64, device=dev) if c.seed_dev else None


def _f64(t):
    return t.detach().to("cpu").to(torch.float64).numpy()


def _int_view(t):
    return t.cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _on_pipe(c, dev):
    """whether the matrix-pipe kernel is what runs this forward case (project.hip: han_project_fwd)"""
    if c.path != "pipe" or (c.flags & FLAG_EXACT_PIPE) or (c.drop > 0 and (c.K, c.FP) != (8, 8)):
        return False
    return bool(c.drop > 0 or c.xbf or (c.flags & FLAG_MATRIX_PIPE) or c.kind == "multi")


# --------------------------------------------------------------------------------------------- checks
def _check_rows(c, dev, H, f1, f2, x, W, a1, a2, b1, b2, tag=""):
    """one meta-path's H (n, 64), f1, f2 (n, K) against the float64 reference"""
    n, K, FP = c.n, c.K, c.FP
    tdt = torch.bfloat16 if c.bf16_table else torch.float32
    assert H.shape == (n, D) and H.dtype == tdt and f1.shape == (n, K) and f2.shape == (n, K), tag
    ref, S = fwd_reference(x, W, K, FP, c.drop, c.eff_seed, c.row_offset)
    bits = None
    if c.fts > 0:
        bits = torch.tensor(rng_ref.fts_mask(c.eff_seed, n, D, c.fts, c.row_offset).astype(np.int64))
        got_bits = (_int_view(H) & 1).to(torch.int64)
        assert torch.equal(got_bits, bits), (tag, "keep bits of the projected-row dropout")
    Hc = H.cpu()
    if not c.random:
        want = torch.tensor(ref, dtype=torch.float64).to(torch.float32).to(tdt)      # exact in fp32; bf16: nearest even
        if bits is None:
            bad = (Hc != want)
        else:       # the stamped bit aside
            it = _int_view(Hc).dtype
            bad = ((_int_view(Hc) & ~1).view(tdt) != (_int_view(want) & ~1).view(tdt))
            want = ((_int_view(want) & ~1) | bits.to(it)).view(tdt)                  # the rows as stored
        assert not bad.any(), (tag, "H", int(bad.sum()), bad.nonzero()[:4].tolist(),
                               Hc[bad][:4].tolist(), want[bad][:4].tolist())
        stored = want.to(torch.float64).numpy()
    else:
        b = bound(c.f, S, c, _on_pipe(c, dev))
        tol = b + (2.0 ** -8 * (np.abs(ref) + b) if c.bf16_table else 0.0)      # bf16: 8 significand bits
        if bits is not None:       # the stamped bit moves the stored value by at most one unit in its last place
            tol = tol + (np.abs(ref) + tol) * (2.0 ** -7 if c.bf16_table else 2.0 ** -23)
        err = np.abs(_f64(Hc) - ref)
        assert (err <= tol).all(), (tag, "H", float((err / np.maximum(tol, 1e-300)).max()))
        stored = _f64(Hc)
    st = stored.reshape(n, K, FP)
    for name, got, a, bb in (("f1", f1, a1, b1), ("f2", f2, a2, b2)):
        fref = (st * a[None]).sum(-1) + bb
        if not c.random and c.fts == 0:
            assert torch.equal(got.cpu(), torch.tensor(fref).to(torch.float32)), (tag, name)
        else:
            Sf = (np.abs(st) * np.abs(a)[None]).sum(-1) + np.abs(bb)
            err = np.abs(_f64(got) - fref)
            assert (err <= 1.01 * (FP + 1) * U * Sf).all(), (tag, name, float((err / Sf).max() / U))


def check_fwd(ops, dev, c):
    """project_fwd (c.P == 1, kind "fwd") against the float64 reference"""
    x, W, a1, a2, b1, b2 = make_inputs(c)
    xt = x_tensor(x, dev, c)
    tdt = torch.bfloat16 if c.bf16_table else torch.float32
    args = (xt, _t(W[0], dev), _t(a1[0], dev), _t(a2[0], dev), _t(b1[0], dev), _t(b2[0], dev))
    out = ops.project_fwd(*args, in_drop=c.drop, fts_drop=c.fts, seed=c.seed, row_offset=c.row_offset,
                          table_dtype=tdt, seed_dev=_seed_dev(dev, c), flags=c.flags, want_keep=c.keep_table)
    if c.keep_table:
        assert len(out) == 4
        if dev.type != "cpu":
            assert out[3] is not None and out[3].numel() == c.n * c.f + 128
    _check_rows(c, dev, out[0], out[1], out[2], x, W[0], a1[0], a2[0], b1[0], b2[0])


def check_fwd_multi(ops, dev, c):
    """project_fwd_multi against the float64 reference, and, for the meta-paths the fused kernel ran, bit for bit
    against the single-path matrix-pipe kernel"""
    x, W, a1, a2, b1, b2 = make_inputs(c)
    xt = x_tensor(x, dev, c)
    tdt = torch.bfloat16 if c.bf16_table else torch.float32
    Wt, a1t, a2t, b1t, b2t = (_t(v, dev) for v in (W, a1, a2, b1, b2))
    H, f1, f2 = ops.project_fwd_multi(xt, Wt, a1t, a2t, b1t, b2t, table_dtype=tdt, flags=c.flags)
    assert H.shape == (c.P, c.n, D) and f1.shape == (c.P, c.n, c.K)
    for p in range(c.P):
        _check_rows(c, dev, H[p], f1[p], f2[p], x, W[p], a1[p], a2[p], b1[p], b2[p], tag=f"p={p}")
        if p < c.P - c.P % 2:       # the same products in the same order (an odd last meta-path is not fused)
            Hs, g1, g2 = ops.project_fwd(xt, Wt[p], a1t[p], a2t[p], b1t[p], b2t[p], table_dtype=tdt,
                                         flags=FLAG_MATRIX_PIPE)
            assert torch.equal(H[p], Hs), p
            if c.FP != 8:           # both took the scores from those rows with project_scores_kernel
                assert torch.equal(f1[p], g1) and torch.equal(f2[p], g2), p


def _check_matrix(c, got, ref, S, L, name):
    if not c.random:
        want = torch.tensor(ref, dtype=torch.float64).to(torch.float32)
        bad = got.cpu() != want
        assert not bad.any(), (name, int(bad.sum()), bad.nonzero()[:4].tolist(), got.cpu()[bad][:4].tolist(),
                               want[bad][:4].tolist())
    else:
        err = np.abs(_f64(got) - ref)
        tol = bound(L, S, c)
        assert (err <= tol).all(), (name, float((err / np.maximum(tol, 1e-300)).max()))


def check_dw(ops, dev, c):
    """project_bwd against x~^T dH in float64; c.keep_table: through the forward's keep table (the 4x4x1 block
    kernel) and through the hash-regenerating kernel"""
    x, dH = make_inputs(c)
    xt, dHt = x_tensor(x, dev, c), _t(dH, dev)
    ref, S = dw_reference(x, dH, c.K, c.FP, c.drop, c.eff_seed, c.row_offset)
    kw = dict(in_drop=c.drop, seed=c.seed, row_offset=c.row_offset, seed_dev=_seed_dev(dev, c))
    if c.out_slice:
        buf = torch.full((3, c.f, D), SENTINEL, dtype=torch.float32, device=dev)
        dW = ops.project_bwd(xt, dHt, c.K, c.FP, out=buf[1], **kw)
        assert dW.data_ptr() == buf[1].data_ptr()
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[2] == SENTINEL).all())
    else:
        dW = ops.project_bwd(xt, dHt, c.K, c.FP, **kw)
    assert dW.shape == (c.f, D)
    _check_matrix(c, dW, ref, S, c.n, "dW")
    if c.keep_table:
        rng = np.random.default_rng(c.f)
        W = _t(_ints(rng, (c.f, D), 1), dev)
        a, b = _t(_ints(rng, (8, 8), 1), dev), _t(_ints(rng, (8,), 1), dev)
        keep = ops.project_fwd(xt, W, a, a, b, b, want_keep=True, **kw)[3]
        assert keep is not None and keep.numel() == c.n * c.f + 128
        dWk = ops.project_bwd(xt, dHt, c.K, c.FP, keep=keep, **kw)
        _check_matrix(c, dWk, ref, S, c.n, "dW through the keep table")
        assert torch.equal(dWk, dW)


def check_dx(ops, dev, c):
    """project_bwd_input against sum_k m_k / keep * dH_k W_k^T in float64"""
    dH, W = make_inputs(c)
    ref, S = dx_reference(dH, W, c.K, c.FP, c.drop, c.eff_seed, c.row_offset)
    kw = dict(in_drop=c.drop, seed=c.seed, row_offset=c.row_offset, seed_dev=_seed_dev(dev, c))
    if c.out_slice:
        buf = torch.full((c.n, 3, c.f), SENTINEL, dtype=torch.float32, device=dev)
        dX = ops.project_bwd_input(_t(dH, dev), _t(W, dev), c.K, c.FP, out=buf[:, 1, :], **kw)
        assert dX.data_ptr() == buf[:, 1, :].data_ptr()
        assert bool((buf[:, 0, :] == SENTINEL).all()) and bool((buf[:, 2, :] == SENTINEL).all())
    else:
        dX = ops.project_bwd_input(_t(dH, dev), _t(W, dev), c.K, c.FP, **kw)
    assert dX.shape == (c.n, c.f)
    _check_matrix(c, dX, ref, S, c.FP, "dX")


CHECKS = {"fwd": check_fwd, "multi": check_fwd_multi, "dw": check_dw, "dx": check_dx}


def check(ops, dev, c):
    CHECKS[c.kind](ops, dev, c)
