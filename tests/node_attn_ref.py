"""float64 reference of the K2 node attention (han_amd/csrc/node_attn.hip; utils/layers.py:26-35,46) and of its two
backward halves, with a running fp32 error bound, the mirror of the host dispatch (CELLS) and the seeded inputs the host
and the GPU tests share (test infrastructure, NumPy only).

Every function takes the fp32 (or widened bf16) values the kernel sees and promotes them to float64 (`up`); the scalars
of the C ABI (slope, 1 / keep) are `float` there and are formed in np.float32 first.  Next to each result `x` stands an
elementwise bound `e_x` on |fp32 kernel - float64|, built from u = 2^-24 (`U`) and counts of roundings read from the
kernel source (line numbers: node_attn.hip); nothing here is a measurement, and the intrinsic terms are those of
tests/loss_opt_ref.py and tests/sem_attn_ref.py:  __expf(t) (2 + 2|t|) u relative, the subtraction in front of it
|t| u in the exponent, __logf 4u max(1, |log|), an IEEE division 5u (2.5 ulp), a result below the smallest normal may be
flushed: TINY absolute.

Forward (consume_edges :243-324, write_row :327-356), row i, head k, entry (j, w):
f2      recomputed from the gathered row (:269): dot4, a product and three additions in the lane (4 roundings), the
        log2(F' / 4) butterfly levels of head_sum (:36-45) -- HS = 4 + log2(F' / 4) on the longest path -- and the bias:
                                                       e_f2 = (HS + 1) u (|Hs| . |a2| + |b2|)     (0 where f2 is given)
x, e    x = (f1 + f2) w: an addition and a product; e = fmaxf(x, slope x): one product
                                                       e_x = |w| e_f2 + 2u |x|        e_e = e_x + u |e|
        sg = (x > 0 ? 1 : slope) w is discontinuous: an entry with |x| <= e_x is UNDECIDED and adds p (1 - slope) |w|
        to the bounds of tsum and aggp (its share of the sum) instead of being skipped.
p, l    online softmax.  A term enters as __expf(e - mc) and is then multiplied by one factor __expf(m_old - m_new) per
        later step of its lane group (:276-283) and per fold (RowState::merge :182-196, the finish kernel's fold
        :918-930).  The exponents telescope to t = e - m <= 0: (2 + 3|t|) u for all factors together plus, per factor, its
        ulp (2u) and the product (u); per entry the lane adds, one rounding (:288, :315).  The longest path of a row:
            a 16-lane group per row  (RPW = 4, :470-488)    P = n + 3 ceil(n / 4)          n entries, 4 per step
            a wave per row           (RPW = 1, :397-457)    P = ceil(n / 4) + 3 S(n) + 2 FOLD
                S(n) = steps of 16 edges per 64-entry piece + single steps of 4 for its tail (:418-454; the masked
                steps of the fp32 eval kernel :403-416 and the 8-step unroll of HAN_FLAG_K2_DEEP are fewer)
            chunks                   (:842-963)             P = P_wave(chunk) + FOLD (ceil(chunks / 16) + 16)
        FOLD = 6: two __expf (2u each), a product and an addition.  Both scores of an exponent move (E = e_e + the
        largest e_e of the row, as in loss_opt_ref):
                                                       rho = expm1(E + (P + 3|t|) u)
        the relative error of l, a sum of positive terms, is the weighted mean  rden = sum w rho  (w = p / l), and the
        normalised weight carries  r = (1 + rho)(1 + C_FIN u) / (1 - rden) - 1  with C_FIN = 8: 1 / l (5u), the two
        1 / keep factors and the product with the accumulator (write_row :331-339):
                                                       e_w = w r + TINY
agg     sum w am Hd (am in {0, 1}, Hd the kept stored elements; both 1 / keep factors, fp32 scalars, applied once):
                                                       e_agg = ikc ikf sum e_w |am Hd|
out     pre = agg + c + res: two additions;  ELU(x <= 0) = __expf(x) - 1:
                 e_pre = e_agg + 2u (|agg| + |c| + |res|)      e_out = e_pre + [(2 + 2|pre|) u e^pre + u |out|]  (pre <= e_pre)
lse     m + __logf(l):  -log1p(-rden) + 4u max(1, |log l|) + u (|m| + |log l| + |lse|);   -1e30 exactly for an empty row
tsum    sum w sg:      sum (e_w |sg| + [undecided] w (1 - slope)|w_ij|)
aggp    the same weights times |am Hd|
coefs   node_attn_coef_kernel (:1738-1798): a lane takes every 64th entry (two __expf, a product and an addition per
        entry: 6) and six butterfly folds: P = 6 ceil(n / 64) + 6 FOLD, the same r.

Row-local backward (node_attn_bwd_rows_kernel :982-1052), from the GIVEN out, dOut, aggp, tsum, f1, lse:
g       da = out + 1 (u), g = dOut da (u): e_g = 2u |g|; a bf16 table stores RN_bf16(g): the stored value must lie in
        [RN(g - e_g), RN(g + e_g)].  s, df1 and z are then formed from the STORED g (the kernel's own), not from the
        reference's: no error is charged twice.
pre     __logf(da): u (from da) + 4u max(1, |log da|);  an output that rounded to -1 has g = 0 and adds an exact zero.
s       F' terms g (pre - c - res): two subtractions, a product, the lane's chain of four and head_sum (HS):
                 e_s = sum |g| (e_pt + 2u (|pre| + |c| + |res|)) + (HS + 1) u sum |g (pre - c - res)|
df1     dp - s tsum:   (HS + 1) u sum |g aggp| + |tsum| e_s + 2u (|dp| + |s tsum|)
dc      sum_i g (unrounded): the lane's chain over its rows, the block's 16 groups, han_reduce_slabs (depth_rows)

Transposed-graph backward (bwd_consume :1122-1179, bwd_consume_pred :1200-1260, write_src :1262-1273), source j:
alpha   x = (st.f1 + f2) w, e = lrelu(x), t = e - st.lse: rho_a = expm1(2u |x| + u |e| + (2 + 3|t|) u); the sign of x
        is decided exactly (a rounded sum and product keep their sign), so sg carries no doubt here.
dot     F' products g hd (dot4 and head_sum: HS), hd = H mk one product more:      (HS + 2) u sum |g hd|
df2     term = alpha sg (am dot - s): am dot, the subtraction, alpha sg, the product (4u); the sum over the row:
        P_sum = n (group per row), ceil(n / 4) + 2 (wave per row, :1387-1393), per chunk the same plus
        ceil(chunks / 16) + 16 in the finish kernel (:1622-1668)
acc     alpha am g: two products;  dH = acc mk + df1 a1 + df2 a2: three roundings per term.
An alpha below TINY is flushed: such entries carry TINY absolute, like every weight.

Score gradients (score_param_bwd_kernel :1674-1714 and the SCORE forms :1395-1431): depth x u x sum |terms| with the
depth of tests/test_bwd_cols_scores_gpu._depth (score_depth / depth_rows here).

Lean kernels (HAN_FLAG_LEAN: fp32 table of at most 16 384 rows, mean degree >= 64, scores read from the table;
lean_fwd_step :535-603, node_attn_fwd_lean_kernel :607-680, node_attn_fwd_h8_kernel :688-839).  The softmax runs in log2
units: f1 log2e (the constant and a product: 2u |f1|), one fused multiply-add with f2 (the constant: u |f2|, the
rounding: u |x|), the edge value (u |x|):              e_x = |w| (2 |f1| + |f2|) u + 2u |x|
exp2 is v_exp_f32 itself (2u), its argument t log2e.  Steps of 16 edges: a 16-lane group adds 4 of them, an 8-lane group
of the one-lane-per-head kernel 2; two (three) folds.  P_wave(n) + FOLD covers both.  The folds of the 16-lane kernel
convert m back (m ln2: 2u |m|) and use __expf; lse = m ln2 + __logf(l): E and e_lse carry 4u |m| and 2u |m| more.
Lean backward (node_attn_bwd_cols_h8_kernel :1443-1568; the DEDUP gather is bwd_consume on whole rows): the arithmetic of
the gather; dot is an in-lane chain of 8 at 8 x 8 (9 with hd = H mk); P_sum = ceil(n / 4) + 3.

Dense form (node_attn_dense.h; 8 x 8, binary, fp32, density >= 0.65): a FIXED shift per row, m_i = lrelu(xF), xF = f1_i + F,
F = max_j f2_j, and p = max(A_i B_j, C_i D_j) with A = e^(xF - m), C = e^(slope xF - m), B = e^y, D = e^(slope y),
y = f2_j - F (:176-187, :239-240, :270-273).  Exponent errors: xF (u |xF|, in both A and C), m (u |m|), the two
subtractions, slope xF and slope y, y itself; four __expf (2 + 2|t|) u, a product:
                 rho = expm1((2|xF| + |m| + 3|xF - m| + 3|slope xF - m| + 4|y| + 5 + P) u)
The sums run over EVERY table column (a masked p is +0): l in a lane over 8 columns per 32-column tile, the products on
v_mfma_f32_16x16x4_f32 counted as one rounding per k index (32 per tile, as sem_attn_ref counts that pipe), the S segments
in the finish kernel (:139-151): P = 32 tiles + S + 2 for all of them.  lse = m_i + __logf(l): the bound of lse with m_i
and log l = lse - m_i (down to -80) in the place of the running maximum.  The sign of x = f1 + f2 is taken from x itself
(:281): decided.  The backward (:372-531): alpha = max(A'_i B_j, C'_i D_j), A' = e^(xF - lse_i): the same rho with lse_i for
m; dot on the matrix pipe (8 k indices) with hd = H mk: 9u sum |g hd|; t = wv dot - al s with wv = al / keep: four
roundings and the slope, relative to |wv dot| + |al s|; the same P.  When a head's scores range over more than 80 the
device falls back to the lean CSR kernels (dense_range :96-117): the lean bounds.

CELLS lists the kernel instances the host dispatch (launch_fwd_rows :1880-1915, launch_fwd_v, launch_fwd_lean_v,
launch_bwd_rows :1983-2007, launch_bwd_cols_v, dense_front, the entry points) reaches from han_amd.ops, by template
arguments (dense_f2_range_kernel and csr_to_bitmask_kernel run in front of every dense call and have no output of their
own to compare).  tests/test_node_attn_ref_host.py checks reference, bounds and this mirror without a GPU.
"""
import functools
import types

import numpy as np

from tests import rng_ref
from tests.loss_opt_ref import TINY, U, ratio, up  # noqa: F401  (re-exported for the tests)

D = 64
HEADS = ((16, 4), (8, 8), (4, 16), (2, 32), (1, 64))            # (K, F')
SLOPE = float(np.float32(0.2))                                  # han_amd.ops.LEAKY_SLOPE as the C ABI's float
NEG_BIG = float(np.float32(-1.0e30))                            # HAN_NEG_BIG
GS_Z_ALL_ZERO = 0x3F800000
ACT_IDENTITY, ACT_ELU = 0, 1
FOLD = 6


def hs(FP):
    """Roundings on the longest path of dot4 / the lane's chain of four followed by head_sum<FP>."""
    return 4 + {4: 0, 8: 1, 16: 2, 32: 3, 64: 4}[FP]


C_FIN = 8
SEED_DEV = 0x0123456789ABCDEF

# ------------------------------------------------------------------------------------------------ dispatch mirror
SHORT_DEG, SPLIT_DEG, SPLIT_CHUNK = 16, 1024, 512               # han_amd.ops.SHORT_DEG / SPLIT_DEG / SPLIT_CHUNK
LOW_DEGREE = 12.0                                               # kLowDegree
GRID_CAP = 8192                                                 # attn_grid: 256 * 8 * 4 blocks of 4 waves
REDUCE_BLOCKS = 1024                                            # kReduceBlocks
SHORT, WAVE, CHUNK = 0, 1, 2


def attn_grid(units):
    return min(max(-(-int(units) // 4), 1), GRID_CAP)


def row_forms(deg, binned=True, split_deg=SPLIT_DEG, empty_mid=False):
    """Per row the launch that computes it: SHORT (a 16-lane group), WAVE or CHUNK (for_each_bin, CSRGraph.row_bins)."""
    deg = np.asarray(deg, dtype=np.int64)
    if binned:
        short = (deg < SHORT_DEG) & ((deg > 0) | (not empty_mid))
    else:
        short = np.full(deg.shape, bool(deg.sum() < LOW_DEGREE * len(deg)))
    return np.where(deg > split_deg, CHUNK, np.where(short, SHORT, WAVE))


def grid_passes(deg, binned=True, split_deg=SPLIT_DEG, chunk=SPLIT_CHUNK):
    """{launch: (work units, grid, passes of the grid-stride loop)} of a forward / transposed-graph launch."""
    f = row_forms(deg, binned, split_deg)
    out = {}
    for form, name, per in ((SHORT, "short", 4), (WAVE, "wave", 1)):
        n = int((f == form).sum())
        if n:
            units = -(-n // per)
            out[name] = (units, attn_grid(units), -(-units // (4 * attn_grid(units))))
    nch = int(sum(-(-int(d) // chunk) for d in np.asarray(deg)[f == CHUNK]))
    if nch:
        out["chunk"] = (nch, attn_grid(nch), -(-nch // (4 * attn_grid(nch))))
    return out


def _ceil(a, b):
    return -(-a // b)


def _steps_wave(n):
    rem = n % 64
    return (n // 64) * 4 + rem // 16 + _ceil(rem % 16, 4)


def _p_wave(n):
    return _ceil(n, 4) + 3 * _steps_wave(n) + 2 * FOLD


def fwd_path(deg, forms, chunk=SPLIT_CHUNK):
    """P of the module docstring, per row."""
    n = np.asarray(deg, dtype=np.int64)
    nc = _ceil(n, chunk)
    return np.where(forms == SHORT, n + 3 * _ceil(n, 4),
                    np.where(forms == WAVE, _p_wave(n), _p_wave(np.minimum(n, chunk)) + FOLD * (_ceil(nc, 16) + 16)))


def coef_path(deg):
    return 6 * _ceil(np.asarray(deg, dtype=np.int64), 64) + 6 * FOLD


def bwd_path(deg, forms, chunk=SPLIT_CHUNK):
    """P_sum of the module docstring, per source row."""
    n = np.asarray(deg, dtype=np.int64)
    nc = _ceil(n, chunk)
    return np.where(forms == SHORT, n, np.where(forms == WAVE, _ceil(n, 4) + 2,
                                                _ceil(np.minimum(n, chunk), 4) + 2 + _ceil(nc, 16) + 16))


def _reduce_slabs_depth(rows):
    return _ceil(rows, 64) + 1 + 2 + 16            # han_reduce_slabs: an accumulator's chain, four accumulators, 16 slices


def depth_rows(N):
    """bwd_rows' dc and score_param_bwd: the product, a lane group's chain over its rows, 16 groups, the slab."""
    grid = min(max(_ceil(N, 16), 1), REDUCE_BLOCKS)
    return 1 + _ceil(N, 16 * grid) + 16 + _reduce_slabs_depth(grid)


def score_depth(launches):
    """han_node_attn_bwd_cols_scores; launches = [(rows of the launch, rows per wave)] (test_bwd_cols_scores_gpu._depth)."""
    slab_rows = lane = 0
    for n_work, rpw in launches:
        units = _ceil(n_work, rpw)
        grid = attn_grid(units)
        lane = max(lane, _ceil(units, 4 * grid))
        slab_rows += grid
    d = 1 + lane + 16
    if slab_rows > REDUCE_BLOCKS:
        d += _ceil(slab_rows, 256)
        slab_rows = 256
    return d + _reduce_slabs_depth(slab_rows)


def _b(x):
    return int(bool(x))


def fwd_cells(K, FP, bf16, val, train, coef_drop, fts_drop, gid=False, f2_src=False, shared_hash=False, deep=False,
              forms=(SHORT, WAVE, CHUNK)):
    """Names of the kernel instances one node_attn_fwd call launches (launch_fwd_rows, launch_fwd_v)."""
    fast = bool(train and coef_drop > 0 and fts_drop > 0 and not gid and not f2_src)
    bf, v, t = _b(bf16), _b(val), _b(train)
    out = []
    if SHORT in forms:
        out.append(f"fwd<FP={FP},TRAIN={t},RPW=4,U=4,BF={bf},VAL={v},FAST={_b(fast)},SPLIT=0>")
    if WAVE in forms:
        if FP == 8 and not val and train and fast and shared_hash:
            out.append(f"fwd<FP=8,TRAIN=1,RPW=1,U=4,BF={bf},VAL=0,FAST=1,SPLIT=1,DD=1>")
        elif train:
            out.append(f"fwd<FP={FP},TRAIN=1,RPW=1,U=4,BF={bf},VAL={v},FAST={_b(fast)},SPLIT=1>")
        elif bf16 and deep:
            out.append(f"fwd<FP={FP},TRAIN=0,RPW=1,U=8,BF=1,VAL={v},FAST=0,SPLIT=1>")
        else:
            out.append(f"fwd<FP={FP},TRAIN=0,RPW=1,U=4,BF={bf},VAL={v},FAST=0,SPLIT={bf}>")
    if CHUNK in forms:
        out += [f"fwd_chunk<FP={FP},TRAIN={t},U=4,BF={bf},VAL={v}>", f"fwd_finish<FP={FP},TRAIN={t}>"]
    return out


def bwd_mode(bf16, coef_drop, gid, masked, full_gather=False, zero_rows=False):
    if bf16 or coef_drop == 0 or gid or masked:
        return 0
    return 2 if full_gather else (3 if zero_rows else 1)


def bwd_cells(K, FP, bf16, val, coef_drop, gid=False, masked=False, full_gather=False, zero_rows=False, score=False,
              forms=(SHORT, WAVE, CHUNK)):
    """Names of the kernel instances one node_attn_bwd_cols(_scores) call launches (launch_bwd_rows, launch_bwd_cols_v)."""
    mode = bwd_mode(bf16, coef_drop, gid, masked, full_gather, zero_rows)
    fast = bool(coef_drop > 0 and not gid)
    bf, v = _b(bf16), _b(val)
    out = []
    for form, rpw in ((SHORT, 4), (WAVE, 1)):
        if form not in forms:
            continue
        if masked and not score:
            out.append(f"bwd_cols<FP={FP},RPW={rpw},U=4,BF={bf},VAL={v},FAST=0,MASKED=1,MODE=0>")
        else:
            f = _b(fast) if mode == 0 else 1
            out.append(f"bwd_cols<FP={FP},RPW={rpw},U=4,BF={bf},VAL={v},FAST={f},MASKED=0,MODE={mode + (4 if score else 0)}>")
    if CHUNK in forms and not score:
        out += [f"bwd_chunk<FP={FP},U=4,BF={bf if mode == 0 else 0},VAL={v},MODE={mode}>", f"bwd_finish<FP={FP},BF={bf}>"]
    return out


def lean_fwd_cells(K, FP, val, train):
    return [f"fwd_h8<TRAIN={_b(train)},VAL={_b(val)}>" if FP == 8 else f"fwd_lean<FP={FP},TRAIN={_b(train)},VAL={_b(val)}>"]


def lean_bwd_cells(K, FP, val, gid=False):
    if FP == 8 and not gid:
        return [f"bwd_h8<VAL={_b(val)}>"]
    return [f"bwd_cols<FP={FP},RPW=1,U=4,BF=0,VAL={_b(val)},FAST=0,MASKED=0,DEDUP=1>"]


DENSE_CELLS = ["fwd_dense<TRAIN=0>", "fwd_dense_finish<TRAIN=0>", "fwd_dense<TRAIN=1>", "fwd_dense_finish<TRAIN=1>",
               "bwd_dense", "bwd_dense_finish"]
DENSE_MAX_RANGE = 80.0                                          # kDenseMaxRange


def dense_split(rows, nt):
    """(tiles, S): 32-column tiles of the table and the segments a dense launch cuts them into (dense_split)."""
    bx = _ceil(rows, 64)
    t = _ceil(nt, 32)
    want = min(max(_ceil(1024, max(bx, 1)), 1), max(t, 1))
    tps = max(_ceil(t, want), 1)
    return t, max(_ceil(t, tps), 1)


def dense_applies(f2):
    """The device-side verdict of dense_range: every head's scores within DENSE_MAX_RANGE (fp32 subtraction)."""
    f2 = np.asarray(f2, dtype=np.float32)
    return bool(((f2.max(0) - f2.min(0)) <= np.float32(DENSE_MAX_RANGE)).all())


def _all_cells():
    cells = list(DENSE_CELLS)
    for K, FP in HEADS:
        for val in (False, True):
            cells += lean_fwd_cells(K, FP, val, False) + lean_fwd_cells(K, FP, val, True)
            cells += lean_bwd_cells(K, FP, val) + lean_bwd_cells(K, FP, val, gid=True)
    for K, FP in HEADS:
        for bf in (False, True):
            cells += [f"bwd_rows<FP={FP},BF={_b(bf)}>", f"score_param<FP={FP},BF={_b(bf)}>"]
            for val in (False, True):
                for train, cd, fd in ((False, 0, 0), (True, 0, 0), (True, .5, .5)):      # eval, train, FAST
                    cells += fwd_cells(K, FP, bf, val, train, cd, fd)
                for cd, gid in ((0.0, False), (0.5, True), (0.5, False)):                # MODE 0 (plain, FAST = 0 / 1) ...
                    for score in (False, True):
                        cells += bwd_cells(K, FP, bf, val, cd, gid=gid, score=score)
                if not bf:                                                               # ... and 1, 2, 3 (fp32 tables)
                    for kw in (dict(full_gather=True), dict(zero_rows=True)):
                        for score in (False, True):
                            cells += bwd_cells(K, FP, bf, val, 0.5, score=score, **kw)
                cells += bwd_cells(K, FP, bf, val, 0.5, masked=True)
            if bf:
                cells += fwd_cells(K, FP, True, False, False, 0, 0, deep=True, forms=(WAVE,))
                cells += fwd_cells(K, FP, True, True, False, 0, 0, deep=True, forms=(WAVE,))
        cells.append(f"coef<K={K}>")
    cells += fwd_cells(8, 8, False, False, True, .5, .5, shared_hash=True, forms=(WAVE,))
    cells += fwd_cells(8, 8, True, False, True, .5, .5, shared_hash=True, forms=(WAVE,))
    return sorted(set(cells))


CELLS = _all_cells()


# ------------------------------------------------------------------------------------------------ helpers
def seg_sum(v, rp):
    """Sums of the segments rp[i] .. rp[i + 1] of v along axis 0 (np.add.reduceat; empty segments give 0)."""
    out = np.zeros((len(rp) - 1,) + v.shape[1:])
    ne = rp[1:] > rp[:-1]
    if ne.any():
        out[ne] = np.add.reduceat(v, rp[:-1][ne], axis=0)
    return out


def seg_max(v, rp, empty):
    out = np.full((len(rp) - 1,) + v.shape[1:], float(empty))
    ne = rp[1:] > rp[:-1]
    if ne.any():
        out[ne] = np.maximum.reduceat(v, rp[:-1][ne], axis=0)
    return out


def keep_bits(H32, bf16):
    """The keep bit of every stored element: bit 0 (fp32) or bit 16 of the widened bf16 value."""
    bits = np.ascontiguousarray(H32, dtype=np.float32).view(np.uint32)
    return ((bits >> np.uint32(16 if bf16 else 0)) & np.uint32(1)).astype(np.float64)


def bf16_round(x):
    """float64 / float32 -> the bf16 value (as float64) han_f32_to_bf16_bits stores: to fp32, then nearest-even."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return (r & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32).astype(np.float64)


def inv_keep(drop):
    """1.f / (1.f - drop) as han_set_dropout forms it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(drop)))


def _in(a):
    """An input as float64: fp32 (or bf16-widened) values promoted; float64 arrays (the host tests' exact chain) as they are."""
    a = np.asarray(a)
    return a if a.dtype == np.float64 else up(a)


def _slabs(rowptr, max_edges=1 << 12):
    """Row ranges of at most max_edges entries each (a single longer row stands alone)."""
    n = len(rowptr) - 1
    lo = 0
    while lo < n:
        hi = int(np.searchsorted(rowptr, rowptr[lo] + max_edges, side="right")) - 1
        hi = min(max(hi, lo + 1), n)
        yield lo, hi
        lo = hi


def _act(pre, e_pre, elu):
    if not elu:
        return pre, e_pre
    out = np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0.0)))
    extra = np.where(pre <= e_pre, (2 + 2 * np.abs(pre)) * U * np.exp(np.minimum(pre, 0.0)) + U * np.abs(out), 0.0)
    return out, e_pre + extra


# ------------------------------------------------------------------------------------------------ forward
def fwd_ref(rowptr, colidx, H, f1, a2, b2, c, *, bf16=False, values=None, train=False, coef_drop=0.0, fts_drop=0.0,
            seed=0, seed_dev=None, row_offset=0, gid=None, res=None, elu=True, f2=None, path=None, binned=True,
            split=(SPLIT_DEG, SPLIT_CHUNK), want_coef=False, plant=(), lean=False, row_ids=None, dense=False):
    """The forward of the module docstring for every row.  H (NT, 64) float32 (a bf16 table widened); f2 (NT, K): given
    scores (f2_src, the lean kernels, node_attn_coefs) instead of recomputed ones.  path: per-row P (default: from the
    dispatch mirror).  plant: deliberate errors for the host tests ("ignore_keep", "swap_mask", "keep_twice").
    row_ids: the ids of the rows in their graph when the rows given are a sample of it (sample_rows): the dropout keys.
    Returns a namespace: out, lse, aggp, tsum (+ e_*), coef / e_coef (E, K) when asked, undecided (entries)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx, dtype=np.int64)
    K, FP = a2.shape
    N = len(rowptr) - 1
    deg = np.diff(rowptr)
    H32 = np.ascontiguousarray(H, dtype=np.float32)
    Hs_all = H32.astype(np.float64).reshape(-1, K, FP)
    f1, a2, b2, c = _in(f1), _in(a2), _in(b2), _in(c)
    resv = np.zeros((N, D)) if res is None else _in(res)
    seed = rng_ref.resolve_seed(seed, seed_dev)
    ikc = inv_keep(coef_drop) if train else 1.0
    ikf = inv_keep(fts_drop) if (train and fts_drop > 0) else 1.0
    if train and fts_drop > 0 and "ignore_keep" not in plant:
        Hd_all = Hs_all * keep_bits(H32, bf16).reshape(-1, K, FP)
    else:
        Hd_all = Hs_all
    if path is None:
        path = _p_wave(deg) + FOLD if lean else fwd_path(deg, row_forms(deg, binned, split[0]), split[1])
    tscale = float(np.log2(np.e)) if lean else 1.0
    if dense:
        tiles, S = dense_split(N, H32.shape[0])
        path = np.full(N, 32 * tiles + S + 2, dtype=np.int64)
        Fmax = _in(f2).max(0)
    scale = ikc * ikf * (ikc if "keep_twice" in plant else 1.0)
    r = types.SimpleNamespace(N=N, K=K, FP=FP, undecided=0)
    agg, e_agg = np.zeros((N, K, FP)), np.zeros((N, K, FP))
    r.aggp, r.e_aggp = np.zeros((N, K, FP)), np.zeros((N, K, FP))
    r.tsum, r.e_tsum = np.zeros((N, K)), np.zeros((N, K))
    r.lse, r.e_lse = np.full((N, K), NEG_BIG), np.zeros((N, K))
    if want_coef:
        r.coef, r.e_coef = np.zeros((len(colidx), K)), np.zeros((len(colidx), K))
    for lo, hi in _slabs(rowptr):
        e0, e1 = int(rowptr[lo]), int(rowptr[hi])
        if e1 == e0:
            continue
        rp = rowptr[lo:hi + 1] - e0
        cols = colidx[e0:e1]
        rows = np.repeat(np.arange(hi - lo), deg[lo:hi])
        Hs = Hs_all[cols]
        if f2 is not None:
            f2e, e_f2 = _in(f2)[cols], 0.0
        else:
            f2e = (Hs * a2).sum(-1) + b2
            e_f2 = (hs(FP) + 1) * U * ((np.abs(Hs) * np.abs(a2)).sum(-1) + np.abs(b2))
        w = np.ones((e1 - e0, 1)) if values is None else up(values)[e0:e1, None]
        x = (f1[lo:hi][rows] + f2e) * w
        e_x = np.abs(w) * e_f2 + 2 * U * np.abs(x)
        if lean:
            e_x = np.abs(w) * (2 * np.abs(f1[lo:hi][rows]) + np.abs(f2e)) * U + 2 * U * np.abs(x)
        sg = np.where(x > 0, 1.0, SLOPE) * w
        e = np.where(x > 0, x, SLOPE * x)
        e_e = e_x + U * np.abs(e)
        undec = np.abs(x) <= e_x
        r.undecided += int(undec.sum())
        m = seg_max(e, rp, NEG_BIG)
        t = e - m[rows]
        p = np.exp(t)
        l = seg_sum(p, rp)
        ne = deg[lo:hi] > 0
        lsafe = np.where(l > 0, l, 1.0)
        wgt = p / lsafe[rows]
        E = e_e + seg_max(e_e, rp, 0.0)[rows]
        if lean:
            E = E + 4 * U * np.abs(m[rows])
        rho = np.expm1(E + (path[lo:hi][rows][:, None] + 3 * tscale * np.abs(t)) * U)
        if dense:
            xF = (f1[lo:hi] + Fmax)[rows]
            mF = np.where(xF > 0, xF, SLOPE * xF)
            y = f2e - Fmax
            rho = np.expm1((2 * np.abs(xF) + np.abs(mF) + 3 * np.abs(xF - mF) + 3 * np.abs(SLOPE * xF - mF) + 4 * np.abs(y)
                            + 5 + path[lo:hi][rows][:, None]) * U)
        rden = seg_sum(wgt * rho, rp)
        assert (rden < 0.5).all()
        ew = wgt * ((1 + rho) * (1 + C_FIN * U) / (1 - rden[rows]) - 1) + TINY
        am = np.ones_like(wgt)
        if train and coef_drop > 0:
            gj = cols if gid is None else np.asarray(gid, dtype=np.int64)[cols]
            gi = (rows + lo if row_ids is None else np.asarray(row_ids, dtype=np.int64)[rows + lo]) + row_offset
            am = rng_ref.coef_draws(seed, gj, gi, K, coef_drop) if "swap_mask" in plant else \
                rng_ref.coef_draws(seed, gi, gj, K, coef_drop)
        Hd = Hd_all[cols]
        wa = (wgt * am)[:, :, None]
        agg[lo:hi] = seg_sum(wa * Hd, rp) * scale
        aHd = np.abs(Hd) * am[:, :, None]
        e_agg[lo:hi] = seg_sum(ew[:, :, None] * aHd, rp) * scale
        if want_coef:
            r.coef[e0:e1] = wgt * am * ikc
            r.e_coef[e0:e1] = ew * am * ikc
        if train or want_coef:
            lg = np.log(lsafe)
            r.lse[lo:hi] = np.where(ne[:, None], m + lg, NEG_BIG)
            if dense:      # the fixed shift in the place of the running maximum: the same lse, other magnitudes
                mD = f1[lo:hi] + Fmax
                mD = np.where(mD > 0, mD, SLOPE * mD)
                m, lg = mD, m + lg - mD
            r.e_lse[lo:hi] = np.where(ne[:, None], -np.log1p(-rden) + 4 * U * np.maximum(1.0, np.abs(lg))
                                      + U * ((3 if lean else 1) * np.abs(m) + np.abs(lg) + np.abs(m + lg)), 0.0)
            esg = ew * np.abs(sg) + np.where(undec, wgt * (1 - SLOPE) * np.abs(w), 0.0)
            r.tsum[lo:hi] = seg_sum(wgt * sg, rp)
            r.e_tsum[lo:hi] = seg_sum(esg, rp)
            r.aggp[lo:hi] = seg_sum(wa * sg[:, :, None] * Hd, rp) * scale
            r.e_aggp[lo:hi] = seg_sum(esg[:, :, None] * aHd, rp) * scale
    r.agg, r.e_agg = agg.reshape(N, D), e_agg.reshape(N, D)
    r.aggp, r.e_aggp = r.aggp.reshape(N, D), r.e_aggp.reshape(N, D)
    r.pre = r.agg + c + resv
    r.e_pre = r.e_agg + 2 * U * (np.abs(r.agg) + np.abs(c) + np.abs(resv))
    r.out, r.e_out = _act(r.pre, r.e_pre, elu)
    return r


def fwd_ratios(r, out, saved=None):
    """err / bound per output of one node_attn_fwd call (NumPy arrays; saved = (lse, aggp, tsum))."""
    res = {"out": ratio(out, r.out, r.e_out)}
    if saved is not None:
        res.update(lse=ratio(saved[0], r.lse, r.e_lse), aggp=ratio(saved[1], r.aggp, r.e_aggp),
                   tsum=ratio(saved[2], r.tsum, r.e_tsum))
    return res


# ------------------------------------------------------------------------------------------------ row-local backward
def bwd_rows_ref(dOut, out, aggp, tsum, f1, lse, c, K, FP, *, res=None, elu=True, bf16=False, g_stored=None, plant=()):
    """The row-local backward of the module docstring.  g_stored (N, 64): the g values the kernel stored (widened); s,
    df1 and z are formed from them (default: from the reference's own rounded g).  plant: "s_with_c", "unrounded_g"."""
    dOut, o, aggp, tsum, c = _in(dOut), _in(out), _in(aggp), _in(tsum), _in(c)
    N = o.shape[0]
    resv = np.zeros((N, D)) if res is None else _in(res)
    neg = (o <= 0) & bool(elu)
    da = np.where(neg, o + 1.0, 1.0)
    live = da > 0
    lg = np.log(np.where(live, da, 1.0))
    pre = np.where(neg, lg, o)
    e_pt = np.where(neg & live, U + 4 * U * np.maximum(1.0, np.abs(lg)), 0.0)
    r = types.SimpleNamespace(N=N)
    r.g = g = dOut * da
    r.e_g = e_g = 2 * U * np.abs(g)
    r.g_lo, r.g_hi = (bf16_round(g - e_g), bf16_round(g + e_g)) if bf16 else (g - e_g, g + e_g)
    r.dc, r.e_dc = g.sum(0), e_g.sum(0) + depth_rows(N) * U * np.abs(g).sum(0)
    gs = _in(g_stored) if g_stored is not None else (bf16_round(g) if bf16 else g)
    r.gs = gs
    gsk = gs.reshape(N, K, FP)
    inner = pre - resv - (0.0 if "s_with_c" in plant else c)
    terms = (gs * inner).reshape(N, K, FP)
    r.s = terms.sum(-1)
    r.e_s = (np.abs(gs) * (e_pt + 2 * U * (np.abs(pre) + np.abs(c) + np.abs(resv)))).reshape(N, K, FP).sum(-1) \
        + (hs(FP) + 1) * U * np.abs(terms).sum(-1)
    gd = g.reshape(N, K, FP) if "unrounded_g" in plant else gsk
    dpt = gd * aggp.reshape(N, K, FP)
    dp = dpt.sum(-1)
    r.df1 = dp - r.s * tsum
    r.e_df1 = (hs(FP) + 1) * U * np.abs(dpt).sum(-1) + np.abs(tsum) * r.e_s + 2 * U * (np.abs(dp) + np.abs(r.s * tsum))
    r.z = np.where((gsk == 0).all(-1), GS_Z_ALL_ZERO, 0).astype(np.uint32)
    return r


# ------------------------------------------------------------------------------------------------ transposed-graph backward
def bwd_cols_ref(colptr, rowidx, g, stats, H, f2, df1, a1, a2, *, bf16=False, values=None, coef_drop=0.0, fts_drop=0.0,
                 seed=0, seed_dev=None, src_offset=0, dst_offset=0, gid=None, binned=True, split=(SPLIT_DEG, SPLIT_CHUNK),
                 empty_mid=False, lean=False, row_ids=None, dense=False):
    """The transposed-graph backward of the module docstring.  g (NT, 64): the stored g rows widened; stats (NT, K, 4).
    Entries with rowidx < 0 are dropped.  Returns dH, df2 (+ e_*) and `flushed`, the entries with an alpha below TINY."""
    colptr = np.asarray(colptr, dtype=np.int64)
    rowidx = np.asarray(rowidx, dtype=np.int64)
    K, FP = a1.shape
    NS = len(colptr) - 1
    deg = np.diff(colptr)
    path = _ceil(deg, 4) + 3 if lean else bwd_path(deg, row_forms(deg, binned, split[0], empty_mid), split[1])
    cdot = max(hs(FP) + 2, 10) if lean else hs(FP) + 2
    g64 = _in(g).reshape(-1, K, FP)
    st = _in(stats)
    H32 = np.ascontiguousarray(H, dtype=np.float32)
    Hk = H32.astype(np.float64).reshape(NS, K, FP)
    mk = keep_bits(H32, bf16).reshape(NS, K, FP) * inv_keep(fts_drop) if fts_drop > 0 else np.ones((NS, K, FP))
    hd_all = Hk * mk
    f2, df1, a1, a2 = _in(f2), _in(df1), _in(a1), _in(a2)
    if dense:
        tiles, S = dense_split(NS, g64.shape[0])
        path = np.full(NS, 32 * tiles + S + 2, dtype=np.int64)
        Fmax = f2.max(0)
    seed = rng_ref.resolve_seed(seed, seed_dev)
    ikc = inv_keep(coef_drop)
    r = types.SimpleNamespace(NS=NS, flushed=0, entries=0)
    acc, e_acc = np.zeros((NS, K, FP)), np.zeros((NS, K, FP))
    r.df2, r.e_df2 = np.zeros((NS, K)), np.zeros((NS, K))
    for lo, hi in _slabs(colptr):
        e0, e1 = int(colptr[lo]), int(colptr[hi])
        if e1 == e0:
            continue
        rp = colptr[lo:hi + 1] - e0
        src = np.repeat(np.arange(lo, hi), deg[lo:hi])
        dst = rowidx[e0:e1]
        livee = dst >= 0
        d = np.where(livee, dst, 0)
        w = np.ones((e1 - e0, 1)) if values is None else up(values)[e0:e1, None]
        x = (st[d, :, 0] + f2[src]) * w
        sg = np.where(x > 0, 1.0, SLOPE) * w
        e = np.where(x > 0, x, SLOPE * x)
        t = e - st[d, :, 1]
        alpha = np.exp(t) * livee[:, None]
        rho = np.expm1(2 * U * np.abs(x) + U * np.abs(e) + (2 + 3 * np.abs(t)) * U)
        if dense:
            xF = st[d, :, 0] + Fmax
            y = f2[src] - Fmax
            lse_i = st[d, :, 1]
            rho = np.expm1((2 * np.abs(xF) + 3 * np.abs(xF - lse_i) + 3 * np.abs(SLOPE * xF - lse_i) + 4 * np.abs(y) + 5) * U)
        r.flushed += int(((alpha < TINY) & livee[:, None]).sum())
        r.entries += int(livee.sum()) * K
        am = np.full_like(alpha, 1.0)
        if coef_drop > 0:
            gi = (d if gid is None else np.asarray(gid, dtype=np.int64)[d]) + dst_offset
            gsrc = src if row_ids is None else np.asarray(row_ids, dtype=np.int64)[src]
            am = rng_ref.coef_draws(seed, gi, gsrc + src_offset, K, coef_drop) * ikc
        gk = g64[d]
        gh = gk * hd_all[src]
        dot, adot = gh.sum(-1), np.abs(gh).sum(-1)
        s = st[d, :, 2]
        inner = am * dot - s
        term = alpha * sg * inner
        e_term = np.abs(alpha * sg) * (cdot * U * am * adot + U * (np.abs(am * dot) + np.abs(s))) \
            + (rho + 4 * U) * np.abs(term) + TINY * np.abs(sg * inner) * livee[:, None]
        if dense:
            e_term = np.abs(alpha * sg) * (9 * U * am * adot + (rho + 5 * U) * (np.abs(am * dot) + np.abs(s))) \
                + TINY * np.abs(sg) * (np.abs(am * dot) + np.abs(s))
        P = path[lo:hi][:, None]
        r.df2[lo:hi] = seg_sum(term, rp)
        r.e_df2[lo:hi] = seg_sum(e_term, rp) + P * U * seg_sum(np.abs(term), rp)
        wt = (alpha * am)[:, :, None] * gk
        acc[lo:hi] = seg_sum(wt, rp)
        e_acc[lo:hi] = seg_sum((rho + 2 * U)[:, :, None] * np.abs(wt) + (TINY * am * livee[:, None])[:, :, None] * np.abs(gk), rp) \
            + P[:, :, None] * U * seg_sum(np.abs(wt), rp)
    t1, t2, t3 = acc * mk, df1[:, :, None] * a1, r.df2[:, :, None] * a2
    r.dH = (t1 + t2 + t3).reshape(NS, D)
    r.e_dH = (e_acc * mk + r.e_df2[:, :, None] * np.abs(a2) + 3 * U * (np.abs(t1) + np.abs(t2) + np.abs(t3))).reshape(NS, D)
    return r


# ------------------------------------------------------------------------------------------------ score gradients
def score_ref(H, df1, df2, K, FP, depth):
    """da1, da2 (K, F'), db1, db2 (K,) with bounds depth x u x sum |terms| (H as stored)."""
    Hk = up(H).reshape(-1, K, FP)
    r = types.SimpleNamespace()
    for name, dname, d in (("da1", "db1", _in(df1)), ("da2", "db2", _in(df2))):
        setattr(r, name, np.einsum("jk,jkf->kf", d, Hk))
        setattr(r, "e_" + name, depth * U * np.einsum("jk,jkf->kf", np.abs(d), np.abs(Hk)))
        setattr(r, dname, d.sum(0))
        setattr(r, "e_" + dname, depth * U * np.abs(d).sum(0))
    return r


def score_ratios(r, got):
    return {n: ratio(g, getattr(r, n), getattr(r, "e_" + n)) for n, g in zip(("da1", "da2", "db1", "db2"), got)}


# ------------------------------------------------------------------------------------------------ inputs
EDGE_LENGTHS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
EDGE_LONG = (1023, 1024, 1025, 2500)          # the SPLIT_DEG / SPLIT_CHUNK boundary of han_amd.ops, no monkeypatch
EDGE_NT = 2579                                # a prime above the longest row: columns stay distinct within a row


def graph_from_lengths(lengths, nt, stride=13):
    """rowptr, colidx: row i lists (7 i + stride e) % nt for e < lengths[i] -- distinct within a row while
    lengths[i] <= nt and gcd(stride, nt) = 1."""
    lens = np.asarray(lengths, dtype=np.int64)
    assert lens.max(initial=0) <= nt and np.gcd(stride, nt) == 1
    rowptr = np.zeros(len(lens) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    i = np.repeat(np.arange(len(lens)), lens)
    e = np.arange(rowptr[-1]) - rowptr[:-1][i]
    return rowptr, ((7 * i + stride * e) % nt).astype(np.int32)


@functools.lru_cache(maxsize=None)
def edge_graph():
    """About 400 rows: the lengths of EDGE_LENGTHS cycling (the 4- and 16-edge step edges, the short / wave bin edge), the
    rows of EDGE_LONG spread among them; the first and the last row hold entries.  (The long rows need a table of at least
    2500 rows for distinct columns: EDGE_NT, not the 257 rows the short ones would do with.)"""
    lens = [EDGE_LENGTHS[(i + 1) % len(EDGE_LENGTHS)] for i in range(23 * len(EDGE_LENGTHS) + 6)]
    for k, n in enumerate(EDGE_LONG):
        lens[37 + 91 * k] = n
    assert lens[0] > 0 and lens[-1] > 0
    rowptr, colidx = graph_from_lengths(lens, EDGE_NT)
    for a in (rowptr, colidx):
        a.setflags(write=False)
    return rowptr, colidx


LOOP_NT = 4099                                # a small table: the gather of the loop cases stays cheap
LOOP_SPLIT = (16, 16)                         # SPLIT_DEG = SPLIT_CHUNK of the chunk case
LOOP_ROWS = 2 * 16 * REDUCE_BLOCKS + 5        # bwd_rows / score_param_bwd: 1024 blocks of 16 lane groups, twice, and 5


@functools.lru_cache(maxsize=None)
def loop_graph(kind):
    """Graphs that send every block of a launch round its grid-stride loop twice and a few a third time (attn_grid caps
    at 8192 blocks of 4 waves): "wave" 2 x 32768 + 5 rows of 16 .. 24 entries; "short" 2 x 131072 + 7 rows of 1 .. 15
    entries (four to a wave; most hold 1 .. 3, every 16th 15 and every 16th 8, to keep the float64 work in seconds);
    "chunk" rows of 17 / 32 / 33 / 48 entries that LOOP_SPLIT cuts into 2 x 32768 + 5 chunks.  Table: LOOP_NT rows."""
    if kind == "wave":
        i = np.arange(2 * 32768 + 5)
        lens = 16 + (7 * i) % 9
    elif kind == "short":
        i = np.arange(2 * 131072 + 7)
        lens = np.where(i % 16 == 5, 15, np.where(i % 16 == 11, 8, 1 + i % 3))
    else:
        lens = np.tile(np.array([17, 32, 33, 48]), 6554)        # 10 chunks per 4 rows: 65540
        lens[0] = 33                                            # + 1
    rowptr, colidx = graph_from_lengths(lens, LOOP_NT)
    for a in (rowptr, colidx):
        a.setflags(write=False)
    return rowptr, colidx


@functools.lru_cache(maxsize=None)
def dense_graph(n, nt):
    """n rows against nt columns, density >= 0.65: lengths between 0.66 nt and nt, one empty row, one full row, columns
    distinct within a row (the bit mask holds no repeated entry)."""
    lens = (0.66 * nt + (np.arange(n) * 37 % 101) / 100.0 * 0.34 * nt).astype(np.int64)
    lens[n // 2] = 0
    lens[n // 3] = nt
    rowptr, colidx = graph_from_lengths(lens, nt, stride=11)
    assert rowptr[-1] >= 0.65 * n * nt
    for a in (rowptr, colidx):
        a.setflags(write=False)
    return rowptr, colidx


LEAN_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 333)      # mean 89: the lean kernels take the graph
LEAN_NT = 1031                                                              # density 9 %: not the dense form


@functools.lru_cache(maxsize=None)
def lean_graph():
    """131 rows against a 1031-row table, mean degree >= 64 (han_amd.ops._use_lean), density far below DENSE_MIN_DENSITY."""
    lens = [LEAN_LENGTHS[(i + 3) % len(LEAN_LENGTHS)] for i in range(131)]
    rowptr, colidx = graph_from_lengths(lens, LEAN_NT)
    assert rowptr[-1] >= 64 * 131 and lens[0] > 0 and lens[-1] > 0
    for a in (rowptr, colidx):
        a.setflags(write=False)
    return rowptr, colidx


def sample_rows(rowptr, colidx, rows):
    """(rowptr, colidx) of the rows `rows` alone, in that order."""
    rows = np.asarray(rows, dtype=np.int64)
    lens = np.diff(rowptr)[rows]
    rp = np.zeros(len(rows) + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    idx = np.repeat(rowptr[:-1][rows] - rp[:-1], lens) + np.arange(rp[-1])
    return rp, colidx[idx]


LEAN_LOOP_ROWS = 2 * 32768 + 5                # a wave per row on 8192 blocks of 4


def lean_loop_sample(n=LEAN_LOOP_ROWS, seed=0):
    """The rows of the lean loop case that get the float64 comparison: the first and the last 256 rows of each grid pass
    and 4096 random ones (the rest is checked finite)."""
    per = 4 * GRID_CAP
    pick = set(np.random.default_rng([n, seed]).permutation(n)[:4096].tolist())
    for lo in range(0, n, per):
        hi = min(lo + per, n)
        pick |= set(range(lo, min(lo + 256, hi))) | set(range(max(hi - 256, lo), hi))
    return np.array(sorted(pick), dtype=np.int64)


def transpose(rowptr, colidx, nt, values=None):
    """(colptr, rowidx[, values]) of the transposed graph, destinations ascending (CSRGraph.transpose's order)."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(colidx, kind="stable")
    colptr = np.zeros(nt + 1, dtype=np.int64)
    colptr[1:] = np.cumsum(np.bincount(colidx, minlength=nt))
    out = (colptr, rows[order].astype(np.int32))
    return out + ((values[order],) if values is not None else ())


def stamp_keep_bits(H32, bf16, keep):
    """H with the lowest stored mantissa bit of every element replaced by keep (0 / 1), as K1 stamps it."""
    bits = np.ascontiguousarray(H32, dtype=np.float32).view(np.uint32).copy()
    sh = np.uint32(16 if bf16 else 0)
    bits = (bits & ~(np.uint32(1) << sh)) | (keep.astype(np.uint32) << sh)
    return bits.view(np.float32)


@functools.lru_cache(maxsize=None)
def fwd_inputs(K, FP, bf16, n_rows, nt, kind="plain", fts_drop=0.0, seed=0):
    """Seeded forward inputs (read-only): H (nt, 64) float32 (bf16 values widened; keep bits stamped from the fts stream
    of rng_ref when fts_drop > 0), f1 (n_rows, K), f2 (nt, K) = the float64 scores rounded (for the f2 / coefs calls), a2,
    b2, c, res, values.  kind "wide": scores spread over more than 80."""
    rng = np.random.default_rng([K, FP, int(bf16), n_rows, nt, seed, int(kind == "wide")])
    H = rng.standard_normal((nt, D)).astype(np.float32)
    if bf16:
        H = bf16_round(H).astype(np.float32)
    if fts_drop > 0:
        H = stamp_keep_bits(H, bf16, rng_ref.fts_mask(5 + seed, nt, D, fts_drop).astype(np.uint32))
    sc = 25.0 if kind == "wide" else 0.6
    a2 = (rng.standard_normal((K, FP)) * sc / np.sqrt(FP)).astype(np.float32)
    b2 = (rng.standard_normal(K) * 0.1).astype(np.float32)
    f1 = (rng.standard_normal((n_rows, K)) * (0.25 * sc)).astype(np.float32)
    f2 = ((up(H).reshape(nt, K, FP) * up(a2)).sum(-1) + up(b2)).astype(np.float32)
    c = (rng.standard_normal(D) * 0.2).astype(np.float32)
    res = (rng.standard_normal((n_rows, D)) * 0.5).astype(np.float32)
    d = dict(H=H, f1=f1, f2=f2, a2=a2, b2=b2, c=c, res=res)
    for v in d.values():
        v.setflags(write=False)
    return d


def edge_values(nnz, seed=0):
    """Stored adjacency values in [0.25, 1.75) with a tenth of them negative."""
    rng = np.random.default_rng([nnz, seed, 77])
    v = 0.25 + 1.5 * rng.random(nnz)
    return np.where(rng.random(nnz) < 0.1, -v, v).astype(np.float32)


def sort_rows_by_score(rowptr, colidx, f2, head=0):
    """The entries of every row reordered so that the head's score ascends: the maximum arrives last."""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.lexsort((up(f2)[colidx, head], rows))
    return colidx[order]


@functools.lru_cache(maxsize=None)
def bwd_rows_inputs(K, FP, N, seed=0):
    """Synthetic inputs of the row-local backward (read-only): outputs exactly -1, 0, just below 0 and just above -1
    among ELU outputs, heads whose dOut is all +-0."""
    rng = np.random.default_rng([K, FP, N, seed, 3])
    pre = rng.standard_normal((N, D)) * 2.0
    out = np.where(pre > 0, pre, np.expm1(pre)).astype(np.float32)
    kind = rng.integers(0, 40, size=(N, D))
    out[kind == 0] = -1.0
    out[kind == 1] = 0.0
    out[kind == 2] = -np.float32(2.0 ** -24)
    out[kind == 3] = np.float32(-1.0) + np.float32(2.0 ** -24)
    dOut = rng.standard_normal((N, D)).astype(np.float32)
    zero = rng.random((N, K)) < 0.25
    dk = dOut.reshape(N, K, FP)
    dk[zero] = 0.0
    dk[zero & (rng.random((N, K)) < 0.5)] = -0.0
    d = dict(out=out, dOut=dOut, aggp=rng.standard_normal((N, D)).astype(np.float32),
             tsum=(0.2 + 0.8 * rng.random((N, K))).astype(np.float32), f1=rng.standard_normal((N, K)).astype(np.float32),
             lse=(rng.standard_normal((N, K)) + 2).astype(np.float32), c=(rng.standard_normal(D) * 0.2).astype(np.float32),
             res=(rng.standard_normal((N, D)) * 0.5).astype(np.float32), zero=zero)
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def bwd_cols_inputs(K, FP, bf16, ns, nt, fts_drop=0.0, seed=0):
    """Synthetic inputs of the transposed-graph backward (read-only): H, f2, df1 (ns rows), a1, a2, and the gs table of
    nt destinations as g (nt, 64) float32 (bf16 values widened) and stats (nt, K, 4): finite records, alpha =
    exp(lrelu(f1 + f2) - lse) stays below 1, a quarter of the heads all zero with z set."""
    rng = np.random.default_rng([K, FP, int(bf16), ns, nt, seed, 9])
    H = rng.standard_normal((ns, D)).astype(np.float32)
    if bf16:
        H = bf16_round(H).astype(np.float32)
    if fts_drop > 0:
        H = stamp_keep_bits(H, bf16, rng_ref.fts_mask(5 + seed, ns, D, fts_drop).astype(np.uint32))
    g = rng.standard_normal((nt, K, FP)).astype(np.float32)
    zero = rng.random((nt, K)) < 0.25
    g[zero] = 0.0
    g = g.reshape(nt, D)
    if bf16:
        g = bf16_round(g).astype(np.float32)
    stats = np.zeros((nt, K, 4), dtype=np.float32)
    stats[:, :, 0] = rng.standard_normal((nt, K)) * 0.5
    stats[:, :, 1] = 2.0 + rng.random((nt, K))
    stats[:, :, 2] = rng.standard_normal((nt, K)) * 0.1
    stats[:, :, 3] = np.where(zero, np.uint32(GS_Z_ALL_ZERO), np.uint32(0)).astype(np.uint32).view(np.float32)
    df1 = rng.standard_normal((ns, K)).astype(np.float32)
    d = dict(H=H, f2=(rng.standard_normal((ns, K)) * 0.5).astype(np.float32), df1=df1,
             a1=(rng.standard_normal((K, FP)) * 0.3).astype(np.float32),
             a2=(rng.standard_normal((K, FP)) * 0.3).astype(np.float32), g=g, stats=stats)
    for v in d.values():
        v.setflags(write=False)
    return d
