"""float64 reference of the K3 semantic attention (han_amd/csrc/sem_attn.hip; utils/layers.py:152-159) and of its
gradients, with a running fp32 error bound, and the seeded inputs the host and the GPU tests share (test infrastructure,
NumPy only).

    pre = M W + b      v = tanh(pre)      s_p = v_p . u      beta = softmax_p(s)      Z = sum_p beta_p M_p

Every function takes the fp32 values the kernel sees and promotes them to float64 (`up`).  Next to each result `x`
stands an elementwise bound `e_x` on |fp32 kernel - float64|, built from u = 2^-24 (`U`, the relative rounding error of
one fp32 operation) and counts of roundings; nothing here is a measurement.  The kernels reorder every sum freely
(MFMA k-steps, 16-lane butterflies, lane groups, waves through LDS, blocks through slabs), so no summation order is
assumed: a sum of n terms, each term the result of at most one rounded product, carries at most n roundings per term,
|error| <= n u sum |terms|.  Errors of inputs are propagated to first order with the second-order products kept where
an input error is not itself O(u) (e_s in the wide-range case), hence the expm1 / exp below.

pre     fp32 pipe (v_mfma_f32_16x16x4_f32): D fused multiply-adds, the bias addition: (D + 1) roundings.
        bf16 x 6 pipe (han_b6.h): x = h + m + l and w = h' + m' + l' exactly, by truncation, so the three terms of a
        number share its sign and |h| + |m| + |l| = |x|: the absolute sum of the kept products does not exceed |x w|.
        Six of the nine products are formed (each exact in the fp32 accumulator); dropped are m l', l m' and l l',
        |m| < 2^-8 |x|, |l| < 2^-16 |x|:  2^-24 + 2^-24 + 2^-32 < 3u of |x w| per k index.  The accumulation is counted
        as one rounding per k index, as on the fp32 pipe: an output sees 6 D / 32 instructions of K = 32, and this count
        holds as long as such an instruction rounds no more often than after every sixth of the products it adds (the
        one property of the matrix pipe the bound relies on; a pipe that rounded after every product would need 6 D).
        One bound for every kernel form, C_MM = 3, C_PRE = C_MM + 1:
                                                       e_pre = (D + C_PRE) u (|M| |W| + |b|)
v       fast_tanh(x) = 1 - 2 rcp(1 + e), e = __expf(2x) (sem_attn.hip:35-40).  2x is exact.  __expf(t) is
        v_exp_f32(t * log2(e)): the rounded constant and the rounded product move the exponent by 2 |t| u log2(e), the
        result by 2 |t| u relative; v_exp_f32 is good to 1 ulp (<= 2u relative) and v_rcp_f32 to 1 ulp (AMD Instinct
        CDNA3 / CDNA4 ISA guides, the VOP1 opcode descriptions of V_EXP_F32 and V_RCP_F32: "1 ULP accuracy"; the
        same figures stand behind `__expf` in loss_opt_ref).  So e carries (2 + 4|x|) u relative, d = 1 + e one
        rounding, q = rcp(d) the error of e scaled by e / (1 + e) = (1 + v) / 2 plus u + 2u, 2q = 1 - v is exact
        and the last subtraction rounds once:
                 |fast_tanh(x) - tanh(x)| <= c_t u,    c_t = (1 - v^2)(1 + 2|x|) + 3 (1 - v) + |v|
        c_t is 4 at x = 0, 1 for v -> 1, 7 for v -> -1 and peaks at 7.4 near x = -1.6: the absolute error is below
        7.5u = 4.5e-7, and the "~2e-7" of the code comment is the typical size (4u = 2.4e-7 around 0), not the bound.
        The error of pre moves tanh by at most e_pre sech^2(x) e^(2 e_pre) (sech^2(x + d) <= sech^2(x) e^(2|d|)):
                                                       e_v = e_pre (1 - v^2) e^(2 e_pre) + c_t u
        (e^(2x) <= 1 + 2x + 4x^2 for x < 1/4 in the code.)
s       A products and additions in any order:         e_s = e_v |u| + A u (|v| |u|)
beta    x_p = s_p - max s.  exp(x_p) as the kernel forms it: both scores move (E_p = e_s[p] + e_s[argmax], the pattern
        of loss_opt_ref), the subtraction rounds (|x| u in the exponent), __expf as above (2 + 2|x|) u:
                                                       rho_p = expm1(E_p + (2 + 3|x_p|) u)
        The block-level kernels run an online softmax: a term is rescaled by up to P - 1 factors exp(m_old - m_new),
        whose exponents telescope to |x_p|, each factor with its __expf ulp (2u), a product and an addition: at most
        4P roundings per term of the denominator (the wave-local kernels add P terms directly: fewer).  The relative
        error of a sum of positive terms is the weighted mean of theirs:
                                                       rden = sum_q beta_q expm1(E_q + (4P + 3|x_q|) u)
        1 / den is an IEEE-accurate-to-2.5-ulp division (5u), the product with it one rounding:
                                                       r_p = (1 + rho_p)(1 + 6u) / (1 - rden) - 1
        A result of v_exp_f32 below the smallest normal is flushed to zero:    e_beta = beta r + TINY
Z       The wave-local kernels multiply the stored beta with M_p and add P terms; the block-level ones carry
        exp(.) M_p through the same rescaling chain as the denominator and scale by 1 / den at the end.  One weight
        bound for both, rz_p = (1 + expm1(E_p + (4P + 1 + 3|x_p|) u))(1 + 6u) / (1 - rden) - 1 >= r_p:
                                                       e_Z = sum_p (beta_p rz_p + TINY) |M_p| + P u sum_p beta_p |M_p|

The backward kernel RECEIVES the fp32 beta of the forward.  The reference's backward therefore starts from that given
beta promoted to float64 (`bt`), not from its own: otherwise the forward error would be charged twice.

dbeta   dbeta_p = dZ . M_p, D terms:                    e_dbeta = D u (|dZ| . |M_p|)
ds      c = sum_q bt_q dbeta_q (P terms), ds_p = bt_p (dbeta_p - c) (a subtraction and a product):
                 e_c = sum_q bt_q e_dbeta_q + P u sum_q bt_q |dbeta_q|
                                                       e_ds = bt_p (e_dbeta_p + e_c)(1 + 2u) + 2u |ds_p| + TINY
dpre    g = 1 - v^2 from the kernel's own v (a product, a subtraction, both of magnitude <= 1):
                 e_g = 2|v| e_v + e_v^2 + 2u
        dpre = (ds u_a) g, two products; x1 = |u_a| (e_ds g + |ds| e_g + e_ds e_g):
                                                       e_dpre = x1 (1 + 2u) + 2u |dpre| + TINY
        This is an absolute bound: where 1 - v^2 cancels (|v| -> 1) the 2u of e_g carries it.
dM      dM_p = bt_p dZ + dpre W^T: A + 1 terms in any order (the run-time-width kernels add the slices of A one launch
        after the other), on either matrix pipe (C_MM as for pre; an operand below the smallest normal may be flushed):
                 e_dM = e_dpre |W|^T + (A + 1 + C_MM) u (|dpre| |W|^T + |bt_p dZ|) + TINY (1 + sum_a |W|)
dW, db, du   sums over rows.  T = number of live nodes (dZ row not all zero).  A dead node has dbeta = 0 exactly, hence
        c = 0, ds = bt (0 - 0) = 0 and dpre = 0: it adds exact zeros, and so do the padding rows (ds = 0).  So at most
        T P terms round, whatever the order across lane, wave, block and slab:
                 e_dW = |M|^T e_dpre + (T P + C_MM) u |M|^T |dpre|
                 e_db = sum e_dpre + T P u sum |dpre|
                 e_du = sum (e_ds |v| + |ds| e_v + e_ds e_v) + (T P + 1) u sum |ds| |v|
        (du adds ds v with the kernel's v: one product more per term.)

The dispatch of sem_attn.hip is mirrored below in named constants (ROWS, BWD_BLOCKS, FWD_CAP, B6_ROWS); CELLS holds one
entry per cell of it, each with the smallest N (computed, `loop_n`) at which every block of the forward AND of the
backward grid passes its row loop two to three times.  tests/test_sem_attn_ref_host.py checks reference, bounds and
these constants without a GPU.
"""
import collections
import functools
import math
import types

import numpy as np

from tests.loss_opt_ref import TINY, U, ratio, up  # noqa: F401  (re-exported for the tests)

C_MM = 3
C_PRE = C_MM + 1

# ------------------------------------------------------------------------------------------------ dispatch mirror
ROWS = 64                     # rows per block iteration (4 waves x 16)
TILE = 16
BWD_BLOCKS = 256              # kSemBwdBlocks
FWD_CAP = {"wave": 1024, "b6": 768, "block": 768, "gen4": 512, "gen8": 512, "wide": 1024}
B6_ROWS = 64 * 1024           # from this many rows on the wave-local kernels use the bf16 x 6 pipe
WIDE_A_SLICE = 64             # WideBwdLds::AS
WIDE_D_CHUNK = 128            # kWideDChunk
FLAG_EXACT, FLAG_PAIRS, FLAG_G3_F32 = 8, 16, 32          # han_amd.ops.FLAG_K3_*
POW2 = (1, 2, 4, 8, 16)


def family(P, D, A):
    if not (D in (64, 128) and 64 <= A <= 256):
        return "wide"
    if D == 64 and A <= 128:
        return "wave" if P in POW2 else "block"
    return "gen4" if D == 64 else "gen8"


def uses_b6(N, P, D, A, flags):
    return family(P, D, A) == "wave" and N * P >= B6_ROWS and not flags & FLAG_EXACT


def nodes_per_unit(P):
    """Nodes of one block iteration: a chunk of 64 / P whole nodes; the wave-local kernels take four 16-row tiles, which
    hold 64 / P whole nodes as well (P divides 16)."""
    return ROWS // P


def grids(N, P, D, A, flags):
    """(units, forward grid, backward grid): a unit is what one block takes per iteration; block b takes units
    b, b + grid, ...  (The bf16-pipe backward takes two tiles per wave and pass: units b and b + grid together.)"""
    fam = family(P, D, A)
    units = max(1, -(-N // nodes_per_unit(P)))
    cap = FWD_CAP["b6" if uses_b6(N, P, D, A, flags) else fam]
    return units, min(units, cap), min(units, BWD_BLOCKS)


def wide_fwd_slice(A):
    return 256 if A % 256 == 0 else 192 if A % 192 == 0 else 128 if A % 128 == 0 else 64


def kernel_names(N, P, D, A, flags):
    """The template instances han_sem_attn_fwd / _bwd launch."""
    fam, ca, pc = family(P, D, A), min(A // 64, 4), P if P in POW2 else 16
    if fam == "wide":
        return f"fwd_wide<CA={wide_fwd_slice(A) // 64}>", "bwd_wide"
    if fam == "block":
        return f"fwd<CA={ca}>", f"bwd<CA={ca}>"
    if fam in ("gen4", "gen8"):
        dt = 4 if fam == "gen4" else 8
        return f"fwd_gen<CA={ca},DT={dt}>", f"bwd_gen<DT={dt}>"
    if not uses_b6(N, P, D, A, flags):
        return f"fwd_wave<CA={ca},P={pc}>", f"bwd_wave<CA={ca},P={pc}>"
    if ca == 2 and flags & FLAG_PAIRS:
        return f"fwd_wave_b6<CA={ca},P={pc}>", f"bwd_pair_b6<P={pc}>"
    return f"fwd_wave_b6<CA={ca},P={pc}>", f"bwd_wave_b6<CA={ca},P={pc},G3B={int(not flags & FLAG_G3_F32)}>"


class Cell(collections.namedtuple("Cell", "kind P D A flags")):
    """One cell of the dispatch.  kind: "wave" (fp32, below the switch: only the backward can loop there), "exact"
    (fp32 with FLAG_EXACT past the switch), "b6", "block", "gen4", "gen8", "wide"."""

    @property
    def cap(self):
        if self.kind == "wave":
            return BWD_BLOCKS
        return max(BWD_BLOCKS, FWD_CAP["wave" if self.kind == "exact" else self.kind])

    @property
    def N(self):
        return loop_n(self.P, self.cap)

    @property
    def id(self):
        return f"{self.kind}-P{self.P}-D{self.D}-A{self.A}-f{self.flags}"


def loop_n(P, cap):
    """2 cap + 5 units: every block takes two of them and five blocks three; then a remainder of 16 // P + 1 nodes:
    a full 16-row tile and a partial one (a single row at P = 1; P = 16 has no partial tiles, P > 16 one node)."""
    return (2 * cap + 5) * nodes_per_unit(P) + TILE // P + 1


CELLS = (
    [Cell("wave", P, 64, A, 0) for A in (64, 128) for P in POW2]
    + [Cell("exact", P, 64, A, FLAG_EXACT) for A in (64, 128) for P in POW2]
    + [Cell("b6", P, 64, A, 0) for A in (64, 128) for P in POW2]
    + [Cell("b6", 4, 64, 128, FLAG_G3_F32), Cell("b6", 16, 64, 64, FLAG_G3_F32),
       Cell("b6", 2, 64, 128, FLAG_PAIRS), Cell("b6", 8, 64, 128, FLAG_PAIRS)]
    + [Cell("block", 3, 64, 128, 0), Cell("block", 5, 64, 64, 0), Cell("block", 7, 64, 128, 0),
       Cell("block", 64, 64, 64, 0), Cell("block", 33, 64, 128, 0)]
    + [Cell("gen4", 4, 64, 192, 0), Cell("gen4", 3, 64, 256, 0), Cell("gen4", 16, 64, 256, 0)]
    + [Cell("gen8", 2, 128, 64, 0), Cell("gen8", 3, 128, 128, 0), Cell("gen8", 8, 128, 192, 0),
       Cell("gen8", 5, 128, 256, 0)]
    # the widest three with one or two nodes per chunk (36 .. 66 rows of 64): half the rows at the same number of chunks
    + [Cell("wide", 4, 192, 64, 0), Cell("wide", 3, 256, 128, 0), Cell("wide", 36, 320, 320, 0),
       Cell("wide", 22, 192, 384, 0), Cell("wide", 33, 256, 512, 0)]
)
# (P, N) pairs on both sides of the switch to the bf16 x 6 kernels, D = 64, A = 128 / 64, flags 0
SWITCH = [(1, 65535, 128), (1, 65536, 128), (16, 4095, 64), (16, 4096, 64)]
# one or two shapes per kernel family for the small-N, wide-range, poison and determinism tests
FAMILY_SHAPES = [(4, 64, 128), (16, 64, 64), (1, 64, 64), (3, 64, 128), (33, 64, 64), (3, 64, 256), (5, 128, 192),
                 (3, 192, 384), (8, 320, 128)]
SMALL_N = [1, 15, 16, 17, 63, 65]
# wide-range cases: the families at N = 257, the bf16-pipe kernels (flags 0 / G3_F32 / PAIRS) just past the switch
WIDE_RANGE = [(P, D, A, 257, 0) for (P, D, A) in FAMILY_SHAPES] + \
             [(8, 64, 128, 8200, 0), (8, 64, 128, 8200, FLAG_G3_F32), (8, 64, 128, 8200, FLAG_PAIRS), (2, 64, 64, 32800, 0)]


def small_ns(P):
    """SMALL_N, and for the chunked kernels the sizes around one chunk (64 mod P padding rows in a full chunk)."""
    nb = nodes_per_unit(P)
    return sorted(set(SMALL_N + ([nb, nb + 1, 2 * nb + 1] if P not in POW2 else [])))


# ------------------------------------------------------------------------------------------------ reference
def _fwd(M, W, b, uo):
    """M (n, P, D), W (D, A), b, uo (A,) in float64 -> everything of the forward with its bounds."""
    n, P, D = M.shape
    A = W.shape[1]
    aW, au = np.abs(W), np.abs(uo)
    r = types.SimpleNamespace(n=n, P=P, D=D, A=A)
    r.pre = pre = M @ W + b
    e_pre = (D + C_PRE) * U * (np.abs(M) @ aW + np.abs(b))
    apre = np.abs(pre)
    q = np.exp(-2.0 * apre)                  # tanh and sech^2 from one exponential, without cancellation in 1 - v^2
    av = (1.0 - q) / (1.0 + q)
    r.v = v = np.copysign(av, pre)
    r.g = g = 4.0 * q / (1.0 + q) ** 2
    c_t = g * (1 + 2 * apre) + 3 * (1 - v) + av
    assert e_pre.max() < 0.25                # e^(2x) <= 1 + 2x + 4x^2 there
    r.e_v = e_v = e_pre * g * (1 + 2 * e_pre + 4 * e_pre * e_pre) + c_t * U
    r.s = s = v @ uo
    r.e_s = e_s = e_v @ au + A * U * (av @ au)
    am = s.argmax(1)
    rows = np.arange(n)
    x = s - s[rows, am][:, None]
    ex = np.exp(x)
    r.beta = beta = ex / ex.sum(1, keepdims=True)
    E = e_s + e_s[rows, am][:, None]
    ax = np.abs(x)
    rho = np.expm1(E + (2 + 3 * ax) * U)
    rden = (beta * np.expm1(E + (4 * P + 3 * ax) * U)).sum(1, keepdims=True)
    assert (rden < 0.5).all()
    r.e_beta = beta * ((1 + rho) * (1 + 6 * U) / (1 - rden) - 1) + TINY
    rz = (1 + np.expm1(E + (4 * P + 1 + 3 * ax) * U)) * (1 + 6 * U) / (1 - rden) - 1
    aM = np.abs(M)
    r.Z = np.einsum("np,npd->nd", beta, M)
    r.e_Z = np.einsum("np,npd->nd", beta * rz + TINY, aM) + P * U * np.einsum("np,npd->nd", beta, aM)
    return r


def _bwd(r, M, W, uo, dZ, bt):
    """The backward for the rows of r (the forward of the same rows), from the GIVEN beta bt (n, P) in float64."""
    P, D, A = r.P, r.D, r.A
    aM, aW, au = np.abs(M), np.abs(W), np.abs(uo)
    v, av, g, e_v = r.v, np.abs(r.v), r.g, r.e_v
    dbeta = np.einsum("nd,npd->np", dZ, M)
    e_dbeta = D * U * np.einsum("nd,npd->np", np.abs(dZ), aM)
    c = (bt * dbeta).sum(1, keepdims=True)
    e_c = (bt * e_dbeta).sum(1, keepdims=True) + P * U * (bt * np.abs(dbeta)).sum(1, keepdims=True)
    r.ds = ds = bt * (dbeta - c)
    r.e_ds = e_ds = bt * (e_dbeta + e_c) * (1 + 2 * U) + 2 * U * np.abs(ds) + TINY
    e_g = 2 * av * e_v + e_v * e_v + 2 * U
    ads, eds = np.abs(ds)[:, :, None], e_ds[:, :, None]
    r.dpre = dpre = ds[:, :, None] * uo * g
    x1 = au * (eds * g + ads * e_g + eds * e_g)
    r.e_dpre = e_dpre = x1 * (1 + 2 * U) + 2 * U * np.abs(dpre) + TINY
    direct = bt[:, :, None] * dZ[:, None, :]
    r.dM = direct + dpre @ W.T
    r.e_dM = (e_dpre @ aW.T + (A + 1 + C_MM) * U * (np.abs(dpre) @ aW.T + np.abs(direct))
              + TINY * (1 + aW.sum(1)))
    r.dsv = ds[:, :, None] * v
    r.e_dsv = eds * av + ads * e_v + eds * e_v
    return r


def _f64(case):
    return up(case["w"]), up(case["b"]), up(case["u"])


@functools.lru_cache(maxsize=8)
def small_ref(kind, N, P, D, A, flags=0):
    """(case, reference from the reference's own beta) of make_case(...), cached; for the small cases of the host tests."""
    case = make_case(kind, N, P, D, A, flags)
    return case, sem_ref(case)


@functools.lru_cache(maxsize=4)
def cached_case(kind, N, P, D, A, flags=0):
    """make_case(...), cached: the tests of one cell share the inputs (read-only)."""
    return make_case(kind, N, P, D, A, flags)


def sem_ref(case, beta_in=None, nodes=None):
    """The whole reference at once (small cases, or the rows `nodes` of a large one): the forward, and the backward
    from beta_in (default: the reference's own beta, for the comparison with autograd).  dW / db / du sum over the
    given rows with T = the live ones among them."""
    W, b, uo = _f64(case)
    sel = slice(None) if nodes is None else np.asarray(nodes)
    M, dZ = up(case["M"][sel]), up(case["dZ"][sel])
    r = _fwd(M, W, b, uo)
    bt = r.beta if beta_in is None else up(np.asarray(beta_in)[sel])
    _bwd(r, M, W, uo, dZ, bt)
    live = (dZ != 0).any(1)
    r.live = live
    r.T = T = int(live.sum())
    n, P, D = M.shape
    Mf, aMf = M.reshape(n * P, D), np.abs(M).reshape(n * P, D)
    dp, e_dp = r.dpre.reshape(n * P, -1), np.where(live[:, None, None], r.e_dpre, 0.0).reshape(n * P, -1)
    r.dW = Mf.T @ dp
    r.e_dW = aMf.T @ e_dp + (T * P + C_MM) * U * (aMf.T @ np.abs(dp))
    r.db = dp.sum(0)
    r.e_db = e_dp.sum(0) + T * P * U * np.abs(dp).sum(0)
    r.du = r.dsv.sum((0, 1))
    r.e_du = np.where(live[:, None, None], r.e_dsv, 0.0).sum((0, 1)) + (T * P + 1) * U * np.abs(r.dsv).sum((0, 1))
    return r


def _blocks(N, P, A):
    step = max(1, (1 << 21) // (P * A))
    return [(lo, min(N, lo + step)) for lo in range(0, N, step)]


def dense_ratios(case, Z, beta, dM=None, grads=None):
    """err / bound of Z, beta, the row sums of beta and (for the first len(dM) nodes) dM over EVERY row, computed block
    by block so that the float64 intermediates of a 130 000-row case never exist at once.  The backward starts from the
    given beta.  grads = (dW, db, du) of a backward over all N nodes adds their ratios (T = the live nodes)."""
    W, b, uo = _f64(case)
    N, P, D = case["M"].shape
    A = W.shape[1]
    out = {"Z": 0.0, "beta": 0.0, "sum_beta": 0.0}
    nb = 0 if dM is None else dM.shape[0]
    if nb:
        out["dM"] = 0.0
    assert grads is None or nb == N
    acc = [np.zeros((D, A)), np.zeros((D, A)), np.zeros((D, A)), np.zeros(A), np.zeros(A), np.zeros(A), np.zeros(A),
           np.zeros(A), np.zeros(A)]
    for lo, hi in _blocks(N, P, A):
        M = up(case["M"][lo:hi])
        r = _fwd(M, W, b, uo)
        out["Z"] = max(out["Z"], ratio(Z[lo:hi], r.Z, r.e_Z))
        out["beta"] = max(out["beta"], ratio(beta[lo:hi], r.beta, r.e_beta))
        out["sum_beta"] = max(out["sum_beta"], ratio(np.asarray(beta[lo:hi], dtype=np.float64).sum(1), 1.0, r.e_beta.sum(1)))
        if lo < nb:
            h2 = min(hi, nb)
            k = h2 - lo
            rb = _fwd(M[:k], W, b, uo) if k < hi - lo else r
            dZ = up(case["dZ"][lo:h2])
            _bwd(rb, M[:k], W, uo, dZ, up(beta[lo:h2]))
            out["dM"] = max(out["dM"], ratio(dM[lo:h2], rb.dM, rb.e_dM))
            if grads is not None:
                live = (dZ != 0).any(1)[:, None, None]
                Mf, aMf = M[:k].reshape(k * P, D), np.abs(M[:k]).reshape(k * P, D)
                dp, e_dp = rb.dpre.reshape(k * P, A), np.where(live, rb.e_dpre, 0.0).reshape(k * P, A)
                for i, x in enumerate((Mf.T @ dp, aMf.T @ e_dp, aMf.T @ np.abs(dp), dp.sum(0), e_dp.sum(0),
                                       np.abs(dp).sum(0), rb.dsv.sum((0, 1)), np.where(live, rb.e_dsv, 0.0).sum((0, 1)),
                                       np.abs(rb.dsv).sum((0, 1)))):
                    acc[i] += x
    if grads is not None:
        TP = int((case["dZ"] != 0).any(1).sum()) * P
        out["dW"] = ratio(grads[0], acc[0], acc[1] + (TP + C_MM) * U * acc[2])
        out["db"] = ratio(grads[1], acc[3], acc[4] + TP * U * acc[5])
        out["du"] = ratio(grads[2], acc[6], acc[7] + (TP + 1) * U * acc[8])
    return out


def planted_ratios(case, ref, Z, beta, dM, dW, db, du, live):
    """err / bound of a planted case: ref = sem_ref(case, beta, nodes=live)."""
    return {"Z": ratio(Z[live], ref.Z, ref.e_Z), "beta": ratio(beta[live], ref.beta, ref.e_beta),
            "dM": ratio(dM[live], ref.dM, ref.e_dM), "dW": ratio(dW, ref.dW, ref.e_dW),
            "db": ratio(db, ref.db, ref.e_db), "du": ratio(du, ref.du, ref.e_du)}


# ------------------------------------------------------------------------------------------------ inputs
N_RANDOM_LIVE = 8
KINDS = {"dense": 0, "planted": 1, "wide_range": 2}


def _draw(N, P, D, A, kind, w_scale, u_scale):
    rng = np.random.default_rng([P, D, A, N, KINDS[kind]])
    M = rng.standard_normal((N, P, D), dtype=np.float32)
    w = (rng.standard_normal((D, A)) * (w_scale / math.sqrt(D))).astype(np.float32)
    b = (rng.standard_normal(A) * 0.1).astype(np.float32)
    u = (rng.standard_normal(A) * (u_scale / math.sqrt(A))).astype(np.float32)
    return rng, dict(M=M, w=w, b=b, u=u)


def dense_case(N, P, D, A):
    """Every node live.  w_omega ~ 1 / sqrt(D) and u_omega ~ 2 / sqrt(A): pre is O(1), the scores have a standard
    deviation near 1 and the softmax is not saturated (the host test asserts it)."""
    rng, case = _draw(N, P, D, A, "dense", 1.0, 2.0)
    case["dZ"] = rng.standard_normal((N, D), dtype=np.float32)
    return case


def planted_positions(N, P, D, A, flags):
    """The nodes where a kernel can go wrong, from the forward and the backward grid of the cell: node 0 and N - 1; the
    first and the last node of the units 0 (block 0, first iteration), grid - 1 (last block, first iteration), grid
    (block 0, second iteration), 2 grid - 1, 2 grid and of the last unit; the first node of the last full 16-row tile
    (the partial tile holds node N - 1); one node in each 16-lane group of a tile (P <= 16); the last node of a chunk,
    next to its padding rows, and the first of the next one (P not a power of two)."""
    npu = nodes_per_unit(P)
    units, gf, gb = grids(N, P, D, A, flags)
    nodes = {0, N - 1}
    for grid in (gf, gb):
        for unit in (0, grid - 1, grid, 2 * grid - 1, 2 * grid, units - 1):
            if 0 <= unit < units:
                nodes |= {unit * npu, min((unit + 1) * npu, N) - 1}
    full = (N * P) // TILE
    if full:
        nodes.add(((full - 1) * TILE) // P)
    if P <= TILE:
        nodes |= {(ROWS + TILE + 4 * g) // P for g in range(4)}
    if P not in POW2:
        nodes |= {2 * npu - 1, 2 * npu}
    return sorted(n for n in nodes if 0 <= n < N)


def planted_case(N, P, D, A, flags=0, positions=None):
    """dZ is zero except on the planted nodes and N_RANDOM_LIVE random ones (at most 64 in all).  u_omega ~ 1 / sqrt(A):
    hardly any node is saturated, so every live node carries weight in dW, db and du (the host test asserts it)."""
    rng, case = _draw(N, P, D, A, "planted", 1.0, 1.0)
    pos = planted_positions(N, P, D, A, flags) if positions is None else list(positions)
    extra = rng.permutation(N)[:N_RANDOM_LIVE]
    live = np.unique(np.concatenate([np.asarray(pos, dtype=np.int64), extra]))
    assert live.size <= 64
    dZ = np.zeros((N, D), dtype=np.float32)
    dZ[live] = rng.standard_normal((live.size, D), dtype=np.float32)
    if P > 1:       # dbeta_0 - dbeta_1 is about D / 4 +- sqrt(2 D): no live node with an accidentally tiny ds
        dZ[live] += np.float32(0.25) * (case["M"][live, 0] - case["M"][live, 1])
    case["dZ"] = dZ
    case["live"] = live
    return case


def wide_range_case(N, P, D, A):
    """pre ~ N(0, 4^2): most |v| are near 1, and u_omega is scaled so that the largest |score| is 80: losing beta
    underflow, 1 - v^2 cancels.  Every node is live."""
    rng, case = _draw(N, P, D, A, "wide_range", 4.0, 2.0)
    W, b, uo = _f64(case)
    s = np.tanh(up(case["M"]) @ W + b) @ uo
    case["u"] = (case["u"] * np.float32(80.0 / np.abs(s).max())).astype(np.float32)
    case["dZ"] = rng.standard_normal((N, D), dtype=np.float32)
    return case


def make_case(kind, N, P, D, A, flags=0):
    if kind == "dense":
        return dense_case(N, P, D, A)
    if kind == "planted":
        return planted_case(N, P, D, A, flags)
    return wide_range_case(N, P, D, A)
