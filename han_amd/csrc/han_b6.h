// The "bf16 x 6" toolkit of the matrix-pipe kernels (K1: project.hip, K3: sem_attn.hip).
//
// An fp32 number splits EXACTLY into three bf16 terms by truncation, x = hi + mid + lo (8 + 8 + 8
// significand bits; every subtraction below is exact).  With both operands split, the six products
//     hi*hi' + hi*mid' + mid*hi' + hi*lo' + lo*hi' + mid*mid'
// (each bf16 x bf16 product is exact in the fp32 accumulator) leave out only mid*lo', lo*mid', lo*lo':
// < 2^-23 of |x w| per term, the size of an fp32 rounding -- against 6 MFMAs of
// v_mfma_f32_16x16x32_bf16 (16 cycles each, K = 32) where the exact-fp32 pipe needs 8
// v_mfma_f32_16x16x4_f32 of 32 cycles: 2.7x less matrix time.
#pragma once
#include "han_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float float2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));      // a bf16x8 MFMA operand as four packed pairs

// x == h + m + l exactly; each term has <= 8 significand bits (its low 16 bits are zero)
__device__ __forceinline__ void han_b6_split(float x, uint32_t &h, uint32_t &m, uint32_t &l) {
    h = __float_as_uint(x) & 0xFFFF0000u;
    const float r1 = x - __uint_as_float(h);
    m = __float_as_uint(r1) & 0xFFFF0000u;
    l = __float_as_uint(r1 - __uint_as_float(m));
}
// two truncated terms -> one packed bf16 pair (element 0 in the low half)
__device__ __forceinline__ uint32_t han_b6_pack(uint32_t e0, uint32_t e1) {
    return __builtin_amdgcn_perm(e1, e0, 0x07060302u);
}
// 8 consecutive floats -> the three packed bf16x8 fragments.  Two values at a time: the two subtractions of the
// split are packed (v_pk_add_f32), 4.5 instead of 5.5 vector instructions per value.
__device__ __forceinline__ void han_b6_split8(const float (&v)[8], i32x4 &fh, i32x4 &fm, i32x4 &fl) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float2_t x = {v[2 * q], v[2 * q + 1]};
        const u32x2 hb = __builtin_bit_cast(u32x2, x) & 0xFFFF0000u;
        const float2_t r1 = x - __builtin_bit_cast(float2_t, hb);
        const u32x2 mb = __builtin_bit_cast(u32x2, r1) & 0xFFFF0000u;
        const u32x2 lb = __builtin_bit_cast(u32x2, r1 - __builtin_bit_cast(float2_t, mb));
        fh[q] = (int)han_b6_pack(hb[0], hb[1]);
        fm[q] = (int)han_b6_pack(mb[0], mb[1]);
        fl[q] = (int)han_b6_pack(lb[0], lb[1]);
    }
}
// the same into f[0] = h, f[1] = m, f[2] = l, from an array or from the two 16-byte halves of an octet
__device__ __forceinline__ void han_b6_split8(const float (&v)[8], i32x4 (&f)[3]) { han_b6_split8(v, f[0], f[1], f[2]); }
__device__ __forceinline__ void han_b6_split8(const float4_t &lo, const float4_t &hi, i32x4 (&f)[3]) {
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    han_b6_split8(v, f[0], f[1], f[2]);
}

__device__ __forceinline__ f32x4 han_b6_mfma(const i32x4 &a, const i32x4 &b, const f32x4 &c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                   0, 0, 0);
}

// The six-product chains, small terms first; a / b = the (h, m, l) fragments of the A / B operand.  TWO summation
// orders exist and fp32 accumulation is not associative: each order is pinned by bitwise equality of its kernels'
// results with what they have always produced, not by taste.  Do not "unify" them.
//
// K1 order: (m,m) (l,h) (m,h) (h,l) (h,m) (h,h).  XBF: a bf16 A operand is its own high term -- `a` holds one
// fragment and the three products with the (zero) m / l terms are left out.
template <bool XBF>
__device__ __forceinline__ f32x4 han_b6_chain_k1(const i32x4 *a, const i32x4 &bh, const i32x4 &bm, const i32x4 &bl,
                                                 f32x4 c) {
    if (!XBF) {
        c = han_b6_mfma(a[1], bm, c);
        c = han_b6_mfma(a[2], bh, c);
        c = han_b6_mfma(a[1], bh, c);
    }
    c = han_b6_mfma(a[0], bl, c);
    c = han_b6_mfma(a[0], bm, c);
    c = han_b6_mfma(a[0], bh, c);
    return c;
}
// K3 order: (m,m) (l,h) (h,l) (m,h) (h,m) (h,h).
__device__ __forceinline__ f32x4 han_b6_chain_k3(const i32x4 (&a)[3], const i32x4 (&b)[3], f32x4 c) {
    c = han_b6_mfma(a[1], b[1], c);
    c = han_b6_mfma(a[2], b[0], c);
    c = han_b6_mfma(a[0], b[2], c);
    c = han_b6_mfma(a[1], b[0], c);
    c = han_b6_mfma(a[0], b[1], c);
    c = han_b6_mfma(a[0], b[0], c);
    return c;
}
