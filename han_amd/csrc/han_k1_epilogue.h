// K1 -- the stored-row contract of the projection forward kernels (project.hip, project_sparse.hip), written once.
// Whatever computed a row of H, it leaves the kernel the same way (utils/layers.py:23-24, 31-32):
//   1. the element is scaled by 1/keep of the input dropout (the kernel's own: it knows whether it drew any);
//   2. it is rounded to bf16 (nearest even) if the table is bf16;
//   3. with projected-row dropout (thr_fts < 2^16) its keep bit replaces the LOWEST mantissa bit of the STORED element
//      (fp32 bit 0 / bf16 bit 0): stream fts_stream = 2 + 4 * slice, counter (row + row_offset, d / 4), field d % 4.
//      K2 reads the bit while it gathers, the backward redraws it;
//   4. it is stored;
//   5. f1 = H_k . a1_k + b1_k and f2 likewise are taken from the row AS STORED.
// Two lane layouts reach this point: the tile form (C/D layout of a 16x16 MFMA tile: a lane holds (row, 16 t + l15),
// t < 4) and the row form (lane q of a 16-lane group holds the columns 4q .. 4q+3 of a row).  Where the helpers are cut,
// and where a caller keeps a loop of its own, is what leaves every kernel's resources as they were (tools/kernel_diff.py;
// profiles/r14_k1_epilogue_dropped_steps.txt has the cuts that did not).
#pragma once
#include "han_common.h"

// What the epilogue of one table reads: the base of ProjFwdArgs and SparseFwdArgs, the argument of
// project_scores_kernel; the fused multi-path kernel fills the scores half per meta-path.
struct K1Epilogue {
    void *H;                // fp32 or bf16 (h_bf16), 64 elements per row
    int h_bf16;
    int64_t N;
    const float *a1, *a2, *b1, *b2;
    float *f1, *f2;         // null f1: this kernel takes no scores
    uint32_t seed_lo, seed_hi;
    const uint64_t *seed_dev;
    uint32_t thr_fts;       // < 2^16: stamp keep bits into H
    uint32_t fts_stream;    // HAN_STREAM_FTS + 4 * slice (HAN_FLAG_FTS_SLICE: slices of a wide head)
    int64_t row_offset;
};

// --------------------------------------------------------------------------------------------- the tile form
// steps 2-4 for the raw value v of (row, 16 t + l15), t after t in the caller's loop; returns the value as stored
__device__ __forceinline__ float k1_store_elem(const K1Epilogue &e, int64_t row, int t, int l15, float v) {
    uint32_t keepbit = 0, stamp = 0;
    if (e.thr_fts < HAN_KEEP_ALL) {
        const int d = 16 * t + l15;
        const HanRand64 rn = han_rand64(e.seed_lo, e.seed_hi, e.fts_stream, (uint32_t)(row + e.row_offset), (uint32_t)(d >> 2));
        keepbit = rn.field(d & 3) < e.thr_fts ? 1u : 0u;
        stamp = 1;
    }
    if (e.h_bf16) {
        uint32_t b = han_f32_to_bf16_bits(v);
        if (stamp) b = (b & ~1u) | keepbit;
        if (row < e.N) reinterpret_cast<uint16_t *>(e.H)[row * HAN_D + 16 * t + l15] = (uint16_t)b;
        return __uint_as_float(b << 16);
    }
    if (stamp) v = __uint_as_float((__float_as_uint(v) & ~1u) | keepbit);
    if (row < e.N) reinterpret_cast<float *>(e.H)[row * HAN_D + 16 * t + l15] = v;
    return v;
}

// this lane's score vector elements of the columns (16 t + l15)
__device__ __forceinline__ void k1_tile_coeffs(const K1Epilogue &e, int l15, float (&a1c)[4], float (&a2c)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        a1c[t] = e.a1[16 * t + l15];
        a2c[t] = e.a2[16 * t + l15];
    }
}

// f1 = H_k . a1_k + b1_k, f2 likewise, for the row whose stored elements (row, 16t + l15), t < 4, this lane
// holds in vst[]: the F' columns of a head sit in min(F',16) consecutive lanes of a 16-lane group and in
// max(1, F'/16) column tiles.  Epilogue code (once per output element), not a hot loop.
template <int FP>
__device__ __forceinline__ void tile_scores(const K1Epilogue &a, int64_t row, bool row_ok, const float (&vst)[4],
                                            const float (&a1c)[4], const float (&a2c)[4], int l15) {
    constexpr int K = HAN_D / FP;
    constexpr int NT = FP >= 16 ? FP / 16 : 1;       // column tiles per head
    constexpr int NL = FP >= 16 ? 16 : FP;           // lanes per head inside a tile
    float r1[4 / NT], r2[4 / NT];
#pragma unroll
    for (int u = 0; u < 4 / NT; ++u) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int t = u * NT; t < (u + 1) * NT; ++t) {
            s1 += vst[t] * a1c[t];
            s2 += vst[t] * a2c[t];
        }
        // butterfly over the head's NL lanes on DPP operands (bitwise the __shfl_xor butterfly, without its 3-4
        // ds_bpermute round trips per sum: the fused eval kernel issued 1024 of them per wave)
        if (NL > 1) { s1 += han_dpp_xor16<1>(s1); s2 += han_dpp_xor16<1>(s2); }
        if (NL > 2) { s1 += han_dpp_xor16<2>(s1); s2 += han_dpp_xor16<2>(s2); }
        if (NL > 4) { s1 += han_dpp_xor16<4>(s1); s2 += han_dpp_xor16<4>(s2); }
        if (NL > 8) { s1 += han_dpp_xor16<8>(s1); s2 += han_dpp_xor16<8>(s2); }
        r1[u] = s1;
        r2[u] = s2;
    }
    if (FP == 8) {
        // lanes 0 / 8 of the group hold heads 2u / 2u+1: bring the odd heads over and let lane 0 write the
        // row's 8 scores as two 16-byte stores (16 scattered 4-byte stores per row cost as much as the
        // separate scores kernel they replaced)
        float4_t o1[2], o2[2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float e1 = han_dpp_xor16<8>(r1[u]), e2 = han_dpp_xor16<8>(r2[u]);
            o1[u >> 1][2 * (u & 1)] = r1[u] + a.b1[2 * u];
            o1[u >> 1][2 * (u & 1) + 1] = e1 + a.b1[2 * u + 1];
            o2[u >> 1][2 * (u & 1)] = r2[u] + a.b2[2 * u];
            o2[u >> 1][2 * (u & 1) + 1] = e2 + a.b2[2 * u + 1];
        }
        if (row_ok && l15 == 0) {
            float4_t *p1 = reinterpret_cast<float4_t *>(a.f1 + row * K), *p2 = reinterpret_cast<float4_t *>(a.f2 + row * K);
            p1[0] = o1[0]; p1[1] = o1[1];
            p2[0] = o2[0]; p2[1] = o2[1];
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < 4 / NT; ++u) {
        const int head = FP >= 16 ? u : (16 * u + l15) / FP;
        if (row_ok && (l15 % NL) == 0) {
            a.f1[row * K + head] = r1[u] + a.b1[head];
            a.f2[row * K + head] = r2[u] + a.b2[head];
        }
    }
}

// --------------------------------------------------------------------------------------------- the row form
// Steps 2-4 for a lane's columns c = 4q .. 4q+3 of `row` (d = 4q + i -> counter d / 4 = q, field i): the row's four
// draws; element i rounded and stamped (the CALLER loops over i: a loop in here is unrolled before it is inlined, and
// the kernels come out with other registers); the row, as stored, written by the lanes the caller picks.
__device__ __forceinline__ HanRand64 k1_row_draws(const K1Epilogue &e, int64_t row, int q) {
    HanRand64 rn = {0u, 0u};
    if (e.thr_fts < HAN_KEEP_ALL) rn = han_rand64(e.seed_lo, e.seed_hi, e.fts_stream, (uint32_t)(row + e.row_offset), (uint32_t)q);
    return rn;
}

template <bool BF>
__device__ __forceinline__ float4_t k1_row_stamp(const K1Epilogue &e, const HanRand64 &rn, float4_t v, int i) {
    const uint32_t keepbit = rn.field(i) < e.thr_fts ? 1u : 0u;
    if (BF) {
        uint32_t b = han_f32_to_bf16_bits(v[i]);
        if (e.thr_fts < HAN_KEEP_ALL) b = (b & ~1u) | keepbit;
        v[i] = __uint_as_float(b << 16);          // the value as stored (what the scores see)
    } else if (e.thr_fts < HAN_KEEP_ALL) {
        v[i] = __uint_as_float((__float_as_uint(v[i]) & ~1u) | keepbit);
    }
    return v;
}

template <bool BF>
__device__ __forceinline__ void k1_row_store(const K1Epilogue &e, int64_t row, int c, const float4_t &v) {
    if (BF) {      // already rounded: pack the high halves
        uint2 w;
        w.x = (__float_as_uint(v[0]) >> 16) | (__float_as_uint(v[1]) & 0xFFFF0000u);
        w.y = (__float_as_uint(v[2]) >> 16) | (__float_as_uint(v[3]) & 0xFFFF0000u);
        *reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(e.H) + row * 64 + c) = w;
    } else {
        *reinterpret_cast<float4_t *>(reinterpret_cast<float *>(e.H) + row * 64 + c) = v;
    }
}

// step 5: this lane's elements of a1 / a2 ...
__device__ __forceinline__ void k1_row_coeffs(const K1Epilogue &e, int c, float4_t &a14, float4_t &a24) {
    a14 = *reinterpret_cast<const float4_t *>(e.a1 + c);
    a24 = *reinterpret_cast<const float4_t *>(e.a2 + c);
}

// ... and H_k . a1_k, H_k . a2_k of the head the lane's columns lie in (F' >= 4): its four products, then the __shfl_xor
// butterfly over the head's F'/4 lanes, all of which must be here.  Lane (4q) % F' == 0 writes f[row * K + 4q / F'] = s + b.
template <int FP>
__device__ __forceinline__ void k1_row_scores(float4_t v, float4_t a14, float4_t a24, float &s1, float &s2) {
    s1 = v[0] * a14[0] + v[1] * a14[1] + v[2] * a14[2] + v[3] * a14[3];
    s2 = v[0] * a24[0] + v[1] * a24[1] + v[2] * a24[2] + v[3] * a24[3];
#pragma unroll
    for (int o = 1; o < FP / 4; o <<= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
}

// --------------------------------------------------------------------------------------------- host
static inline bool han_k1_dtype(int code) { return code == HAN_DTYPE_F32 || code == HAN_DTYPE_BF16; }
// the parameter, output and keep-table pointers of one meta-path
struct K1Path { const float *W, *a1, *a2, *b1, *b2; void *H; float *f1, *f2; uint8_t *keep; };

// The checks han_project_fwd, han_project_fwd_multi and han_project_sparse_fwd share, in the order all three make
// them (each returns 0 for N == 0 before).  `x`: the input's own pointer (X / rowptr); `layout_ok` / `n_ok`: the entry
// point's own conditions on the input's layout (HAN_E_BADARG) and on the row count (HAN_E_UNSUPPORTED).
static inline int han_k1_check_fwd(const void *x, const K1Path &q, int64_t N, int F, bool layout_ok, bool n_ok, int K,
                                   int FP, int x_dtype, int table_dtype, float in_drop, float fts_drop) {
    if (!x || !q.W || !q.a1 || !q.a2 || !q.b1 || !q.b2 || !q.H || !q.f1 || !q.f2 || N < 0 || F <= 0 || !layout_ok)
        return HAN_E_BADARG;
    if (!n_ok) return HAN_E_UNSUPPORTED;
    if (!han_fp_supported(K, FP)) return HAN_E_UNSUPPORTED;
    if (!han_k1_dtype(x_dtype) || !han_k1_dtype(table_dtype)) return HAN_E_UNSUPPORTED;
    if (in_drop < 0.f || in_drop >= 1.f || fts_drop < 0.f || fts_drop >= 1.f) return HAN_E_BADARG;
    return 0;
}

// the epilogue of meta-path q; `scores` false: f1 / f2 are not taken by the kernel that gets it
static inline K1Epilogue han_k1_epilogue(const K1Path &q, bool scores, int table_dtype, int64_t N, uint64_t seed,
                                         const uint64_t *seed_dev, float fts_drop, int flags, int64_t row_offset) {
    K1Epilogue e;
    e.H = q.H; e.h_bf16 = table_dtype == HAN_DTYPE_BF16; e.N = N;
    e.a1 = q.a1; e.a2 = q.a2; e.b1 = q.b1; e.b2 = q.b2; e.f1 = scores ? q.f1 : nullptr; e.f2 = scores ? q.f2 : nullptr;
    e.seed_lo = (uint32_t)seed; e.seed_hi = (uint32_t)(seed >> 32); e.seed_dev = seed_dev;
    e.thr_fts = han_drop_threshold(fts_drop);
    e.fts_stream = HAN_STREAM_FTS + 4u * (uint32_t)HAN_FLAG_FTS_SLICE_OF(flags);
    e.row_offset = row_offset;
    return e;
}
