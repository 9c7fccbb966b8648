// K1 sparse -- the first-layer projection of a CSR feature matrix (bag-of-words rows: ACM 1870 columns, DBLP 334,
// almost all zero), forward and dW (gfx950).
//
// Reference arithmetic: utils/layers.py:18-24,31-32, exactly as project.hip computes it.  Input dropout multiplies
// elements (layers.py:18-19), so a zero stays a zero whatever its draw: visiting only the stored entries and
// regenerating their draws -- counter (global row, f * ceil(K/4) + k/4), field k % 4 -- gives the dense kernels'
// numbers up to the order of the fp32 sums.
//
// Lane map (the short-row kernels of node_attn.hip): a wave owns one output row (forward: row n of H; dW: feature f);
// its four 16-lane groups each take every fourth stored entry, lane q of a group the columns 4q .. 4q+3 of the
// gathered 256-B row (W[colidx[e]] / dH[rowidx[e]]: one 16-byte load per lane, a whole row per group).  With
// F' >= 4 a lane's four columns lie in one head: one hash and one 16-bit field per lane and entry.  A batch of 64
// entries brings its indices in with one coalesced load, and four steps are issued back to back, so a wave has 16
// row gathers in flight (sparse_gather_sum).  The four groups' partial rows are added in a fixed order at the end:
// bitwise reproducible, no atomics.
#include "han_k1_epilogue.h"

namespace {

// the stored-row half (han_k1_epilogue.h) plus the CSR triple and the input dropout
struct SparseFwdArgs : K1Epilogue {
    const int64_t *rowptr;
    const int32_t *colidx;
    const float *vals;      // null: every stored entry is 1
    const float *W;
    uint32_t thr_in;        // input dropout (its seed is the epilogue's)
    float inv_keep_in;
};

// sum_e vals[e] * keep(.) * table[idx[e]][4q .. 4q+3] over the entries [beg, end) of one output row, for the whole
// wave (beg / end are wave-uniform; every lane returns the total of its four columns).  FWD: idx[e] is the feature
// (the hash's b counter), `fixed` the global row; dW: idx[e] is the row (the a counter), `fixed` the feature.
// The entries go by in batches of 64: ONE coalesced load brings the batch's indices (and values) into the wave, a
// lane per entry; group g then takes the entries 4j + g, whose index it reads from lane 4j + g, four j at a time --
// the addresses of a round's four row gathers are known before the first of them is issued, so 16 rows per wave are
// in flight and a row of R entries costs about 1 + R/16 memory round trips.  (The first form walked the entries
// with a dependent index load -> row load pair per trip: 2 R/4 round trips, and at the ACM shape -- 36 entries per
// row -- the training forward's waves spent 11 k cycles where 3 k were work: profiles/r12_k1_sparse_first_form.jsonl.)
template <int FP, bool DROP, bool FWD>
__device__ __forceinline__ float4_t sparse_gather_sum(const int32_t *idx, const float *vals, const float *table,
                                                      int64_t beg, int64_t end, int lane, uint32_t seed_lo,
                                                      uint32_t seed_hi, uint32_t thr_in, uint32_t fixed, int64_t row_offset) {
    constexpr int K = HAN_D / FP;
    constexpr int KQ = (K + 3) / 4;      // one RNG call = four 16-bit draws = four heads
    const int g = lane >> 4, q = lane & 15;
    const int head = (4 * q) / FP;       // F' >= 4: a lane's four columns lie in one head
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t base = beg; base < end; base += 64) {
        const int cnt = end - base < 64 ? (int)(end - base) : 64;
        int32_t my_i = 0;
        float my_v = 0.f;                // entries beyond the batch: index 0 (a row that exists), value 0
        if (lane < cnt) {
            my_i = idx[base + lane];
            my_v = vals ? vals[base + lane] : 1.f;
        }
#pragma unroll
        for (int j0 = 0; j0 < 16; j0 += 4) {
            if (4 * j0 >= cnt) break;    // wave-uniform
            int32_t ii[4];
            float vv[4];
            float4_t tt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int src = 4 * (j0 + u) + g;
                ii[u] = __shfl(my_i, src, 64);
                vv[u] = __shfl(my_v, src, 64);
                tt[u] = han_load_row4<false>(table, ii[u], q);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float v = vv[u];
                if (DROP) {
                    const uint32_t a = FWD ? fixed : (uint32_t)(ii[u] + row_offset);
                    const uint32_t b = (FWD ? (uint32_t)ii[u] : fixed) * (uint32_t)KQ + (uint32_t)(head >> 2);
                    const HanRand64 rn = han_rand64(seed_lo, seed_hi, HAN_STREAM_SEQ, a, b);
                    v = rn.field(head & 3) < thr_in ? v : 0.f;
                }
                const bool live = 4 * (j0 + u) + g < cnt;      // (a slot beyond the batch adds nothing, whatever row 0 holds)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = live ? fmaf(v, tt[u][c], acc[c]) : acc[c];
            }
        }
    }
    float4_t s;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float v = acc[c];
        v += __shfl_xor(v, 16, 64);      // (g0 + g1), (g2 + g3): the same bits in both partners
        v += __shfl_xor(v, 32, 64);
        s[c] = v;
    }
    return s;
}

// one wave per row; scale, then the row form of han_k1_epilogue.h (lane group 0 stores)
template <int FP, bool BF, bool DROP>
__global__ __launch_bounds__(256) void project_sparse_fwd_kernel(const SparseFwdArgs a_in) {
    SparseFwdArgs a = a_in;
    han_resolve_seed(a.seed_lo, a.seed_hi, a.seed_dev);
    constexpr int K = HAN_D / FP;
    const int lane = threadIdx.x & 63, g = lane >> 4, q = lane & 15;
    const int head = (4 * q) / FP;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.N) return;      // wave-uniform
    float4_t v = sparse_gather_sum<FP, DROP, true>(a.colidx, a.vals, a.W, a.rowptr[row], a.rowptr[row + 1], lane,
                                                   a.seed_lo, a.seed_hi, a.thr_in, (uint32_t)(row + a.row_offset), 0);
    if (DROP) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= a.inv_keep_in;
    }
    const HanRand64 rn = k1_row_draws(a, row, q);
#pragma unroll
    for (int i = 0; i < 4; ++i) v = k1_row_stamp<BF>(a, rn, v, i);
    if (g == 0) k1_row_store<BF>(a, row, 4 * q, v);
    float4_t a14, a24;
    k1_row_coeffs(a, 4 * q, a14, a24);
    float s1, s2;
    k1_row_scores<FP>(v, a14, a24, s1, s2);      // the whole wave is here: the in-head shuffles are safe
    if (g == 0 && (4 * q) % FP == 0) {
        a.f1[row * K + head] = s1 + a.b1[head];
        a.f2[row * K + head] = s2 + a.b2[head];
    }
}

struct SparseBwdArgs {
    const int64_t *colptr;
    const int32_t *rowidx;
    const float *vals_t;    // null: every stored entry is 1
    const int32_t *chunk_col;                 // per chunk: its (long) column
    const int64_t *chunk_start, *chunk_end;   // per chunk: its entries [start, end) of rowidx / vals_t
    const int32_t *long_cols;                 // the columns longer than col_chunk, ascending
    const int64_t *long_ptr;                  // (n_long + 1): chunks [long_ptr[i], long_ptr[i+1]) belong to long_cols[i]
    const float *dH;
    float *dW;
    float *partial;         // (n_chunks, 64): the chunks' raw sums
    int F;
    int64_t n_chunks, n_long, col_chunk;
    uint32_t seed_lo, seed_hi, thr_in;
    const uint64_t *seed_dev;
    float inv_keep_in;
    int64_t row_offset;
};

// wave w < F: column w, written straight to dW unless it is a long one (left to its chunks); wave F + c: chunk c of
// a long column, raw sum to partial[c]
template <int FP, bool DROP>
__global__ __launch_bounds__(256) void project_sparse_bwd_kernel(const SparseBwdArgs a_in) {
    SparseBwdArgs a = a_in;
    han_resolve_seed(a.seed_lo, a.seed_hi, a.seed_dev);
    const int lane = threadIdx.x & 63, g = lane >> 4, q = lane & 15;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.F + a.n_chunks) return;      // wave-uniform
    int64_t beg, end;
    int f;
    float *out;
    float scale;
    if (w < a.F) {
        f = (int)w;
        beg = a.colptr[f]; end = a.colptr[f + 1];
        if (end - beg > a.col_chunk) return;
        out = a.dW + (int64_t)f * HAN_D;
        scale = DROP ? a.inv_keep_in : 1.f;
    } else {
        const int64_t c = w - a.F;
        f = a.chunk_col[c];
        beg = a.chunk_start[c]; end = a.chunk_end[c];
        out = a.partial + c * HAN_D;
        scale = 1.f;
    }
    float4_t v = sparse_gather_sum<FP, DROP, false>(a.rowidx, a.vals_t, a.dH, beg, end, lane, a.seed_lo, a.seed_hi,
                                                    a.thr_in, (uint32_t)f, a.row_offset);
    if (g == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= scale;
        *reinterpret_cast<float4_t *>(out + 4 * q) = v;
    }
}

// a 16-lane group per long column: its chunks' partial rows in ascending chunk order
__global__ __launch_bounds__(256) void project_sparse_merge_kernel(const SparseBwdArgs a) {
    const int q = threadIdx.x & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (i >= a.n_long) return;
    float4_t s = {0.f, 0.f, 0.f, 0.f};
    const int64_t c1 = a.long_ptr[i + 1];
    for (int64_t c = a.long_ptr[i]; c < c1; c += 8) {      // eight loads ahead; the additions keep the chunk order
        float4_t p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            p[u] = *reinterpret_cast<const float4_t *>(a.partial + (c + u < c1 ? c + u : c1 - 1) * HAN_D + 4 * q);
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += c + u < c1 ? p[u][e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] *= a.inv_keep_in;
    *reinterpret_cast<float4_t *>(a.dW + (int64_t)a.long_cols[i] * HAN_D + 4 * q) = s;
}

}  // namespace

extern "C" int han_project_sparse_fwd(const int64_t *rowptr, const int32_t *colidx, const float *vals, const float *W,
                                      const float *a1, const float *a2, const float *b1, const float *b2, void *H,
                                      int table_dtype, float *f1, float *f2, int64_t N, int F, int K, int FP,
                                      float in_drop, float fts_drop, uint64_t seed, const uint64_t *seed_dev,
                                      int64_t row_offset, int flags, void *stream) {
    if (N == 0) return 0;   // nothing to do; pointers of empty tensors may be null
    // (a matrix without entries may carry a null colidx; the values are fp32)
    const K1Path q = {W, a1, a2, b1, b2, H, f1, f2, nullptr};
    const int bad = han_k1_check_fwd(rowptr, q, N, F, true, N < ((int64_t)1 << 31), K, FP, HAN_DTYPE_F32, table_dtype,
                                     in_drop, fts_drop);
    if (bad != 0) return bad;
    SparseFwdArgs a;
    static_cast<K1Epilogue &>(a) = han_k1_epilogue(q, true, table_dtype, N, seed, seed_dev, fts_drop, flags, row_offset);
    a.rowptr = rowptr; a.colidx = colidx; a.vals = vals; a.W = W;
    a.thr_in = han_drop_threshold(in_drop); a.inv_keep_in = 1.f / (1.f - in_drop);
    const unsigned grid = (unsigned)((N + 3) / 4);
    const bool bf = table_dtype == HAN_DTYPE_BF16;
    HAN_DISPATCH_BOOL(DROP, in_drop > 0.f, HAN_DISPATCH_FP_BF(FP, bf,
        project_sparse_fwd_kernel<FPC, BF, DROP><<<grid, 256, 0, (hipStream_t)stream>>>(a)));
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t han_project_sparse_bwd_workspace(int64_t n_chunks) {
    return n_chunks > 0 ? (size_t)n_chunks * HAN_D * sizeof(float) : 0;
}

extern "C" int han_project_sparse_bwd(const int64_t *colptr, const int32_t *rowidx, const float *vals_t,
                                      int64_t col_chunk, int64_t n_long, int64_t n_chunks, const int32_t *long_cols,
                                      const int64_t *long_ptr, const int32_t *chunk_col, const int64_t *chunk_start,
                                      const int64_t *chunk_end, const float *dH, float *dW, void *workspace,
                                      size_t workspace_bytes, int64_t N, int F, int K, int FP, float in_drop,
                                      uint64_t seed, const uint64_t *seed_dev, int64_t row_offset, void *stream) {
    if (!colptr || !dW || N < 0 || F <= 0 || col_chunk < 1 || n_long < 0 || n_chunks < n_long) return HAN_E_BADARG;
    if (N > 0 && !dH) return HAN_E_BADARG;
    if (n_long > 0 && (!long_cols || !long_ptr || !chunk_col || !chunk_start || !chunk_end)) return HAN_E_BADARG;
    if (N >= ((int64_t)1 << 31)) return HAN_E_UNSUPPORTED;
    if (!han_fp_supported(K, FP)) return HAN_E_UNSUPPORTED;
    if (in_drop < 0.f || in_drop >= 1.f) return HAN_E_BADARG;
    if (n_chunks > 0 && (!workspace || workspace_bytes < han_project_sparse_bwd_workspace(n_chunks))) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    SparseBwdArgs a;
    a.colptr = colptr; a.rowidx = rowidx; a.vals_t = vals_t;
    a.chunk_col = chunk_col; a.chunk_start = chunk_start; a.chunk_end = chunk_end;
    a.long_cols = long_cols; a.long_ptr = long_ptr;
    a.dH = dH; a.dW = dW; a.partial = (float *)workspace; a.F = F;
    a.n_chunks = n_chunks; a.n_long = n_long; a.col_chunk = col_chunk;
    han_set_dropout(a, seed, seed_dev, in_drop, a.thr_in, a.inv_keep_in);
    a.row_offset = row_offset;
    // N == 0 runs too: every feature is without entries and dW gets its zero rows (the caller may overwrite a
    // gradient buffer with dW, so every row is written on every call)
    const unsigned grid = (unsigned)(((int64_t)F + n_chunks + 3) / 4);
    HAN_DISPATCH_FP(FP, HAN_DISPATCH_BOOL(DROP, in_drop > 0.f,
        project_sparse_bwd_kernel<FPC, DROP><<<grid, 256, 0, st>>>(a)))
    HAN_CHECK_LAUNCH();
    if (n_long > 0) {
        project_sparse_merge_kernel<<<(unsigned)((n_long + 15) / 16), 256, 0, st>>>(a);
        HAN_CHECK_LAUNCH();
    }
    return 0;
}
