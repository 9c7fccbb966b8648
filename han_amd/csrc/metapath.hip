// K0: meta-path graphs from typed relations -- the boolean sparse-sparse product C = A B of two CSR graphs
// (entry (i, j) of C present iff some l has (i, l) in A and (l, j) in B), in two passes over the same expansion:
// count (unique columns per row), then -- after the caller's scan of the counts into c_rowptr -- fill.
// No buffer of the size of the expansion exists: every candidate column is produced, used and dropped inside
// one workgroup, so the extra device memory is the caller's O(rows + nnz(C)).
//
// Rows are binned by their bound ub_i = sum over l in A_i of deg_B(l) (+ 1 with HAN_SPGEMM_DIAG):
//   short rows (ub <= short_max): one wave per row.  The candidates are staged in LDS (slots from a scan over the
//       B-row lengths), sorted by a bitonic network sized to the next power of two of ub, and the first of every
//       run of equal columns is counted / written.
//   long rows: one 256-thread workgroup per row.  An LDS bit map over a tile of tile_cols columns, set with LDS
//       atomicOr; count = popcount, fill = a block scan of the per-thread popcounts, every thread then emits the set
//       bits of its own contiguous words in ascending order.  A column space wider than one tile is swept tile by
//       tile and the row's candidates are re-read for every tile: a long row costs ub x ceil(n_cols / tile_cols)
//       candidate reads.
// Both forms write sorted, unique columns, so the output does not depend on scheduling (bitwise deterministic).
// Offsets (row pointers, bounds, output positions) are int64 throughout.
#include "han_common.h"

namespace {

constexpr int kBoundsBlock = 256;    // 16 lanes per row
constexpr int kBoundsCap = 8192;
constexpr int kShortCap = 8192;      // persistent grids: blocks stride over the binned row list
constexpr int kLongBlock = 256;
constexpr int kLongCap = 1024;

struct SpgemmArgs {
    const int64_t *a_rowptr;
    const int32_t *a_colidx;
    const int64_t *b_rowptr;
    const int32_t *b_colidx;
    int64_t n_rows, n_mid, n_cols;
    const int32_t *rows;             // every row id once, the *n_long long rows first
    const int64_t *n_long;           // device word
    int stage_cap;                   // LDS staging entries of the short kernel (a power of two >= short_max)
    int64_t tile_cols;               // columns per bit-map tile of the long kernel (a multiple of 32)
    int diag;
    int64_t *counts;                 // count pass
    const int64_t *c_rowptr;         // fill pass
    int32_t *c_colidx;
};

// ub_i: a 16-lane group per row
__global__ __launch_bounds__(kBoundsBlock) void spgemm_row_bounds(const int64_t *__restrict__ a_rowptr,
                                                                  const int32_t *__restrict__ a_colidx,
                                                                  const int64_t *__restrict__ b_rowptr,
                                                                  int64_t n_rows, int64_t n_mid, int64_t extra,
                                                                  int64_t *__restrict__ ub) {
    const int q = threadIdx.x & 15;
    for (int64_t i = ((int64_t)blockIdx.x * kBoundsBlock + threadIdx.x) >> 4; i < n_rows;
         i += (int64_t)gridDim.x * (kBoundsBlock / 16)) {
        const int64_t a1 = a_rowptr[i + 1];
        int64_t s = 0;
        for (int64_t e = a_rowptr[i] + q; e < a1; e += 16) {
            const int32_t l = a_colidx[e];
            if ((uint64_t)l < (uint64_t)n_mid) s += b_rowptr[l + 1] - b_rowptr[l];
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
        if (q == 0) ub[i] = s + extra;
    }
}

// Calls f(p, c) for every candidate column c of `row` (one call per product, repeats included; p = the candidate's
// position in A-row order) spread over the G threads of the block -- G consecutive A entries at a time: an
// inclusive scan of their B-row lengths in LDS, then thread t takes positions t, t + G, ... of the chunk and finds
// its A entry by a binary search over the scan (balanced whatever the B-row lengths).  Returns the candidate count.
// Every thread of the block must call it (it synchronises).
template <int G, typename F>
__device__ __forceinline__ int64_t for_each_candidate(const SpgemmArgs &a, int64_t row, int64_t *s_off,
                                                      int64_t *s_beg, F &&f) {
    const int t = threadIdx.x;
    const int64_t a0 = a.a_rowptr[row], a1 = a.a_rowptr[row + 1];
    int64_t base = 0;
    for (int64_t c0 = a0; c0 < a1; c0 += G) {
        int64_t deg = 0, beg = 0;
        if (c0 + t < a1) {
            const int32_t l = a.a_colidx[c0 + t];
            if ((uint64_t)l < (uint64_t)a.n_mid) {
                beg = a.b_rowptr[l];
                deg = a.b_rowptr[l + 1] - beg;
            }
        }
        if (t == 0) s_off[0] = 0;
        s_off[t + 1] = deg;
        s_beg[t] = beg;
        __syncthreads();
#pragma unroll
        for (int d = 1; d < G; d <<= 1) {
            const int64_t v = t >= d ? s_off[t + 1 - d] : 0;
            __syncthreads();
            s_off[t + 1] += v;
            __syncthreads();
        }
        const int64_t total = s_off[G];
        for (int64_t p = t; p < total; p += G) {
            int lo = 0, hi = G;      // s_off[lo] <= p < s_off[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid] <= p) lo = mid;
                else hi = mid;
            }
            f(base + p, a.b_colidx[s_beg[lo] + (p - s_off[lo])]);
        }
        base += total;
        __syncthreads();         // s_off / s_beg are rewritten by the next chunk
    }
    return base;
}

template <bool FILL>
__device__ __forceinline__ void spgemm_short_rows(const SpgemmArgs &a) {
    extern __shared__ int32_t stage[];         // a.stage_cap entries
    __shared__ int64_t s_off[65], s_beg[64];
    const int t = threadIdx.x;
    const int cap = a.stage_cap;
    for (int64_t r = *a.n_long + blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const int64_t row = a.rows[r];
        int64_t nc = for_each_candidate<64>(a, row, s_off, s_beg, [&](int64_t p, int32_t c) {
            if (p < cap) stage[p] = c;
        });
        if (a.diag) {
            if (t == 0 && nc < cap) stage[nc] = (int32_t)row;
            ++nc;
        }
        const int n = nc < cap ? (int)nc : cap;      // (nc <= cap always: the caller bins by the same bound)
        int64_t cnt = 0;
        if (n > 0) {
            int P = 64;
            while (P < n) P <<= 1;
            for (int p = n + t; p < P; p += 64) stage[p] = INT32_MAX;     // pads sort last
            __syncthreads();
            for (int k = 2; k <= P; k <<= 1) {
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int q = t; q < (P >> 1); q += 64) {
                        const int lo = 2 * q - (q & (j - 1)), hi = lo + j;
                        const int32_t x = stage[lo], y = stage[hi];
                        if ((x > y) == ((lo & k) == 0)) {
                            stage[lo] = y;
                            stage[hi] = x;
                        }
                    }
                    __syncthreads();
                }
            }
            const int64_t base = FILL ? a.c_rowptr[row] : 0, end = FILL ? a.c_rowptr[row + 1] : 0;
            for (int p0 = 0; p0 < n; p0 += 64) {
                const int p = p0 + t;
                int32_t v = 0;
                bool head = false;
                if (p < n) {
                    v = stage[p];
                    head = p == 0 || stage[p - 1] != v;
                }
                const uint64_t m = __ballot(head);
                if (FILL && head) {
                    const int64_t pos = base + cnt + __popcll(m & ((1ull << t) - 1ull));
                    if (pos < end) a.c_colidx[pos] = v;
                }
                cnt += __popcll(m);
            }
        }
        if (!FILL && t == 0) a.counts[row] = cnt;
        __syncthreads();                 // the stage is rewritten by the next row
    }
}

// exclusive scan of v over the 256 threads of the block (every thread also gets the total)
__device__ __forceinline__ int block_excl_scan256(int v, int *s_wave, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[w] = x;
    __syncthreads();
    int pre = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kLongBlock / 64; ++k) {
        pre += k < w ? s_wave[k] : 0;
        total += s_wave[k];
    }
    __syncthreads();
    return pre + x - v;
}

template <bool FILL>
__device__ __forceinline__ void spgemm_long_rows(const SpgemmArgs &a) {
    extern __shared__ uint32_t bits[];         // min(tile_cols, n_cols rounded up to 32) / 32 words
    __shared__ int64_t s_off[kLongBlock + 1], s_beg[kLongBlock];
    __shared__ int s_wave[kLongBlock / 64];
    const int t = threadIdx.x;
    const int64_t n_long = *a.n_long;
    for (int64_t r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int64_t row = a.rows[r];
        const int64_t base = FILL ? a.c_rowptr[row] : 0, end = FILL ? a.c_rowptr[row + 1] : 0;
        int64_t total = 0;
        for (int64_t lo = 0; lo < a.n_cols; lo += a.tile_cols) {
            const int64_t width = a.n_cols - lo < a.tile_cols ? a.n_cols - lo : a.tile_cols;
            const int W = (int)((width + 31) >> 5);
            for (int w = t; w < W; w += kLongBlock) bits[w] = 0u;
            __syncthreads();
            for_each_candidate<kLongBlock>(a, row, s_off, s_beg, [&](int64_t, int32_t c) {
                const int64_t off = (int64_t)c - lo;
                if (off >= 0 && off < width) atomicOr(&bits[off >> 5], 1u << (off & 31));
            });
            if (a.diag && t == 0) {
                const int64_t off = row - lo;
                if (off >= 0 && off < width) atomicOr(&bits[off >> 5], 1u << (off & 31));
            }
            __syncthreads();
            const int wpt = (W + kLongBlock - 1) / kLongBlock;         // thread t owns words [w0, w1)
            const int w0 = t * wpt < W ? t * wpt : W, w1 = w0 + wpt < W ? w0 + wpt : W;
            int mine = 0;
            for (int w = w0; w < w1; ++w) mine += __popc(bits[w]);
            int tile_total;
            const int excl = block_excl_scan256(mine, s_wave, tile_total);
            if (FILL) {
                int64_t pos = base + total + excl;
                for (int w = w0; w < w1; ++w) {
                    uint32_t b = bits[w];
                    while (b) {
                        const int k = __ffs(b) - 1;
                        b &= b - 1u;
                        if (pos < end) a.c_colidx[pos] = (int32_t)(lo + 32 * (int64_t)w + k);
                        ++pos;
                    }
                }
            }
            total += tile_total;
            __syncthreads();             // the bit map is cleared for the next tile / row
        }
        if (!FILL && t == 0) a.counts[row] = total;
    }
}

__global__ __launch_bounds__(64) void spgemm_short_count(SpgemmArgs a) { spgemm_short_rows<false>(a); }
__global__ __launch_bounds__(64) void spgemm_short_fill(SpgemmArgs a) { spgemm_short_rows<true>(a); }
__global__ __launch_bounds__(kLongBlock) void spgemm_long_count(SpgemmArgs a) { spgemm_long_rows<false>(a); }
__global__ __launch_bounds__(kLongBlock) void spgemm_long_fill(SpgemmArgs a) { spgemm_long_rows<true>(a); }

int spgemm_launch(bool fill, const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                  const int32_t *b_colidx, int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t *rows,
                  const int64_t *n_long, int64_t short_max, int64_t tile_cols, int flags, int64_t *counts,
                  const int64_t *c_rowptr, int32_t *c_colidx, void *stream) {
    if (!a_rowptr || !b_rowptr || !rows || !n_long || n_rows < 0 || n_mid < 0 || n_cols < 0) return HAN_E_BADARG;
    if (fill ? !c_rowptr : !counts) return HAN_E_BADARG;
    if (short_max < 0 || short_max > HAN_SPGEMM_MAX_SHORT || tile_cols < 32 || tile_cols % 32 != 0 ||
        tile_cols > HAN_SPGEMM_MAX_TILE)
        return HAN_E_BADARG;
    if ((flags & HAN_SPGEMM_DIAG) && n_rows != n_cols) return HAN_E_BADARG;
    if (n_rows == 0) return 0;
    SpgemmArgs a;
    a.a_rowptr = a_rowptr; a.a_colidx = a_colidx; a.b_rowptr = b_rowptr; a.b_colidx = b_colidx;
    a.n_rows = n_rows; a.n_mid = n_mid; a.n_cols = n_cols;
    a.rows = rows; a.n_long = n_long;
    int cap = 64;
    while (cap < short_max) cap <<= 1;
    a.stage_cap = cap;
    a.tile_cols = tile_cols;
    a.diag = (flags & HAN_SPGEMM_DIAG) ? 1 : 0;
    a.counts = counts; a.c_rowptr = c_rowptr; a.c_colidx = c_colidx;
    hipStream_t st = (hipStream_t)stream;
    const int64_t bm_cols = n_cols < tile_cols ? (n_cols + 31) / 32 * 32 : tile_cols;
    const size_t bm_bytes = (size_t)(bm_cols > 0 ? bm_cols : 32) / 8;
    const unsigned g_long = (unsigned)(n_rows < kLongCap ? n_rows : kLongCap);
    const unsigned g_short = (unsigned)(n_rows < kShortCap ? n_rows : kShortCap);
    hipError_t e = han_launch_lds(fill ? spgemm_long_fill : spgemm_long_count, dim3(g_long), dim3(kLongBlock),
                                  bm_bytes, st, a);
    if (e != hipSuccess) return (int)e;
    e = han_launch_lds(fill ? spgemm_short_fill : spgemm_short_count, dim3(g_short), dim3(64),
                       (size_t)cap * sizeof(int32_t), st, a);
    if (e != hipSuccess) return (int)e;
    return 0;
}

}  // namespace

extern "C" int han_spgemm_row_bounds(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                                     int64_t n_rows, int64_t n_mid, int flags, int64_t *ub, void *stream) {
    if (!a_rowptr || !b_rowptr || !ub || n_rows < 0 || n_mid < 0) return HAN_E_BADARG;
    if (n_rows == 0) return 0;
    spgemm_row_bounds<<<han_grid_for(n_rows, kBoundsBlock / 16, kBoundsCap), kBoundsBlock, 0, (hipStream_t)stream>>>(
        a_rowptr, a_colidx, b_rowptr, n_rows, n_mid, (flags & HAN_SPGEMM_DIAG) ? 1 : 0, ub);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_spgemm_count(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                                const int32_t *b_colidx, int64_t n_rows, int64_t n_mid, int64_t n_cols,
                                const int32_t *rows, const int64_t *n_long, int64_t short_max, int64_t tile_cols,
                                int flags, int64_t *counts, void *stream) {
    return spgemm_launch(false, a_rowptr, a_colidx, b_rowptr, b_colidx, n_rows, n_mid, n_cols, rows, n_long,
                         short_max, tile_cols, flags, counts, nullptr, nullptr, stream);
}

extern "C" int han_spgemm_fill(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                               const int32_t *b_colidx, int64_t n_rows, int64_t n_mid, int64_t n_cols,
                               const int32_t *rows, const int64_t *n_long, int64_t short_max, int64_t tile_cols,
                               int flags, const int64_t *c_rowptr, int32_t *c_colidx, void *stream) {
    return spgemm_launch(true, a_rowptr, a_colidx, b_rowptr, b_colidx, n_rows, n_mid, n_cols, rows, n_long,
                         short_max, tile_cols, flags, nullptr, c_rowptr, c_colidx, stream);
}
