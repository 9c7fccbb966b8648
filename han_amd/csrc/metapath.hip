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
// Weighted graphs (further down): the int64 instance counts of C in one more pass over the same bins, PathSim of a
// counted graph, and the per-row top-k cut of a graph with values.
// Sampled neighbours (the last section): meta-path-guided random walks instead of the product, a wave per start row.
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

// Calls f(p, ea, eb) for every product of `row` (repeats included; p = the product's position in A-row order, ea / eb
// the entries of A and B it joins) spread over the G threads of the block -- G consecutive A entries at a time: an
// inclusive scan of their B-row lengths in LDS, then thread t takes positions t, t + G, ... of the chunk and finds
// its A entry by a binary search over the scan (balanced whatever the B-row lengths).  Returns the product count.
// Every thread of the block must call it (it synchronises).
template <int G, typename F>
__device__ __forceinline__ int64_t for_each_product(const SpgemmArgs &a, int64_t row, int64_t *s_off,
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
            f(base + p, c0 + lo, s_beg[lo] + (p - s_off[lo]));
        }
        base += total;
        __syncthreads();         // s_off / s_beg are rewritten by the next chunk
    }
    return base;
}

// f(p, c) for every candidate column c of `row`: the column of every product
template <int G, typename F>
__device__ __forceinline__ int64_t for_each_candidate(const SpgemmArgs &a, int64_t row, int64_t *s_off,
                                                      int64_t *s_beg, F &&f) {
    return for_each_product<G>(a, row, s_off, s_beg, [&](int64_t p, int64_t, int64_t eb) { f(p, a.b_colidx[eb]); });
}

// ascending bitonic sort of the P (a power of two >= 64) LDS entries of `stage` by one wave (a 64-thread block); the
// entries must be visible (a barrier after the last write) and are when it returns
template <typename T>
__device__ __forceinline__ void bitonic_sort_wave(T *stage, int P) {
    const int t = threadIdx.x;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = t; q < (P >> 1); q += 64) {
                const int lo = 2 * q - (q & (j - 1)), hi = lo + j;
                const T x = stage[lo], y = stage[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    stage[lo] = y;
                    stage[hi] = x;
                }
            }
            __syncthreads();
        }
    }
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
            bitonic_sort_wave(stage, P);
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

// exclusive scan of v over the G threads of the block (every thread also gets the total)
template <int G>
__device__ __forceinline__ int block_excl_scan(int v, int *s_wave, int &total) {
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
    for (int k = 0; k < G / 64; ++k) {
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
            const int excl = block_excl_scan<kLongBlock>(mine, s_wave, tile_total);
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

// checks the arguments that count, fill and values share and sets them in `a` (0, or HAN_E_BADARG)
int spgemm_args(SpgemmArgs &a, const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                const int32_t *b_colidx, int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t *rows,
                const int64_t *n_long, int64_t short_max, int64_t tile_cols, int flags) {
    if (!a_rowptr || !b_rowptr || !rows || !n_long || n_rows < 0 || n_mid < 0 || n_cols < 0) return HAN_E_BADARG;
    if (short_max < 0 || short_max > HAN_SPGEMM_MAX_SHORT || tile_cols < 32 || tile_cols % 32 != 0 ||
        tile_cols > HAN_SPGEMM_MAX_TILE)
        return HAN_E_BADARG;
    if ((flags & HAN_SPGEMM_DIAG) && n_rows != n_cols) return HAN_E_BADARG;
    a.a_rowptr = a_rowptr; a.a_colidx = a_colidx; a.b_rowptr = b_rowptr; a.b_colidx = b_colidx;
    a.n_rows = n_rows; a.n_mid = n_mid; a.n_cols = n_cols;
    a.rows = rows; a.n_long = n_long;
    int cap = 64;
    while (cap < short_max) cap <<= 1;
    a.stage_cap = cap;
    a.tile_cols = tile_cols;
    a.diag = (flags & HAN_SPGEMM_DIAG) ? 1 : 0;
    return 0;
}

size_t spgemm_bitmap_bytes(int64_t n_cols, int64_t tile_cols) {
    const int64_t bm_cols = n_cols < tile_cols ? (n_cols + 31) / 32 * 32 : tile_cols;
    return (size_t)(bm_cols > 0 ? bm_cols : 32) / 8;
}

unsigned spgemm_grid(int64_t n_rows, int cap) { return (unsigned)(n_rows < cap ? n_rows : cap); }

int spgemm_launch(bool fill, const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                  const int32_t *b_colidx, int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t *rows,
                  const int64_t *n_long, int64_t short_max, int64_t tile_cols, int flags, int64_t *counts,
                  const int64_t *c_rowptr, int32_t *c_colidx, void *stream) {
    SpgemmArgs a;
    const int rc = spgemm_args(a, a_rowptr, a_colidx, b_rowptr, b_colidx, n_rows, n_mid, n_cols, rows, n_long,
                               short_max, tile_cols, flags);
    if (rc != 0) return rc;
    if (fill ? !c_rowptr : !counts) return HAN_E_BADARG;
    if (n_rows == 0) return 0;
    a.counts = counts; a.c_rowptr = c_rowptr; a.c_colidx = c_colidx;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = han_launch_lds(fill ? spgemm_long_fill : spgemm_long_count, dim3(spgemm_grid(n_rows, kLongCap)),
                                  dim3(kLongBlock), spgemm_bitmap_bytes(n_cols, tile_cols), st, a);
    if (e != hipSuccess) return (int)e;
    e = han_launch_lds(fill ? spgemm_short_fill : spgemm_short_count, dim3(spgemm_grid(n_rows, kShortCap)), dim3(64),
                       (size_t)a.stage_cap * sizeof(int32_t), st, a);
    if (e != hipSuccess) return (int)e;
    return 0;
}

// ---- the counted product: one values pass over the finished structure of C ------------------------------------------
// c_ij = sum over the products of row i that land on column j of a_val x b_val (1 where an operand has no values),
// int64, integer adds only: the sum does not depend on the order of the adds, so the result is bitwise reproducible.
// The columns of C are known (han_spgemm_fill), so no candidate is sorted again:
//   short rows: the wave copies the row of C into LDS beside one int64 accumulator per entry; every product finds its
//       entry by a binary search over those columns and is added with an LDS atomic; the accumulators are then stored.
//   long rows: the bit map of the tile is set from the row of C (not from the candidates), per-word prefix popcounts are
//       computed once per tile, and a product on column c goes to the global slot c_rowptr[row] + (entries of the
//       earlier tiles) + (set bits below c) with a 64-bit atomic add -- only this workgroup touches the row.
// c_vals is cleared by the entry point (a memset on the stream): an entry without a product (the added diagonal) is 0.
struct SpgemmValArgs {
    SpgemmArgs g;                    // (g.c_colidx is only read here)
    const int64_t *a_vals, *b_vals;  // NULL: every stored entry is 1
    int64_t *c_vals;
};

__device__ __forceinline__ int64_t product_value(const SpgemmValArgs &v, int64_t ea, int64_t eb) {
    return (v.a_vals ? v.a_vals[ea] : 1) * (v.b_vals ? v.b_vals[eb] : 1);
}

__global__ __launch_bounds__(64) void spgemm_short_values(SpgemmValArgs v) {
    extern __shared__ int64_t acc[];           // stage_cap accumulators, then stage_cap columns
    __shared__ int64_t s_off[65], s_beg[64];
    const SpgemmArgs &a = v.g;
    const int t = threadIdx.x;
    const int cap = a.stage_cap;
    int32_t *cols = reinterpret_cast<int32_t *>(acc + cap);
    for (int64_t r = *a.n_long + blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const int64_t row = a.rows[r];
        const int64_t base = a.c_rowptr[row], len = a.c_rowptr[row + 1] - base;
        if (len <= 0 || len > cap) continue;   // (len <= ub <= cap when C was filled under the same bins)
        const int n = (int)len;
        for (int p = t; p < n; p += 64) {
            cols[p] = a.c_colidx[base + p];
            acc[p] = 0;
        }
        __syncthreads();
        for_each_product<64>(a, row, s_off, s_beg, [&](int64_t, int64_t ea, int64_t eb) {
            const int32_t c = a.b_colidx[eb];
            int lo = 0, hi = n;                // first position with cols[pos] >= c
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cols[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < n && cols[lo] == c)
                atomicAdd(reinterpret_cast<unsigned long long *>(&acc[lo]), (unsigned long long)product_value(v, ea, eb));
        });
        for (int p = t; p < n; p += 64) v.c_vals[base + p] = acc[p];     // (for_each_product ends on a barrier)
        __syncthreads();                       // cols / acc are rewritten by the next row
    }
}

__global__ __launch_bounds__(kLongBlock) void spgemm_long_values(SpgemmValArgs v) {
    extern __shared__ uint32_t bits[];         // W words of the tile's bit map, then W prefix popcounts
    __shared__ int64_t s_off[kLongBlock + 1], s_beg[kLongBlock];
    __shared__ int s_wave[kLongBlock / 64];
    const SpgemmArgs &a = v.g;
    const int t = threadIdx.x;
    const int64_t n_long = *a.n_long;
    const int64_t tile_w = ((a.n_cols < a.tile_cols ? a.n_cols : a.tile_cols) + 31) >> 5;
    uint32_t *pre = bits + (tile_w > 0 ? tile_w : 1);
    for (int64_t r = blockIdx.x; r < n_long; r += gridDim.x) {
        const int64_t row = a.rows[r];
        const int64_t base = a.c_rowptr[row], end = a.c_rowptr[row + 1];
        int64_t total = 0;                     // entries of the row in the tiles before this one
        for (int64_t lo = 0; lo < a.n_cols && base + total < end; lo += a.tile_cols) {
            const int64_t width = a.n_cols - lo < a.tile_cols ? a.n_cols - lo : a.tile_cols;
            const int W = (int)((width + 31) >> 5);
            for (int w = t; w < W; w += kLongBlock) bits[w] = 0u;
            __syncthreads();
            for (int64_t e = base + total + t; e < end; e += kLongBlock) {     // ascending: the tile's entries come first
                const int64_t off = (int64_t)a.c_colidx[e] - lo;
                if (off >= width) break;
                if (off >= 0) atomicOr(&bits[off >> 5], 1u << (off & 31));
            }
            __syncthreads();
            const int wpt = (W + kLongBlock - 1) / kLongBlock;         // thread t owns words [w0, w1)
            const int w0 = t * wpt < W ? t * wpt : W, w1 = w0 + wpt < W ? w0 + wpt : W;
            int mine = 0;
            for (int w = w0; w < w1; ++w) mine += __popc(bits[w]);
            int tile_total;
            int below = block_excl_scan<kLongBlock>(mine, s_wave, tile_total);
            for (int w = w0; w < w1; ++w) {
                pre[w] = (uint32_t)below;
                below += __popc(bits[w]);
            }
            __syncthreads();
            if (tile_total > 0) {
                const int64_t tile_base = base + total;
                for_each_product<kLongBlock>(a, row, s_off, s_beg, [&](int64_t, int64_t ea, int64_t eb) {
                    const int64_t off = (int64_t)a.b_colidx[eb] - lo;
                    if (off < 0 || off >= width) return;
                    const uint32_t word = bits[off >> 5], bit = 1u << (off & 31);
                    if (!(word & bit)) return;                         // (not a column of C: a foreign structure)
                    const int64_t pos = tile_base + pre[off >> 5] + __popc(word & (bit - 1u));
                    if (pos < end)
                        atomicAdd(reinterpret_cast<unsigned long long *>(&v.c_vals[pos]),
                                  (unsigned long long)product_value(v, ea, eb));
                });
            }
            total += tile_total;
            __syncthreads();             // the bit map is cleared for the next tile / row
        }
    }
}

// ---- PathSim ---------------------------------------------------------------------------------------------------------
constexpr int kRowBlock = 256;       // a wave per row, four rows per block
constexpr int kRowCap = 8192;

// diag[i] = the count of (i, i), 0 when row i does not hold it: a binary search over the row's ascending columns,
// a thread per row
__global__ __launch_bounds__(kRowBlock) void pathsim_diag(const int64_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ colidx,
                                                          const int64_t *__restrict__ counts, int64_t n,
                                                          int64_t *__restrict__ diag) {
    for (int64_t i = (int64_t)blockIdx.x * kRowBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRowBlock) {
        int64_t lo = rowptr[i], hi = rowptr[i + 1];
        const int64_t end = hi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)colidx[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        diag[i] = (lo < end && (int64_t)colidx[lo] == i) ? counts[lo] : 0;
    }
}

// w_ij = 2 c_ij / (c_ii + c_jj) in double, stored as fp32; w_ii = 1
__global__ __launch_bounds__(kRowBlock) void pathsim_values(const int64_t *__restrict__ rowptr,
                                                            const int32_t *__restrict__ colidx,
                                                            const int64_t *__restrict__ counts, int64_t n,
                                                            const int64_t *__restrict__ diag, float *__restrict__ w) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = ((int64_t)blockIdx.x * kRowBlock + threadIdx.x) >> 6; i < n;
         i += (int64_t)gridDim.x * (kRowBlock / 64)) {
        const int64_t e1 = rowptr[i + 1], dii = diag[i];
        for (int64_t e = rowptr[i] + lane; e < e1; e += 64) {
            const int64_t j = colidx[e];
            float x = 1.0f;
            if (j != i) {
                const int64_t djj = (uint64_t)j < (uint64_t)n ? diag[j] : 0;
                x = (float)(2.0 * (double)counts[e] / (double)(dii + djj));
            }
            w[e] = x;
        }
    }
}

// ---- per-row top-k ---------------------------------------------------------------------------------------------------
// The usual monotone map of fp32 bits to unsigned: a < b (as finite floats) iff ord(a) < ord(b); -0 sorts below +0.
__device__ __forceinline__ uint32_t float_ord(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// 16 lanes per row: counts[i] = min(k, entries off the diagonal) + (keep_diag ? entries on it : 0)
__global__ __launch_bounds__(kBoundsBlock) void topk_count(const int64_t *__restrict__ rowptr,
                                                           const int32_t *__restrict__ colidx, int64_t n, int64_t k,
                                                           int keep_diag, int64_t *__restrict__ counts) {
    const int q = threadIdx.x & 15;
    for (int64_t i = ((int64_t)blockIdx.x * kBoundsBlock + threadIdx.x) >> 4; i < n;
         i += (int64_t)gridDim.x * (kBoundsBlock / 16)) {
        const int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
        int64_t nd = 0;
        for (int64_t e = e0 + q; e < e1; e += 16) nd += (int64_t)colidx[e] == i;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) nd += __shfl_xor(nd, o, 16);
        const int64_t off = e1 - e0 - nd;
        if (q == 0) counts[i] = (off < k ? off : k) + (keep_diag ? nd : 0);
    }
}

constexpr int kTopkWaveMax = 2048;   // rows up to this many entries: a wave each; longer rows: a 256-thread workgroup

// One row per block of G threads (G = 64 takes the rows of at most kTopkWaveMax entries, G = 256 the others; each launch
// strides over every row and skips those of the other).  A row with more than k entries off the diagonal is decided by
// the k-th largest ord among them: an MSB-first radix select, 8 bits per round, over a 256-bin LDS histogram finds that
// value `thr` and how many of the entries equal to it are still needed; one pass in column order then keeps the
// entries above thr and the first `need` entries equal to thr -- with ascending columns, the ties of smaller column.
template <int G>
__device__ __forceinline__ void topk_fill_rows(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                               const float *__restrict__ vals, int64_t n, int64_t k, int keep_diag,
                                               const int64_t *__restrict__ o_rowptr, int32_t *__restrict__ o_colidx,
                                               float *__restrict__ o_vals) {
    __shared__ int hist[256];
    __shared__ int s_wave[G / 64];
    __shared__ int s_sel[2];
    const int t = threadIdx.x;
    constexpr int B = 256 / G;                 // histogram bins per thread, taken from the top
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t e0 = rowptr[i], e1 = rowptr[i + 1];
        if (e1 <= e0 || ((e1 - e0 > kTopkWaveMax) != (G > 64))) continue;
        int nd = 0;
        for (int64_t e = e0 + t; e < e1; e += G) nd += (int64_t)colidx[e] == i;
        int nd_total;
        block_excl_scan<G>(nd, s_wave, nd_total);
        uint32_t thr = 0u;
        int64_t need = 0;
        const bool cut = e1 - e0 - nd_total > k;
        if (cut) {
            uint32_t mask = 0u;
            need = k;
            for (int shift = 24; shift >= 0; shift -= 8) {
                for (int b = t; b < 256; b += G) hist[b] = 0;
                __syncthreads();
                for (int64_t e = e0 + t; e < e1; e += G) {
                    const uint32_t o = float_ord(vals[e]);
                    if ((int64_t)colidx[e] != i && (o & mask) == thr) atomicAdd(&hist[(o >> shift) & 255u], 1);
                }
                __syncthreads();
                int mine = 0;                  // thread t owns the digits 255 - t B, ..., 255 - t B - (B - 1)
#pragma unroll
                for (int q = 0; q < B; ++q) mine += hist[255 - (t * B + q)];
                int all;
                const int above = block_excl_scan<G>(mine, s_wave, all);
                if (above < need && need <= (int64_t)above + mine) {          // exactly one thread
                    int64_t left = need - above;
                    int d = 255 - t * B;
                    while (hist[d] < left) left -= hist[d--];
                    s_sel[0] = d;
                    s_sel[1] = (int)left;
                }
                __syncthreads();
                thr |= (uint32_t)s_sel[0] << shift;
                mask |= 255u << shift;
                need = s_sel[1];
                __syncthreads();             // hist / s_sel are rewritten by the next round
            }
        }
        const int64_t o_end = o_rowptr[i + 1];
        int64_t pos = o_rowptr[i], ties = 0;
        for (int64_t c0 = e0; c0 < e1; c0 += G) {
            const int64_t e = c0 + t;
            bool keep = false, tie = false;
            int32_t c = 0;
            float x = 0.f;
            if (e < e1) {
                c = colidx[e];
                x = vals[e];
                if ((int64_t)c == i) keep = keep_diag != 0;
                else if (!cut) keep = true;
                else {
                    const uint32_t o = float_ord(x);
                    tie = o == thr;
                    keep = o > thr;
                }
            }
            int n_tie, n_keep;
            const int tie_before = block_excl_scan<G>(tie ? 1 : 0, s_wave, n_tie);
            keep = keep || (tie && ties + tie_before < need);
            const int keep_before = block_excl_scan<G>(keep ? 1 : 0, s_wave, n_keep);
            if (keep && pos + keep_before < o_end) {
                o_colidx[pos + keep_before] = c;
                o_vals[pos + keep_before] = x;
            }
            ties += n_tie;
            pos += n_keep;
        }
    }
}

__global__ __launch_bounds__(64) void topk_fill_wave(const int64_t *rowptr, const int32_t *colidx, const float *vals,
                                                     int64_t n, int64_t k, int keep_diag, const int64_t *o_rowptr,
                                                     int32_t *o_colidx, float *o_vals) {
    topk_fill_rows<64>(rowptr, colidx, vals, n, k, keep_diag, o_rowptr, o_colidx, o_vals);
}
__global__ __launch_bounds__(256) void topk_fill_block(const int64_t *rowptr, const int32_t *colidx, const float *vals,
                                                       int64_t n, int64_t k, int keep_diag, const int64_t *o_rowptr,
                                                       int32_t *o_colidx, float *o_vals) {
    topk_fill_rows<256>(rowptr, colidx, vals, n, k, keep_diag, o_rowptr, o_colidx, o_vals);
}


// ---- sampled neighbours: meta-path-guided random walks -----------------------------------------------------------------
// (the definition: include/han_hip.h.)  One wave per start row, a persistent grid striding over the rows.  A lane runs
// kWalkUnroll walks at a time -- every hop is two dependent loads (row pointers, then the drawn entry), so the only
// parallelism inside a walk is across walks: 4 x 64 walks of a wave are in flight together, and eight waves per SIMD
// hide the rest.  The end points go to LDS (a dead walk as kWalkDead, above any int32 column), are sorted by the
// short-row sorter, and the first of every run of equal columns is compacted in place beside its position: the run
// lengths are the visit counts.  A row with more than `fanout` distinct end points (off the diagonal with diag) is cut
// by count: a histogram of walks + 1 LDS bins gives the smallest count kept and how many of the columns with exactly
// that count are still needed; one pass in column order then keeps those of smaller column (as topk_fill_rows).
// count and fill walk again rather than stage rows x (fanout + 1) words: the K0 convention (no scratch of the size of
// the output, one kernel body, bitwise the same walks by construction).
constexpr int kWalkUnroll = 4;
constexpr int kWalkCap = 4 * kShortCap;
constexpr uint32_t kWalkDead = 0xFFFFFFFFu;

struct WalkArgs {
    const int64_t *rowptr[HAN_WALK_MAX_HOPS];
    const int32_t *colidx[HAN_WALK_MAX_HOPS];
    int64_t next_rows[HAN_WALK_MAX_HOPS];      // the nodes hop h leads to: rows of hop h + 1, n_cols after the last
    int n_hops, walks, fanout, diag;
    int stage_cap;                   // LDS entries of the sort: a power of two >= max(walks, 64)
    uint32_t seed_lo, seed_hi;
    int64_t row_base, n_rows;
    int64_t *counts;                 // count pass
    const int64_t *c_rowptr;         // fill pass
    int32_t *c_colidx, *c_visits;
};

template <bool FILL>
__device__ __forceinline__ void walk_rows(const WalkArgs &a) {
    extern __shared__ uint32_t wstage[];       // stage_cap end points, stage_cap + 1 run starts, walks + 1 bins
    const int t = threadIdx.x;
    const int P = a.stage_cap, W = a.walks, L = a.n_hops;
    uint32_t *ends = wstage;
    int *start = reinterpret_cast<int *>(wstage + P);
    int *hist = start + P + 1;
    const uint32_t bq = (uint32_t)((L + 1) >> 1);
    const uint64_t below = (1ull << t) - 1ull;
    for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
        const int64_t i = a.row_base + r;
        // the walks
        for (int w0 = 0; w0 < P; w0 += 64 * kWalkUnroll) {
            int64_t cur[kWalkUnroll];
            bool alive[kWalkUnroll];
#pragma unroll
            for (int u = 0; u < kWalkUnroll; ++u) {
                cur[u] = i;
                alive[u] = w0 + 64 * u + t < W;
            }
            for (int h = 0; h < L; ++h) {
                const int64_t *__restrict__ rp = a.rowptr[h];
                const int32_t *__restrict__ ci = a.colidx[h];
                const int64_t nxt = a.next_rows[h];
                int64_t beg[kWalkUnroll], deg[kWalkUnroll];
#pragma unroll
                for (int u = 0; u < kWalkUnroll; ++u) {
                    beg[u] = 0;
                    deg[u] = 0;
                    if (alive[u]) {
                        beg[u] = rp[cur[u]];
                        deg[u] = rp[cur[u] + 1] - beg[u];
                    }
                }
#pragma unroll
                for (int u = 0; u < kWalkUnroll; ++u) {
                    alive[u] = alive[u] && deg[u] > 0;
                    if (alive[u]) {
                        const uint32_t w = (uint32_t)(w0 + 64 * u + t);
                        const HanRand64 d = han_rand64(a.seed_lo, a.seed_hi, HAN_STREAM_WALK, (uint32_t)i,
                                                       w * bq + (uint32_t)(h >> 1));
                        const uint32_t rnd = (h & 1) ? d.y : d.x;
                        const uint64_t e = ((uint64_t)rnd * (uint64_t)(uint32_t)deg[u]) >> 32;
                        cur[u] = ci[beg[u] + (int64_t)e];
                        alive[u] = (uint64_t)cur[u] < (uint64_t)nxt;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kWalkUnroll; ++u) {
                const int w = w0 + 64 * u + t;
                if (w < P) ends[w] = alive[u] ? (uint32_t)cur[u] : kWalkDead;      // (the pads beyond W are dead too)
            }
        }
        __syncthreads();
        bitonic_sort_wave(ends, P);
        // the first of every run of equal columns, compacted in place: ends[k] the k-th distinct column, start[k] the
        // position of its run (a write lands at or below the position it was read from, and a chunk is read -- the
        // barrier -- before it is written)
        int nu = 0, n_live = 0, seen_diag = 0;
        uint32_t prev_last = kWalkDead;
        for (int p0 = 0; p0 < P; p0 += 64) {
            const uint32_t v = ends[p0 + t];
            uint32_t prev = __shfl_up(v, 1, 64);
            if (t == 0) prev = prev_last;
            const bool live = v != kWalkDead;
            const bool head = live && (p0 + t == 0 || v != prev);
            const uint64_t m = __ballot(head);
            prev_last = __shfl(v, 63, 64);
            __syncthreads();
            if (head) {
                const int k = nu + __popcll(m & below);
                ends[k] = v;
                start[k] = p0 + t;
            }
            seen_diag |= __ballot(head && a.diag && (int64_t)v == i) != 0ull;
            nu += __popcll(m);
            n_live += __popcll(__ballot(live));
            __syncthreads();
            if (n_live < p0 + 64) break;         // (uniform: only dead walks follow)
        }
        if (t == 0) start[nu] = n_live;
        const int add_diag = (a.diag && !seen_diag) ? 1 : 0;     // (i, i) with count 0 joins the row
        const int n_off = nu - seen_diag;                        // the columns that compete for fanout
        const bool cut = n_off > a.fanout;
        if (!FILL) {
            if (t == 0) a.counts[r] = (int64_t)(cut ? a.fanout : n_off) + (a.diag ? 1 : 0);
            __syncthreads();                 // the stage is rewritten by the next row
            continue;
        }
        __syncthreads();
        int thr = 0, need = 0;
        if (cut) {
            for (int b = t; b <= W; b += 64) hist[b] = 0;
            __syncthreads();
            for (int k = t; k < nu; k += 64)
                if (!(a.diag && (int64_t)ends[k] == i)) atomicAdd(&hist[start[k + 1] - start[k]], 1);
            __syncthreads();
            const int B = (W + 63) >> 6;     // lane t owns the counts W - t B, ..., W - t B - (B - 1) (those >= 1)
            int mine = 0;
            for (int q = 0; q < B; ++q) {
                const int c = W - t * B - q;
                if (c >= 1) mine += hist[c];
            }
            int x = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d, 64);
                if (t >= d) x += y;
            }
            const int above = x - mine;
            int c = 0, left = 0;
            const bool sel = above < a.fanout && a.fanout <= above + mine;       // exactly one lane (cut)
            if (sel) {
                left = a.fanout - above;
                c = W - t * B;
                while (c > 1 && hist[c] < left) left -= hist[c--];
            }
            const int src = __ffsll((unsigned long long)__ballot(sel)) - 1;
            thr = __shfl(c, src, 64);
            need = __shfl(left, src, 64);
        }
        const int64_t base = a.c_rowptr[r], end = a.c_rowptr[r + 1];
        int kept = 0, ties = 0, kept_below = 0;
        for (int k0 = 0; k0 < nu; k0 += 64) {
            const int k = k0 + t;
            bool keep = false, tie = false, lower = false;
            uint32_t col = 0u;
            int cnt = 0;
            if (k < nu) {
                col = ends[k];
                cnt = start[k + 1] - start[k];
                lower = (int64_t)col < i;
                if (a.diag && (int64_t)col == i) keep = true;
                else if (!cut) keep = true;
                else {
                    tie = cnt == thr;
                    keep = cnt > thr;
                }
            }
            const int tie_before = __popcll(__ballot(tie) & below);
            keep = keep || (tie && ties + tie_before < need);
            const uint64_t mk = __ballot(keep);
            if (keep) {
                const int64_t pos = base + kept + __popcll(mk & below) + ((add_diag && !lower) ? 1 : 0);
                if (pos < end) {
                    a.c_colidx[pos] = (int32_t)col;
                    a.c_visits[pos] = cnt;
                }
            }
            ties += __popcll(__ballot(tie));
            kept += __popcll(mk);
            kept_below += __popcll(__ballot(keep && lower));
        }
        if (add_diag && t == 0 && base + kept_below < end) {
            a.c_colidx[base + kept_below] = (int32_t)i;
            a.c_visits[base + kept_below] = 0;
        }
        __syncthreads();                     // the stage is rewritten by the next row
    }
}

// (eight waves per SIMD: the walks are latency-bound; without the bound the fill form takes 105 scalar registers = 7 waves)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void metapath_walk_count(WalkArgs a) { walk_rows<false>(a); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void metapath_walk_fill(WalkArgs a) { walk_rows<true>(a); }

int walk_launch(bool fill, const int64_t *const *hop_rowptr, const int32_t *const *hop_colidx, const int64_t *hop_rows,
                int n_hops, int64_t n_cols, int64_t row_base, int64_t n_rows, int walks, int fanout, uint64_t seed,
                int diag, int64_t *counts, const int64_t *c_rowptr, int32_t *c_colidx, int32_t *c_visits,
                void *stream) {
    if (!hop_rowptr || !hop_colidx || !hop_rows || n_hops < 1 || n_hops > HAN_WALK_MAX_HOPS) return HAN_E_BADARG;
    if (walks < 1 || walks > HAN_WALK_MAX_WALKS || fanout < 1 || fanout > walks) return HAN_E_BADARG;
    if (n_cols < 0 || n_cols > INT32_MAX || row_base < 0 || n_rows < 0) return HAN_E_BADARG;
    WalkArgs a;
    for (int h = 0; h < HAN_WALK_MAX_HOPS; ++h) {
        a.rowptr[h] = nullptr; a.colidx[h] = nullptr; a.next_rows[h] = 0;
    }
    for (int h = 0; h < n_hops; ++h) {
        if (!hop_rowptr[h] || hop_rows[h] < 0) return HAN_E_BADARG;
        a.rowptr[h] = hop_rowptr[h];
        a.colidx[h] = hop_colidx[h];
        a.next_rows[h] = h + 1 < n_hops ? hop_rows[h + 1] : n_cols;
    }
    if (row_base + n_rows > hop_rows[0]) return HAN_E_BADARG;
    if (diag && n_cols != hop_rows[0]) return HAN_E_BADARG;
    if (fill ? !c_rowptr : !counts) return HAN_E_BADARG;
    if (n_rows == 0) return 0;
    a.n_hops = n_hops; a.walks = walks; a.fanout = fanout; a.diag = diag ? 1 : 0;
    int cap = 64;
    while (cap < walks) cap <<= 1;
    a.stage_cap = cap;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.row_base = row_base; a.n_rows = n_rows;
    a.counts = counts; a.c_rowptr = c_rowptr; a.c_colidx = c_colidx; a.c_visits = c_visits;
    const size_t lds = ((size_t)2 * cap + 1 + (size_t)walks + 1) * sizeof(uint32_t);
    const hipError_t e = han_launch_lds(fill ? metapath_walk_fill : metapath_walk_count,
                                        dim3(han_grid_for(n_rows, 1, kWalkCap)), dim3(64), lds, (hipStream_t)stream, a);
    return e == hipSuccess ? 0 : (int)e;
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

extern "C" int han_spgemm_values(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *a_vals,
                                 const int64_t *b_rowptr, const int32_t *b_colidx, const int64_t *b_vals,
                                 int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t *rows,
                                 const int64_t *n_long, int64_t short_max, int64_t tile_cols, int flags,
                                 const int64_t *c_rowptr, const int32_t *c_colidx, int64_t nnz_c, int64_t *c_vals,
                                 void *stream) {
    SpgemmValArgs v;
    const int rc = spgemm_args(v.g, a_rowptr, a_colidx, b_rowptr, b_colidx, n_rows, n_mid, n_cols, rows, n_long,
                               short_max, tile_cols, flags);
    if (rc != 0) return rc;
    if (!c_rowptr || nnz_c < 0 || (nnz_c > 0 && (!c_colidx || !c_vals))) return HAN_E_BADARG;
    if (n_rows == 0 || nnz_c == 0) return 0;
    v.g.counts = nullptr; v.g.c_rowptr = c_rowptr; v.g.c_colidx = const_cast<int32_t *>(c_colidx);
    v.a_vals = a_vals; v.b_vals = b_vals; v.c_vals = c_vals;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(c_vals, 0, (size_t)nnz_c * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    e = han_launch_lds(spgemm_long_values, dim3(spgemm_grid(n_rows, kLongCap)), dim3(kLongBlock),
                       2 * spgemm_bitmap_bytes(n_cols, tile_cols), st, v);
    if (e != hipSuccess) return (int)e;
    e = han_launch_lds(spgemm_short_values, dim3(spgemm_grid(n_rows, kShortCap)), dim3(64),
                       (size_t)v.g.stage_cap * (sizeof(int64_t) + sizeof(int32_t)), st, v);
    if (e != hipSuccess) return (int)e;
    return 0;
}

extern "C" int han_csr_pathsim(const int64_t *rowptr, const int32_t *colidx, const int64_t *counts, int64_t n,
                               int64_t *diag, float *values, void *stream) {
    if (!rowptr || !diag || n < 0) return HAN_E_BADARG;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    pathsim_diag<<<han_grid_for(n, kRowBlock, kRowCap), kRowBlock, 0, st>>>(rowptr, colidx, counts, n, diag);
    HAN_CHECK_LAUNCH();
    pathsim_values<<<han_grid_for(n, kRowBlock / 64, kRowCap), kRowBlock, 0, st>>>(rowptr, colidx, counts, n, diag,
                                                                                    values);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_csr_row_topk_count(const int64_t *rowptr, const int32_t *colidx, int64_t n_rows, int64_t k,
                                      int keep_diag, int64_t *counts, void *stream) {
    if (!rowptr || !counts || n_rows < 0 || k < 1) return HAN_E_BADARG;
    if (n_rows == 0) return 0;
    topk_count<<<han_grid_for(n_rows, kBoundsBlock / 16, kBoundsCap), kBoundsBlock, 0, (hipStream_t)stream>>>(
        rowptr, colidx, n_rows, k, keep_diag ? 1 : 0, counts);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_csr_row_topk_fill(const int64_t *rowptr, const int32_t *colidx, const float *values,
                                     int64_t n_rows, int64_t k, int keep_diag, const int64_t *out_rowptr,
                                     int32_t *out_colidx, float *out_values, void *stream) {
    if (!rowptr || !out_rowptr || n_rows < 0 || k < 1) return HAN_E_BADARG;
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    topk_fill_block<<<han_grid_for(n_rows, 1, kLongCap), 256, 0, st>>>(rowptr, colidx, values, n_rows, k,
                                                                       keep_diag ? 1 : 0, out_rowptr, out_colidx,
                                                                       out_values);
    HAN_CHECK_LAUNCH();
    topk_fill_wave<<<han_grid_for(n_rows, 1, 4 * kShortCap), 64, 0, st>>>(rowptr, colidx, values, n_rows, k,
                                                                          keep_diag ? 1 : 0, out_rowptr, out_colidx,
                                                                          out_values);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_metapath_walk_count(const int64_t *const *hop_rowptr, const int32_t *const *hop_colidx,
                                       const int64_t *hop_rows, int n_hops, int64_t n_cols, int64_t row_base,
                                       int64_t n_rows, int walks, int fanout, uint64_t seed, int diag, int64_t *counts,
                                       void *stream) {
    return walk_launch(false, hop_rowptr, hop_colidx, hop_rows, n_hops, n_cols, row_base, n_rows, walks, fanout, seed,
                       diag, counts, nullptr, nullptr, nullptr, stream);
}

extern "C" int han_metapath_walk_fill(const int64_t *const *hop_rowptr, const int32_t *const *hop_colidx,
                                      const int64_t *hop_rows, int n_hops, int64_t n_cols, int64_t row_base,
                                      int64_t n_rows, int walks, int fanout, uint64_t seed, int diag,
                                      const int64_t *c_rowptr, int32_t *c_colidx, int32_t *c_visits, void *stream) {
    return walk_launch(true, hop_rowptr, hop_colidx, hop_rows, n_hops, n_cols, row_base, n_rows, walks, fanout, seed,
                       diag, nullptr, c_rowptr, c_colidx, c_visits, stream);
}
