// Evaluation of the final embeddings on the GPU (jhyexp.py:20-86): brute-force k nearest neighbours with a
// majority vote, contingency tables for F1 / NMI / ARI, one Lloyd iteration of k-means, and the silhouette score of a
// clustering (data/exp.py:46-49).
//
// Distances are d2 = |q|^2 + |t|^2 - 2 q.t.  The q.t term runs on the exact-fp32 matrix pipe
// (v_mfma_f32_16x16x4_f32) in tiles of 64 x 64 pairs per workgroup step; the distance matrix never exists in
// memory: a lane sees its 16 candidates of a tile in registers and keeps a sorted list of the best ones.
//
// Tile layout (all three tile kernels).  A workgroup of 4 waves stages 64 "column" rows (queries / data rows) and 64 "row"
// rows (train rows / centres), 64 embedding columns at a time, into LDS as [64][kLd] fp32, zero-filled past the
// matrix edges and past D (so a D that is no multiple of 4 is padded in LDS, never in memory).  Wave w owns the
// column rows 16 w .. 16 w + 15 and walks all 64 row rows as four 16 x 16 accumulators.  The MFMA sums over its K
// index, so WHICH four embedding columns a lane group feeds per step is free as long as both operands agree: lane
// group g = lane >> 4 takes columns 16 g + 4 s .. + 3 in step s, one ds_read_b128 per operand and four MFMAs.
// Result map: lane (n = lane & 15, g) holds, in acc[j][r], the product of column row 16 w + n and row row
// 16 j + 4 g + r.
#include "han_common.h"

namespace {

constexpr int kTile = 64;          // rows per staged operand tile
constexpr int kChunk = 64;         // embedding columns per stage
constexpr int kLd = 68;            // LDS row stride (floats): 16-byte aligned rows, row starts 4 banks apart
constexpr int kBlock = 256;
constexpr int kMaxD = 512;
constexpr int kMaxK = 16;          // neighbours
constexpr int kMaxCentres = 64;
constexpr int kSplitRows = 256;    // a train-set split is a multiple of this many rows
constexpr int kMaxSplit = 64;
constexpr int kTargetBlocks = 512; // split the train set until the grid has about this many workgroups
constexpr int kAssignCap = 2048;   // workgroups of the assignment kernel (one inertia partial each)
constexpr int kAccumCap = 1024;    // workgroups of the row-sum kernel (one slab each)
constexpr size_t kSlabBudget = 64u << 20;
constexpr int kMaxTable = 4096;    // Ca * Cb of a contingency table

__device__ __forceinline__ bool pair_less(float d, int i, float od, int oi) { return d < od || (d == od && i < oi); }

// rows [row0, row0 + 64) x columns [col0, col0 + 64) of M (n x D, leading dimension ld) -> s[64][kLd]
__device__ __forceinline__ void stage_tile(float *s, const float *M, int64_t ld, int64_t row0, int64_t n, int col0,
                                           int D) {
    for (int e = threadIdx.x; e < kTile * kChunk; e += kBlock) {
        const int r = e >> 6, c = e & 63;
        const int64_t row = row0 + r;
        const int col = col0 + c;
        s[r * kLd + c] = (row < n && col < D) ? M[row * ld + col] : 0.f;
    }
}

// acc[j] += rows(16 j ..) of Rs  x  columns(16 w ..) of Cs over one staged chunk, for the first nj (uniform) row tiles
__device__ __forceinline__ void mma_chunk(float4_t (&acc)[4], const float *Rs, const float *Cs, int w, int lane,
                                          int nj = 4) {
    const int n = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float4_t b = *reinterpret_cast<const float4_t *>(Cs + (16 * w + n) * kLd + 16 * g + 4 * s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nj) break;
            const float4_t a = *reinterpret_cast<const float4_t *>(Rs + (16 * j + n) * kLd + 16 * g + 4 * s);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc[j], 0, 0, 0);
        }
    }
}

// |row|^2 of every row, 16 lanes per row; a fixed order, exact for small integers
__global__ __launch_bounds__(kBlock) void row_norms(const float *M, int64_t ld, int64_t n, int D, float *out) {
    const int j = threadIdx.x & 15;
    const int64_t stride = (int64_t)gridDim.x * (kBlock / 16);
    const int64_t rounds = (n + stride - 1) / stride;          // whole 16-lane groups stay active for the DPP sum
    for (int64_t it = 0; it < rounds; ++it) {
        const int64_t row = it * stride + (int64_t)blockIdx.x * (kBlock / 16) + (threadIdx.x >> 4);
        float s = 0.f;
        if (row < n)
            for (int c = j; c < D; c += 16) {
                const float x = M[row * ld + c];
                s = fmaf(x, x, s);
            }
        s = han_row16_sum(s);
        if (row < n && j == 0) out[row] = s;
    }
}

// sorted list of the KC smallest (d2, index) pairs of one lane
template <int KC>
struct TopList {
    float d[KC];
    int i[KC];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < KC; ++j) { d[j] = __builtin_inff(); i[j] = 0x7FFFFFFF; }
    }
    __device__ __forceinline__ void offer(float cd, int ci) {
        if (!pair_less(cd, ci, d[KC - 1], i[KC - 1])) return;
#pragma unroll
        for (int j = KC - 1; j > 0; --j) {
            const bool up = pair_less(cd, ci, d[j - 1], i[j - 1]);
            const bool here = !up && pair_less(cd, ci, d[j], i[j]);
            d[j] = up ? d[j - 1] : (here ? cd : d[j]);
            i[j] = up ? i[j - 1] : (here ? ci : i[j]);
        }
        if (pair_less(cd, ci, d[0], i[0])) { d[0] = cd; i[0] = ci; }
    }
};

struct KnnArgs {
    const float *Q, *T, *qn, *tn;
    int64_t ldq, ldt, Nq, Nt, split_rows;
    int D, k;
    int32_t *out_idx;      // [split][Nq][k]
    float *out_d2;
};

template <int KC>
__global__ __launch_bounds__(kBlock) void knn_tiles(const KnnArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTile * kLd];
    __shared__ float tns[kTile];
    float *Rs = smem, *Cs = smem + kTile * kLd;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kTile;
    const int64_t t_begin = (int64_t)blockIdx.y * a.split_rows;
    const int64_t t_end = min(a.Nt, t_begin + a.split_rows);
    const int64_t myq = q0 + 16 * w + n;
    const float qnorm = myq < a.Nq ? a.qn[myq] : 0.f;
    const int nch = (a.D + kChunk - 1) / kChunk;
    TopList<KC> top;
    top.init();
    for (int64_t t0 = t_begin; t0 < t_end; t0 += kTile) {
        float4_t acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = float4_t{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            stage_tile(Rs, a.T, a.ldt, t0, t_end, c * kChunk, a.D);
            if (nch > 1 || t0 == t_begin) stage_tile(Cs, a.Q, a.ldq, q0, a.Nq, c * kChunk, a.D);
            if (c == 0 && threadIdx.x < kTile) tns[threadIdx.x] = t0 + threadIdx.x < t_end ? a.tn[t0 + threadIdx.x] : 0.f;
            __syncthreads();
            mma_chunk(acc, Rs, Cs, w, lane);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tl = 16 * j + 4 * g + r;
                if (t0 + tl < t_end) top.offer((qnorm + tns[tl]) - 2.f * acc[j][r], (int)(t0 + tl));
            }
    }
    // the four lanes of a query: groups 1..3 hand their lists to group 0 through LDS
    __syncthreads();
    float *md = smem;
    int *mi = reinterpret_cast<int *>(smem) + kBlock * KC;
    static_assert(2 * kBlock * kMaxK <= 2 * kTile * kLd, "merge lists fit the staging area");
#pragma unroll
    for (int j = 0; j < KC; ++j) { md[threadIdx.x * KC + j] = top.d[j]; mi[threadIdx.x * KC + j] = top.i[j]; }
    __syncthreads();
    if (g == 0 && myq < a.Nq) {
        for (int og = 1; og < 4; ++og) {
            const int src = (64 * w + 16 * og + n) * KC;
#pragma unroll
            for (int j = 0; j < KC; ++j) top.offer(md[src + j], mi[src + j]);
        }
        const int64_t o = ((int64_t)blockIdx.y * a.Nq + myq) * a.k;
#pragma unroll
        for (int j = 0; j < KC; ++j)
            if (j < a.k) { a.out_idx[o + j] = top.i[j]; a.out_d2[o + j] = top.d[j]; }
    }
}

// a thread per query: the lists of the train-set splits, each sorted, into one
template <int KC>
__global__ __launch_bounds__(kBlock) void knn_merge(const int32_t *pidx, const float *pd2, int nsplit, int64_t Nq, int k,
                                                    int32_t *idx, float *d2) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= Nq) return;
    TopList<KC> top;
    top.init();
    for (int s = 0; s < nsplit; ++s) {
        const int64_t o = ((int64_t)s * Nq + q) * k;
        for (int j = 0; j < k; ++j) top.offer(pd2[o + j], pidx[o + j]);
    }
#pragma unroll
    for (int j = 0; j < KC; ++j)
        if (j < k) { idx[q * k + j] = top.i[j]; d2[q * k + j] = top.d[j]; }
}

// mode of the k neighbour labels, ties to the smallest class id: k^2 compares in registers
__global__ __launch_bounds__(kBlock) void knn_vote(const int32_t *idx, const int32_t *labels, int32_t *pred, int64_t Nq,
                                                   int k, int64_t Nt) {
    const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (q >= Nq) return;
    int lab[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) {
        lab[j] = -1;
        if (j < k) {
            const int t = idx[q * k + j];
            if (t >= 0 && t < Nt) lab[j] = labels[t];
        }
    }
    int best = 0x7FFFFFFF, best_n = 0;
#pragma unroll
    for (int x = 0; x < kMaxK; ++x) {
        int c = 0;
#pragma unroll
        for (int y = 0; y < kMaxK; ++y) c += (y < k && lab[y] == lab[x]) ? 1 : 0;
        if (x < k && (c > best_n || (c == best_n && lab[x] < best))) { best = lab[x]; best_n = c; }
    }
    pred[q] = best;
}

// table[a * Cb + b] += 1 per element; table[Ca * Cb] (the flag word) != 0 when a label was out of range
__global__ __launch_bounds__(kBlock) void contingency_kernel(const int32_t *la, const int32_t *lb, int64_t n, int Ca, int Cb,
                                                             unsigned long long *table) {
    extern __shared__ int cnt[];
    const int cells = Ca * Cb;
    for (int e = threadIdx.x; e < cells; e += kBlock) cnt[e] = 0;
    __syncthreads();
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int x = la[i], y = lb[i];
        if ((unsigned)x >= (unsigned)Ca || (unsigned)y >= (unsigned)Cb) bad = true;
        else atomicAdd(&cnt[x * Cb + y], 1);
    }
    if (bad) atomicAdd(&table[cells], 1ull);
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += kBlock)
        if (cnt[e]) atomicAdd(&table[e], (unsigned long long)cnt[e]);
}

struct AssignArgs {
    const float *X, *C, *xn, *cn;
    int64_t ldx, N, tiles, tiles_per_block;
    int D, k;
    const int32_t *prev;
    int32_t *labels;
    float *d2;
    unsigned long long *counts, *changed;
    double *inertia_part;      // one per workgroup
};

__global__ __launch_bounds__(kBlock) void kmeans_assign(const AssignArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTile * kLd];
    __shared__ float cns[kMaxCentres];
    __shared__ int cnt[kMaxCentres];
    __shared__ int chg;
    __shared__ double part[kBlock];
    float *Rs = smem, *Cs = smem + kTile * kLd;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    if (threadIdx.x < kMaxCentres) {
        cns[threadIdx.x] = threadIdx.x < a.k ? a.cn[threadIdx.x] : 0.f;
        cnt[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) chg = 0;
    const int nch = (a.D + kChunk - 1) / kChunk;
    const int64_t tile_begin = (int64_t)blockIdx.x * a.tiles_per_block;
    const int64_t tile_end = min(a.tiles, tile_begin + a.tiles_per_block);
    double iner = 0.0;
    for (int64_t tile = tile_begin; tile < tile_end; ++tile) {
        const int64_t x0 = tile * kTile;
        float4_t acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = float4_t{0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < nch; ++c) {
            __syncthreads();
            stage_tile(Cs, a.X, a.ldx, x0, a.N, c * kChunk, a.D);
            if (nch > 1 || tile == tile_begin) stage_tile(Rs, a.C, a.D, 0, a.k, c * kChunk, a.D);
            __syncthreads();
            mma_chunk(acc, Rs, Cs, w, lane, (a.k + 15) >> 4);      // row tiles past the last centre hold zeros
        }
        const int64_t row = x0 + 16 * w + n;
        const float xnorm = row < a.N ? a.xn[row] : 0.f;
        float best = __builtin_inff();
        int bi = 0x7FFFFFFF;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = 16 * j + 4 * g + r;
                if (ci < a.k) {
                    const float d = (xnorm + cns[ci]) - 2.f * acc[j][r];
                    if (pair_less(d, ci, best, bi)) { best = d; bi = ci; }
                }
            }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float od = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (pair_less(od, oi, best, bi)) { best = od; bi = oi; }
        }
        if (g == 0 && row < a.N) {
            if ((unsigned)bi >= (unsigned)a.k) bi = 0;          // a row of NaNs compares with nothing
            const bool moved = a.prev ? a.prev[row] != bi : true;
            a.labels[row] = bi;
            if (a.d2) a.d2[row] = best;
            iner += (double)best;
            atomicAdd(&cnt[bi], 1);
            if (moved) atomicAdd(&chg, 1);
        }
    }
    part[threadIdx.x] = iner;
    __syncthreads();
    if (threadIdx.x < a.k && cnt[threadIdx.x]) atomicAdd(&a.counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (chg) atomicAdd(a.changed, (unsigned long long)chg);
        double s = 0.0;
        for (int t = 0; t < kBlock; ++t) s += part[t];
        a.inertia_part[blockIdx.x] = s;
    }
}

// per-cluster row sums of one workgroup's rows, in double: thread (group, column) adds its rows in order into the
// group's own LDS table; the four tables are added in a fixed order into the workgroup's slab
__global__ __launch_bounds__(kBlock) void kmeans_row_sums(const float *X, int64_t ldx, const int32_t *labels, int64_t N, int D,
                                                         int k, int64_t rows_per_block, int dp, double *slab) {
    extern __shared__ double tab[];      // [4][k][64]
    const int grp = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int col = blockIdx.y * 64 + c;
    for (int e = threadIdx.x; e < 4 * k * 64; e += kBlock) tab[e] = 0.0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(N, r0 + rows_per_block);
    double *mine = tab + (size_t)grp * k * 64 + c;
    int64_t r = r0 + grp;
    for (; r + 12 < r1; r += 16) {
        const int l0 = labels[r], l1 = labels[r + 4], l2 = labels[r + 8], l3 = labels[r + 12];
        float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
        if (col < D) {
            x0 = X[r * ldx + col]; x1 = X[(r + 4) * ldx + col];
            x2 = X[(r + 8) * ldx + col]; x3 = X[(r + 12) * ldx + col];
        }
        mine[l0 * 64] += (double)x0;
        mine[l1 * 64] += (double)x1;
        mine[l2 * 64] += (double)x2;
        mine[l3 * 64] += (double)x3;
    }
    for (; r < r1; r += 4) mine[labels[r] * 64] += col < D ? (double)X[r * ldx + col] : 0.0;
    __syncthreads();
    for (int e = threadIdx.x; e < k * 64; e += kBlock) {
        const double s = ((tab[e] + tab[k * 64 + e]) + tab[2 * k * 64 + e]) + tab[3 * k * 64 + e];
        slab[((size_t)blockIdx.x * k + (e >> 6)) * dp + blockIdx.y * 64 + (e & 63)] = s;
    }
}

// new centre = sum of the slabs (in order) / count; a cluster without rows keeps its centre.  Thread 0 also adds
// the inertia partials in order.
__global__ __launch_bounds__(kBlock) void kmeans_finish(const double *slab, int nslab, int dp, const float *C, int D, int k,
                                                       const unsigned long long *counts, float *newC,
                                                       const double *inertia_part, int nparts, double *inertia) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < k * D) {
        const int cl = e / D, d = e - cl * D;
        double s = 0.0;
        for (int b = 0; b < nslab; ++b) s += slab[((size_t)b * k + cl) * dp + d];
        const unsigned long long cnt = counts[cl];
        newC[e] = cnt ? (float)(s / (double)cnt) : C[e];
    }
    if (e == 0) {
        double s = 0.0;
        for (int b = 0; b < nparts; ++b) s += inertia_part[b];
        *inertia = s;
    }
}

// ---- silhouette (data/exp.py:46-49) -----------------------------------------------------------------------------
// S(i, c) = sum over the rows j of cluster c of |x_i - x_j|, for a row tile of 64 rows i against the column rows
// [blockIdx.y * split_rows, + split_rows).  The rows are grouped by cluster, so the column tiles are cut at the segment
// (and split) boundaries and a tile holds rows of ONE cluster: a lane adds the (at most 16) distances it sees of a
// tile in fp32 in a fixed order, adds that to its double sum of the cluster, and at the end of the cluster the four
// lanes of a row are added in a fixed order.  No accumulator is indexed by a label.
struct SilArgs {
    const float *X, *xn;
    const int64_t *seg;      // (k + 1) segment bounds
    int64_t ldx, N, split_rows;
    int D, k;
    double *slab;            // [split][k][N] partial S(i, c); NULL with one split: a and b are formed here
    double *ab;              // [2][N]: a, then b
};

// a and b of a row from its sums: n_own rows in its cluster (itself included), `best` the smallest mean distance to
// another non-empty cluster (+inf: there is none)
__device__ __forceinline__ void sil_ab(double s_own, int64_t n_own, double best, double *a, double *b) {
    *a = n_own > 1 ? s_own / (double)(n_own - 1) : 0.0;
    *b = best < __builtin_inf() ? best : 0.0;
}

__global__ __launch_bounds__(kBlock) void sil_tiles(const SilArgs a) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTile * kLd];
    __shared__ float tns[kTile];
    __shared__ int64_t segs[kMaxCentres + 1];
    float *Rs = smem, *Cs = smem + kTile * kLd;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    if (threadIdx.x <= a.k) segs[threadIdx.x] = a.seg[threadIdx.x];
    const int64_t q0 = (int64_t)blockIdx.x * kTile;
    const int64_t t_begin = (int64_t)blockIdx.y * a.split_rows;
    const int64_t t_end = min(a.N, t_begin + a.split_rows);
    const int64_t myq = q0 + 16 * w + n;
    const float qnorm = myq < a.N ? a.xn[myq] : 0.f;
    const int nch = (a.D + kChunk - 1) / kChunk;
    double s_own = 0.0, best = __builtin_inf();
    int64_t n_own = 0;
    bool staged = false;                                     // the row tile is in Cs (one chunk: staged once)
    __syncthreads();
    for (int c = 0; c < a.k; ++c) {
        const int64_t c0 = segs[c], c1 = segs[c + 1];
        const int64_t lo = max(c0, t_begin), hi = min(c1, t_end);      // inside [0, N) whatever seg holds
        double S = 0.0;
        for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
            const int nj = (int)((min(hi - t0, (int64_t)kTile) + 15) >> 4);
            float4_t acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = float4_t{0.f, 0.f, 0.f, 0.f};
            for (int ch = 0; ch < nch; ++ch) {
                __syncthreads();
                stage_tile(Rs, a.X, a.ldx, t0, hi, ch * kChunk, a.D);
                if (nch > 1 || !staged) stage_tile(Cs, a.X, a.ldx, q0, a.N, ch * kChunk, a.D);
                if (ch == 0 && threadIdx.x < kTile) tns[threadIdx.x] = t0 + threadIdx.x < hi ? a.xn[t0 + threadIdx.x] : 0.f;
                __syncthreads();
                mma_chunk(acc, Rs, Cs, w, lane, nj);
            }
            staged = true;
            float part = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tl = 16 * j + 4 * g + r;
                    if (t0 + tl < hi) {
                        const float d2 = (qnorm + tns[tl]) - 2.f * acc[j][r];
                        part += t0 + tl == myq ? 0.f : sqrtf(fmaxf(d2, 0.f));      // the pair (i, i) by its index
                    }
                }
            S += (double)part;
        }
        S += __shfl_xor(S, 16, 64);                          // (g0 + g1) + (g2 + g3) in every lane of the row
        S += __shfl_xor(S, 32, 64);
        if (a.slab) {
            if (g == 0 && myq < a.N) a.slab[((size_t)blockIdx.y * a.k + c) * a.N + myq] = S;
        } else if (myq >= c0 && myq < c1) {
            s_own = S;
            n_own = c1 - c0;
        } else if (c1 > c0) {
            best = fmin(best, S / (double)(c1 - c0));
        }
    }
    if (!a.slab && g == 0 && myq < a.N) sil_ab(s_own, n_own, best, &a.ab[myq], &a.ab[a.N + myq]);
}

// a thread per row: a and b (from the slabs of the splits, added in order, when there are any), s, and the sum of
// the workgroup's s in row order
__global__ __launch_bounds__(kBlock) void sil_finish(const int64_t *seg, int k, int64_t N, const double *slab, int nsplit,
                                                    const double *ab, float *a_out, float *b_out, float *s_out,
                                                    double *part) {
    __shared__ int64_t segs[kMaxCentres + 1];
    __shared__ double ps[kBlock];
    if (threadIdx.x <= k) segs[threadIdx.x] = seg[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double s = 0.0;
    if (i < N) {
        double av, bv, s_own = 0.0, best = __builtin_inf();
        int64_t n_own = 0;
        bool other = false;                                  // another cluster has rows
        for (int c = 0; c < k; ++c) {
            const int64_t c0 = segs[c], c1 = segs[c + 1];
            if (c1 <= c0) continue;
            const bool own = i >= c0 && i < c1;
            if (own) n_own = c1 - c0;
            else other = true;
            if (slab) {
                double S = 0.0;
                for (int sp = 0; sp < nsplit; ++sp) S += slab[((size_t)sp * k + c) * N + i];
                if (own) s_own = S;
                else best = fmin(best, S / (double)(c1 - c0));
            }
        }
        if (slab) {
            sil_ab(s_own, n_own, best, &av, &bv);
        } else {
            av = ab[i];
            bv = ab[N + i];
        }
        const double m = fmax(av, bv);
        s = (n_own > 1 && other && m > 0.0) ? (bv - av) / m : 0.0;
        const float sf = (float)s;
        s = (double)sf;                                      // the sum is that of the fp32 values written
        if (a_out) a_out[i] = (float)av;
        if (b_out) b_out[i] = (float)bv;
        if (s_out) s_out[i] = sf;
    }
    ps[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int e = 0; e < kBlock; ++e) t += ps[e];
        part[blockIdx.x] = t;
    }
}

// one workgroup: the partials of sil_finish, each thread its own in order, then the 256 threads in order
__global__ __launch_bounds__(kBlock) void sil_total(const double *part, int64_t nparts, double *sum) {
    __shared__ double ps[kBlock];
    double t = 0.0;
    for (int64_t e = threadIdx.x; e < nparts; e += kBlock) t += part[e];
    ps[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int e = 0; e < kBlock; ++e) s += ps[e];
        *sum = s;
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// train-set splits of a KNN call: enough workgroups to fill the device when there are few queries
inline int knn_splits(int64_t Nq, int64_t Nt, int64_t *split_rows) {
    const int64_t qblocks = (Nq + kTile - 1) / kTile;
    int64_t ns = (kTargetBlocks + qblocks - 1) / qblocks;
    const int64_t units = (Nt + kSplitRows - 1) / kSplitRows;
    if (ns > units) ns = units;
    if (ns > kMaxSplit) ns = kMaxSplit;
    if (ns < 1) ns = 1;
    const int64_t rows = ((units + ns - 1) / ns) * kSplitRows;
    *split_rows = rows;
    return (int)((Nt + rows - 1) / rows);
}

struct KmeansPlan {
    int64_t tiles, tiles_per_block, rows_per_block;
    int assign_blocks, sum_blocks, dp;
    size_t off_cn, off_part, off_slab, bytes;
};

inline KmeansPlan kmeans_plan(int64_t N, int D, int k) {
    KmeansPlan p;
    p.tiles = (N + kTile - 1) / kTile;
    p.assign_blocks = (int)(p.tiles < kAssignCap ? (p.tiles < 1 ? 1 : p.tiles) : kAssignCap);
    p.tiles_per_block = (p.tiles + p.assign_blocks - 1) / p.assign_blocks;
    p.dp = ((D + 63) / 64) * 64;
    const size_t slab_bytes = (size_t)k * p.dp * sizeof(double);
    int64_t cap = (int64_t)(kSlabBudget / slab_bytes);
    if (cap > kAccumCap) cap = kAccumCap;
    if (cap < 1) cap = 1;
    int64_t sb = (N + kBlock - 1) / kBlock;
    if (sb > cap) sb = cap;
    if (sb < 1) sb = 1;
    p.sum_blocks = (int)sb;
    p.rows_per_block = (N + sb - 1) / sb;
    p.off_cn = align256((size_t)N * sizeof(float));
    p.off_part = p.off_cn + align256(kMaxCentres * sizeof(float));
    p.off_slab = p.off_part + align256((size_t)kAssignCap * sizeof(double));
    p.bytes = p.off_slab + align256((size_t)p.sum_blocks * slab_bytes);
    return p;
}

inline int norms_grid(int64_t n) { return han_grid_for(n, kBlock / 16, 8192); }

// the column range of a silhouette call is split like the train set of a KNN call; slabs only with more than one split
struct SilPlan {
    int64_t split_rows, finish_blocks;
    int nsplit;
    size_t off_ab, off_part, off_slab, bytes;
};

inline SilPlan sil_plan(int64_t N, int k) {
    SilPlan p;
    p.nsplit = knn_splits(N, N, &p.split_rows);
    p.finish_blocks = (N + kBlock - 1) / kBlock;
    p.off_ab = align256((size_t)N * sizeof(float));
    p.off_part = p.off_ab + align256((size_t)2 * N * sizeof(double));
    p.off_slab = p.off_part + align256((size_t)p.finish_blocks * sizeof(double));
    p.bytes = p.off_slab + (p.nsplit > 1 ? align256((size_t)p.nsplit * k * N * sizeof(double)) : 0);
    return p;
}

}  // namespace

extern "C" size_t han_knn_topk_workspace(int64_t Nq, int64_t Nt, int D, int k) {
    if (Nq <= 0 || Nt <= 0 || D < 1 || k < 1) return 0;
    int64_t rows;
    const int ns = knn_splits(Nq, Nt, &rows);
    size_t b = align256((size_t)Nq * sizeof(float)) + align256((size_t)Nt * sizeof(float));
    if (ns > 1) b += 2 * align256((size_t)ns * Nq * k * sizeof(float));
    return b;
}

extern "C" int han_knn_topk(const float *Q, int64_t ldq, const float *T, int64_t ldt, int32_t *idx, float *d2,
                            void *workspace, size_t workspace_bytes, int64_t Nq, int64_t Nt, int D, int k,
                            void *stream) {
    if (Nq < 0 || Nt < 0 || D < 1 || k < 1 || ldq < D || ldt < D || k > Nt) return HAN_E_BADARG;
    if (k > kMaxK || D > kMaxD || Nt > 0x7FFFFFFF) return HAN_E_UNSUPPORTED;
    if (Nq == 0) return 0;
    if (!Q || !T || !idx || !d2 || !workspace) return HAN_E_BADARG;
    if (workspace_bytes < han_knn_topk_workspace(Nq, Nt, D, k)) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int64_t rows;
    const int ns = knn_splits(Nq, Nt, &rows);
    char *ws = (char *)workspace;
    float *qn = (float *)ws;
    float *tn = (float *)(ws + align256((size_t)Nq * sizeof(float)));
    char *parts = (char *)tn + align256((size_t)Nt * sizeof(float));
    const size_t part_bytes = align256((size_t)ns * Nq * k * sizeof(float));
    row_norms<<<norms_grid(Nq), kBlock, 0, st>>>(Q, ldq, Nq, D, qn);
    HAN_CHECK_LAUNCH();
    row_norms<<<norms_grid(Nt), kBlock, 0, st>>>(T, ldt, Nt, D, tn);
    HAN_CHECK_LAUNCH();
    KnnArgs a;
    a.Q = Q; a.T = T; a.qn = qn; a.tn = tn; a.ldq = ldq; a.ldt = ldt; a.Nq = Nq; a.Nt = Nt; a.split_rows = rows;
    a.D = D; a.k = k;
    a.out_idx = ns > 1 ? (int32_t *)parts : idx;
    a.out_d2 = ns > 1 ? (float *)(parts + part_bytes) : d2;
    const dim3 grid((unsigned)((Nq + kTile - 1) / kTile), (unsigned)ns);
    const int64_t mgrid = (Nq + kBlock - 1) / kBlock;
#define HAN_KNN_LAUNCH(KC)                                                                                        \
    do {                                                                                                          \
        knn_tiles<KC><<<grid, kBlock, 0, st>>>(a);                                                                \
        HAN_CHECK_LAUNCH();                                                                                       \
        if (ns > 1) {                                                                                             \
            knn_merge<KC><<<(unsigned)mgrid, kBlock, 0, st>>>(a.out_idx, a.out_d2, ns, Nq, k, idx, d2);           \
            HAN_CHECK_LAUNCH();                                                                                   \
        }                                                                                                         \
    } while (0)
    if (k == 1) HAN_KNN_LAUNCH(1);
    else if (k <= 8) HAN_KNN_LAUNCH(8);
    else HAN_KNN_LAUNCH(16);
#undef HAN_KNN_LAUNCH
    return 0;
}

extern "C" int han_knn_vote(const int32_t *idx, const int32_t *labels_train, int32_t *pred, int64_t Nq, int k,
                            int64_t Nt, void *stream) {
    if (Nq < 0 || Nt < 0 || k < 1) return HAN_E_BADARG;
    if (k > kMaxK) return HAN_E_UNSUPPORTED;
    if (Nq == 0) return 0;
    if (!idx || !labels_train || !pred) return HAN_E_BADARG;
    knn_vote<<<(unsigned)((Nq + kBlock - 1) / kBlock), kBlock, 0, (hipStream_t)stream>>>(idx, labels_train, pred, Nq, k, Nt);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_contingency(const int32_t *a, const int32_t *b, int64_t n, int Ca, int Cb, int64_t *table,
                               void *stream) {
    if (n < 0 || Ca < 1 || Cb < 1 || !table) return HAN_E_BADARG;
    if ((int64_t)Ca * Cb > kMaxTable) return HAN_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(table, 0, ((size_t)Ca * Cb + 1) * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return 0;
    if (!a || !b) return HAN_E_BADARG;
    contingency_kernel<<<han_grid_for(n, 4 * kBlock, 1024), kBlock, (size_t)Ca * Cb * sizeof(int), st>>>(
        a, b, n, Ca, Cb, (unsigned long long *)table);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t han_kmeans_step_workspace(int64_t N, int D, int k) {
    if (N <= 0 || D < 1 || k < 1 || k > kMaxCentres) return 0;
    return kmeans_plan(N, D, k).bytes;
}

extern "C" int han_kmeans_step(const float *X, int64_t ldx, const float *C, const int32_t *prev, int32_t *labels,
                               float *d2, int64_t *counts, float *new_centres, double *inertia, int64_t *changed,
                               void *workspace, size_t workspace_bytes, int64_t N, int D, int k, void *stream) {
    if (N < 0 || D < 1 || k < 1 || ldx < D) return HAN_E_BADARG;
    if (k > kMaxCentres || D > kMaxD) return HAN_E_UNSUPPORTED;
    if (!C || !counts || !new_centres || !inertia || !changed) return HAN_E_BADARG;
    if (N > 0 && (!X || !labels || !workspace)) return HAN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)k * sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(changed, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    if (N == 0) {
        e = hipMemsetAsync(inertia, 0, sizeof(double), st);
        if (e != hipSuccess) return (int)e;
        e = hipMemcpyAsync(new_centres, C, (size_t)k * D * sizeof(float), hipMemcpyDeviceToDevice, st);
        return (int)e;
    }
    const KmeansPlan p = kmeans_plan(N, D, k);
    if (workspace_bytes < p.bytes) return HAN_E_WORKSPACE;
    char *ws = (char *)workspace;
    float *xn = (float *)ws, *cn = (float *)(ws + p.off_cn);
    double *part = (double *)(ws + p.off_part), *slab = (double *)(ws + p.off_slab);
    row_norms<<<norms_grid(N), kBlock, 0, st>>>(X, ldx, N, D, xn);
    HAN_CHECK_LAUNCH();
    row_norms<<<norms_grid(k), kBlock, 0, st>>>(C, D, k, D, cn);
    HAN_CHECK_LAUNCH();
    AssignArgs a;
    a.X = X; a.C = C; a.xn = xn; a.cn = cn; a.ldx = ldx; a.N = N; a.tiles = p.tiles; a.tiles_per_block = p.tiles_per_block;
    a.D = D; a.k = k; a.prev = prev; a.labels = labels; a.d2 = d2;
    a.counts = (unsigned long long *)counts; a.changed = (unsigned long long *)changed; a.inertia_part = part;
    kmeans_assign<<<p.assign_blocks, kBlock, 0, st>>>(a);
    HAN_CHECK_LAUNCH();
    e = han_launch_lds(kmeans_row_sums, dim3(p.sum_blocks, p.dp / 64), dim3(kBlock), (size_t)4 * k * 64 * sizeof(double), st,
                       X, ldx, (const int32_t *)labels, N, D, k, p.rows_per_block, p.dp, slab);
    if (e != hipSuccess) return (int)e;
    kmeans_finish<<<(k * D + kBlock - 1) / kBlock, kBlock, 0, st>>>(slab, p.sum_blocks, p.dp, C, D, k,
                                                                  (const unsigned long long *)counts, new_centres, part,
                                                                  p.assign_blocks, inertia);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t han_silhouette_workspace(int64_t N, int D, int k) {
    if (N <= 0 || D < 1 || D > kMaxD || k < 2 || k > kMaxCentres || N > 0x7FFFFFFF) return 0;
    return sil_plan(N, k).bytes;
}

extern "C" int han_silhouette(const float *X, int64_t ldx, const int64_t *seg_ptr, int64_t N, int D, int k, float *a,
                              float *b, float *s, double *sum, void *workspace, size_t workspace_bytes, void *stream) {
    if (N < 0 || D < 1 || k < 2 || ldx < D) return HAN_E_BADARG;
    if (k > kMaxCentres || D > kMaxD || N > 0x7FFFFFFF) return HAN_E_UNSUPPORTED;
    if (!sum) return HAN_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) return (int)hipMemsetAsync(sum, 0, sizeof(double), st);
    if (!X || !seg_ptr || !workspace) return HAN_E_BADARG;
    const SilPlan p = sil_plan(N, k);
    if (workspace_bytes < p.bytes) return HAN_E_WORKSPACE;
    char *ws = (char *)workspace;
    float *xn = (float *)ws;
    double *ab = (double *)(ws + p.off_ab), *part = (double *)(ws + p.off_part);
    double *slab = p.nsplit > 1 ? (double *)(ws + p.off_slab) : nullptr;
    row_norms<<<norms_grid(N), kBlock, 0, st>>>(X, ldx, N, D, xn);
    HAN_CHECK_LAUNCH();
    SilArgs t;
    t.X = X; t.xn = xn; t.seg = seg_ptr; t.ldx = ldx; t.N = N; t.split_rows = p.split_rows; t.D = D; t.k = k;
    t.slab = slab; t.ab = ab;
    sil_tiles<<<dim3((unsigned)((N + kTile - 1) / kTile), (unsigned)p.nsplit), kBlock, 0, st>>>(t);
    HAN_CHECK_LAUNCH();
    sil_finish<<<(unsigned)p.finish_blocks, kBlock, 0, st>>>(seg_ptr, k, N, slab, p.nsplit, ab, a, b, s, part);
    HAN_CHECK_LAUNCH();
    sil_total<<<1, kBlock, 0, st>>>(part, p.finish_blocks, sum);
    HAN_CHECK_LAUNCH();
    return 0;
}
