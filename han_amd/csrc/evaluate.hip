// Evaluation of the final embeddings on the GPU (jhyexp.py:20-86): brute-force k nearest neighbours with a
// majority vote, contingency tables for F1 / NMI / ARI, one Lloyd iteration of k-means, the silhouette score of a
// clustering (data/exp.py:46-49), and exact t-SNE in two dimensions (sklearn.manifold, jhyexp.py:16).
//
// Distances are d2 = |q|^2 + |t|^2 - 2 q.t.  The q.t term runs on the exact-fp32 matrix pipe
// (v_mfma_f32_16x16x4_f32) in tiles of 64 x 64 pairs per workgroup step; the distance matrix never exists in
// memory: a lane sees its 16 candidates of a tile in registers and keeps a sorted list of the best ones.
//
// Tile layout (all six tile kernels).  A workgroup of 4 waves stages 64 "column" rows (queries / data rows) and 64 "row"
// rows (train rows / centres), 64 embedding columns at a time, into LDS as [64][kLd] fp32, zero-filled past the
// matrix edges and past D (so a D that is no multiple of 4 is padded in LDS, never in memory).  Wave w owns the
// column rows 16 w .. 16 w + 15 and walks all 64 row rows as four 16 x 16 accumulators.  The MFMA sums over its K
// index, so WHICH four embedding columns a lane group feeds per step is free as long as both operands agree: lane
// group g = lane >> 4 takes columns 16 g + 4 s .. + 3 in step s, one ds_read_b128 per operand and four MFMAs.
// Result map: lane (n = lane & 15, g) holds, in acc[j][r], the product of column row 16 w + n and row row
// 16 j + 4 g + r.
//
// Written once and shared (the roundings of this file are pinned bit for bit; a second copy is where one drifts):
//   TilePos, pair_product   a lane's place, and one 64 x 64 tile of q.t over all stages of D with the row rows' norms:
//                           knn_tiles, sil_tiles, tsne_rowmin / calib / step_tiles (kmeans_assign: see its comment)
//   for_pairs               the walk of a lane's 16 pairs: knn_tiles, sil_tiles, tsne_rowmin_tiles, tsne_calib_tiles
//                           (tsne_step_tiles and kmeans_assign: see there)
//   d2_norms, tsne_d2       the two forms of a pair's distance; they round differently, on purpose
//   row4_sum                the four lanes of a column row: sil_tiles, tsne_calib_tiles, tsne_step_tiles
//   block_sums              the workgroup's sum in thread order: sil_finish, tsne_rowsum_parts, block_totals,
//                           tsne_update (two values behind one barrier); kmeans_assign keeps its own (see there)
// Host side: one plan per entry-point family (knn_plan, kmeans_plan, sil_plan, tsne_plan), laid out with Regions and
// read by both the *_workspace function and the entry point; norms_and_grid launches row_norms and gives a tile
// kernel's (row tiles, splits) grid.
#include <utility>

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
__device__ __forceinline__ void mma_chunk(float4_t (&acc)[4], const float *Rs, const float *Cs, int w, int lane, int nj) {
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

// a lane's place: workgroup (x, y) takes the column rows [q0, q0 + 64) against the row rows [t_begin, t_end) of n_rows,
// this lane the column row myq
struct TilePos {
    int lane, w, n, g;
    int64_t q0, t_begin, t_end, myq;
    __device__ __forceinline__ TilePos(int64_t split_rows, int64_t n_rows)
        : lane(threadIdx.x & 63), w(threadIdx.x >> 6), n(lane & 15), g(lane >> 4), q0((int64_t)blockIdx.x * kTile),
          t_begin((int64_t)blockIdx.y * split_rows), t_end(min(n_rows, t_begin + split_rows)), myq(q0 + 16 * w + n) {}
};

// the operands of pair_product: row rows [.., end) of M with their norms, and the n column rows of M
struct TileRows {
    const float *M, *norms;
    int64_t ld, end;
};
struct TileCols {
    const float *M;
    int64_t ld, n;
};

// acc = (row rows [t0, min(t0 + 64, R.end))) x (column tile q0) as mma_chunk leaves it, the row rows' norms in tns;
// `extra` stages what else the epilogue reads per row row between the same two barriers.  `staged`: the column tile
// is in LDS already (one stage: it is staged once per workgroup).  Returns the 16-row tiles in use; ALL4 issues all
// four whatever the tail, as knn_tiles always has (a tail-dependent count in its MFMA loop is a change to measure).
template <bool ALL4, class Extra>
__device__ __forceinline__ int pair_product(float4_t (&acc)[4], float *smem, float *tns, const TileRows R, const TileCols C,
                                            int D, int64_t q0, int64_t t0, bool &staged, Extra extra) {
    float *Rs = smem, *Cs = smem + kTile * kLd;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nch = (D + kChunk - 1) / kChunk;
    const int nj = ALL4 ? 4 : (int)((min(R.end - t0, (int64_t)kTile) + 15) >> 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();
        stage_tile(Rs, R.M, R.ld, t0, R.end, ch * kChunk, D);
        if (nch > 1 || !staged) stage_tile(Cs, C.M, C.ld, q0, C.n, ch * kChunk, D);
        if (ch == 0) {
            if (threadIdx.x < kTile) tns[threadIdx.x] = t0 + threadIdx.x < R.end ? R.norms[t0 + threadIdx.x] : 0.f;
            extra();
        }
        __syncthreads();
        mma_chunk(acc, Rs, Cs, w, lane, nj);
    }
    staged = true;
    return nj;
}

// f(j, r, tl, t) for the 16 pairs of a lane of group g in the tile at t0 whose row row t = t0 + tl lies before `end`:
// the product is acc[j][r], the row row's norm tns[tl]
template <class F>
__device__ __forceinline__ void for_pairs(int g, int64_t t0, int64_t end, F f) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tl = 16 * j + 4 * g + r;
            if (t0 + tl < end) f(j, r, tl, t0 + tl);
        }
}

// The two forms of a pair's d2 from the norms and the product.  d2_norms, of KNN, k-means and the silhouette: the
// plain expression, NOT clamped: the neighbours and the nearest centre are the smallest computed values under
// (d2, index), and a clamp would turn what cancellation left slightly negative into ties (the silhouette clamps where
// it takes the root).  tsne_d2, of every t-SNE kernel: an explicit fma, clamped at 0, because d2 - m feeds an exponent
// and the row minimum m must be the minimum of what the later passes see.  The two may differ in the last bit and
// each is pinned by bit-for-bit tests, so neither stands in for the other.
__device__ __forceinline__ float d2_norms(float qn, float tn, float dot) { return (qn + tn) - 2.f * dot; }
__device__ __forceinline__ float tsne_d2(float qn, float tn, float dot) {
    return fmaxf(__builtin_fmaf(-2.f, dot, qn + tn), 0.f);
}

// (g0 + g1) + (g2 + g3) of the four lanes of a column row, in every one of them
__device__ __forceinline__ double row4_sum(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// out[i * stride] = the workgroup's sum of v[i], the 256 threads in order (thread 0 adds them behind one barrier)
template <int NV>
__device__ __forceinline__ void block_sums(const double (&v)[NV], double *out, int64_t stride) {
    __shared__ double ps[NV][kBlock];
#pragma unroll
    for (int i = 0; i < NV; ++i) ps[i][threadIdx.x] = v[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) t[i] = 0.0;
        for (int e = 0; e < kBlock; ++e)
#pragma unroll
            for (int i = 0; i < NV; ++i) t[i] += ps[i][e];
#pragma unroll
        for (int i = 0; i < NV; ++i) out[i * stride] = t[i];
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
    const TilePos p(a.split_rows, a.Nt);
    const float qnorm = p.myq < a.Nq ? a.qn[p.myq] : 0.f;
    TopList<KC> top;
    top.init();
    bool staged = false;
    for (int64_t t0 = p.t_begin; t0 < p.t_end; t0 += kTile) {
        float4_t acc[4];
        pair_product<true>(acc, smem, tns, TileRows{a.T, a.tn, a.ldt, p.t_end}, TileCols{a.Q, a.ldq, a.Nq}, a.D, p.q0, t0,
                           staged, [] {});
        for_pairs(p.g, t0, p.t_end,
                  [&](int j, int r, int tl, int64_t t) { top.offer(d2_norms(qnorm, tns[tl], acc[j][r]), (int)t); });
    }
    // the four lanes of a query: groups 1..3 hand their lists to group 0 through LDS
    __syncthreads();
    float *md = smem;
    int *mi = reinterpret_cast<int *>(smem) + kBlock * KC;
    static_assert(2 * kBlock * kMaxK <= 2 * kTile * kLd, "merge lists fit the staging area");
#pragma unroll
    for (int j = 0; j < KC; ++j) { md[threadIdx.x * KC + j] = top.d[j]; mi[threadIdx.x * KC + j] = top.i[j]; }
    __syncthreads();
    if (p.g == 0 && p.myq < a.Nq) {
        for (int og = 1; og < 4; ++og) {
            const int src = (64 * p.w + 16 * og + p.n) * KC;
#pragma unroll
            for (int j = 0; j < KC; ++j) top.offer(md[src + j], mi[src + j]);
        }
        const int64_t o = ((int64_t)blockIdx.y * a.Nq + p.myq) * a.k;
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

// The product loop here is its own and not pair_product: the roles are swapped.  A workgroup walks data tiles, so the
// COLUMN operand (the data rows) is staged again for every tile, the row operand (all the centres: no tile of them to
// walk, no split) is what stays in LDS with one stage, and the centres' norms are loaded once per workgroup.  A flag
// for all that would make pair_product branch on its caller.  The walk and the ordered sum are spelled out too: on
// for_pairs and block_sums the k-means line at 10^6 rows missed the parent's spread in one of two A/B jobs (DESIGN).
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
                    const float d = d2_norms(xnorm, cns[ci], acc[j][r]);
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

// the tile arguments of a call on X against itself (silhouette, t-SNE): both operands of pair_product
struct SelfTiles {
    const float *X, *xn;
    int64_t ldx, N, split_rows;
    int D;
    __device__ __forceinline__ TileRows rows(int64_t end) const { return TileRows{X, xn, ldx, end}; }
    __device__ __forceinline__ TileCols cols() const { return TileCols{X, ldx, N}; }
};

// ---- silhouette (data/exp.py:46-49) -----------------------------------------------------------------------------
// S(i, c) = sum over the rows j of cluster c of |x_i - x_j|, for a row tile of 64 rows i against the column rows
// [blockIdx.y * split_rows, + split_rows).  The rows are grouped by cluster, so the column tiles are cut at the segment
// (and split) boundaries and a tile holds rows of ONE cluster: a lane adds the (at most 16) distances it sees of a
// tile in fp32 in a fixed order, adds that to its double sum of the cluster, and at the end of the cluster the four
// lanes of a row are added in a fixed order.  No accumulator is indexed by a label.
struct SilArgs {
    SelfTiles t;
    const int64_t *seg;      // (k + 1) segment bounds
    int k;
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
    const TilePos p(a.t.split_rows, a.t.N);
    const int64_t N = a.t.N, myq = p.myq;
    if (threadIdx.x <= a.k) segs[threadIdx.x] = a.seg[threadIdx.x];
    const float qnorm = myq < N ? a.t.xn[myq] : 0.f;
    double s_own = 0.0, best = __builtin_inf();
    int64_t n_own = 0;
    bool staged = false;
    __syncthreads();
    for (int c = 0; c < a.k; ++c) {
        const int64_t c0 = segs[c], c1 = segs[c + 1];
        const int64_t lo = max(c0, p.t_begin), hi = min(c1, p.t_end);      // inside [0, N) whatever seg holds
        double S = 0.0;
        for (int64_t t0 = lo; t0 < hi; t0 += kTile) {
            float4_t acc[4];
            pair_product<false>(acc, smem, tns, a.t.rows(hi), a.t.cols(), a.t.D, p.q0, t0, staged, [] {});
            float part = 0.f;
            for_pairs(p.g, t0, hi, [&](int j, int r, int tl, int64_t t) {
                const float d2 = d2_norms(qnorm, tns[tl], acc[j][r]);
                part += t == myq ? 0.f : sqrtf(fmaxf(d2, 0.f));      // the pair (i, i) by its index
            });
            S += (double)part;
        }
        S = row4_sum(S);
        if (a.slab) {
            if (p.g == 0 && myq < N) a.slab[((size_t)blockIdx.y * a.k + c) * N + myq] = S;
        } else if (myq >= c0 && myq < c1) {
            s_own = S;
            n_own = c1 - c0;
        } else if (c1 > c0) {
            best = fmin(best, S / (double)(c1 - c0));
        }
    }
    if (!a.slab && p.g == 0 && myq < N) sil_ab(s_own, n_own, best, &a.ab[myq], &a.ab[N + myq]);
}

// a thread per row: a and b (from the slabs of the splits, added in order, when there are any), s, and the sum of
// the workgroup's s in row order
__global__ __launch_bounds__(kBlock) void sil_finish(const int64_t *seg, int k, int64_t N, const double *slab, int nsplit,
                                                    const double *ab, float *a_out, float *b_out, float *s_out,
                                                    double *part) {
    __shared__ int64_t segs[kMaxCentres + 1];
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
    block_sums({s}, &part[blockIdx.x], 0);
}

// workgroup b: out[b] = the partials part[b * nparts ..), each thread its own in order, then the 256 threads in order
__global__ __launch_bounds__(kBlock) void block_totals(const double *part, int64_t nparts, double *out) {
    double t = 0.0;
    for (int64_t e = threadIdx.x; e < nparts; e += kBlock) t += part[(int64_t)blockIdx.x * nparts + e];
    block_sums({t}, &out[blockIdx.x], 0);
}

// ---- t-SNE (jhyexp.py:16, data/exp.py:20: sklearn.manifold, method="exact") ---------------------------------------
// Row tile i against the column rows [blockIdx.y * split_rows, + split_rows), as sil_tiles walks them.  Nothing of
// N x N is stored: a calibration pass and a gradient step both form d2 per pair again, and the step forms p_ij from
// three floats per row (beta, the row minimum m of d2, the sum Z of that row's kernel).  A lane adds the at most 16
// pairs it sees of a tile in fp32, carries its sums in double across tiles, and the four lanes of a row are added in a
// fixed order; every (row, split) sum goes to a slab and the per-row kernels add the slabs in split order.
constexpr int kTsneSums = 5;       // per row and split: A (2), R (2), W
constexpr int kTsneSumsKL = 7;     // + sum e p (log e p - log w), sum e p
constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kFltMax = 3.402823466e+38f, kFltMin = 1.175494351e-38f;

// the beta a pass evaluates for the bisection state `next` (negative: a closed row's), inside the finite fp32 range
__device__ __forceinline__ float tsne_beta32(double next) {
    return fminf(fmaxf((float)fabs(next), kFltMin), kFltMax);
}

// beta * log2(e), finite: exp(-beta x) = exp2(-(this) x), and 0 * this = 0 for the nearest neighbour
__device__ __forceinline__ float tsne_bl2(float beta) { return fminf(beta * kLog2e, kFltMax); }

// m_i = min over j != i of d2_ij, per split
__global__ __launch_bounds__(kBlock) void tsne_rowmin_tiles(const SelfTiles a, float *slab /* [split][N] */) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTile * kLd];
    __shared__ float tns[kTile];
    const TilePos p(a.split_rows, a.N);
    const int64_t myq = p.myq;
    const float qnorm = myq < a.N ? a.xn[myq] : 0.f;
    float best = __builtin_inff();
    bool staged = false;
    for (int64_t t0 = p.t_begin; t0 < p.t_end; t0 += kTile) {
        float4_t acc[4];
        pair_product<false>(acc, smem, tns, a.rows(p.t_end), a.cols(), a.D, p.q0, t0, staged, [] {});
        for_pairs(p.g, t0, p.t_end, [&](int j, int r, int tl, int64_t t) {
            if (t != myq) best = fminf(best, tsne_d2(qnorm, tns[tl], acc[j][r]));
        });
    }
    best = fminf(best, __shfl_xor(best, 16, 64));
    best = fminf(best, __shfl_xor(best, 32, 64));
    if (p.g == 0 && myq < a.N) slab[(size_t)blockIdx.y * a.N + myq] = best;
}

// a thread per row: the minimum over the splits, and the bisection's start (beta = 1, no bound yet)
__global__ __launch_bounds__(kBlock) void tsne_calib_init(const float *slab, int nsplit, int64_t N, float *dmin, double *state) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    float m = __builtin_inff();
    for (int sp = 0; sp < nsplit; ++sp) m = fminf(m, slab[(size_t)sp * N + i]);
    dmin[i] = m;
    state[i] = 1.0;
    state[N + i] = -__builtin_inf();
    state[2 * N + i] = __builtin_inf();
}

// Z_i = sum_j exp(-beta_i (d2_ij - m_i)) and E_i = sum_j (d2_ij - m_i) exp(..) at the beta the state asks for
__global__ __launch_bounds__(kBlock) void tsne_calib_tiles(const SelfTiles a, const double *state, const float *dmin,
                                                           double *slab /* [split][2][N] */) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTile * kLd];
    __shared__ float tns[kTile];
    const TilePos p(a.split_rows, a.N);
    const int64_t myq = p.myq;
    const bool mine = myq < a.N;
    const float qnorm = mine ? a.xn[myq] : 0.f;
    const float m = mine ? dmin[myq] : 0.f;
    const float nbl2 = mine ? -tsne_bl2(tsne_beta32(state[myq])) : 0.f;
    double Z = 0.0, E = 0.0;
    bool staged = false;
    for (int64_t t0 = p.t_begin; t0 < p.t_end; t0 += kTile) {
        float4_t acc[4];
        pair_product<false>(acc, smem, tns, a.rows(p.t_end), a.cols(), a.D, p.q0, t0, staged, [] {});
        float z = 0.f, e = 0.f;
        for_pairs(p.g, t0, p.t_end, [&](int j, int r, int tl, int64_t col) {
            if (col != myq) {
                const float x = fmaxf(tsne_d2(qnorm, tns[tl], acc[j][r]) - m, 0.f);
                const float t = __builtin_amdgcn_exp2f(nbl2 * x);
                z += t;
                e = __builtin_fmaf(x, t, e);
            }
        });
        Z += (double)z;
        E += (double)e;
    }
    Z = row4_sum(Z);
    E = row4_sum(E);
    if (p.g == 0 && mine) {
        slab[((size_t)blockIdx.y * 2 + 0) * a.N + myq] = Z;
        slab[((size_t)blockIdx.y * 2 + 1) * a.N + myq] = E;
    }
}

// a thread per open row: Z and E from the slabs in split order, H = log Z + beta E / Z, one step of
// _binary_search_perplexity in double.  A row within tol of the target is closed: state[0] = -beta.  beta / zsum get
// the beta this pass evaluated and its Z; *open_rows (cleared before) counts the rows still open.
__global__ __launch_bounds__(kBlock) void tsne_calib_update(const double *slab, int nsplit, int64_t N, double log_perp, double tol,
                                                            double *state, float *beta, float *zsum,
                                                            unsigned long long *open_rows) {
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const double next = i < N ? state[i] : -1.0;
    if (next > 0.0) {
        double Z = 0.0, E = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) {
            Z += slab[((size_t)sp * 2 + 0) * N + i];
            E += slab[((size_t)sp * 2 + 1) * N + i];
        }
        const float bf = tsne_beta32(next);
        const double diff = (log(Z) + (double)bf * E / Z) - log_perp;
        beta[i] = bf;
        zsum[i] = (float)Z;
        if (fabs(diff) <= tol) {
            state[i] = -(double)bf;
        } else {
            double lo = state[N + i], hi = state[2 * N + i], b = next;
            if (diff > 0.0) {
                lo = b;
                b = hi == __builtin_inf() ? b * 2.0 : (b + hi) * 0.5;
            } else {
                hi = b;
                b = lo == -__builtin_inf() ? b * 0.5 : (b + lo) * 0.5;
            }
            state[i] = b;
            state[N + i] = lo;
            state[2 * N + i] = hi;
            atomicAdd(&cnt, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(open_rows, (unsigned long long)cnt);
}

struct TsneStepArgs {
    SelfTiles t;
    const float *beta, *dmin, *zsum, *Y;
    float scale, floor;      // e / (2 N) and e 2^-52: e p_ij = max((c_ij + c_ji) scale, floor)
    double *slab;            // [split][kTsneSums or kTsneSumsKL][N]
};

// what a lane adds up over its pairs of one tile
struct TsnePairSums {
    float a0, a1, r0, r1, w, k1, k2;
};

// One pair of the step.  Every rounding is written out, so the sums of the KL form are bit for bit those of the
// plain form.  cj: (bl2, m, 1 / Z) of the column row; on = false for the pair (i, i) and past the last row.
template <bool KL>
__device__ __forceinline__ void tsne_pair(TsnePairSums &s, float d2, float nbl2_i, float m_i, float iz_i, float nbl2_j, float m_j,
                                          float iz_j, float dy0, float dy1, bool on, float scale, float floor) {
#pragma clang fp contract(off)
    const float ei = __builtin_amdgcn_exp2f(nbl2_i * fmaxf(d2 - m_i, 0.f));
    const float ej = __builtin_amdgcn_exp2f(nbl2_j * fmaxf(d2 - m_j, 0.f));
    const float ep = fmaxf(__builtin_fmaf(ei, iz_i, ej * iz_j) * scale, floor);
    const float w = on ? __builtin_amdgcn_rcpf(__builtin_fmaf(dy0, dy0, __builtin_fmaf(dy1, dy1, 1.f))) : 0.f;
    const float pw = ep * w, w2 = w * w;
    s.a0 = __builtin_fmaf(pw, dy0, s.a0);
    s.a1 = __builtin_fmaf(pw, dy1, s.a1);
    s.r0 = __builtin_fmaf(w2, dy0, s.r0);
    s.r1 = __builtin_fmaf(w2, dy1, s.r1);
    s.w += w;
    if (KL && on) {
        s.k1 = __builtin_fmaf(ep, __logf(ep) - __logf(w), s.k1);
        s.k2 += ep;
    }
}

template <bool KL>
__global__ __launch_bounds__(kBlock) void tsne_step_tiles(const TsneStepArgs a) {
    constexpr int NS = KL ? kTsneSumsKL : kTsneSums;
    __shared__ __attribute__((aligned(16))) float smem[2 * kTile * kLd];
    __shared__ __attribute__((aligned(16))) float cp[6][kTile];      // column rows: norm, -beta log2 e, m, 1 / Z, y0, y1
    const TilePos p(a.t.split_rows, a.t.N);
    const int w = p.w, g = p.g;
    const int64_t N = a.t.N, t_end = p.t_end, myq = p.myq;
    const bool mine = myq < N;
    const float qnorm = mine ? a.t.xn[myq] : 0.f;
    const float nbl2 = mine ? -tsne_bl2(a.beta[myq]) : 0.f, m = mine ? a.dmin[myq] : 0.f;
    const float iz = mine ? 1.f / a.zsum[myq] : 0.f;
    const float y0 = mine ? a.Y[2 * myq] : 0.f, y1 = mine ? a.Y[2 * myq + 1] : 0.f;
    double sum[NS];
#pragma unroll
    for (int e = 0; e < NS; ++e) sum[e] = 0.0;
    bool staged = false;
    for (int64_t t0 = p.t_begin; t0 < t_end; t0 += kTile) {
        float4_t acc[4];
        const int nj = pair_product<false>(acc, smem, cp[0], a.t.rows(t_end), a.t.cols(), a.t.D, p.q0, t0, staged, [&] {
            const int r = threadIdx.x & 63;
            const int64_t row = t0 + r;
            const bool in = row < t_end;
            if (w == 1) {
                cp[1][r] = in ? -tsne_bl2(a.beta[row]) : 0.f;
                cp[2][r] = in ? a.dmin[row] : 0.f;
            } else if (w == 2) {
                cp[3][r] = in ? 1.f / a.zsum[row] : 0.f;
            } else if (w == 3) {
                cp[4][r] = in ? a.Y[2 * row] : 0.f;
                cp[5][r] = in ? a.Y[2 * row + 1] : 0.f;
            }
        });
        TsnePairSums s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // not for_pairs: six column vectors are read once per 16-row tile, and the walk ends at the last tile in use
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nj) break;
            float4_t c[6];
#pragma unroll
            for (int e = 0; e < 6; ++e) c[e] = *reinterpret_cast<const float4_t *>(&cp[e][16 * j + 4 * g]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t col = t0 + 16 * j + 4 * g + r;
                tsne_pair<KL>(s, tsne_d2(qnorm, c[0][r], acc[j][r]), nbl2, m, iz, c[1][r], c[2][r], c[3][r], y0 - c[4][r],
                              y1 - c[5][r], col < t_end && col != myq, a.scale, a.floor);
            }
        }
        sum[0] += (double)s.a0;
        sum[1] += (double)s.a1;
        sum[2] += (double)s.r0;
        sum[3] += (double)s.r1;
        sum[4] += (double)s.w;
        if (KL) {
            sum[5] += (double)s.k1;
            sum[6] += (double)s.k2;
        }
    }
#pragma unroll
    for (int e = 0; e < NS; ++e) {
        const double v = row4_sum(sum[e]);
        if (g == 0 && mine) a.slab[((size_t)blockIdx.y * NS + e) * N + myq] = v;
    }
}

// W_i from the slabs in split order, and the sum of a workgroup's rows in row order
__global__ __launch_bounds__(kBlock) void tsne_rowsum_parts(const double *slab, int nsplit, int ns, int64_t N, double *part) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double s = 0.0;
    if (i < N)
        for (int sp = 0; sp < nsplit; ++sp) s += slab[((size_t)sp * ns + 4) * N + i];
    block_sums({s}, &part[blockIdx.x], 0);
}

// _gradient_descent's update of one coordinate, every product and sum rounded on its own; returns gains * grad
__device__ __forceinline__ float tsne_descend(float g, float *y, float *upd, float *gain, float momentum, float lr, float min_gain) {
#pragma clang fp contract(off)
    const float u = *upd;
    float gn = *gain;
    gn = __fmul_rn(u, g) < 0.f ? __fadd_rn(gn, 0.2f) : __fmul_rn(gn, 0.8f);
    gn = fmaxf(gn, min_gain);
    const float gg = __fmul_rn(gn, g);
    const float un = __fsub_rn(__fmul_rn(momentum, u), __fmul_rn(lr, gg));
    *gain = gn;
    *upd = un;
    *y = __fadd_rn(*y, un);
    return gg;
}

struct TsneUpdateArgs {
    const double *slab, *zq;
    int nsplit, ns;
    int64_t N, nparts;
    float *Y, *update, *gains, *grad;
    float momentum, lr, min_gain;
    double *part;            // [2][nparts]: sum of (gains * grad)^2, KL terms
};

// a thread per row: A and R from the slabs in split order, grad = 4 (A - R / Z_q), the update rule, and the
// workgroup's partials of |gains * grad|^2 and of the KL sum in row order
__global__ __launch_bounds__(kBlock) void tsne_update(const TsneUpdateArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double nrm = 0.0, kl = 0.0;
    if (i < a.N) {
        double s[kTsneSumsKL] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int sp = 0; sp < a.nsplit; ++sp)
#pragma unroll
            for (int e = 0; e < kTsneSumsKL; ++e)
                if (e != 4 && e < a.ns) s[e] += a.slab[((size_t)sp * a.ns + e) * a.N + i];
        const double zq = *a.zq;
        for (int c = 0; c < 2; ++c) {
            const float g = (float)(4.0 * (s[c] - s[2 + c] / zq));
            if (a.grad) a.grad[2 * i + c] = g;
            const float gg = tsne_descend(g, a.Y + 2 * i + c, a.update + 2 * i + c, a.gains + 2 * i + c, a.momentum, a.lr,
                                          a.min_gain);
            nrm += (double)gg * (double)gg;
        }
        kl = s[5] + log(zq) * s[6];
    }
    block_sums({nrm, kl}, a.part + blockIdx.x, a.nparts);
}

// a workspace, region by region: add() gives the next region's offset; every region starts on a 256-byte boundary
struct Regions {
    size_t bytes = 0;
    size_t add(size_t b) { return std::exchange(bytes, bytes + ((b + 255) & ~(size_t)255)); }
};

// |row|^2 of M's n rows into `out`; returns the grid of a tile kernel with them on the column axis: (row tiles, splits)
inline dim3 norms_and_grid(const float *M, int64_t ld, int64_t n, int D, float *out, int nsplit, hipStream_t st) {
    row_norms<<<han_grid_for(n, kBlock / 16, 8192), kBlock, 0, st>>>(M, ld, n, D, out);
    return dim3((unsigned)((n + kTile - 1) / kTile), (unsigned)nsplit);
}

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

// Every workspace starts with the norms of the column rows (offset 0).  KNN: then the train rows' norms and, with more
// than one split, the splits' lists [split][Nq][k]: indices, then distances.
struct KnnPlan {
    int64_t split_rows;
    int nsplit;
    size_t off_tn, off_idx, off_d2, bytes;
};

inline KnnPlan knn_plan(int64_t Nq, int64_t Nt, int k) {
    KnnPlan p;
    Regions r;
    p.nsplit = knn_splits(Nq, Nt, &p.split_rows);
    const size_t lists = p.nsplit > 1 ? (size_t)p.nsplit * Nq * k * sizeof(float) : 0;
    r.add((size_t)Nq * sizeof(float));
    p.off_tn = r.add((size_t)Nt * sizeof(float));
    p.off_idx = r.add(lists);
    p.off_d2 = r.add(lists);
    p.bytes = r.bytes;
    return p;
}

struct KmeansPlan {
    int64_t tiles, tiles_per_block, rows_per_block;
    int assign_blocks, sum_blocks, dp;
    size_t off_cn, off_part, off_slab, bytes;
};

inline KmeansPlan kmeans_plan(int64_t N, int D, int k) {
    KmeansPlan p;
    Regions r;
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
    r.add((size_t)N * sizeof(float));
    p.off_cn = r.add(kMaxCentres * sizeof(float));
    p.off_part = r.add((size_t)kAssignCap * sizeof(double));
    p.off_slab = r.add((size_t)p.sum_blocks * slab_bytes);
    p.bytes = r.bytes;
    return p;
}

// the column range of a silhouette call is split like the train set of a KNN call; slabs only with more than one split
struct SilPlan {
    int64_t split_rows, finish_blocks;
    int nsplit;
    size_t off_ab, off_part, off_slab, bytes;
};

inline SilPlan sil_plan(int64_t N, int k) {
    SilPlan p;
    Regions r;
    p.nsplit = knn_splits(N, N, &p.split_rows);
    p.finish_blocks = (N + kBlock - 1) / kBlock;
    r.add((size_t)N * sizeof(float));
    p.off_ab = r.add((size_t)2 * N * sizeof(double));
    p.off_part = r.add((size_t)p.finish_blocks * sizeof(double));
    p.off_slab = r.add(p.nsplit > 1 ? (size_t)p.nsplit * k * N * sizeof(double) : 0);
    p.bytes = r.bytes;
    return p;
}

// t-SNE: the column range is split as in han_silhouette; every (row, split) sum goes through a slab
struct TsnePlan {
    int64_t split_rows, row_blocks;
    int nsplit;
    size_t off_part, off_slab, bytes;
};

inline TsnePlan tsne_plan(int64_t N) {
    TsnePlan p;
    Regions r;
    p.nsplit = knn_splits(N, N, &p.split_rows);
    p.row_blocks = (N + kBlock - 1) / kBlock;
    r.add((size_t)N * sizeof(float));
    p.off_part = r.add((size_t)2 * p.row_blocks * sizeof(double));
    p.off_slab = r.add((size_t)p.nsplit * kTsneSumsKL * N * sizeof(double));
    p.bytes = r.bytes;
    return p;
}

}  // namespace

extern "C" size_t han_knn_topk_workspace(int64_t Nq, int64_t Nt, int D, int k) {
    if (Nq <= 0 || Nt <= 0 || D < 1 || k < 1) return 0;
    return knn_plan(Nq, Nt, k).bytes;
}

extern "C" int han_knn_topk(const float *Q, int64_t ldq, const float *T, int64_t ldt, int32_t *idx, float *d2,
                            void *workspace, size_t workspace_bytes, int64_t Nq, int64_t Nt, int D, int k,
                            void *stream) {
    if (Nq < 0 || Nt < 0 || D < 1 || k < 1 || ldq < D || ldt < D || k > Nt) return HAN_E_BADARG;
    if (k > kMaxK || D > kMaxD || Nt > 0x7FFFFFFF) return HAN_E_UNSUPPORTED;
    if (Nq == 0) return 0;
    if (!Q || !T || !idx || !d2 || !workspace) return HAN_E_BADARG;
    const KnnPlan p = knn_plan(Nq, Nt, k);
    if (workspace_bytes < p.bytes) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int ns = p.nsplit;
    char *ws = (char *)workspace;
    float *qn = (float *)ws, *tn = (float *)(ws + p.off_tn);
    const dim3 grid = norms_and_grid(Q, ldq, Nq, D, qn, ns, st);
    HAN_CHECK_LAUNCH();
    norms_and_grid(T, ldt, Nt, D, tn, 1, st);
    HAN_CHECK_LAUNCH();
    const KnnArgs a = {Q, T, qn, tn, ldq, ldt, Nq, Nt, p.split_rows, D, k,
                       ns > 1 ? (int32_t *)(ws + p.off_idx) : idx, ns > 1 ? (float *)(ws + p.off_d2) : d2};
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
    norms_and_grid(X, ldx, N, D, xn, 1, st);
    HAN_CHECK_LAUNCH();
    norms_and_grid(C, D, k, D, cn, 1, st);
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
    const dim3 grid = norms_and_grid(X, ldx, N, D, xn, p.nsplit, st);
    HAN_CHECK_LAUNCH();
    const SilArgs t = {{X, xn, ldx, N, p.split_rows, D}, seg_ptr, k, slab, ab};
    sil_tiles<<<grid, kBlock, 0, st>>>(t);
    HAN_CHECK_LAUNCH();
    sil_finish<<<(unsigned)p.finish_blocks, kBlock, 0, st>>>(seg_ptr, k, N, slab, p.nsplit, ab, a, b, s, part);
    HAN_CHECK_LAUNCH();
    block_totals<<<1, kBlock, 0, st>>>(part, p.finish_blocks, sum);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t han_tsne_workspace(int64_t N, int D) {
    if (N <= 0 || D < 1 || D > kMaxD || N > 0x7FFFFFFF) return 0;
    return tsne_plan(N).bytes;
}

extern "C" int han_tsne_calibrate(const float *X, int64_t ldx, int64_t N, int D, float perplexity, float tol, int steps,
                                  int restart, float *beta, float *dmin, float *zsum, double *state, int64_t *open_rows,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    if (N < 0 || D < 1 || ldx < D || steps < 0) return HAN_E_BADARG;
    if (D > kMaxD || N > 0x7FFFFFFF) return HAN_E_UNSUPPORTED;
    if (N <= 1) return 0;
    if (!(perplexity >= 1.f) || !((double)perplexity < (double)N) || !(tol >= 0.f)) return HAN_E_BADARG;      // NaN: neither
    if (!X || !beta || !dmin || !zsum || !state || !open_rows || !workspace) return HAN_E_BADARG;
    const TsnePlan p = tsne_plan(N);
    if (workspace_bytes < p.bytes) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *xn = (float *)ws;
    double *slab = (double *)(ws + p.off_slab);
    const SelfTiles t = {X, xn, ldx, N, p.split_rows, D};
    const dim3 grid = norms_and_grid(X, ldx, N, D, xn, p.nsplit, st);
    HAN_CHECK_LAUNCH();
    if (restart) {
        tsne_rowmin_tiles<<<grid, kBlock, 0, st>>>(t, (float *)slab);
        HAN_CHECK_LAUNCH();
        tsne_calib_init<<<(unsigned)p.row_blocks, kBlock, 0, st>>>((const float *)slab, p.nsplit, N, dmin, state);
        HAN_CHECK_LAUNCH();
    }
    for (int s = 0; s < steps; ++s) {
        tsne_calib_tiles<<<grid, kBlock, 0, st>>>(t, state, dmin, slab);
        HAN_CHECK_LAUNCH();
        const hipError_t e = hipMemsetAsync(open_rows, 0, sizeof(int64_t), st);
        if (e != hipSuccess) return (int)e;
        tsne_calib_update<<<(unsigned)p.row_blocks, kBlock, 0, st>>>(slab, p.nsplit, N, log((double)perplexity), (double)tol,
                                                                    state, beta, zsum, (unsigned long long *)open_rows);
        HAN_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int han_tsne_step(const float *X, int64_t ldx, const float *beta, const float *dmin, const float *zsum, float *Y,
                             float *update, float *gains, float *grad, double *stats, int64_t N, int D,
                             float exaggeration, float momentum, float lr, float min_gain, int want_kl, void *workspace,
                             size_t workspace_bytes, void *stream) {
    if (N < 0 || D < 1 || ldx < D) return HAN_E_BADARG;
    if (D > kMaxD || N > 0x7FFFFFFF) return HAN_E_UNSUPPORTED;
    if (N <= 1) return 0;
    if (!(exaggeration > 0.f) || !(exaggeration < kFltMax)) return HAN_E_BADARG;
    if (!X || !beta || !dmin || !zsum || !Y || !update || !gains || !stats || !workspace) return HAN_E_BADARG;
    const TsnePlan p = tsne_plan(N);
    if (workspace_bytes < p.bytes) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *xn = (float *)ws;
    double *part = (double *)(ws + p.off_part), *slab = (double *)(ws + p.off_slab);
    const int ns = want_kl ? kTsneSumsKL : kTsneSums;
    const TsneStepArgs a = {{X, xn, ldx, N, p.split_rows, D}, beta, dmin, zsum, Y,
                            (float)((double)exaggeration / (2.0 * (double)N)), exaggeration * 0x1p-52f, slab};
    const dim3 grid = norms_and_grid(X, ldx, N, D, xn, p.nsplit, st);
    HAN_CHECK_LAUNCH();
    if (want_kl) tsne_step_tiles<true><<<grid, kBlock, 0, st>>>(a);
    else tsne_step_tiles<false><<<grid, kBlock, 0, st>>>(a);
    HAN_CHECK_LAUNCH();
    tsne_rowsum_parts<<<(unsigned)p.row_blocks, kBlock, 0, st>>>(slab, p.nsplit, ns, N, part);
    HAN_CHECK_LAUNCH();
    block_totals<<<1, kBlock, 0, st>>>(part, p.row_blocks, stats);
    HAN_CHECK_LAUNCH();
    TsneUpdateArgs u;
    u.slab = slab; u.zq = stats; u.nsplit = p.nsplit; u.ns = ns; u.N = N; u.nparts = p.row_blocks;
    u.Y = Y; u.update = update; u.gains = gains; u.grad = grad;
    u.momentum = momentum; u.lr = lr; u.min_gain = min_gain; u.part = part;
    tsne_update<<<(unsigned)p.row_blocks, kBlock, 0, st>>>(u);
    HAN_CHECK_LAUNCH();
    block_totals<<<want_kl ? 2 : 1, kBlock, 0, st>>>(part, p.row_blocks, stats + 1);
    HAN_CHECK_LAUNCH();
    return 0;
}
