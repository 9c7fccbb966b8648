// K0: ego blocks -- the neighbourhood of a batch of seed nodes cut out of the meta-path graphs (han_amd/minibatch.py).
//
// ego_expand   one breadth-first hop over one graph: every row at level h stamps h + 1 on its unvisited columns.
// ego_count    entries of every block row: the whole stored row where it is kept, one (r, r) entry on the rim.
// ego_fill     the block rows: columns through the local-id map, stored order / repeats / values as they are.
//
// Integer loads and stores only.  All writers of a word write the same value in a launch (expand) or own their
// positions (fill), so the results are bitwise the same from run to run.  Rows longer than split_deg are served by the
// chunk table of the INPUT graph (CSRGraph.row_split: built once per graph), a wave per chunk; every other row by a
// wave, lanes striding the entries (coalesced colidx / values; the one random access is level[col] / local[col]).
#include "han_common.h"

namespace {

constexpr int kBlock = 256;          // four waves
constexpr int kWaves = kBlock / 64;
constexpr int kCap = 8192;           // persistent grids: waves stride over their items

struct EgoLong {                     // han_row_split_t's chunk table of the input graph (n_chunks == 0: none)
    int64_t split_deg, n_chunks;
    const int64_t *long_rows;
    const int32_t *chunk_long;
    const int64_t *chunk_start, *chunk_end;
};

__device__ __forceinline__ void expand_entries(const int32_t *__restrict__ colidx, int64_t e0, int64_t e1, int lane,
                                               int64_t n, int32_t next, int32_t *level) {
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int64_t c = colidx[e];
        if ((uint64_t)c < (uint64_t)n && level[c] < 0) level[c] = next;
    }
}

// A wave takes 64 consecutive rows: one coalesced read of their levels, then it walks the rows at level h one by one.
// A word only ever changes from -1 to h + 1 in this launch, so no row joins or leaves the set {level == h} under it.
__global__ __launch_bounds__(kBlock) void ego_expand_rows(const int64_t *__restrict__ rowptr,
                                                          const int32_t *__restrict__ colidx, int64_t n, int32_t h,
                                                          int64_t split_deg, int32_t *level) {
    const int lane = threadIdx.x & 63;
    const int64_t n_groups = (n + 63) >> 6;
    for (int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; g < n_groups;
         g += (int64_t)gridDim.x * kWaves) {
        const int64_t i = g * 64 + lane;
        int64_t e0 = 0, e1 = 0;
        bool live = false;
        if (i < n && level[i] == h) {
            e0 = rowptr[i];
            e1 = rowptr[i + 1];
            live = e1 > e0 && (split_deg <= 0 || e1 - e0 <= split_deg);
        }
        uint64_t todo = __ballot(live);
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            expand_entries(colidx, __shfl(e0, src, 64), __shfl(e1, src, 64), lane, n, h + 1, level);
        }
    }
}

__global__ __launch_bounds__(kBlock) void ego_expand_chunks(const int32_t *__restrict__ colidx, int64_t n, int32_t h,
                                                            EgoLong t, int32_t *level) {
    const int lane = threadIdx.x & 63;
    for (int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; c < t.n_chunks;
         c += (int64_t)gridDim.x * kWaves) {
        const int64_t i = t.long_rows[t.chunk_long[c]];
        if ((uint64_t)i >= (uint64_t)n || level[i] != h) continue;
        expand_entries(colidx, t.chunk_start[c], t.chunk_end[c], lane, n, h + 1, level);
    }
}

// source row of block row r, or -1 when it is outside the input
__device__ __forceinline__ int64_t source_row(const int64_t *__restrict__ rows, int64_t r, int64_t n_in) {
    const int64_t v = rows[r];
    return (uint64_t)v < (uint64_t)n_in ? v : -1;
}

__device__ __forceinline__ bool row_kept(const int32_t *__restrict__ level, int64_t v, int32_t hops) {
    if (!level) return true;
    const int32_t l = level[v];
    return l >= 0 && l < hops;
}

__global__ __launch_bounds__(kBlock) void ego_count(const int64_t *__restrict__ rowptr,
                                                    const int64_t *__restrict__ rows,
                                                    const int32_t *__restrict__ level, int32_t hops, int64_t n_in,
                                                    int64_t n_out, int64_t *__restrict__ counts) {
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * kBlock) {
        const int64_t v = source_row(rows, r, n_in);
        int64_t c = 0;
        if (v >= 0) c = row_kept(level, v, hops) ? rowptr[v + 1] - rowptr[v] : 1;
        counts[r] = c;
    }
}

struct EgoFill {
    const int64_t *rowptr;
    const int32_t *colidx;
    const float *values;             // NULL: no values
    const int64_t *rows;
    const int32_t *level;            // NULL: every row is kept
    const int32_t *local;            // NULL: columns stay as they are
    int32_t hops;
    int64_t n_in, n_cols, n_out;
    const int64_t *out_rowptr;
    int32_t *out_colidx;
    float *out_values;
};

__device__ __forceinline__ void fill_entries(const EgoFill &a, int64_t e0, int64_t e1, int64_t o0, int lane) {
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        int32_t c = a.colidx[e];
        if (a.local) c = (uint32_t)c < (uint64_t)a.n_cols ? a.local[c] : -1;
        a.out_colidx[o0 + (e - e0)] = c;
        if (a.out_values) a.out_values[o0 + (e - e0)] = a.values ? a.values[e] : 1.0f;
    }
}

__global__ __launch_bounds__(kBlock) void ego_fill_rows(EgoFill a, int64_t split_deg) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; r < a.n_out;
         r += (int64_t)gridDim.x * kWaves) {
        const int64_t v = source_row(a.rows, r, a.n_in);
        if (v < 0) continue;
        const int64_t o0 = a.out_rowptr[r];
        if (!row_kept(a.level, v, a.hops)) {          // the rim: (r, r) alone
            if (lane == 0) {
                a.out_colidx[o0] = (int32_t)r;
                if (a.out_values) a.out_values[o0] = 1.0f;
            }
            continue;
        }
        const int64_t e0 = a.rowptr[v], e1 = a.rowptr[v + 1];
        if (split_deg > 0 && e1 - e0 > split_deg) continue;      // ego_fill_chunks
        fill_entries(a, e0, e1, o0, lane);
    }
}

// chunk c of the input graph's long row v lands at the same offset inside block row local[v]
__global__ __launch_bounds__(kBlock) void ego_fill_chunks(EgoFill a, EgoLong t) {
    const int lane = threadIdx.x & 63;
    for (int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6; c < t.n_chunks;
         c += (int64_t)gridDim.x * kWaves) {
        const int64_t v = t.long_rows[t.chunk_long[c]];
        if ((uint64_t)v >= (uint64_t)a.n_in || (uint64_t)v >= (uint64_t)a.n_cols || !row_kept(a.level, v, a.hops))
            continue;
        const int64_t r = a.local[v];
        if ((uint64_t)r >= (uint64_t)a.n_out) continue;
        const int64_t e0 = t.chunk_start[c];
        fill_entries(a, e0, t.chunk_end[c], a.out_rowptr[r] + (e0 - a.rowptr[v]), lane);
    }
}

int set_long(EgoLong &t, int64_t split_deg, int64_t n_chunks, const int64_t *long_rows, const int32_t *chunk_long,
             const int64_t *chunk_start, const int64_t *chunk_end) {
    if (n_chunks < 0) return HAN_E_BADARG;
    if (n_chunks > 0 && (split_deg < 1 || !long_rows || !chunk_long || !chunk_start || !chunk_end)) return HAN_E_BADARG;
    t.split_deg = n_chunks > 0 ? split_deg : 0;
    t.n_chunks = n_chunks;
    t.long_rows = long_rows;
    t.chunk_long = chunk_long;
    t.chunk_start = chunk_start;
    t.chunk_end = chunk_end;
    return 0;
}

}  // namespace

extern "C" int han_ego_expand(const int64_t *rowptr, const int32_t *colidx, int64_t n, int h, int64_t split_deg,
                              int64_t n_chunks, const int64_t *long_rows, const int32_t *chunk_long,
                              const int64_t *chunk_start, const int64_t *chunk_end, int32_t *level, void *stream) {
    if (!rowptr || !level || n < 0 || n > INT32_MAX || h < 0 || h == INT32_MAX) return HAN_E_BADARG;
    EgoLong t;
    if (const int e = set_long(t, split_deg, n_chunks, long_rows, chunk_long, chunk_start, chunk_end)) return e;
    if (n == 0 || !colidx) return 0;
    const hipStream_t st = (hipStream_t)stream;
    ego_expand_rows<<<han_grid_for((n + 63) / 64, kWaves, kCap), kBlock, 0, st>>>(rowptr, colidx, n, (int32_t)h,
                                                                                t.split_deg, level);
    HAN_CHECK_LAUNCH();
    if (t.n_chunks) {
        ego_expand_chunks<<<han_grid_for(t.n_chunks, kWaves, kCap), kBlock, 0, st>>>(colidx, n, (int32_t)h, t, level);
        HAN_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int han_ego_count(const int64_t *rowptr, const int64_t *rows, const int32_t *level, int hops, int64_t n_in,
                             int64_t n_out, int64_t *counts, void *stream) {
    if (!rowptr || n_in < 0 || n_out < 0 || (level && hops < 1)) return HAN_E_BADARG;
    if (n_out == 0) return 0;
    if (!rows || !counts) return HAN_E_BADARG;
    ego_count<<<han_grid_for(n_out, kBlock, kCap), kBlock, 0, (hipStream_t)stream>>>(rowptr, rows, level, (int32_t)hops,
                                                                                    n_in, n_out, counts);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_ego_fill(const int64_t *rowptr, const int32_t *colidx, const float *values, const int64_t *rows,
                            const int32_t *level, int hops, const int32_t *local, int64_t n_in, int64_t n_cols,
                            int64_t n_out, int64_t split_deg, int64_t n_chunks, const int64_t *long_rows,
                            const int32_t *chunk_long, const int64_t *chunk_start, const int64_t *chunk_end,
                            const int64_t *out_rowptr, int32_t *out_colidx, float *out_values, void *stream) {
    if (!rowptr || n_in < 0 || n_out < 0 || n_cols < 0 || n_cols > INT32_MAX || n_out > INT32_MAX ||
        (level && hops < 1))
        return HAN_E_BADARG;
    EgoLong t;
    if (const int e = set_long(t, split_deg, n_chunks, long_rows, chunk_long, chunk_start, chunk_end)) return e;
    if (t.n_chunks && !local) return HAN_E_BADARG;       // a chunk finds its block row through the map
    if (n_out == 0) return 0;
    if (!rows || !out_rowptr || !out_colidx) return HAN_E_BADARG;
    EgoFill a;
    a.rowptr = rowptr; a.colidx = colidx; a.values = values; a.rows = rows; a.level = level; a.local = local;
    a.hops = (int32_t)hops; a.n_in = n_in; a.n_cols = n_cols; a.n_out = n_out;
    a.out_rowptr = out_rowptr; a.out_colidx = out_colidx; a.out_values = out_values;
    const hipStream_t st = (hipStream_t)stream;
    ego_fill_rows<<<han_grid_for(n_out, kWaves, kCap), kBlock, 0, st>>>(a, t.split_deg);
    HAN_CHECK_LAUNCH();
    if (t.n_chunks) {
        ego_fill_chunks<<<han_grid_for(t.n_chunks, kWaves, kCap), kBlock, 0, st>>>(a, t);
        HAN_CHECK_LAUNCH();
    }
    return 0;
}
