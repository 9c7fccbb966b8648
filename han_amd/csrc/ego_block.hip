// K0: ego blocks -- the neighbourhood of a batch of seed nodes cut out of the meta-path graphs (han_amd/minibatch.py).
//
// ego_expand   one breadth-first hop over one graph: every row at level h stamps h + 1 on its unvisited columns.
// ego_count    entries of every block row: the whole stored row where it is kept, one (r, r) entry on the rim.
// ego_fill     the block rows: columns through the local-id map, stored order / repeats / values as they are.
// ego_sample_* the same three steps with a random fan-out per row ("sampled blocks" below).
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

// ---- sampled blocks: at most `fanout` entries per row besides the self entries ---------------------------------------
// (the rule: include/han_hip.h.)  The key of the entry at stored position k of row v is the first word of
// han_rand64(seed, HAN_STREAM_EGO * (graph + 1), v, k); a row with more than `fanout` entries off the diagonal keeps
// those of the `fanout` smallest (key, k).  ego_sample_expand decides a row once, at the hop that walks it -- an
// MSB-first radix select over a 256-bin LDS histogram, 8 bits per round, as csr_row_topk's (metapath.hip), finds the
// fanout-th smallest key `thr` and how many of the entries equal to it are still needed -- and stores (thr, need, kept
// count) under the row's global id; the fill pass draws the keys again and keeps the self entries, the keys below thr
// and the first `need` equal to it in stored order.  A block of G threads serves a row: G = 64 (a wave; 64 consecutive
// rows are looked at together, as in ego_expand_rows) up to split_deg entries, G = 256 for the rows of the long list.
// Every pass over a row hashes its entries again: a long row costs 6 passes in expand (self count, 4 rounds, stamp).
struct EgoSample {
    uint32_t seed_lo, seed_hi, stream;
    uint32_t *thr;                   // per global row, written by the hop that expands the row:
    int32_t *need;                   //   -1: the whole row is kept; else the entries with key == thr still needed
    int64_t *kept;                   //   entries of the sampled row
};

struct SampleLds {
    int hist[256];
    int wave[kWaves];
    int sel[2];
    int nself;
};

__device__ __forceinline__ uint32_t sample_key(const EgoSample &s, int64_t v, int64_t k) {
    return han_rand64(s.seed_lo, s.seed_hi, s.stream, (uint32_t)v, (uint32_t)k).x;
}

// how many threads of the block before this one raise the flag (every thread also gets the total)
template <int G>
__device__ __forceinline__ int flag_excl_scan(bool f, int *s_wave, int &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t b = __ballot(f);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (G == 64) {
        total = __popcll(b);
        return before;
    }
    if (lane == 0) s_wave[w] = __popcll(b);
    __syncthreads();
    int pre = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < G / 64; ++k) {
        pre += k < w ? s_wave[k] : 0;
        total += s_wave[k];
    }
    __syncthreads();
    return pre + before;
}

template <int G>
__device__ __forceinline__ bool block_any(bool f) {
    if (G == 64) return __ballot(f) != 0;
    return __syncthreads_or(f) != 0;
}

constexpr int kStep = 4;

// The decision of row v = [e0, e1), taken by the whole block (every branch is uniform over it).
template <int G>
__device__ __forceinline__ void sample_select(const int32_t *__restrict__ colidx, int64_t v, int64_t e0, int64_t e1,
                                              int32_t fanout, const EgoSample &s, SampleLds &m, uint32_t &thr,
                                              int32_t &need) {
    const int t = threadIdx.x;
    thr = 0u;
    need = -1;
    if (e1 - e0 <= fanout) {                  // nothing to cut, however many self entries there are
        if (t == 0) {
            s.thr[v] = 0u;
            s.need[v] = -1;
            s.kept[v] = e1 - e0;
        }
        return;
    }
    if (t == 0) m.nself = 0;
    __syncthreads();
    int nd = 0;
    for (int64_t e = e0 + t; e < e1; e += kStep * G) {        // kStep loads in flight per thread: a long row is
        int32_t c[kStep];                                      // bound by their latency, not by the hash
#pragma unroll
        for (int q = 0; q < kStep; ++q) c[q] = e + q * G < e1 ? colidx[e + q * G] : -1;
#pragma unroll
        for (int q = 0; q < kStep; ++q) nd += (int64_t)c[q] == v;
    }
    if (nd) atomicAdd(&m.nself, nd);
    __syncthreads();
    const int64_t nself = m.nself;
    __syncthreads();                          // nself is cleared for the next row
    if (e1 - e0 - nself > fanout) {
        uint32_t mask = 0u;
        need = fanout;
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int b = t; b < 256; b += G) m.hist[b] = 0;
            __syncthreads();
            for (int64_t e = e0 + t; e < e1; e += kStep * G) {
                int32_t c[kStep];
#pragma unroll
                for (int q = 0; q < kStep; ++q) c[q] = e + q * G < e1 ? colidx[e + q * G] : (int32_t)v;
#pragma unroll
                for (int q = 0; q < kStep; ++q) {
                    if ((int64_t)c[q] == v) continue;          // a self entry, or past the end
                    const uint32_t x = sample_key(s, v, e + q * G - e0);
                    if ((x & mask) == thr) atomicAdd(&m.hist[(x >> shift) & 255u], 1);
                }
            }
            __syncthreads();
            if (t < 64) {                      // the first wave: lane t owns the digits 4 t .. 4 t + 3, ascending
                const int mine = m.hist[4 * t] + m.hist[4 * t + 1] + m.hist[4 * t + 2] + m.hist[4 * t + 3];
                int incl = mine;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int y = __shfl_up(incl, d, 64);
                    if (t >= d) incl += y;
                }
                const int below = incl - mine;
                if (below < need && need <= below + mine) {               // exactly one lane
                    int left = need - below, d = 4 * t;
                    while (m.hist[d] < left) left -= m.hist[d++];
                    m.sel[0] = d;
                    m.sel[1] = left;
                }
            }
            __syncthreads();
            thr |= (uint32_t)m.sel[0] << shift;
            mask |= 255u << shift;
            need = m.sel[1];
            __syncthreads();                  // hist / sel are rewritten by the next round
        }
    }
    if (t == 0) {
        s.thr[v] = thr;
        s.need[v] = need;
        s.kept[v] = need < 0 ? e1 - e0 : (int64_t)fanout + nself;
    }
}

// emit(e, column, rank) for every kept entry of row v, rank = its position in the sampled row (RANK; else 0).
template <int G, bool RANK, typename Emit>
__device__ __forceinline__ void sample_walk(const int32_t *__restrict__ colidx, int64_t v, int64_t e0, int64_t e1,
                                            const EgoSample &s, uint32_t thr, int32_t need, int *s_wave, Emit emit) {
    const int t = threadIdx.x;
    if (need < 0) {
        for (int64_t e = e0 + t; e < e1; e += G) emit(e, colidx[e], e - e0);
        return;
    }
    int64_t ties = 0, pos = 0;
    for (int64_t c0 = e0; c0 < e1; c0 += kStep * G) {          // kStep runs of G entries: their loads together, and
        int32_t c[kStep];                                      // one vote skips the runs that keep nothing
        bool keep[kStep], tie[kStep], any = false;
#pragma unroll
        for (int q = 0; q < kStep; ++q) c[q] = c0 + q * G + t < e1 ? colidx[c0 + q * G + t] : 0;
#pragma unroll
        for (int q = 0; q < kStep; ++q) {
            const int64_t e = c0 + q * G + t;
            keep[q] = tie[q] = false;
            if (e < e1) {
                if ((int64_t)c[q] == v) keep[q] = true;
                else {
                    const uint32_t x = sample_key(s, v, e - e0);
                    keep[q] = x < thr;
                    tie[q] = x == thr;
                }
            }
            any = any || keep[q] || tie[q];
        }
        if (!block_any<G>(any)) continue;
#pragma unroll
        for (int q = 0; q < kStep; ++q) {                      // in stored order
            if (c0 + q * G >= e1) break;
            const int64_t e = c0 + q * G + t;
            int n_tie;
            const int tie_before = flag_excl_scan<G>(tie[q], s_wave, n_tie);
            const bool k = keep[q] || (tie[q] && ties + tie_before < need);
            ties += n_tie;
            if (RANK) {
                int n_keep;
                const int keep_before = flag_excl_scan<G>(k, s_wave, n_keep);
                if (k) emit(e, c[q], pos + keep_before);
                pos += n_keep;
            } else if (k) {
                emit(e, c[q], 0);
            }
        }
    }
}

template <int G>
__device__ __forceinline__ void sample_expand_row(const int32_t *__restrict__ colidx, int64_t v, int64_t e0,
                                                  int64_t e1, int64_t n, int32_t next, int32_t fanout,
                                                  const EgoSample &s, SampleLds &m, int32_t *level) {
    uint32_t thr;
    int32_t need;
    sample_select<G>(colidx, v, e0, e1, fanout, s, m, thr, need);
    sample_walk<G, false>(colidx, v, e0, e1, s, thr, need, m.wave, [&](int64_t, int32_t c, int64_t) {
        if ((uint64_t)c < (uint64_t)n && level[c] < 0) level[c] = next;
    });
}

// A wave (the block) takes 64 consecutive rows, as ego_expand_rows; an empty row is decided by its own lane.
__global__ __launch_bounds__(64) void ego_sample_expand_rows(const int64_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ colidx, int64_t n, int32_t h,
                                                             int32_t fanout, int64_t split_deg, EgoSample s,
                                                             int32_t *level) {
    __shared__ SampleLds m;
    const int lane = threadIdx.x;
    const int64_t n_groups = (n + 63) >> 6;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t i = g * 64 + lane;
        int64_t e0 = 0, e1 = 0;
        bool live = false;
        if (i < n && level[i] == h) {
            e0 = rowptr[i];
            e1 = rowptr[i + 1];
            live = e1 > e0 && (split_deg <= 0 || e1 - e0 <= split_deg);
            if (e1 <= e0) {
                s.thr[i] = 0u;
                s.need[i] = -1;
                s.kept[i] = 0;
            }
        }
        uint64_t todo = __ballot(live);
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            sample_expand_row<64>(colidx, g * 64 + src, __shfl(e0, src, 64), __shfl(e1, src, 64), n, h + 1, fanout, s,
                                  m, level);
        }
    }
}

__global__ __launch_bounds__(kBlock) void ego_sample_expand_long(const int64_t *__restrict__ rowptr,
                                                                 const int32_t *__restrict__ colidx, int64_t n,
                                                                 int32_t h, int32_t fanout, int64_t n_long,
                                                                 const int64_t *__restrict__ long_rows, EgoSample s,
                                                                 int32_t *level) {
    __shared__ SampleLds m;
    for (int64_t j = blockIdx.x; j < n_long; j += gridDim.x) {
        const int64_t i = long_rows[j];
        if ((uint64_t)i >= (uint64_t)n || level[i] != h) continue;
        sample_expand_row<kBlock>(colidx, i, rowptr[i], rowptr[i + 1], n, h + 1, fanout, s, m, level);
    }
}

__global__ __launch_bounds__(kBlock) void ego_sample_count(const int64_t *__restrict__ rows,
                                                           const int32_t *__restrict__ level, int32_t hops,
                                                           const int64_t *__restrict__ kept, int64_t n_in,
                                                           int64_t n_out, int64_t *__restrict__ counts) {
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n_out; r += (int64_t)gridDim.x * kBlock) {
        const int64_t v = source_row(rows, r, n_in);
        int64_t c = 0;
        if (v >= 0) c = row_kept(level, v, hops) ? kept[v] : 1;
        counts[r] = c;
    }
}

// Block row r = the kept entries of row v in stored order; no store at or beyond out_rowptr[r + 1], whatever the counts.
template <int G>
__device__ __forceinline__ void sample_fill_row(const EgoFill &a, const EgoSample &s, int64_t v, int64_t r, int64_t e0,
                                                int64_t e1, int *s_wave) {
    const int64_t o0 = a.out_rowptr[r], o_end = a.out_rowptr[r + 1];
    sample_walk<G, true>(a.colidx, v, e0, e1, s, s.thr[v], s.need[v], s_wave, [&](int64_t e, int32_t c, int64_t rank) {
        if (o0 + rank >= o_end) return;
        a.out_colidx[o0 + rank] = (uint32_t)c < (uint64_t)a.n_cols ? a.local[c] : -1;
        if (a.out_values) a.out_values[o0 + rank] = a.values ? a.values[e] : 1.0f;
    });
}

__global__ __launch_bounds__(64) void ego_sample_fill_rows(EgoFill a, EgoSample s, int64_t split_deg) {
    __shared__ int s_wave[kWaves];
    const int lane = threadIdx.x;
    const int64_t n_groups = (a.n_out + 63) >> 6;
    for (int64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const int64_t r = g * 64 + lane;
        const int64_t v = r < a.n_out ? source_row(a.rows, r, a.n_in) : -1;
        int64_t e0 = 0, e1 = 0;
        bool live = false;
        if (v >= 0) {
            if (!row_kept(a.level, v, a.hops)) {          // the rim: (r, r) alone
                const int64_t o0 = a.out_rowptr[r];
                if (o0 < a.out_rowptr[r + 1]) {
                    a.out_colidx[o0] = (int32_t)r;
                    if (a.out_values) a.out_values[o0] = 1.0f;
                }
            } else {
                e0 = a.rowptr[v];
                e1 = a.rowptr[v + 1];
                live = e1 > e0 && (split_deg <= 0 || e1 - e0 <= split_deg);
            }
        }
        uint64_t todo = __ballot(live);
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            sample_fill_row<64>(a, s, __shfl(v, src, 64), g * 64 + src, __shfl(e0, src, 64), __shfl(e1, src, 64),
                                s_wave);
        }
    }
}

__global__ __launch_bounds__(kBlock) void ego_sample_fill_long(EgoFill a, EgoSample s, int64_t n_long,
                                                               const int64_t *__restrict__ long_rows) {
    __shared__ int s_wave[kWaves];
    for (int64_t j = blockIdx.x; j < n_long; j += gridDim.x) {
        const int64_t v = long_rows[j];
        if ((uint64_t)v >= (uint64_t)a.n_in || !row_kept(a.level, v, a.hops)) continue;
        const int64_t r = a.local[v];
        if ((uint64_t)r >= (uint64_t)a.n_out) continue;
        sample_fill_row<kBlock>(a, s, v, r, a.rowptr[v], a.rowptr[v + 1], s_wave);
    }
}

// the key of graph `graph` and the long-row list; HAN_E_BADARG for what the entry points refuse
int set_sample(EgoSample &s, uint64_t seed, int graph, int64_t &split_deg, int64_t n_long, const int64_t *long_rows) {
    if (graph < 0 || graph >= (1 << 30) - 1 || n_long < 0) return HAN_E_BADARG;
    if (n_long > 0 && (split_deg < 1 || !long_rows)) return HAN_E_BADARG;
    if (n_long == 0) split_deg = 0;
    s.seed_lo = (uint32_t)seed;
    s.seed_hi = (uint32_t)(seed >> 32);
    s.stream = HAN_STREAM_EGO * ((uint32_t)graph + 1u);
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

extern "C" int han_ego_sample_expand(const int64_t *rowptr, const int32_t *colidx, int64_t n, int h, int fanout,
                                     uint64_t seed, int graph, int64_t split_deg, int64_t n_long,
                                     const int64_t *long_rows, int32_t *level, uint32_t *thr, int32_t *need,
                                     int64_t *kept, void *stream) {
    if (!rowptr || !level || !thr || !need || !kept || n < 0 || n > INT32_MAX || h < 0 || h == INT32_MAX || fanout < 1)
        return HAN_E_BADARG;
    EgoSample s;
    if (const int e = set_sample(s, seed, graph, split_deg, n_long, long_rows)) return e;
    if (n == 0 || !colidx) return 0;
    s.thr = thr; s.need = need; s.kept = kept;
    const hipStream_t st = (hipStream_t)stream;
    ego_sample_expand_rows<<<han_grid_for((n + 63) / 64, 1, 4 * kCap), 64, 0, st>>>(rowptr, colidx, n, (int32_t)h,
                                                                                  (int32_t)fanout, split_deg, s, level);
    HAN_CHECK_LAUNCH();
    if (n_long) {
        ego_sample_expand_long<<<han_grid_for(n_long, 1, kCap), kBlock, 0, st>>>(rowptr, colidx, n, (int32_t)h,
                                                                                 (int32_t)fanout, n_long, long_rows, s,
                                                                                 level);
        HAN_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int han_ego_sample_count(const int64_t *rows, const int32_t *level, int hops, const int64_t *kept,
                                    int64_t n_in, int64_t n_out, int64_t *counts, void *stream) {
    if (!level || !kept || hops < 1 || n_in < 0 || n_out < 0) return HAN_E_BADARG;
    if (n_out == 0) return 0;
    if (!rows || !counts) return HAN_E_BADARG;
    ego_sample_count<<<han_grid_for(n_out, kBlock, kCap), kBlock, 0, (hipStream_t)stream>>>(rows, level, (int32_t)hops,
                                                                                           kept, n_in, n_out, counts);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_ego_sample_fill(const int64_t *rowptr, const int32_t *colidx, const float *values,
                                   const int64_t *rows, const int32_t *level, int hops, const int32_t *local,
                                   int64_t n_in, int64_t n_out, uint64_t seed, int graph, int64_t split_deg,
                                   int64_t n_long, const int64_t *long_rows, const uint32_t *thr, const int32_t *need,
                                   const int64_t *out_rowptr, int32_t *out_colidx, float *out_values, void *stream) {
    if (!rowptr || !level || !local || !thr || !need || hops < 1 || n_in < 0 || n_in > INT32_MAX || n_out < 0 ||
        n_out > INT32_MAX)
        return HAN_E_BADARG;
    EgoSample s;
    if (const int e = set_sample(s, seed, graph, split_deg, n_long, long_rows)) return e;
    if (n_out == 0) return 0;
    if (!rows || !out_rowptr || !out_colidx) return HAN_E_BADARG;
    s.thr = const_cast<uint32_t *>(thr); s.need = const_cast<int32_t *>(need); s.kept = nullptr;
    EgoFill a;
    a.rowptr = rowptr; a.colidx = colidx; a.values = values; a.rows = rows; a.level = level; a.local = local;
    a.hops = (int32_t)hops; a.n_in = n_in; a.n_cols = n_in; a.n_out = n_out;
    a.out_rowptr = out_rowptr; a.out_colidx = out_colidx; a.out_values = out_values;
    const hipStream_t st = (hipStream_t)stream;
    ego_sample_fill_rows<<<han_grid_for((n_out + 63) / 64, 1, 4 * kCap), 64, 0, st>>>(a, s, split_deg);
    HAN_CHECK_LAUNCH();
    if (n_long) {
        ego_sample_fill_long<<<han_grid_for(n_long, 1, kCap), kBlock, 0, st>>>(a, s, n_long, long_rows);
        HAN_CHECK_LAUNCH();
    }
    return 0;
}
