// Classifier + masked loss, optimiser, and the bias-matrix -> CSR input step (gfx950).
//
// Reference arithmetic:
//   models/gat.py:65-72        logits = (1/HC) sum_h (Z Wc[h] + bc[h])
//   models/base_gattn.py:41-48 masked softmax cross-entropy
//   models/base_gattn.py:61-69 masked accuracy
//   models/base_gattn.py:12-24 L2 on every trainable + tf.train.AdamOptimizer
//   utils/process.py:14-25     additive bias matrix (edge <=> entry > -1e8)
// All of it is row-local streaming work (HBM-bound, tiny next to K2).
#include "han_common.h"

namespace {

constexpr int MAXC = 16;
constexpr int kClsBlocks = 2048;   // 8 waves per SIMD: the per-row chain (load, dot, reduce, exp) is latency-bound

// slab row: [64*C] dWm | [C] dbm | loss | acc
struct ClsArgs {
    const float *Z, *Wc, *bc;
    const int32_t *labels;
    const uint8_t *mask;
    float row_weight;
    float *logits, *dZ, *slab;
    int64_t N;
    int C, HC;
};

// Sum over an aligned group of 16 lanes as a butterfly (lane distances 1, 2, 4, 8): every lane adds the same pairs in the
// same order, so all 16 hold the SAME bits.  han_row16_sum ends in two row rotations instead, after which the four quads
// of a group hold differently associated sums (an ulp apart).  Here lane c stores logit c while lane 0 takes the
// argmax and the loss from its own copies: with the rotations two classes with identical weights got different stored
// logits, and the argmax of the stored row could differ from the one the accuracy counted.  Same four DPP adds.
__device__ __forceinline__ float cls_row16_sum(float v) {
    v += han_dpp_xor16<1>(v);
    v += han_dpp_xor16<2>(v);
    v += han_dpp_xor16<4>(v);
    v += han_dpp_xor16<8>(v);
    return v;
}

constexpr int WC_LD = 65;      // row stride of the class-per-lane kernel's LDS matrix (classifier_body.h)

// the fused kernels, over every row
#define CLS_KERNEL classifier_kernel
#define CLS_WIDE_KERNEL classifier_wide_kernel
#define CLS_PARAMS const ClsArgs a
#define CLS_ROW(it) (it)
#include "classifier_body.h"
#undef CLS_KERNEL
#undef CLS_WIDE_KERNEL
#undef CLS_PARAMS
#undef CLS_ROW
// han_classifier_loss_live: the rows live[0 .. a.N)
#define CLS_KERNEL classifier_live_kernel
#define CLS_WIDE_KERNEL classifier_wide_live_kernel
#define CLS_PARAMS const ClsArgs a, const int32_t *live
#define CLS_ROW(it) ((int64_t)live[it])
#include "classifier_body.h"
#undef CLS_KERNEL
#undef CLS_WIDE_KERNEL
#undef CLS_PARAMS
#undef CLS_ROW

// the tuned kernels: up to MAXC classes 16 rows per block iteration (CM = 4, 8 or 16), beyond that class-per-lane
template <int NV>
static void launch_classifier(const ClsArgs &a, bool bwd, int grid, hipStream_t st) {
    HAN_DISPATCH_BOOL(BWD, bwd, {
        switch (a.C <= 4 ? 4 : a.C <= 8 ? 8 : a.C <= MAXC ? 16 : 0) {
            case 4: classifier_kernel<BWD, 4, NV><<<grid, 256, 0, st>>>(a); break;
            case 8: classifier_kernel<BWD, 8, NV><<<grid, 256, 0, st>>>(a); break;
            case 16: classifier_kernel<BWD, 16, NV><<<grid, 256, 0, st>>>(a); break;
            default: classifier_wide_kernel<BWD, NV><<<grid, 256, 0, st>>>(a); break;
        }
    });
}

// ... over the row list `live` (a.N entries)
template <int NV>
static void launch_classifier_live(const ClsArgs &a, const int32_t *live, bool bwd, int grid, hipStream_t st) {
    HAN_DISPATCH_BOOL(BWD, bwd, {
        switch (a.C <= 4 ? 4 : a.C <= 8 ? 8 : a.C <= MAXC ? 16 : 0) {
            case 4: classifier_live_kernel<BWD, 4, NV><<<grid, 256, 0, st>>>(a, live); break;
            case 8: classifier_live_kernel<BWD, 8, NV><<<grid, 256, 0, st>>>(a, live); break;
            case 16: classifier_live_kernel<BWD, 16, NV><<<grid, 256, 0, st>>>(a, live); break;
            default: classifier_wide_live_kernel<BWD, NV><<<grid, 256, 0, st>>>(a, live); break;
        }
    });
}

__global__ void adam_kernel(float *p, const float *g, float *m, float *v, int64_t n, float lr_t, float b1,
                            float b2, float eps, float l2, const int64_t *step_dev) {
    if (step_dev) {   // lr_t holds the base rate; the bias correction comes from the device step count
        const double t = (double)*step_dev;
        lr_t = (float)((double)lr_t * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float pi = p[i];
        const float gi = g[i] + l2 * pi;             // d/dp of l2_coef * p^2/2
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - lr_t * mi / (sqrtf(vi) + eps);
    }
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float *p, int64_t n, float *partial) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) s += p[i] * p[i];
    s = han_wave_sum(s);
    __shared__ float w[4];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

__global__ void sumsq_finish_kernel(const float *partial, int nblocks, float *out) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += 64) s += partial[i];
    s = han_wave_sum(s);
    if (threadIdx.x == 0) out[0] = 0.5f * s;
}

// one wave per row of the dense bias matrix
__global__ __launch_bounds__(256) void bias_count_kernel(const float *bias, int64_t N, int64_t ld,
                                                         int64_t *counts) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    int cnt = 0;
    for (int64_t c0 = 0; c0 < N; c0 += 64) {
        const int64_t c = c0 + lane;
        const bool edge = c < N && bias[row * ld + c] > -1e8f;
        cnt += __popcll(__ballot(edge));
    }
    if (lane == 0) counts[row] = cnt;
}

__global__ __launch_bounds__(256) void bias_fill_kernel(const float *bias, int64_t N, int64_t ld,
                                                        const int64_t *rowptr, int32_t *colidx) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    int64_t pos = rowptr[row];
    for (int64_t c0 = 0; c0 < N; c0 += 64) {
        const int64_t c = c0 + lane;
        const bool edge = c < N && bias[row * ld + c] > -1e8f;
        const unsigned long long b = __ballot(edge);
        if (edge) colidx[pos + __popcll(b & ((1ull << lane) - 1ull))] = (int32_t)c;
        pos += __popcll(b);
    }
}


// ---------------------------------------------------------------------------------------------
// Any embedding width (D a multiple of 64: a last layer of 8 heads x 32, hid_units = [128] ...) and any
// class count (round 3; models/gat.py:61-72 leaves both free).  Three small kernels instead of one:
//   cls_mean_kernel   WmT[c][d] = mean_h Wc[h][d][c], bm[c] = mean_h bc[h][c]   (the head average, once)
//   cls_gen_kernel    one wave per row, lane = feature: logit_c = wave_sum(z . WmT[c]) + bm[c] class by class
//                     (online max / sum / first argmax), loss + accuracy; backward: dl_c, dZ = sum_c dl_c WmT[c]
//                     in registers, dl rows to a scratch table.  Rows outside the loss mask have dl == 0
//                     exactly: their dZ row is written as zeros and the class loop is skipped.
//   cls_dw_kernel     dWm = Z^T dL over the MASKED rows only (the others add exactly 0), one block per
//                     (row split, 64-feature tile, 16-class tile), lane = feature; db from the feature-tile-0 blocks
// NV = registers holding the row (64*NV >= D), or 0: any width, the row is re-read from L1 per class.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cls_mean_kernel(const float *Wc, const float *bc, float *WmT, float *bm,
                                                       int D, int C, int HC) {
    const float invh = 1.f / (float)HC;
    const int64_t n = (int64_t)D * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i / D), d = (int)(i % D);
        float s = 0.f;
        for (int h = 0; h < HC; ++h) s += Wc[(int64_t)h * n + (int64_t)d * C + c];
        WmT[i] = s * invh;
    }
    if (blockIdx.x == 0)
        for (int c = threadIdx.x; c < C; c += 256) {
            float s = 0.f;
            for (int h = 0; h < HC; ++h) s += bc[h * C + c];
            bm[c] = s * invh;
        }
}

struct ClsGenArgs {
    const float *Z, *WmT, *bm;
    const int32_t *labels;
    const uint8_t *mask;
    float row_weight;
    float *logits, *dZ, *dL, *slab;    // slab: [gridDim.x][2] loss | acc
    int64_t N;
    int D, C;
};

template <bool BWD, int NV>
__global__ __launch_bounds__(256) void cls_gen_kernel(const ClsGenArgs a) {
    constexpr int NR = NV > 0 ? NV : 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int D = a.D, C = a.C, nv = D / 64;
    float loss_acc = 0.f, acc_acc = 0.f;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + w, nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave0; row < a.N; row += nwaves) {
        const float *zrow = a.Z + row * D + lane;
        float z[NR];
        if (NV > 0) {
#pragma unroll
            for (int v = 0; v < NR; ++v) z[v] = v < nv ? zrow[64 * v] : 0.f;
        }
        float mx = HAN_NEG_BIG, se = 0.f, llab = 0.f;
        int am = 0;
        const int lab = a.labels[row];
        const bool live = a.mask[row] != 0;      // the predicate cls_dw_kernel skips rows by: a live row ALWAYS gets its dL row
        const float wgt = live ? a.row_weight : 0.f;
        for (int c = 0; c < C; ++c) {
            const float *wr = a.WmT + (int64_t)c * D + lane;
            float part = 0.f;
            if (NV > 0) {
#pragma unroll
                for (int v = 0; v < NR; ++v) part += v < nv ? z[v] * wr[64 * v] : 0.f;
            } else {
                for (int v = 0; v < nv; ++v) part += zrow[64 * v] * wr[64 * v];
            }
            const float lg = han_wave_sum(part) + a.bm[c];
            if (lane == 0) a.logits[row * C + c] = lg;
            if (lg > mx) {       // first maximum, as argmax
                se = se * __expf(mx - lg) + 1.f;
                mx = lg;
                am = c;
            } else {
                se += __expf(lg - mx);
            }
            llab = (c == lab) ? lg : llab;
        }
        if (lane == 0) {
            loss_acc += wgt * (mx + __logf(se) - llab);
            acc_acc += wgt * (am == lab ? 1.f : 0.f);
        }
        if (BWD) {
            float dz[NR];
#pragma unroll
            for (int v = 0; v < NR; ++v) dz[v] = 0.f;
            if (live) {              // wave-uniform: rows outside the mask have dl == 0 exactly (a live row with
                                     // row_weight == 0 writes zeros: cls_dw_kernel reads the dL row of every live row)
                const float inv = 1.f / se;
                if (NV == 0)
                    for (int v = 0; v < nv; ++v) a.dZ[row * D + 64 * v + lane] = 0.f;
                for (int c = 0; c < C; ++c) {
                    // lane 0 wrote the logit; it reads it back (same thread) and hands it to the wave
                    const float lg = __int_as_float(__builtin_amdgcn_readfirstlane(
                        __float_as_int(lane == 0 ? a.logits[row * C + c] : 0.f)));
                    const float dl = wgt * (__expf(lg - mx) * inv - (c == lab ? 1.f : 0.f));
                    if (lane == 0) a.dL[row * C + c] = dl;
                    const float *wr = a.WmT + (int64_t)c * D + lane;
                    if (NV > 0) {
#pragma unroll
                        for (int v = 0; v < NR; ++v) dz[v] += v < nv ? dl * wr[64 * v] : 0.f;
                    } else {
                        for (int v = 0; v < nv; ++v) a.dZ[row * D + 64 * v + lane] += dl * wr[64 * v];
                    }
                }
            }
            if (NV > 0 || !live) {
                if (NV > 0) {
#pragma unroll
                    for (int v = 0; v < NR; ++v)
                        if (v < nv) a.dZ[row * D + 64 * v + lane] = dz[v];
                } else {
                    for (int v = 0; v < nv; ++v) a.dZ[row * D + 64 * v + lane] = 0.f;
                }
            }
        }
    }
    __shared__ float red[4][2];
    if (lane == 0) { red[w][0] = loss_acc; red[w][1] = acc_acc; }
    __syncthreads();
    if (threadIdx.x < 2)
        a.slab[(int64_t)blockIdx.x * 2 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// slab row per row split: [D*C] dWm | [C] dbm.  grid = (splits, D/64 feature tiles, ceil(C/16) class tiles)
__global__ __launch_bounds__(256) void cls_dw_kernel(const float *Z, const float *dL, const uint8_t *mask, float *slab,
                                                     int64_t N, int D, int C) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int d0 = 64 * blockIdx.y, c0 = 16 * blockIdx.z;
    const int nc = C - c0 < 16 ? C - c0 : 16;
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = per * blockIdx.x, r1 = (r0 + per < N) ? r0 + per : N;
    float acc[16], dbacc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { acc[j] = 0.f; dbacc[j] = 0.f; }
    for (int64_t row = r0 + w; row < r1; row += 4) {
        if (mask && !mask[row]) continue;               // wave-uniform; dl of such a row is exactly 0
        const float z = Z[row * D + d0 + lane];
        const float *dl = dL + row * C + c0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float v = j < nc ? dl[j] : 0.f;
            acc[j] += z * v;
            dbacc[j] += v;
        }
    }
    __shared__ float red[4][16][65];
#pragma unroll
    for (int j = 0; j < 16; ++j) red[w][j][lane] = acc[j];
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) red[w][j][64] = dbacc[j];
    }
    __syncthreads();
    float *out = slab + (int64_t)blockIdx.x * ((int64_t)D * C + C);
    for (int i = threadIdx.x; i < 16 * 64; i += 256) {
        const int j = i & 15, d = i >> 4;
        if (j < nc) out[(int64_t)(d0 + d) * C + c0 + j] = red[0][j][d] + red[1][j][d] + red[2][j][d] + red[3][j][d];
    }
    if (blockIdx.y == 0 && threadIdx.x < nc)
        out[(int64_t)D * C + c0 + threadIdx.x] = red[0][threadIdx.x][64] + red[1][threadIdx.x][64] + red[2][threadIdx.x][64] + red[3][threadIdx.x][64];
}

// dZ = dL . Wm^T for a given dL (the backward of the logits alone, HeteGAT_multi.inference without the fused loss)
__global__ __launch_bounds__(256) void cls_dz_kernel(const float *dL, const float *WmT, float *dZ, int64_t N, int D, int C) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + w, nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave0; row < N; row += nwaves) {
        const float *dl = dL + row * C;
        for (int f = lane; f < D; f += 64) {
            float s = 0.f;
            for (int c = 0; c < C; ++c) s += dl[c] * WmT[(int64_t)c * D + f];
            dZ[row * D + f] = s;
        }
    }
}

constexpr int kClsGenBlocks = 2048;

static int cls_dw_splits(int D, int C) {
    const int tiles = (D / 64) * ((C + 15) / 16);
    int s = 1024 / tiles;
    return s < 1 ? 1 : (s > 256 ? 256 : s);
}

// workspace of the three-kernel paths, offsets in floats: WmT (at 0) | bm | loss/acc slabs | dL | dW slabs; the
// backward of given dlogits (han_classifier_bwd) has neither slabs of loss / accuracy nor a dL table of its own
struct ClsGenWs { size_t bm, la, dL, dws, floats; };

static ClsGenWs cls_gen_ws(int64_t N, int D, int C, bool loss) {
    ClsGenWs w;
    w.bm = (size_t)D * C;
    w.la = w.bm + (size_t)C;
    w.dL = w.la + (loss ? (size_t)kClsGenBlocks * 2 : 0);
    w.dws = w.dL + (loss ? (size_t)N * C : 0);
    w.floats = w.dws + (size_t)cls_dw_splits(D, C) * ((size_t)D * C + C);
    return w;
}

static bool cls_shape(int D, int C) { return D >= 64 && D % 64 == 0 && C >= 1; }
static bool cls_tuned(int D, int C) { return (D == 64 || D == 128) && C >= 1 && C <= 64; }

// the head gradients dWc | dbc of a slab row [D*C] | [C]: every head receives the same (1/HC)-scaled gradient
// (models/gat.py:72 averages them); loss_acc, when given, takes the two slab columns behind them as a third segment
static HanReduceOut cls_head_grads(float *dWc, float *dbc, float *loss_acc, int D, int C, int HC) {
    const int dc = D * C;
    HanReduceOut o = han_reduce_to(dWc, dc + C + (loss_acc ? 2 : 0));
    o.nseg = loss_acc ? 3 : 2;
    o.ptr[1] = dbc; o.ptr[2] = loss_acc;
    o.seg_end[0] = dc; o.seg_end[1] = dc + C;
    o.scale[0] = o.scale[1] = 1.f / (float)HC;
    o.rep[0] = o.rep[1] = HC;
    o.rep_stride[0] = (int64_t)dc; o.rep_stride[1] = C;
    return o;
}

static int launch_cls_mean(const float *Wc, const float *bc, float *ws, const ClsGenWs &w, int D, int C, int HC, hipStream_t st) {
    cls_mean_kernel<<<han_grid_for((int64_t)D * C, 256, 256), 256, 0, st>>>(Wc, bc, ws, ws + w.bm, D, C, HC);
    HAN_CHECK_LAUNCH();
    return 0;
}

// dWm = Z^T dL per row split, then the head gradients from the slabs
static int launch_cls_dw(const float *Z, const float *dL, const uint8_t *mask, float *dws, float *dWc, float *dbc,
                         int64_t N, int D, int C, int HC, hipStream_t st) {
    const int S = cls_dw_splits(D, C), width = D * C + C;
    cls_dw_kernel<<<dim3(S, D / 64, (C + 15) / 16), 256, 0, st>>>(Z, dL, mask, dws, N, D, C);
    HAN_CHECK_LAUNCH();
    const hipError_t e = han_reduce_slabs(dws, S, width, width, cls_head_grads(dWc, dbc, nullptr, D, C, HC), st);
    return e != hipSuccess ? (int)e : 0;
}

}  // namespace

extern "C" size_t han_classifier_workspace(int64_t N, int D, int C, int) {
    if (cls_shape(D, C) && !cls_tuned(D, C)) return cls_gen_ws(N, D, C, true).floats * sizeof(float);
    return (size_t)kClsBlocks * (size_t)(D * C + C + 2) * sizeof(float);
}

extern "C" int han_classifier_loss(const float *Z, const float *Wc, const float *bc, const int32_t *labels,
                                   const uint8_t *mask, float row_weight, float *logits, float *loss_acc,
                                   float *dZ, float *dWc, float *dbc, void *workspace, size_t workspace_bytes,
                                   int64_t N, int D, int C, int HC, void *stream) {
    if (!Z || !Wc || !bc || !labels || !mask || !logits || !loss_acc || !workspace || N < 0 || HC <= 0)
        return HAN_E_BADARG;
    if (!cls_shape(D, C)) return HAN_E_UNSUPPORTED;
    const bool bwd = dZ != nullptr;
    if (bwd && (!dWc || !dbc)) return HAN_E_BADARG;
    if (workspace_bytes < han_classifier_workspace(N, D, C, HC)) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    if (!cls_tuned(D, C)) {       // any embedding width / class count: the three-kernel path
        const ClsGenWs w = cls_gen_ws(N, D, C, true);
        ClsGenArgs g;
        g.Z = Z; g.WmT = ws; g.bm = ws + w.bm; g.labels = labels; g.mask = mask; g.row_weight = row_weight;
        g.logits = logits; g.dZ = dZ; g.dL = ws + w.dL; g.slab = ws + w.la; g.N = N; g.D = D; g.C = C;
        const int rc = launch_cls_mean(Wc, bc, ws, w, D, C, HC, st);
        if (rc != 0) return rc;
        const int grid = han_grid_for(N > 0 ? N : 1, 4, kClsGenBlocks);
        HAN_DISPATCH_BOOL(BWD, bwd, {      // NV: registers holding the row, 0 beyond 1024 columns
            switch (D <= 256 ? 4 : D <= 512 ? 8 : D <= 1024 ? 16 : 0) {
                case 4: cls_gen_kernel<BWD, 4><<<grid, 256, 0, st>>>(g); break;
                case 8: cls_gen_kernel<BWD, 8><<<grid, 256, 0, st>>>(g); break;
                case 16: cls_gen_kernel<BWD, 16><<<grid, 256, 0, st>>>(g); break;
                default: cls_gen_kernel<BWD, 0><<<grid, 256, 0, st>>>(g); break;
            }
        });
        HAN_CHECK_LAUNCH();
        const hipError_t e = han_reduce_slabs(g.slab, grid, 2, 2, han_reduce_to(loss_acc, 2), st);
        if (e != hipSuccess) return (int)e;
        return bwd ? launch_cls_dw(Z, g.dL, mask, ws + w.dws, dWc, dbc, N, D, C, HC, st) : 0;
    }
    ClsArgs a;
    a.Z = Z; a.Wc = Wc; a.bc = bc; a.labels = labels; a.mask = mask; a.row_weight = row_weight;
    a.logits = logits; a.dZ = dZ; a.slab = ws; a.N = N; a.C = C; a.HC = HC;
    const int grid = han_grid_for(N > 0 ? N : 1, C > MAXC ? 4 : 16, kClsBlocks);      // class-per-lane: one wave per row
    if (D == 128) launch_classifier<2>(a, bwd, grid, st);
    else launch_classifier<1>(a, bwd, grid, st);
    HAN_CHECK_LAUNCH();
    // one second-stage launch: the head gradients and loss / accuracy (the last two slab columns)
    const int width = D * C + C + 2;
    const hipError_t e = bwd ? han_reduce_slabs(ws, grid, width, width, cls_head_grads(dWc, dbc, loss_acc, D, C, HC), st)
                             : han_reduce_slabs(ws + D * C + C, grid, width, 2, han_reduce_to(loss_acc, 2), st);
    return e != hipSuccess ? (int)e : 0;
}

extern "C" int han_classifier_loss_live(const float *Z, const float *Wc, const float *bc, const int32_t *labels,
                                        const uint8_t *mask, float row_weight, float *logits, float *loss_acc,
                                        float *dZ, float *dWc, float *dbc, void *workspace, size_t workspace_bytes,
                                        const int32_t *live, int64_t n_live, int64_t N, int D, int C, int HC,
                                        void *stream) {
    if (!Z || !Wc || !bc || !labels || !mask || !logits || !loss_acc || !workspace || N < 0 || HC <= 0 || n_live < 0 ||
        n_live > N || (n_live > 0 && !live))
        return HAN_E_BADARG;
    if (!cls_tuned(D, C)) return HAN_E_UNSUPPORTED;      // the fused kernels only
    const bool bwd = dZ != nullptr;
    if (bwd && (!dWc || !dbc)) return HAN_E_BADARG;
    if (workspace_bytes < han_classifier_workspace(N, D, C, HC)) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n_live == 0) {      // no row, no launch: the sums over no rows
        hipError_t e = hipMemsetAsync(loss_acc, 0, 2 * sizeof(float), st);
        if (e == hipSuccess && bwd) e = hipMemsetAsync(dWc, 0, (size_t)HC * D * C * sizeof(float), st);
        if (e == hipSuccess && bwd) e = hipMemsetAsync(dbc, 0, (size_t)HC * C * sizeof(float), st);
        return (int)e;
    }
    float *ws = (float *)workspace;
    ClsArgs a;
    a.Z = Z; a.Wc = Wc; a.bc = bc; a.labels = labels; a.mask = mask; a.row_weight = row_weight;
    a.logits = logits; a.dZ = dZ; a.slab = ws; a.N = n_live; a.C = C; a.HC = HC;
    const int grid = han_grid_for(n_live, C > MAXC ? 4 : 16, kClsBlocks);      // the grid and the slab rows follow the list
    if (D == 128) launch_classifier_live<2>(a, live, bwd, grid, st);
    else launch_classifier_live<1>(a, live, bwd, grid, st);
    HAN_CHECK_LAUNCH();
    const int width = D * C + C + 2;
    const hipError_t e = bwd ? han_reduce_slabs(ws, grid, width, width, cls_head_grads(dWc, dbc, loss_acc, D, C, HC), st)
                             : han_reduce_slabs(ws + D * C + C, grid, width, 2, han_reduce_to(loss_acc, 2), st);
    return e != hipSuccess ? (int)e : 0;
}

extern "C" size_t han_classifier_bwd_workspace(int64_t N, int D, int C, int) {
    return cls_shape(D, C) ? cls_gen_ws(N, D, C, false).floats * sizeof(float) : 0;
}

extern "C" int han_classifier_bwd(const float *Z, const float *Wc, const float *bc, const float *dlogits, float *dZ,
                                  float *dWc, float *dbc, void *workspace, size_t workspace_bytes, int64_t N, int D,
                                  int C, int HC, void *stream) {
    if (!Z || !Wc || !bc || !dlogits || !dZ || !dWc || !dbc || !workspace || N < 0 || HC <= 0) return HAN_E_BADARG;
    if (!cls_shape(D, C)) return HAN_E_UNSUPPORTED;
    const ClsGenWs w = cls_gen_ws(N, D, C, false);
    if (workspace_bytes < w.floats * sizeof(float)) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    const int rc = launch_cls_mean(Wc, bc, ws, w, D, C, HC, st);
    if (rc != 0) return rc;
    cls_dz_kernel<<<han_grid_for(N > 0 ? N : 1, 4, kClsGenBlocks), 256, 0, st>>>(dlogits, ws, dZ, N, D, C);
    HAN_CHECK_LAUNCH();
    return launch_cls_dw(Z, dlogits, nullptr, ws + w.dws, dWc, dbc, N, D, C, HC, st);
}

extern "C" int han_adam_step(float *param, const float *grad, float *m, float *v, int64_t n, float lr_t,
                             float beta1, float beta2, float eps, float l2_coef, const int64_t *step_dev,
                             void *stream) {
    if (!param || !grad || !m || !v || n < 0) return HAN_E_BADARG;
    if (n == 0) return 0;
    adam_kernel<<<han_grid_for(n, 256, 2048), 256, 0, (hipStream_t)stream>>>(param, grad, m, v, n, lr_t, beta1,
                                                                            beta2, eps, l2_coef, step_dev);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_l2_half_sumsq(const float *param, int64_t n, float *out, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    if (!param || !out || !workspace || n < 0) return HAN_E_BADARG;
    if (workspace_bytes < 4096 * sizeof(float)) return HAN_E_WORKSPACE;
    const int grid = han_grid_for(n > 0 ? n : 1, 256, 1024);
    sumsq_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(param, n, (float *)workspace);
    HAN_CHECK_LAUNCH();
    sumsq_finish_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const float *)workspace, grid, out);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_bias_row_counts(const float *bias, int64_t N, int64_t ld, int64_t *counts, void *stream) {
    if (!bias || !counts || N < 0 || ld < N) return HAN_E_BADARG;
    if (N == 0) return 0;
    bias_count_kernel<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(bias, N, ld, counts);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_bias_fill_csr(const float *bias, int64_t N, int64_t ld, const int64_t *rowptr,
                                 int32_t *colidx, void *stream) {
    if (!bias || !rowptr || !colidx || N < 0 || ld < N) return HAN_E_BADARG;
    if (N == 0) return 0;
    bias_fill_kernel<<<(unsigned)((N + 3) / 4), 256, 0, (hipStream_t)stream>>>(bias, N, ld, rowptr, colidx);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_abi_version(void) { return HAN_ABI_VERSION; }

extern "C" const char *han_error_string(int code) {
    switch (code) {
        case 0: return "ok";
        case HAN_E_BADARG: return "han: bad argument (null pointer, negative size or inconsistent shape)";
        case HAN_E_UNSUPPORTED: return "han: shape not supported by this build (K*FP == 64 with FP in {4,8,16,32,64}; D and A multiples of 64)";
        case HAN_E_WORKSPACE: return "han: workspace too small";
        case HAN_E_NOT_ELIGIBLE: return "han: this call is outside the combined kernel's shapes; nothing was launched (use the separate entry points)";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "han: unknown error";
    }
}

// ---------------------------------------------------------------------------------------------
// Multi-label objective (han_classifier_multilabel): models/base_gattn.py:50-59 (masked sigmoid cross-entropy, TF's
// stable form, mean over the C classes of a row) and :71-94 (micro-F1).  Per class, with e = exp(-|x|):
//   loss term   max(x, 0) - x y + log(1 + e)
//   sigma       1 / (1 + e) for x >= 0, e / (1 + e) otherwise        dlogits = (w / C) (sigma - y)
//   prediction  x > 0                                                (round(sigmoid(x)), half to even)
// Labels are bit words: class c of a row is bit c % 64 of word c / 64.  The counts tp | fp | fn of the masked rows are
// integers from the lane to the slab to the finishing kernel, which also forms micro-F1 = 2 tp / (2 tp + fp + fn) in
// double (NaN for tp == 0, the reference's 0 / 0).  The softmax kernels above are not touched: the fused forms are
// their thread maps with another objective (multilabel_body.h), the any-shape form is a row kernel that writes the dL
// table for cls_dw_kernel.
// ---------------------------------------------------------------------------------------------
namespace {

struct MlArgs {
    const float *Z, *Wc, *bc;
    const unsigned long long *bits;
    const uint8_t *mask;
    float row_weight;
    float *logits, *dZ, *slab;
    unsigned long long *cslab;      // [gridDim.x][3] tp | fp | fn
    int64_t N;
    int C, HC;
};

__device__ __forceinline__ float ml_exp(float x) { return __expf(-fabsf(x)); }

__device__ __forceinline__ float ml_loss(float x, unsigned y, float e) {
    return (fmaxf(x, 0.f) - (y ? x : 0.f)) + __logf(1.f + e);
}

__device__ __forceinline__ float ml_sigma(float x, float e) { return (x >= 0.f ? 1.f : e) / (1.f + e); }

#define ML_KERNEL multilabel_kernel
#define ML_WIDE_KERNEL multilabel_wide_kernel
#define ML_PARAMS const MlArgs a
#define ML_ROW(it) (it)
#include "multilabel_body.h"
#undef ML_KERNEL
#undef ML_WIDE_KERNEL
#undef ML_PARAMS
#undef ML_ROW
// the row list: the rows live[0 .. a.N)
#define ML_KERNEL multilabel_live_kernel
#define ML_WIDE_KERNEL multilabel_wide_live_kernel
#define ML_PARAMS const MlArgs a, const int32_t *live
#define ML_ROW(it) ((int64_t)live[it])
#include "multilabel_body.h"
#undef ML_KERNEL
#undef ML_WIDE_KERNEL
#undef ML_PARAMS
#undef ML_ROW

template <int NV>
static void launch_multilabel(const MlArgs &a, const int32_t *live, bool bwd, int grid, hipStream_t st) {
    const int cm = a.C <= 4 ? 4 : a.C <= 8 ? 8 : a.C <= MAXC ? 16 : 0;
    HAN_DISPATCH_BOOL(BWD, bwd, {
        if (live) {
            switch (cm) {
                case 4: multilabel_live_kernel<BWD, 4, NV><<<grid, 256, 0, st>>>(a, live); break;
                case 8: multilabel_live_kernel<BWD, 8, NV><<<grid, 256, 0, st>>>(a, live); break;
                case 16: multilabel_live_kernel<BWD, 16, NV><<<grid, 256, 0, st>>>(a, live); break;
                default: multilabel_wide_live_kernel<BWD, NV><<<grid, 256, 0, st>>>(a, live); break;
            }
        } else {
            switch (cm) {
                case 4: multilabel_kernel<BWD, 4, NV><<<grid, 256, 0, st>>>(a); break;
                case 8: multilabel_kernel<BWD, 8, NV><<<grid, 256, 0, st>>>(a); break;
                case 16: multilabel_kernel<BWD, 16, NV><<<grid, 256, 0, st>>>(a); break;
                default: multilabel_wide_kernel<BWD, NV><<<grid, 256, 0, st>>>(a); break;
            }
        }
    });
}

struct MlGenArgs {
    const float *Z, *WmT, *bm;
    const unsigned long long *bits;
    const uint8_t *mask;
    float row_weight;
    float *logits, *dZ, *dL, *slab;    // slab: [gridDim.x] loss
    unsigned long long *cslab;
    int64_t N;
    int D, C, NW;                      // NW = label words per row
};

// Any width / class count: one wave per row, lane = feature, class by class as cls_gen_kernel -- but the sigmoid
// objective needs no statistics of the row, so one pass over the classes gives logit, loss term, count, dl and the dZ
// update.  Rows outside the mask get a dZ row of zeros and no dL row (cls_dw_kernel skips them by the same predicate).
template <bool BWD, int NV>
__global__ __launch_bounds__(256) void ml_gen_kernel(const MlGenArgs a) {
    constexpr int NR = NV > 0 ? NV : 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int D = a.D, C = a.C, nv = D / 64;
    const float invc = 1.f / (float)C;
    float loss_acc = 0.f;
    unsigned long long tp = 0, fp = 0, fn = 0;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + w, nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave0; row < a.N; row += nwaves) {
        const float *zrow = a.Z + row * D + lane;
        float z[NR];
        if (NV > 0) {
#pragma unroll
            for (int v = 0; v < NR; ++v) z[v] = v < nv ? zrow[64 * v] : 0.f;
        }
        const bool live = __builtin_amdgcn_readfirstlane((int)a.mask[row]) != 0;      // the same byte in every lane
        const float wgt = live ? a.row_weight : 0.f;
        const float wc = wgt * invc;
        const unsigned long long *yrow = a.bits + row * a.NW;
        unsigned long long yw = 0;
        float rs = 0.f;
        float dz[NR];
#pragma unroll
        for (int v = 0; v < NR; ++v) dz[v] = 0.f;
        if (BWD && NV == 0)
            for (int v = 0; v < nv; ++v) a.dZ[row * D + 64 * v + lane] = 0.f;
        for (int c = 0; c < C; ++c) {
            if ((c & 63) == 0) yw = yrow[c >> 6];
            const unsigned y = (unsigned)(yw >> (c & 63)) & 1u;
            const float *wr = a.WmT + (int64_t)c * D + lane;
            float part = 0.f;
            if (NV > 0) {
#pragma unroll
                for (int v = 0; v < NR; ++v) part += v < nv ? z[v] * wr[64 * v] : 0.f;
            } else {
                for (int v = 0; v < nv; ++v) part += zrow[64 * v] * wr[64 * v];
            }
            const float lg = han_wave_sum(part) + a.bm[c];
            if (lane == 0) a.logits[row * C + c] = lg;
            if (live) {                 // wave-uniform; a row outside the mask: its logits and nothing else
                const float e = ml_exp(lg);
                rs += ml_loss(lg, y, e);
                const unsigned p = lg > 0.f ? 1u : 0u;
                tp += p & y;
                fp += p & (y ^ 1u);
                fn += (p ^ 1u) & y;
                if (BWD) {
                    const float dl = wc * (ml_sigma(lg, e) - (float)y);
                    if (lane == 0) a.dL[row * C + c] = dl;
                    if (NV > 0) {
#pragma unroll
                        for (int v = 0; v < NR; ++v) dz[v] += v < nv ? dl * wr[64 * v] : 0.f;
                    } else {
                        for (int v = 0; v < nv; ++v) a.dZ[row * D + 64 * v + lane] += dl * wr[64 * v];
                    }
                }
            }
        }
        if (lane == 0 && live) loss_acc += wgt * (rs * invc);
        if (BWD && NV > 0) {
#pragma unroll
            for (int v = 0; v < NR; ++v)
                if (v < nv) a.dZ[row * D + 64 * v + lane] = dz[v];
        }
    }
    __shared__ float red[4];
    __shared__ unsigned long long cnt[4][3];
    if (lane == 0) { red[w] = loss_acc; cnt[w][0] = tp; cnt[w][1] = fp; cnt[w][2] = fn; }
    __syncthreads();
    if (threadIdx.x == 0) a.slab[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    if (threadIdx.x < 3)
        a.cslab[(int64_t)blockIdx.x * 3 + threadIdx.x] =
            cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
}

// the counts of the blocks -> counts[3] (int64) and loss_acc[1] = micro-F1; one block of 192 threads
__global__ __launch_bounds__(192) void ml_finish_kernel(const unsigned long long *cslab, int nblocks, float *loss_acc,
                                                        long long *counts) {
    __shared__ unsigned long long part[3][64];
    __shared__ unsigned long long tot[3];
    const int k = threadIdx.x >> 6, j = threadIdx.x & 63;
    unsigned long long s = 0;
    for (int b = j; b < nblocks; b += 64) s += cslab[(int64_t)b * 3 + k];
    part[k][j] = s;
    __syncthreads();
    if (j == 0) {
        unsigned long long t = 0;
        for (int i = 0; i < 64; ++i) t += part[k][i];
        tot[k] = t;
        counts[k] = (long long)t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tp = (double)tot[0], rest = (double)tot[1] + (double)tot[2];
        loss_acc[1] = tot[0] == 0 ? __int_as_float(0x7FC00000) : (float)(2.0 * tp / (2.0 * tp + rest));
    }
}

// workspace: the float part (the slabs of the fused kernels, or the three-kernel layout of cls_gen_ws with ONE loss
// column used), then, 8-byte aligned, the count slab [blocks][3]
struct MlWs { size_t counts, bytes; };

static MlWs ml_ws(int64_t N, int D, int C) {
    MlWs w;
    const size_t floats = cls_tuned(D, C) ? (size_t)kClsBlocks * (size_t)(D * C + C + 1) : cls_gen_ws(N, D, C, true).floats;
    w.counts = (floats * sizeof(float) + 7) / 8 * 8;
    w.bytes = w.counts + (size_t)(cls_tuned(D, C) ? kClsBlocks : kClsGenBlocks) * 3 * sizeof(unsigned long long);
    return w;
}

}  // namespace

extern "C" size_t han_classifier_multilabel_workspace(int64_t N, int D, int C, int) {
    if (!cls_shape(D, C) || N < 0) return 0;
    return ml_ws(N, D, C).bytes;
}

extern "C" int han_classifier_multilabel(const float *Z, const float *Wc, const float *bc, const uint64_t *label_bits,
                                         const uint8_t *mask, float row_weight, float *logits, float *loss_acc,
                                         int64_t *counts, float *dZ, float *dWc, float *dbc, void *workspace,
                                         size_t workspace_bytes, const int32_t *live, int64_t n_live, int64_t N, int D,
                                         int C, int HC, void *stream) {
    if (!Z || !Wc || !bc || !label_bits || !mask || !logits || !loss_acc || !counts || !workspace || N < 0 || HC <= 0)
        return HAN_E_BADARG;
    if (live && (n_live < 0 || n_live > N)) return HAN_E_BADARG;
    const bool bwd = dZ != nullptr;
    if (bwd && (!dWc || !dbc)) return HAN_E_BADARG;
    if (!cls_shape(D, C)) return HAN_E_UNSUPPORTED;
    const bool tuned = cls_tuned(D, C);
    if (live && !tuned) return HAN_E_UNSUPPORTED;      // the row list: the fused kernels only
    const MlWs mw = ml_ws(N, D, C);
    if (workspace_bytes < mw.bytes) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float *ws = (float *)workspace;
    unsigned long long *cslab = (unsigned long long *)((char *)workspace + mw.counts);
    const unsigned long long *bits = (const unsigned long long *)label_bits;
    if (live && n_live == 0) {      // no row, no launch: the sums over no rows, and 0 / 0 for the metric (all-ones is a NaN)
        hipError_t e = hipMemsetAsync(loss_acc, 0, sizeof(float), st);
        if (e == hipSuccess) e = hipMemsetAsync(loss_acc + 1, 0xFF, sizeof(float), st);
        if (e == hipSuccess) e = hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), st);
        if (e == hipSuccess && bwd) e = hipMemsetAsync(dWc, 0, (size_t)HC * D * C * sizeof(float), st);
        if (e == hipSuccess && bwd) e = hipMemsetAsync(dbc, 0, (size_t)HC * C * sizeof(float), st);
        return (int)e;
    }
    if (!tuned) {       // head average -> row kernel -> Z^T dL over the masked rows
        const ClsGenWs w = cls_gen_ws(N, D, C, true);
        MlGenArgs g;
        g.Z = Z; g.WmT = ws; g.bm = ws + w.bm; g.bits = bits; g.mask = mask; g.row_weight = row_weight;
        g.logits = logits; g.dZ = dZ; g.dL = ws + w.dL; g.slab = ws + w.la; g.cslab = cslab; g.N = N; g.D = D; g.C = C;
        g.NW = (C + 63) / 64;
        const int rc = launch_cls_mean(Wc, bc, ws, w, D, C, HC, st);
        if (rc != 0) return rc;
        const int grid = han_grid_for(N > 0 ? N : 1, 4, kClsGenBlocks);
        HAN_DISPATCH_BOOL(BWD, bwd, {
            switch (D <= 256 ? 4 : D <= 512 ? 8 : D <= 1024 ? 16 : 0) {
                case 4: ml_gen_kernel<BWD, 4><<<grid, 256, 0, st>>>(g); break;
                case 8: ml_gen_kernel<BWD, 8><<<grid, 256, 0, st>>>(g); break;
                case 16: ml_gen_kernel<BWD, 16><<<grid, 256, 0, st>>>(g); break;
                default: ml_gen_kernel<BWD, 0><<<grid, 256, 0, st>>>(g); break;
            }
        });
        HAN_CHECK_LAUNCH();
        const hipError_t e = han_reduce_slabs(g.slab, grid, 1, 1, han_reduce_to(loss_acc, 1), st);
        if (e != hipSuccess) return (int)e;
        ml_finish_kernel<<<1, 192, 0, st>>>(cslab, grid, loss_acc, (long long *)counts);
        HAN_CHECK_LAUNCH();
        return bwd ? launch_cls_dw(Z, g.dL, mask, ws + w.dws, dWc, dbc, N, D, C, HC, st) : 0;
    }
    const int64_t rows = live ? n_live : N;
    MlArgs a;
    a.Z = Z; a.Wc = Wc; a.bc = bc; a.bits = bits; a.mask = mask; a.row_weight = row_weight;
    a.logits = logits; a.dZ = dZ; a.slab = ws; a.cslab = cslab; a.N = rows; a.C = C; a.HC = HC;
    const int grid = han_grid_for(rows > 0 ? rows : 1, C > MAXC ? 4 : 16, kClsBlocks);
    if (D == 128) launch_multilabel<2>(a, live, bwd, grid, st);
    else launch_multilabel<1>(a, live, bwd, grid, st);
    HAN_CHECK_LAUNCH();
    // one second-stage launch: the head gradients and the loss (the last slab column); then the counts
    const int width = D * C + C + 1;
    const hipError_t e = bwd ? han_reduce_slabs(ws, grid, width, width, cls_head_grads(dWc, dbc, loss_acc, D, C, HC), st)
                             : han_reduce_slabs(ws + D * C + C, grid, width, 1, han_reduce_to(loss_acc, 1), st);
    if (e != hipSuccess) return (int)e;
    ml_finish_kernel<<<1, 192, 0, st>>>(cslab, grid, loss_acc, (long long *)counts);
    HAN_CHECK_LAUNCH();
    return 0;
}
