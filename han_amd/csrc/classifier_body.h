// The two fused classifier kernels of loss_opt.hip, included once per form (the way sem_attn_fold_body.h shares the K3
// backward): CLS_KERNEL / CLS_WIDE_KERNEL name the kernels, CLS_PARAMS is their parameter list and CLS_ROW(it) the row of
// loop step `it` -- the step itself (han_classifier_loss: a.N rows), or live[it] (han_classifier_loss_live: a.N counts
// the entries of the ascending row list).  A row's arithmetic is the same text either way, so its logits and dZ keep
// their bits.  No include guard: included inside the anonymous namespace of loss_opt.hip, after ClsArgs.

// CM = compile-time bound on the class count (4, 8 or 16): every per-class loop is
// unrolled to CM, so small C does not pay for 16 shuffle reductions per row.
// NV = float4 column groups per lane: the embedding width is D = 64*NV (lane q of a 16-lane
// group owns columns 64v + 4q .. 4q+3, v < NV); NV = 2 serves the 128-wide embeddings.
template <bool BWD, int CM, int NV>
__global__ __launch_bounds__(256) void CLS_KERNEL(CLS_PARAMS) {
    constexpr int D = 64 * NV;
    constexpr int NT = 4 * NV;        // features per lane
    __shared__ float Wm[D * MAXC];
    __shared__ float bm[MAXC];
    const int C = a.C;
    const float invh = 1.f / (float)a.HC;
    for (int i = threadIdx.x; i < D * C; i += 256) {
        float s = 0.f;
        for (int h = 0; h < a.HC; ++h) s += a.Wc[(int64_t)h * D * C + i];
        Wm[i] = s * invh;
    }
    if (threadIdx.x < C) {
        float s = 0.f;
        for (int h = 0; h < a.HC; ++h) s += a.bc[h * C + threadIdx.x];
        bm[threadIdx.x] = s * invh;
    }
    __syncthreads();
    const int q = threadIdx.x & 15;
    const int64_t grp0 = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int64_t ngrp = (int64_t)gridDim.x * 16;
    float dW[NT][CM];
    float dbacc[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        dbacc[c] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) dW[t][c] = 0.f;
    }
    float loss_acc = 0.f, acc_acc = 0.f;
    // this lane's rows of the averaged classifier matrix and the biases, in registers;
    // feature of slot t: 64*(t/4) + 4*q + t%4
    float wq[NT][CM], bq[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        bq[c] = c < C ? bm[c] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) wq[t][c] = c < C ? Wm[(64 * (t >> 2) + 4 * q + (t & 3)) * C + c] : 0.f;
    }
    for (int64_t it = grp0; it < a.N; it += ngrp) {
        const int64_t row = CLS_ROW(it);
        float z[NT];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float4_t z4 = *reinterpret_cast<const float4_t *>(a.Z + row * D + 64 * v + 4 * q);
#pragma unroll
            for (int t = 0; t < 4; ++t) z[4 * v + t] = z4[t];
        }
        float lg[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) s += z[t] * wq[t][c];
            s = cls_row16_sum(s);
            lg[c] = c < C ? s + bq[c] : HAN_NEG_BIG;
        }
        if (q < C) {
            float v = 0.f;
#pragma unroll
            for (int c = 0; c < CM; ++c) v = (q == c) ? lg[c] : v;
            a.logits[row * C + q] = v;
        }
        float mx = lg[0];
        int am = 0;
#pragma unroll
        for (int c = 1; c < CM; ++c)
            if (lg[c] > mx) { mx = lg[c]; am = c; }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < CM; ++c) se += c < C ? __expf(lg[c] - mx) : 0.f;
        const int lab = a.labels[row];
        const float w = a.mask[row] ? a.row_weight : 0.f;
        float llab = 0.f;
#pragma unroll
        for (int c = 0; c < CM; ++c) llab = (c == lab) ? lg[c] : llab;
        if (q == 0) {
            loss_acc += w * (mx + __logf(se) - llab);
            acc_acc += w * (am == lab ? 1.f : 0.f);
        }
        if (BWD) {
            const float inv = 1.f / se;
            float dl[CM];
            float dz[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) dz[t] = 0.f;
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                dl[c] = c < C ? w * (__expf(lg[c] - mx) * inv - (c == lab ? 1.f : 0.f)) : 0.f;
                if (c < C) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        dz[t] += dl[c] * wq[t][c];
                        dW[t][c] += z[t] * dl[c];
                    }
                    if (q == 0) dbacc[c] += dl[c];
                }
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                float4_t o;
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] = dz[4 * v + t];
                *reinterpret_cast<float4_t *>(a.dZ + row * D + 64 * v + 4 * q) = o;
            }
        }
    }
    // block reduction: 16 groups -> one slab row.
    __syncthreads();
    float *scr = Wm;                  // [D*C]
    __shared__ float sc2[MAXC + 2];   // db | loss | acc
    const int grp = threadIdx.x >> 4;
    // Small class counts (the 16 groups' partial rows fit 33 KB of LDS): every group writes its row, ONE barrier,
    // every thread adds the 16 partials of its columns in group order -- instead of 16 barrier rounds through one
    // scratch row (at the size of the reference's data sets those rounds were half of this kernel's 14 us).
    constexpr int PW = D * CM + CM + 2;                 // dW | db | loss | acc of one group
    constexpr bool PAR = PW * 16 * 4 <= 34 * 1024;
    __shared__ float part[PAR ? 16 * PW : 1];
    if (PAR) {
        float *mine = part + grp * PW;
        if (BWD) {
#pragma unroll
            for (int c = 0; c < CM; ++c)
#pragma unroll
                for (int t = 0; t < NT; ++t) mine[(64 * (t >> 2) + 4 * q + (t & 3)) * CM + c] = dW[t][c];
            if (q == 0) {
#pragma unroll
                for (int c = 0; c < CM; ++c) mine[D * CM + c] = dbacc[c];
            }
        }
        if (q == 0) {
            mine[D * CM + CM] = loss_acc;
            mine[D * CM + CM + 1] = acc_acc;
        }
        __syncthreads();
        const int width = D * C + C + 2;
        float *out = a.slab + (int64_t)blockIdx.x * width;
        for (int i = threadIdx.x; i < width; i += 256) {
            int src;                                        // column i of the slab row -> its slot in a group's partial row
            if (i < D * C) src = (i / C) * CM + (i % C);
            else if (i < D * C + C) src = D * CM + (i - D * C);
            else src = D * CM + CM + (i - D * C - C);
            float v = 0.f;
            if (BWD || i >= D * C + C) {
#pragma unroll
                for (int r = 0; r < 16; ++r) v += part[r * PW + src];
            }
            out[i] = v;
        }
        return;
    }
    // larger class bounds: serialise the groups through Wm-sized scratch (one group adds at a time; 16 barriers)
    for (int r = 0; r < 16; ++r) {
        if (grp == r) {
            if (BWD) {
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c < C) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            const int idx = (64 * (t >> 2) + 4 * q + (t & 3)) * C + c;
                            scr[idx] = (r == 0 ? 0.f : scr[idx]) + dW[t][c];
                        }
                        if (q == 0) sc2[c] = (r == 0 ? 0.f : sc2[c]) + dbacc[c];
                    }
                }
            }
            if (q == 0) {
                sc2[MAXC] = (r == 0 ? 0.f : sc2[MAXC]) + loss_acc;
                sc2[MAXC + 1] = (r == 0 ? 0.f : sc2[MAXC + 1]) + acc_acc;
            }
        }
        __syncthreads();
    }
    const int width = D * C + C + 2;
    float *out = a.slab + (int64_t)blockIdx.x * width;
    for (int i = threadIdx.x; i < width; i += 256) {
        float v;
        if (i < D * C) v = BWD ? scr[i] : 0.f;
        else if (i < D * C + C) v = BWD ? sc2[i - D * C] : 0.f;
        else v = sc2[MAXC + (i - D * C - C)];
        out[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// Many classes (16 < C <= 64): one wave per row, lane c = class c.  The averaged classifier column of
// the lane's class and its gradient accumulator live in registers (2*D VGPRs); the row z is broadcast
// element by element with v_readlane (lane d holds z[d], z[d + 64]); softmax statistics are wave
// reductions; dZ is formed by lane d from the LDS copy of the matrix (row stride C_LD = 65: lanes that
// step d hit different banks).  ~ (2D + C) * 3 vector instructions per row -- several times the cost
// per row of the small-C kernel, which keeps 16 rows per block iteration; only used when C > 16.
// ---------------------------------------------------------------------------------------------

template <bool BWD, int NV>
__global__ __launch_bounds__(256) void CLS_WIDE_KERNEL(CLS_PARAMS) {
    constexpr int D = 64 * NV;
    __shared__ float Wl[D * WC_LD];       // averaged matrix [d][c]; reused as the reduction scratch at the end
    __shared__ float sc2[64 + 2];         // db | loss | acc
    const int C = a.C;
    const float invh = 1.f / (float)a.HC;
    for (int i = threadIdx.x; i < D * C; i += 256) {
        float s = 0.f;
        for (int h = 0; h < a.HC; ++h) s += a.Wc[(int64_t)h * D * C + i];
        Wl[(i / C) * WC_LD + (i % C)] = s * invh;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool cls = lane < C;
    float bq = 0.f;
    if (cls)
        for (int h = 0; h < a.HC; ++h) bq += a.bc[h * C + lane];
    bq *= invh;
    float wcol[D], dwcol[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        wcol[d] = cls ? Wl[d * WC_LD + lane] : 0.f;
        dwcol[d] = 0.f;
    }
    float dbacc = 0.f, loss_acc = 0.f, acc_acc = 0.f;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + w, nwaves = (int64_t)gridDim.x * 4;
    for (int64_t it = wave0; it < a.N; it += nwaves) {
        const int64_t row = CLS_ROW(it);
        float z[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) z[v] = a.Z[row * D + 64 * v + lane];
        float lg = bq;
#pragma unroll
        for (int d = 0; d < D; ++d)
            lg += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[d >> 6]), d & 63)) * wcol[d];
        if (cls) a.logits[row * C + lane] = lg;
        const float lgm = cls ? lg : HAN_NEG_BIG;
        float mx = lgm;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const unsigned long long hit = __ballot(cls && lgm == mx);
        const int am = __ffsll((long long)hit) - 1;              // first maximum, as argmax
        const float ex = cls ? __expf(lg - mx) : 0.f;
        const float se = han_wave_sum(ex);
        const int lab = a.labels[row];
        const float wgt = a.mask[row] ? a.row_weight : 0.f;
        const float llab = __shfl(lg, lab, 64);
        if (lane == 0) {
            loss_acc += wgt * (mx + __logf(se) - llab);
            acc_acc += wgt * (am == lab ? 1.f : 0.f);
        }
        if (BWD) {
            const float dl = cls ? wgt * (ex / se - (lane == lab ? 1.f : 0.f)) : 0.f;
            dbacc += dl;
#pragma unroll
            for (int d = 0; d < D; ++d)
                dwcol[d] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[d >> 6]), d & 63)) * dl;
            float dz[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) dz[v] = 0.f;
            for (int c = 0; c < C; ++c) {
                const float dlc = __shfl(dl, c, 64);
#pragma unroll
                for (int v = 0; v < NV; ++v) dz[v] += dlc * Wl[(64 * v + lane) * WC_LD + c];
            }
#pragma unroll
            for (int v = 0; v < NV; ++v) a.dZ[row * D + 64 * v + lane] = dz[v];
        }
    }
    // block reduction: the 4 waves add their dW columns one after the other into the LDS matrix
    __syncthreads();
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww) {
            if (BWD && cls) {
#pragma unroll
                for (int d = 0; d < D; ++d) Wl[d * WC_LD + lane] = (ww == 0 ? 0.f : Wl[d * WC_LD + lane]) + dwcol[d];
                sc2[lane] = (ww == 0 ? 0.f : sc2[lane]) + dbacc;
            }
            if (lane == 0) {
                sc2[64] = (ww == 0 ? 0.f : sc2[64]) + loss_acc;
                sc2[65] = (ww == 0 ? 0.f : sc2[65]) + acc_acc;
            }
        }
        __syncthreads();
    }
    const int width = D * C + C + 2;
    float *out = a.slab + (int64_t)blockIdx.x * width;
    for (int i = threadIdx.x; i < width; i += 256) {
        float v;
        if (i < D * C) v = BWD ? Wl[(i / C) * WC_LD + (i % C)] : 0.f;
        else if (i < D * C + C) v = BWD ? sc2[i - D * C] : 0.f;
        else v = sc2[64 + (i - D * C - C)];
        out[i] = v;
    }
}
