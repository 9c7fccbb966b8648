// The two fused multi-label classifier kernels of loss_opt.hip (han_classifier_multilabel), included once per form the
// way classifier_body.h is: ML_KERNEL / ML_WIDE_KERNEL name the kernels, ML_PARAMS is their parameter list and
// ML_ROW(it) the row of loop step `it` -- the step itself, or live[it] for the row list (a.N then counts the entries
// of the list).  A row's arithmetic is the same text either way, so its logits and dZ keep their bits.  The thread
// maps, the register-resident classifier matrix and the block reductions are those of classifier_body.h; what differs
// is the objective: per class the sigmoid cross-entropy term (ml_loss), the gradient (w / C) (sigma - y) from the same
// exponential (ml_sigma), the prediction x > 0, and the integer counts tp | fp | fn of the masked rows, which go to a
// slab of their own (a.cslab, one row of three 64-bit words per block).  Labels: one 64-bit word per row (C <= 64).
// No include guard: included inside an anonymous namespace of loss_opt.hip, after MlArgs.

// slab row: [D*C] dWm | [C] dbm | loss
template <bool BWD, int CM, int NV>
__global__ __launch_bounds__(256) void ML_KERNEL(ML_PARAMS) {
    constexpr int D = 64 * NV;
    constexpr int NT = 4 * NV;        // features per lane
    __shared__ float Wm[D * MAXC];
    __shared__ float bm[MAXC];
    __shared__ unsigned long long cnt[16][3];
    const int C = a.C;
    const float invh = 1.f / (float)a.HC;
    const float invc = 1.f / (float)C;
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
    float loss_acc = 0.f;
    unsigned tp = 0, fp = 0, fn = 0;
    const unsigned cmask = (1u << C) - 1u;      // C <= 16
    float wq[NT][CM], bq[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        bq[c] = c < C ? bm[c] : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) wq[t][c] = c < C ? Wm[(64 * (t >> 2) + 4 * q + (t & 3)) * C + c] : 0.f;
    }
    for (int64_t it = grp0; it < a.N; it += ngrp) {
        const int64_t row = ML_ROW(it);
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
            lg[c] = s + bq[c];
        }
        if (q < C) {
            float v = 0.f;
#pragma unroll
            for (int c = 0; c < CM; ++c) v = (q == c) ? lg[c] : v;
            a.logits[row * C + q] = v;
        }
        const unsigned y = (unsigned)a.bits[row] & cmask;
        const bool on = a.mask[row] != 0;
        const float w = on ? a.row_weight : 0.f;
        float dz[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) dz[t] = 0.f;
        // a row outside the mask adds nothing to the loss, the counts or a gradient: only its logits (above) and a dZ
        // row of zeros (below) are written, and no exponential or logarithm is evaluated for it
        if (on) {
            float ex[CM];
            float rs = 0.f;
            unsigned pm = 0;
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                ex[c] = ml_exp(lg[c]);
                rs += c < C ? ml_loss(lg[c], (y >> c) & 1u, ex[c]) : 0.f;
                pm |= (c < C && lg[c] > 0.f) ? 1u << c : 0u;
            }
            if (q == 0) {
                loss_acc += w * (rs * invc);
                tp += __popc(pm & y);
                fp += __popc(pm & ~y);
                fn += __popc(~pm & y);
            }
            if (BWD) {
                const float wc = w * invc;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c < C) {
                        const float dl = wc * (ml_sigma(lg[c], ex[c]) - (float)((y >> c) & 1u));
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            dz[t] += dl * wq[t][c];
                            dW[t][c] += z[t] * dl;
                        }
                        if (q == 0) dbacc[c] += dl;
                    }
                }
            }
        }
        if (BWD) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                float4_t o;
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] = dz[4 * v + t];
                *reinterpret_cast<float4_t *>(a.dZ + row * D + 64 * v + 4 * q) = o;
            }
        }
    }
    // block reduction: 16 groups -> one slab row, and one row of counts
    const int grp = threadIdx.x >> 4;
    if (q == 0) { cnt[grp][0] = tp; cnt[grp][1] = fp; cnt[grp][2] = fn; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += cnt[r][threadIdx.x];
        a.cslab[(int64_t)blockIdx.x * 3 + threadIdx.x] = s;
    }
    float *scr = Wm;                  // [D*C]
    __shared__ float sc2[MAXC + 1];   // db | loss
    // small class bounds: every group writes its partial row, one barrier, every thread adds the 16 partials of its
    // columns in group order (classifier_body.h)
    constexpr int PW = D * CM + CM + 1;                 // dW | db | loss of one group
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
        if (q == 0) mine[D * CM + CM] = loss_acc;
        __syncthreads();
        const int width = D * C + C + 1;
        float *out = a.slab + (int64_t)blockIdx.x * width;
        for (int i = threadIdx.x; i < width; i += 256) {
            int src;                                        // column i of the slab row -> its slot in a group's partial row
            if (i < D * C) src = (i / C) * CM + (i % C);
            else if (i < D * C + C) src = D * CM + (i - D * C);
            else src = D * CM + CM;
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
            if (q == 0) sc2[MAXC] = (r == 0 ? 0.f : sc2[MAXC]) + loss_acc;
        }
        __syncthreads();
    }
    const int width = D * C + C + 1;
    float *out = a.slab + (int64_t)blockIdx.x * width;
    for (int i = threadIdx.x; i < width; i += 256) {
        float v;
        if (i < D * C) v = BWD ? scr[i] : 0.f;
        else if (i < D * C + C) v = BWD ? sc2[i - D * C] : 0.f;
        else v = sc2[MAXC];
        out[i] = v;
    }
}

// ---------------------------------------------------------------------------------------------
// 16 < C <= 64: one wave per row, lane c = class c (CLS_WIDE_KERNEL's map: the lane's column of the averaged matrix and
// its gradient accumulator in 2*D VGPRs, the row broadcast by v_readlane, dZ from the LDS copy of the matrix).  The
// predictions of a row are one ballot, the counts three popcounts against the row's label word.
// ---------------------------------------------------------------------------------------------
template <bool BWD, int NV>
__global__ __launch_bounds__(256) void ML_WIDE_KERNEL(ML_PARAMS) {
    constexpr int D = 64 * NV;
    __shared__ float Wl[D * WC_LD];       // averaged matrix [d][c]; reused as the reduction scratch at the end
    __shared__ float sc2[64 + 1];         // db | loss
    __shared__ unsigned long long cnt[4][3];
    const int C = a.C;
    const float invh = 1.f / (float)a.HC;
    const float invc = 1.f / (float)C;
    for (int i = threadIdx.x; i < D * C; i += 256) {
        float s = 0.f;
        for (int h = 0; h < a.HC; ++h) s += a.Wc[(int64_t)h * D * C + i];
        Wl[(i / C) * WC_LD + (i % C)] = s * invh;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool cls = lane < C;
    const unsigned long long cmask = C >= 64 ? ~0ull : (1ull << C) - 1ull;
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
    float dbacc = 0.f, loss_acc = 0.f;
    unsigned tp = 0, fp = 0, fn = 0;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + w, nwaves = (int64_t)gridDim.x * 4;
    for (int64_t it = wave0; it < a.N; it += nwaves) {
        const int64_t row = ML_ROW(it);
        float z[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) z[v] = a.Z[row * D + 64 * v + lane];
        float lg = bq;
#pragma unroll
        for (int d = 0; d < D; ++d)
            lg += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[d >> 6]), d & 63)) * wcol[d];
        if (cls) a.logits[row * C + lane] = lg;
        const unsigned long long y = a.bits[row] & cmask;
        const unsigned yl = (unsigned)(y >> lane) & 1u;
        const bool on = __builtin_amdgcn_readfirstlane((int)a.mask[row]) != 0;      // the same byte in every lane
        const float wgt = on ? a.row_weight : 0.f;
        float dz[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) dz[v] = 0.f;
        // wave-uniform (a wave owns the row): a row outside the mask gets its logits and a dZ row of zeros, nothing else
        if (on) {
            const float ex = ml_exp(lg);
            const float rs = han_wave_sum(cls ? ml_loss(lg, yl, ex) : 0.f);
            const unsigned long long pm = __ballot(cls && lg > 0.f);
            if (lane == 0) {
                loss_acc += wgt * (rs * invc);
                tp += __popcll(pm & y);
                fp += __popcll(pm & ~y);
                fn += __popcll(~pm & y);
            }
            if (BWD) {
                const float dl = cls ? (wgt * invc) * (ml_sigma(lg, ex) - (float)yl) : 0.f;
                dbacc += dl;
#pragma unroll
                for (int d = 0; d < D; ++d)
                    dwcol[d] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(z[d >> 6]), d & 63)) * dl;
                for (int c = 0; c < C; ++c) {
                    const float dlc = __shfl(dl, c, 64);
#pragma unroll
                    for (int v = 0; v < NV; ++v) dz[v] += dlc * Wl[(64 * v + lane) * WC_LD + c];
                }
            }
        }
        if (BWD) {
#pragma unroll
            for (int v = 0; v < NV; ++v) a.dZ[row * D + 64 * v + lane] = dz[v];
        }
    }
    // block reduction: the 4 waves add their dW columns one after the other into the LDS matrix
    if (lane == 0) { cnt[w][0] = tp; cnt[w][1] = fp; cnt[w][2] = fn; }
    __syncthreads();
    if (threadIdx.x < 3)
        a.cslab[(int64_t)blockIdx.x * 3 + threadIdx.x] =
            cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww) {
            if (BWD && cls) {
#pragma unroll
                for (int d = 0; d < D; ++d) Wl[d * WC_LD + lane] = (ww == 0 ? 0.f : Wl[d * WC_LD + lane]) + dwcol[d];
                sc2[lane] = (ww == 0 ? 0.f : sc2[lane]) + dbacc;
            }
            if (lane == 0) sc2[64] = (ww == 0 ? 0.f : sc2[64]) + loss_acc;
        }
        __syncthreads();
    }
    const int width = D * C + C + 1;
    float *out = a.slab + (int64_t)blockIdx.x * width;
    for (int i = threadIdx.x; i < width; i += 256) {
        float v;
        if (i < D * C) v = BWD ? Wl[(i / C) * WC_LD + (i % C)] : 0.f;
        else if (i < D * C + C) v = BWD ? sc2[i - D * C] : 0.f;
        else v = sc2[64];
        out[i] = v;
    }
}
