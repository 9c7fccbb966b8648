// K3 in the published form -- semantic attention with ONE weight per meta-path (gfx950).
//
// han.pdf sec. 4.2, eq. 7-9:
//   s_ip = u . tanh(W^T M_ip + b)        (N,P)   never stored
//   w_p  = (1/N) sum_i s_ip              (P)     the node MEAN of each meta-path's score
//   beta = softmax_p(w)                  (P)
//   Z_i  = sum_p beta_p M_ip             (N,D)
// utils/layers.py:156 takes the softmax per node instead (sem_attn.hip); here the P weights are shared by all nodes, so
// the forward needs the scores of every row before any row of Z can be written, and the backward couples every row of
// dM to every row of dZ through P scalars:
//   dbeta_p = sum_i <dZ_i, M_ip>     dw_p = beta_p (dbeta_p - sum_q beta_q dbeta_q)     ds_ip = dw_p / N  for every node
//   dpre_ip = ds_ip u (1 - v_ip^2)   dM_ip = beta_p dZ_i + W dpre_ip
//   dW = sum M_ip (x) dpre_ip        db = sum dpre_ip       du = sum ds_ip v_ip
//
// M is (N,P,D) contiguous = R = N*P rows; row r belongs to meta-path r % P and node r / P.  Every kernel that walks the
// rows does so in tiles of 64 rows per block iteration, one 16-row matrix-pipe tile per wave; P need not divide 16 or
// 64 and a node may straddle a tile or a block's range.
//
// Forward (two reads of M, one write of Z):
//   sem_mean_score_kernel       pre = M_tile . W on exact-fp32 MFMA (W fragments from LDS), tanh, the dot with u and the
//                               fold to one score per row fused; a row's score is added IN DOUBLE to the sum of its
//                               meta-path; one row of P doubles per block goes to a slab
//   sem_mean_fwd_finish_kernel  slab rows added in block order, / N, softmax over P in double -> beta (P floats), w (P doubles)
//   sem_mean_combine_kernel     Z_i = sum_p beta_p M_ip, a streaming kernel with 256-B coalesced row loads
// Backward (two reads of M, one of dZ, one write of dM; one more read of M and a read-modify-write of dM per further
// 64-column slice of the attention space where it is sliced):
//   sem_mean_dbeta_kernel       per-block sum_i <dZ_i, M_ip> in double -> slab
//   sem_mean_bwd_finish_kernel  ds_p = dw_p / N (P floats on the device)
//   sem_mean_bwd_kernel         G1 recomputes pre, G3 = M_tile^T . dpre, G2 = dpre . W^T, epilogue beta_p dZ_i + G2;
//                               dW | db | du per block into a slab, reduced by han_reduce_slabs
// No float atomics, no value through the host, every sum in a fixed order: a call's results are bit-identical from run
// to run.  v (N*P*A floats) is never written.
//
// The helpers restated from sem_attn.hip (fast_tanh, load_bu, row_score) are copies and not shared: with a shared
// helper the compiler schedules the kernels there differently and tools/kernel_diff.py no longer calls them identical.
#include "han_b6.h"

namespace {

__device__ __forceinline__ float fast_tanh(float x) {
    // 1 - 2/(1+e^{2x}) with v_exp_f32 + v_rcp_f32; absolute error ~2e-7, saturates at +-1
    const float e = __expf(2.f * x);
    return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + e);
}

constexpr int ROWS = 64;                 // rows per block iteration (4 waves x 16)
constexpr int kMaxP = 64;                // meta-paths: one lane of a wave each
constexpr int kMeanStreamBlocks = 1024;  // score, d beta and combine kernels: four 4-wave blocks per CU
constexpr int kMeanBwdBlocks = 256;      // main backward pass: one 4-wave block per CU (104 KB of LDS at A = 128)

// b_omega / u_omega of this lane's column in each of the TA 16-column tiles from column `col` on
template <int TA>
__device__ __forceinline__ void load_bu(const float *bw, const float *uw, int col, float (&bcol)[TA], float (&ucol)[TA]) {
#pragma unroll
    for (int t = 0; t < TA; ++t) {
        bcol[t] = bw[col + 16 * t];
        ucol[t] = uw[col + 16 * t];
    }
}

// Score of the accumulator's row `reg` (row 4*l4 + reg of the tile): s = sum_a u_a tanh(pre_a + b_a); every lane of
// the 16-lane group gets the sum.
template <int TA>
__device__ __forceinline__ float row_score(const f32x4 (&acc)[TA], int reg, const float (&bcol)[TA],
                                           const float (&ucol)[TA]) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TA; ++t) s += fast_tanh(acc[t][reg] + bcol[t]) * ucol[t];
    return han_row16_sum(s);
}

// One value per row of a wave's 16-row tile (`vals`, the wave's own LDS line, rows r0 .. r0 + 15) is added to the
// running sum of the row's meta-path: lane p < P owns meta-path p, and adds its rows in row order, in double.
__device__ __forceinline__ void fold_tile(const float *vals, int64_t r0, int64_t R, int P, int lane, double &sum) {
    int p = (int)(r0 % P);
    const int n = R - r0 < 16 ? (int)(R - r0) : 16;
    for (int j = 0; j < n; ++j) {
        if (p == lane) sum += (double)vals[j];
        p = p + 1 == P ? 0 : p + 1;
    }
}

// The four waves' sums of a block, added in wave order, become the block's slab row of P doubles.
__device__ __forceinline__ void block_path_sums(double sum, double (&red)[4][kMaxP], double *slab, int P) {
    red[threadIdx.x >> 6][threadIdx.x & 63] = sum;
    __syncthreads();
    if (threadIdx.x < P) {
        const int p = threadIdx.x;
        slab[(int64_t)blockIdx.x * P + p] = ((red[0][p] + red[1][p]) + red[2][p]) + red[3][p];
    }
}

// sum over the slab rows of column p, in block order
__device__ __forceinline__ double slab_column_sum(const double *slab, int nblocks, int P, int p) {
    double s = 0.0;
    int b = 0;
    for (; b + 8 <= nblocks; b += 8) {      // eight loads in flight; the additions keep the block order
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = slab[(int64_t)(b + j) * P + p];
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; b < nblocks; ++b) s += slab[(int64_t)b * P + p];
    return s;
}

// ---------------------------------------------------------------------------------------------
// Forward, score pass.  LDS: Womega [D][A + 16] (rows k and k+1 hit disjoint bank halves), whole: 139 KB at D = 128,
// A = 256 -- one block per CU there, four at D = 64, A = 128.
// ---------------------------------------------------------------------------------------------
template <int CA, int DT>
__global__ __launch_bounds__(256) void sem_mean_score_kernel(const float *__restrict__ M, const float *Wg,
                                                             const float *bw, const float *uw, double *slab,
                                                             int64_t R, int P) {
    constexpr int D = 16 * DT;
    constexpr int A = 64 * CA;
    constexpr int TA = A / 16;
    constexpr int WLD = A + 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];      // [D][WLD]
    __shared__ float sct[4][16];            // the scores of each wave's tile
    __shared__ double red[4][kMaxP];
    for (int i = threadIdx.x; i < D * A; i += 256) smem[(i / A) * WLD + (i % A)] = Wg[i];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    float bcol[TA], ucol[TA];
    load_bu<TA>(bw, uw, l15, bcol, ucol);
    __syncthreads();
    double sum = 0.0;
    const int64_t nblk = (R + ROWS - 1) / ROWS;
    for (int64_t tb = blockIdx.x; tb < nblk; tb += gridDim.x) {
        const int64_t r0 = tb * ROWS + 16 * w;
        if (r0 >= R) continue;      // the whole wave; there is no block barrier inside the loop
        const int64_t ra = r0 + l15 < R ? r0 + l15 : R - 1;
        const float *mrow = M + ra * D + l4;
        f32x4 acc[TA];
#pragma unroll
        for (int t = 0; t < TA; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int ks = 0; ks < D / 4; ++ks) {
            const float a = mrow[4 * ks];
            const float *wr = smem + (4 * ks + l4) * WLD + l15;
#pragma unroll
            for (int t = 0; t < TA; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[16 * t], acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const float s = row_score<TA>(acc, reg, bcol, ucol);
            if (l15 == 0) sct[w][4 * l4 + reg] = s;
        }
        // the wave reads back its own line: LDS operations of a wave complete in order
        fold_tile(sct[w], r0, R, P, lane, sum);
    }
    block_path_sums(sum, red, slab, P);
}

// One block: w_p = (1/N) sum of the slab rows, beta = softmax over P, both in double.
__global__ __launch_bounds__(64) void sem_mean_fwd_finish_kernel(const double *slab, int nblocks, int P, int64_t N,
                                                                 float *beta, double *wmean) {
    __shared__ double wv[kMaxP];
    const int p = threadIdx.x;
    if (p < P) wv[p] = slab_column_sum(slab, nblocks, P, p) / (double)N;
    __syncthreads();
    if (p < P) {
        double mx = wv[0];
        for (int q = 1; q < P; ++q) mx = wv[q] > mx ? wv[q] : mx;
        double den = 0.0;
        for (int q = 0; q < P; ++q) den += exp(wv[q] - mx);
        beta[p] = (float)(exp(wv[p] - mx) / den);
        if (wmean) wmean[p] = wv[p];
    }
}

// Z_i = sum_p beta_p M_ip: a thread owns four features of a node, D/4 neighbouring lanes one row (256-B or 512-B
// coalesced loads), 1024 / D nodes per block iteration.
template <int DT>
__global__ __launch_bounds__(256) void sem_mean_combine_kernel(const float *__restrict__ M, const float *__restrict__ beta,
                                                               float *Z, int64_t N, int P) {
    constexpr int Q = 4 * DT;       // 16-byte pieces of a row
    __shared__ float bt[kMaxP];
    if (threadIdx.x < P) bt[threadIdx.x] = beta[threadIdx.x];
    __syncthreads();
    const int64_t items = N * Q;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
        const int64_t node = it / Q;
        const int q = (int)(it % Q);
        const float4_t *src = reinterpret_cast<const float4_t *>(M + node * P * (16 * DT)) + q;
        float4_t z = src[0] * bt[0];      // not 0 + ...: with P = 1, Z is M bit for bit
#pragma unroll 4
        for (int p = 1; p < P; ++p) z += src[p * Q] * bt[p];
        reinterpret_cast<float4_t *>(Z)[it] = z;
    }
}

// ---------------------------------------------------------------------------------------------
// Backward, d beta pass: <dZ_{r / P}, M_r> of every row, folded per meta-path like the scores.  A 16-lane group owns a
// row (lane = features 4*l15 .. + 3 of each 64-column part), a wave four rows at a time.
// ---------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void sem_mean_dbeta_kernel(const float *__restrict__ M, const float *__restrict__ dZ,
                                                             double *slab, int64_t N, int P) {
    constexpr int D = 16 * DT;
    constexpr int NQ = D / 64;
    __shared__ float sct[4][16];
    __shared__ double red[4][kMaxP];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int64_t R = N * P;
    double sum = 0.0;
    const int64_t nblk = (R + ROWS - 1) / ROWS;
    for (int64_t tb = blockIdx.x; tb < nblk; tb += gridDim.x) {
        const int64_t r0 = tb * ROWS + 16 * w;
        if (r0 >= R) continue;
        const int64_t n0 = r0 / P;
        const int p0 = (int)(r0 - n0 * P);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int off = 4 * it + l4;
            const int64_t row = r0 + off < R ? r0 + off : R - 1;
            int64_t node = n0 + (p0 + off) / P;
            node = node < N ? node : N - 1;
            float d = 0.f;
#pragma unroll
            for (int f = 0; f < NQ; ++f) {
                const float4_t mv = *reinterpret_cast<const float4_t *>(M + row * D + 64 * f + 4 * l15);
                const float4_t dz = *reinterpret_cast<const float4_t *>(dZ + node * D + 64 * f + 4 * l15);
                d += mv[0] * dz[0] + mv[1] * dz[1] + mv[2] * dz[2] + mv[3] * dz[3];
            }
            d = han_row16_sum(d);
            if (l15 == 0) sct[w][off] = d;
        }
        fold_tile(sct[w], r0, R, P, lane, sum);
    }
    block_path_sums(sum, red, slab, P);
}

// One block: ds_p = beta_p (dbeta_p - sum_q beta_q dbeta_q) / N, in double.
__global__ __launch_bounds__(64) void sem_mean_bwd_finish_kernel(const double *slab, int nblocks, int P, int64_t N,
                                                                 const float *beta, float *ds) {
    __shared__ double dbv[kMaxP];
    const int p = threadIdx.x;
    if (p < P) dbv[p] = slab_column_sum(slab, nblocks, P, p);
    __syncthreads();
    if (p < P) {
        double S = 0.0;
        for (int q = 0; q < P; ++q) S += (double)beta[q] * dbv[q];
        ds[p] = (float)((double)beta[p] * (dbv[p] - S) / (double)N);
    }
}

// ---------------------------------------------------------------------------------------------
// Backward, main pass over the attention columns [a_off, a_off + AS), AS = 16 * TS: the whole width at D = 64,
// A <= 128, else slices of 64 columns (a lane keeps D * AS / 64 dW accumulators); one launch per slice, and the slices
// after the first ADD their dM term.  The tile flow G1 -> dpre -> G3 -> G2 is wave-local: ds and beta depend on the
// row's meta-path alone, so there is no block barrier in the main loop.
// LDS: Womega twice, [D][AS + 16] for G1 | [D][AS + 2] for G2 | dpre [4 waves][16][AS + 2] | ds [64] | beta [64];
// the gradient reduction reuses the two copies of Womega.
// slab row per block: [D*A] dW | [A] db | [A] du   (A = the FULL attention width)
// ---------------------------------------------------------------------------------------------
template <int D, int AS>
struct MeanBwdLds {
    static constexpr int WLD1 = AS + 16;   // G1 B-operand reads: lanes step a, lane groups step f
    static constexpr int WLD2 = AS + 2;    // G2 reads: lanes step f / r, lane groups step a
    static constexpr int w2 = D * WLD1, dp = w2 + D * WLD2, dsl = dp + 4 * 16 * WLD2, btl = dsl + kMaxP;
    static constexpr int red = D * AS + 2 * AS;
    static constexpr size_t bytes = (btl + kMaxP) * sizeof(float);
    static_assert(red <= dp, "the gradient reduction reuses the two copies of Womega");
};

template <int DT, int TS>
__global__ __launch_bounds__(256) void sem_mean_bwd_kernel(const float *__restrict__ M, const float *Wg,
                                                           const float *bw, const float *uw, const float *beta,
                                                           const float *dsp, const float *dZ, float *dM, float *slab,
                                                           int64_t N, int P, int A, int a_off) {
    constexpr int D = 16 * DT;
    constexpr int AS = 16 * TS;
    constexpr int TA = TS;
    using L = MeanBwdLds<D, AS>;
    constexpr int WLD1 = L::WLD1, WLD2 = L::WLD2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *W1 = smem;                         // [D][WLD1]
    float *W2 = smem + L::w2;                 // [D][WLD2]
    float *dp = smem + L::dp;                 // [4 waves][16][WLD2]
    float *dsl = smem + L::dsl;               // [64]  d s of a meta-path
    float *btl = smem + L::btl;               // [64]  beta of a meta-path
    for (int i = threadIdx.x; i < D * AS; i += 256) {
        const float v = Wg[(int64_t)(i / AS) * A + a_off + (i % AS)];
        W1[(i / AS) * WLD1 + (i % AS)] = v;
        W2[(i / AS) * WLD2 + (i % AS)] = v;
    }
    if (threadIdx.x < kMaxP) {
        dsl[threadIdx.x] = threadIdx.x < P ? dsp[threadIdx.x] : 0.f;
        btl[threadIdx.x] = threadIdx.x < P ? beta[threadIdx.x] : 0.f;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    float bcol[TA], ucol[TA], du[TA], db[TA];
    f32x4 dW[DT][TA];
    load_bu<TA>(bw, uw, a_off + l15, bcol, ucol);
#pragma unroll
    for (int t = 0; t < TA; ++t) {
        du[t] = 0.f;
        db[t] = 0.f;
#pragma unroll
        for (int ft = 0; ft < DT; ++ft) dW[ft][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    float *mydp = dp + w * 16 * WLD2;
    __syncthreads();
    const int64_t R = N * P;
    const int64_t nblk = (R + ROWS - 1) / ROWS;
    for (int64_t tb = blockIdx.x; tb < nblk; tb += gridDim.x) {
        const int64_t r0 = tb * ROWS + 16 * w;
        if (r0 >= R) continue;      // the whole wave
        const int64_t n0 = r0 / P;
        const int p0 = (int)(r0 - n0 * P);
        // ---- G1: pre = M_tile . Womega
        f32x4 acc[TA];
#pragma unroll
        for (int t = 0; t < TA; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        {
            const int64_t ra = r0 + l15 < R ? r0 + l15 : R - 1;
            const float *mrow = M + ra * D + l4;
#pragma unroll 8
            for (int ks = 0; ks < D / 4; ++ks) {
                const float a = mrow[4 * ks];
                const float *wr = W1 + (4 * ks + l4) * WLD1 + l15;
#pragma unroll
                for (int t = 0; t < TA; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[16 * t], acc[t], 0, 0, 0);
            }
        }
        // ---- dpre in the accumulator layout (row r = 4*l4 + reg, col a = 16t + l15); rows past the end get d s = 0
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int off = 4 * l4 + reg;
            const float ds = r0 + off < R ? dsl[(p0 + off) % P] : 0.f;
#pragma unroll
            for (int t = 0; t < TA; ++t) {
                const float v = fast_tanh(acc[t][reg] + bcol[t]);
                const float d = ds * ucol[t] * (1.f - v * v);
                du[t] += ds * v;
                db[t] += d;
                acc[t][reg] = d;
                mydp[off * WLD2 + 16 * t + l15] = d;
            }
        }
        // ---- G3: dW += M_tile^T . dpre   (k-step `reg` holds rows 4g + reg, g = lane group)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t rg = r0 + 4 * l4 + reg < R ? r0 + 4 * l4 + reg : R - 1;
            const float *mrow = M + rg * D + l15;
#pragma unroll
            for (int ft = 0; ft < DT; ++ft) {
                const float a = mrow[16 * ft];
#pragma unroll
                for (int t = 0; t < TA; ++t)
                    dW[ft][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, acc[t][reg], dW[ft][t], 0, 0, 0);
            }
        }
        // ---- G2: dMx = dpre . Womega^T   (A operand from the wave's LDS tile)
        f32x4 acc2[DT];
#pragma unroll
        for (int ft = 0; ft < DT; ++ft) acc2[ft] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int ks = 0; ks < AS / 4; ++ks) {
            const float a = mydp[l15 * WLD2 + 4 * ks + l4];
#pragma unroll
            for (int ft = 0; ft < DT; ++ft) {
                const float b = W2[(16 * ft + l15) * WLD2 + 4 * ks + l4];
                acc2[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc2[ft], 0, 0, 0);
            }
        }
        // ---- dM_r = beta_{r % P} dZ_{r / P} + G2
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int off = 4 * l4 + reg;
            const int64_t row = r0 + off;
            if (row < R) {
                const int64_t n = n0 + (p0 + off) / P;
                const float bt = btl[(p0 + off) % P];
#pragma unroll
                for (int ft = 0; ft < DT; ++ft) {
                    const int f = 16 * ft + l15;
                    float *dst = dM + row * D + f;
                    if (a_off == 0) *dst = acc2[ft][reg] + bt * dZ[n * D + f];
                    else *dst += acc2[ft][reg];
                }
            }
        }
    }
    // ---- parameter gradients: lane groups -> waves (LDS) -> slab row
#pragma unroll
    for (int t = 0; t < TA; ++t) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            du[t] += __shfl_xor(du[t], o, 64);
            db[t] += __shfl_xor(db[t], o, 64);
        }
    }
    __syncthreads();
    float *red = smem;   // [D*AS] dW | [AS] db | [AS] du  (fits inside W1 + W2)
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww) {
#pragma unroll
            for (int ft = 0; ft < DT; ++ft)
#pragma unroll
                for (int t = 0; t < TA; ++t)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int idx = (16 * ft + 4 * l4 + reg) * AS + 16 * t + l15;
                        red[idx] = (ww == 0 ? 0.f : red[idx]) + dW[ft][t][reg];
                    }
            if (l4 == 0) {
#pragma unroll
                for (int t = 0; t < TA; ++t) {
                    const int idx = D * AS + 16 * t + l15;
                    red[idx] = (ww == 0 ? 0.f : red[idx]) + db[t];
                    red[idx + AS] = (ww == 0 ? 0.f : red[idx + AS]) + du[t];
                }
            }
        }
        __syncthreads();
    }
    float *out = slab + (int64_t)blockIdx.x * ((int64_t)D * A + 2 * A);
    for (int i = threadIdx.x; i < D * AS; i += 256) out[(int64_t)(i / AS) * A + a_off + (i % AS)] = red[i];
    for (int i = threadIdx.x; i < AS; i += 256) {
        out[(int64_t)D * A + a_off + i] = red[D * AS + i];
        out[(int64_t)D * A + A + a_off + i] = red[D * AS + AS + i];
    }
}

// ---------------------------------------------------------------------------------------------
// Host side.  Workspace: [kMeanStreamBlocks][64] doubles (the score / d beta slab) | ds [64] floats |
// [kMeanBwdBlocks][D*A + 2A] floats (the dW | db | du slab of the backward)
// ---------------------------------------------------------------------------------------------
constexpr size_t kPathSlabBytes = (size_t)kMeanStreamBlocks * kMaxP * sizeof(double);
constexpr size_t kDsBytes = 256;

bool mean_shape_ok(int P, int D, int A) {
    return P >= 1 && P <= kMaxP && (D == 64 || D == 128) && (A == 64 || A == 128 || A == 192 || A == 256);
}

int mean_stream_grid(int64_t R) { return han_grid_for(R, ROWS, kMeanStreamBlocks); }

template <int CA, int DT>
hipError_t launch_score(const float *M, const float *w, const float *b, const float *u, double *slab, int64_t R, int P,
                        hipStream_t st) {
    const size_t lds = (size_t)(16 * DT) * (64 * CA + 16) * sizeof(float);
    return han_launch_lds(sem_mean_score_kernel<CA, DT>, mean_stream_grid(R), 256, lds, st, M, w, b, u, slab, R, P);
}

// the main backward pass: every slice of AS = 16 * TS columns in turn; a block's slab row fills up slice by slice
template <int DT, int TS>
hipError_t launch_bwd_main(const float *M, const float *w, const float *b, const float *u, const float *beta,
                           const float *ds, const float *dZ, float *dM, float *slab, int64_t N, int P, int A, int grid,
                           hipStream_t st) {
    for (int a_off = 0; a_off < A; a_off += 16 * TS) {
        const hipError_t e = han_launch_lds(sem_mean_bwd_kernel<DT, TS>, grid, 256, MeanBwdLds<16 * DT, 16 * TS>::bytes, st,
                                            M, w, b, u, beta, ds, dZ, dM, slab, N, P, A, a_off);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

extern "C" size_t han_sem_attn_mean_workspace(int64_t N, int P, int D, int A) {
    (void)N; (void)P;
    if (D <= 0 || A <= 0) return 0;
    return kPathSlabBytes + kDsBytes + (size_t)kMeanBwdBlocks * ((size_t)D * A + 2 * (size_t)A) * sizeof(float);
}

extern "C" int han_sem_attn_mean_fwd(const float *M, const float *w_omega, const float *b_omega, const float *u_omega,
                                     float *Z, float *beta, double *wmean, void *workspace, size_t workspace_bytes,
                                     int64_t N, int P, int D, int A, int flags, void *stream) {
    (void)flags;
    if (N == 0) return 0;   // nothing to do; row pointers of empty tensors may be null
    if (!M || !w_omega || !b_omega || !u_omega || !Z || !beta || !workspace || ((uintptr_t)workspace & 7) || N < 0 || P <= 0)
        return HAN_E_BADARG;
    if (!mean_shape_ok(P, D, A)) return HAN_E_UNSUPPORTED;
    if (workspace_bytes < han_sem_attn_mean_workspace(N, P, D, A)) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *pslab = (double *)workspace;
    const int64_t R = N * P;
    hipError_t e = hipSuccess;
    HAN_DISPATCH_CA(A, HAN_DISPATCH_BOOL(D128, D == 128,
                                         e = launch_score<CA, D128 ? 8 : 4>(M, w_omega, b_omega, u_omega, pslab, R, P, st)));
    if (e != hipSuccess) return (int)e;
    sem_mean_fwd_finish_kernel<<<1, 64, 0, st>>>(pslab, mean_stream_grid(R), P, N, beta, wmean);
    HAN_CHECK_LAUNCH();
    const int grid = han_grid_for(N * (D / 4), 256, kMeanStreamBlocks);
    if (D == 128) sem_mean_combine_kernel<8><<<grid, 256, 0, st>>>(M, beta, Z, N, P);
    else sem_mean_combine_kernel<4><<<grid, 256, 0, st>>>(M, beta, Z, N, P);
    HAN_CHECK_LAUNCH();
    return 0;
}

extern "C" int han_sem_attn_mean_bwd(const float *M, const float *w_omega, const float *b_omega, const float *u_omega,
                                     const float *beta, const float *dZ, float *dM, float *dw_omega, float *db_omega,
                                     float *du_omega, void *workspace, size_t workspace_bytes, int64_t N, int P, int D,
                                     int A, int flags, void *stream) {
    (void)flags;
    if (N == 0) return 0;
    if (!M || !w_omega || !b_omega || !u_omega || !beta || !dZ || !dM || !dw_omega || !db_omega || !du_omega ||
        !workspace || ((uintptr_t)workspace & 7) || N < 0 || P <= 0)
        return HAN_E_BADARG;
    if (!mean_shape_ok(P, D, A)) return HAN_E_UNSUPPORTED;
    if (workspace_bytes < han_sem_attn_mean_workspace(N, P, D, A)) return HAN_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *pslab = (double *)workspace;
    float *ds = (float *)((char *)workspace + kPathSlabBytes);
    float *slab = (float *)((char *)workspace + kPathSlabBytes + kDsBytes);
    const int64_t R = N * P;
    const int sgrid = mean_stream_grid(R);
    if (D == 128) sem_mean_dbeta_kernel<8><<<sgrid, 256, 0, st>>>(M, dZ, pslab, N, P);
    else sem_mean_dbeta_kernel<4><<<sgrid, 256, 0, st>>>(M, dZ, pslab, N, P);
    HAN_CHECK_LAUNCH();
    sem_mean_bwd_finish_kernel<<<1, 64, 0, st>>>(pslab, sgrid, P, N, beta, ds);
    HAN_CHECK_LAUNCH();
    const int grid = han_grid_for(R, ROWS, kMeanBwdBlocks);
    hipError_t e;
    if (D == 128) e = launch_bwd_main<8, 4>(M, w_omega, b_omega, u_omega, beta, ds, dZ, dM, slab, N, P, A, grid, st);
    else if (A == 128) e = launch_bwd_main<4, 8>(M, w_omega, b_omega, u_omega, beta, ds, dZ, dM, slab, N, P, A, grid, st);
    else e = launch_bwd_main<4, 4>(M, w_omega, b_omega, u_omega, beta, ds, dZ, dM, slab, N, P, A, grid, st);
    if (e != hipSuccess) return (int)e;
    const int width = D * A + 2 * A;
    HanReduceOut o = han_reduce_to(dw_omega, width);
    o.ptr[1] = db_omega; o.ptr[2] = du_omega;
    o.seg_end[0] = D * A; o.seg_end[1] = D * A + A; o.seg_end[2] = width;
    o.nseg = 3;
    return (int)han_reduce_slabs(slab, grid, width, width, o, st);
}
