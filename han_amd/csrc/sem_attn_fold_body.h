// The kernel text of sem_attn_fold.h, which includes it once per kernel (K3_FOLD_KERNEL: its name, K3_FOLD_ARGS: its
// argument struct, K3FoldArgs or K3FoldLiveArgs).  No include guard: it is meant to be included twice.
template <int CA, int P>
__global__ __launch_bounds__(256) void K3_FOLD_KERNEL(const float *__restrict__ M, const float *Wg,
                                                    const float *bw, const float *uw,
                                                    const float *beta, const float *dZ,
                                                    float *slab, int64_t N, const K3_FOLD_ARGS fa) {
    using FA = K3_FOLD_ARGS;
    static_assert(P == 1 || P == 2 || P == 4, "a node's rows inside one lane group");
    constexpr bool LIVE = FA::kLive;
    constexpr int A = 64 * CA;
    constexpr int TA = A / 16;
    constexpr int SLABW = 64 * A + 2 * A + P * 64;      // floats per slab row
    using L = B6BwdLds<A>;
    constexpr int WLD2 = L::WLD2, W2LDB = L::W2LDB;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned char *Wt = reinterpret_cast<unsigned char *>(smem);        // G1 B operand: [3][A][SA_WLDB] (transposed [a][k])
    unsigned char *W2s = Wt + L::w2s;                                   // G2 B operand: [3][64 f][W2LDB] (as stored [f][a])
    float *dp = reinterpret_cast<float *>(Wt + L::dp);                  // [4 waves][16][WLD2] fp32
    // b_omega | u_omega: in registers at A = 64; A = 128 has no sixteen registers for them (with them the P = 4 kernel
    // spills four) and reads the two values of a column tile from LDS, as that kernel does for P = 8 / 16
    constexpr bool BU_LDS = CA == 2;
    float *bus = reinterpret_cast<float *>(Wt + L::bus);
    if (BU_LDS)
        for (int it = threadIdx.x; it < 2 * A; it += 256) bus[it] = it < A ? bw[it] : uw[it - A];
    // behind the layout of B6BwdLds: c (P,64)  (A = 128 leaves 12 KB of the CU's 160)
    const float *cs = bus + 2 * A;
    for (int it = threadIdx.x; it < P * 64; it += 256) bus[2 * A + it] = fa.c[it];
    stage_w_t<A, 256, SA_WLDB, false>(Wg, Wt);
    stage_w_fa<CA, 256>(Wg, W2s);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    float bcol[BU_LDS ? 1 : TA], ucol[BU_LDS ? 1 : TA], du[TA], db[TA];
    f32x4 dW[4][TA];
    if constexpr (!BU_LDS) load_bu<TA>(bw, uw, l15, bcol, ucol);
#pragma unroll
    for (int t = 0; t < TA; ++t) {
        du[t] = 0.f;
        db[t] = 0.f;
#pragma unroll
        for (int ft = 0; ft < 4; ++ft) dW[ft][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    float *mydp = dp + w * 16 * WLD2;
    __syncthreads();
    const int64_t R = N * P;
    const int64_t ntiles = (R + 15) / 16;
    // LIVE: the wave's id ring; slot `cur` holds the ids of the tile at hand, the other slot those of the tile behind it
    // (lanes 0 .. 15 write a slot and every lane of the SAME wave reads it later: program order and the wave's in-order
    // LDS keep the two apart, deliberately without a barrier -- as for mydp, the wave's dpre tile)
    int *ring = reinterpret_cast<int *>(bus + 2 * A + P * 64) + w * 32;
    int cur = 0;
    auto slot_after = [](int s) { return s ^ 1; };
    auto load_ids = [&](int64_t tile) {      // node id of tile row l15 (rows past the end: the last row's)
        const int64_t r = tile * 16 + (lane & 15);
        if constexpr (LIVE) return (int)k3_fold_live(fa)[(r < R ? r : R - 1) / P];
        else return 0;
    };
    // node ids of rows 4 l4 + rr of the tile in `slot` (P rows a node: 4 / P ids)
    auto ring_ids = [&](int slot, int l4r, int (&id)[4 / P]) {
#pragma unroll
        for (int k = 0; k < 4 / P; ++k) id[k] = ring[slot * 16 + 4 * l4r + k * P];
    };
    // The rows of a tile come from HBM and with one wave per SIMD nothing else hides that
    // latency, so the row-local inputs (M rows, dZ rows, beta) are fetched ONE TILE AHEAD into
    // registers -- which also pulls the tile into L2 for the strided fragment loads of G1 / G3
    // (3.47 -> 3.20 ms at SYN-1M).
    const int64_t tstride = (int64_t)gridDim.x * 4;
    float4_t mv_n[4], dz_n[4];
    float bt_n[4];
    auto fetch_rows = [&](int64_t tile, int slot) {
        const int64_t g0n = tile * 16 + 4 * l4;
        int id[4 / P];
        if constexpr (LIVE) ring_ids(slot, l4, id);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t row = g0n + rr;
            const bool ok = row < R;
            const int64_t rc = ok ? row : R - 1;
            if constexpr (LIVE) {
                // (a node id the compiler cannot see through, per row: with P > 1 it would otherwise load a node's dZ
                // row once for its P rows, build the products of d beta around the shared operand and round them in
                // another order than the full kernel, which cannot know that rows share a node -- 1 ulp in ds)
                int ndv = id[rr / P];
                asm volatile("" : "+v"(ndv));
                const int64_t nd = ndv;
                const int64_t sr = nd * P + (ok ? rr % P : P - 1);
                mv_n[rr] = *reinterpret_cast<const float4_t *>(M + sr * 64 + 4 * l15);
                dz_n[rr] = *reinterpret_cast<const float4_t *>(dZ + nd * 64 + 4 * l15);
                bt_n[rr] = ok ? beta[sr] : 0.f;
            } else {
            mv_n[rr] = *reinterpret_cast<const float4_t *>(M + rc * 64 + 4 * l15);
            dz_n[rr] = *reinterpret_cast<const float4_t *>(dZ + (rc / P) * 64 + 4 * l15);
            bt_n[rr] = ok ? beta[rc] : 0.f;        // beta is (N,P) flat == row index
            }
        }
    };
    if constexpr (LIVE) {      // the ids of the wave's first two tiles (the only id latency that is not hidden)
        const int64_t t0 = (int64_t)blockIdx.x * 4 + w;
        const int i0 = load_ids(t0), i1 = load_ids(t0 + (int64_t)gridDim.x * 4);
        if (lane < 16) {
            ring[lane] = i0;
            ring[16 + lane] = i1;
        }
    }
    fetch_rows((int64_t)blockIdx.x * 4 + w, 0);
    // What else the row pass reads of rows g0 .. g0 + 3 -- aggp (features 4 l15 .. + 3) and tsum, f1, lse of this
    // lane's head --, requested in front of G2 and in flight under its MFMAs (a tile ahead they would have to live
    // through G1 / G3, where the registers are); a clamped row reads row R - 1's node.  The second tile of a pass
    // also re-reads its M rows (from L2: fetch_rows brought them a tile ago) instead of keeping them through G1 / G3;
    // the first tile's are kept for G3 anyway.
    // The lane's offsets into the fold's tables are formed anew in every tile, from a lane index the compiler cannot
    // see through (fold_lane): formed once, in front of the loop, they take a dozen registers through G1 / G3 that
    // A = 128 does not have -- the kernel then spills.
    float4_t ap_n[4], mo_n[4];
    float ts_n[4], f1_n[4], ls_n[4];
    float4_t dcacc[P];      // dc[p][4 l15 ..] of this lane's rows
#pragma unroll
    for (int p2 = 0; p2 < P; ++p2) dcacc[p2] = (float4_t){0.f, 0.f, 0.f, 0.f};
    auto fold_lane = [&]() {
        int lf = lane;
        asm volatile("" : "+v"(lf));
        return lf;
    };
    auto fetch_fold = [&](int64_t tile, bool with_m, int slot) {
        const int lf = fold_lane(), l15 = lf & 15, l4 = lf >> 4;
        const int64_t g0n = tile * 16 + 4 * l4;
        int id[4 / P];
        if constexpr (LIVE) ring_ids(slot, l4, id);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t row = g0n + rr;
            // 32-bit byte offsets from the tables' (scalar) base pointers -- the entry point admits no N beyond them:
            // 64-bit lane addresses of 6 P tables would be kept in registers across the loop
            uint32_t nn;
            if constexpr (LIVE) nn = (uint32_t)id[rr / P];
            else nn = (uint32_t)((row < R ? row : R - 1) / P);
            const int pp = rr % P;
            const uint32_t hoff = (nn * 8 + (l15 >> 1)) * 4;
            ap_n[rr] = *reinterpret_cast<const float4_t *>(reinterpret_cast<const char *>(fa.aggp[pp]) + (nn * 256 + 16 * l15));
            ts_n[rr] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(fa.tsum[pp]) + hoff);
            f1_n[rr] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(fa.f1[pp]) + hoff);
            ls_n[rr] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(fa.lse[pp]) + hoff);
            if constexpr (LIVE) {
                if (with_m) mo_n[rr] = *reinterpret_cast<const float4_t *>(M + ((int64_t)nn * P + (row < R ? pp : P - 1)) * 64 + 4 * l15);
            } else {
            if (with_m) mo_n[rr] = *reinterpret_cast<const float4_t *>(M + (row < R ? row : R - 1) * 64 + 4 * l15);
            }
        }
    };
    float4_t araw[4];      // G1: this lane's 16 k-values of its row (k = 32 s + 8 l4 + j), one tile ahead
    {
        const int64_t t0 = (int64_t)blockIdx.x * 4 + w;
        int64_t ra = t0 * 16 + l15 < R ? t0 * 16 + l15 : R - 1;
        if constexpr (LIVE) ra = (int64_t)ring[l15] * P + (t0 * 16 + l15 < R ? l15 % P : P - 1);
        const float *mr = M + ra * 64 + 8 * l4;
        araw[0] = *reinterpret_cast<const float4_t *>(mr);
        araw[1] = *reinterpret_cast<const float4_t *>(mr + 4);
        araw[2] = *reinterpret_cast<const float4_t *>(mr + 32);
        araw[3] = *reinterpret_cast<const float4_t *>(mr + 36);
    }
    auto fetch_araw = [&](int64_t tile, int slot) {
        const int lf = fold_lane(), l15 = lf & 15, l4 = lf >> 4;
        const int64_t rn = tile * 16 + l15;
        int64_t ra = rn < R ? rn : R - 1;
        if constexpr (LIVE) ra = (int64_t)ring[slot * 16 + l15] * P + (rn < R ? l15 % P : P - 1);
        const float *mr = M + ra * 64 + 8 * l4;
        araw[0] = *reinterpret_cast<const float4_t *>(mr);
        araw[1] = *reinterpret_cast<const float4_t *>(mr + 4);
        araw[2] = *reinterpret_cast<const float4_t *>(mr + 32);
        araw[3] = *reinterpret_cast<const float4_t *>(mr + 36);
    };
    for (int64_t tile0 = (int64_t)blockIdx.x * 4 + w; tile0 < ntiles; tile0 += 2 * tstride) {
      f32x4 dps[TA];            // dpre of the pass's first tile, kept until the second tile's column tile t is done
      float4_t mvs[4];          // the first tile's rows
      i32x4 mf[4][3];        // G3's A fragments, M^T of both tiles (k-slot (l4, j) = tile j / 4, row 4 l4 + j % 4)
      // the second tile of the last pass may lie past the end: its rows are clamped, beta = 0 makes every one of
      // its contributions zero and its stores are masked
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int64_t tile = tile0 + u * tstride;
        const int64_t r0 = tile * 16;
        const int64_t g0 = r0 + 4 * l4;           // first row of this lane group
        [[maybe_unused]] int id2 = 0;             // LIVE: the ids of the second next tile, on their way
        if constexpr (LIVE) id2 = load_ids(tile + 2 * tstride);
        // ---- d beta, d s inside the lane group (lane = features 4*l15 .. 4*l15+3)
        float ds[4], bt[4];
        float4_t mvc[4], dzc[4];      // this tile's rows: features 4 l15 .. 4 l15 + 3 of rows g0 .. g0 + 3
        {
            float dbt[4];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float4_t mv = mv_n[rr], dz = dz_n[rr];
                mvc[rr] = mv;
                if (u == 0) mvs[rr] = mv;
                dzc[rr] = dz;
                float d = mv[0] * dz[0] + mv[1] * dz[1] + mv[2] * dz[2] + mv[3] * dz[3];
                d = han_row16_sum(d);
                dbt[rr] = d;
                bt[rr] = bt_n[rr];
            }
            fetch_rows(tile + tstride, slot_after(cur));      // next tile: in flight under this tile's MFMAs
#pragma unroll
            for (int k = 0; k < 4 / P; ++k) {
                float S = 0.f;
#pragma unroll
                for (int p2 = 0; p2 < P; ++p2) S += bt[k * P + p2] * dbt[k * P + p2];
#pragma unroll
                for (int p2 = 0; p2 < P; ++p2) ds[k * P + p2] = bt[k * P + p2] * (dbt[k * P + p2] - S);
            }
        }
        if (u == 1) {
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                const float v[8] = {mvs[0][ft], mvs[1][ft], mvs[2][ft], mvs[3][ft],
                                    mvc[0][ft], mvc[1][ft], mvc[2][ft], mvc[3][ft]};
                han_b6_split8(v, mf[ft]);
            }
        }
        // ---- G1: pre = M_tile . Womega
        f32x4 acc[TA];
#pragma unroll
        for (int t = 0; t < TA; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        {
            i32x4 af[2][3];     // G1's A fragments: exact 3-way bf16 split of this tile's rows
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const float v[8] = {araw[2 * s2][0], araw[2 * s2][1], araw[2 * s2][2], araw[2 * s2][3],
                                    araw[2 * s2 + 1][0], araw[2 * s2 + 1][1], araw[2 * s2 + 1][2], araw[2 * s2 + 1][3]};
                han_b6_split8(v, af[s2][0], af[s2][1], af[s2][2]);
            }
            fetch_araw(tile + tstride, slot_after(cur));      // next tile's rows, in flight under the MFMAs
            // G3's A operand is mvc: index i of tile ft = feature 4 i + ft (dpre of a padding row is 0)
            // Column tile by column tile: G1(t) -> dpre(t) -> G3(t).  The VALU work of dpre(t)
            // (tanh, products, LDS store) has no dependence on the MFMAs of G1(t+1), so the
            // scheduler can run it in their shadow instead of after all of G1.
#pragma unroll
            for (int t = 0; t < TA; ++t) {
                {
                    f32x4 c = acc[t];
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        i32x4 b[3];
                        load_b3(Wt + (16 * t + l15) * SA_WLDB + (32 * s2 + 8 * l4) * 2, A * SA_WLDB, b);
                        c = han_b6_chain_k3(af[s2], b, c);
                    }
                    acc[t] = c;
                }
                float bcol_t, ucol_t;
                if constexpr (BU_LDS) {
                    bcol_t = bus[16 * t + l15];
                    ucol_t = bus[A + 16 * t + l15];
                } else {
                    bcol_t = bcol[t];
                    ucol_t = ucol[t];
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const float v = fast_tanh(acc[t][reg] + bcol_t);
                    const float d = ds[reg] * ucol_t * (1.f - v * v);
                    du[t] += ds[reg] * v;
                    db[t] += d;
                    acc[t][reg] = d;
                    mydp[(4 * l4 + reg) * WLD2 + 16 * t + l15] = d;
                }
                // G3 of both tiles' column tile t: dWomega[4 i + ft][16 t + n] += sum over the 32 rows of
                // M[row][4 i + ft] dpre[row][16 t + n]
                if (u == 0) {
                    dps[t] = acc[t];
                } else {
                    const float v[8] = {dps[t][0], dps[t][1], dps[t][2], dps[t][3],
                                        acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
                    i32x4 d[3];
                    han_b6_split8(v, d);
#pragma unroll
                    for (int ft = 0; ft < 4; ++ft) dW[ft][t] = han_b6_chain_k3(mf[ft], d, dW[ft][t]);
                }
            }
        }
        // ---- G2: dMx = dpre . Womega^T   (A operand from the wave's LDS tile)
        // the accumulators start at beta * dZ (the direct term of dM): they end as dM
        fetch_fold(tile, u == 1, cur);
        f32x4 acc2[4];
#pragma unroll
        for (int ft = 0; ft < 4; ++ft)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) acc2[ft][reg] = bt[reg] * dzc[reg][ft];
#pragma unroll
        for (int s2 = 0; s2 < A / 32; ++s2) {       // K = 32 columns of the attention space per step
            i32x4 a[3], b[3];
            g2_afrag<CA>(mydp + l15 * WLD2, s2, l4, a);
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                load_b3(W2s + (16 * ft + l15) * W2LDB + (4 * s2 + l4) * 16, 64 * W2LDB, b);
                acc2[ft] = han_b6_chain_k3(a, b, acc2[ft]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        {
            // ---- the row pass of K2's backward on (dM, M) of rows g0 .. g0 + 3, statement for statement
            const bool elu = fa.act == HAN_ACT_ELU;
            const int lf = fold_lane(), l15 = lf & 15, l4 = lf >> 4;
            const int64_t g0 = r0 + 4 * l4;
            int id[4 / P];
            if constexpr (LIVE) ring_ids(cur, l4, id);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int pp = reg % P;
                const int64_t row = g0 + reg;
                const bool ok = row < R;
                uint32_t nn;
                if constexpr (LIVE) nn = (uint32_t)id[reg / P];
                else nn = (uint32_t)(row / P);
                const float4_t c4 = *reinterpret_cast<const float4_t *>(cs + pp * 64 + 4 * l15);
                float4_t g4;
                float sp = 0.f, dpv = 0.f;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float o = u == 0 ? mvc[reg][t] : mo_n[reg][t];
                    const bool neg = elu && o <= 0.f;
                    const float da = neg ? o + 1.f : 1.f;
                    // (the logarithm of every lane, of 1 where the row pass takes none: no branch around it -- one of
                    // 64 lanes nearly always needs it, and the branches would cut the tile's schedule into pieces)
                    const bool lg = neg && da > 0.f;
                    const float lv = __logf(lg ? da : 1.f);
                    const float pt = neg ? (lg ? lv : 0.f) : o;
                    g4[t] = acc2[t][reg] * da;
                    sp = __builtin_fmaf(g4[t], pt - c4[t], sp);
                    dpv = __builtin_fmaf(g4[t], ap_n[reg][t], dpv);
                }
                sp += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(sp), 0xB1, 0xF, 0xF, true));    // the head's lane pair
                dpv += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(dpv), 0xB1, 0xF, 0xF, true));
                // z of the record (han_hip.h): the magnitude bits of the head's eight g values, ORed -- 0 iff all are +-0
                uint32_t zb = (__float_as_uint(g4[0]) | __float_as_uint(g4[1]) | __float_as_uint(g4[2]) | __float_as_uint(g4[3])) << 1;
                zb |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)zb, 0xB1, 0xF, 0xF, true);
                if (ok) {
                    dcacc[pp] = dcacc[pp] + g4;      // dc: this lane's partial sum, in row order
                    const uint32_t goff = nn * kFoldRowBytes;
                    *reinterpret_cast<float4_t *>(fa.gs[pp] + (goff + 16 * l15)) = g4;
                    if (!(l15 & 1)) {
                        const uint32_t head = l15 >> 1;
                        *reinterpret_cast<float *>(reinterpret_cast<char *>(fa.df1[pp]) + (nn * 8 + head) * 4) =
                            __builtin_fmaf(-sp, ts_n[reg], dpv);
                        *reinterpret_cast<float4_t *>(fa.gs[pp] + (goff + kFoldStatsAt + 16 * head)) =
                            (float4_t){f1_n[reg], ls_n[reg], sp, __uint_as_float(zb == 0u ? HAN_GS_Z_ALL_ZERO : 0u)};
                    }
                }
            }
            if constexpr (LIVE) {      // the tile's slot is free: the ids that arrived under this tile take it
                if (lf < 16) ring[cur * 16 + lf] = id2;
                cur = slot_after(cur);
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
#pragma unroll
    for (int p2 = 0; p2 < P; ++p2)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            dcacc[p2][t] += __shfl_xor(dcacc[p2][t], 16, 64);
            dcacc[p2][t] += __shfl_xor(dcacc[p2][t], 32, 64);
        }
    __syncthreads();
    if (l4 == 0) {      // the dpre tiles are done with: [4 waves][P][64] partial dc
#pragma unroll
        for (int p2 = 0; p2 < P; ++p2) *reinterpret_cast<float4_t *>(dp + (w * P + p2) * 64 + 4 * l15) = dcacc[p2];
    }
    float *red = smem;   // [64*A] dW | [A] db | [A] du  (fits inside the split-Womega region)
    for (int ww = 0; ww < 4; ++ww) {
        if (w == ww) {
#pragma unroll
            for (int ft = 0; ft < 4; ++ft)
#pragma unroll
                for (int t = 0; t < TA; ++t)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int idx = (16 * l4 + 4 * reg + ft) * A + 16 * t + l15;     // feature 4 i + ft, i = 4 l4 + reg
                        red[idx] = (ww == 0 ? 0.f : red[idx]) + dW[ft][t][reg];
                    }
            if (l4 == 0) {
#pragma unroll
                for (int t = 0; t < TA; ++t) {
                    const int idx = 64 * A + 16 * t + l15;
                    red[idx] = (ww == 0 ? 0.f : red[idx]) + db[t];
                    red[idx + A] = (ww == 0 ? 0.f : red[idx + A]) + du[t];
                }
            }
        }
        __syncthreads();
    }
    float *out = slab + (int64_t)blockIdx.x * SLABW;
    for (int i = threadIdx.x; i < 64 * A + 2 * A; i += 256) out[i] = red[i];
    // dc: wave 0 + 1 + 2 + 3, behind dW | db | du
    for (int i = threadIdx.x; i < P * 64; i += 256)
        out[64 * A + 2 * A + i] = ((dp[i] + dp[P * 64 + i]) + dp[2 * P * 64 + i]) + dp[3 * P * 64 + i];
}
