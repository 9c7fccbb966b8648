// The body of the wave-local K3 forward on the bf16 matrix pipe, included once per form behind the kernel's signature
// (the way sem_attn_fold_body.h shares the backward's text): sem_attn_fwd_wave_b6_kernel in sem_attn.hip with
// K3_FWD_LIVE 0, sem_attn_fwd_wave_b6_live_kernel in sem_attn_fwd_live.h, which adds `live`, with K3_FWD_LIVE 1.
//   0: han_sem_attn_fwd -- tile row r is row r of M (N * P rows).
//   1: han_sem_attn_fwd_live -- the kernel's N is n_live and tile row r is row (live[r / P], r % P) of M: 16 / P nodes
//      of the ascending id list per tile; Z and beta are written at node live[r / P] of the full-size arrays and
//      nothing else is read or written.  Nothing else changes, so the identity list gives the bits of form 0, and a
//      row's bits do not depend on which other rows are listed.  The next tile's M rows stay in flight under the MFMAs;
//      for that the ids are needed one tile further ahead: each wave keeps a ring of two 16-id slots in LDS behind
//      Womega (kFwdRingBytes; slot `cur` = the tile at hand, the other slot = the tile behind it), as
//      sem_attn_bwd_wave_b6_live_kernel does.  Lanes 0 .. 15 write a slot and every lane of the SAME wave reads it
//      later: program order and the wave's in-order LDS keep the two apart, deliberately without a barrier.  Every id
//      index is clamped to the list (rows past the end take the last listed node's last row, as form 0 takes row R - 1).
// Every `#if K3_FWD_LIVE` leaves form 0 the text it was.  No include guard.
{
    constexpr int A = 64 * CA;
    constexpr int TA = A / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // [3][A][128 B], XOR-swizzled: the 16-byte chunk g of row a sits at chunk g ^ ((a >> 1) & 7).  Two 128-B rows span
    // the 64 banks, so the 16 lanes that read chunk g of 16 consecutive rows (8 of each parity) hit 64 different banks
    // WITHOUT padding the rows to 144 B -- 48 KB instead of 54 KB at A = 128: three blocks per CU instead of two (round 3)
    constexpr int FWLDB = B6FwdLds<A>::LDB;
    unsigned char *Wt = reinterpret_cast<unsigned char *>(smem);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    stage_w_t<A, 256, FWLDB, true>(Wg, Wt);
    __syncthreads();
    float bcol[TA], ucol[TA];
    load_bu<TA>(bw, uw, l15, bcol, ucol);
    const int64_t R = N * P;
    const int64_t ntiles = (R + 15) / 16;
    const int64_t tstride = (int64_t)gridDim.x * 4;
    float4_t araw[4];      // the contraction's A operand: this lane's 16 k-values of its row, one tile ahead
#if K3_FWD_LIVE
    int *ring = reinterpret_cast<int *>(Wt + B6FwdLds<A>::bytes) + w * 32;
    int cur = 0;
    auto load_ids = [&](int64_t tile) {      // node id of tile row l15 (rows past the end: the last row's)
        const int64_t r = tile * 16 + l15;
        return (int)live[(r < R ? r : R - 1) / P];
    };
    auto load_arow_live = [&](int64_t tile, int slot) {      // load_arow with the row taken from the ring
        const int64_t rn = tile * 16 + l15;
        const int64_t ra = (int64_t)ring[slot * 16 + l15] * P + (rn < R ? l15 % P : P - 1);
        const float *mr = M + ra * 64 + 8 * l4;
        araw[0] = *reinterpret_cast<const float4_t *>(mr);
        araw[1] = *reinterpret_cast<const float4_t *>(mr + 4);
        araw[2] = *reinterpret_cast<const float4_t *>(mr + 32);
        araw[3] = *reinterpret_cast<const float4_t *>(mr + 36);
    };
    {      // the ids of the wave's first two tiles (the only id latency that is not hidden)
        const int64_t t0 = (int64_t)blockIdx.x * 4 + w;
        const int i0 = load_ids(t0), i1 = load_ids(t0 + tstride);
        if (lane < 16) {
            ring[lane] = i0;
            ring[16 + lane] = i1;
        }
        load_arow_live(t0, 0);
    }
#else
    load_arow(M, (int64_t)blockIdx.x * 4 + w, R, l15, l4, araw);
#endif
    for (int64_t tile = (int64_t)blockIdx.x * 4 + w; tile < ntiles; tile += tstride) {
        const int64_t r0 = tile * 16;
        f32x4 acc[TA];
#pragma unroll
        for (int t = 0; t < TA; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        i32x4 af[2][3];
        split_arow(araw, af);
#if K3_FWD_LIVE
        const int id2 = load_ids(tile + 2 * tstride);      // the ids of the tile after next, in flight under this tile
        load_arow_live(tile + tstride, cur ^ 1);           // next tile, in flight under the MFMAs
        int ids[4];                                        // node of rows 4 l4 + rr of this tile
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) ids[rr] = ring[cur * 16 + 4 * l4 + rr];
#else
        load_arow(M, tile + tstride, R, l15, l4, araw);      // next tile, in flight under the MFMAs
#endif
        float4_t mz[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t row = r0 + 4 * l4 + rr;
#if K3_FWD_LIVE
            mz[rr] = *reinterpret_cast<const float4_t *>(M + ((int64_t)ids[rr] * P + (row < R ? rr % P : P - 1)) * 64 + 4 * l15);
#else
            mz[rr] = *reinterpret_cast<const float4_t *>(M + (row < R ? row : R - 1) * 64 + 4 * l15);
#endif
        }
#pragma unroll
        for (int t = 0; t < TA; ++t) {
            f32x4 c = acc[t];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                i32x4 b[3];
                load_b3(Wt + (16 * t + l15) * FWLDB + (((4 * s2 + l4) ^ ((l15 >> 1) & 7)) * 16), A * FWLDB, b);
                c = han_b6_chain_k3(af[s2], b, c);
            }
            acc[t] = c;
            __builtin_amdgcn_sched_barrier(0);      // keep one column tile's 6 fragment reads in flight, not all 48
        }
        float sc[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sc[reg] = row_score<TA>(acc, reg, bcol, ucol);
#if K3_FWD_LIVE
        wave_node_softmax_live<P>(sc, mz, r0, R, l15, l4, Z, beta, ids);
        if (lane < 16) ring[cur * 16 + lane] = id2;      // the tile's slot is free: the ids that arrived under it take it
        cur ^= 1;
#else
        wave_node_softmax<P>(sc, mz, r0, R, l15, l4, Z, beta);
#endif
    }
}
