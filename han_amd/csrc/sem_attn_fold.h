// K3 backward with the row-local half of the K2 backward in its epilogue (gfx950): the body and the kernel of
// han_sem_attn_bwd_rows.  Included by sem_attn.hip alone, inside its unnamed namespace, behind the bf16-pipe backward
// kernel whose LDS layout (B6BwdLds), staging and fragment helpers it uses.
#pragma once

// sem_attn_bwd_wave_b6_kernel<CA, P, true> of sem_attn.hip (P <= 4: a node's rows inside one lane group; G3 on the bf16
// pipe) once more, with another epilogue.  Up to G2 the two are to be kept in step statement for statement.  It is a
// second instance and not one body for both because that kernel compiled from a shared body selects other LDS
// instructions (paired reads and writes) than it does from its own text, and the existing kernels are to stay the
// code they were.
// The epilogue: the row-local half of the K2 backward (node_attn.hip: node_attn_bwd_rows_kernel at F' = 8, fp32 tables,
// no residual).  M is the K2 output and dM the row pass's only other row input, and the layouts
// coincide: a lane ends a tile with acc2[ft][reg] = dM[row g0 + reg][4 l15 + ft] and still holds mvc[reg] = M of the
// same four elements -- the row pass's 16-lane group per row, q = l15, head = l15 >> 1.  Row g0 + reg is node
// (g0 + reg) / P, meta-path reg % P (P divides 4).  So dM is not written: the epilogue forms g = dM ELU'(M), the head
// sums s = g . (pre - c) and g . aggp, writes the [g | (f1, lse, s, z) x 8] row of meta-path reg % P's table and
// df1 = g . aggp - s tsum, and adds g to dc[p][4 l15 ..] in registers (lane groups -> waves -> P * 64 more floats of the
// block's slab row at the end).  g, s and df1 are the row pass's bits: its
// roundings (read from its ISA: both head sums are fma chains from 0, df1 is one fma) are written out.
struct K3FoldArgs {
    const float *aggp[4], *tsum[4], *f1[4], *lse[4];   // per meta-path: (N,64) | (N,8) | (N,8) | (N,8)
    char *gs[4];                                       // per meta-path: (N, kFoldRowBytes) [g | stats] rows
    float *df1[4];                                     // per meta-path: (N,8)
    const float *c;                                    // (P,64)
    int act;                                           // HAN_ACT_ELU | HAN_ACT_IDENTITY
    static constexpr bool kLive = false;
};
// han_sem_attn_bwd_rows_live: the tile rows are (live[t], p), t < n_live -- the kernel's N is n_live
struct K3FoldLiveArgs : K3FoldArgs {
    const int32_t *live;                               // (n_live) ascending node ids
    static constexpr bool kLive = true;
};
__device__ __forceinline__ const int32_t *k3_fold_live(const K3FoldArgs &) { return nullptr; }
__device__ __forceinline__ const int32_t *k3_fold_live(const K3FoldLiveArgs &a) { return a.live; }
constexpr int kFoldRowBytes = 384;      // GsRow<8, false> of node_attn.hip: 64 fp32 g | 8 x (f1, lse, s, z)
constexpr int kFoldStatsAt = 256;

// No dM; slab rows of 64 A + 2 A + 64 P floats; P * 256 more bytes of LDS than B6BwdLds.
// FA = K3FoldLiveArgs (LIVE): the same tiles over a row list.  Tile row r is row (live[r / P], r % P) of M, beta and the
// tables and row live[r / P] of dZ; nothing else changes, so the identity list gives the bits of the full kernel.  The
// node ids of a tile are one more level of indirection in front of the one-tile-ahead row fetches, so they are fetched
// TWO tiles ahead: a lane asks for the id of tile row l15 at the top of a tile and holds it through the tile in ONE
// register (A = 128, P = 4 has no three to keep the ids of the current, the next and the second next tile); at the
// tile's end it takes the slot of the tile just done in the wave's ring of two 16-id slots in LDS (kFoldRingBytes
// behind c), from which the fetches read the ids they need when they need them.  The wave alone writes and reads its
// ring.  Every `if constexpr (LIVE)` leaves the full kernel the text it was.
// One text, two kernels: sem_attn_fold_body.h is included once per kernel name and argument struct.  (A template argument
// would put the row-list kernels under the full kernel's name, and a device function called by both makes the compiler
// select other LDS instructions for the full kernel -- paired reads and writes -- than it does from the kernel's own
// text; the full kernel is to stay the code it was.)
constexpr int kFoldRingBytes = 4 * 2 * 16 * (int)sizeof(int);
#define K3_FOLD_KERNEL sem_attn_bwd_wave_b6_fold_kernel
#define K3_FOLD_ARGS K3FoldArgs
#include "sem_attn_fold_body.h"
#undef K3_FOLD_KERNEL
#undef K3_FOLD_ARGS
// han_sem_attn_bwd_rows_live: N = n_live
#define K3_FOLD_KERNEL sem_attn_bwd_wave_b6_live_kernel
#define K3_FOLD_ARGS K3FoldLiveArgs
#include "sem_attn_fold_body.h"
#undef K3_FOLD_KERNEL
#undef K3_FOLD_ARGS
