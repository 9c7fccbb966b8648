/* han_hip.h -- C ABI of libhan_hip.so: the MI355X (gfx950) HAN hot path.
 *
 * Every entry point takes raw DEVICE pointers plus a hipStream_t (passed as
 * void*), launches on that stream, never allocates, never synchronises, and
 * returns 0 on success or a negative HAN_E_* / positive hipError_t code.
 * The caller owns every buffer.  Shapes use the notation of SURVEY.md sec. 8:
 *   N   destination rows owned by this call (local rows of a node partition)
 *   NT  rows of the gather tables (== N on one GPU; local + halo otherwise)
 *   F   input feature width          K  attention heads (n_heads[0])
 *   FP  features per head (hid_units[0])     D = K*FP  (this build: D == 64)
 *   P   meta-paths     A  mp_att_size     C  classes
 * All floating-point data is fp32, row-major, dense; indices are int64
 * (row/col pointers) and int32 (neighbour ids).
 *
 * The reference has no native interface for this path: it is Python on
 * TensorFlow 1.x.  Each function names the reference call site it replaces
 * (paths relative to the reference root); the Python binding that mirrors the
 * reference's own layer API is han_amd/layers.py.
 */
#ifndef HAN_HIP_H
#define HAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAN_ABI_VERSION 15

#define HAN_E_BADARG   (-1)   /* null pointer, negative size, inconsistent shape.  The forward
                              * entry points return 0 at once for N == 0 (empty tensors may
                              * carry null data pointers)                                  */
#define HAN_E_UNSUPPORTED (-2) /* shape outside this build (e.g. K*FP != 64)     */
#define HAN_E_WORKSPACE (-3)  /* workspace too small                            */
#define HAN_E_NOT_ELIGIBLE (-4) /* han_project_fwd_both and han_node_attn_bwd_cols_scores only: valid arguments, but outside
                                 * the forms of the combined kernels; nothing was launched or written, the caller makes the
                                 * two separate calls instead */

#define HAN_ACT_IDENTITY 0
#define HAN_ACT_ELU      1
/* `flags` of han_node_attn_fwd / han_node_attn_bwd_cols */
#define HAN_FLAG_XCD_ORDER 1   /* graph has locality (neighbour ids close to the row id): give the blocks of one
                                  XCD a contiguous share of the rows in flight, so that the eight L2s cache eight
                                  different source windows.  Speed only; off for graphs without structure, where it
                                  measured 9 % slower in the HBM regime (eight separate index / output streams). */

#define HAN_FLAG_LEAN 256      /* small graphs whose table lives in the L2s (a few thousand rows) with long rows -- the reference's own
                                  data sets -- are bound by vector-instruction issue, not by memory.  han_node_attn_fwd then reads
                                  the neighbour scores from f2_src (a 4-byte gather per edge and head) instead of recomputing them,
                                  runs the softmax in log2 units and computes ONE attention-dropout hash per (edge, four heads);
                                  for 8 heads x 8 columns one lane owns a whole head of an edge.  han_node_attn_bwd_cols: the same
                                  hash sharing, and the one-lane-per-head map for 8 x 8.  fp32 tables, table_gid NULL.  Not for
                                  large tables: the score gather would cost a memory line per edge there.                      */
#define HAN_FLAG_K2_DEEP 512    /* measurements only: the bf16 eval forward with 8 steps (32 rows) in flight per wave instead of 4
                                  (rounds 2-3's form: more registers, fewer waves; tools/k2_regimes.py --deep)               */
#define HAN_FLAG_K2_SHARED_HASH 1024 /* measurements only: han_node_attn_fwd, training forward of the 8 x 8 shape with both dropouts
                                  on, with ONE attention-dropout hash per lane and 4-edge step, the other three edges' words taken
                                  from the lane's DPP quad -- bitwise the same draws; no faster          */
#define HAN_FLAG_K2_FULL_GATHER 2048 /* measurements only: han_node_attn_bwd_cols requests the whole g row of every edge, as it did
                                  before the row and chunk kernels learned to leave out what attention dropout makes unused.  By
                                  default a lane loads its part of g_i only where the draw of its own (edge, head) kept the
                                  coefficient; a dropped head contributes exact zeros, so dH and df2 are bitwise those of this
                                  form for finite g.  The one difference: a non-finite g under a DROPPED head no longer turns
                                  the sums into NaN (the full gather multiplies it by zero), a non-finite g under a kept head
                                  still does.  Predicated are fp32 tables with attention dropout, table_gid NULL and no
                                  HAN_FLAG_MASKED_EDGES; every other launch gathers whole rows with or without this flag
                                  (bf16 tables, table_gid, masked edges, the lean, one-lane-per-head and dense kernels).
                                  This flag wins over HAN_FLAG_K2_ZERO_ROWS: the full gather ignores z.                      */
#define HAN_FLAG_K2_ZERO_ROWS 4096 /* han_node_attn_bwd_cols, a hint: most rows of the gs table hold a zero gradient (a one-layer
                                  model whose loss mask covers at most half of the rows).  The predicated launches (see above)
                                  then also leave out the g piece of a head whose statistics record says that it holds only
                                  zeros (z, see the gs row below): such a piece contributes exact zeros, so dH and df2 keep
                                  their bits for finite g, lse and f1.  The g loads then wait for the statistics of their
                                  edge: at N = 1M a loss of 0.05 ms (2.51 -> 2.56, +2 %) where no z is set and a gain of 0.73 ms
                                  (2.51 -> 1.78, -29 %) where nine records in ten have it; hence a flag.  Launches that are
                                  not predicated ignore it, and without it z is not read.                                   */
#define HAN_FLAG_MASKED_EDGES 64 /* han_node_attn_bwd_cols: entries of rowidx below 0 are skipped IN PLACE (their destination's
                                  g row is identically zero -- a destination outside the loss mask of a one-layer model);
                                  the remaining terms are summed in the positions and order of the full pass, so the
                                  results are bit-identical to it.  Opt-in (HANTrainer(masked_backward=True)).          */
#define HAN_FLAG_K2_ROW_SUBSET 8192 /* han_node_attn_fwd: `split` (required) lists exactly the rows to compute -- short_rows,
                                  mid_rows and long_rows together, each row in the set its length puts it in; an empty set
                                  launches nothing (no launch over all N rows).  Rows that are not listed are neither read
                                  nor written in any output, and a listed row gets the bits the full launch gives it (the
                                  same kernels, the same per-row arithmetic, dropout keyed by global ids).  For any head
                                  shape and either table type.  HAN_E_UNSUPPORTED, before any launch, together with
                                  HAN_FLAG_LEAN, with a han_dense_t, or with a non-empty set whose list pointer is NULL
                                  (no identity lists).  For callers that read only some rows of the result: a trainer
                                  whose loss and metrics are sums over a fixed mask (HANTrainer(live_forward=...)).      */
/* `flags` of han_project_fwd: which matrix pipe runs the projection (default 0: the library chooses --
 * the bf16 x 6 kernel for training forwards and bf16 features, the exact-fp32 kernel otherwise).
 * Both have fp32-class accuracy; the switches exist for measurements and tests.                     */
#define HAN_FLAG_K1_EXACT_PIPE  2   /* v_mfma_f32_16x16x4_f32 kernels only                                 */
#define HAN_FLAG_K1_MATRIX_PIPE 4   /* the bf16 x 6 kernel wherever it applies (also the fp32 eval forward) */
#define HAN_FLAG_K1_PAIRS      32   /* measurements only: han_project_fwd_multi fuses 2 meta-paths per block, not 4 */
#define HAN_FLAG_K1_4WAVE      16   /* measurements only: the round-2 form of the bf16 x 6 kernel (4 waves x 2 row tiles,
                                       two waves per SIMD) instead of 8 waves x 1 tile (four per SIMD)                     */
/* han_project_fwd, heads wider than the 64 columns of a K1 / K2 row (hid_units > 64, models/gat.py:42-57): such a head runs
 * as ceil(F'/64) column slices, each a K = 1, F' = 64 call with the SAME seed -- so the slices share the per-head
 * input-dropout and attention-dropout draws, as one head must -- and slice s draws its projected-row dropout
 * (layers.py:31-32, one draw per column) from stream 2 + 4 s.  The caller adds the slices' partial scores
 * (b1 / b2 in slice 0 only) and hands the totals to K2 (han_node_attn_fwd: f2_src).                              */
#define HAN_FLAG_FTS_SLICE(s)     (((s) & 0xFF) << 8)
#define HAN_FLAG_FTS_SLICE_OF(fl) (((fl) >> 8) & 0xFF)
/* `flags` of han_sem_attn_fwd / han_sem_attn_bwd */
#define HAN_FLAG_K3_EXACT_PIPE  8   /* fp32 MFMA kernels also for large inputs (default: bf16 x 6 from 65 536 rows) */
#define HAN_FLAG_K3_PAIRS      16   /* measurements only: han_sem_attn_bwd at mp_att_size = 128 with two waves sharing a tile
                                     * (two waves per SIMD, 64 attention columns each) -- not faster: DESIGN.md section 3 */
#define HAN_FLAG_K3_G3_F32     32   /* measurements only: han_sem_attn_bwd's dW product on the fp32 matrix pipe, tile by tile
                                     * (the round-3 form) instead of two tiles per step on the bf16 pipe                   */

/* storage type of X and of the gather tables H / g ("bf16 feats" of the 10M-node
 * config): everything is accumulated in fp32; any head shape (8 x 8 is the tuned one) */
#define HAN_DTYPE_F32  0
#define HAN_DTYPE_BF16 1

/* Seeds.  Every dropout site is a counter-based hash of (seed, stream, global ids), so a
 * forward, its backward and every node partition regenerate identical masks.  `seed` is
 * passed by value; `seed_dev` (device pointer, or NULL) exists for captured hipGraphs,
 * whose kernel arguments are frozen at capture: when non-NULL the effective seed is
 * splitmix64(seed + *seed_dev), read on the device at kernel start, and the host bumps
 * that device word between replays.  Pass NULL for plain stream launches.            */

int han_abi_version(void);
const char *han_error_string(int code);

/* ---- K1: feature projection + attention scores ---------------------------
 * utils/layers.py:18-24 for all K heads of one meta-path:
 *   Xk = dropout_k(X, keep=1-in_drop)      (re-sampled per head, :18-19)
 *   H[:, k*FP:(k+1)*FP] = Xk @ W[:, k*FP:(k+1)*FP]          (:20)
 *   f1[:,k] = H_k . a1[k] + b1[k];  f2[:,k] = H_k . a2[k] + b2[k]   (:23-24)
 * and the Bernoulli draw of the projected-row dropout (:31-32, which the
 * reference applies AFTER the scores were taken from the undropped rows): when
 * fts_drop > 0 the keep bit of H[n][d] is stamped into mantissa bit 0 of that
 * float (a 1-ulp perturbation seen consistently by f1/f2, K2 and the backward),
 * so that K2 applies the mask while it gathers at no extra memory traffic.
 * X (N,F) ldx>=F (elements; x_dtype fp32 or bf16); W (F,D); a1,a2 (K,FP); b1,b2 (K);
 * H (N,D) in table_dtype (f1/f2 are taken from the rows as stored); f1,f2 (N,K).
 * in_drop == 0 -> no input dropout.  row_offset = global id of row 0 (RNG key).
 * workspace: han_project_fwd_workspace() bytes (short inputs -- fewer 128-row tiles than CUs -- split the
 * reduction over F and sum partial tiles from it in a fixed order; long inputs keep the pre-split image of W
 * there, see below); may be NULL when that is 0.                            */
size_t han_project_fwd_workspace(int64_t N, int F, int K, int FP);
/* Round 4: long inputs (at least 16 384 rows, no split over F) may run on the bf16 x 6 matrix-pipe kernels, which
 * read W from a pre-split, LDS-ready image built in the workspace by a small launch in front of the projection
 * (every block used to split the same W tiles again and store them through 4-way bank conflicts):
 * han_project_fwd_workspace() then returns the image size, ceil(F / 32) * 12 288 bytes -- no longer 0 --, and
 * han_project_fwd_multi_workspace() the size for the P meta-paths of one han_project_fwd_multi call.        */
size_t han_project_fwd_multi_workspace(int64_t N, int F, int K, int FP, int P);
/* Keep table of the per-head input dropout (layers.py:18-19), written by the training forward and
 * read by han_project_bwd so that dW does not regenerate the draws: N rows of F bytes (F % 8 == 0);
 * the 8 bytes of features 8o .. 8o+7 of row n form one little-endian 64-bit word whose bit
 *     32*q + 16*(k % 2) + 4*(k / 2) + i        (q = 0,1; i = 0..3; head k = 0..7)
 * is 1 iff head k keeps feature f = 8o + 4q + i of row n -- i.e. the word IS the 64-lane mask of the
 * dW kernel's v_mfma_f32_4x4x1_16B_f32 A operand, and dW reads it as such: every wave fetches the
 * four words of its 32 features of a row with one scalar load, which has no range check.  A wave whose
 * features begin beyond F reads on into the next row and, from the last row, beyond N*F: the 128 B of
 * slack are what those loads may touch there (at most N*F + 119, han_project_bwd_keep_last_byte();
 * nothing read beyond F reaches a result).  han_project_keep_bytes() returns the size the caller
 * allocates (N*F + 128 B), or 0 when this shape has no table (then pass NULL and the backward
 * regenerates the draws from the seed):
 * built for K == 8, FP == 8, F % 8 == 0, ldx % 4 == 0, N >= 32768 (the matrix-pipe forward).        */
size_t han_project_keep_bytes(int64_t N, int F, int64_t ldx, int K, int FP);
/* Index of the last byte of the keep table that han_project_bwd's scalar loads may touch for an (N, F)
 * input (host-side arithmetic shared with the kernel; added under ABI 15); -1 when N <= 0 or F <= 0.  */
int64_t han_project_bwd_keep_last_byte(int64_t N, int F);
int han_project_fwd(const void *X, int x_dtype, int64_t ldx, const float *W, const float *a1,
                    const float *a2, const float *b1, const float *b2, void *H,
                    int table_dtype, float *f1, float *f2, void *workspace,
                    size_t workspace_bytes, int64_t N, int F, int K, int FP,
                    float in_drop, float fts_drop, uint64_t seed, const uint64_t *seed_dev, int64_t row_offset,
                    uint8_t *keep, int flags, void *stream);

/* All P meta-paths of ONE shared feature matrix in one call (the reference feeds the same matrix to every
 * meta-path: ex_acm3025.py:86, models/gat.py:39).  W (P,F,D), a1/a2 (P,K,FP), b1/b2 (P,K), H (P,N,D),
 * f1/f2 (P,N,K), all contiguous over p; seeds: HOST array of P seeds (may be NULL when in_drop == fts_drop == 0);
 * keep: NULL or P tables, han_project_keep_bytes() apart.  The eval forward of long inputs (no dropout, P >= 2,
 * N >= 16384 -- N >= 32641 from F = 128, where shorter inputs split F --, 16-byte aligned rows) runs fused: X is
 * read, split and staged once for 4 (or 2) meta-paths per block; an odd last meta-path and every other case is a
 * loop over han_project_fwd, with the same results.                                                    */
int han_project_fwd_multi(const void *X, int x_dtype, int64_t ldx, const float *W, const float *a1,
                          const float *a2, const float *b1, const float *b2, void *H, int table_dtype,
                          float *f1, float *f2, void *workspace, size_t workspace_bytes, int64_t N,
                          int F, int K, int FP, int P, float in_drop, float fts_drop,
                          const uint64_t *seeds, const uint64_t *seed_dev, int64_t row_offset,
                          uint8_t *keep, int flags, void *stream);

/* The training forward AND the eval forward of P meta-paths in ONE pass over X per meta-path (added under ABI 15: new
 * entry points only, nothing existing changed).  For a trainer whose eval forward of epoch t and training forward of
 * epoch t + 1 project the same X with the same parameters: the training kernel already holds the unmasked X fragments
 * in registers, so the eval products ride along and the eval forward's own read, split and staging of X goes.
 * Arguments as han_project_fwd_multi (in_drop / fts_drop / seeds / keep are the TRAINING forward's) plus the eval
 * outputs H_eval (P,N,D), f1_eval / f2_eval (P,N,K).  On return 0
 *   H, f1, f2, keep      hold the bytes han_project_fwd_multi writes with the same seeds and dropout rates,
 *   H_eval, f1_eval, f2_eval   the bytes it writes with in_drop == fts_drop == 0.
 * It runs only where both of those calls would take the matrix-pipe kernels for every meta-path -- fp32 X and fp32
 * tables, in_drop > 0, a keep table (han_project_keep_bytes() != 0 and keep != NULL), P even, 16-byte aligned rows
 * with F % 4 == 0, neither HAN_FLAG_K1_EXACT_PIPE nor HAN_FLAG_K1_4WAVE -- and returns HAN_E_NOT_ELIGIBLE everywhere
 * else, after the argument checks of han_project_fwd_multi (same order, same codes) and before any launch.
 * X MUST BE FINITE: the two heads of a 16-column tile share an accumulator (each multiplied against zeros in the
 * other's columns), so a kept Inf / NaN of one head turns its sibling's columns of that row into NaN, where the
 * separate training forward keeps a non-finite value inside its own head.
 * workspace: han_project_fwd_both_workspace() bytes (the W images of the P meta-paths).  N == 0 returns 0.   */
size_t han_project_fwd_both_workspace(int64_t N, int F, int K, int FP, int P);
int han_project_fwd_both(const void *X, int x_dtype, int64_t ldx, const float *W, const float *a1,
                         const float *a2, const float *b1, const float *b2, void *H, int table_dtype,
                         float *f1, float *f2, void *H_eval, float *f1_eval, float *f2_eval, void *workspace,
                         size_t workspace_bytes, int64_t N, int F, int K, int FP, int P, float in_drop,
                         float fts_drop, const uint64_t *seeds, const uint64_t *seed_dev, int64_t row_offset,
                         uint8_t *keep, int flags, void *stream);

/* dW = Xk^T dH.  keep: the table the forward of the SAME seed wrote (then no draw is regenerated), or
 * NULL: per head dropout masks regenerated from the seed.
 * workspace: han_project_bwd_workspace() bytes, any contents.              */
size_t han_project_bwd_workspace(int64_t N, int F, int K, int FP);
int han_project_bwd(const void *X, int x_dtype, int64_t ldx, const float *dH, float *dW,
                    void *workspace, size_t workspace_bytes, int64_t N, int F, int K,
                    int FP, float in_drop, uint64_t seed, const uint64_t *seed_dev, int64_t row_offset,
                    const uint8_t *keep, void *stream);

/* dX = sum_k mask_k/keep * (dH_k W_k^T): gradient w.r.t. the layer INPUT, needed only
 * for layers >= 1 of a multi-layer stack (models/gat.py:48-57).  dH (N,D); W (F,D);
 * dX (N,F) with row stride ldo (a slice of the previous layer's dM).            */
int han_project_bwd_input(const float *dH, const float *W, float *dX, int64_t ldo, int64_t N,
                          int F, int K, int FP, float in_drop, uint64_t seed, const uint64_t *seed_dev,
                          int64_t row_offset, void *stream);

/* ---- K1 sparse: the first-layer projection of a CSR feature matrix (ABI 10) ----
 * Bag-of-words features are almost all zero, and input dropout (layers.py:18-19) multiplies elements: a zero stays
 * a zero whatever its draw.  These two entry points visit only the stored entries and regenerate exactly the draws
 * the dense kernels use (counter (global row, f * ceil(K/4) + k/4), field k % 4), so they compute what
 * han_project_fwd / han_project_bwd compute on the densified matrix, up to the order of the fp32 sums.
 *
 * han_project_sparse_fwd: the contract of han_project_fwd with the CSR triple in place of X, x_dtype, ldx:
 *   rowptr (N+1) int64, colidx (nnz) int32 in [0, F), vals (nnz) fp32 or NULL (every stored entry is 1);
 *   H[n, d] = 1/keep * sum_e vals[e] * keep_{d/FP}(n + row_offset, colidx[e]) * W[colidx[e], d];
 * the epilogue (projected-row dropout bit, HAN_FLAG_FTS_SLICE, bf16 rounding, f1 / f2 from the row as stored) is
 * han_project_fwd's.  A row without entries stores the (stamped) zero and gets f1 = b1, f2 = b2.  No workspace and no
 * keep table: dW regenerates the draws.  N == 0 returns 0 at once; N >= 2^31: HAN_E_UNSUPPORTED.                */
int han_project_sparse_fwd(const int64_t *rowptr, const int32_t *colidx, const float *vals, const float *W,
                           const float *a1, const float *a2, const float *b1, const float *b2, void *H,
                           int table_dtype, float *f1, float *f2, int64_t N, int F, int K, int FP,
                           float in_drop, float fts_drop, uint64_t seed, const uint64_t *seed_dev,
                           int64_t row_offset, int flags, void *stream);

/* han_project_sparse_bwd: dW (F,D) from the TRANSPOSED (CSC) image of the matrix: colptr (F+1) int64, rowidx (nnz)
 * int32 in [0, N), ascending within a column, vals_t (nnz) or NULL;
 *   dW[f, d] = 1/keep * sum over the stored (n, f) of vals * keep_{d/FP}(n + row_offset, f) * dH[n, d].
 * No float atomics: a wave sums a column in a fixed order, so the result is bitwise reproducible.  EVERY row of dW
 * is written on every call (a feature without entries gets an exact zero row; N == 0 zeroes dW).
 * A column can be as long as N, so the columns with more than col_chunk entries ("long": long_cols (n_long) int32,
 * ascending) are cut into chunks of at most col_chunk entries: chunk c covers the entries [chunk_start[c],
 * chunk_end[c]) of column chunk_col[c] (int64 / int64 / int32, n_chunks each), the chunks of long_cols[i] are
 * [long_ptr[i], long_ptr[i+1]) (int64, n_long + 1), in entry order.  A wave per chunk writes a partial row to the
 * workspace (han_project_sparse_bwd_workspace(n_chunks) bytes, any contents) and a second launch adds a column's
 * partial rows in ascending chunk order.  n_long == 0: the chunk arguments and the workspace may be NULL.       */
size_t han_project_sparse_bwd_workspace(int64_t n_chunks);
int han_project_sparse_bwd(const int64_t *colptr, const int32_t *rowidx, const float *vals_t, int64_t col_chunk,
                           int64_t n_long, int64_t n_chunks, const int32_t *long_cols, const int64_t *long_ptr,
                           const int32_t *chunk_col, const int64_t *chunk_start, const int64_t *chunk_end,
                           const float *dH, float *dW, void *workspace, size_t workspace_bytes, int64_t N, int F,
                           int K, int FP, float in_drop, uint64_t seed, const uint64_t *seed_dev,
                           int64_t row_offset, void *stream);

/* Degree bins and row splitting for skewed graphs (optional; pass NULL for none: the library then picks ONE row
 * shape for the whole launch from E / N).
 * Bins (round 4): real meta-path graphs mix rows of a few entries with rows of thousands (DBLP APA: mean 2.7, max
 * 46; the power-law workload of SURVEY.md section 8d).  With n_short + n_mid > 0 the launch is degree-binned:
 *   short_rows (n_short, int32 row ids): rows with fewer than HAN_SHORT_DEG entries (incl. empty rows) -- one 16-lane
 *       group per row, four rows per wave, the row's ids one coalesced load; best ordered by ceil(deg / 4), then id,
 *       so that the four rows of a wave need the same number of steps;
 *   mid_rows (n_mid): rows of HAN_SHORT_DEG .. split_deg entries -- a wave per row;
 *   rows beyond split_deg: the chunks below.
 * A list pointer may be NULL when its bin holds every row of the launch (n == N: identity).  Every row must be in
 * exactly one of the three sets (under HAN_FLAG_K2_ROW_SUBSET of han_node_attn_fwd: every row TO COMPUTE, and no
 * other); each row is processed by one fixed kernel in a fixed order (bitwise reproducible).
 * Splitting: rows (sources, in the backward) with more than split_deg stored entries are skipped by the main
 * launch; each is cut into chunks of consecutive edges [chunk_start, chunk_end),
 * one wave per chunk produces a partial state in `workspace`, and a finishing
 * launch merges a row's chunks in order (deterministic).  chunk_long[c] indexes
 * long_rows; long_ptr (n_long+1) gives each long row's chunk range.  n_long == 0: no row is split (the chunk
 * fields are then not read; split_deg must still bound the rows listed in mid_rows).            */
#define HAN_SHORT_DEG 16
typedef struct han_row_split {
    int64_t split_deg, n_long, n_chunks;
    const int64_t *long_rows, *long_ptr;
    const int32_t *chunk_long;
    const int64_t *chunk_start, *chunk_end;
    void *workspace;
    size_t workspace_bytes;       /* >= han_row_split_workspace(n_chunks) */
    int64_t n_short, n_mid;       /* degree bins; both 0: not binned */
    const int32_t *short_rows, *mid_rows;
} han_row_split_t;
size_t han_row_split_workspace(int64_t n_chunks);

/* Small dense graphs on the matrix pipe (round 4; optional, pass NULL for none).  The reference computes its heads
 * densely -- N x N logits, an additive mask, matmul(coefs, seq_fts): utils/layers.py:26-34 -- and its own data sets ARE
 * dense (ACM PSP 24 % of all pairs, DBLP APCPA / APTPA 30 % / 78 %).  With a han_dense_t the forward / the transposed-
 * graph backward run as 16 x 16 x 4 fp32 MFMA tiles over an adjacency BIT MASK, with the exponential taken out of the
 * inner loop (exp(LeakyReLU(x)) = max(e^x, e^0.2x): per-node factors).  Built for 8 heads x 8 columns, fp32 tables,
 * table_gid NULL, edge_val NULL, graphs without repeated entries (han_csr_to_bitmask counts them), HAN_FLAG_LEAN set and
 * f2_src given: when the per-head range of the scores exceeds 80 (checked on the device) the lean CSR kernel runs
 * instead, in the same call.  bits: [rows][ld_words] 32-bit words, bit (j & 31) of word (j >> 5) of row i set iff the
 * graph stores the entry (i, j); n_table = rows of the table the columns index.                                        */
typedef struct han_dense {
    const uint32_t *bits;
    int64_t ld_words;             /* >= ceil(n_table / 32) */
    int64_t n_table;
    void *workspace;              /* 16-byte aligned */
    size_t workspace_bytes;       /* >= han_node_attn_dense_workspace(rows, n_table, train) */
} han_dense_t;
size_t han_node_attn_dense_workspace(int64_t rows, int64_t n_table, int train);
/* CSR -> bit mask.  *repeated (device int, or NULL) receives the number of entries that were already present (entries outside
 * [0, n_table) -- e.g. the -1 of HAN_FLAG_MASKED_EDGES graphs -- are skipped and counted too: such a graph has no dense form).
 * Launches a memset of bits (and of *repeated) and one kernel on `stream`.                                     */
int han_csr_to_bitmask(const int64_t *rowptr, const int32_t *colidx, int64_t N, int64_t n_table,
                       uint32_t *bits, int64_t ld_words, int *repeated, void *stream);

/* ---- K2: node-level attention ---------------------------------------------
 * utils/layers.py:26-35,46 (dense mask form) == :95-118,127 (sparse form) over
 * the stored neighbours only:
 *   e_ij = LeakyReLU(f1_i + f2_j), alpha = softmax_j, out_i = act(sum_j
 *   drop(alpha_ij) drop(H_j) + c).
 * rowptr (N+1) int64, colidx (E) int32 indexing the NT-row table H (NT,D) (the
 * UNDROPPED projected rows; with fts_drop > 0 bit 0 of every element is its keep
 * bit, as han_project_fwd stamped it); the neighbour score
 * f2_j = H_j[k].a2[k] + b2[k] is recomputed from the gathered row.  table_gid (NT)
 * int32 or NULL: the GLOBAL node id of each table row when the table is a
 * [local | halo] table of a node partition (the dropout RNG is keyed by global
 * ids); NULL means the table index is the global id.  res (N,D) or NULL: the
 * residual term conv1d(seq, F', 1) of layers.py:38-40, added before the activation.
 * edge_val (E) fp32 in colidx order or NULL: the stored values of sp_attn_head's
 * SparseTensor adj_mat, which SCALE the logits (e_ij = LeakyReLU(v_ij*(f1_i+f2_j)),
 * layers.py:95-98) -- NULL is the binary adjacency every shipped config uses.
 * f1 (N,K) for the local rows; a2 (K,FP); b2 (K); c (D).  out row i is written
 * at out + i*out_stride (so the K heads land directly in M[:,p,:],
 * models/gat.py:46,58-60).  Training extras (lse, aggp, tsum: all or none NULL; pre: optional, the
 * backward does not need it): pre (N,D)
 * pre-activation, lse (N,K) log-sum-exp of the scores, aggp (N,D) and tsum (N,K)
 * -- the LeakyReLU'-weighted aggregates that make df1 row-local in the backward.
 * f2_src (NT,K) or NULL: the scores of the table rows.  With K = 1, F' = 64 the neighbour score is GATHERED from
 * this table instead of being recomputed from the row -- the slices of a head wider than 64 columns share the
 * head's scores (f1 / f2_src then hold the totals over the slices; a2 / b2 are not read); with HAN_FLAG_LEAN the
 * lean kernels read it for any head shape; otherwise it is not read.  The backward needs nothing
 * new: han_node_attn_bwd_cols already takes f2 and df1 as inputs, and its slices' df1 / df2 add up (the
 * softmax backward is linear in d alpha); the caller adds (df2_total - df2_slice) x a2_slice to dH.          */
int han_node_attn_fwd(const int64_t *rowptr, const int32_t *colidx, const float *edge_val,
                      const void *H,
                      int table_dtype, const int32_t *table_gid, const float *f1, const float *f2_src,
                      const float *a2, const float *b2, const float *c, const float *res,
                      float *out, int64_t out_stride, float *pre, float *lse, float *aggp,
                      float *tsum, int64_t N, int64_t E, int K, int FP, float slope,
                      float coef_drop, float fts_drop, uint64_t seed, const uint64_t *seed_dev, int64_t row_offset,
                      int activation, int flags, const han_row_split_t *split, const han_dense_t *dense, void *stream);

/* The attention coefficients themselves (attn_head(..., return_coef=True),
 * utils/layers.py:27-30,43-44; models/gat.py:143-172 averages them over the heads):
 * coef[e*K+k] = drop(alpha_ij)[k] for the stored entry e = (i,j) in CSR order, or with
 * mean_heads != 0 coef[e] = mean_k of those.  f1, f2 (N,K)/(NT,K) as han_project_fwd
 * wrote them; coef_drop/seed/row_offset/table_gid as in the forward (so the draws are
 * the ones that forward used).  Diagnostic output: not used by training.            */
int han_node_attn_coefs(const int64_t *rowptr, const int32_t *colidx, const float *edge_val,
                        const int32_t *table_gid, const float *f1, const float *f2, float *coef,
                        int mean_heads, int64_t N, int64_t E, int K, int FP, float slope,
                        float coef_drop, uint64_t seed, const uint64_t *seed_dev, int64_t row_offset, void *stream);

/* Backward tables: ONE fused row per destination i,
 *   [ g_i : D elements of table_dtype | (f1_i, lse_i, s_i, z_i)[k] : 4 x 32 bits per head k ]
 * padded to whole 128-B lines; han_gs_row_bytes() gives the row size (K = 8, F' = 8: 384 B with
 * fp32 g, 256 B with bf16 g).  Under a node partition this is the ONLY table the backward moves
 * per meta-path (one collective instead of one for g and one for the statistics).
 * z, the fourth word of a record, is read as bits: 0 = the F' stored g values of head k in row i may be
 * anything; any non-zero pattern = all of them are +0 or -0.  The library's producers write
 * HAN_GS_Z_ALL_ZERO exactly where that holds, 0 elsewhere.  Under HAN_FLAG_K2_ZERO_ROWS the predicated
 * launches of han_node_attn_bwd_cols do not request the g piece of a head whose z is set -- with finite
 * statistics (f1, lse: a finite coefficient) it could only add zeros; with a non-finite coefficient the
 * full gather yields NaN (inf * 0) where this form does not, as for a non-finite g under a dropped head.
 * z is an optimisation only: 0 everywhere is always correct (it is what tables written before the word
 * had a meaning hold).  A caller that builds gs rows itself writes 0 or, where it knows the head's g to
 * be all zero, HAN_GS_Z_ALL_ZERO -- never garbage.                                             */
#define HAN_GS_Z_ALL_ZERO 0x3F800000u   /* the bits of 1.0f: survives any float view of the record */
size_t han_gs_row_bytes(int K, int FP, int table_dtype);

/* Backward, step 1 (row-local): from dOut (N,D; row stride dout_stride), the forward's OUTPUT rows `out`
 * (N,D; row stride out_stride -- e.g. M[:,p,:]) and the saved aggp/tsum/f1/lse compute
 *   pre = act^-1(out): identity, or for ELU  out > 0: out,  out <= 0: log(out + 1)  (round 3: the pre-activation
 *         is no longer stored -- 256 B per row less to write, to keep and to read; act'(pre) = out > 0 ? 1 : out + 1)
 *   g = dOut * act'(pre)   (rounded to table_dtype; the sums below use the rounded value)
 *   s_i[k] = g_i[k] . (pre_i - c)[k]
 *   df1_i[k] = g_i[k] . aggp_i[k] - s_i[k] * tsum_i[k]        -> df1 (N,K)
 *   z_i[k] = HAN_GS_Z_ALL_ZERO if every stored g_i[k] is +-0, else 0
 *   gs row i = [ g_i | (f1, lse, s, z)[k] ]                    -> gs (N rows of han_gs_row_bytes())
 *   dc += sum_i g_i  (written, not accumulated; unrounded g)  -> dc (D)
 * workspace: han_node_attn_bwd_workspace() bytes.                          */
size_t han_node_attn_bwd_workspace(int64_t N, int K, int FP);
int han_node_attn_bwd_rows(const float *dOut, int64_t dout_stride, const float *out, int64_t out_stride,
                           const float *aggp, const float *tsum, const float *f1,
                           const float *lse, const float *c, const float *res, void *gs,
                           int table_dtype, float *df1, float *dc, void *workspace,
                           size_t workspace_bytes, int64_t N, int K, int FP, int activation,
                           void *stream);

/* Backward, step 2 (gather over the TRANSPOSED graph, no float atomics):
 * colptr (NS+1) / rowidx (E) list, for each source row j owned by this call,
 * the destination rows i (indices into the NT-row fused table gs).  Produces for each source j
 *   df2_j[k] = sum_i dl_ij,   dH_j = mH_j/keep * sum_i drop(alpha_ij) g_i
 *                                     + df1_j a1 + df2_j a2
 * H (keep bits in bit 0 when fts_drop > 0), f2, df1 are the NS local source rows;
 * dH (NS,D), df2 (NS,K) outputs.
 * src_offset / the ids in rowidx + dst_offset are the global ids used as RNG
 * keys (must match the forward).  edge_val (E) or NULL: the forward's adjacency
 * values permuted into the transposed graph's order.                         */
int han_node_attn_bwd_cols(const int64_t *colptr, const int32_t *rowidx, const float *edge_val,
                           const void *gs, const int32_t *table_gid, const void *H,
                           int table_dtype, const float *f2,
                           const float *df1, const float *a1, const float *a2,
                           float *dH, float *df2, int64_t NS, int64_t E, int K, int FP, float slope,
                           float coef_drop, float fts_drop, uint64_t seed, const uint64_t *seed_dev,
                           int64_t src_offset, int64_t dst_offset, int flags,
                           const han_row_split_t *split, const han_dense_t *dense, void *stream);

/* Backward, steps 2 AND 3 in one pass: han_node_attn_bwd_cols, and the gather also takes
 * han_score_param_bwd's sums over ALL NS source rows -- da1, da2 (K,FP), db1, db2 (K) from H as stored (keep bit
 * included, not masked, not scaled), df1 and the df2 it writes -- instead of a second pass over H, df1 and df2.
 * dH and df2 are the BYTES of han_node_attn_bwd_cols.  The sums are taken per block and then over the blocks in a fixed
 * order (no float atomics): the same bits from call to call, within rounding of han_score_param_bwd's, whose order
 * differs.  Only the row kernels have this form.  Returns, after every argument check and with nothing launched or
 * written, HAN_E_NOT_ELIGIBLE for: NS == 0; HAN_FLAG_LEAN or HAN_FLAG_MASKED_EDGES; `dense` with a bit mask; a `split`
 * with long rows (n_long > 0) or whose bins do not list every source row.  The caller then makes the two calls.
 * Check order: null pointers and sizes (HAN_E_BADARG), shapes and dtypes (HAN_E_UNSUPPORTED), dropout rates
 * (HAN_E_BADARG), workspace_bytes (HAN_E_WORKSPACE), eligibility.                                             */
size_t han_node_attn_bwd_cols_scores_workspace(int64_t NS, int K, int FP);
int han_node_attn_bwd_cols_scores(const int64_t *colptr, const int32_t *rowidx, const float *edge_val,
                                  const void *gs, const int32_t *table_gid, const void *H,
                                  int table_dtype, const float *f2,
                                  const float *df1, const float *a1, const float *a2,
                                  float *dH, float *df2, int64_t NS, int64_t E, int K, int FP, float slope,
                                  float coef_drop, float fts_drop, uint64_t seed, const uint64_t *seed_dev,
                                  int64_t src_offset, int64_t dst_offset, int flags,
                                  const han_row_split_t *split, const han_dense_t *dense, float *da1, float *da2,
                                  float *db1, float *db2, void *workspace, size_t workspace_bytes, void *stream);

/* Backward, step 3: gradients of the score parameters
 *   da1[k,f] = sum_n df1[n,k] H[n,k,f]   da2 likewise with df2
 *   db1[k] = sum_n df1[n,k]              db2[k] = sum_n df2[n,k]            */
size_t han_score_param_bwd_workspace(int64_t N, int K, int FP);
int han_score_param_bwd(const void *H, int table_dtype, const float *df1, const float *df2,
                        float *da1, float *da2, float *db1, float *db2, void *workspace,
                        size_t workspace_bytes, int64_t N, int K, int FP, void *stream);

/* ---- K3: semantic-level (meta-path) attention ------------------------------
 * utils/layers.py:152-159: v = tanh(M Womega + bomega); s = v . uomega;
 * beta = softmax over P PER NODE; Z = sum_p beta_p M_p.
 * M (N,P,D); Womega (D,A); bomega,uomega (A); Z (N,D); beta (N,P).
 * D and A: any multiples of 64 (zero-pad narrower ones: exact).  D in {64,128} with
 * A <= 256 run the tuned kernels, anything wider the run-time-width kernels
 * (models/gat.py:42-61 leaves the last layer's width and mp_att_size free).   */
int han_sem_attn_fwd(const float *M, const float *w_omega, const float *b_omega,
                     const float *u_omega, float *Z, float *beta, int64_t N, int P,
                     int D, int A, int flags, void *stream);

/* dZ (N,D) -> dM (N,P,D), dWomega (D,A), dbomega (A), duomega (A).
 * beta is the forward's output.                                            */
size_t han_sem_attn_bwd_workspace(int64_t N, int P, int D, int A);
int han_sem_attn_bwd(const float *M, const float *w_omega, const float *b_omega,
                     const float *u_omega, const float *beta, const float *dZ, float *dM,
                     float *dw_omega, float *db_omega, float *du_omega, void *workspace,
                     size_t workspace_bytes, int64_t N, int P, int D, int A, int flags, void *stream);

/* ---- K3 as published: one weight per meta-path (added under ABI 15: three new entry points, nothing existing
 * changed) ----
 * han.pdf sec. 4.2, eq. 7-9: s_ip = u . tanh(W^T M_ip + b); w_p = (1/N) sum_i s_ip; beta = softmax over P of w;
 * Z_i = sum_p beta_p M_ip.  The difference from utils/layers.py:156 (han_sem_attn_fwd): the softmax is taken ONCE, over
 * the node means of the scores, not per node -- beta is P floats shared by every node, and wmean (may be null) receives
 * the P means in double.  M (N,P,D); Womega (D,A); bomega, uomega (A); Z (N,D).
 * Shapes: D in {64, 128}, A in {64, 128, 192, 256}, 1 <= P <= 64, any N >= 1; anything else HAN_E_UNSUPPORTED before any
 * launch (zero-pad narrower D / A to a multiple of 64: exact).  HAN_E_BADARG: a null pointer other than wmean, a
 * workspace not 8-byte aligned, N < 0, P <= 0; HAN_E_WORKSPACE: workspace_bytes below
 * han_sem_attn_mean_workspace(N, P, D, A), which serves both entries.  N == 0 returns 0 with nothing launched.  Neither
 * entry allocates or synchronises; no value travels through the host; results are bit-identical from run to run.
 * `flags` is reserved (pass 0).                                                                                    */
size_t han_sem_attn_mean_workspace(int64_t N, int P, int D, int A);
int han_sem_attn_mean_fwd(const float *M, const float *w_omega, const float *b_omega, const float *u_omega,
                          float *Z, float *beta /* P floats */, double *wmean /* P doubles, may be null */,
                          void *workspace, size_t workspace_bytes, int64_t N, int P, int D, int A, int flags,
                          void *stream);

/* Backward of han_sem_attn_mean_fwd (han.pdf eq. 7-9; unlike utils/layers.py:156 every row of dM depends on every row of
 * dZ, through the P scalars d w_p): dZ (N,D) -> dM (N,P,D), dWomega (D,A), dbomega (A), duomega (A).
 *   dbeta_p = sum_i <dZ_i, M_ip>;  dw_p = beta_p (dbeta_p - sum_q beta_q dbeta_q);  ds_ip = dw_p / N;
 *   dpre_ip = ds_ip u (1 - v_ip^2);  dM_ip = beta_p dZ_i + W dpre_ip;  dW = sum M_ip (x) dpre_ip; db = sum dpre_ip;
 *   du = sum ds_ip v_ip.
 * beta (P floats) is the forward's output.  Shapes, return codes and workspace as for the forward.                  */
int han_sem_attn_mean_bwd(const float *M, const float *w_omega, const float *b_omega, const float *u_omega,
                          const float *beta /* P floats */, const float *dZ, float *dM, float *dw_omega,
                          float *db_omega, float *du_omega, void *workspace, size_t workspace_bytes, int64_t N, int P,
                          int D, int A, int flags, void *stream);

/* han_sem_attn_bwd with the row-local step of the K2 backward (han_node_attn_bwd_rows) of all P meta-paths in its
 * epilogue, for an M that is the K2 output itself: row (n, p) of M is the output row n of meta-path p's
 * han_node_attn_fwd, and nothing else consumes M.  dM is not written.  aggp, tsum, f1, lse, gs and df1 are HOST
 * arrays of P DEVICE pointers, each as han_node_attn_bwd_rows takes it (gs: fp32 rows of han_gs_row_bytes(8, 8,
 * HAN_DTYPE_F32) bytes); c (P,D) and dc (P,D) hold all meta-paths.  g, f1, lse, s and df1 are the bits the two
 * calls give; dc is the same sum in another order.
 * HAN_E_UNSUPPORTED, before any launch, unless D == 64, A in {64, 128}, P in {1, 2, 4}, N * P >= 65 536, K == 8,
 * FP == 8, table_dtype == HAN_DTYPE_F32, activation is HAN_ACT_ELU or HAN_ACT_IDENTITY and flags holds none of
 * HAN_FLAG_K3_EXACT_PIPE, HAN_FLAG_K3_PAIRS, HAN_FLAG_K3_G3_F32: the caller then runs the two calls.            */
size_t han_sem_attn_bwd_rows_workspace(int64_t N, int P, int D, int A);
int han_sem_attn_bwd_rows(const float *M, const float *w_omega, const float *b_omega, const float *u_omega,
                          const float *beta, const float *dZ, const float *const *aggp, const float *const *tsum,
                          const float *const *f1, const float *const *lse, const float *c, void *const *gs,
                          float *const *df1, float *dw_omega, float *db_omega, float *du_omega, float *dc,
                          void *workspace, size_t workspace_bytes, int64_t N, int P, int D, int A, int K, int FP,
                          int table_dtype, int activation, int flags, void *stream);

/* han_sem_attn_bwd_rows over a row list (added under ABI 15: a new entry point, nothing existing changed): `live` holds
 * n_live ascending node ids (device, int32, each < N, none twice), and only rows (live[t], p) take part.  M, dZ, beta and
 * the per-meta-path inputs are read at node live[t]; the [g | stats] row and df1 are written at node live[t] of the
 * full-size (N-row) tables; rows of nodes that are not listed are neither read nor written.  dw / db / du / dc are the
 * sums over the listed rows -- what the full entry gives when dZ is zero in every other row.  The grid and the
 * reduction follow n_live * P; n_live == 0 launches no kernel and writes zeros to dw / db / du / dc.  With
 * live = 0 .. N - 1 every output holds the bits of han_sem_attn_bwd_rows.
 * HAN_E_UNSUPPORTED by the rule of han_sem_attn_bwd_rows WITHOUT its lower bound on the row count: the kernel's loops
 * are correct for any count (the bound there only says from where the bf16 pipe is the form han_sem_attn_bwd runs), so
 * D == 64, A in {64, 128}, P in {1, 2, 4}, K == 8, FP == 8, fp32 tables, ELU or identity, none of the three K3 flags.
 * Workspace: han_sem_attn_bwd_rows_workspace(N, P, D, A).                                                          */
int han_sem_attn_bwd_rows_live(const float *M, const float *w_omega, const float *b_omega, const float *u_omega,
                               const float *beta, const float *dZ, const float *const *aggp, const float *const *tsum,
                               const float *const *f1, const float *const *lse, const float *c, void *const *gs,
                               float *const *df1, float *dw_omega, float *db_omega, float *du_omega, float *dc,
                               void *workspace, size_t workspace_bytes, const int32_t *live, int64_t n_live, int64_t N,
                               int P, int D, int A, int K, int FP, int table_dtype, int activation, int flags,
                               void *stream);

/* han_sem_attn_fwd over a row list (an addition under ABI 15): live (n_live) holds ascending int32 node ids, each below
 * N, none twice.  Rows (live[t], p) of M are read; Z and beta are written at node live[t] of the full-size arrays;
 * nothing else is read or written.  The kernel is the bf16-pipe wave kernel of han_sem_attn_fwd with a tile's 16 rows
 * taken from the list (16 / P nodes per tile), at any count: with live = 0 .. N - 1 and N * P >= 65 536 every output
 * holds the bits of han_sem_attn_fwd, and a listed row's bits do not depend on which other rows are listed.
 * D == 64, A in {64, 128}, P in {1, 2, 4}, not HAN_FLAG_K3_EXACT_PIPE; anything else HAN_E_UNSUPPORTED before any
 * launch (the caller then runs the full entry).  n_live == 0 launches nothing.                                    */
int han_sem_attn_fwd_live(const float *M, const float *w_omega, const float *b_omega, const float *u_omega, float *Z,
                          float *beta, const int32_t *live, int64_t n_live, int64_t N, int P, int D, int A, int flags,
                          void *stream);

/* ---- classifier + masked loss ----------------------------------------------
 * models/gat.py:65-72: logits = (1/HC) sum_h (Z Wc[h] + bc[h]);  Wc (HC,D,C).
 * models/base_gattn.py:41-48,61-69: per-row masked softmax-CE and accuracy
 * terms with row weight w_i = mask_i * inv_mask_mean / n_total:
 *   loss_acc[0] = sum_i w_i CE_i,  loss_acc[1] = sum_i w_i [argmax == label]
 * labels are class ids (int32, argmax of the one-hot rows); mask uint8.
 * If dZ != NULL also writes dlogits (N,C) = w_i (softmax - onehot) and
 * dZ = dlogits @ mean_h(Wc[h])^T, dWc (HC,D,C), dbc (HC,C).
 * D: any multiple of 64; C: any class count (D in {64,128} with C <= 64: the fused
 * single-launch kernels; otherwise head average -> row kernel -> Z^T dlogits over
 * the masked rows).                                                          */
size_t han_classifier_workspace(int64_t N, int D, int C, int HC);
int han_classifier_loss(const float *Z, const float *Wc, const float *bc,
                        const int32_t *labels, const uint8_t *mask, float row_weight,
                        float *logits, float *loss_acc, float *dZ, float *dWc, float *dbc,
                        void *workspace, size_t workspace_bytes, int64_t N, int D, int C,
                        int HC, void *stream);

/* han_classifier_loss over a row list (an addition under ABI 15): live (n_live) holds ascending int32 node ids, each
 * below N, none twice.  Only the listed rows of Z, labels and mask are read; logits rows, and dZ rows when dZ != NULL,
 * are written at the listed rows of the full-size arrays and nowhere else, with the bits han_classifier_loss gives
 * them (the same kernel text and per-row arithmetic); loss_acc, dWc and dbc are the sums over the listed rows, mask
 * still applied per row.  For callers whose Z holds no defined values outside the list (the full entry multiplies the
 * loss of an unmasked row by a zero weight, and 0 x NaN is NaN).  The fused shapes only: D in {64, 128}, C <= 64,
 * anything else HAN_E_UNSUPPORTED before any launch.  n_live == 0 launches no kernel and writes zeros to loss_acc (and
 * dWc, dbc).  Workspace: han_classifier_workspace(N, D, C, HC).                                                      */
int han_classifier_loss_live(const float *Z, const float *Wc, const float *bc, const int32_t *labels,
                             const uint8_t *mask, float row_weight, float *logits, float *loss_acc, float *dZ,
                             float *dWc, float *dbc, void *workspace, size_t workspace_bytes, const int32_t *live,
                             int64_t n_live, int64_t N, int D, int C, int HC, void *stream);

/* The multi-label objective (added under ABI 15: two new entry points, nothing existing changed): models/base_gattn.py:50-59,71-94 -- masked sigmoid cross-entropy and micro-F1 --
 * on the logits of han_classifier_loss.  label_bits (N, ceil(C/64)) uint64: class c of a row is bit c % 64 of word
 * c / 64 (8 B per row up to 64 classes).  Per row i with logits x, labels y in {0,1}^C, w_i = mask_i ? row_weight : 0:
 *   loss      = sum_i w_i (1/C) sum_c [ max(x_c, 0) - x_c y_c + log(1 + exp(-|x_c|)) ]     (TF's stable form, then
 *               reduce_mean(axis=1), then the mask weighting of :56-59)
 *   dlogits   = (w_i / C) (sigma(x_c) - y_c), sigma from the same e = exp(-|x_c|): 1 / (1 + e) for x_c >= 0, e / (1 + e)
 *               otherwise -- no overflow for any finite logit; rows outside the mask get exact zeros
 *   predicted = (x_c > 0): round(sigmoid(x)) with half-to-even in exact arithmetic (sigma(0) = 1/2 rounds to 0); an fp32
 *               sigmoid followed by round maps tiny positive logits to 0 -- a difference inside the logits' own
 *               rounding error
 *   tp, fp, fn  over the rows with mask_i != 0 and all classes, exact integers (accumulated as integers throughout);
 *               micro_f1 = 2 tp / (2 tp + fp + fn) in double (algebraically :90-92), NaN when tp == 0 (the reference's 0/0)
 * Writes logits (N,C), loss_acc[0] = loss, loss_acc[1] = micro_f1 (float), counts[3] = {tp, fp, fn} (int64), all on the
 * device; with dZ != NULL also dZ (N,D), dWc (HC,D,C), dbc (HC,C).  Cross-block sums are slabs reduced in a fixed
 * order: bitwise reproducible, no atomics.  D in {64,128} with C <= 64: fused single-launch kernels (16 lanes per row
 * up to 16 classes, class-per-lane beyond); any other multiple of 64 / class count: head average -> row kernel ->
 * Z^T dlogits over the masked rows.
 * live (NULL: every row): n_live ascending int32 node ids, each below N, none twice -- the contract of
 * han_classifier_loss_live: only the listed rows of Z, label_bits and mask are read, only the listed rows of logits
 * and dZ are written, with the bits of the full call; the sums run over the list.  The fused shapes only.  n_live == 0
 * launches no kernel and writes zeros (loss, counts, dWc, dbc) and NaN for micro_f1.
 * HAN_E_BADARG: a null pointer, a negative size, n_live > N, dZ without dWc / dbc; HAN_E_UNSUPPORTED, before any launch:
 * D % 64 != 0, or `live` outside the fused shapes; HAN_E_WORKSPACE: workspace_bytes below
 * han_classifier_multilabel_workspace(N, D, C, HC).                                                               */
size_t han_classifier_multilabel_workspace(int64_t N, int D, int C, int HC);
int han_classifier_multilabel(const float *Z, const float *Wc, const float *bc, const uint64_t *label_bits,
                              const uint8_t *mask, float row_weight, float *logits, float *loss_acc, int64_t *counts,
                              float *dZ, float *dWc, float *dbc, void *workspace, size_t workspace_bytes,
                              const int32_t *live, int64_t n_live, int64_t N, int D, int C, int HC, void *stream);

/* The backward of the logits alone (HeteGAT_multi.inference returns logits; a caller
 * that forms its own loss hands back dlogits (N,C)):  dZ = dlogits @ mean_h(Wc[h])^T,
 * dWc[h] = Z^T dlogits / HC, dbc[h] = sum_n dlogits / HC.  Same shape rules.      */
size_t han_classifier_bwd_workspace(int64_t N, int D, int C, int HC);
int han_classifier_bwd(const float *Z, const float *Wc, const float *bc, const float *dlogits,
                       float *dZ, float *dWc, float *dbc, void *workspace,
                       size_t workspace_bytes, int64_t N, int D, int C, int HC, void *stream);

/* ---- optimiser --------------------------------------------------------------
 * models/base_gattn.py:12-24: L2 on every trainable + tf.train.AdamOptimizer:
 *   g' = g + l2_coef * p;  m,v EMAs;  p -= lr_t * m / (sqrt(v) + eps)
 * with lr_t = lr * sqrt(1-beta2^t)/(1-beta1^t) computed by the caller when step_dev is
 * NULL; when step_dev (device int64, the step count t >= 1) is given, `lr_t` is the BASE
 * rate lr and the bias correction is computed on the device (captured hipGraphs).  */
int han_adam_step(float *param, const float *grad, float *m, float *v, int64_t n,
                  float lr_t, float beta1, float beta2, float eps, float l2_coef,
                  const int64_t *step_dev, void *stream);

/* sum over all parameters of p^2/2 (the L2 term of the reported loss).
 * out[0] written.  workspace: 4096 floats.                                 */
int han_l2_half_sumsq(const float *param, int64_t n, float *out, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ---- input format: additive bias matrix -> CSR ----------------------------
 * utils/process.py:14-25 produces bias (N,N) in {0,-1e9}; an edge is an entry
 * > -1e8.  Two launches: counts per row (then the caller scans) and fill.  */
int han_bias_row_counts(const float *bias, int64_t N, int64_t ld, int64_t *counts,
                        void *stream);
int han_bias_fill_csr(const float *bias, int64_t N, int64_t ld, const int64_t *rowptr,
                      int32_t *colidx, void *stream);

/* ---- K0: meta-path graphs from typed relations ------------------------------
 * The boolean product C = A B of two CSR graphs: entry (i, j) of C is present iff some l has (i, l) in A and (l, j)
 * in B.  A meta-path graph (APA, APCPA, ...) is such a product along its typed relations (paper-author, paper-
 * conference, ... edge lists; han_amd/metapath.py); the reference reads them preprocessed (ex_acm3025.py:57-87).
 * A (n_rows x n_mid): a_rowptr (n_rows+1) int64, a_colidx int32; B (n_mid x n_cols) likewise.  Their columns need not
 * be sorted or unique; a colidx may be NULL when its graph has no entries (c_colidx likewise).  Every row of C holds
 * strictly increasing columns.  flags: HAN_SPGEMM_DIAG also sets (i, i) (square products, n_rows == n_cols).
 * Three launches:
 *   han_spgemm_row_bounds: ub (n_rows) int64, ub_i = sum over l in A_i of deg_B(l), + 1 with HAN_SPGEMM_DIAG -- the
 *       candidates of row i, an upper bound of its entries;
 *   the caller bins the rows by ub: `rows` (n_rows int32) lists every row once, the rows with ub > short_max first,
 *       and the device word *n_long holds their number (the binning needs no copy to the host);
 *   han_spgemm_count: counts (n_rows) int64, the entries of every row; the caller scans them into c_rowptr (n_rows+1)
 *       and allocates c_colidx (c_rowptr[n_rows] entries);
 *   han_spgemm_fill: c_colidx.
 * Rows with ub <= short_max (<= HAN_SPGEMM_MAX_SHORT) are sorted in LDS, a wave each; the others set bits in an LDS bit
 * map of tile_cols columns (a multiple of 32, <= HAN_SPGEMM_MAX_TILE), a workgroup each, and read their candidates
 * once per tile of [0, n_cols).  count and fill take the same rows, n_long, short_max, tile_cols and flags.       */
#define HAN_SPGEMM_DIAG 1
#define HAN_SPGEMM_MAX_SHORT 4096
#define HAN_SPGEMM_MAX_TILE (1 << 19)
int han_spgemm_row_bounds(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                          int64_t n_rows, int64_t n_mid, int flags, int64_t *ub, void *stream);
int han_spgemm_count(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                     const int32_t *b_colidx, int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t *rows,
                     const int64_t *n_long, int64_t short_max, int64_t tile_cols, int flags, int64_t *counts,
                     void *stream);
int han_spgemm_fill(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *b_rowptr,
                    const int32_t *b_colidx, int64_t n_rows, int64_t n_mid, int64_t n_cols, const int32_t *rows,
                    const int64_t *n_long, int64_t short_max, int64_t tile_cols, int flags,
                    const int64_t *c_rowptr, int32_t *c_colidx, void *stream);

/* ---- K0: weighted meta-path graphs (ABI 8) ----------------------------------
 * han_spgemm_values: the counted product over the structure han_spgemm_fill wrote.  c_vals (nnz_c) int64,
 *   c_ij = sum over l of a_il b_lj: one term per pair of stored entries (i, l) of A and (l, j) of B, so a repeated
 *   stored entry counts once per repetition.  a_vals / b_vals: int64, one per stored entry of A / B, or NULL = every
 *   stored entry is 1.  Sums are int64 and integer adds only (wrap-around beyond 2^63 is not detected), so the result
 *   does not depend on scheduling.  An entry of C that no product reaches -- the (i, i) HAN_SPGEMM_DIAG added -- is 0.
 *   Takes the rows, n_long, short_max, tile_cols and flags of the count and fill calls that made c_rowptr / c_colidx
 *   (nnz_c = c_rowptr[n_rows]); c_vals needs no initialisation (it is cleared on the stream).  Not checked: that C is
 *   that structure.  With another one nothing is written out of bounds, but a product whose column is not in its row
 *   of C is dropped and a short-bin row of C longer than short_max (rounded up to a power of two) keeps 0.
 *   a_colidx / b_colidx / c_colidx / c_vals may be NULL when their graph has no entries.
 * han_csr_pathsim: values (nnz) fp32 of a square counted graph (n x n, strictly increasing columns in every row --
 *   not checked), w_ij = 2 c_ij / (c_ii + c_jj) evaluated in double and rounded once to fp32; w_ii = 1 exactly
 *   (also when c_ii = 0); c_jj = 0 when row j does not store (j, j).  diag: n int64 of caller scratch (the c_ii, found
 *   by a binary search per row).  An off-diagonal entry with c_ii + c_jj = 0 gives what IEEE division gives.
 * han_csr_row_topk_count / _fill: per row the k (>= 1) entries of largest value that are not (i, i), and with
 *   keep_diag != 0 also (i, i); ties go to the smaller column; the output keeps the row's column order, values travel
 *   with their columns; a row with at most k entries off the diagonal is kept whole.  Rows must hold strictly
 *   increasing columns (not checked; otherwise which of several equal values stay is unspecified, nothing is written
 *   out of bounds).  Values are ordered by the monotone map of fp32 bits to unsigned: a total order on the finite
 *   values and the infinities (-0 below +0); where NaN sorts is unspecified.  count: counts (n_rows) int64; the
 *   caller scans them into out_rowptr (n_rows+1) and allocates out_colidx / out_values; fill writes both.  count and
 *   fill take the same k and keep_diag.
 * All four run on `stream`, allocate nothing and never synchronise.                                                  */
int han_spgemm_values(const int64_t *a_rowptr, const int32_t *a_colidx, const int64_t *a_vals,
                      const int64_t *b_rowptr, const int32_t *b_colidx, const int64_t *b_vals, int64_t n_rows,
                      int64_t n_mid, int64_t n_cols, const int32_t *rows, const int64_t *n_long, int64_t short_max,
                      int64_t tile_cols, int flags, const int64_t *c_rowptr, const int32_t *c_colidx, int64_t nnz_c,
                      int64_t *c_vals, void *stream);
int han_csr_pathsim(const int64_t *rowptr, const int32_t *colidx, const int64_t *counts, int64_t n, int64_t *diag,
                    float *values, void *stream);
int han_csr_row_topk_count(const int64_t *rowptr, const int32_t *colidx, int64_t n_rows, int64_t k, int keep_diag,
                           int64_t *counts, void *stream);
int han_csr_row_topk_fill(const int64_t *rowptr, const int32_t *colidx, const float *values, int64_t n_rows,
                          int64_t k, int keep_diag, const int64_t *out_rowptr, int32_t *out_colidx,
                          float *out_values, void *stream);

/* ---- K0: sampled meta-path neighbours (ABI 11) ------------------------------
 * Meta-path-guided random walks instead of the product: from every start node `walks` walks along the chain of
 * n_hops graphs (1 <= n_hops <= HAN_WALK_MAX_HOPS), the end points counted per start row, and the `fanout` most
 * visited kept -- a CSR row of at most fanout + 1 entries whatever the product would hold.
 * hop h (rows = current nodes, columns = next nodes): hop_rowptr[h] (hop_rows[h] + 1) int64, hop_colidx[h] int32 --
 * HOST arrays of n_hops DEVICE pointers (read during the call, not kept); hop_rows: host array of the row counts;
 * a hop_colidx[h] may be NULL when its graph has no entries.  Columns need not be sorted or unique: a repeated
 * stored entry is as many parallel edges.  n_cols: the columns of the last hop.
 * Start node i = row_base + r, r in [0, n_rows) (row_base + n_rows <= hop_rows[0]); walk w in [0, walks),
 * 1 <= walks <= HAN_WALK_MAX_WALKS: cur = i, and for h = 0 .. n_hops - 1
 *     deg = the stored entries of row cur of hop h; deg == 0: the walk dies and counts nowhere;
 *     (x, y) = han_rand64(seed, stream 3, a = (uint32) i, b = w * ((n_hops + 1) / 2) + (h >> 1));
 *     r = (h & 1) ? y : x;   e = ((uint64) r * deg) >> 32;   cur = colidx[rowptr[cur] + e].
 * The draw depends on (seed, i, w, h) alone: not on the launch shape, the row range or the lane that walks.  The
 * multiply-high map picks an entry with probability within 2^-32 of 1 / deg (relative bias below deg / 2^32).  Not
 * checked: deg < 2^32 (the caller's; the low 32 bits are used, nothing is read out of bounds).  A column outside the
 * next hop's rows (or outside [0, n_cols) at the end) ends the walk like a dead end.
 * Row r of the result: c_j = walks of i that end in j.  diag == 0: the 1 <= fanout <= walks columns of largest c_j,
 * ties to the smaller column.  diag != 0 (n_cols == hop_rows[0]): (i, i) is always stored with its own visit count,
 * possibly 0, and does not compete: the fanout best of the OTHER columns are kept beside it.  Columns strictly
 * ascending; a row whose walks all died is empty (diag: (i, i) alone, count 0).
 *   han_metapath_walk_count: counts (n_rows) int64, the entries of every row; the caller scans them into c_rowptr
 *       (n_rows + 1, local rows) and allocates c_colidx / c_visits (c_rowptr[n_rows] entries each);
 *   han_metapath_walk_fill: the same walks again (same arguments), c_colidx int32 and c_visits int32 = c_j.
 * A wave per start row; end points, their sort, the run lengths and a histogram of the counts stay in LDS: nothing of
 * n_rows x walks words exists in device memory, integer LDS adds only, so the result is bitwise reproducible.
 * Both run on `stream`, allocate nothing and never synchronise.  No seed_dev variant: building a graph is never
 * captured into a hipGraph.                                                                                         */
#define HAN_WALK_MAX_HOPS 8
#define HAN_WALK_MAX_WALKS 4096
int han_metapath_walk_count(const int64_t *const *hop_rowptr, const int32_t *const *hop_colidx,
                            const int64_t *hop_rows, int n_hops, int64_t n_cols, int64_t row_base, int64_t n_rows,
                            int walks, int fanout, uint64_t seed, int diag, int64_t *counts, void *stream);
int han_metapath_walk_fill(const int64_t *const *hop_rowptr, const int32_t *const *hop_colidx,
                           const int64_t *hop_rows, int n_hops, int64_t n_cols, int64_t row_base, int64_t n_rows,
                           int walks, int fanout, uint64_t seed, int diag, const int64_t *c_rowptr,
                           int32_t *c_colidx, int32_t *c_visits, void *stream);

/* ---- K0: ego blocks (ABI 14) --------------------------------------------------
 * The neighbourhood of a batch of seed nodes cut out of square graphs over the same n nodes (han_amd/minibatch.py):
 * a breadth-first level per node, then the block's rows with their columns renumbered.  Graphs are CSR as everywhere
 * (rowptr int64, colidx int32; columns need not be sorted or unique), a colidx / values pointer may be NULL when the
 * graph has no entries.  Integer loads and stores only: results are bitwise the same from run to run.
 * The chunk table (split_deg, n_chunks, long_rows, chunk_long, chunk_start, chunk_end) is han_row_split_t's, of the
 * INPUT graph: rows with more than split_deg entries are left to their chunks, a wave each; n_chunks == 0 (pointers
 * may be NULL): every row is walked by one wave, whatever its length.  Not checked: that the table describes rowptr.
 * han_ego_expand: one hop over one graph.  level (n) int32, -1 = unvisited: every row i with level[i] == h writes
 *   h + 1 into level[c] of each of its columns c that is still unvisited (columns outside [0, n) are skipped).  All
 *   writers of a word write the same value, a visited word never changes, so the outcome does not depend on timing.
 *   The caller sets level = 0 on the seeds and issues the graphs of hop h one after another on the stream, then
 *   hop h + 1: level becomes the breadth-first distance over the union of the graphs.
 * han_ego_count: counts (n_out) int64, the entries of every output row r with source row v = rows[r] (int64): the
 *   stored entries of row v where the row is kept, 1 where it is not (the rim), 0 for v outside [0, n_in).  A row is
 *   kept iff 0 <= level[v] < hops; level == NULL keeps every row (hops is then ignored).
 * han_ego_fill: out_rowptr (n_out + 1) int64 = the scanned counts.  A kept row is row v as stored -- order, repeated
 *   entries and values as they are --, its columns c replaced by local[c] (int32 over n_cols; -1 for c outside
 *   [0, n_cols)), or unchanged with local == NULL; a rim row holds (r, r) alone.  out_values (or NULL): the values,
 *   1.0 on the rim and wherever values == NULL.  With a chunk table local must be given and invert rows on the kept
 *   rows (local[rows[r]] == r): chunk c of row v lands at its offset inside row local[v].
 * A NULL rowptr / level / rows / counts / out_rowptr / out_colidx, a negative size, hops < 1 beside a level array, a
 * chunk table with a NULL array or split_deg < 1, and n (expand) or n_cols / n_out (fill) beyond INT32_MAX are
 * HAN_E_BADARG, decided before any launch; n == 0 / n_out == 0 return 0 and launch nothing.  All three run on `stream`,
 * allocate nothing and never synchronise.                                                                            */
int han_ego_expand(const int64_t *rowptr, const int32_t *colidx, int64_t n, int h, int64_t split_deg,
                   int64_t n_chunks, const int64_t *long_rows, const int32_t *chunk_long, const int64_t *chunk_start,
                   const int64_t *chunk_end, int32_t *level, void *stream);
int han_ego_count(const int64_t *rowptr, const int64_t *rows, const int32_t *level, int hops, int64_t n_in,
                  int64_t n_out, int64_t *counts, void *stream);
int han_ego_fill(const int64_t *rowptr, const int32_t *colidx, const float *values, const int64_t *rows,
                 const int32_t *level, int hops, const int32_t *local, int64_t n_in, int64_t n_cols, int64_t n_out,
                 int64_t split_deg, int64_t n_chunks, const int64_t *long_rows, const int32_t *chunk_long,
                 const int64_t *chunk_start, const int64_t *chunk_end, const int64_t *out_rowptr, int32_t *out_colidx,
                 float *out_values, void *stream);

/* ---- K0: sampled ego blocks (added under ABI 15: new entry points only, nothing existing changed) ----
 * The same block with a random fan-out: a row keeps its self entries (column == row) and at most `fanout` of its
 * other entries.  The key of the entry at stored position k of row v of graph `graph` is the first word x of
 * han_rand64(seed, stream 4 * (graph + 1), a = v, b = k) (csrc/han_common.h; tests/rng_ref.py).  A row with d <= fanout
 * entries off the diagonal keeps them all; otherwise it keeps the `fanout` entries of smallest (x, k) -- equal keys go
 * to the smaller stored position.  Kept entries stay in stored order with their values (no reweighting), repeated
 * entries are entries of their own.  Rows of up to 2^31 - 1 entries.  Integer stores only, all writers of a word write
 * the same value: bitwise the same from run to run.
 * The long-row list (split_deg, n_long, long_rows) is han_row_split_t's of the INPUT graph: the rows with more than
 * split_deg entries, a 256-thread workgroup each; every other row is served by a wave.  n_long == 0 (pointer may be
 * NULL): every row by a wave.  Not checked: that the list describes rowptr.
 * han_ego_sample_expand: one hop over one graph, as han_ego_expand, over the SELECTED entries: every row i with
 *   level[i] == h is decided -- thr[i] (the fanout-th smallest key), need[i] (entries equal to thr still kept, in
 *   stored order; -1: the whole row is kept) and kept[i] (entries of the sampled row), arrays of n elements that are
 *   written and read for expanded rows only -- and writes h + 1 into the level of the unvisited columns of its
 *   selected entries.  fanout may differ from hop to hop; a row is expanded once, at the hop of its level.
 * han_ego_sample_count: counts[r] = kept[rows[r]] where 0 <= level[rows[r]] < hops, 1 on the rim, 0 for a row outside
 *   [0, n_in).
 * han_ego_sample_fill: the rows counted above from the stored decision and the keys drawn again; columns through
 *   local (int32 over n_in), a rim row holds (r, r) alone; out_values (or NULL): the values, 1.0 on the rim and where
 *   values == NULL.  local must invert rows on the kept rows.  No store lands at or beyond out_rowptr[r + 1].
 * HAN_E_BADARG, before any launch: a NULL rowptr / level / thr / need / kept / local / rows / counts / out_rowptr /
 * out_colidx, a negative size, n / n_in / n_out beyond INT32_MAX, fanout < 1, hops < 1, h < 0, graph < 0, a long-row
 * list without its array or with split_deg < 1.  n == 0, a NULL colidx (no entries: the caller zeroes kept) and
 * n_out == 0 return 0 and launch nothing.                                                                          */
int han_ego_sample_expand(const int64_t *rowptr, const int32_t *colidx, int64_t n, int h, int fanout, uint64_t seed,
                          int graph, int64_t split_deg, int64_t n_long, const int64_t *long_rows, int32_t *level,
                          uint32_t *thr, int32_t *need, int64_t *kept, void *stream);
int han_ego_sample_count(const int64_t *rows, const int32_t *level, int hops, const int64_t *kept, int64_t n_in,
                         int64_t n_out, int64_t *counts, void *stream);
int han_ego_sample_fill(const int64_t *rowptr, const int32_t *colidx, const float *values, const int64_t *rows,
                        const int32_t *level, int hops, const int32_t *local, int64_t n_in, int64_t n_out,
                        uint64_t seed, int graph, int64_t split_deg, int64_t n_long, const int64_t *long_rows,
                        const uint32_t *thr, const int32_t *need, const int64_t *out_rowptr, int32_t *out_colidx,
                        float *out_values, void *stream);

/* ---- evaluation of the embeddings (ABI 9) -----------------------------------
 * The reference scores final_embed on the host with scikit-learn: my_KNN (jhyexp.py:20-51) and my_Kmeans
 * (jhyexp.py:54-86), called at ex_acm3025.py:288-289.  These entry points are the device side of both.
 * Embeddings are fp32, row-major, with a leading dimension in elements (>= D); 1 <= D <= 512.  Squared distances
 * have the form d2 = |q|^2 + |t|^2 - 2 q.t with the q.t term on the exact-fp32 matrix pipe; no pair matrix is ever
 * stored.  Every result is bitwise the same from run to run (no floating-point atomics; cross-block sums are
 * slabs added in a fixed order).
 *
 * han_knn_topk: KNeighborsClassifier(n_neighbors=k).fit(x[:split]).kneighbors(x[split:]), jhyexp.py:38-41.
 *   Q (Nq, D) queries, T (Nt, D) train rows, 1 <= k <= 16.  idx (Nq, k) int32 / d2 (Nq, k) fp32: per query the k
 *   smallest pairs under the total order (d2, train index), ascending -- equal distances go to the smaller index.
 *   k > Nt: HAN_E_BADARG; k > 16, D > 512 or Nt >= 2^31: HAN_E_UNSUPPORTED; Nq == 0 returns 0.  workspace:
 *   han_knn_topk_workspace() bytes (the row norms; with few queries the train set is split over workgroups and the
 *   partial lists are merged from it).
 * han_knn_vote: KNeighborsClassifier(weights="uniform").predict, jhyexp.py:41: pred[q] = the most frequent of
 *   labels_train[idx[q, :]], ties to the smallest class id (k^2 compares in registers, no table sized by the class
 *   count).  An idx entry outside [0, Nt) is skipped.
 * han_contingency: the count table behind f1_score (jhyexp.py:43-44) and normalized_mutual_info_score /
 *   adjusted_rand_score (jhyexp.py:70-71): table[x * Cb + y] = number of i with a[i] == x and b[i] == y, int64,
 *   Ca * Cb <= 4096.  `table` holds Ca * Cb + 1 words and is cleared on the stream; the LAST word is a flag: non-zero
 *   when some label was outside [0, Ca) / [0, Cb) (such elements are not counted) -- the caller reads it with the
 *   table and treats it as HAN_E_BADARG.
 * han_kmeans_step: one Lloyd iteration of KMeans(n_clusters=k).fit, jhyexp.py:62-68.  X (N, D), C (k, D) contiguous,
 *   1 <= k <= 64; prev (N) int32 or NULL.  labels (N) int32: the nearest centre, ties to the smaller centre index;
 *   d2 (N) fp32 or NULL: that distance; counts (k) int64; new_centres (k, D) fp32: the mean of each cluster's rows
 *   (summed in double in a fixed order) -- a cluster without rows keeps its centre and has count 0 (scikit-learn
 *   relocates such a centre); *inertia (double): the sum of the fp32 d2, added in double in a fixed order;
 *   *changed (int64): rows whose label differs from prev (N when prev is NULL).  counts / changed are cleared on
 *   the stream.  workspace: han_kmeans_step_workspace() bytes.                                              */
size_t han_knn_topk_workspace(int64_t Nq, int64_t Nt, int D, int k);
int han_knn_topk(const float *Q, int64_t ldq, const float *T, int64_t ldt, int32_t *idx, float *d2,
                 void *workspace, size_t workspace_bytes, int64_t Nq, int64_t Nt, int D, int k, void *stream);
int han_knn_vote(const int32_t *idx, const int32_t *labels_train, int32_t *pred, int64_t Nq, int k, int64_t Nt,
                 void *stream);
int han_contingency(const int32_t *a, const int32_t *b, int64_t n, int Ca, int Cb, int64_t *table, void *stream);
size_t han_kmeans_step_workspace(int64_t N, int D, int k);
int han_kmeans_step(const float *X, int64_t ldx, const float *C, const int32_t *prev, int32_t *labels, float *d2,
                    int64_t *counts, float *new_centres, double *inertia, int64_t *changed, void *workspace,
                    size_t workspace_bytes, int64_t N, int D, int k, void *stream);

/* ---- silhouette of a clustering of the embeddings (ABI 12) ------------------
 * The second copy of the reference's clustering evaluation (data/exp.py:25-62) also reports
 * silhouette_score(x, estimator.labels_, metric='euclidean') of every k-means fit (data/exp.py:46-49).  This is
 * scikit-learn's silhouette_samples on the device, O(N^2 D) on the exact-fp32 matrix pipe with the tiles of
 * han_knn_topk; distances are sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j)), no pair matrix is stored, and every result
 * is bitwise the same from run to run (no floating-point atomics; sums that cross a tile are carried in double and
 * added in a fixed order).
 *
 * X (N, D) fp32 with leading dimension ldx >= D, 1 <= D <= 512, N < 2^31.  The rows are GROUPED BY CLUSTER: rows
 * [seg_ptr[c], seg_ptr[c + 1]) are cluster c, seg_ptr (k + 1) int64 on the device, seg_ptr[0] = 0, seg_ptr[k] = N,
 * 2 <= k <= 64; a cluster may be empty.  A seg_ptr that is not such a sequence gives meaningless numbers (reads stay
 * inside X).  With n_c the size of cluster c, L the cluster of row i and S(i, c) the sum of |x_i - x_j| over the rows
 * j of c (the pair j = i contributes exactly 0, by its index):
 *   a[i] = S(i, L) / (n_L - 1), 0 when n_L = 1;   b[i] = min over c != L with n_c > 0 of S(i, c) / n_c (0 when there
 *   is no such cluster);   s[i] = (b - a) / max(a, b), and 0 when n_L = 1, when max(a, b) = 0 or when no other
 *   cluster has rows;   *sum (double, on the device) = the sum of the fp32 s[i], added in double in a fixed order.
 * a, b, s are (N) fp32 and may each be NULL.  N == 0 returns 0 with *sum = 0.  k < 2, ldx < D, a NULL X / seg_ptr /
 * sum / workspace: HAN_E_BADARG; k > 64, D > 512 or N >= 2^31: HAN_E_UNSUPPORTED.  workspace:
 * han_silhouette_workspace() bytes (row norms, a and b in double, the partial sums; with few row tiles the column
 * range is split over workgroups and the per-(row, cluster) partial sums are merged from it).                */
size_t han_silhouette_workspace(int64_t N, int D, int k);
int han_silhouette(const float *X, int64_t ldx, const int64_t *seg_ptr, int64_t N, int D, int k, float *a, float *b,
                   float *s, double *sum, void *workspace, size_t workspace_bytes, void *stream);

/* ---- t-SNE of the embeddings (ABI 13) ---------------------------------------
 * Both evaluation modules of the reference import sklearn.manifold (jhyexp.py:16, data/exp.py:20) for the
 * two-dimensional t-SNE picture of final_embed.  These entry points are scikit-learn's TSNE(n_components=2,
 * method="exact") on the device: _utils._binary_search_perplexity and _joint_probabilities (han_tsne_calibrate),
 * _kl_divergence with one degree of freedom and one iteration of _gradient_descent (han_tsne_step).  Pair distances are
 * d2 = max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) on the exact-fp32 matrix pipe with the tiles of han_knn_topk, the pair
 * j = i is excluded by its index, and NO N x N array is stored at any N: a step forms p_ij again from three floats per
 * row.  Every result is bitwise the same from run to run (no floating-point atomics; a lane adds the pairs of a tile in
 * fp32, sums that cross a tile are carried in double and added in a fixed order).
 *
 * X (N, D) fp32 with leading dimension ldx >= D, 1 <= D <= 512, N < 2^31.
 * han_tsne_calibrate: per row i the beta_i with entropy H(P_i) = log(perplexity).  Distances are shifted by the row
 *   minimum m_i = min over j != i of d2_ij (the one departure from scikit-learn: the same P, no underflow of the sum):
 *   Z_i = sum_j exp(-beta_i (d2_ij - m_i)),  E_i = sum_j (d2_ij - m_i) exp(..),  H = log Z_i + beta_i E_i / Z_i.
 *   restart != 0 finds dmin (N) = m and starts the bisection (beta = 1, no bounds); then `steps` bisection passes run
 *   back to back on the stream -- all rows together, one pass over all pairs each --: double or halve while a bound is
 *   infinite, else move to the midpoint; a row with |H - log perplexity| <= tol is closed and keeps its beta.
 *   state (3, N) double: the next beta (NEGATIVE: minus the beta of a closed row), the lower and the upper bound; beta
 *   is clamped to the finite fp32 range when a pass evaluates it.  beta (N) / zsum (N) fp32 always hold the last
 *   EVALUATED beta and its Z (what scikit-learn's P is built from when a row never closes); *open_rows (int64, on the
 *   device) the rows not closed after the last pass; steps == 0 leaves beta, zsum and *open_rows as they are (after a
 *   restart alone nothing has been evaluated yet).  perplexity must be finite, >= 1 and < N, tol >= 0.
 * han_tsne_step: one iteration.  c_ij = exp(-beta_i (d2_ij - m_i)) / Z_i,  p_ij = max((c_ij + c_ji) / (2 N), 2^-52),
 *   dy = y_i - y_j,  w = 1 / (1 + |dy|^2),  e = exaggeration:
 *     A_i = sum_j e p_ij w dy,  R_i = sum_j w^2 dy,  W_i = sum_j w,  Z_q = sum_i W_i,  grad_i = 4 (A_i - R_i / Z_q),
 *     KL = sum_ij e p_ij (log(e p_ij) - log w + log Z_q)        (scikit-learn's floor on q is not reproduced).
 *   Then, per element of (N, 2), every product and sum rounded on its own in fp32:
 *     gains = max(update * grad < 0 ? gains + 0.2 : gains * 0.8, min_gain);
 *     update = momentum * update - lr * (gains * grad);   Y += update.
 *   Y, update, gains (N, 2) fp32 in/out; grad (N, 2) fp32 or NULL: the gradient BEFORE the gains are applied.
 *   stats (3) double on the device: [0] Z_q, [1] the sum of (gains * grad)^2 (the squared norm scikit-learn compares
 *   with min_grad_norm), [2] KL when want_kl != 0, untouched otherwise; want_kl and grad change no other output bit.
 * N <= 1 returns 0 and launches nothing.  A NULL pointer (but grad), ldx < D, D < 1, a bad perplexity / tol /
 * exaggeration: HAN_E_BADARG; D > 512 or N >= 2^31: HAN_E_UNSUPPORTED; all decided before anything touches the
 * device.  workspace: han_tsne_workspace() bytes for both (row norms, the per-split slabs, the partial sums); 0 for an
 * unsupported shape.  Both run on `stream` and never synchronise.                                                   */
size_t han_tsne_workspace(int64_t N, int D);
int han_tsne_calibrate(const float *X, int64_t ldx, int64_t N, int D, float perplexity, float tol, int steps,
                       int restart, float *beta, float *dmin, float *zsum, double *state, int64_t *open_rows,
                       void *workspace, size_t workspace_bytes, void *stream);
int han_tsne_step(const float *X, int64_t ldx, const float *beta, const float *dmin, const float *zsum, float *Y,
                  float *update, float *gains, float *grad, double *stats, int64_t N, int D, float exaggeration,
                  float momentum, float lr, float min_gain, int want_kl, void *workspace, size_t workspace_bytes,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HAN_HIP_H */
