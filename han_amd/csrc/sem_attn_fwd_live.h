// han_sem_attn_fwd_live: the bf16-pipe wave kernel of the K3 forward over a row list (N = n_live); the body, and what
// the list changes in it, is sem_attn_fwd_b6_body.h.  Included by sem_attn.hip behind the full kernel.
// the id ring of the row-list form: per wave two slots of 16 node ids, behind Womega
constexpr int kFwdRingBytes = 4 * 2 * 16 * (int)sizeof(int);
template <int CA, int P>
__global__ __launch_bounds__(256) void sem_attn_fwd_wave_b6_live_kernel(const float *__restrict__ M, const float *Wg,
                                                                        const float *bw, const float *uw, float *Z,
                                                                        float *beta, int64_t N,
                                                                        const int32_t *__restrict__ live)
#define K3_FWD_LIVE 1
#include "sem_attn_fwd_b6_body.h"
#undef K3_FWD_LIVE
