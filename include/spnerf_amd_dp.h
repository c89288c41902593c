/* Data-parallel training-step exports of libspnerf_amd.so (gfx950): what a rank of an N-rank
 * ray-batch data-parallel run needs at the start and the end of a captured training step, beside
 * include/spnerf_amd_train.h.  A separate header so that the older ABIs stay as they are; the
 * conventions are theirs: every function returns SPNERF_OK or a negative SPNERF_E_* code with the
 * text in spnerf_last_error, pointers are device pointers unless noted, `stream` is a hipStream_t,
 * and no call synchronises with the host, allocates, or uses atomics on global memory — every call
 * can be captured in a HIP graph.
 *
 * Every rank uploads the SAME epoch plan (spnerf_amd_train.h: plan_rows, perm, state — built from
 * the same seed, no collective) whose B is the GLOBAL batch; rank r of `world` trains rows
 * [r b, (r + 1) b) of each global batch, b = B / world. */
#ifndef SPNERF_AMD_DP_H
#define SPNERF_AMD_DP_H

#include "spnerf_amd_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_DP_ABI_VERSION 1

int32_t spnerf_dp_abi_version(void);

/* The data-parallel sibling of spnerf_train_step_begin, one small launch.  With c = state->cursor
 * and b = B / world:
 *
 *   *cur               = plan_rows[c]
 *   batch_idx[0..b)    = perm[c B + rank b ..)          this rank's rays
 *   global_idx[0..B)   = perm[c B ..)                   the global batch (NULL: not written)
 *   clamp[0..2)        = rays[perm[c B] ld_rays + 6 .. + 8)
 *                        near / far of the GLOBAL batch's first ray: the guided clamp every rank
 *                        shares (`rays`: the dataset's (N, ld_rays) fp32 rows; rays and clamp are
 *                        both NULL or both set; ld_rays >= 8 when set)
 *   labels_global[i]   = sems[perm[c B + i]], i < B     int64 labels of the global batch, the
 *                        cross-entropy's denominator (sems and labels_global both NULL or both set)
 *   state->cursor      = c + 1
 *
 * With the cursor outside [0, n_steps), or B != state->B, nothing is read out of range: every
 * output and the cursor stay as they were and SPNERF_TRAIN_ERR_PAST_END / SPNERF_TRAIN_ERR_BATCH
 * is set in state->error.  perm's entries index `rays` and `sems` (the caller's plan holds a
 * permutation of the dataset's rows).  1 <= B < 2^31, world >= 1, 0 <= rank < world, B % world == 0.
 * With world = 1, rank = 0 it writes the cur and batch_idx spnerf_train_step_begin writes. */
int32_t spnerf_dp_step_begin(spnerf_train_state* state, const spnerf_train_step_scalars* plan_rows,
                             const int64_t* perm, spnerf_train_step_scalars* cur, int64_t* batch_idx,
                             int64_t* global_idx, int64_t B, int32_t rank, int32_t world, const float* rays,
                             int64_t ld_rays, float* clamp, const int64_t* sems, int64_t* labels_global, void* stream);

/* spnerf_adam_step_dev with every gradient element multiplied by `grad_scale` as it is loaded:
 * g' = (float)(g * grad_scale), one rounding, then spnerf_adam_step_dev's arithmetic on g' (same
 * block-to-tensor search, one pass over the tensors).  The host rounds grad_scale once from
 * 1.0 / world, so that Adam consumes the all-reduce's SUM and no separate pass divides the
 * gradient.  grad_scale == 1.0f is bit-equal to spnerf_adam_step_dev.  For a power-of-two world
 * the result is bit-equal to dividing the gradient by world first: x * 2^-k and x / 2^k round
 * the same, subnormal results included.  For any other world the result is DEFINED as the
 * product with the rounded reciprocal, which may differ from the quotient in the last bit.
 * grad_scale must be finite and > 0. */
int32_t spnerf_adam_step_dev_scaled(int32_t n, void* const* params, const void* const* grads, void* const* exp_avg,
                                    void* const* exp_avg_sq, const int64_t* numel,
                                    const spnerf_train_step_scalars* cur, double beta1, double beta2, double eps,
                                    float grad_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_DP_H */
