/* Training-step exports of libspnerf_amd.so (gfx950): what lets ONE replay of one HIP graph cover a
 * whole training step of the reference trainer (main.py:95-106,125-186) — advancing the schedule,
 * picking the batch, gather, render, loss, backward and Adam — with nothing that changes per step
 * left as a host scalar baked into a captured launch.  A separate header so that the older ABIs
 * stay as they are; the conventions are theirs: every function returns SPNERF_OK or a negative
 * SPNERF_E_* code with the text in spnerf_last_error, pointers are device pointers unless noted,
 * `stream` is a hipStream_t, and no call synchronises with the host, allocates, or uses atomics on
 * global memory — results are bit-reproducible from run to run and every call can be captured in a
 * HIP graph.
 *
 * The epoch plan.  The host computes each step's scalars in double, exactly as the host-scalar
 * path does (so the device path is bit-identical by construction, not by a device pow), and
 * uploads them once per epoch, outside the graph, with that epoch's permutation of the rays:
 *
 *   plan_rows[n_steps]   one spnerf_train_step_scalars per step of the epoch
 *   perm[n_steps * B]    int64 ray indices: step k of the epoch trains on perm[k B .. k B + B)
 *   state                one spnerf_train_state {cursor, n_steps, B, error}
 *
 * spnerf_train_step_begin copies row `cursor` to a fixed address `cur` that every other kernel of
 * the step reads its scalars from, copies the step's index slice into the gather's static index
 * buffer, and advances the cursor. */
#ifndef SPNERF_AMD_TRAIN_H
#define SPNERF_AMD_TRAIN_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_TRAIN_ABI_VERSION 1

/* spnerf_train_state.error bits */
#define SPNERF_TRAIN_ERR_PAST_END 1 /* step_begin with cursor outside [0, n_steps)                 */
#define SPNERF_TRAIN_ERR_BATCH 2    /* step_begin's B differs from the plan's                      */

/* One step's scalars (24 bytes). */
typedef struct spnerf_train_step_scalars {
    float noise_std;      /* the float the host path passes to the composites at that step          */
    float lr;             /* the epoch's learning rate (reported; Adam reads adam_step_size)        */
    float adam_step_size; /* (float)(lr / (1 - beta1^t))                                            */
    float adam_bc2_sqrt;  /* (float)sqrt(1 - beta2^t)                                               */
    int64_t step;         /* the global step t >= 1                                                 */
} spnerf_train_step_scalars;

/* The device-resident description of the uploaded plan (32 bytes). */
typedef struct spnerf_train_state {
    int64_t cursor;  /* next row of the plan, advanced by spnerf_train_step_begin                   */
    int64_t n_steps; /* rows of the plan                                                            */
    int64_t B;       /* rays per step                                                               */
    int64_t error;   /* SPNERF_TRAIN_ERR_* bits, set by the kernel, never cleared by it             */
} spnerf_train_state;

int32_t spnerf_train_abi_version(void);

/* One small launch: cur = plan_rows[cursor], batch_idx[0..B) = perm[cursor B ..], cursor += 1.
 * With the cursor outside [0, n_steps), or B != state->B, nothing is read out of range: cur,
 * batch_idx and the cursor stay as they were and the matching error bit is set (the caller reads
 * it once per epoch).  1 <= B < 2^31. */
int32_t spnerf_train_step_begin(spnerf_train_state* state, const spnerf_train_step_scalars* plan_rows,
                                const int64_t* perm, spnerf_train_step_scalars* cur, int64_t* batch_idx, int64_t B,
                                void* stream);

/* spnerf_adam_step with the step's two bias-correction scalars read from the device:
 * step_size = cur->adam_step_size, bc2_sqrt = cur->adam_bc2_sqrt; beta1, beta2 and eps are rounded
 * on the host as spnerf_adam_step rounds them.  Same arithmetic, same block-to-tensor search:
 * bit-equal to spnerf_adam_step at (lr, step) when cur holds that step's scalars.  The lists are host
 * arrays of device pointers, read before the call returns. */
int32_t spnerf_adam_step_dev(int32_t n, void* const* params, const void* const* grads, void* const* exp_avg,
                             void* const* exp_avg_sq, const int64_t* numel, const spnerf_train_step_scalars* cur,
                             double beta1, double beta2, double eps, void* stream);

/* spnerf_composite_forward / _backward with noise_std read from the device (a pointer into cur).
 * The host cannot know whether *noise_std is 0, so with rng set the draw is always made and
 * multiplied: a draw is finite (Box-Muller of u1 in [2^-24, 1]: |draw| < 5.8), so at
 * *noise_std == 0 the product is +-0 and sigma's relu sees the same value as on the scalar path,
 * which skips the draw — outputs and gradients are bit-equal. */
int32_t spnerf_composite_forward_dev(int64_t n_rays, int32_t n_samples, const float* z, const float* out,
                                     int32_t n_out, const float* noise, const float* noise_std, int32_t sem_col,
                                     int32_t n_sem, int32_t flags, float* rgb, float* depth, float* weights,
                                     float* transparency, float* sem_logits, const spnerf_rng* rng, void* stream);
int32_t spnerf_composite_backward_dev(int64_t n_rays, int32_t n_samples, const float* z, const float* out,
                                      int32_t n_out, const float* noise, const float* noise_std, int32_t sem_col,
                                      int32_t n_sem, int32_t flags, const float* g_rgb, const float* g_depth,
                                      const float* g_weights, const float* g_transparency, const float* g_sem,
                                      float* d_out, const spnerf_rng* rng, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_TRAIN_H */
