// The start of a captured training step (include/spnerf_amd_train.h): the step's row of the epoch
// plan to the fixed address the step's other kernels read their scalars from, the step's slice of
// the epoch's permutation into the gather's static index buffer, and the cursor advanced — what the
// host did per step before (a host-to-device copy of the indices, host floats baked into the
// launches) as one small launch that a HIP graph replays.
#include "common.h"

#include "../../include/spnerf_amd_dp.h"
#include "../../include/spnerf_amd_train.h"

namespace spn {

// One block: every thread reads the cursor before thread 0 moves it (the barrier), so the slice
// copied is the one the row belongs to.  The state is written with plain stores by thread 0.
__global__ __launch_bounds__(256) void k_train_step_begin(spnerf_train_state* st, const spnerf_train_step_scalars* rows,
                                                          const int64_t* perm, spnerf_train_step_scalars* cur,
                                                          int64_t* batch_idx, int64_t B) {
    const int64_t c = st->cursor, n = st->n_steps, planB = st->B;
    __syncthreads();
    const bool in_range = c >= 0 && c < n;
    if (!in_range || planB != B) {   // nothing read out of range, cur / batch_idx / cursor as they were
        if (threadIdx.x == 0)
            st->error = st->error | (!in_range ? SPNERF_TRAIN_ERR_PAST_END : 0) | (planB != B ? SPNERF_TRAIN_ERR_BATCH : 0);
        return;
    }
    const int64_t* src = perm + c * B;
    for (int64_t i = threadIdx.x; i < B; i += blockDim.x) batch_idx[i] = src[i];
    if (threadIdx.x == 0) {
        *cur = rows[c];
        st->cursor = c + 1;
    }
}

// The data-parallel step's start (include/spnerf_amd_dp.h): the same discipline — every thread
// reads the cursor, the barrier, thread 0 moves it — with this rank's slice of the global batch,
// the global batch itself, its labels and its first ray's near / far.  perm is read-only here, so
// the gathers through it need no ordering against the copies.
__global__ __launch_bounds__(256) void k_dp_step_begin(spnerf_train_state* st, const spnerf_train_step_scalars* rows,
                                                       const int64_t* perm, spnerf_train_step_scalars* cur,
                                                       int64_t* batch_idx, int64_t* global_idx, int64_t B, int64_t b,
                                                       int64_t rank, const float* rays, int64_t ld_rays, float* clamp,
                                                       const int64_t* sems, int64_t* labels_global) {
    const int64_t c = st->cursor, n = st->n_steps, planB = st->B;
    __syncthreads();
    const bool in_range = c >= 0 && c < n;
    if (!in_range || planB != B) {   // nothing read out of range, every output and the cursor as they were
        if (threadIdx.x == 0)
            st->error = st->error | (!in_range ? SPNERF_TRAIN_ERR_PAST_END : 0) | (planB != B ? SPNERF_TRAIN_ERR_BATCH : 0);
        return;
    }
    const int64_t* src = perm + c * B;
    const int64_t* mine = src + rank * b;
    for (int64_t i = threadIdx.x; i < b; i += blockDim.x) batch_idx[i] = mine[i];
    if (global_idx || sems) {
        for (int64_t i = threadIdx.x; i < B; i += blockDim.x) {
            const int64_t r = src[i];
            if (global_idx) global_idx[i] = r;
            if (sems) labels_global[i] = sems[r];
        }
    }
    if (rays && threadIdx.x < 2) clamp[threadIdx.x] = rays[src[0] * ld_rays + 6 + threadIdx.x];
    if (threadIdx.x == 0) {
        *cur = rows[c];
        st->cursor = c + 1;
    }
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_train_abi_version(void) { return SPNERF_TRAIN_ABI_VERSION; }

extern "C" int32_t spnerf_train_step_begin(spnerf_train_state* state, const spnerf_train_step_scalars* plan_rows,
                                           const int64_t* perm, spnerf_train_step_scalars* cur, int64_t* batch_idx,
                                           int64_t B, void* stream) {
    SPN_ARG(state && plan_rows && perm && cur && batch_idx, "train_step_begin: NULL pointer");
    SPN_ARG(B >= 1 && B < (1ll << 31), "train_step_begin: bad batch size B = %lld", (long long)B);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_step_begin", s, 0.0, (double)B * 16.0);
    hipLaunchKernelGGL(k_train_step_begin, dim3(1), dim3(256), 0, s, state, plan_rows, perm, cur, batch_idx, B);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_dp_abi_version(void) { return SPNERF_DP_ABI_VERSION; }

extern "C" int32_t spnerf_dp_step_begin(spnerf_train_state* state, const spnerf_train_step_scalars* plan_rows,
                                        const int64_t* perm, spnerf_train_step_scalars* cur, int64_t* batch_idx,
                                        int64_t* global_idx, int64_t B, int32_t rank, int32_t world, const float* rays,
                                        int64_t ld_rays, float* clamp, const int64_t* sems, int64_t* labels_global,
                                        void* stream) {
    SPN_ARG(state && plan_rows && perm && cur && batch_idx, "dp_step_begin: NULL pointer");
    SPN_ARG(B >= 1 && B < (1ll << 31), "dp_step_begin: bad batch size B = %lld", (long long)B);
    SPN_ARG(world >= 1, "dp_step_begin: bad world size %d", (int)world);
    SPN_ARG(rank >= 0 && rank < world, "dp_step_begin: rank %d outside [0, %d)", (int)rank, (int)world);
    SPN_ARG(B % world == 0, "dp_step_begin: the global batch %lld does not divide over %d ranks", (long long)B, (int)world);
    SPN_ARG((rays != nullptr) == (clamp != nullptr), "dp_step_begin: rays and clamp go together");
    SPN_ARG(!rays || ld_rays >= 8, "dp_step_begin: ld_rays = %lld < 8 (near / far are columns 6, 7)", (long long)ld_rays);
    SPN_ARG((sems != nullptr) == (labels_global != nullptr), "dp_step_begin: sems and labels_global go together");
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("dp_step_begin", s, 0.0, (double)B * 40.0);
    hipLaunchKernelGGL(k_dp_step_begin, dim3(1), dim3(256), 0, s, state, plan_rows, perm, cur, batch_idx, global_idx, B,
                       B / world, (int64_t)rank, rays, ld_rays, clamp, sems, labels_global);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
