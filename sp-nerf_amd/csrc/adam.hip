// Adam over a list of fp32 parameter tensors in one launch (the optimizer step of the training
// loop, reference main.py:97: torch.optim.Adam(parameters, lr, weight_decay=0), default betas / eps).
// torch's fused multi-tensor Adam took ~100 us per C2 step for 2.7 M parameters (0.75 TB/s):
// here every block owns 4096 consecutive elements of one tensor (found by a binary search over
// the per-tensor block prefix held in the kernel arguments), each thread 4 x float4.
#include <cmath>

#include "common.h"

#include "../../include/spnerf_amd_dp.h"
#include "../../include/spnerf_amd_train.h"

namespace spn {

constexpr int kAdamSeg = 48;           // tensors per launch (kernel-argument budget)
constexpr int kAdamChunk = 256 * 16;   // elements per block

struct AdamSeg {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
};
struct AdamArgs {
    AdamSeg s[kAdamSeg];
    int64_t first_block[kAdamSeg + 1];  // prefix of per-tensor block counts
    int nseg;
    float w1, beta2, w2, eps, step_size, bc2_sqrt;  // w = 1 - beta, rounded from double like torch's scalars
};

// torch's single-tensor Adam arithmetic (torch/optim/adam.py _single_tensor_adam):
// m.lerp_(g, 1-b1); v = v*b2 + (1-b2)*g*g; p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps)
// step_size and bc2_sqrt come from the arguments (k_adam) or from the step's device-resident
// scalars (k_adam_dev, spnerf_adam_step_dev): one arithmetic for both.  The roundings are spelled
// out instead of being left to the compiler's contraction, which decides by what else shares the
// function (a product is fused into the following add exactly where fmaf stands; the pragma is
// honoured under -ffp-contract=fast-honor-pragmas, see the Makefile).  VEC, the 16-byte path, fuses
// v·β2 into the sum and rounds (w2·g)·g; the element path rounds v·β2 and fuses the other product.
// The asymmetry has no merit of its own: it is what the compiler chose for k_adam's two paths
// before this function was shared, written down so that spnerf_adam_step's results stay what they
// were.
template <bool VEC>
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a, float step_size,
                                      float bc2_sqrt) {
#pragma clang fp contract(off)
    const float w = a.w1;
    const float d = g - m;
    m = w < 0.5f ? __builtin_fmaf(w, d, m) : __builtin_fmaf(-(1.f - w), d, g);
    const float gg = a.w2 * g;
    v = VEC ? __builtin_fmaf(v, a.beta2, gg * g) : __builtin_fmaf(gg, g, v * a.beta2);
    const float denom = sqrtf(v) / bc2_sqrt + a.eps;
    p = __builtin_fmaf(-step_size, m / denom, p);
}

// A gradient element of the scaled entry (spnerf_adam_step_dev_scaled): the product rounded to
// float on its own, never contracted into adam1's g - m, so that scale = 2^-k gives the bits of a
// gradient divided beforehand (subnormals included) and scale = 1 gives g itself.
__device__ __forceinline__ float scaled_grad(float g, float scale) {
#pragma clang fp contract(off)
    return g * scale;
}

// SCALED: every gradient element goes through scaled_grad as it is loaded; otherwise `scale` is
// not read and the code is what it was before the template parameter.
template <bool SCALED>
__device__ __forceinline__ void adam_block(const AdamArgs& a, float step_size, float bc2_sqrt, float scale = 1.f) {
    typedef const __attribute__((address_space(4))) AdamArgs* KArgs;
    const KArgs ka = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    const int64_t b = blockIdx.x;
    int lo = 0, hi = a.nseg - 1;  // last segment with first_block <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ka->first_block[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    const AdamSeg sg{ka->s[lo].p, ka->s[lo].g, ka->s[lo].m, ka->s[lo].v, ka->s[lo].n};  // scalar loads
    const int64_t base = (b - ka->first_block[lo]) * kAdamChunk;
    const bool vec = ((reinterpret_cast<uintptr_t>(sg.p) | reinterpret_cast<uintptr_t>(sg.g) |
                       reinterpret_cast<uintptr_t>(sg.m) | reinterpret_cast<uintptr_t>(sg.v)) & 15) == 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = base + (int64_t)(q * 256 + threadIdx.x) * 4;
        if (vec && i + 3 < sg.n) {
            f32x4 p = ld4(sg.p + i), g = ld4(sg.g + i), m = ld4(sg.m + i), v = ld4(sg.v + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = p[e], me = m[e], ve = v[e];
                adam1<true>(pe, SCALED ? scaled_grad(g[e], scale) : g[e], me, ve, a, step_size, bc2_sqrt);
                p[e] = pe;
                m[e] = me;
                v[e] = ve;
            }
            st4(sg.p + i, p);
            st4(sg.m + i, m);
            st4(sg.v + i, v);
        } else {
            for (int64_t j = i; j < i + 4 && j < sg.n; ++j) {
                float p = sg.p[j], m = sg.m[j], v = sg.v[j];
                adam1<false>(p, SCALED ? scaled_grad(sg.g[j], scale) : sg.g[j], m, v, a, step_size, bc2_sqrt);
                sg.p[j] = p;
                sg.m[j] = m;
                sg.v[j] = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_adam(AdamArgs a) { adam_block<false>(a, a.step_size, a.bc2_sqrt); }

// the kernel-argument block is the first argument in every kernel (adam_block reads the tensor
// table through the kernarg segment pointer)
__global__ __launch_bounds__(256) void k_adam_dev(AdamArgs a, const spnerf_train_step_scalars* cur) {
    adam_block<false>(a, cur->adam_step_size, cur->adam_bc2_sqrt);
}

__global__ __launch_bounds__(256) void k_adam_dev_scaled(AdamArgs a, const spnerf_train_step_scalars* cur, float scale) {
    adam_block<true>(a, cur->adam_step_size, cur->adam_bc2_sqrt, scale);
}

// the tensor table of one launch from entry i of the lists on: up to kAdamSeg non-empty tensors
static int32_t adam_fill(AdamArgs& a, int& i, int32_t n, void* const* params, const void* const* grads,
                         void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel, int64_t* blocks_out) {
    int64_t blocks = 0;
    for (; i < n && a.nseg < kAdamSeg; ++i) {
        SPN_ARG(numel[i] >= 0, "adam_step: tensor %d has negative size", i);
        if (numel[i] == 0) continue;
        a.s[a.nseg] = AdamSeg{(float*)params[i], (const float*)grads[i], (float*)exp_avg[i], (float*)exp_avg_sq[i],
                              numel[i]};
        a.first_block[a.nseg] = blocks;
        blocks += (numel[i] + kAdamChunk - 1) / kAdamChunk;
        ++a.nseg;
    }
    a.first_block[a.nseg] = blocks;
    *blocks_out = blocks;
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_adam_step(int32_t n, void* const* params, const void* const* grads, void* const* exp_avg,
                                    void* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2,
                                    double eps, int32_t step, void* stream) {
    SPN_ARG(n >= 0 && (n == 0 || (params && grads && exp_avg && exp_avg_sq && numel)), "adam_step: bad lists");
    SPN_ARG(step >= 1 && lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0,
            "adam_step: bad hyper-parameters");
    hipStream_t s = (hipStream_t)stream;
    const double bc1 = 1.0 - std::pow(beta1, step), bc2 = 1.0 - std::pow(beta2, step);
    for (int i = 0; i < n;) {
        AdamArgs a{};
        a.w1 = (float)(1.0 - beta1);
        a.beta2 = (float)beta2;
        a.w2 = (float)(1.0 - beta2);
        a.eps = (float)eps;
        a.step_size = (float)(lr / bc1);
        a.bc2_sqrt = (float)std::sqrt(bc2);
        int64_t blocks = 0;
        SPN_TRY(adam_fill(a, i, n, params, grads, exp_avg, exp_avg_sq, numel, &blocks));
        if (blocks == 0) continue;
        SPN_ARG(blocks < (1ll << 31), "adam_step: too many elements");
        ProfScope prof("adam", s, 0.0, 0.0);
        hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(256), 0, s, a);
        SPN_HIP(hipGetLastError());
    }
    return SPNERF_OK;
}

// spnerf_adam_step_dev (scale == nullptr) and spnerf_adam_step_dev_scaled: one host path, two kernels
static int32_t adam_step_dev(const char* what, int32_t n, void* const* params, const void* const* grads,
                             void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel,
                             const spnerf_train_step_scalars* cur, double beta1, double beta2, double eps,
                             const float* scale, void* stream) {
    SPN_ARG(n >= 0 && (n == 0 || (params && grads && exp_avg && exp_avg_sq && numel)), "%s: bad lists", what);
    SPN_ARG(cur, "%s: NULL step scalars", what);
    SPN_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0, "%s: bad hyper-parameters", what);
    SPN_ARG(!scale || (std::isfinite(*scale) && *scale > 0.f), "%s: grad_scale must be finite and > 0", what);
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < n;) {
        AdamArgs a{};
        a.w1 = (float)(1.0 - beta1);
        a.beta2 = (float)beta2;
        a.w2 = (float)(1.0 - beta2);
        a.eps = (float)eps;
        int64_t blocks = 0;
        SPN_TRY(adam_fill(a, i, n, params, grads, exp_avg, exp_avg_sq, numel, &blocks));
        if (blocks == 0) continue;
        SPN_ARG(blocks < (1ll << 31), "%s: too many elements", what);
        ProfScope prof("adam", s, 0.0, 0.0);
        if (scale) hipLaunchKernelGGL(k_adam_dev_scaled, dim3((unsigned)blocks), dim3(256), 0, s, a, cur, *scale);
        else hipLaunchKernelGGL(k_adam_dev, dim3((unsigned)blocks), dim3(256), 0, s, a, cur);
        SPN_HIP(hipGetLastError());
    }
    return SPNERF_OK;
}

extern "C" int32_t spnerf_adam_step_dev(int32_t n, void* const* params, const void* const* grads, void* const* exp_avg,
                                        void* const* exp_avg_sq, const int64_t* numel,
                                        const spnerf_train_step_scalars* cur, double beta1, double beta2, double eps,
                                        void* stream) {
    return adam_step_dev("adam_step_dev", n, params, grads, exp_avg, exp_avg_sq, numel, cur, beta1, beta2, eps, nullptr,
                         stream);
}

extern "C" int32_t spnerf_adam_step_dev_scaled(int32_t n, void* const* params, const void* const* grads,
                                               void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel,
                                               const spnerf_train_step_scalars* cur, double beta1, double beta2,
                                               double eps, float grad_scale, void* stream) {
    return adam_step_dev("adam_step_dev_scaled", n, params, grads, exp_avg, exp_avg_sq, numel, cur, beta1, beta2, eps,
                         &grad_scale, stream);
}
