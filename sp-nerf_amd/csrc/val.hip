// Validation-loss kernels (include/spnerf_amd_val.h).
//
//  * k_val_solar_terms — the sibling of k_composite_products (view.hip) for the solar pass: one
//    wavefront per ray, the ray's S x NO row block of the sun-only forward staged once into the
//    wave's LDS slice, the composite's own march (composite.h: α, T and w bit for bit those of
//    k_composite_fwd), and from them the two per-ray sums of solar_correction (metrics.py:17-24):
//    Σ (T − sun)² and 1 − Σ w·sun.  Each product is rounded before it is added (no fused
//    multiply-add), a lane adds its samples in index order and the wave's xor butterfly adds the
//    lanes: the order can be restated exactly.  Only 8 B per ray leave the kernel; the per-sample
//    weights, transparency and sun column (12 B per sample through render_rays) are never stored.
//  * k_val_loss / k_val_loss_finish — one pass over the view's planes in the scheme of
//    k_view_metrics: six fp64 sums, each workgroup's partials stored, one workgroup adding them in
//    workgroup order and forming the terms of SNerfLoss / SatNerfLoss (metrics.py:27-65).  Fixed
//    grid, fixed order, no atomics on global memory: two calls give the same bits.
#include <cmath>

#include "../../include/spnerf_amd_val.h"
#include "composite.h"

namespace spn {

struct SolarArgs {
    CompArgs c;   // what march() reads: B, S, NO, z, out, noise, noise_std, rng
    int sun_col;
    int64_t ray_begin;
    float *term2, *term3;
};

// One sample's share of the two sums: s2 += (T − sun)², s3 += w·sun, every product rounded before
// it is added.  The pragma keeps the compiler from fusing them (it is honoured under
// -ffp-contract=fast-honor-pragmas, see composite.h: shade_colour), so that the sums can be restated
// operation by operation.
__device__ __forceinline__ void solar_sample(float T, float w, float sun, float& s2, float& s3) {
#pragma clang fp contract(off)
    const float d = T - sun;
    const float p2 = d * d, p3 = w * sun;
    s2 = s2 + p2;
    s3 = s3 + p3;
}

template <int EPL>
__global__ __launch_bounds__(256) void k_val_solar_terms(SolarArgs v) {
    extern __shared__ __attribute__((aligned(16))) float sh_rows[];
    const CompArgs& a = v.c;
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= a.B) return;  // wave-uniform; the LDS slices are wave-private (no block barrier)
    const int S = a.S, NO = a.NO;
    float* rows = sh_rows + (threadIdx.x >> 6) * (S * NO);
    stage_rows(a.out + ray * (int64_t)(S * NO), rows, S * NO, lane);
    RayState<EPL> st;
    march<EPL>(a, ray, lane, rows, st);
    float s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = lane * EPL + j;
        if (e >= S) continue;
        solar_sample(st.T[j], st.w[j], rows[e * NO + v.sun_col], s2, s3);
    }
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    if (lane == 0) {
        v.term2[v.ray_begin + ray] = s2;
        v.term3[v.ray_begin + ray] = __fsub_rn(1.f, s3);
    }
}

template <int EPL>
static int32_t launch_solar(const SolarArgs& v, hipStream_t s) {
    const size_t per_wave = (size_t)v.c.S * v.c.NO * sizeof(float);
    const int wpb = comp_waves_per_block(per_wave);
    const dim3 grid((unsigned)((v.c.B + wpb - 1) / wpb)), block(64 * wpb);
    hipLaunchKernelGGL(k_val_solar_terms<EPL>, grid, block, per_wave * wpb, s, v);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

// ---- the loss of a view ---------------------------------------------------------------------------

constexpr int kLossThreads = 256;
constexpr int kLossMaxBlocks = 1024;   // also the finish's summation length
constexpr int kLossSums = 6;           // Σ(rgb−t)², Σ(rgb_c−t)², Σ(rgb−t)²/(2b²), Σ log b, Σ term2, Σ term3

// a fixed function of the view's size alone
static int loss_blocks(int64_t n_rays) {
    const int64_t nb = (n_rays + kLossThreads - 1) / kLossThreads;
    return (int)(nb < kLossMaxBlocks ? nb : kLossMaxBlocks);
}

struct LossArgs {
    int64_t n;
    const float *rgb, *tgt, *rgb_c, *beta, *term2, *term3;
    double lambda_sc, beta_min;
    double* part;   // [blocks][kLossSums]
};

__global__ __launch_bounds__(kLossThreads) void k_val_loss(LossArgs m) {
    __shared__ double s_part[kLossThreads / 64][kLossSums];
    const int tid = threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kLossThreads;
    double acc[kLossSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t r = (int64_t)blockIdx.x * kLossThreads + tid; r < m.n; r += stride) {
        double sq = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double t = (double)m.tgt[3 * r + k];
            const double d = (double)m.rgb[3 * r + k] - t;
            sq += d * d;
            if (m.rgb_c) {
                const double dc = (double)m.rgb_c[3 * r + k] - t;
                acc[1] += dc * dc;
            }
        }
        acc[0] += sq;
        if (m.beta) {
            const double b = (double)m.beta[r] + m.beta_min;
            acc[2] += sq / (2.0 * b * b);
            acc[3] += log(b);
        }
        if (m.term2) {
            acc[4] += (double)m.term2[r];
            acc[5] += (double)m.term3[r];
        }
    }
#pragma unroll
    for (int k = 0; k < kLossSums; ++k) {
        const double t = wave_sum(acc[k]);
        if ((tid & 63) == 0) s_part[tid >> 6][k] = t;
    }
    __syncthreads();
    if (tid < kLossSums) {
        double t = 0.0;
        for (int w = 0; w < kLossThreads / 64; ++w) t += s_part[w][tid];
        m.part[(int64_t)blockIdx.x * kLossSums + tid] = t;
    }
}

__global__ __launch_bounds__(64) void k_val_loss_finish(LossArgs m, int nblocks, spnerf_val_loss_result* res) {
    __shared__ double s_tot[kLossSums];
    const int tid = threadIdx.x;
    if (tid < kLossSums) {
        double t = 0.0;
        for (int b = 0; b < nblocks; ++b) t += m.part[(int64_t)b * kLossSums + tid];   // workgroup order
        s_tot[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        const double n = (double)m.n;
        spnerf_val_loss_result r{};
        r.n = n;
        r.color = (m.beta ? s_tot[2] : s_tot[0]) / (3.0 * n);
        double loss = r.color;
        if (m.rgb_c) {
            r.color_coarse = s_tot[1] / (3.0 * n);
            loss += r.color_coarse;
        }
        if (m.beta) {
            r.logbeta = (3.0 + s_tot[3] / n) / 2.0;
            loss += r.logbeta;
        }
        if (m.term2) {
            r.sc_term2 = m.lambda_sc / 3.0 * (s_tot[4] / n);
            r.sc_term3 = m.lambda_sc / 3.0 * (s_tot[5] / n);
            loss += r.sc_term2;
            loss += r.sc_term3;
        }
        r.loss = loss;
        *res = r;
    }
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_val_abi_version(void) { return SPNERF_VAL_ABI_VERSION; }

extern "C" int32_t spnerf_val_solar_terms(int64_t n_rays, int32_t n_samples, const float* z, const float* out,
                                          int32_t out_stride, int32_t sun_col, const float* noise, float noise_std,
                                          int64_t ray_begin, float* term2, float* term3, const spnerf_rng* rng,
                                          void* stream) {
    SPN_ARG(z && out, "val_solar_terms: NULL z or out");
    SPN_ARG(term2 && term3, "val_solar_terms: NULL term2 or term3");
    SPN_ARG(n_rays >= 0, "val_solar_terms: n_rays %lld is negative", (long long)n_rays);
    SPN_ARG(n_samples >= 1 && n_samples <= 256, "val_solar_terms: n_samples %d must be in [1, 256]", n_samples);
    SPN_ARG(sun_col >= 0 && out_stride >= 4, "val_solar_terms: sun_col %d outside the row (out_stride %d, sigma in column 3)",
            sun_col, out_stride);
    SPN_ARG(out_stride >= sun_col + 1, "val_solar_terms: out_stride %d is below sun_col + 1 = %d", out_stride, sun_col + 1);
    SPN_ARG((size_t)2 * n_samples * out_stride * sizeof(float) <= 64 * 1024,
            "val_solar_terms: n_samples x out_stride = %d x %d too large", n_samples, out_stride);
    SPN_ARG(ray_begin >= 0, "val_solar_terms: ray_begin %lld is negative", (long long)ray_begin);
    if (n_rays == 0) return SPNERF_OK;
    SolarArgs v{};
    v.c.B = n_rays; v.c.S = n_samples; v.c.NO = out_stride;
    v.c.z = z; v.c.out = out; v.c.noise = noise; v.c.noise_std = noise_std;
    if (!noise && rng && noise_std != 0.f) v.c.rng = *rng;
    v.sun_col = sun_col;
    v.ray_begin = ray_begin;
    v.term2 = term2; v.term3 = term3;
    hipStream_t s = (hipStream_t)stream;
    const double P = (double)n_rays * n_samples;
    ProfScope prof("val_solar_terms", s, 0.0, P * (out_stride * 4.0 + 4.0 + (noise ? 4.0 : 0.0)) + n_rays * 8.0);
    if (n_samples <= 64) return launch_solar<1>(v, s);
    if (n_samples <= 128) return launch_solar<2>(v, s);
    return launch_solar<4>(v, s);
}

extern "C" int64_t spnerf_val_loss_workspace_bytes(int64_t n_rays) {
    SPN_ARG(n_rays >= 1, "val_loss_workspace_bytes: n_rays %lld must be positive", (long long)n_rays);
    return (int64_t)((size_t)loss_blocks(n_rays) * kLossSums * sizeof(double));
}

extern "C" int32_t spnerf_val_loss(int64_t n_rays, const float* rgb, const float* target_rgb, const float* rgb_coarse,
                                   const float* beta, const float* term2, const float* term3, double lambda_sc,
                                   double beta_min, void* workspace, spnerf_val_loss_result* result, void* stream) {
    SPN_ARG(rgb && target_rgb && workspace && result, "val_loss: NULL image, workspace or result");
    SPN_ARG(n_rays >= 1, "val_loss: n_rays %lld must be positive", (long long)n_rays);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "val_loss: workspace not 16-byte aligned");
    SPN_ARG((term2 != nullptr) == (term3 != nullptr), "val_loss: term2 and term3 go together");
    SPN_ARG(!(beta && rgb_coarse), "val_loss: beta with rgb_coarse (the fine uncertainty term needs per-sample beta)");
    SPN_ARG(!beta || beta_min > 0.0, "val_loss: beta_min %g must be positive", beta_min);
    const int nb = loss_blocks(n_rays);
    LossArgs m{};
    m.n = n_rays; m.rgb = rgb; m.tgt = target_rgb; m.rgb_c = rgb_coarse; m.beta = beta; m.term2 = term2; m.term3 = term3;
    m.lambda_sc = lambda_sc; m.beta_min = beta_min;
    m.part = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("val_loss", s, 0.0, (double)n_rays * (24.0 + (rgb_coarse ? 12.0 : 0.0) + (beta ? 4.0 : 0.0) + (term2 ? 8.0 : 0.0)));
    hipLaunchKernelGGL(k_val_loss, dim3(nb), dim3(kLossThreads), 0, s, m);
    SPN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_val_loss_finish, dim3(1), dim3(64), 0, s, m, nb, result);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
