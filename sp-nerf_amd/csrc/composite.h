// What the per-ray compositing kernels share (csrc/composite.hip: forward and backward;
// csrc/view.hip: the inference-only image products): the argument block, the per-sample
// alpha / transparency / weights march of one ray and the staging of a ray's S x NO row block.
#pragma once
#include "common.h"
#include "wave.h"

namespace spn {

struct CompArgs {
    int64_t B;
    int S, NO, sem_col, n_sem, weights_only;
    const float *z, *out, *noise;
    float noise_std;
    spnerf_rng rng;   // noise drawn on the device when rng.state is set (and noise is null)
    float *rgb, *depth, *w, *T, *sem;
    const float *g_rgb, *g_depth, *g_w, *g_T, *g_sem;
    float* d_out;
    // weights-only passes with SPNERF_COMP_SUN_COLUMN: the sun-visibility column out (forward),
    // its gradient into d_out's sun column (backward) — the solar pass's sun_sc (rendering.py:177)
    float* sun_out;
    const float* g_sun;
    // spnerf_composite_*_dev: noise_std read from the device (a captured training step's schedule,
    // include/spnerf_amd_train.h); null on every other path, which reads the argument above
    const float* noise_std_dev;
};

__device__ __forceinline__ float relu_t(float x) { return x != x ? x : (x > 0.f ? x : 0.f); }

template <int EPL>
struct RayState {
    float z[EPL], al[EPL], t[EPL], T[EPL], w[EPL], r[EPL], E[EPL], dl[EPL];
};

// per-sample alpha / transparency / weights of one ray (spnerf.py:116-128)
// rows: the ray's S x NO output block (LDS copy)
template <int EPL>
__device__ __forceinline__ void march(const CompArgs& a, int64_t ray, int lane, const float* rows, RayState<EPL>& st) {
    const int S = a.S;
    const float noise_std = a.noise_std_dev ? *a.noise_std_dev : a.noise_std;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = lane * EPL + j;
        st.z[j] = e < S ? a.z[ray * S + e] : 0.f;
    }
    const float zn0 = __shfl_down(st.z[0], 1, 64);
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = lane * EPL + j;
        if (e < S) {
            const int64_t p = ray * S + e;
            float sg = rows[e * a.NO + 3];
            if (a.noise) sg = sg + a.noise[p] * noise_std;
            else if (a.rng.state) sg = sg + rng_normal(a.rng, ray, e) * noise_std;
            const float zn = j + 1 < EPL ? st.z[j + 1] : zn0;
            const float dl = e == S - 1 ? 1e10f : zn - st.z[j];
            const float r = relu_t(sg);
            const float E = expf(-dl * r);
            const float al = 1.f - E;
            st.dl[j] = dl;
            st.r[j] = r;
            st.E[j] = E;
            st.al[j] = al;
            st.t[j] = (1.f - al) + 1e-10f;
        } else {
            st.dl[j] = st.r[j] = st.E[j] = st.al[j] = 0.f;
            st.t[j] = 1.f;
        }
    }
    // exclusive cumprod in double (torch's CPU cumprod accumulates in double), rounded once
    double run = 1.0, excl[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        excl[j] = run;
        run *= (double)st.t[j];
    }
    const double incl = wave_scan_mul(run, lane);
    double lane_excl = __shfl_up(incl, 1, 64);
    if (lane == 0) lane_excl = 1.0;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        st.T[j] = (float)(lane_excl * excl[j]);
        st.w[j] = st.al[j] * st.T[j];
    }
}

// the ray's contiguous S·NO floats: HBM → this wave's LDS slice, 16-B pieces when aligned, up to
// 8 loads per lane in flight before their LDS stores
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, float* dst, int n, int lane) {
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int nq = n >> 2;
        for (int base = 0; base < nq; base += 512) {
            f32x4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = min(base + lane + 64 * k, nq - 1);  // clamped: unconditional loads
                v[k] = ld4(src + 4 * i);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = base + lane + 64 * k;
                if (i < nq) reinterpret_cast<f32x4*>(dst)[i] = v[k];
            }
        }
    } else {
        for (int i = lane; i < n; i += 64) dst[i] = src[i];
    }
    wave_lds_sync();
}

// One sample's share of a ray's depth and colour (spnerf.py:130-134,156): depth += w·z and
// c += (w·albedo)·(sun + (1 − sun)·sky).  The forward composite and the image-products kernel
// (view.hip) both accumulate through this one function and must agree bit for bit, so the
// roundings are spelled out instead of being left to the compiler's contraction, which decides
// by what else shares the loop body: a product is fused into the following add exactly where
// fmaf stands.  The asymmetry — the red channel's irradiance is a rounded product plus sun, the
// other two are fused — has no merit of its own: it is what the compiler happened to choose for
// k_composite_fwd before this function existed, written down so that the composite's results
// stay what they were.  The pragma is honoured under -ffp-contract=fast-honor-pragmas (hipcc's
// default, and named in the Makefile); under plain -ffp-contract=fast it would be ignored.
__device__ __forceinline__ void shade_depth(float w, float z, float& dsum) { dsum = __builtin_fmaf(w, z, dsum); }
__device__ __forceinline__ void shade_colour(float w, const float* o, float& c0, float& c1, float& c2) {
#pragma clang fp contract(off)
    const float sun = o[4], om = 1.f - sun;
    const float t0 = w * o[0], p0 = om * o[5];
    c0 = __builtin_fmaf(t0, sun + p0, c0);
    c1 = __builtin_fmaf(w * o[1], __builtin_fmaf(om, o[6], sun), c1);
    c2 = __builtin_fmaf(w * o[2], __builtin_fmaf(om, o[7], sun), c2);
}

// rays (waves) per block of a kernel that keeps `per_wave` bytes of LDS per ray: 4, or 1 when four
// row blocks would not fit
inline int comp_waves_per_block(size_t per_wave) { return per_wave * 4 <= 64 * 1024 ? 4 : 1; }

}  // namespace spn
