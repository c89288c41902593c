// Whole-view kernels (include/spnerf_amd_view.h).
//
//  * k_composite_products — the inference-only sibling of k_composite_fwd (composite.hip): one
//    wavefront per ray, the ray's S x NO row block staged once into the wave's LDS slice, the same
//    march (so rgb and depth come out bit for bit as the composite's), and besides them the image
//    products of eval.py:76-101 — Σ w·sun, Σ w·albedo, Σ w·sky, Σ w·β — the mean semantic logits and
//    their argmax.  Only per-ray values leave the kernel, written to caller-owned image planes at
//    plane[ray_begin + ray]; the per-sample weights and transparency (8 B per sample in the
//    composite) are never stored.
//  * k_view_metrics / k_view_metrics_finish — one pass over a rendered view and its targets:
//    Σ (rgb − target)² in fp64 and the (C + 1) x C confusion table of (label, predicted class).
//    Each workgroup keeps its partials in LDS and stores them; one workgroup sums the partials in
//    workgroup order and writes mse, psnr, n, correct and the table.  Fixed grid, fixed order, no
//    atomics on global memory: two calls give the same bits.
#include <cmath>

#include "../../include/spnerf_amd_view.h"
#include "composite.h"

namespace spn {

struct ProductArgs {
    CompArgs c;   // what march() reads: B, S, NO, z, out, noise, noise_std, rng, sem_col, n_sem
    spnerf_view_planes p;
    int64_t ray_begin;
    int beta_col;
};

constexpr int kSemBatch = 4;   // semantic classes reduced together with the twelve image sums

// wave_sum of 16 values at once.  At the steps 32, 16, 8, 4 a lane keeps the half of its values
// that its lane bit selects and trades the other half with its partner, so each step adds exactly
// the pair wave_sum's xor butterfly adds (v + shfl_xor(v, off)) and the summation tree of every
// value — hence every bit of its sum — is wave_sum's; 8 + 4 + 2 + 1 exchanges and two plain steps
// instead of 16 x 6.  Returns, in lanes 4k .. 4k + 3, the wave's sum of value k.
__device__ __forceinline__ float wave_sum16(f32x16 v, int lane) {   // a vector value: constant element indices only
#pragma unroll
    for (int half = 8, off = 32; half >= 1; half >>= 1, off >>= 1) {
        const bool hi = lane & off;
#pragma unroll
        for (int k = 0; k < half; ++k) {
            float lo = v[k], up = v[k + half];
            asm volatile("" : "+v"(lo), "+v"(up));   // or the selects below become a runtime-indexed element read
            const float keep = hi ? up : lo, send = hi ? lo : up;
            v[k] = keep + __shfl_xor(send, off, 64);
        }
    }
    float r = v[0];
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 1, 64);
    return r;
}

template <int EPL>
__global__ __launch_bounds__(256) void k_composite_products(ProductArgs v) {
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
    const int64_t px = v.ray_begin + ray;
    // One pass over the ray's rows fills 16 per-lane sums: [0] depth and [1..3] colour through the
    // composite's own accumulation (composite.h: bit for bit its values), [4] w·sun, [5..7]
    // w·albedo, [8..10] w·sky, [11] w·β (eval.py:76-101: fp32, a lane's samples in index order),
    // [12..15] the first four semantic logits, unweighted as the composite sums them.
    const int bc = v.beta_col, nq = a.n_sem < kSemBatch ? a.n_sem : kSemBatch;
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int e = lane * EPL + j;
        if (e >= S) continue;
        const float* o = rows + e * NO;
        const float w = st.w[j];
        float d = acc[0], c0 = acc[1], c1 = acc[2], c2 = acc[3];
        shade_depth(w, st.z[j], d);
        shade_colour(w, o, c0, c1, c2);
        acc[0] = d; acc[1] = c0; acc[2] = c1; acc[3] = c2;
        acc[4] += w * o[4];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            acc[5 + q] += w * o[q];
            acc[8 + q] += w * o[5 + q];
        }
        if (bc >= 0) acc[11] += w * o[bc];
#pragma unroll
        for (int c = 0; c < kSemBatch; ++c)
            if (c < nq) acc[12 + c] += o[a.sem_col + c];
    }
    // all 16 through one transposing butterfly: lane 4k ends with the wave's sum of value k
    const float tot = wave_sum16(acc, lane);
    const int k = lane >> 2;
    const bool owner = (lane & 3) == 0;
    if (owner) {
        if (k == 0) {
            if (v.p.depth) v.p.depth[px] = tot;
        } else if (k < 4) {
            if (v.p.rgb) v.p.rgb[px * 3 + (k - 1)] = fminf(fmaxf(tot, 0.f), 1.f);
        } else if (k == 4) {
            if (v.p.sun) v.p.sun[px] = tot;
        } else if (k < 8) {
            if (v.p.albedo) v.p.albedo[px * 3 + (k - 5)] = tot;
        } else if (k < 11) {
            if (v.p.sky) v.p.sky[px * 3 + (k - 8)] = tot;
        } else if (k == 11) {
            if (v.p.beta && bc >= 0) v.p.beta[px] = tot;
        }
    }
    if (a.n_sem == 0 || !(v.p.sem_logits || v.p.sem_class)) return;
    // the mean logits as the composite forms them; torch.argmax over them: the first maximum, a
    // NaN counting as the maximum (the first NaN stands)
    const float mine = tot / (float)S;   // in lane 4·(12 + c): the mean of class c < 4
    if (owner && k >= 12 && k - 12 < nq && v.p.sem_logits) v.p.sem_logits[px * a.n_sem + (k - 12)] = mine;
    float best = 0.f;
    int cls = 0;
    for (int c = 0; c < a.n_sem; ++c) {
        float m;
        if (c < kSemBatch) {
            m = __shfl(mine, 4 * (12 + c), 64);
        } else {   // classes past the batch: one butterfly each
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < EPL; ++j) {
                const int e = lane * EPL + j;
                if (e < S) s += rows[e * NO + a.sem_col + c];
            }
            m = wave_sum(s) / (float)S;   // the xor butterfly leaves the same bits in every lane
            if (lane == 0 && v.p.sem_logits) v.p.sem_logits[px * a.n_sem + c] = m;
        }
        if (c == 0 || (best == best && (m > best || m != m))) {
            best = m;
            cls = c;
        }
    }
    if (lane == 0 && v.p.sem_class) v.p.sem_class[px] = cls;
}

template <int EPL>
static int32_t launch_products(const ProductArgs& v, hipStream_t s) {
    const size_t per_wave = (size_t)v.c.S * v.c.NO * sizeof(float);
    const int wpb = comp_waves_per_block(per_wave);
    const dim3 grid((unsigned)((v.c.B + wpb - 1) / wpb)), block(64 * wpb);
    hipLaunchKernelGGL(k_composite_products<EPL>, grid, block, per_wave * wpb, s, v);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

// ---- image metrics ------------------------------------------------------------------------------

constexpr int kMetricThreads = 256;
constexpr int kMetricMaxBlocks = 1024;   // 4 workgroups per CU; also the finish's summation length
constexpr int kTableMax = (SPNERF_VIEW_MAX_CLASSES + 1) * SPNERF_VIEW_MAX_CLASSES;

// a fixed function of the view's size alone
static int metric_blocks(int64_t n_rays) {
    const int64_t nb = (n_rays + kMetricThreads - 1) / kMetricThreads;
    return (int)(nb < kMetricMaxBlocks ? nb : kMetricMaxBlocks);
}

struct MetricArgs {
    int64_t n;
    const float *rgb, *tgt;
    const int32_t* cls;
    const int64_t* lab;
    int C;          // 0: no table
    double* sq;     // [blocks]
    int64_t* tab;   // [blocks][(C + 1) * C]
};

__global__ __launch_bounds__(kMetricThreads) void k_view_metrics(MetricArgs m) {
    __shared__ unsigned int s_tab[kTableMax];
    __shared__ double s_sq[kMetricThreads / 64];
    const int tid = threadIdx.x;
    const int ncell = (m.C + 1) * m.C;
    for (int i = tid; i < ncell; i += kMetricThreads) s_tab[i] = 0u;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kMetricThreads;
    const int64_t t0 = (int64_t)blockIdx.x * kMetricThreads + tid;
    // squared error over the 3N values, four consecutive values per step (16-B loads when both
    // images are 16-B aligned), the tail one by one
    const int64_t n3 = 3 * m.n, nq = n3 >> 2;
    double acc = 0.0;
    if (((reinterpret_cast<uintptr_t>(m.rgb) | reinterpret_cast<uintptr_t>(m.tgt)) & 15) == 0) {
        for (int64_t i = t0; i < nq; i += stride) {
            const f32x4 a = ld4(m.rgb + 4 * i), b = ld4(m.tgt + 4 * i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)a[k] - (double)b[k];
                acc += d * d;
            }
        }
    } else {
        for (int64_t i = t0; i < nq; i += stride) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double d = (double)m.rgb[4 * i + k] - (double)m.tgt[4 * i + k];
                acc += d * d;
            }
        }
    }
    for (int64_t i = 4 * nq + t0; i < n3; i += stride) {
        const double d = (double)m.rgb[i] - (double)m.tgt[i];
        acc += d * d;
    }
    // the confusion table: integer counts in LDS (their order does not matter)
    if (ncell) {
        for (int64_t r = t0; r < m.n; r += stride) {
            const int64_t l = m.lab[r];
            const int32_t c = m.cls[r];
            const int row = (l >= 0 && l < m.C) ? (int)l : m.C;
            if (c >= 0 && c < m.C) atomicAdd(&s_tab[row * m.C + c], 1u);
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) s_sq[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < kMetricThreads / 64; ++w) t += s_sq[w];
        m.sq[blockIdx.x] = t;
    }
    for (int i = tid; i < ncell; i += kMetricThreads) m.tab[(int64_t)blockIdx.x * ncell + i] = (int64_t)s_tab[i];
}

__global__ __launch_bounds__(kMetricThreads) void k_view_metrics_finish(MetricArgs m, int nblocks,
                                                                        spnerf_view_metrics_result* res) {
    __shared__ int64_t s_tab[kTableMax];
    const int tid = threadIdx.x;
    const int ncell = (m.C + 1) * m.C;
    for (int i = tid; i < ncell; i += kMetricThreads) {
        int64_t t = 0;
        for (int b = 0; b < nblocks; ++b) t += m.tab[(int64_t)b * ncell + i];
        s_tab[i] = t;
        res->table[i] = t;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int b = 0; b < nblocks; ++b) t += m.sq[b];   // workgroup order
        const double mse = t / (double)(3 * m.n);
        res->mse = mse;
        res->psnr = -10.0 * log10(mse);
        res->n = m.n;
        int64_t ok = 0;
        for (int c = 0; c < m.C; ++c) ok += s_tab[c * m.C + c];
        res->correct = ok;
    }
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_view_abi_version(void) { return SPNERF_VIEW_ABI_VERSION; }

extern "C" int32_t spnerf_view_composite_products(int64_t n_rays, int32_t n_samples, const float* z, const float* out,
                                                  int32_t n_out, const float* noise, float noise_std, int32_t sem_col,
                                                  int32_t n_sem, int32_t beta_col, int64_t ray_begin,
                                                  const spnerf_view_planes* planes, const spnerf_rng* rng, void* stream) {
    SPN_ARG(z && out, "view_composite_products: NULL z or out");
    SPN_ARG(planes, "view_composite_products: NULL planes");
    SPN_ARG(n_rays >= 0, "view_composite_products: n_rays %lld is negative", (long long)n_rays);
    SPN_ARG(n_samples >= 1 && n_samples <= 256, "view_composite_products: n_samples %d must be in [1, 256]", n_samples);
    SPN_ARG(n_out >= 8 && n_sem >= 0 && sem_col >= 0 && sem_col + n_sem <= n_out,
            "view_composite_products: bad output layout (n_out %d, sem_col %d, n_sem %d)", n_out, sem_col, n_sem);
    SPN_ARG(beta_col == -1 || (beta_col >= 8 && beta_col < n_out), "view_composite_products: beta_col %d is neither -1 nor in [8, %d)",
            beta_col, n_out);
    SPN_ARG((size_t)2 * n_samples * n_out * sizeof(float) <= 64 * 1024,
            "view_composite_products: n_samples x n_out = %d x %d too large", n_samples, n_out);
    SPN_ARG(ray_begin >= 0, "view_composite_products: ray_begin %lld is negative", (long long)ray_begin);
    SPN_ARG(!planes->beta || beta_col >= 0, "view_composite_products: a beta plane needs beta_col");
    SPN_ARG(!(planes->sem_logits || planes->sem_class) || n_sem > 0, "view_composite_products: semantic planes need n_sem > 0");
    if (n_rays == 0) return SPNERF_OK;
    ProductArgs v{};
    v.c.B = n_rays; v.c.S = n_samples; v.c.NO = n_out; v.c.sem_col = sem_col; v.c.n_sem = n_sem;
    v.c.z = z; v.c.out = out; v.c.noise = noise; v.c.noise_std = noise_std;
    if (!noise && rng && noise_std != 0.f) v.c.rng = *rng;
    v.p = *planes;
    v.ray_begin = ray_begin;
    v.beta_col = beta_col;
    hipStream_t s = (hipStream_t)stream;
    const double P = (double)n_rays * n_samples;
    const int per_ray = (planes->rgb ? 3 : 0) + (planes->depth ? 1 : 0) + (planes->sun ? 1 : 0) + (planes->albedo ? 3 : 0) +
                        (planes->sky ? 3 : 0) + (planes->beta ? 1 : 0) + (planes->sem_logits ? n_sem : 0) +
                        (planes->sem_class ? 1 : 0);   // 12 + C with every plane of a model without β
    ProfScope prof("composite_products", s, 0.0, P * (n_out * 4.0 + 4.0) + n_rays * 4.0 * per_ray);
    if (n_samples <= 64) return launch_products<1>(v, s);
    if (n_samples <= 128) return launch_products<2>(v, s);
    return launch_products<4>(v, s);
}

extern "C" int64_t spnerf_view_metrics_workspace_bytes(int64_t n_rays, int32_t n_classes) {
    SPN_ARG(n_rays >= 1, "view_metrics_workspace_bytes: n_rays %lld must be positive", (long long)n_rays);
    SPN_ARG(n_classes >= 0 && n_classes <= SPNERF_VIEW_MAX_CLASSES, "view_metrics_workspace_bytes: n_classes %d outside [0, %d]",
            n_classes, SPNERF_VIEW_MAX_CLASSES);
    const size_t nb = (size_t)metric_blocks(n_rays);
    return (int64_t)(align16(nb * sizeof(double)) + align16(nb * (size_t)(n_classes + 1) * n_classes * sizeof(int64_t)));
}

extern "C" int32_t spnerf_view_metrics(int64_t n_rays, const float* rgb, const float* target_rgb, const int32_t* sem_class,
                                       const int64_t* labels, int32_t n_classes, void* workspace,
                                       spnerf_view_metrics_result* result, void* stream) {
    SPN_ARG(rgb && target_rgb && workspace && result, "view_metrics: NULL image, workspace or result");
    SPN_ARG(n_rays >= 1, "view_metrics: n_rays %lld must be positive", (long long)n_rays);
    SPN_ARG(n_classes >= 0 && n_classes <= SPNERF_VIEW_MAX_CLASSES, "view_metrics: n_classes %d outside [0, %d]", n_classes,
            SPNERF_VIEW_MAX_CLASSES);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "view_metrics: workspace not 16-byte aligned");
    SPN_ARG((sem_class != nullptr) == (labels != nullptr), "view_metrics: sem_class and labels go together");
    const int nb = metric_blocks(n_rays);
    MetricArgs m{};
    m.n = n_rays; m.rgb = rgb; m.tgt = target_rgb; m.cls = sem_class; m.lab = labels;
    m.C = sem_class ? n_classes : 0;
    m.sq = (double*)workspace;
    m.tab = (int64_t*)((char*)workspace + align16((size_t)nb * sizeof(double)));
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("view_metrics", s, 0.0, (double)n_rays * (24.0 + (m.C ? 12.0 : 0.0)));
    hipLaunchKernelGGL(k_view_metrics, dim3(nb), dim3(kMetricThreads), 0, s, m);
    SPN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_view_metrics_finish, dim3(1), dim3(kMetricThreads), 0, s, m, nb, result);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
