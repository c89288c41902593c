// Training-set tensors on gfx950 (include/spnerf_amd_data.h) — the arithmetic of the reference's
// datasets/satellite_scene.py load_depth_data (:241-279), init_scaling_params (:397-406) and
// load_semantic_data (:316-375); the file reading there stays with the caller.
//
// One thread per keypoint / pixel, fp64 localisation from csrc/rpc.h, everything after the fp32
// cast in the reference's fp32 sequence.  Minima and maxima are reduced inside the wave first; the
// correl range of an image goes through per-block partials that the scatter kernel reduces again
// (it needs the range before it can write anything), the depth range and the scene bounds are
// folded into their in/out buffers with one integer atomic min / max per wave and value.
#include "../../include/spnerf_amd_data.h"
#include "rpc.h"
#include "wave.h"

namespace spn {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPartials = 256;  // blocks of k_correl_range; 2 floats each in the workspace
static_assert(kMaxPartials <= kBlock && kMaxPartials * 2 * sizeof(float) <= SPNERF_DATA_WORKSPACE_BYTES, "workspace");

// a * x + b with two roundings, as torch evaluates `s * (1 - w) + m` and `o + far * d` (hipcc
// contracts a * x + b into one fused multiply-add by default, and its __fmul_rn / __fadd_rn are
// plain operators)
__device__ __forceinline__ float mul_then_add(float a, float x, float b) {
#pragma clang fp contract(off)
    const float p = a * x;
    return p + b;
}

// min / max that keep a NaN, like torch.min / torch.max
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ float wave_nan_min(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = nan_min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_nan_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_xor(v, off, 64));
    return v;
}

// (min, max) over the block, in every thread
__device__ __forceinline__ void block_range(float& lo, float& hi) {
    __shared__ float s_lo[kWaves], s_hi[kWaves];
    lo = wave_nan_min(lo);
    hi = wave_nan_max(hi);
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    lo = s_lo[0];
    hi = s_hi[0];
    for (int w = 1; w < kWaves; ++w) {
        lo = nan_min(lo, s_lo[w]);
        hi = nan_max(hi, s_hi[w]);
    }
}

// Float min / max on global memory with the integer atomics: floats of one sign order like their
// bit patterns (reversed when negative), and a positive pattern is the larger signed integer.
// v + 0 turns -0 into +0; a NaN never enters (callers fold finite values).
__device__ __forceinline__ void atomic_min_f32(float* p, float v) {
    v += 0.0f;
    if (v >= 0.f)
        atomicMin(reinterpret_cast<int*>(p), __float_as_int(v));
    else
        atomicMax(reinterpret_cast<unsigned int*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_f32(float* p, float v) {
    v += 0.0f;
    if (v >= 0.f)
        atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
    else
        atomicMin(reinterpret_cast<unsigned int*>(p), __float_as_uint(v));
}

// ---- depth priors ---------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_correl_range(const float* __restrict__ correl, int64_t K,
                                                         float* __restrict__ partials) {
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < K; i += (int64_t)gridDim.x * kBlock) {
        const float c = correl[i];
        lo = nan_min(c, lo);
        hi = nan_max(c, hi);
    }
    block_range(lo, hi);
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = lo;
        partials[2 * blockIdx.x + 1] = hi;
    }
}

struct DepthArgs {
    RpcCam cam;
    int height, width;
    float center[3], range, stdscale, margin;
    const double* pix;
    const float* pts3d;
    const float* correl;
    int64_t K;
    const float* partials;
    int n_partials;
    float *deprays, *depths, *valid, *std, *depth_range;
};

__global__ __launch_bounds__(kBlock) void k_depth_priors(DepthArgs a) {
    // the image's correl range from the partials of k_correl_range (at most one per thread)
    float cmin = INFINITY, cmax = -INFINITY;
    if ((int)threadIdx.x < a.n_partials) {
        cmin = a.partials[2 * threadIdx.x];
        cmax = a.partials[2 * threadIdx.x + 1];
    }
    block_range(cmin, cmax);

    const int64_t k = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    float dlo = INFINITY, dhi = -INFINITY;
    if (k < a.K) {
        const double col = a.pix[2 * k], row = a.pix[2 * k + 1];
        float v[8];
        rpc_ray(a.cam, col, row, v);
        normalize_ray(v, a.center, a.range);
        float d[3];
        for (int j = 0; j < 3; ++j)
            d[j] = __fsub_rn(__fdiv_rn(__fsub_rn(a.pts3d[3 * k + j], a.center[j]), a.range), v[j]);
        const float depth = sqrtf(fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0])));
        const float w = __fdiv_rn(__fsub_rn(a.correl[k], cmin), __fsub_rn(cmax, cmin));
        const float sd = mul_then_add(a.stdscale, __fsub_rn(1.0f, w), a.margin);
        const int64_t c = (int64_t)col, r = (int64_t)row;
        if (c >= 0 && c < a.width && r >= 0 && r < a.height) {  // never scatter outside the planes
            const int64_t q = r * a.width + c;
            float* o = a.deprays + q * 8;
            for (int j = 0; j < 8; ++j) o[j] = v[j];
            a.depths[2 * q] = depth;
            a.depths[2 * q + 1] = w;
            a.valid[q] = 1.0f;
            a.std[q] = sd;
            if (depth == depth) dlo = dhi = depth;
        }
    }
    dlo = wave_nan_min(dlo);
    dhi = wave_nan_max(dhi);
    if ((threadIdx.x & 63) == 0 && dlo <= dhi) {
        atomic_min_f32(a.depth_range, dlo);
        atomic_max_f32(a.depth_range + 1, dhi);
    }
}

// ---- scene bounds ---------------------------------------------------------------------------

struct BoundsArgs {
    RpcCam cam;
    int ncols;
    int64_t n;
    float* bounds;
};

__global__ __launch_bounds__(kBlock) void k_scene_bounds(BoundsArgs a) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < a.n) {
        float v[8];
        rpc_ray(a.cam, (double)(i % a.ncols), (double)(i / a.ncols), v);
        for (int j = 0; j < 3; ++j) {
            const float f = mul_then_add(v[7], v[3 + j], v[j]);  // far_pt = o + far * d
            lo[j] = fminf(v[j], f);
            hi[j] = fmaxf(v[j], f);
        }
    }
    for (int j = 0; j < 3; ++j) {
        lo[j] = wave_nan_min(lo[j]);
        hi[j] = wave_nan_max(hi[j]);
    }
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < 3; ++j)
            if (lo[j] <= hi[j]) {
                atomic_min_f32(a.bounds + j, lo[j]);
                atomic_max_f32(a.bounds + 3 + j, hi[j]);
            }
}

// ---- semantic labels ------------------------------------------------------------------------

struct SemArgs {
    const uint8_t* r8;
    const int32_t* r32;
    const int32_t* lut;
    int Hs, Ws, Hd, Wd, height, width, sd, dense;
    // fp32 scales in / out of F.interpolate(mode='nearest'), formed on the host:
    // source → target rows / cols (sparse), source → downsampled and downsampled → target (dense)
    float s_row, s_col, d_row, d_col, u_row, u_col;
    int64_t* labels;
    float* valid;
};

__device__ __forceinline__ int nearest_src(int dst, float scale, int n_in) {
    const int s = (int)floorf(__fmul_rn((float)dst, scale));
    return s < n_in - 1 ? s : n_in - 1;
}

__global__ __launch_bounds__(kBlock) void k_semantic_labels(SemArgs a) {
    const int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x;
    if (i >= (int64_t)a.height * a.width) return;
    const int r = (int)(i / a.width), c = (int)(i % a.width);
    int sr, sc;
    if (a.dense) {
        sr = nearest_src(nearest_src(r, a.u_row, a.Hd), a.d_row, a.Hs);
        sc = nearest_src(nearest_src(c, a.u_col, a.Wd), a.d_col, a.Ws);
    } else {
        sr = nearest_src(r, a.s_row, a.Hs);
        sc = nearest_src(c, a.s_col, a.Ws);
    }
    const int64_t at = (int64_t)sr * a.Ws + sc;
    const int code = a.r8 ? (int)a.r8[at] : a.r32[at];
    int label = (code >= 0 && code < 256) ? a.lut[code] : SPNERF_DATA_VOID_LABEL;
    bool on = label != SPNERF_DATA_VOID_LABEL;
    if (!a.dense) {
        on = on && r % a.sd == 0 && c % a.sd == 0;
        if (!on) label = SPNERF_DATA_VOID_LABEL;
    }
    a.labels[i] = label;
    a.valid[i] = on ? 1.0f : 0.0f;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_data_abi_version(void) { return SPNERF_DATA_ABI_VERSION; }

extern "C" int32_t spnerf_depth_priors(const double* rpc, double min_alt, double max_alt, int32_t height, int32_t width,
                                       const float* center, float range, const double* pixels, const float* pts3d,
                                       const float* correl, int64_t K, float stdscale, float margin, float* deprays,
                                       float* depths, float* valid_depth, float* depth_std, float* depth_range,
                                       void* workspace, void* stream) {
    SPN_ARG(rpc && center && pixels && pts3d && correl, "depth_priors: NULL input");
    SPN_ARG(deprays && depths && valid_depth && depth_std && depth_range && workspace, "depth_priors: NULL output");
    SPN_ARG(height > 0 && width > 0, "depth_priors: bad image size %d x %d", height, width);
    SPN_ARG(K >= 1, "depth_priors: K = %lld keypoints (the correl range of no keypoint is undefined)", (long long)K);
    SPN_ARG(K <= (int64_t)height * width, "depth_priors: %lld keypoints on %d x %d pixels cannot be distinct",
            (long long)K, height, width);
    SPN_ARG(range > 0, "depth_priors: bad range");
    hipStream_t s = (hipStream_t)stream;
    const int64_t hw = (int64_t)height * width;
    DepthArgs a{};
    rpc_unpack(a.cam, rpc, 1.0, min_alt, max_alt);
    a.height = height;
    a.width = width;
    for (int k = 0; k < 3; ++k) a.center[k] = center[k];
    a.range = range;
    a.stdscale = stdscale;
    a.margin = margin;
    a.pix = pixels;
    a.pts3d = pts3d;
    a.correl = correl;
    a.K = K;
    a.partials = (const float*)workspace;
    const int64_t blocks = (K + kBlock - 1) / kBlock;
    a.n_partials = (int)(blocks < kMaxPartials ? blocks : kMaxPartials);
    a.deprays = deprays;
    a.depths = depths;
    a.valid = valid_depth;
    a.std = depth_std;
    a.depth_range = depth_range;
    ProfScope prof("depth_priors", s, 0.0, 4.0 * 12 * hw + 32.0 * K);
    SPN_HIP(hipMemsetAsync(deprays, 0, sizeof(float) * 8 * hw, s));
    SPN_HIP(hipMemsetAsync(depths, 0, sizeof(float) * 2 * hw, s));
    SPN_HIP(hipMemsetAsync(valid_depth, 0, sizeof(float) * hw, s));
    SPN_HIP(hipMemsetAsync(depth_std, 0, sizeof(float) * hw, s));
    hipLaunchKernelGGL(k_correl_range, dim3(a.n_partials), dim3(kBlock), 0, s, correl, K, (float*)workspace);
    SPN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_depth_priors, dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_scene_bounds(const double* rpc, double downscale, double min_alt, double max_alt,
                                       int32_t n_rows, int32_t n_cols, float* bounds, void* stream) {
    SPN_ARG(rpc && bounds, "scene_bounds: NULL pointer");
    SPN_ARG(downscale > 0, "scene_bounds: bad downscale");
    SPN_ARG(n_rows >= 0 && n_cols >= 0, "scene_bounds: bad rectangle %d x %d", n_rows, n_cols);
    BoundsArgs a{};
    rpc_unpack(a.cam, rpc, downscale, min_alt, max_alt);
    a.ncols = n_cols;
    a.n = (int64_t)n_rows * n_cols;
    a.bounds = bounds;
    if (a.n == 0) return SPNERF_OK;
    ProfScope prof("scene_bounds", (hipStream_t)stream, 0.0, 0.0);
    hipLaunchKernelGGL(k_scene_bounds, dim3((unsigned)((a.n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_semantic_labels(const void* raster, int32_t raster_is_i32, int32_t Hs, int32_t Ws,
                                          const int32_t* lut, int32_t height, int32_t width, int32_t sem_downscale,
                                          int32_t dense, int64_t* labels, float* valid, void* stream) {
    SPN_ARG(raster && lut && labels && valid, "semantic_labels: NULL pointer");
    SPN_ARG(Hs > 0 && Ws > 0 && height > 0 && width > 0, "semantic_labels: bad size (%d x %d) -> (%d x %d)", Hs, Ws,
            height, width);
    SPN_ARG(sem_downscale >= 1, "semantic_labels: bad sem_downscale %d", sem_downscale);
    SemArgs a{};
    a.r8 = raster_is_i32 ? nullptr : (const uint8_t*)raster;
    a.r32 = raster_is_i32 ? (const int32_t*)raster : nullptr;
    a.lut = lut;
    a.Hs = Hs;
    a.Ws = Ws;
    a.Hd = Hs / sem_downscale;
    a.Wd = Ws / sem_downscale;
    SPN_ARG(!dense || (a.Hd >= 1 && a.Wd >= 1), "semantic_labels: a %d x %d raster has no 1/%d downsampling", Hs, Ws,
            sem_downscale);
    a.height = height;
    a.width = width;
    a.sd = sem_downscale;
    a.dense = dense != 0;
    a.s_row = (float)Hs / (float)height;
    a.s_col = (float)Ws / (float)width;
    if (a.dense) {
        a.d_row = (float)Hs / (float)a.Hd;
        a.d_col = (float)Ws / (float)a.Wd;
        a.u_row = (float)a.Hd / (float)height;
        a.u_col = (float)a.Wd / (float)width;
    }
    a.labels = labels;
    a.valid = valid;
    const int64_t n = (int64_t)height * width;
    ProfScope prof("semantic_labels", (hipStream_t)stream, 0.0, 12.0 * n);
    hipLaunchKernelGGL(k_semantic_labels, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
