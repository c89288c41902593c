// LPIPS (AlexNet) of one image pair (include/spnerf_amd_lpips.h).
//
// Activations are NHWC fp32 and hold both images, [2][h][w][C]: row m of a layer's matrix is
// position (image, y, x), so a convolution is C[m][o] = A[m][:] · W[o][:] + b[o] with A the im2col
// gather of its input, and one launch of the fp32 MFMA GEMM (gemm_nt, bias epilogue) serves both
// images.  What the GEMM stores is the value before the ReLU; every reader applies it.
//  * k_lpips_gather1 — conv1's rows from the two caller images through their element strides: the
//    [0, 1] -> [-1, 1] map, the scaling layer and the zero border in one pass; k = (ky 11 + kx) 3 + c,
//    363 columns zero-filled to 384.
//  * k_lpips_gather  — rows of a later convolution: k = (ky ks + kx) C_in + c, so four consecutive
//    k are four consecutive channels of one input position (C_in is a multiple of 4): one 16-byte
//    load, the ReLU, one 16-byte store.  One workgroup per row: the row's position is decoded once.
//  * k_lpips_pool    — max-pool 3 / stride 2 of the ReLU of a tap, four channels per thread.
//  * k_lpips_dist    — one wave per position of a tap: the two images' channel rows (contiguous in
//    NHWC) are read once, the channel norms and the lin-weighted squared difference are summed in
//    fp64 over the wave, and a workgroup writes one fp64 partial sum.  Also the writer of
//    features_out.
//  * k_lpips_finish  — one workgroup adds each tap's partial sums in a fixed order (as
//    k_ssim_finish) and writes the result.
// A NaN survives every stage (the ReLU and the pool keep it), nothing is indexed by data.
// Bands: a convolution whose gather does not fit the workspace runs over consecutive row ranges;
// a value of C depends on its own row of A only and the GEMM adds its K-steps in one order, so the
// bits do not depend on the band size.
#include <algorithm>

#include "../../include/spnerf_amd_lpips.h"
#include "common.h"
#include "gemm_f32.h"

namespace spn {

constexpr int kLpTaps = SPNERF_LPIPS_TAPS;
constexpr int kLpCin[kLpTaps] = {3, 64, 192, 384, 256};
constexpr int kLpCout[kLpTaps] = {64, 192, 384, 256, 256};
constexpr int kLpKs[kLpTaps] = {11, 5, 3, 3, 3};
constexpr int kLpPad[kLpTaps] = {2, 2, 1, 1, 1};
constexpr int kLpK1 = 363, kLpThreads = 256;
constexpr int kLpBandRows = 32;    // band sizes are multiples of this many rows
constexpr int kLpMaxParts = 1024;  // partial sums per tap

constexpr int lp_kp(int l) { return (kLpCin[l] * kLpKs[l] * kLpKs[l] + 31) / 32 * 32; }
// offsets into the packed weights
constexpr int64_t lp_woff(int l) {
    int64_t o = 0;
    for (int j = 0; j < l; ++j) o += (int64_t)kLpCout[j] * (lp_kp(j) + 2);
    return o;
}
constexpr int64_t lp_boff(int l) { return lp_woff(l) + (int64_t)kLpCout[l] * lp_kp(l); }
constexpr int64_t lp_loff(int l) { return lp_boff(l) + kLpCout[l]; }
constexpr int64_t kLpWeightFloats = lp_woff(kLpTaps);
static_assert(lp_kp(0) == 384 && lp_kp(1) == 1600 && lp_kp(2) == 1728 && lp_kp(3) == 3456 && lp_kp(4) == 2304, "K");
static_assert(kLpWeightFloats % 4 == 0, "packed segments stay 16-byte aligned");

// NaN-keeping ReLU (fmaxf would return 0 for a NaN)
__device__ __forceinline__ float lp_relu(float v) { return v < 0.f ? 0.f : v; }
__device__ __forceinline__ f32x4 lp_relu4(f32x4 v) { return f32x4{lp_relu(v[0]), lp_relu(v[1]), lp_relu(v[2]), lp_relu(v[3])}; }
__device__ __forceinline__ float lp_max(float m, float v) { return (v > m || v != v) ? v : m; }

struct LpPackArgs {
    const float* w[kLpTaps];
    const float* b[kLpTaps];
    const float* lin[kLpTaps];
    float* out;
};

__global__ __launch_bounds__(kLpThreads) void k_lpips_pack(LpPackArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * kLpThreads + threadIdx.x; i < kLpWeightFloats; i += (int64_t)gridDim.x * kLpThreads) {
        float v = 0.f;
#pragma unroll
        for (int l = 0; l < kLpTaps; ++l) {
            const int Kp = lp_kp(l), ci = kLpCin[l], ks = kLpKs[l];
            if (i >= lp_woff(l) && i < lp_boff(l)) {
                const int64_t j = i - lp_woff(l);
                const int o = (int)(j / Kp), k = (int)(j - (int64_t)o * Kp);
                if (k < ci * ks * ks) {
                    const int p = k / ci, c = k - p * ci;   // p = ky * ks + kx
                    v = a.w[l][((int64_t)o * ci + c) * ks * ks + p];
                }
            } else if (i >= lp_boff(l) && i < lp_loff(l)) {
                v = a.b[l][i - lp_boff(l)];
            } else if (i >= lp_loff(l) && i < lp_loff(l) + kLpCout[l]) {
                v = a.lin[l][i - lp_loff(l)];
            }
        }
        a.out[i] = v;
    }
}

struct LpGather1Args {
    const float *x, *y;
    float* out;
    int64_t cs, rs, ps, m0;
    int H, W, Ho, Wo, normalize;
};

__global__ __launch_bounds__(kLpThreads) void k_lpips_gather1(LpGather1Args a) {
    const int64_t m = a.m0 + blockIdx.x;
    const int P = a.Ho * a.Wo;
    const int img = (int)(m / P), r = (int)(m - (int64_t)img * P);
    const int oy = r / a.Wo, ox = r - oy * a.Wo;
    const float* src = img ? a.y : a.x;
    float* dst = a.out + (int64_t)blockIdx.x * lp_kp(0);
    for (int k = threadIdx.x; k < lp_kp(0); k += kLpThreads) {
        float v = 0.f;
        if (k < kLpK1) {
            const int p = k / 3, c = k - 3 * p;
            const int ky = p / 11, kx = p - 11 * ky;
            const int iy = oy * 4 - 2 + ky, ix = ox * 4 - 2 + kx;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                float t = src[c * a.cs + iy * a.rs + ix * a.ps];
                if (a.normalize) t = 2.f * t - 1.f;
                const float shift = c == 0 ? -0.030f : c == 1 ? -0.088f : -0.188f;
                const float scale = c == 0 ? 0.458f : c == 1 ? 0.448f : 0.450f;
                v = (t - shift) / scale;
            }
        }
        dst[k] = v;
    }
}

struct LpGatherArgs {
    const float* in;   // [2][Hi][Wi][Cin], before the ReLU
    float* out;        // [rows][Kp]
    int64_t m0;
    int Hi, Wi, Cin, ks, pad, Kp;   // stride 1: the output is Hi x Wi
};

__global__ __launch_bounds__(kLpThreads) void k_lpips_gather(LpGatherArgs a) {
    const int64_t m = a.m0 + blockIdx.x;
    const int P = a.Hi * a.Wi;
    const int img = (int)(m / P), r = (int)(m - (int64_t)img * P);
    const int oy = r / a.Wi, ox = r - oy * a.Wi;
    const float* src = a.in + (int64_t)img * P * a.Cin;
    float* dst = a.out + (int64_t)blockIdx.x * a.Kp;
    for (int k4 = threadIdx.x * 4; k4 < a.Kp; k4 += kLpThreads * 4) {
        const int p = k4 / a.Cin, c = k4 - p * a.Cin;
        const int ky = p / a.ks, kx = p - ky * a.ks;
        const int iy = oy - a.pad + ky, ix = ox - a.pad + kx;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ky < a.ks && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi)
            v = lp_relu4(ld4(src + ((int64_t)iy * a.Wi + ix) * a.Cin + c));
        st4(dst + k4, v);
    }
}

struct LpPoolArgs {
    const float* in;   // [2][Hi][Wi][C], before the ReLU
    float* out;        // [2][Ho][Wo][C], after it
    int64_t n4;        // 2 Ho Wo C / 4
    int Hi, Wi, Ho, Wo, C;
};

__global__ __launch_bounds__(kLpThreads) void k_lpips_pool(LpPoolArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kLpThreads + threadIdx.x;
    if (i >= a.n4) return;
    const int c4n = a.C / 4;
    const int64_t pos = i / c4n;
    const int c = (int)(i - pos * c4n) * 4;
    const int P = a.Ho * a.Wo;
    const int img = (int)(pos / P), r = (int)(pos - (int64_t)img * P);
    const int oy = r / a.Wo, ox = r - oy * a.Wo;
    // the window rows 2 oy .. 2 oy + 2 are inside: Ho = (Hi - 3) / 2 + 1
    const float* src = a.in + (((int64_t)img * a.Hi + 2 * oy) * a.Wi + 2 * ox) * a.C + c;
    f32x4 m = ld4(src);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const f32x4 v = ld4(src + ((int64_t)dy * a.Wi + dx) * a.C);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = lp_max(m[e], v[e]);
        }
    st4(a.out + pos * a.C + c, lp_relu4(m));
}

__device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// f: [2][P][C] before the ReLU; C a multiple of 64 and at most 384
__global__ __launch_bounds__(kLpThreads) void k_lpips_dist(const float* __restrict__ f, const float* __restrict__ lin, int64_t P,
                                                           int C, float* __restrict__ feat, double* __restrict__ part) {
    __shared__ double s_wave[kLpThreads / 64];
    constexpr int J = 6;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t nw = (int64_t)gridDim.x * (kLpThreads / 64);
    float w[J];
#pragma unroll
    for (int j = 0; j < J; ++j) w[j] = 64 * j < C ? lin[64 * j + lane] : 0.f;
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * (kLpThreads / 64) + wid; p < P; p += nw) {   // wave-uniform
        const float* a = f + p * C;
        const float* b = f + (P + p) * C;
        float va[J], vb[J];
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            va[j] = vb[j] = 0.f;
            if (64 * j < C) {
                va[j] = lp_relu(a[64 * j + lane]);
                vb[j] = lp_relu(b[64 * j + lane]);
                if (feat) {
                    feat[p * C + 64 * j + lane] = va[j];
                    feat[(P + p) * C + 64 * j + lane] = vb[j];
                }
                sa += (double)va[j] * (double)va[j];
                sb += (double)vb[j] * (double)vb[j];
            }
        }
        const double na = sqrt(lp_wave_sum(sa)) + 1e-10, nb = sqrt(lp_wave_sum(sb)) + 1e-10;
        double d = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const double t = (double)va[j] / na - (double)vb[j] / nb;
            d += (double)w[j] * (t * t);
        }
        acc += lp_wave_sum(d);
    }
    if (lane == 0) s_wave[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < kLpThreads / 64; ++i) t += s_wave[i];
        part[blockIdx.x] = t;
    }
}

struct LpFinishArgs {
    const double* part;   // [taps][kLpMaxParts]
    int nparts[kLpTaps];
    int h[kLpTaps], w[kLpTaps];
    spnerf_lpips_result* res;
};

__global__ __launch_bounds__(kLpThreads) void k_lpips_finish(LpFinishArgs a) {
    __shared__ double s[kLpThreads];
    __shared__ double s_l[kLpTaps];
    const int tid = threadIdx.x;
    for (int l = 0; l < kLpTaps; ++l) {
        double t = 0.0;
        for (int i = tid; i < a.nparts[l]; i += kLpThreads) t += a.part[l * kLpMaxParts + i];
        s[tid] = t;
        __syncthreads();
        for (int off = kLpThreads / 2; off > 0; off >>= 1) {
            if (tid < off) s[tid] += s[tid + off];
            __syncthreads();
        }
        if (tid == 0) s_l[l] = s[0] / ((double)a.h[l] * (double)a.w[l]);
        __syncthreads();
    }
    if (tid == 0) {
        double t = 0.0;
        for (int l = 0; l < kLpTaps; ++l) {
            t += s_l[l];
            a.res->layer[l] = s_l[l];
            a.res->h[l] = a.h[l];
            a.res->w[l] = a.w[l];
        }
        a.res->lpips = t;
    }
}

// sizes of everything for one image size, in floats
struct LpPlan {
    int h[kLpTaps], w[kLpTaps];
    int hp[2], wp[2];                 // the two pooled maps
    int64_t M[kLpTaps];               // rows of each convolution: 2 h w
    int64_t act[kLpTaps], pool[2];    // offsets of the activations
    int64_t part, band;               // offsets of the partial sums and of the gather band
    int64_t band_min, band_full;      // floats of the smallest band and of the largest whole gather
    int64_t feat[kLpTaps + 1];        // offsets into features_out
};

static int32_t lp_plan(const char* who, int32_t H, int32_t W, LpPlan* p) {
    SPN_ARG(H >= SPNERF_LPIPS_MIN_SIDE && W >= SPNERF_LPIPS_MIN_SIDE, "%s: image %d x %d smaller than %d on a side", who, H, W,
            SPNERF_LPIPS_MIN_SIDE);
    SPN_ARG(H <= SPNERF_LPIPS_MAX_SIDE && W <= SPNERF_LPIPS_MAX_SIDE, "%s: image %d x %d larger than %d on a side", who, H, W,
            SPNERF_LPIPS_MAX_SIDE);
    p->h[0] = (H + 4 - 11) / 4 + 1;
    p->w[0] = (W + 4 - 11) / 4 + 1;
    p->hp[0] = (p->h[0] - 3) / 2 + 1;
    p->wp[0] = (p->w[0] - 3) / 2 + 1;
    p->h[1] = p->hp[0];
    p->w[1] = p->wp[0];
    p->hp[1] = (p->h[1] - 3) / 2 + 1;
    p->wp[1] = (p->w[1] - 3) / 2 + 1;
    for (int l = 2; l < kLpTaps; ++l) {
        p->h[l] = p->hp[1];
        p->w[l] = p->wp[1];
    }
    int64_t o = 0;
    p->band_min = p->band_full = 0;
    p->feat[0] = 0;
    for (int l = 0; l < kLpTaps; ++l) {
        p->M[l] = 2 * (int64_t)p->h[l] * p->w[l];
        p->act[l] = o;
        o += p->M[l] * kLpCout[l];
        p->feat[l + 1] = p->feat[l] + p->M[l] * kLpCout[l];
        if (l < 2) {
            p->pool[l] = o;
            o += 2 * (int64_t)p->hp[l] * p->wp[l] * kLpCout[l];
        }
        p->band_min = std::max(p->band_min, std::min<int64_t>(p->M[l], kLpBandRows) * lp_kp(l));
        p->band_full = std::max(p->band_full, p->M[l] * lp_kp(l));
    }
    p->part = o;
    o += (int64_t)kLpTaps * kLpMaxParts * 2;   // doubles
    p->band = o;
    return SPNERF_OK;
}

// rows of convolution l per band when the band holds `band_floats`
static int64_t lp_band_rows(const LpPlan& p, int l, int64_t band_floats) {
    const int64_t fit = band_floats / lp_kp(l);
    return fit >= p.M[l] ? p.M[l] : fit / kLpBandRows * kLpBandRows;
}

static int32_t lp_conv(const LpPlan& p, int l, const float* in, float* act, float* band,
                       int64_t band_floats, const float* wts, const LpGather1Args& g1, hipStream_t s) {
    const int64_t step = lp_band_rows(p, l, band_floats);
    const int Kp = lp_kp(l);
    for (int64_t m0 = 0; m0 < p.M[l]; m0 += step) {
        const int64_t rows = std::min(step, p.M[l] - m0);
        if (l == 0) {
            LpGather1Args g = g1;
            g.out = band;
            g.m0 = m0;
            hipLaunchKernelGGL(k_lpips_gather1, dim3((unsigned)rows), dim3(kLpThreads), 0, s, g);
        } else {
            LpGatherArgs g{};
            g.in = in; g.out = band; g.m0 = m0;
            g.Hi = p.h[l]; g.Wi = p.w[l]; g.Cin = kLpCin[l]; g.ks = kLpKs[l]; g.pad = kLpPad[l]; g.Kp = Kp;
            hipLaunchKernelGGL(k_lpips_gather, dim3((unsigned)rows), dim3(kLpThreads), 0, s, g);
        }
        SPN_HIP(hipGetLastError());
        NTArgs nt;
        nt.A = band; nt.lda = Kp; nt.K1 = Kp;
        nt.B = wts + lp_woff(l); nt.ldb = Kp;
        nt.C = act + m0 * kLpCout[l]; nt.ldc = kLpCout[l];
        nt.M = (int)rows; nt.N = kLpCout[l]; nt.K = Kp;
        nt.bias = wts + lp_boff(l);
        SPN_TRY(gemm_nt(nt, s));
    }
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_lpips_abi_version(void) { return SPNERF_LPIPS_ABI_VERSION; }

extern "C" int64_t spnerf_lpips_weights_floats(void) { return kLpWeightFloats; }

extern "C" int32_t spnerf_lpips_pack_weights(const float* const* conv_w, const float* const* conv_b, const float* const* lin,
                                             float* packed, void* stream) {
    SPN_ARG(conv_w && conv_b && lin && packed, "lpips_pack_weights: NULL argument");
    SPN_ARG(((uintptr_t)packed & 15) == 0, "lpips_pack_weights: packed buffer not 16-byte aligned");
    LpPackArgs a{};
    for (int l = 0; l < kLpTaps; ++l) {
        SPN_ARG(conv_w[l] && conv_b[l] && lin[l], "lpips_pack_weights: NULL weights of tap %d", l);
        a.w[l] = conv_w[l]; a.b[l] = conv_b[l]; a.lin[l] = lin[l];
    }
    a.out = packed;
    hipLaunchKernelGGL(k_lpips_pack, dim3(1024), dim3(kLpThreads), 0, (hipStream_t)stream, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int64_t spnerf_lpips_workspace_bytes(int32_t H, int32_t W, int64_t max_bytes) {
    LpPlan p;
    SPN_TRY(lp_plan("lpips_workspace_bytes", H, W, &p));
    const int64_t full = (p.band + p.band_full) * 4, least = (p.band + p.band_min) * 4;
    if (max_bytes <= 0 || max_bytes >= full) return full;
    return std::max(least, max_bytes & ~(int64_t)15);
}

extern "C" int32_t spnerf_lpips_bands(int32_t H, int32_t W, int64_t workspace_bytes, int32_t* bands) {
    LpPlan p;
    SPN_TRY(lp_plan("lpips_bands", H, W, &p));
    SPN_ARG(bands, "lpips_bands: NULL output");
    const int64_t band_floats = workspace_bytes / 4 - p.band;
    SPN_ARG(band_floats >= p.band_min, "lpips_bands: workspace of %lld bytes too small, %d x %d needs %lld",
            (long long)workspace_bytes, H, W, (long long)((p.band + p.band_min) * 4));
    for (int l = 0; l < kLpTaps; ++l) bands[l] = cdiv(p.M[l], lp_band_rows(p, l, band_floats));
    return SPNERF_OK;
}

extern "C" int64_t spnerf_lpips_features_floats(int32_t H, int32_t W) {
    LpPlan p;
    SPN_TRY(lp_plan("lpips_features_floats", H, W, &p));
    return p.feat[kLpTaps];
}

extern "C" int32_t spnerf_lpips(const float* x, const float* y, int32_t H, int32_t W, int64_t channel_stride, int64_t row_stride,
                                int64_t pixel_stride, int32_t normalize, const float* packed_weights, void* workspace,
                                int64_t workspace_bytes, float* features_out, spnerf_lpips_result* result, void* stream) {
    SPN_ARG(x && y, "lpips: NULL image");
    SPN_ARG(packed_weights && workspace && result, "lpips: NULL weights, workspace or result");
    LpPlan p;
    SPN_TRY(lp_plan("lpips", H, W, &p));
    SPN_ARG(channel_stride >= 0 && row_stride >= 0 && pixel_stride >= 0, "lpips: negative stride (%lld, %lld, %lld)",
            (long long)channel_stride, (long long)row_stride, (long long)pixel_stride);
    SPN_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)packed_weights & 15) == 0,
            "lpips: workspace or weights not 16-byte aligned");
    SPN_ARG(((uintptr_t)result & 7) == 0 && ((uintptr_t)features_out & 3) == 0, "lpips: result not 8-byte aligned");
    const int64_t band_floats = workspace_bytes / 4 - p.band;
    SPN_ARG(band_floats >= p.band_min, "lpips: workspace of %lld bytes too small, %d x %d needs %lld", (long long)workspace_bytes, H,
            W, (long long)((p.band + p.band_min) * 4));
    hipStream_t s = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* band = ws + p.band;
    double* part = (double*)(ws + p.part);
    LpGather1Args g1{};
    g1.x = x; g1.y = y;
    g1.cs = channel_stride; g1.rs = row_stride; g1.ps = pixel_stride;
    g1.H = H; g1.W = W; g1.Ho = p.h[0]; g1.Wo = p.w[0]; g1.normalize = normalize != 0;
    for (int l = 0; l < kLpTaps; ++l) {
        // the input of convolution l: the pooled tap for 1 and 2, the tap itself after that
        const float* in = l == 0 ? nullptr : l <= 2 ? ws + p.pool[l - 1] : ws + p.act[l - 1];
        SPN_TRY(lp_conv(p, l, in,ws + p.act[l], band, band_floats, packed_weights, g1, s));
        if (l < 2) {
            LpPoolArgs a{};
            a.in = ws + p.act[l]; a.out = ws + p.pool[l];
            a.Hi = p.h[l]; a.Wi = p.w[l]; a.Ho = p.hp[l]; a.Wo = p.wp[l]; a.C = kLpCout[l];
            a.n4 = 2 * (int64_t)a.Ho * a.Wo * a.C / 4;
            hipLaunchKernelGGL(k_lpips_pool, dim3((unsigned)cdiv(a.n4, kLpThreads)), dim3(kLpThreads), 0, s, a);
            SPN_HIP(hipGetLastError());
        }
    }
    LpFinishArgs f{};
    f.part = part;
    f.res = result;
    for (int l = 0; l < kLpTaps; ++l) {
        const int64_t P = p.M[l] / 2;
        f.nparts[l] = (int)std::min<int64_t>(cdiv(P, kLpThreads / 64), kLpMaxParts);
        f.h[l] = p.h[l];
        f.w[l] = p.w[l];
        hipLaunchKernelGGL(k_lpips_dist, dim3((unsigned)f.nparts[l]), dim3(kLpThreads), 0, s, (const float*)(ws + p.act[l]),
                           packed_weights + lp_loff(l), P, kLpCout[l], features_out ? features_out + p.feat[l] : nullptr,
                           part + (int64_t)l * kLpMaxParts);
        SPN_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lpips_finish, dim3(1), dim3(kLpThreads), 0, s, f);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
