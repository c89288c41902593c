// Structural similarity of two fp32 images in fp64 (include/spnerf_amd_image.h).
//
//  * k_ssim_tiles<R> — one 256-thread workgroup per 16 x 32 output tile per channel.  The tile and
//    its halo of R = ws / 2 values of both images go into LDS through the mirrored index (torch's
//    'reflect': no edge value repeated), addressed by element strides, so planar CHW, interleaved
//    HWC and padded rows are one code path.  The horizontal Gaussian pass over x, y, x², y², xy
//    writes five fp64 planes [16 + 2R][32] to LDS (the products of two fp32 values are exact in
//    fp64); the vertical pass, the map and the tile's sum follow in fp64.  Both LDS images are
//    read along a row by consecutive lanes: 32 consecutive floats (ds_read_b32, 32 banks) in the
//    horizontal pass, 32 consecutive doubles = one 256-B bank row (ds_read_b64, 64 banks) in the
//    vertical one, so neither needs padding.  LDS is sized by R at launch: 27.3 KiB at ws 3,
//    41.0 KiB at ws 11.
//  * k_ssim_finish — one workgroup: per channel, thread t adds the tile sums t, t + 256, … in that
//    order, a fixed tree adds the 256 totals, thread 0 adds the channels in order and writes the
//    result.  Fixed grid, fixed order, no atomics: two calls give the same bits.
#include <cmath>

#include "../../include/spnerf_amd_image.h"
#include "common.h"

namespace spn {

constexpr int kSsimTH = 16, kSsimTW = 32, kSsimThreads = 256;
constexpr int kSsimMaxSide = kSsimTH * 65535;   // grid.y and grid.z hold 65535 workgroups

struct SsimArgs {
    const float *x, *y;
    double* map;    // NULL, or [C][H][W]
    double* part;   // [C][tiles_y][tiles_x]
    int64_t cs, rs, ps;
    int H, W, R;
    double c1, c2;
    double g[SPNERF_IMAGE_MAX_WINDOW];   // the normalised 1-D window, ws entries
};

// index i of a row of n values mirrored about its ends, for i in [-R, n - 1 + R] with R < n; the
// clamp keeps the halo of a partial tile (indices past n - 1 + R, read by no valid output) inside
// the image
__device__ __forceinline__ int mirror(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ double ssim_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int R>
__global__ __launch_bounds__(kSsimThreads) void k_ssim_tiles(SsimArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sh_h[];
    __shared__ double s_wave[kSsimThreads / 64];
    constexpr int WS = 2 * R + 1, SH = kSsimTH + 2 * R, SW = kSsimTW + 2 * R, PL = SH * kSsimTW;
    double* hq = sh_h;                                      // [5][SH][TW]
    float* xs = reinterpret_cast<float*>(hq + 5 * PL);      // [SH][SW]
    float* ys = xs + SH * SW;
    const int tid = threadIdx.x, c = blockIdx.z;
    const int x0 = blockIdx.x * kSsimTW, y0 = blockIdx.y * kSsimTH;
    const float* px = a.x + c * a.cs;
    const float* py = a.y + c * a.cs;
    for (int i = tid; i < SH * SW; i += kSsimThreads) {
        const int sy = i / SW, sx = i - sy * SW;
        const int64_t off = (int64_t)mirror(y0 - R + sy, a.H) * a.rs + (int64_t)mirror(x0 - R + sx, a.W) * a.ps;
        xs[i] = px[off];
        ys[i] = py[off];
    }
    __syncthreads();
    for (int i = tid; i < PL; i += kSsimThreads) {          // horizontal pass
        const int sy = i / kSsimTW, x = i % kSsimTW;
        const float* xr = xs + sy * SW + x;
        const float* yr = ys + sy * SW + x;
        double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < WS; ++k) {
            const double u = (double)xr[k], v = (double)yr[k], w = a.g[k];
            h[0] += w * u;
            h[1] += w * v;
            h[2] += w * (u * u);
            h[3] += w * (v * v);
            h[4] += w * (u * v);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hq[q * PL + i] = h[q];
    }
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < kSsimTH * kSsimTW / kSsimThreads; ++j) {   // vertical pass and the map
        const int i = tid + j * kSsimThreads;
        const int ty = i / kSsimTW, x = i % kSsimTW;
        const int gy = y0 + ty, gx = x0 + x;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < WS; ++k) {
            const double w = a.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += w * hq[q * PL + (ty + k) * kSsimTW + x];
        }
        const double mu1 = m[0], mu2 = m[1];
        const double s1 = m[2] - mu1 * mu1, s2 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
        const double num = (2.0 * mu1 * mu2 + a.c1) * (2.0 * s12 + a.c2);
        const double den = (mu1 * mu1 + mu2 * mu2 + a.c1) * (s1 + s2 + a.c2) + 1e-12;
        const double val = num / den;
        if (gy < a.H && gx < a.W) {
            sum += val;
            if (a.map) a.map[((int64_t)c * a.H + gy) * a.W + gx] = val;
        }
    }
    sum = ssim_wave_sum(sum);
    if ((tid & 63) == 0) s_wave[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < kSsimThreads / 64; ++w) t += s_wave[w];
        a.part[((int64_t)c * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(kSsimThreads) void k_ssim_finish(const double* part, int C, int64_t tiles, int64_t hw,
                                                              spnerf_image_ssim_result* res) {
    __shared__ double s[kSsimThreads];
    __shared__ double s_ch[SPNERF_IMAGE_MAX_CHANNELS];
    const int tid = threadIdx.x;
    for (int c = 0; c < C; ++c) {
        double t = 0.0;
        for (int64_t i = tid; i < tiles; i += kSsimThreads) t += part[c * tiles + i];
        s[tid] = t;
        __syncthreads();
        for (int off = kSsimThreads / 2; off > 0; off >>= 1) {
            if (tid < off) s[tid] += s[tid + off];
            __syncthreads();
        }
        if (tid == 0) s_ch[c] = s[0];
        __syncthreads();
    }
    if (tid == 0) {
        double t = 0.0;
        for (int c = 0; c < SPNERF_IMAGE_MAX_CHANNELS; ++c) {
            if (c < C) t += s_ch[c];
            res->channel_mean[c] = c < C ? s_ch[c] / (double)hw : 0.0;
        }
        res->ssim = t / (double)(C * hw);
        res->n = C * hw;
    }
}

template <int R>
static int32_t launch_ssim(const SsimArgs& a, dim3 grid, hipStream_t s) {
    constexpr int SH = kSsimTH + 2 * R, SW = kSsimTW + 2 * R;
    constexpr size_t lds = (size_t)5 * SH * kSsimTW * sizeof(double) + (size_t)2 * SH * SW * sizeof(float);
    hipLaunchKernelGGL(k_ssim_tiles<R>, grid, dim3(kSsimThreads), lds, s, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

// the checks the two exports share
static int32_t ssim_shape(const char* who, int32_t C, int32_t H, int32_t W, int32_t ws) {
    SPN_ARG(ws >= 3 && ws <= SPNERF_IMAGE_MAX_WINDOW && (ws & 1), "%s: window size %d must be odd and in [3, %d]", who, ws,
            SPNERF_IMAGE_MAX_WINDOW);
    SPN_ARG(C >= 1 && C <= SPNERF_IMAGE_MAX_CHANNELS, "%s: %d channels outside [1, %d]", who, C, SPNERF_IMAGE_MAX_CHANNELS);
    SPN_ARG(H >= 0 && W >= 0, "%s: image size %d x %d is negative", who, H, W);
    SPN_ARG(H > ws / 2 && W > ws / 2, "%s: image %d x %d too small for a mirrored border of %d", who, H, W, ws / 2);
    SPN_ARG(H <= kSsimMaxSide && W <= kSsimMaxSide, "%s: image %d x %d larger than %d on a side", who, H, W, kSsimMaxSide);
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_image_abi_version(void) { return SPNERF_IMAGE_ABI_VERSION; }

extern "C" int64_t spnerf_image_ssim_workspace_bytes(int32_t C, int32_t H, int32_t W, int32_t ws) {
    SPN_TRY(ssim_shape("image_ssim_workspace_bytes", C, H, W, ws));
    const size_t tiles = (size_t)cdiv(H, kSsimTH) * cdiv(W, kSsimTW);
    return (int64_t)((C * tiles * sizeof(double) + 15) & ~(size_t)15);
}

extern "C" int32_t spnerf_image_ssim(const float* x, const float* y, int32_t C, int32_t H, int32_t W, int64_t channel_stride,
                                     int64_t row_stride, int64_t pixel_stride, int32_t ws, double max_val, void* workspace,
                                     double* map, spnerf_image_ssim_result* result, void* stream) {
    SPN_ARG(x && y, "image_ssim: NULL image");
    SPN_ARG(workspace && result, "image_ssim: NULL workspace or result");
    SPN_TRY(ssim_shape("image_ssim", C, H, W, ws));
    SPN_ARG(channel_stride >= 0 && row_stride >= 0 && pixel_stride >= 0, "image_ssim: negative stride (%lld, %lld, %lld)",
            (long long)channel_stride, (long long)row_stride, (long long)pixel_stride);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "image_ssim: workspace not 16-byte aligned");
    SPN_ARG(((uintptr_t)result & 7) == 0 && ((uintptr_t)map & 7) == 0, "image_ssim: result or map not 8-byte aligned");
    SsimArgs a{};
    a.x = x; a.y = y; a.map = map; a.part = (double*)workspace;
    a.cs = channel_stride; a.rs = row_stride; a.ps = pixel_stride;
    a.H = H; a.W = W; a.R = ws / 2;
    a.c1 = (0.01 * max_val) * (0.01 * max_val);
    a.c2 = (0.03 * max_val) * (0.03 * max_val);
    double total = 0.0;
    for (int i = 0; i < ws; ++i) {
        const double d = (double)(i - ws / 2);
        a.g[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        total += a.g[i];
    }
    for (int i = 0; i < ws; ++i) a.g[i] /= total;
    const dim3 grid((unsigned)cdiv(W, kSsimTW), (unsigned)cdiv(H, kSsimTH), (unsigned)C);
    hipStream_t s = (hipStream_t)stream;
    const double values = (double)C * H * W;
    ProfScope prof("image_ssim", s, 0.0, values * (8.0 + (map ? 8.0 : 0.0)));
    switch (ws / 2) {
        case 1: SPN_TRY(launch_ssim<1>(a, grid, s)); break;
        case 2: SPN_TRY(launch_ssim<2>(a, grid, s)); break;
        case 3: SPN_TRY(launch_ssim<3>(a, grid, s)); break;
        case 4: SPN_TRY(launch_ssim<4>(a, grid, s)); break;
        default: SPN_TRY(launch_ssim<5>(a, grid, s)); break;
    }
    hipLaunchKernelGGL(k_ssim_finish, dim3(1), dim3(kSsimThreads), 0, s, (const double*)a.part, (int)C,
                       (int64_t)grid.x * grid.y, (int64_t)H * W, result);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
