// RPC camera rays on gfx950 — datasets/satellite_scene.py:21-68 (get_rays), :415-425
// (normalize_rays), :449-473 (get_sun_dirs) with modules/utils.py:59-100 (rescale_rpc,
// geodetic_to_ecef), one thread per pixel.
//
// Localization and ECEF are csrc/rpc.h (shared with dataset.hip).
// Precision sequence of the reference: ECEF in fp64 → cast to fp32 (satellite_scene.py:66) →
// centring and scaling in fp32 (:415-425), so the 0.5 m fp32 quantisation of ECEF at
// 5.45e6 m is reproduced, not removed.
#include "../../include/spnerf_amd_data.h"
#include "rpc.h"

namespace spn {

struct RpcArgs {
    RpcCam cam;
    int row0, col0, nrows, ncols;
    const int32_t* pix;  // optional (n, 2) [col, row] pixel list instead of the rectangle
    const double* pixd;  // or the same list as doubles (fractional pixels)
    int64_t n;
    float center[3], range, sun[3];
    int normalize;
    float* out;
    int stride;
};

__global__ __launch_bounds__(256) void k_rpc_rays(RpcArgs a) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double col, row;
    if (a.pixd) {
        col = a.pixd[2 * i];
        row = a.pixd[2 * i + 1];
    } else if (a.pix) {
        col = a.pix[2 * i];
        row = a.pix[2 * i + 1];
    } else {
        col = a.col0 + (double)(i % a.ncols);
        row = a.row0 + (double)(i / a.ncols);
    }
    float v[8];
    rpc_ray(a.cam, col, row, v);
    if (a.normalize) normalize_ray(v, a.center, a.range);
    float* o = a.out + i * a.stride;
    for (int k = 0; k < 8; ++k) o[k] = v[k];
    if (a.stride >= 11)
        for (int k = 0; k < 3; ++k) o[8 + k] = a.sun[k];
}

static int32_t launch_rays(const double* rpc, double downscale, double min_alt, double max_alt, int32_t row0, int32_t col0,
                           int32_t n_rows, int32_t n_cols, const int32_t* pixels, const double* pixels_f64,
                           int64_t n_pixels, const float* center, float range, const float* sun, float* rays,
                           int32_t ray_stride, void* stream) {
    SPN_ARG(rpc && rays, "rpc_rays: NULL pointer");
    SPN_ARG(ray_stride >= 8 && downscale > 0, "rpc_rays: bad stride / downscale");
    SPN_ARG(ray_stride < 11 || sun, "rpc_rays: an 11-wide ray needs the sun direction");
    RpcArgs a{};
    rpc_unpack(a.cam, rpc, downscale, min_alt, max_alt);
    a.row0 = row0;
    a.col0 = col0;
    a.nrows = n_rows;
    a.ncols = n_cols;
    a.pix = pixels;
    a.pixd = pixels_f64;
    a.n = (pixels || pixels_f64) ? n_pixels : (int64_t)n_rows * n_cols;
    a.normalize = center != nullptr;
    if (center)
        for (int k = 0; k < 3; ++k) a.center[k] = center[k];
    a.range = range;
    if (sun)
        for (int k = 0; k < 3; ++k) a.sun[k] = sun[k];
    a.out = rays;
    a.stride = ray_stride;
    if (a.n <= 0) return SPNERF_OK;
    ProfScope prof("rpc_rays", (hipStream_t)stream, 0.0, 4.0 * ray_stride * a.n);
    hipLaunchKernelGGL(k_rpc_rays, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_rpc_rays(const double* rpc, double downscale, double min_alt, double max_alt, int32_t row0,
                                   int32_t col0, int32_t n_rows, int32_t n_cols, const int32_t* pixels, int64_t n_pixels,
                                   const float* center, float range, const float* sun, float* rays, int32_t ray_stride,
                                   void* stream) {
    return launch_rays(rpc, downscale, min_alt, max_alt, row0, col0, n_rows, n_cols, pixels, nullptr, n_pixels, center,
                       range, sun, rays, ray_stride, stream);
}

// include/spnerf_amd_data.h: the pixel list as (n, 2) [col, row] doubles
extern "C" int32_t spnerf_rpc_rays_f64(const double* rpc, double downscale, double min_alt, double max_alt,
                                       const double* pixels, int64_t n_pixels, const float* center, float range,
                                       const float* sun, float* rays, int32_t ray_stride, void* stream) {
    SPN_ARG(pixels && n_pixels >= 0, "rpc_rays_f64: NULL pixel list");
    return launch_rays(rpc, downscale, min_alt, max_alt, 0, 0, 0, 0, nullptr, pixels, n_pixels, center, range, sun, rays,
                       ray_stride, stream);
}
