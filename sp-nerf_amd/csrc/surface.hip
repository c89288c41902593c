// Surface sweep (include/spnerf_amd_surface.h): the plane sweep around a base raster on the ground grid, and
// the two small steps a coarse-to-fine chain needs around it.  Compiled without fused multiply-adds, as
// sweep.hip is (the file-scope pragma below), so the fused sweep has the bits of the staged chain.
//  * k_surface_grey — k_sweep_grey with the altitude of each cell its own: one thread per cell looping over
//    the views, grey_cell (csrc/sweep_cell.h) unchanged.
//  * k_surface_lift, k_surface_upsample — one thread per entry / fine cell; 4 B read and written per entry,
//    four gathered reads per fine cell that neighbouring lanes share.
//  * k_sweep<VMAX, false, true> — csrc/sweep_cell.h's fused sweep with the bases of tile and halo in LDS.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "../../include/spnerf_amd_surface.h"
#include "sweep_cell.h"

namespace spn {

//   cams [V][90]; images [V]; base [cells]; grey [V][cells]; valid [V][cells]
__global__ __launch_bounds__(kSweepThreads) void k_surface_grey(SweepArgs g, double offset, const double* __restrict__ cams,
                                                                const spnerf_rectify_image* __restrict__ images,
                                                                const float* __restrict__ base, float* __restrict__ grey,
                                                                uint8_t* __restrict__ valid) {
    const int64_t cells = (int64_t)g.xsize * g.ysize;
    const int64_t cell = blockIdx.x * (int64_t)kSweepThreads + threadIdx.x;
    if (cell >= cells) return;
    const float b = base[cell];
    if (!isfinite(b)) {
        for (int v = 0; v < g.V; ++v) {
            grey[v * cells + cell] = NAN;
            valid[v * cells + cell] = 0;
        }
        return;
    }
    const int i = (int)(cell % g.xsize);
    const int64_t j = cell / g.xsize;
    const double alt = (double)b + offset;
    double lat, lon;
    utm_inverse(g.xoff + ((double)i + 0.5) * g.res, g.ytop - ((double)j + 0.5) * g.res, g.zone, g.south, &lat, &lon);
    for (int v = 0; v < g.V; ++v) {
        bool ok;
        grey[v * cells + cell] = grey_cell(cams + (int64_t)v * kCam, images[v], g.C, lat, lon, alt, ok);
        valid[v * cells + cell] = ok ? 1 : 0;
    }
}

// out may be base or rel: an entry is read and written by one thread
__global__ __launch_bounds__(kSweepThreads) void k_surface_lift(const float* base, const float* rel, int64_t n, float* out) {
    const int64_t e = blockIdx.x * (int64_t)kSweepThreads + threadIdx.x;
    if (e >= n) return;
    out[e] = (float)((double)base[e] + (double)rel[e]);
}

// the two source indices along one axis of `size` entries and the weight of the second one
__device__ __forceinline__ void upsample_axis(int fine, double f, int size, int& a, int& b, double& t) {
    const double y = ((double)fine + 0.5) / f - 0.5;
    const double y0 = floor(y);
    t = y - y0;
    const int k = (int)y0;   // -1 .. size - 1
    a = min(max(k, 0), size - 1);
    b = min(max(k + 1, 0), size - 1);
}

__global__ __launch_bounds__(kSweepThreads) void k_surface_upsample(const float* __restrict__ coarse, int factor, int hc, int wc, int H,
                                                                    int W, float* __restrict__ out) {
    const int64_t cell = blockIdx.x * (int64_t)kSweepThreads + threadIdx.x;
    if (cell >= (int64_t)H * W) return;
    const int i = (int)(cell % W), j = (int)(cell / W);
    int ja, jb, ia, ib;
    double t, s;
    upsample_axis(j, (double)factor, hc, ja, jb, t);
    upsample_axis(i, (double)factor, wc, ia, ib, s);
    const double h[4] = {(double)coarse[(int64_t)ja * wc + ia], (double)coarse[(int64_t)ja * wc + ib],
                         (double)coarse[(int64_t)jb * wc + ia], (double)coarse[(int64_t)jb * wc + ib]};
    const double w[4] = {(1.0 - t) * (1.0 - s), (1.0 - t) * s, t * (1.0 - s), t * s};
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (isfinite(h[q])) {
            num += w[q] * h[q];
            den += w[q];
        }
    out[cell] = den > 0.0 ? (float)(num / den) : NAN;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_surface_abi_version(void) { return SPNERF_SURFACE_ABI_VERSION; }

extern "C" int32_t spnerf_surface_grey(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                                       int32_t n_views, int32_t channels, const float* base, double offset, float* grey,
                                       uint8_t* valid, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grid && cameras && images && base && grey && valid, "surface_grey: NULL grid, cameras, images, base, grey or valid");
    SPN_TRY(check_grid("surface_grey", grid));
    SPN_TRY(check_views_channels("surface_grey", n_views, channels));
    SPN_ARG(std::isfinite(offset), "surface_grey: offset %g is not finite", offset);
    SweepArgs g{};
    g.xoff = grid->xoff; g.ytop = grid->ytop; g.res = grid->resolution;
    g.xsize = grid->xsize; g.ysize = grid->ysize; g.zone = grid->zone; g.south = grid->south ? 1 : 0; g.V = n_views; g.C = channels;
    const int64_t cells = (int64_t)g.xsize * g.ysize;
    ProfScope prof("surface_grey", st, (double)cells * n_views * grey_flop(channels),
                   (double)cells * (4.0 + n_views * (16.0 * channels + 5.0)));
    hipLaunchKernelGGL(k_surface_grey, dim3(blocks_of(cells, kSweepThreads)), dim3(kSweepThreads), 0, st, g, offset, cameras, images, base, grey, valid);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_surface_lift(const float* base, const float* rel, int64_t count, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(base && rel && out, "surface_lift: NULL base, rel or out");
    SPN_ARG(count >= 1 && count <= ((int64_t)1 << 32), "surface_lift: count %lld outside [1, 2^32]", (long long)count);
    ProfScope prof("surface_lift", st, (double)count, (double)count * 12.0);
    hipLaunchKernelGGL(k_surface_lift, dim3(blocks_of(count, kSweepThreads)), dim3(kSweepThreads), 0, st, base, rel, count, out);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_surface_upsample(const float* coarse, int32_t factor, int32_t ysize, int32_t xsize, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(coarse && out, "surface_upsample: NULL coarse or out");
    SPN_ARG(factor >= 1 && factor <= SPNERF_SURFACE_MAX_FACTOR, "surface_upsample: factor %d outside [1, %d]", factor,
            SPNERF_SURFACE_MAX_FACTOR);
    SPN_TRY(check_cells("surface_upsample", ysize, xsize));
    const int hc = (int)(((int64_t)ysize + factor - 1) / factor), wc = (int)(((int64_t)xsize + factor - 1) / factor);
    const int64_t cells = (int64_t)xsize * ysize;
    ProfScope prof("surface_upsample", st, (double)cells * 16.0, (double)cells * 4.0 + (double)hc * wc * 4.0);
    hipLaunchKernelGGL(k_surface_upsample, dim3(blocks_of(cells, kSweepThreads)), dim3(kSweepThreads), 0, st, coarse, factor, hc, wc, ysize, xsize, out);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_surface_sweep(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                                        int32_t n_views, int32_t channels, const float* base, double off_lo, double step,
                                        int32_t n_planes, int32_t radius, int32_t min_views, double min_std, float* altitude,
                                        float* score, int32_t* index, uint8_t* views, float* volume, void* stream) {
    SPN_ARG(grid && cameras && images && base && altitude && score && index && views,
            "surface_sweep: NULL grid, cameras, images, base, altitude, score, index or views");
    return launch_sweep<false, true>("surface_sweep", grid, cameras, images, n_views, channels, off_lo, step, n_planes, radius, min_views,
                                     min_std, altitude, score, index, views, volume, base, 0.0, (hipStream_t)stream);
}
