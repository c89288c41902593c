// Plane sweep (include/spnerf_amd_sweep.h): a photo-consistency DSM on the ground grid from the camera
// images alone.  The whole translation unit is compiled without fused multiply-adds (the file-scope
// pragma below, honoured under the Makefile's -ffp-contract=fast-honor-pragmas), so the header's
// operation order is the result and a device function gives the same bits in every kernel that uses it.
//  * grey_cell, score_cell<VMAX> and the fused k_sweep<VMAX, GATED, SURFACE> are csrc/sweep_cell.h's, shared with the
//    sweep gated by a visibility floor (occlusion.hip) and the sweep around a base surface (surface.hip); this file
//    instantiates the plain k_sweep.
//  * Pick (csrc/sweep_pick.h) — the running best of a cell and the scores of its two neighbouring planes, fed
//    plane by plane: from a stored volume (k_sweep_pick) or as the planes are scored (k_sweep).
//  * k_sweep_grey, k_sweep_score, k_sweep_pick — the staged path, one thread per cell each.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "sweep_cell.h"

namespace spn {

//   cams [V][90]; images [V]; grey [V][cells]; valid [V][cells]
__global__ __launch_bounds__(kSweepThreads) void k_sweep_grey(SweepArgs g, double alt, const double* __restrict__ cams,
                                                              const spnerf_rectify_image* __restrict__ images,
                                                              float* __restrict__ grey, uint8_t* __restrict__ valid) {
    const int64_t cells = (int64_t)g.xsize * g.ysize;
    const int64_t cell = blockIdx.x * (int64_t)kSweepThreads + threadIdx.x;
    if (cell >= cells) return;
    const int i = (int)(cell % g.xsize);
    const int64_t j = cell / g.xsize;
    double lat, lon;
    utm_inverse(g.xoff + ((double)i + 0.5) * g.res, g.ytop - ((double)j + 0.5) * g.res, g.zone, g.south, &lat, &lon);
    for (int v = 0; v < g.V; ++v) {
        bool ok;
        grey[v * cells + cell] = grey_cell(cams + (int64_t)v * kCam, images[v], g.C, lat, lon, alt, ok);
        valid[v * cells + cell] = ok ? 1 : 0;
    }
}

template <int VMAX>
__global__ __launch_bounds__(kSweepThreads) void k_sweep_score(const float* __restrict__ grey, const uint8_t* __restrict__ valid, int V,
                                                               int ysize, int xsize, int tx, int radius, int min_views, double min_std,
                                                               float* __restrict__ score, uint8_t* __restrict__ views) {
    int tj0, ti0;
    tile_origin(blockIdx.x, tx, tj0, ti0);
    const int j = tj0 + (int)threadIdx.x / kTile, i = ti0 + (int)threadIdx.x % kTile;
    if (j >= ysize || i >= xsize) return;
    const GlobalGreys a{grey, valid, (int64_t)xsize * ysize, xsize};
    int m;
    const float s = score_cell<VMAX>(a, V, max(j - radius, 0), min(j + radius, ysize - 1), max(i - radius, 0), min(i + radius, xsize - 1),
                                     min_views, min_std, m);
    score[(int64_t)j * xsize + i] = s;
    views[(int64_t)j * xsize + i] = (uint8_t)m;
}

__global__ __launch_bounds__(kSweepThreads) void k_sweep_pick(const float* __restrict__ volume, const uint8_t* __restrict__ views_vol, int K,
                                                              int64_t cells, double alt_lo, double step, float* __restrict__ altitude,
                                                              float* __restrict__ score, int32_t* __restrict__ index,
                                                              uint8_t* __restrict__ views) {
    const int64_t cell = blockIdx.x * (int64_t)kSweepThreads + threadIdx.x;
    if (cell >= cells) return;
    Pick p;
    for (int k = 0; k < K; ++k) p.plane(k, volume[k * cells + cell], views_vol[k * cells + cell]);
    altitude[cell] = p.altitude(K, alt_lo, step);
    score[cell] = p.best;
    index[cell] = p.index;
    views[cell] = (uint8_t)p.m;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_sweep_abi_version(void) { return SPNERF_SWEEP_ABI_VERSION; }

extern "C" int32_t spnerf_sweep_grey(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                                     int32_t n_views, int32_t channels, double alt, float* grey, uint8_t* valid, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grid && cameras && images && grey && valid, "sweep_grey: NULL grid, cameras, images, grey or valid");
    SPN_TRY(check_grid("sweep_grey", grid));
    SPN_TRY(check_views_channels("sweep_grey", n_views, channels));
    SPN_ARG(std::isfinite(alt), "sweep_grey: alt %g is not finite", alt);
    SweepArgs g{};
    g.xoff = grid->xoff; g.ytop = grid->ytop; g.res = grid->resolution;
    g.xsize = grid->xsize; g.ysize = grid->ysize; g.zone = grid->zone; g.south = grid->south ? 1 : 0; g.V = n_views; g.C = channels;
    const int64_t cells = (int64_t)g.xsize * g.ysize;
    ProfScope prof("sweep_grey", st, (double)cells * n_views * grey_flop(channels), (double)cells * n_views * (16.0 * channels + 5.0));
    hipLaunchKernelGGL(k_sweep_grey, dim3(blocks_of(cells, kSweepThreads)), dim3(kSweepThreads), 0, st, g, alt, cameras, images, grey, valid);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_sweep_score(const float* grey, const uint8_t* valid, int32_t n_views, int32_t ysize, int32_t xsize,
                                      int32_t radius, int32_t min_views, double min_std, float* score, uint8_t* views, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grey && valid && score && views, "sweep_score: NULL grey, valid, score or views");
    SPN_TRY(check_cells("sweep_score", ysize, xsize));
    SPN_TRY(check_views_channels("sweep_score", n_views, 1));
    SPN_TRY(check_window("sweep_score", n_views, radius, min_views, min_std));
    int tx;
    const unsigned tiles = tiles_of(ysize, xsize, tx);
    const double cells = (double)xsize * ysize;
    ProfScope prof("sweep_score", st, cells * score_flop(n_views, radius), cells * (n_views * 5.0 + 5.0));
    if (n_views <= 4)
        hipLaunchKernelGGL(k_sweep_score<4>, dim3(tiles), dim3(kSweepThreads), 0, st, grey, valid, n_views, ysize, xsize, tx, radius,
                           min_views, min_std, score, views);
    else if (n_views <= 8)
        hipLaunchKernelGGL(k_sweep_score<8>, dim3(tiles), dim3(kSweepThreads), 0, st, grey, valid, n_views, ysize, xsize, tx, radius,
                           min_views, min_std, score, views);
    else
        hipLaunchKernelGGL(k_sweep_score<16>, dim3(tiles), dim3(kSweepThreads), 0, st, grey, valid, n_views, ysize, xsize, tx, radius,
                           min_views, min_std, score, views);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_sweep_pick(const float* volume, const uint8_t* views_vol, int32_t n_planes, int64_t cells, double alt_lo,
                                     double step, float* altitude, float* score, int32_t* index, uint8_t* views, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(volume && views_vol && altitude && score && index && views,
            "sweep_pick: NULL volume, views_vol, altitude, score, index or views");
    SPN_ARG(cells >= 1 && cells <= ((int64_t)1 << 32), "sweep_pick: cells %lld outside [1, 2^32]", (long long)cells);
    SPN_TRY(check_planes("sweep_pick", n_planes, alt_lo, step));
    ProfScope prof("sweep_pick", st, 0.0, (double)cells * (n_planes * 5.0 + 13.0));
    hipLaunchKernelGGL(k_sweep_pick, dim3(blocks_of(cells, kSweepThreads)), dim3(kSweepThreads), 0, st, volume, views_vol, n_planes, cells, alt_lo, step,
                       altitude, score, index, views);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_sweep(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                                int32_t n_views, int32_t channels, double alt_lo, double step, int32_t n_planes, int32_t radius,
                                int32_t min_views, double min_std, float* altitude, float* score, int32_t* index, uint8_t* views,
                                float* volume, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grid && cameras && images && altitude && score && index && views,
            "sweep: NULL grid, cameras, images, altitude, score, index or views");
    return launch_sweep<false>("sweep", grid, cameras, images, n_views, channels, alt_lo, step, n_planes, radius, min_views, min_std,
                               altitude, score, index, views, volume, nullptr, 0.0, st);
}
