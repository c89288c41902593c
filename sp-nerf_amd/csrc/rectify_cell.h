// One cell of the ground grid in one camera, shared by the orthorectification (rectify.hip) and the
// plane sweep (sweep.hip): the RPC projection on a packed camera, its inverse (dsm_view.hip) and the bilinear read, as
// include/spnerf_amd_rectify.h states them, and the host check of a grid.
#pragma once
#include <cmath>

#include "../../include/spnerf_amd_rectify.h"
#include "ground.h"
#include "rpc.h"

namespace spn {

constexpr int kCam = SPNERF_RECTIFY_CAMERA_DOUBLES;

// proj_n (csrc/rpc.h) on a packed camera, from degrees and metres to pixels
__device__ __forceinline__ void project_packed(const double* __restrict__ c, double lat, double lon, double alt, double& col,
                                               double& row) {
    const double la = (lat - c[2]) / c[7], lo = (lon - c[3]) / c[8], al = (alt - c[4]) / c[9];
    col = rpoly(c + 50, la, lo, al) / rpoly(c + 70, la, lo, al) * c[6] + c[1];
    row = rpoly(c + 10, la, lo, al) / rpoly(c + 30, la, lo, al) * c[5] + c[0];
}

// The iteration of csrc/rpc.h (localize_n, the one spnerf_rpc_rays runs) over the projection of a packed camera
// c: normalised image (cn, rn) at the normalised altitude an -> degrees (lat, lon).
__device__ __forceinline__ void proj_packed_n(const double* __restrict__ c, double lat, double lon, double an, double& x, double& y) {
    x = rpoly(c + 50, lat, lon, an) / rpoly(c + 70, lat, lon, an);
    y = rpoly(c + 10, lat, lon, an) / rpoly(c + 30, lat, lon, an);
}

__device__ __forceinline__ void localize_packed(const double* __restrict__ c, double cn, double rn, double an, double& lat_d, double& lon_d) {
    double lon, lat;
    localize_n([c](double la, double lo, double al, double& x, double& y) { proj_packed_n(c, la, lo, al, x, y); }, cn, rn, an, lon, lat);
    lon_d = lon * c[8] + c[3];
    lat_d = lat * c[7] + c[2];
}

// the bilinear read of include/spnerf_amd_rectify.h; false (and NaN in every channel) outside the image
__device__ __forceinline__ bool sample_cell(const spnerf_rectify_image im, int C, double col, double row, float* __restrict__ out) {
#pragma clang fp contract(off)
    const double xl = (double)(im.width - 1), yl = (double)(im.height - 1);
    if (!(col >= 0.0 && col <= xl && row >= 0.0 && row <= yl)) {   // a NaN or an infinity fails a comparison
        for (int c = 0; c < C; ++c) out[c] = NAN;
        return false;
    }
    const double fx0 = floor(col), fy0 = floor(row);
    const double fx = col - fx0, fy = row - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = x0 + 1 < im.width ? x0 + 1 : im.width - 1, y1 = y0 + 1 < im.height ? y0 + 1 : im.height - 1;
    const float* r0 = im.pixels + (int64_t)y0 * im.width * C;
    const float* r1 = im.pixels + (int64_t)y1 * im.width * C;
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    for (int c = 0; c < C; ++c) {
        const double p00 = (double)r0[(int64_t)x0 * C + c], p01 = (double)r0[(int64_t)x1 * C + c];
        const double p10 = (double)r1[(int64_t)x0 * C + c], p11 = (double)r1[(int64_t)x1 * C + c];
        const double top = gx * p00 + fx * p01;
        const double bot = gx * p10 + fx * p11;
        out[c] = (float)(top * gy + bot * fy);
    }
    return true;
}

inline int32_t check_grid(const char* who, const spnerf_ortho_grid* g) {
    SPN_TRY(check_cells(who, g->ysize, g->xsize));
    SPN_ARG(g->zone >= 1 && g->zone <= 60, "%s: UTM zone %d", who, g->zone);
    SPN_ARG(g->resolution > 0.0 && std::isfinite(g->resolution), "%s: resolution %g", who, g->resolution);
    SPN_ARG(std::isfinite(g->xoff) && std::isfinite(g->ytop), "%s: non-finite grid origin", who);
    return SPNERF_OK;
}

}  // namespace spn
