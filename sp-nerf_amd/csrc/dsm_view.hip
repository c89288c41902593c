// A ground-grid DSM seen from a camera (include/spnerf_amd_dsmview.h): the line of sight of every pixel of a
// lattice cast onto the DSM, rasters on the grid read at the hits, and the hits as ECEF points.  Compiled
// without fused multiply-adds (the file-scope pragma below): every product and sum is rounded once, as the
// numpy statement (tests/dsmview_numpy.py) rounds them, so floor(y) and the hit step do not flip against it
// beyond what the two localisations and projections differ by.
//  * k_dsmview_hmax — the maximum of the finite heights, per-workgroup partials; k_shadow_hmax
//    (csrc/shadow.hip) reads fp64 and keeps +inf, so the fp32 DSM has an instance of its own here.
//  * k_dsmview_cast — one thread per pixel, a workgroup on a 16 x 16 patch of the lattice (a wavefront on
//    16 x 4 pixels), so that neighbouring rays walk neighbouring cells of a DSM that fits in L2.  Per pixel:
//    two localisations (the iteration of csrc/rpc.h on the packed camera, its 80 coefficients read through
//    a uniform pointer), two forward projections (csrc/utm.h), and the DDA of csrc/shadow_march.h run the
//    other way: from the camera's end of the segment down to the first step at or below the surface.  The
//    steps above hmax are skipped.  About 1.5e4 fp64 operations and two dependent 4-byte loads per step.
//  * k_dsmview_sample, k_dsmview_ecef — one thread per entry.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "../../include/spnerf_amd_dsmview.h"
#include "rectify_cell.h"
#include "utm.h"
#include "wave.h"

namespace spn {

constexpr int kViewThreads = 256;
constexpr int kViewTile = 16;               // a workgroup's patch of the lattice, kViewTile² == kViewThreads
constexpr int kViewMaxParts = 256;          // partial maxima: 1 KiB, reduced by the first wavefront of every casting workgroup
constexpr double kViewFar = 2147483648.0;   // grid coordinates beyond ±2^31 are a miss

static int view_parts(int64_t cells) {
    const int64_t nb = (cells + 4 * kViewThreads - 1) / (4 * kViewThreads);
    return (int)(nb < kViewMaxParts ? nb : kViewMaxParts);
}

__global__ __launch_bounds__(kViewThreads) void k_dsmview_hmax(const float* __restrict__ dsm, int64_t cells, float* __restrict__ part) {
    __shared__ float s_max[kViewThreads / 64];
    const int tid = threadIdx.x;
    float v = -INFINITY;
    for (int64_t c = (int64_t)blockIdx.x * kViewThreads + tid; c < cells; c += (int64_t)gridDim.x * kViewThreads) {
        const float x = dsm[c];
        if (fabsf(x) < INFINITY) v = fmaxf(v, x);
    }
    v = wave_max(v);
    if ((tid & 63) == 0) s_max[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kViewThreads / 64; ++w) v = fmaxf(v, s_max[w]);
        part[blockIdx.x] = v;
    }
}

struct ViewArgs {
    const float* dsm;
    const double* cam;
    const float* part;
    uint8_t* hit;
    float* altitude;
    double* ground;
    float* cell;
    float* depth;
    double xoff, ytop, res, alt_lo, alt_hi;
    int xsize, ysize, zone, south, nparts;
    int col0, row0, stride, n_cols, n_rows;
};

// One walk along the major axis: p0, q0 the segment's start along the major and the minor axis, dmin its
// extent along the minor one, a = |extent along the major one|, sgn its sign, c0 the first centre line.
struct Walk {
    const float* dsm;
    double p0, q0, dmin, a, c0, sgn, alt_hi, dA, last;
    int64_t smaj, smin;
};

// step m of the walk: false when it does not contribute, else its parameter and its excess
__device__ __forceinline__ bool walk_step(const Walk& w, double m, double& t, double& e) {
    const double cm = w.c0 + w.sgn * m;
    t = (cm - w.p0) * w.sgn / w.a;
    const double y = w.q0 + t * w.dmin;
    if (!(y >= 0.0 && y <= w.last)) return false;
    const double fl = floor(y), f = y - fl;
    const float* p = w.dsm + (int64_t)cm * w.smaj + (int64_t)fl * w.smin;   // cm inside by the caller's range, fl by the test above
    const float g0 = p[0];
    if (!(fabsf(g0) < INFINITY)) return false;
    double hs = (double)g0;
    if (f != 0.0) {   // then y < last, so floor(y) + 1 is inside
        const float g1 = p[w.smin];
        if (!(fabsf(g1) < INFINITY)) return false;
        const double h1 = (double)g1;
        const double v = hs + f * (h1 - hs);
        hs = fmin(fmax(v, fmin(hs, h1)), fmax(hs, h1));
    }
    e = (w.alt_hi + t * w.dA) - hs;
    return true;
}

__global__ __launch_bounds__(kViewThreads) void k_dsmview_cast(ViewArgs g) {
    __shared__ float s_hmax;
    const int tid = threadIdx.x;
    if (tid < 64) {
        float v = -INFINITY;
        for (int p = tid; p < g.nparts; p += 64) v = fmaxf(v, g.part[p]);
        v = wave_max(v);
        if (tid == 0) s_hmax = v;
    }
    __syncthreads();
    const double hmax = (double)s_hmax;
    const int c = blockIdx.x * kViewTile + (tid & (kViewTile - 1));
    const int r = blockIdx.y * kViewTile + tid / kViewTile;
    if (c >= g.n_cols || r >= g.n_rows) return;
    const int64_t o = (int64_t)r * g.n_cols + c;

    const double* __restrict__ cam = g.cam;
    const double col = (double)g.col0 + (double)c * (double)g.stride, row = (double)g.row0 + (double)r * (double)g.stride;
    const double cn = (col - cam[1]) / cam[6], rn = (row - cam[0]) / cam[5];
    double lat, lon, e_hi, n_hi, e_lo, n_lo;
    localize_packed(cam, cn, rn, (g.alt_hi - cam[4]) / cam[9], lat, lon);
    utm_forward(lat, lon, g.zone, g.south, &e_hi, &n_hi);
    localize_packed(cam, cn, rn, (g.alt_lo - cam[4]) / cam[9], lat, lon);
    utm_forward(lat, lon, g.zone, g.south, &e_lo, &n_lo);
    const double dE = e_lo - e_hi, dN = n_lo - n_hi, dA = g.alt_lo - g.alt_hi;
    const double x_hi = (e_hi - g.xoff) / g.res - 0.5, y_hi = (g.ytop - n_hi) / g.res - 0.5;
    const double x_lo = (e_lo - g.xoff) / g.res - 0.5, y_lo = (g.ytop - n_lo) / g.res - 0.5;
    const double dx = x_lo - x_hi, dy = y_lo - y_hi;

    bool hit = false;
    double ts = 0.0;
    const bool near = fabs(x_hi) <= kViewFar && fabs(y_hi) <= kViewFar && fabs(x_lo) <= kViewFar && fabs(y_lo) <= kViewFar;   // false for a NaN
    if (near && hmax > -INFINITY) {
        if (dx == 0.0 && dy == 0.0) {
            const double fi = floor(x_hi + 0.5), fj = floor(y_hi + 0.5);
            if (fi >= 0.0 && fi <= (double)(g.xsize - 1) && fj >= 0.0 && fj <= (double)(g.ysize - 1)) {
                const float gh = g.dsm[(int64_t)fj * g.xsize + (int64_t)fi];
                const double h = (double)gh;
                if (fabsf(gh) < INFINITY && !(h < g.alt_lo)) {
                    hit = true;
                    ts = h >= g.alt_hi ? 0.0 : (g.alt_hi - h) / (g.alt_hi - g.alt_lo);
                }
            }
        } else {
            const bool rows = !(fabs(dx) >= fabs(dy));
            Walk w;
            w.dsm = g.dsm;
            w.p0 = rows ? y_hi : x_hi; w.q0 = rows ? x_hi : y_hi;
            const double dmaj = rows ? dy : dx;
            w.dmin = rows ? dx : dy;
            w.a = fabs(dmaj); w.sgn = dmaj > 0.0 ? 1.0 : -1.0;
            w.c0 = dmaj > 0.0 ? ceil(w.p0) : floor(w.p0);
            w.alt_hi = g.alt_hi; w.dA = dA;
            const int nmaj = rows ? g.ysize : g.xsize, nmin = rows ? g.xsize : g.ysize;
            w.last = (double)(nmin - 1);
            w.smaj = rows ? g.xsize : 1; w.smin = rows ? 1 : g.xsize;
            // the steps on the grid's lines, m_lo..m_hi, and within the segment, u_m <= a (whole numbers below 2^32: exact)
            const double m_lo = fmax(0.0, dmaj > 0.0 ? -w.c0 : w.c0 - (double)(nmaj - 1));
            double m_hi = dmaj > 0.0 ? (double)(nmaj - 1) - w.c0 : w.c0;
            const double u0 = (w.c0 - w.p0) * w.sgn;
            m_hi = fmin(m_hi, floor(w.a - u0) + 2.0);   // past the step beyond the end: the loop tests u_m itself
            if (m_lo <= m_hi) {
                // the first step that may stand at or below hmax: an estimate, then back while the step before does
                double m0 = m_lo;
                if (hmax < g.alt_hi) m0 = fmin(fmax(m_lo, floor((hmax - g.alt_hi) / dA * w.a - u0) - 1.0), m_hi + 1.0);
                while (m0 > m_lo && !(g.alt_hi + ((w.c0 + w.sgn * (m0 - 1.0)) - w.p0) * w.sgn / w.a * dA > hmax)) m0 -= 1.0;
                bool prev = false;
                double tp = 0.0, ep = 0.0;
                for (double m = m0; m <= m_hi; m += 1.0) {
                    const bool beyond = ((w.c0 + w.sgn * m) - w.p0) * w.sgn > w.a;   // the last step: on the line past the alt_lo end
                    double t, e;
                    if (walk_step(w, m, t, e)) {
                        if (e <= 0.0) {
                            // every step below m0 stands above hmax: it contributes a positive excess or nothing
                            for (double b = m0 - 1.0; !prev && b >= m_lo; b -= 1.0) prev = walk_step(w, b, tp, ep);
                            ts = prev ? tp + (t - tp) * (ep / (ep - e)) : t;
                            hit = ts <= 1.0;
                            break;
                        }
                        prev = true; tp = t; ep = e;
                    }
                    if (beyond) break;
                }
            }
        }
    }
    g.hit[o] = hit ? 1 : 0;
    if (hit) {
        g.altitude[o] = (float)(g.alt_hi + ts * dA);
        g.ground[2 * o] = e_hi + ts * dE;
        g.ground[2 * o + 1] = n_hi + ts * dN;
        g.cell[2 * o] = (float)fmin(fmax(x_hi + ts * dx, 0.0), (double)(g.xsize - 1));
        g.cell[2 * o + 1] = (float)fmin(fmax(y_hi + ts * dy, 0.0), (double)(g.ysize - 1));
        g.depth[o] = (float)(ts * sqrt((dE * dE + dN * dN) + dA * dA));
    } else {
        g.altitude[o] = NAN;
        g.ground[2 * o] = NAN;
        g.ground[2 * o + 1] = NAN;
        g.cell[2 * o] = NAN;
        g.cell[2 * o + 1] = NAN;
        g.depth[o] = NAN;
    }
}

__global__ __launch_bounds__(kViewThreads) void k_dsmview_sample(const float* __restrict__ raster, int H, int W,
                                                                 const float* __restrict__ cell, int64_t n, int mode,
                                                                 float* __restrict__ out) {
    const int64_t k = blockIdx.x * (int64_t)kViewThreads + threadIdx.x;
    if (k >= n) return;
    const double x = (double)cell[2 * k], y = (double)cell[2 * k + 1];
    float v = NAN;
    if (x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1)) {
        if (mode == SPNERF_DSMVIEW_NEAREST) {
            v = raster[(int64_t)floor(y + 0.5) * W + (int64_t)floor(x + 0.5)];
        } else {
            const double x0 = floor(x), y0 = floor(y);
            const double s = x - x0, t = y - y0;
            const int ia = (int)x0, ja = (int)y0;
            const int ib = ia + 1 < W ? ia + 1 : W - 1, jb = ja + 1 < H ? ja + 1 : H - 1;
            const double h[4] = {(double)raster[(int64_t)ja * W + ia], (double)raster[(int64_t)ja * W + ib],
                                 (double)raster[(int64_t)jb * W + ia], (double)raster[(int64_t)jb * W + ib]};
            const double wq[4] = {(1.0 - t) * (1.0 - s), (1.0 - t) * s, t * (1.0 - s), t * s};
            double num = 0.0, den = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (isfinite(h[q])) {
                    num += wq[q] * h[q];
                    den += wq[q];
                }
            v = den > 0.0 ? (float)(num / den) : NAN;
        }
    }
    out[k] = v;
}

__global__ __launch_bounds__(kViewThreads) void k_dsmview_ecef(const double* __restrict__ ground, const float* __restrict__ altitude,
                                                               int64_t n, int zone, int south, double* __restrict__ out) {
    const int64_t k = blockIdx.x * (int64_t)kViewThreads + threadIdx.x;
    if (k >= n) return;
    double lat, lon, x, y, z;
    utm_inverse(ground[2 * k], ground[2 * k + 1], zone, south, &lat, &lon);
    ecef(lat, lon, (double)altitude[k], x, y, z);
    out[3 * k] = x;
    out[3 * k + 1] = y;
    out[3 * k + 2] = z;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_dsmview_abi_version(void) { return SPNERF_DSMVIEW_ABI_VERSION; }

extern "C" int64_t spnerf_dsmview_workspace_bytes(int32_t ysize, int32_t xsize) {
    SPN_TRY(check_cells("dsmview_workspace_bytes", ysize, xsize));
    return (int64_t)align16((size_t)view_parts((int64_t)ysize * xsize) * sizeof(float));
}

extern "C" int32_t spnerf_dsmview_cast(const spnerf_ortho_grid* grid, const float* dsm, const double* camera, double alt_lo,
                                       double alt_hi, int32_t col0, int32_t row0, int32_t stride, int32_t n_cols, int32_t n_rows,
                                       void* workspace, uint8_t* hit, float* altitude, double* ground, float* cell, float* depth,
                                       void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grid && dsm && camera && workspace && hit && altitude && ground && cell && depth,
            "dsmview_cast: NULL grid, dsm, camera, workspace, hit, altitude, ground, cell or depth");
    SPN_TRY(check_grid("dsmview_cast", grid));
    SPN_ARG(std::isfinite(alt_lo) && std::isfinite(alt_hi), "dsmview_cast: altitudes %g, %g are not finite", alt_lo, alt_hi);
    SPN_ARG(alt_hi > alt_lo, "dsmview_cast: alt_hi %g must be above alt_lo %g", alt_hi, alt_lo);
    SPN_ARG(stride >= 1, "dsmview_cast: stride %d must be at least 1", stride);
    SPN_ARG(n_cols >= 1 && n_rows >= 1, "dsmview_cast: lattice of %d x %d pixels", n_cols, n_rows);
    SPN_ARG((int64_t)col0 + (int64_t)(n_cols - 1) * stride <= 0x7fffffffLL && (int64_t)row0 + (int64_t)(n_rows - 1) * stride <= 0x7fffffffLL,
            "dsmview_cast: the lattice from (%d, %d), %d x %d pixels of stride %d, leaves the int32 range", col0, row0, n_cols, n_rows,
            stride);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "dsmview_cast: workspace not 16-byte aligned");
    const int64_t cells = (int64_t)grid->xsize * grid->ysize, pixels = (int64_t)n_cols * n_rows;
    const unsigned bx = (unsigned)((n_cols + kViewTile - 1) / kViewTile), by = (unsigned)((n_rows + kViewTile - 1) / kViewTile);
    SPN_ARG(by <= 65535u, "dsmview_cast: %d lattice rows in one call (at most %d)", n_rows, 65535 * kViewTile);
    ViewArgs g{};
    g.dsm = dsm; g.cam = camera; g.part = (const float*)workspace;
    g.hit = hit; g.altitude = altitude; g.ground = ground; g.cell = cell; g.depth = depth;
    g.xoff = grid->xoff; g.ytop = grid->ytop; g.res = grid->resolution; g.alt_lo = alt_lo; g.alt_hi = alt_hi;
    g.xsize = grid->xsize; g.ysize = grid->ysize; g.zone = grid->zone; g.south = grid->south ? 1 : 0; g.nparts = view_parts(cells);
    g.col0 = col0; g.row0 = row0; g.stride = stride; g.n_cols = n_cols; g.n_rows = n_rows;
    ProfScope prof("dsmview_cast", st, (double)pixels * 1.5e4, (double)cells * 4.0 + (double)pixels * 33.0);
    hipLaunchKernelGGL(k_dsmview_hmax, dim3(g.nparts), dim3(kViewThreads), 0, st, dsm, cells, (float*)workspace);
    SPN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_dsmview_cast, dim3(bx, by), dim3(kViewThreads), 0, st, g);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_dsmview_sample(const float* raster, int32_t ysize, int32_t xsize, const float* cell, int64_t count,
                                         int32_t mode, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(raster && cell && out, "dsmview_sample: NULL raster, cell or out");
    SPN_TRY(check_cells("dsmview_sample", ysize, xsize));
    SPN_ARG(count >= 1 && count <= ((int64_t)1 << 32), "dsmview_sample: count %lld outside [1, 2^32]", (long long)count);
    SPN_ARG(mode == SPNERF_DSMVIEW_NEAREST || mode == SPNERF_DSMVIEW_BILINEAR, "dsmview_sample: mode %d is neither nearest (0) nor bilinear (1)",
            mode);
    ProfScope prof("dsmview_sample", st, (double)count * 16.0, (double)count * 28.0);
    hipLaunchKernelGGL(k_dsmview_sample, dim3(blocks_of(count, kViewThreads)), dim3(kViewThreads), 0, st, raster, ysize, xsize, cell, count, mode, out);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_dsmview_ecef(const double* ground, const float* altitude, int64_t count, int32_t zone, int32_t south,
                                       double* ecef_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(ground && altitude && ecef_out, "dsmview_ecef: NULL ground, altitude or ecef");
    SPN_ARG(count >= 1 && count <= ((int64_t)1 << 32), "dsmview_ecef: count %lld outside [1, 2^32]", (long long)count);
    SPN_ARG(zone >= 1 && zone <= 60, "dsmview_ecef: UTM zone %d", zone);
    ProfScope prof("dsmview_ecef", st, (double)count * 400.0, (double)count * 44.0);
    hipLaunchKernelGGL(k_dsmview_ecef, dim3(blocks_of(count, kViewThreads)), dim3(kViewThreads), 0, st, ground, altitude, count, zone, south ? 1 : 0,
                       ecef_out);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
