// Orthorectification (include/spnerf_amd_rectify.h): camera images put onto a UTM ground grid over a DSM.
//  * k_rectify — one thread per cell: the inverse transverse Mercator of the cell centre (csrc/utm.h)
//    once, then per view the RPC projection at the cell's DSM altitude (rpoly of csrc/rpc.h on the
//    packed camera table) and, with images, the bilinear read.  spnerf_rectify_project (no images)
//    and spnerf_rectify (images, pix optional) are launches of this one kernel, so a pixel position
//    is the same machine code whether it is stored or kept in a register.  The camera table and the
//    image table are const __restrict__ kernel parameters read at wavefront-uniform addresses, so
//    they arrive by scalar loads (eleven 64-B s_load per view in the ISA), not once per lane.
//    HBM: 8 B of DSM per cell; per view and cell at most 16·C B of image (four pixels, mostly shared
//    with the neighbouring cells through L2) and 4·C + 1 B out (+ 16 B of pix when asked for).
//  * k_rectify_sample — the same read (sample_cell of csrc/rectify_cell.h, which sweep.hip shares, as
//    it does project_packed) at stored pixel positions.  sample_cell is compiled without fused multiply-adds (#pragma clang fp contract(off), honoured under the
//    Makefile's -ffp-contract=fast-honor-pragmas), so the stated operation order is the result.
//  * k_rectify_view_dirs — one workgroup per view, one thread per ground point (centre, four
//    corners): project at alt_lo, localise at alt_hi (csrc/rpc.h), forward UTM, normalise.
//  * k_rectify_mosaic — one thread per cell: mean or median over the usable views, their count and
//    the RMS deviation from the mean.  The median ranks the at most 64 values by counting (no
//    per-thread array, no scratch): V² compares of values that sit in L1.
#include <cmath>

#include "rectify_cell.h"
#include "utm.h"

namespace spn {

constexpr int kRectifyThreads = 256;
struct RectifyArgs {
    double xoff, ytop, res;
    int64_t cells;
    int xsize, zone, south, V, C;
};

// The tables and planes are kernel parameters of their own, const and __restrict__: only so can the
// compiler prove that the stores of the view loop do not touch the tables and read them by scalar loads.
//   cams [V][90]; images [V], or NULL: positions only; pix [V][cells][2], or NULL; rgb [V][cells][C]; valid [V][cells]
__global__ __launch_bounds__(kRectifyThreads) void k_rectify(RectifyArgs g, const double* __restrict__ dsm,
                                                             const double* __restrict__ cams,
                                                             const spnerf_rectify_image* __restrict__ images,
                                                             double* __restrict__ pix, float* __restrict__ rgb,
                                                             uint8_t* __restrict__ valid) {
    const int64_t cell = blockIdx.x * (int64_t)kRectifyThreads + threadIdx.x;
    if (cell >= g.cells) return;
    const double h = dsm[cell];
    const bool known = h == h;
    double lat = 0.0, lon = 0.0;
    if (known) {
        const int i = (int)(cell % g.xsize);
        const int64_t j = cell / g.xsize;
        utm_inverse(g.xoff + ((double)i + 0.5) * g.res, g.ytop - ((double)j + 0.5) * g.res, g.zone, g.south, &lat, &lon);
    }
    for (int v = 0; v < g.V; ++v) {
        double col = NAN, row = NAN;
        if (known) project_packed(cams + (int64_t)v * kCam, lat, lon, h, col, row);
        const int64_t o = (int64_t)v * g.cells + cell;
        if (pix) {
            pix[2 * o] = col;
            pix[2 * o + 1] = row;
        }
        if (images) valid[o] = sample_cell(images[v], g.C, col, row, rgb + o * g.C) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kRectifyThreads) void k_rectify_sample(const spnerf_rectify_image* __restrict__ images, int V, int C,
                                                                    const double* __restrict__ pix, int64_t cells,
                                                                    float* __restrict__ rgb, uint8_t* __restrict__ valid) {
    const int64_t cell = blockIdx.x * (int64_t)kRectifyThreads + threadIdx.x;
    if (cell >= cells) return;
    for (int v = 0; v < V; ++v) {
        const int64_t o = (int64_t)v * cells + cell;
        valid[o] = sample_cell(images[v], C, pix[2 * o], pix[2 * o + 1], rgb + o * C) ? 1 : 0;
    }
}

struct ViewDirArgs {
    const double* cams;
    float* dirs;
    float* spread;
    double e[5], n[5];   // the centre, then the four corners
    double alt_lo, alt_hi;
    int zone, south;
};

__global__ __launch_bounds__(64) void k_rectify_view_dirs(ViewDirArgs g) {
    __shared__ double s_d[5][3];
    const int t = threadIdx.x, v = blockIdx.x;
    if (t < 5) {
        const double* c = g.cams + (int64_t)v * kCam;
        RpcCam a;
        for (int k = 0; k < 10; ++k) a.off[k] = c[k];
        for (int k = 0; k < 20; ++k) {
            a.rn[k] = c[10 + k];
            a.rd[k] = c[30 + k];
            a.cn[k] = c[50 + k];
            a.cd[k] = c[70 + k];
        }
        a.min_alt = g.alt_lo;
        a.max_alt = g.alt_hi;
        double lat, lon, col, row, lat2, lon2, e2, n2;
        utm_inverse(g.e[t], g.n[t], g.zone, g.south, &lat, &lon);
        project_packed(c, lat, lon, g.alt_lo, col, row);
        localize(a, (col - a.off[1]) / a.off[6], (row - a.off[0]) / a.off[5], (g.alt_hi - a.off[4]) / a.off[9], lon2, lat2);
        utm_forward(lat2, lon2, g.zone, g.south, &e2, &n2);
        const double dx = e2 - g.e[t], dy = n2 - g.n[t], dz = g.alt_hi - g.alt_lo;
        const double nrm = sqrt((dx * dx + dy * dy) + dz * dz);
        s_d[t][0] = dx / nrm;
        s_d[t][1] = dy / nrm;
        s_d[t][2] = dz / nrm;
    }
    __syncthreads();
    if (t == 0) {
        double worst = 0.0;
        for (int p = 1; p < 5; ++p)
            for (int k = 0; k < 3; ++k) {
                const double d = fabs(s_d[p][k] - s_d[0][k]);
                if (d > worst || d != d) worst = d;   // a NaN stands: nothing compares above it
            }
        for (int k = 0; k < 3; ++k) g.dirs[3 * v + k] = (float)s_d[0][k];
        g.spread[v] = (float)worst;
    }
}

// a strict order of (value, view): by value, a NaN last, equal values by view
__device__ __forceinline__ bool sorts_before(float a, int i, float b, int j) {
    if (a < b) return true;
    if (b < a) return false;
    const bool an = a != a, bn = b != b;
    if (an != bn) return bn;
    return i < j;
}

__global__ __launch_bounds__(kRectifyThreads) void k_rectify_mosaic(const float* __restrict__ rgb, const uint8_t* __restrict__ usable,
                                                                    int V, int64_t cells, int C, int mode, float* __restrict__ mosaic,
                                                                    int32_t* __restrict__ count, float* __restrict__ spread) {
#pragma clang fp contract(off)
    const int64_t cell = blockIdx.x * (int64_t)kRectifyThreads + threadIdx.x;
    if (cell >= cells) return;
    uint64_t use = 0;
    int n = 0;
    for (int v = 0; v < V; ++v)
        if (usable[(int64_t)v * cells + cell] == 1) {
            use |= (uint64_t)1 << v;
            ++n;
        }
    count[cell] = n;
    if (n == 0) {
        for (int c = 0; c < C; ++c) mosaic[cell * C + c] = NAN;
        spread[cell] = NAN;
        return;
    }
    const float* x = rgb + cell * C;
    const int64_t stride = cells * C;   // from one view to the next
    const int k_lo = (n - 1) / 2, k_hi = n / 2;
    double dev = 0.0;
    for (int c = 0; c < C; ++c) {
        double sum = 0.0;
        for (int v = 0; v < V; ++v)
            if (use >> v & 1) sum += (double)x[v * stride + c];
        const double mean = sum / (double)n;
        for (int v = 0; v < V; ++v)
            if (use >> v & 1) {
                const double d = (double)x[v * stride + c] - mean;
                dev += d * d;
            }
        double out = mean;
        if (mode == SPNERF_RECTIFY_MEDIAN) {
            double lo = 0.0, hi = 0.0;
            for (int v = 0; v < V; ++v) {
                if (!(use >> v & 1)) continue;
                const float xv = x[v * stride + c];
                int rank = 0;
                for (int u = 0; u < V; ++u)
                    if ((use >> u & 1) && sorts_before(x[u * stride + c], u, xv, v)) ++rank;
                if (rank == k_lo) lo = (double)xv;
                if (rank == k_hi) hi = (double)xv;
            }
            out = (lo + hi) / 2.0;
        }
        mosaic[cell * C + c] = (float)out;
    }
    spread[cell] = (float)sqrt(dev / (double)((int64_t)n * C));
}

static int32_t check_views(const char* who, int32_t n_views) {
    SPN_ARG(n_views > 0 && n_views <= SPNERF_RECTIFY_MAX_VIEWS, "%s: n_views %d outside [1, %d]", who, n_views, SPNERF_RECTIFY_MAX_VIEWS);
    return SPNERF_OK;
}

static int32_t check_channels(const char* who, int32_t channels) {
    SPN_ARG(channels > 0 && channels <= SPNERF_RECTIFY_MAX_CHANNELS, "%s: channels %d outside [1, %d]", who, channels,
            SPNERF_RECTIFY_MAX_CHANNELS);
    return SPNERF_OK;
}

// spnerf_rectify_project (images NULL) and spnerf_rectify
static int32_t launch_rectify(const char* who, const double* dsm, const spnerf_ortho_grid* grid, const double* cameras,
                              const spnerf_rectify_image* images, int32_t n_views, int32_t channels, float* rgb, uint8_t* valid,
                              double* pix, hipStream_t st) {
    SPN_TRY(check_grid(who, grid));
    SPN_TRY(check_views(who, n_views));
    if (images) SPN_TRY(check_channels(who, channels));
    RectifyArgs g{};
    g.xoff = grid->xoff; g.ytop = grid->ytop; g.res = grid->resolution;
    g.cells = (int64_t)grid->xsize * grid->ysize;
    g.xsize = grid->xsize; g.zone = grid->zone; g.south = grid->south ? 1 : 0; g.V = n_views; g.C = channels;
    const double per_view = (images ? 20.0 * channels + 1.0 : 0.0) + (pix ? 16.0 : 0.0);
    ProfScope prof("rectify", st, 0.0, (double)g.cells * (8.0 + n_views * per_view));
    hipLaunchKernelGGL(k_rectify, dim3(blocks_of(g.cells, kRectifyThreads)), dim3(kRectifyThreads), 0, st, g, dsm, cameras, images, pix, rgb, valid);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_rectify_abi_version(void) { return SPNERF_RECTIFY_ABI_VERSION; }

extern "C" int32_t spnerf_rectify_project(const double* dsm, const spnerf_ortho_grid* grid, const double* cameras, int32_t n_views,
                                          double* pix, void* stream) {
    SPN_ARG(dsm && grid && cameras && pix, "rectify_project: NULL dsm, grid, cameras or pix");
    return launch_rectify("rectify_project", dsm, grid, cameras, nullptr, n_views, 0, nullptr, nullptr, pix, (hipStream_t)stream);
}

extern "C" int32_t spnerf_rectify(const double* dsm, const spnerf_ortho_grid* grid, const double* cameras,
                                  const spnerf_rectify_image* images, int32_t n_views, int32_t channels, float* rgb, uint8_t* valid,
                                  double* pix, void* stream) {
    SPN_ARG(dsm && grid && cameras && images && rgb && valid, "rectify: NULL dsm, grid, cameras, images, rgb or valid");
    return launch_rectify("rectify", dsm, grid, cameras, images, n_views, channels, rgb, valid, pix, (hipStream_t)stream);
}

extern "C" int32_t spnerf_rectify_sample(const spnerf_rectify_image* images, int32_t n_views, int32_t channels, const double* pix,
                                         int64_t cells, float* rgb, uint8_t* valid, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(images && pix && rgb && valid, "rectify_sample: NULL images, pix, rgb or valid");
    SPN_ARG(cells >= 1 && cells <= ((int64_t)1 << 32), "rectify_sample: cells %lld outside [1, 2^32]", (long long)cells);
    SPN_TRY(check_views("rectify_sample", n_views));
    SPN_TRY(check_channels("rectify_sample", channels));
    ProfScope prof("rectify_sample", st, 0.0, (double)cells * n_views * (16.0 + 20.0 * channels + 1.0));
    hipLaunchKernelGGL(k_rectify_sample, dim3(blocks_of(cells, kRectifyThreads)), dim3(kRectifyThreads), 0, st, images, n_views, channels, pix, cells, rgb,
                       valid);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_rectify_view_dirs(const spnerf_ortho_grid* grid, const double* cameras, int32_t n_views, double alt_lo,
                                            double alt_hi, float* dirs, float* spread, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grid && cameras && dirs && spread, "rectify_view_dirs: NULL grid, cameras, dirs or spread");
    SPN_TRY(check_grid("rectify_view_dirs", grid));
    SPN_TRY(check_views("rectify_view_dirs", n_views));
    SPN_ARG(std::isfinite(alt_lo) && std::isfinite(alt_hi) && alt_hi > alt_lo, "rectify_view_dirs: alt_hi %g must be above alt_lo %g",
            alt_hi, alt_lo);
    ViewDirArgs g{};
    g.cams = cameras; g.dirs = dirs; g.spread = spread;
    const double w = grid->xsize * grid->resolution, h = grid->ysize * grid->resolution;
    g.e[0] = grid->xoff + w / 2.0;
    g.n[0] = grid->ytop - h / 2.0;
    for (int p = 0; p < 4; ++p) {   // north-west, north-east, south-west, south-east
        g.e[1 + p] = p & 1 ? grid->xoff + w : grid->xoff;
        g.n[1 + p] = p & 2 ? grid->ytop - h : grid->ytop;
    }
    g.alt_lo = alt_lo; g.alt_hi = alt_hi; g.zone = grid->zone; g.south = grid->south ? 1 : 0;
    ProfScope prof("rectify_view_dirs", st, 0.0, (double)n_views * (8.0 * kCam + 16.0));
    hipLaunchKernelGGL(k_rectify_view_dirs, dim3(n_views), dim3(64), 0, st, g);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_rectify_mosaic(const float* rgb, const uint8_t* usable, int32_t n_views, int64_t cells, int32_t channels,
                                         int32_t mode, float* mosaic, int32_t* count, float* spread, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(rgb && usable && mosaic && count && spread, "rectify_mosaic: NULL rgb, usable, mosaic, count or spread");
    SPN_ARG(cells >= 1 && cells <= ((int64_t)1 << 32), "rectify_mosaic: cells %lld outside [1, 2^32]", (long long)cells);
    SPN_TRY(check_views("rectify_mosaic", n_views));
    SPN_TRY(check_channels("rectify_mosaic", channels));
    SPN_ARG(mode == SPNERF_RECTIFY_MEAN || mode == SPNERF_RECTIFY_MEDIAN, "rectify_mosaic: mode %d is neither 0 (mean) nor 1 (median)",
            mode);
    ProfScope prof("rectify_mosaic", st, 0.0, (double)cells * (n_views * (4.0 * channels + 1.0) + 4.0 * channels + 8.0));
    hipLaunchKernelGGL(k_rectify_mosaic, dim3(blocks_of(cells, kRectifyThreads)), dim3(kRectifyThreads), 0, st, rgb, usable, n_views, cells, channels, mode,
                       mosaic, count, spread);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
