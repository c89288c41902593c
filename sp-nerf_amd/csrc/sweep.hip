// Plane sweep (include/spnerf_amd_sweep.h): a photo-consistency DSM on the ground grid from the camera
// images alone.  The whole translation unit is compiled without fused multiply-adds (the file-scope
// pragma below, honoured under the Makefile's -ffp-contract=fast-honor-pragmas), so the header's
// operation order is the result and a device function gives the same bits in every kernel that uses it.
//  * grey_cell — one (view, cell) at one altitude: project_packed, sample_cell (csrc/rectify_cell.h), the
//    channel mean.  Instantiated on the channel count, so the channel values stay in registers.
//  * score_cell<VMAX> — the header's three passes over one cell's window (mean; centred squares; S), the
//    greys read through an accessor: global planes (k_sweep_score) or the LDS tile (k_sweep).  mu_v and
//    sqrt(ss_v) live in arrays indexed by the fully unrolled view loop, i.e. in registers: the kernels are
//    instantiated for VMAX = 4, 8 and 16 and views at or beyond V are predicated off.
//  * Pick (csrc/sweep_pick.h) — the running best of a cell and the scores of its two neighbouring planes, fed
//    plane by plane: from a stored volume (k_sweep_pick) or as the planes are scored (k_sweep).
//  * k_sweep — one workgroup of 256 threads per 16 x 16 tile.  The inverse UTM of the (16 + 2r)² cells of tile
//    and halo once, lat / lon kept in LDS.  Per plane: each wavefront takes runs of 64 halo cells of one
//    view (the view is wavefront-uniform, so camera and image table arrive by scalar loads) and writes
//    grey[v][halo cell] to LDS, NaN standing for invalid; barrier; each thread scores its own cell from
//    LDS; barrier.  LDS: 16·side² B of lat / lon + 4·V·side² B of greys, 45 KB at r = 4, V = 16.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "../../include/spnerf_amd_sweep.h"
#include "rectify_cell.h"
#include "sweep_pick.h"
#include "utm.h"

namespace spn {

constexpr int kTile = SPNERF_SWEEP_TILE;
constexpr int kSweepThreads = kTile * kTile;
static_assert(kSweepThreads == 256, "a tile is one 256-thread workgroup");

template <int C>
__device__ __forceinline__ float grey_channels(const double* __restrict__ cam, const spnerf_rectify_image im, double lat, double lon,
                                               double alt, bool& valid) {
    double col, row;
    project_packed(cam, lat, lon, alt, col, row);
    float px[C];
    const bool ok = sample_cell(im, C, col, row, px);
    double s = (double)px[0];
#pragma unroll
    for (int c = 1; c < C; ++c) s += (double)px[c];
    const float g = (float)(s / (double)C);
    valid = ok && isfinite(g);
    return g;
}

// the grey of one view at one cell (its lat / lon) and altitude; C is wavefront-uniform
__device__ __forceinline__ float grey_cell(const double* __restrict__ cam, const spnerf_rectify_image im, int C, double lat, double lon,
                                           double alt, bool& valid) {
    switch (C) {
        case 1: return grey_channels<1>(cam, im, lat, lon, alt, valid);
        case 2: return grey_channels<2>(cam, im, lat, lon, alt, valid);
        case 3: return grey_channels<3>(cam, im, lat, lon, alt, valid);
        default: return grey_channels<4>(cam, im, lat, lon, alt, valid);
    }
}

// stored planes [V][ysize][xsize]; (j, i) are grid coordinates
struct GlobalGreys {
    const float* __restrict__ grey;
    const uint8_t* __restrict__ valid;
    int64_t cells;
    int xsize;
    __device__ __forceinline__ float g(int v, int j, int i) const { return grey[v * cells + (int64_t)j * xsize + i]; }
    __device__ __forceinline__ bool ok(int v, int j, int i) const { return valid[v * cells + (int64_t)j * xsize + i] == 1; }
};

// the LDS tile [V][side][side]; (j, i) are tile-and-halo coordinates; an invalid cell holds NaN
struct LdsGreys {
    const float* grey;
    int hc, side;
    __device__ __forceinline__ float g(int v, int j, int i) const { return grey[v * hc + j * side + i]; }
    __device__ __forceinline__ bool ok(int v, int j, int i) const {
        const float x = g(v, j, i);
        return x == x;
    }
};

// the score of the cell whose clipped window is rows j0..j1, columns i0..i1 of `a`; m: its usable views
template <int VMAX, class Greys>
__device__ __forceinline__ float score_cell(const Greys& a, int V, int j0, int j1, int i0, int i1, int min_views, double min_std,
                                            int& m) {
    const int n = (j1 - j0 + 1) * (i1 - i0 + 1);
    m = 0;
    if (n < 2) return NAN;
    const double dn = (double)n, floor_ss = dn * (min_std * min_std);
    double mu[VMAX], norm[VMAX];
    unsigned use = 0;
#pragma unroll
    for (int v = 0; v < VMAX; ++v) {
        mu[v] = 0.0;
        norm[v] = 1.0;
        if (v < V) {
            bool ok = true;
            double sum = 0.0;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) {
                    ok = ok && a.ok(v, j, i);
                    sum += (double)a.g(v, j, i);
                }
            const double mean = sum / dn;
            double ss = 0.0;
            for (int j = j0; j <= j1; ++j)
                for (int i = i0; i <= i1; ++i) {
                    const double d = (double)a.g(v, j, i) - mean;
                    ss += d * d;
                }
            if (ok && ss > floor_ss) {   // a NaN fails the comparison
                use |= 1u << v;
                ++m;
                mu[v] = mean;
                norm[v] = sqrt(ss);
            }
        }
    }
    if (m < min_views) return NAN;
    double acc = 0.0;
    for (int j = j0; j <= j1; ++j)
        for (int i = i0; i <= i1; ++i) {
            double S = 0.0;
#pragma unroll
            for (int v = 0; v < VMAX; ++v)
                if (use >> v & 1) S += ((double)a.g(v, j, i) - mu[v]) / norm[v];
            acc += S * S;
        }
    return (float)((acc - (double)m) / ((double)m * (double)(m - 1)));
}

struct SweepArgs {
    double xoff, ytop, res, alt_lo, step, min_std;
    int xsize, ysize, zone, south, V, C, K, radius, min_views;
};

// tile b of a grid whose rows hold `tx` tiles: its first row and column
__device__ __forceinline__ void tile_origin(unsigned b, int tx, int& tj0, int& ti0) {
    tj0 = (int)(b / (unsigned)tx) * kTile;
    ti0 = (int)(b % (unsigned)tx) * kTile;
}

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

// dynamic LDS: lat [hc], lon [hc] fp64, then grey [V][hc] fp32, hc = (kTile + 2·radius)²
template <int VMAX>
__global__ __launch_bounds__(kSweepThreads) void k_sweep(SweepArgs g, int tx, const double* __restrict__ cams,
                                                         const spnerf_rectify_image* __restrict__ images, float* __restrict__ altitude,
                                                         float* __restrict__ score, int32_t* __restrict__ index,
                                                         uint8_t* __restrict__ views, float* __restrict__ volume) {
    extern __shared__ double s_mem[];
    const int r = g.radius, side = kTile + 2 * r, hc = side * side;
    double* s_lat = s_mem;
    double* s_lon = s_mem + hc;
    float* s_grey = reinterpret_cast<float*>(s_mem + 2 * hc);
    const int tid = (int)threadIdx.x;
    int tj0, ti0;
    tile_origin(blockIdx.x, tx, tj0, ti0);

    // the inverse UTM of tile and halo, once; a halo cell outside the grid is NaN: no window reads it
    for (int h = tid; h < hc; h += kSweepThreads) {
        const int j = tj0 - r + h / side, i = ti0 - r + h % side;
        double lat = NAN, lon = NAN;
        if (j >= 0 && j < g.ysize && i >= 0 && i < g.xsize)
            utm_inverse(g.xoff + ((double)i + 0.5) * g.res, g.ytop - ((double)j + 0.5) * g.res, g.zone, g.south, &lat, &lon);
        s_lat[h] = lat;
        s_lon[h] = lon;
    }
    __syncthreads();

    const int j = tj0 + tid / kTile, i = ti0 + tid % kTile;
    const bool mine = j < g.ysize && i < g.xsize;
    const int64_t cells = (int64_t)g.xsize * g.ysize, cell = (int64_t)j * g.xsize + i;
    // the clipped window in tile-and-halo coordinates
    const int j0 = max(j - r, 0) - (tj0 - r), j1 = min(j + r, g.ysize - 1) - (tj0 - r);
    const int i0 = max(i - r, 0) - (ti0 - r), i1 = min(i + r, g.xsize - 1) - (ti0 - r);
    const LdsGreys a{s_grey, hc, side};
    const int runs = (hc + 63) / 64, wave = tid >> 6, lane = tid & 63;
    Pick p;
    for (int k = 0; k < g.K; ++k) {
        const double alt = g.alt_lo + (double)k * g.step;
        for (int item = wave; item < g.V * runs; item += kSweepThreads / 64) {
            const int v = __builtin_amdgcn_readfirstlane(item / runs);
            const int h = (item % runs) * 64 + lane;
            if (h < hc) {
                const double lat = s_lat[h];
                float grey = NAN;
                if (lat == lat) {
                    bool ok;
                    grey = grey_cell(cams + (int64_t)v * kCam, images[v], g.C, lat, s_lon[h], alt, ok);
                    if (!ok) grey = NAN;
                }
                s_grey[v * hc + h] = grey;
            }
        }
        __syncthreads();
        if (mine) {
            int m;
            const float s = score_cell<VMAX>(a, g.V, j0, j1, i0, i1, g.min_views, g.min_std, m);
            p.plane(k, s, m);
            if (volume) volume[k * cells + cell] = s;
        }
        __syncthreads();   // the next plane overwrites the greys
    }
    if (mine) {
        altitude[cell] = p.altitude(g.K, g.alt_lo, g.step);
        score[cell] = p.best;
        index[cell] = p.index;
        views[cell] = (uint8_t)p.m;
    }
}

static int32_t check_views_channels(const char* who, int32_t n_views, int32_t channels) {
    SPN_ARG(n_views >= SPNERF_SWEEP_MIN_VIEWS && n_views <= SPNERF_SWEEP_MAX_VIEWS, "%s: n_views %d outside [%d, %d]", who, n_views,
            SPNERF_SWEEP_MIN_VIEWS, SPNERF_SWEEP_MAX_VIEWS);
    SPN_ARG(channels > 0 && channels <= SPNERF_RECTIFY_MAX_CHANNELS, "%s: channels %d outside [1, %d]", who, channels,
            SPNERF_RECTIFY_MAX_CHANNELS);
    return SPNERF_OK;
}

static int32_t check_window(const char* who, int32_t n_views, int32_t radius, int32_t min_views, double min_std) {
    SPN_ARG(radius >= 1 && radius <= SPNERF_SWEEP_MAX_RADIUS, "%s: radius %d outside [1, %d]", who, radius, SPNERF_SWEEP_MAX_RADIUS);
    SPN_ARG(min_views >= 2 && min_views <= n_views, "%s: min_views %d outside [2, %d]", who, min_views, n_views);
    SPN_ARG(min_std >= 0.0 && std::isfinite(min_std), "%s: min_std %g must be finite and >= 0", who, min_std);
    return SPNERF_OK;
}

static int32_t check_planes(const char* who, int32_t n_planes, double alt_lo, double step) {
    SPN_ARG(n_planes >= 1 && n_planes <= SPNERF_SWEEP_MAX_PLANES, "%s: n_planes %d outside [1, %d]", who, n_planes, SPNERF_SWEEP_MAX_PLANES);
    SPN_ARG(std::isfinite(alt_lo), "%s: alt_lo %g is not finite", who, alt_lo);
    SPN_ARG(step > 0.0 && std::isfinite(step), "%s: step %g must be finite and > 0", who, step);
    return SPNERF_OK;
}

static unsigned tiles_of(int32_t ysize, int32_t xsize, int& tx) {
    tx = (xsize + kTile - 1) / kTile;
    return (unsigned)((int64_t)tx * ((ysize + kTile - 1) / kTile));   // below 2^29 for a grid of at most 2^32 cells
}

static unsigned blocks_of(int64_t cells) { return (unsigned)((cells + kSweepThreads - 1) / kSweepThreads); }

// fp64 operations of one projection, read and channel mean (four 20-term cubics at 64, the
// normalisation, the bilinear read of C channels) and of one cell's score (a division counts as one)
static double grey_flop(int C) { return 4.0 * 64.0 + 12.0 + 4.0 + 8.0 * C + C; }
static double score_flop(int V, int radius) {
    const double n = (2.0 * radius + 1.0) * (2.0 * radius + 1.0);
    return V * 7.0 * n + 2.0 * n;
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
    hipLaunchKernelGGL(k_sweep_grey, dim3(blocks_of(cells)), dim3(kSweepThreads), 0, st, g, alt, cameras, images, grey, valid);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_sweep_score(const float* grey, const uint8_t* valid, int32_t n_views, int32_t ysize, int32_t xsize,
                                      int32_t radius, int32_t min_views, double min_std, float* score, uint8_t* views, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grey && valid && score && views, "sweep_score: NULL grey, valid, score or views");
    SPN_ARG(xsize > 0 && ysize > 0, "sweep_score: grid of %d x %d cells", xsize, ysize);
    SPN_ARG((int64_t)xsize * ysize <= ((int64_t)1 << 32), "sweep_score: grid of %d x %d cells is too large for one call", xsize, ysize);
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
    hipLaunchKernelGGL(k_sweep_pick, dim3(blocks_of(cells)), dim3(kSweepThreads), 0, st, volume, views_vol, n_planes, cells, alt_lo, step,
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
    SPN_TRY(check_grid("sweep", grid));
    SPN_TRY(check_views_channels("sweep", n_views, channels));
    SPN_TRY(check_planes("sweep", n_planes, alt_lo, step));
    SPN_TRY(check_window("sweep", n_views, radius, min_views, min_std));
    SweepArgs g{};
    g.xoff = grid->xoff; g.ytop = grid->ytop; g.res = grid->resolution; g.alt_lo = alt_lo; g.step = step; g.min_std = min_std;
    g.xsize = grid->xsize; g.ysize = grid->ysize; g.zone = grid->zone; g.south = grid->south ? 1 : 0;
    g.V = n_views; g.C = channels; g.K = n_planes; g.radius = radius; g.min_views = min_views;
    int tx;
    const unsigned tiles = tiles_of(g.ysize, g.xsize, tx);
    const int side = kTile + 2 * radius, hc = side * side;
    const size_t lds = (size_t)hc * (16 + 4 * (size_t)n_views);   // at most 46,080 B
    const double cells = (double)g.xsize * g.ysize;
    ProfScope prof("sweep", st, (double)n_planes * ((double)tiles * hc * n_views * grey_flop(channels) + cells * score_flop(n_views, radius)),
                   cells * (13.0 + (volume ? 4.0 * n_planes : 0.0)));
    if (n_views <= 4)
        hipLaunchKernelGGL(k_sweep<4>, dim3(tiles), dim3(kSweepThreads), lds, st, g, tx, cameras, images, altitude, score, index, views,
                           volume);
    else if (n_views <= 8)
        hipLaunchKernelGGL(k_sweep<8>, dim3(tiles), dim3(kSweepThreads), lds, st, g, tx, cameras, images, altitude, score, index, views,
                           volume);
    else
        hipLaunchKernelGGL(k_sweep<16>, dim3(tiles), dim3(kSweepThreads), lds, st, g, tx, cameras, images, altitude, score, index, views,
                           volume);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
