// The device functions and the fused kernel of the plane sweep (include/spnerf_amd_sweep.h), shared by
// sweep.hip (the ungated instances), occlusion.hip (the instances gated by a visibility floor,
// include/spnerf_amd_occlusion.h) and surface.hip (the instances around a base surface,
// include/spnerf_amd_surface.h).  A translation unit includes this under a file-scope
// `#pragma clang fp contract(off)`: the header's operation order is the result, and a device function
// gives the same bits in every kernel that uses it.
//  * grey_cell — one (view, cell) at one altitude: project_packed, sample_cell (csrc/rectify_cell.h), the
//    channel mean.  Instantiated on the channel count, so the channel values stay in registers.
//  * score_cell<VMAX> — the header's three passes over one cell's window (mean; centred squares; S), the
//    greys read through an accessor: global planes (k_sweep_score) or the LDS tile (k_sweep).  mu_v and
//    sqrt(ss_v) live in arrays indexed by the fully unrolled view loop, i.e. in registers: the kernels are
//    instantiated for VMAX = 4, 8 and 16 and views at or beyond V are predicated off.
//  * k_sweep<VMAX, GATED, SURFACE> — one workgroup of 256 threads per 16 x 16 tile.  The inverse UTM of the
//    (16 + 2r)² cells of tile and halo once, lat / lon kept in LDS.  Per plane: each wavefront takes runs of
//    64 halo cells of one view (the view is wavefront-uniform, so camera and image table arrive by scalar
//    loads) and writes grey[v][halo cell] to LDS, NaN standing for invalid; barrier; each thread scores its
//    own cell from LDS; barrier.  LDS: 16·side² B of lat / lon + 4·V·side² B of greys, 45 KB at r = 4,
//    V = 16.  GATED: the floors of tile and halo are read once, into 4·V·side² B more of LDS, and a lane
//    whose (view, halo cell) is gated at the plane writes NaN without projecting or reading the image; the
//    projection sits in a divergent region, which a wavefront with no live lane branches over.  SURFACE
//    (include/spnerf_amd_surface.h): plane k is the surface base + (alt_lo + k·step); the bases of tile and halo
//    are read once, into 4·side² B more of LDS, NaN outside the grid, and a lane whose base is not finite writes
//    NaN the same way.  `prior` is the floor of a GATED instance and the base of a SURFACE one; no instance is both.
#pragma once
#include <cmath>

#include "common.h"

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

// dynamic LDS: lat [hc], lon [hc] fp64, then grey [V][hc] fp32 and, GATED, floor [V][hc] fp32 or, SURFACE, base [hc] fp32;
// hc = (kTile + 2·radius)².
// GATED: view v at a cell is invalid at plane k when (alt_k + slack) < (double)prior[v][cell], prior [V][ysize][xsize] fp32.
// SURFACE: the altitude of a cell at plane k is (double)prior[cell] + alt_k, prior [ysize][xsize] fp32, every view invalid
// where that base is not finite; the picked altitude is lifted by the cell's base, (float)((double)base + (double)altitude).
template <int VMAX, bool GATED, bool SURFACE>
__global__ __launch_bounds__(kSweepThreads) void k_sweep(SweepArgs g, int tx, const double* __restrict__ cams,
                                                         const spnerf_rectify_image* __restrict__ images, float* __restrict__ altitude,
                                                         float* __restrict__ score, int32_t* __restrict__ index,
                                                         uint8_t* __restrict__ views, float* __restrict__ volume,
                                                         const float* __restrict__ prior, double slack) {
    static_assert(!(GATED && SURFACE), "a gated surface sweep is not there");
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
    float* s_prior = s_grey + g.V * hc;
    if constexpr (GATED) {
        // the floors of tile and halo, once for all planes; outside the grid NaN, which gates nothing (and lat is NaN there)
        for (int e = tid; e < g.V * hc; e += kSweepThreads) {
            const int v = e / hc, h = e - v * hc;
            const int j = tj0 - r + h / side, i = ti0 - r + h % side;
            float f = NAN;
            if (j >= 0 && j < g.ysize && i >= 0 && i < g.xsize) f = prior[((int64_t)v * g.ysize + j) * g.xsize + i];
            s_prior[e] = f;
        }
    }
    if constexpr (SURFACE) {
        // the bases of tile and halo, once for all planes; outside the grid NaN (and lat is NaN there)
        for (int h = tid; h < hc; h += kSweepThreads) {
            const int j = tj0 - r + h / side, i = ti0 - r + h % side;
            float b = NAN;
            if (j >= 0 && j < g.ysize && i >= 0 && i < g.xsize) b = prior[(int64_t)j * g.xsize + i];
            s_prior[h] = b;
        }
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
        double reach = 0.0;
        if constexpr (GATED) reach = alt + slack;
        for (int item = wave; item < g.V * runs; item += kSweepThreads / 64) {
            const int v = __builtin_amdgcn_readfirstlane(item / runs);
            const int h = (item % runs) * 64 + lane;
            if (h < hc) {
                const double lat = s_lat[h];
                float grey = NAN;
                bool live = lat == lat;
                if constexpr (GATED) live = live && !(reach < (double)s_prior[v * hc + h]);   // a NaN floor gates nothing
                double at = alt;
                if constexpr (SURFACE) {
                    const float b = s_prior[h];
                    live = live && isfinite(b);
                    at = (double)b + alt;
                }
                if (live) {
                    bool ok;
                    grey = grey_cell(cams + (int64_t)v * kCam, images[v], g.C, lat, s_lon[h], at, ok);
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
        float a = p.altitude(g.K, g.alt_lo, g.step);
        if constexpr (SURFACE) a = (float)((double)s_prior[(tid / kTile + r) * side + tid % kTile + r] + (double)a);
        altitude[cell] = a;
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

// fp64 operations of one projection, read and channel mean (four 20-term cubics at 64, the
// normalisation, the bilinear read of C channels) and of one cell's score (a division counts as one)
static double grey_flop(int C) { return 4.0 * 64.0 + 12.0 + 4.0 + 8.0 * C + C; }
static double score_flop(int V, int radius) {
    const double n = (2.0 * radius + 1.0) * (2.0 * radius + 1.0);
    return V * 7.0 * n + 2.0 * n;
}

// The fused launch of both translation units: the arguments checked as spnerf_sweep states them, the
// instance chosen by the view count.  `prior` is the floor [V][ysize][xsize] of the gated instances and the base
// [ysize][xsize] of the surface instances; `slack` is read by the gated instances only.
template <bool GATED, bool SURFACE = false>
static int32_t launch_sweep(const char* who, const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                            int32_t n_views, int32_t channels, double alt_lo, double step, int32_t n_planes, int32_t radius,
                            int32_t min_views, double min_std, float* altitude, float* score, int32_t* index, uint8_t* views,
                            float* volume, const float* prior, double slack, hipStream_t st) {
    SPN_TRY(check_grid(who, grid));
    SPN_TRY(check_views_channels(who, n_views, channels));
    SPN_TRY(check_planes(who, n_planes, alt_lo, step));
    SPN_TRY(check_window(who, n_views, radius, min_views, min_std));
    SweepArgs g{};
    g.xoff = grid->xoff; g.ytop = grid->ytop; g.res = grid->resolution; g.alt_lo = alt_lo; g.step = step; g.min_std = min_std;
    g.xsize = grid->xsize; g.ysize = grid->ysize; g.zone = grid->zone; g.south = grid->south ? 1 : 0;
    g.V = n_views; g.C = channels; g.K = n_planes; g.radius = radius; g.min_views = min_views;
    int tx;
    const unsigned tiles = tiles_of(g.ysize, g.xsize, tx);
    const int side = kTile + 2 * radius, hc = side * side;
    // ungated at most 46,080 B, a surface sweep 2,304 B more; gated at most 82,944 B, above the 64 KiB a launch gets unasked
    const size_t lds = (size_t)hc * (16 + (GATED ? 8 : 4) * (size_t)n_views + (SURFACE ? 4 : 0));
    const double cells = (double)g.xsize * g.ysize;
    ProfScope prof(who, st, (double)n_planes * ((double)tiles * hc * n_views * grey_flop(channels) + cells * score_flop(n_views, radius)),
                   cells * (13.0 + (volume ? 4.0 * n_planes : 0.0)) + (GATED ? 4.0 * (double)tiles * hc * n_views : 0.0) +
                       (SURFACE ? 4.0 * (double)tiles * hc : 0.0));
    auto launch = [&](auto kernel) -> int32_t {
        if (lds > 65536) SPN_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kSweepThreads), lds, st, g, tx, cameras, images, altitude, score, index, views, volume,
                           prior, slack);
        SPN_HIP(hipGetLastError());
        return SPNERF_OK;
    };
    if (n_views <= 4) return launch(k_sweep<4, GATED, SURFACE>);
    if (n_views <= 8) return launch(k_sweep<8, GATED, SURFACE>);
    return launch(k_sweep<16, GATED, SURFACE>);
}

}  // namespace spn
