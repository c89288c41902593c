// Geometric shadows over a ground-grid DSM (include/spnerf_amd_shadow.h): the DSM cast under K sun
// directions, and the agreement of a learnt sun plane with the result.
//  * k_shadow_hmax — the maximum of the non-NaN heights, per-workgroup partials (a maximum does not
//    depend on the order, so every consumer reduces the partials itself).
//  * k_shadow_cast — one thread per (direction, cell), a wavefront on 64 neighbouring cells of a row
//    and a workgroup on 4 neighbouring rows, so that the wavefront's samples at step m lie on one or
//    two rows (column-major marches) or on one row (row-major ones) of a DSM that fits in L2: plain
//    cached loads.  The march of a cell is a DDA along the major axis of the sun's azimuth; it stops
//    as soon as no later step can change the outputs (the bound from hmax).  Latency-bound: two
//    dependent loads and a dozen fp64 operations per step.  The march itself is csrc/shadow_march.h's,
//    shared with the visibility floor (occlusion.hip).
//    Nothing is fused (#pragma clang fp contract(off), honoured under the Makefile's
//    -ffp-contract=fast-honor-pragmas): every product and sum is rounded once, as the numpy statement
//    (tests/shadow_numpy.py) rounds them, so floor(y) never flips against it.
//  * k_shadow_agreement / k_shadow_agreement_finish — one pass over a sun plane and a shadow plane:
//    fp64 sums and int64 counts per direction, built like k_view_metrics (csrc/view.hip).
#include <cmath>

#include "../../include/spnerf_amd_shadow.h"
#include "common.h"
#include "shadow_march.h"
#include "wave.h"

namespace spn {

constexpr int kShadowDirsPerLaunch = 32;  // the marches of a launch travel as kernel arguments

int hmax_parts(int64_t cells) {
    const int64_t nb = (cells + 4 * kShadowThreads - 1) / (4 * kShadowThreads);
    return (int)(nb < kShadowMaxParts ? nb : kShadowMaxParts);
}

__global__ __launch_bounds__(kShadowThreads) void k_shadow_hmax(const double* __restrict__ dsm, int64_t cells,
                                                               double* __restrict__ part) {
    __shared__ double s_max[kShadowThreads / 64];
    const int tid = threadIdx.x;
    double v = -INFINITY;
    for (int64_t c = (int64_t)blockIdx.x * kShadowThreads + tid; c < cells; c += (int64_t)gridDim.x * kShadowThreads) {
        const double x = dsm[c];
        if (x == x) v = fmax(v, x);
    }
    v = wave_max(v);
    if ((tid & 63) == 0) s_max[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kShadowThreads / 64; ++w) v = fmax(v, s_max[w]);
        part[blockIdx.x] = v;
    }
}

void launch_shadow_hmax(const double* dsm, int64_t cells, double* part, hipStream_t st) {
    hipLaunchKernelGGL(k_shadow_hmax, dim3(hmax_parts(cells)), dim3(kShadowThreads), 0, st, dsm, cells, part);
}

struct ShadowArgs {
    const double* dsm;
    const double* part;
    uint8_t* shadow;   // [n_dirs][H][W], the launch's first direction at entry 0
    double* excess;    // likewise, or NULL
    int H, W, nparts, tiles_x;
    ShadowDir d[kShadowDirsPerLaunch];
};

__global__ __launch_bounds__(kShadowThreads) void k_shadow_cast(ShadowArgs g) {
    __shared__ double s_hmax;
    const int tid = threadIdx.x;
    const double hmax = block_hmax(g.part, g.nparts, &s_hmax);
    const int i = (int)(blockIdx.x % g.tiles_x) * kShadowTileW + (tid & (kShadowTileW - 1));
    const int j = (int)(blockIdx.x / g.tiles_x) * kShadowTileH + tid / kShadowTileW;
    if (i >= g.W || j >= g.H) return;
    const int64_t cell = (int64_t)j * g.W + i;
    const int64_t o = (int64_t)blockIdx.y * g.H * g.W + cell;
    const double h = g.dsm[cell];
    if (h != h) {
        g.shadow[o] = 255;
        if (g.excess) g.excess[o] = h;
        return;
    }
    const bool want = g.excess != nullptr;
    const double run = shadow_march(g.dsm, g.H, g.W, j, i, g.d[blockIdx.y], hmax, h, want);
    g.shadow[o] = run > 0.0 ? 1 : 0;
    if (want) g.excess[o] = run;
}

// ---- agreement of a learnt sun plane with the cast shadows -----------------------------------------

constexpr int kAgreeThreads = 256;
constexpr int kAgreeMaxBlocks = 256;   // per direction; also the finish's summation length

static int agree_blocks(int64_t cells) {
    const int64_t nb = (cells + kAgreeThreads - 1) / kAgreeThreads;
    return (int)(nb < kAgreeMaxBlocks ? nb : kAgreeMaxBlocks);
}

// part[(k·nb + b)] is workgroup b's share of direction k
__global__ __launch_bounds__(kAgreeThreads) void k_shadow_agreement(const float* __restrict__ sun,
                                                                    const uint8_t* __restrict__ shadow, int64_t cells,
                                                                    spnerf_shadow_agreement_result* __restrict__ part) {
    __shared__ double s_f[kAgreeThreads / 64][3];
    __shared__ int64_t s_n[kAgreeThreads / 64][5];
    const int tid = threadIdx.x, k = blockIdx.y;
    const float* sv = sun + (int64_t)k * cells;
    const uint8_t* sh = shadow + (int64_t)k * cells;
    double f[3] = {0.0, 0.0, 0.0};        // sum_sun_lit, sum_sun_shadow, sum_abs
    int64_t n[5] = {0, 0, 0, 0, 0};       // n_lit, n_shadow, tp, fp, fn
    for (int64_t c = (int64_t)blockIdx.x * kAgreeThreads + tid; c < cells; c += (int64_t)gridDim.x * kAgreeThreads) {
        const int s = sh[c];
        const float x = sv[c];
        if (s > 1 || !(fabsf(x) < INFINITY)) continue;
        const double v = (double)x;
        const bool dark = x < 0.5f;
        f[s] += v;
        f[2] += fabs(v - (double)(1 - s));
        n[s] += 1;
        n[2] += (s == 1 && dark);
        n[3] += (s == 0 && dark);
        n[4] += (s == 1 && !dark);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) f[a] = wave_sum(f[a]);
#pragma unroll
    for (int a = 0; a < 5; ++a) n[a] = wave_sum(n[a]);
    if ((tid & 63) == 0) {
        for (int a = 0; a < 3; ++a) s_f[tid >> 6][a] = f[a];
        for (int a = 0; a < 5; ++a) s_n[tid >> 6][a] = n[a];
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kAgreeThreads / 64; ++w) {   // wavefront order
            for (int a = 0; a < 3; ++a) f[a] += s_f[w][a];
            for (int a = 0; a < 5; ++a) n[a] += s_n[w][a];
        }
        spnerf_shadow_agreement_result r;
        r.sum_sun_lit = f[0]; r.sum_sun_shadow = f[1]; r.sum_abs = f[2];
        r.n_lit = n[0]; r.n_shadow = n[1]; r.tp = n[2]; r.fp = n[3]; r.fn = n[4];
        part[(int64_t)k * gridDim.x + blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(kAgreeThreads) void k_shadow_agreement_finish(const spnerf_shadow_agreement_result* __restrict__ part,
                                                                           int nblocks, int n_dirs,
                                                                           spnerf_shadow_agreement_result* __restrict__ res) {
    for (int k = threadIdx.x; k < n_dirs; k += kAgreeThreads) {
        spnerf_shadow_agreement_result t = part[(int64_t)k * nblocks];
        for (int b = 1; b < nblocks; ++b) {   // workgroup order
            const spnerf_shadow_agreement_result p = part[(int64_t)k * nblocks + b];
            t.sum_sun_lit += p.sum_sun_lit; t.sum_sun_shadow += p.sum_sun_shadow; t.sum_abs += p.sum_abs;
            t.n_lit += p.n_lit; t.n_shadow += p.n_shadow; t.tp += p.tp; t.fp += p.fp; t.fn += p.fn;
        }
        res[k] = t;
    }
}

static int32_t check_grid(const char* who, int32_t height, int32_t width) {
    SPN_ARG(height > 0 && width > 0, "%s: grid of %d x %d cells", who, width, height);
    SPN_ARG(height <= (1 << 30) && width <= (1 << 30) && (int64_t)height * width <= ((int64_t)1 << 36),
            "%s: grid of %d x %d cells is too large for one call", who, width, height);
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_shadow_abi_version(void) { return SPNERF_SHADOW_ABI_VERSION; }

extern "C" int64_t spnerf_shadow_workspace_bytes(int32_t height, int32_t width) {
    SPN_TRY(check_grid("shadow_workspace_bytes", height, width));
    return (int64_t)align16((size_t)hmax_parts((int64_t)height * width) * sizeof(double));
}

extern "C" int32_t spnerf_shadow_cast(const double* dsm, int32_t height, int32_t width, double resolution, const float* dirs,
                                      int32_t n_dirs, void* workspace, uint8_t* shadow, double* excess, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(dsm && dirs && workspace && shadow, "shadow_cast: NULL dsm, dirs, workspace or shadow");
    SPN_TRY(check_grid("shadow_cast", height, width));
    SPN_ARG(n_dirs > 0 && n_dirs <= SPNERF_SHADOW_MAX_DIRS, "shadow_cast: n_dirs %d outside [1, %d]", n_dirs, SPNERF_SHADOW_MAX_DIRS);
    SPN_ARG(resolution > 0.0 && std::isfinite(resolution), "shadow_cast: resolution %g", resolution);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "shadow_cast: workspace not 16-byte aligned");
    for (int k = 0; k < n_dirs; ++k) {
        const float* s = dirs + 3 * k;
        SPN_ARG(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]), "shadow_cast: direction %d is not finite", k);
        SPN_ARG(s[2] > 0.f, "shadow_cast: direction %d has up %g: the sun must stand above the horizon", k, (double)s[2]);
    }
    const int64_t cells = (int64_t)height * width;
    const int tiles_x = (width + kShadowTileW - 1) / kShadowTileW;
    const int64_t tiles = (int64_t)tiles_x * ((height + kShadowTileH - 1) / kShadowTileH);
    SPN_ARG(tiles <= 0x7fffffffLL, "shadow_cast: grid of %d x %d cells is too large for one call", width, height);
    const int nparts = hmax_parts(cells);
    ProfScope prof("shadow", st, 0.0, (double)cells * (8.0 + n_dirs * (excess ? 9.0 : 1.0)));
    launch_shadow_hmax(dsm, cells, (double*)workspace, st);
    SPN_HIP(hipGetLastError());
    for (int k0 = 0; k0 < n_dirs; k0 += kShadowDirsPerLaunch) {
        const int nk = n_dirs - k0 < kShadowDirsPerLaunch ? n_dirs - k0 : kShadowDirsPerLaunch;
        ShadowArgs g{};
        g.dsm = dsm; g.part = (const double*)workspace; g.nparts = nparts;
        g.shadow = shadow + (int64_t)k0 * cells;
        g.excess = excess ? excess + (int64_t)k0 * cells : nullptr;
        g.H = height; g.W = width; g.tiles_x = tiles_x;
        for (int k = 0; k < nk; ++k) g.d[k] = shadow_dir(dirs + 3 * (k0 + k), resolution);
        hipLaunchKernelGGL(k_shadow_cast, dim3((unsigned)tiles, (unsigned)nk), dim3(kShadowThreads), 0, st, g);
        SPN_HIP(hipGetLastError());
    }
    return SPNERF_OK;
}

extern "C" int64_t spnerf_shadow_agreement_workspace_bytes(int64_t cells, int32_t n_dirs) {
    SPN_ARG(cells >= 1, "shadow_agreement_workspace_bytes: cells %lld must be positive", (long long)cells);
    SPN_ARG(n_dirs > 0 && n_dirs <= SPNERF_SHADOW_MAX_DIRS, "shadow_agreement_workspace_bytes: n_dirs %d outside [1, %d]", n_dirs,
            SPNERF_SHADOW_MAX_DIRS);
    return (int64_t)align16((size_t)agree_blocks(cells) * n_dirs * sizeof(spnerf_shadow_agreement_result));
}

extern "C" int32_t spnerf_shadow_agreement(const float* sun, const uint8_t* shadow, int64_t cells, int32_t n_dirs,
                                           void* workspace, spnerf_shadow_agreement_result* result, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(sun && shadow && workspace && result, "shadow_agreement: NULL sun, shadow, workspace or result");
    SPN_ARG(cells >= 1, "shadow_agreement: cells %lld must be positive", (long long)cells);
    SPN_ARG(n_dirs > 0 && n_dirs <= SPNERF_SHADOW_MAX_DIRS, "shadow_agreement: n_dirs %d outside [1, %d]", n_dirs,
            SPNERF_SHADOW_MAX_DIRS);
    SPN_ARG(cells <= ((int64_t)1 << 40) / n_dirs, "shadow_agreement: %d x %lld cells in one call", n_dirs, (long long)cells);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "shadow_agreement: workspace not 16-byte aligned");
    const int nb = agree_blocks(cells);
    spnerf_shadow_agreement_result* part = (spnerf_shadow_agreement_result*)workspace;
    ProfScope prof("shadow_agreement", st, 0.0, 5.0 * (double)cells * n_dirs);
    hipLaunchKernelGGL(k_shadow_agreement, dim3(nb, n_dirs), dim3(kAgreeThreads), 0, st, sun, shadow, cells, part);
    SPN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_shadow_agreement_finish, dim3(1), dim3(kAgreeThreads), 0, st, part, nb, n_dirs, result);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
