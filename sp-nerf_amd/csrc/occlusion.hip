// Occlusion (include/spnerf_amd_occlusion.h): the visibility floor of a ground-grid DSM under V lines of
// sight, and the plane sweep gated by it.  Compiled without fused multiply-adds, as sweep.hip is (the
// file-scope pragma below), so the gated sweep has the bits of the staged chain.
//  * k_occlusion_floor — one thread per (view, cell), the workgroup shape of k_shadow_cast (a wavefront on
//    64 neighbouring cells of a row, 4 rows per workgroup) and its march, csrc/shadow_march.h, taken against
//    the reference height 0 with the early stop of the cast's `excess` path: hmax from the partial maxima
//    that shadow.hip's reduction leaves in the workspace.  The cell's own height is not read.
//  * k_occlusion_gate — one thread per (view, cell) of a stored grey / valid pair, in place.
//  * k_sweep<VMAX, true, false> — csrc/sweep_cell.h's fused sweep with the floors of tile and halo in LDS.  LDS and
//    not registers: the lane ↔ (view, halo cell) assignment is the same at every plane, but a lane owns up to
//    VMAX·9/4 = 36 entries at V = 16, r = 4, which would need a fully unrolled, predicated item loop and 36
//    more VGPRs on a 132-VGPR kernel (3 → 2 waves per SIMD), where 4·V·(16 + 2r)² B of LDS cost nothing at the
//    sizes the sweep is run at (V = 4, r = 2: 19 200 B, 8 workgroups per CU by LDS against 4 by registers) and
//    one workgroup per CU instead of three only at V = 16, r = 4 (82 944 B of 160 KiB).
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "../../include/spnerf_amd_occlusion.h"
#include "shadow_march.h"
#include "sweep_cell.h"

namespace spn {

struct FloorArgs {
    const double* dsm;
    const double* part;
    float* floor;   // [n_views][H][W]
    int H, W, nparts, tiles_x;
    ShadowDir d[SPNERF_OCCLUSION_MAX_VIEWS];
};

__global__ __launch_bounds__(kShadowThreads) void k_occlusion_floor(FloorArgs g) {
    __shared__ double s_hmax;
    const int tid = threadIdx.x;
    const double hmax = block_hmax(g.part, g.nparts, &s_hmax);
    const int i = (int)(blockIdx.x % g.tiles_x) * kShadowTileW + (tid & (kShadowTileW - 1));
    const int j = (int)(blockIdx.x / g.tiles_x) * kShadowTileH + tid / kShadowTileW;
    if (i >= g.W || j >= g.H) return;
    const double run = shadow_march(g.dsm, g.H, g.W, j, i, g.d[blockIdx.y], hmax, 0.0, true);
    g.floor[((int64_t)blockIdx.y * g.H + j) * g.W + i] = (float)run;
}

constexpr int kGateThreads = 256;

__global__ __launch_bounds__(kGateThreads) void k_occlusion_gate(float* __restrict__ grey, uint8_t* __restrict__ valid,
                                                                 const float* __restrict__ floor, int64_t n, double alt, double slack) {
    const int64_t e = blockIdx.x * (int64_t)kGateThreads + threadIdx.x;
    if (e >= n) return;
    const double reach = alt + slack;
    if (reach < (double)floor[e]) {   // a NaN floor gates nothing
        grey[e] = NAN;
        valid[e] = 0;
    }
}

static int32_t check_dsm_grid(const char* who, int32_t height, int32_t width) {
    SPN_ARG(height > 0 && width > 0, "%s: grid of %d x %d cells", who, width, height);
    SPN_ARG(height <= (1 << 30) && width <= (1 << 30) && (int64_t)height * width <= ((int64_t)1 << 32),
            "%s: grid of %d x %d cells is too large for one call", who, width, height);
    return SPNERF_OK;
}

static int32_t check_slack(const char* who, double slack) {
    SPN_ARG(slack >= 0.0 && std::isfinite(slack), "%s: slack %g must be finite and >= 0", who, slack);
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_occlusion_abi_version(void) { return SPNERF_OCCLUSION_ABI_VERSION; }

extern "C" int64_t spnerf_occlusion_workspace_bytes(int32_t height, int32_t width) {
    SPN_TRY(check_dsm_grid("occlusion_workspace_bytes", height, width));
    return (int64_t)align16((size_t)hmax_parts((int64_t)height * width) * sizeof(double));
}

extern "C" int32_t spnerf_occlusion_floor(const double* dsm, int32_t height, int32_t width, double resolution, const float* dirs,
                                          int32_t n_views, void* workspace, float* floor, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(dsm && dirs && workspace && floor, "occlusion_floor: NULL dsm, dirs, workspace or floor");
    SPN_TRY(check_dsm_grid("occlusion_floor", height, width));
    SPN_ARG(n_views >= 1 && n_views <= SPNERF_OCCLUSION_MAX_VIEWS, "occlusion_floor: n_views %d outside [1, %d]", n_views,
            SPNERF_OCCLUSION_MAX_VIEWS);
    SPN_ARG(resolution > 0.0 && std::isfinite(resolution), "occlusion_floor: resolution %g", resolution);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "occlusion_floor: workspace not 16-byte aligned");
    FloorArgs g{};
    for (int v = 0; v < n_views; ++v) {
        const float* s = dirs + 3 * v;
        SPN_ARG(std::isfinite(s[0]) && std::isfinite(s[1]) && std::isfinite(s[2]), "occlusion_floor: direction %d is not finite", v);
        SPN_ARG(s[2] > 0.f, "occlusion_floor: direction %d has up %g: the camera must stand above the horizon", v, (double)s[2]);
        g.d[v] = shadow_dir(s, resolution);
    }
    const int64_t cells = (int64_t)height * width;
    g.tiles_x = (width + kShadowTileW - 1) / kShadowTileW;
    const int64_t tiles = (int64_t)g.tiles_x * ((height + kShadowTileH - 1) / kShadowTileH);
    SPN_ARG(tiles <= 0x7fffffffLL, "occlusion_floor: grid of %d x %d cells is too large for one call", width, height);
    g.dsm = dsm; g.part = (const double*)workspace; g.nparts = hmax_parts(cells); g.floor = floor; g.H = height; g.W = width;
    ProfScope prof("occlusion_floor", st, 0.0, (double)cells * (8.0 + 4.0 * n_views));
    launch_shadow_hmax(dsm, cells, (double*)workspace, st);
    SPN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_occlusion_floor, dim3((unsigned)tiles, (unsigned)n_views), dim3(kShadowThreads), 0, st, g);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_occlusion_gate(float* grey, uint8_t* valid, const float* floor, int32_t n_views, int64_t cells, double alt,
                                         double slack, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(grey && valid && floor, "occlusion_gate: NULL grey, valid or floor");
    SPN_ARG(n_views >= 1 && n_views <= SPNERF_OCCLUSION_MAX_VIEWS, "occlusion_gate: n_views %d outside [1, %d]", n_views,
            SPNERF_OCCLUSION_MAX_VIEWS);
    SPN_ARG(cells >= 1 && cells <= ((int64_t)1 << 32), "occlusion_gate: cells %lld outside [1, 2^32]", (long long)cells);
    SPN_ARG(std::isfinite(alt), "occlusion_gate: alt %g is not finite", alt);
    SPN_TRY(check_slack("occlusion_gate", slack));
    const int64_t n = cells * n_views;   // at most 2^36: below 2^28 workgroups
    ProfScope prof("occlusion_gate", st, 0.0, (double)n * 9.0);
    hipLaunchKernelGGL(k_occlusion_gate, dim3((unsigned)((n + kGateThreads - 1) / kGateThreads)), dim3(kGateThreads), 0, st, grey, valid,
                       floor, n, alt, slack);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_occlusion_sweep(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                                          int32_t n_views, int32_t channels, double alt_lo, double step, int32_t n_planes,
                                          int32_t radius, int32_t min_views, double min_std, const float* floor, double slack,
                                          float* altitude, float* score, int32_t* index, uint8_t* views, float* volume, void* stream) {
    SPN_ARG(grid && cameras && images && floor && altitude && score && index && views,
            "occlusion_sweep: NULL grid, cameras, images, floor, altitude, score, index or views");
    SPN_TRY(check_slack("occlusion_sweep", slack));
    return launch_sweep<true>("occlusion_sweep", grid, cameras, images, n_views, channels, alt_lo, step, n_planes, radius, min_views,
                              min_std, altitude, score, index, views, volume, floor, slack, (hipStream_t)stream);
}
