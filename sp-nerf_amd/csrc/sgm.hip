// Semi-global aggregation (include/spnerf_amd_sgm.h): the plane sweep's score volume regularised across
// cells.  The whole translation unit is compiled without fused multiply-adds (the file-scope pragma below),
// and every sum of the header is one fp32 operation here, in the header's order.
// The volume is plane-major [K][cells]; the recurrence walks cells serially and needs all K planes of a
// cell at once, so the three launches work on a cell-major copy [cells][K] held in the caller's workspace:
//  * k_sgm_cost — a 256-thread workgroup owns 64 consecutive cells and loops over the planes 64 at a time:
//    reads 64 x 64 scores with the lanes over cells (256 B per wavefront load), turns them into costs,
//    transposes through a padded LDS tile and writes with the lanes over planes; one byte per cell says
//    whether any plane was scored.
//  * k_sgm_paths<NC> — every direction in one launch (blockIdx.y), one wavefront per path, its lanes over the
//    planes, NC = ceil(K / 64) values per lane in registers (NC = 1, 2, 4, 8: K up to 512).  Per step: the next
//    cell's costs are already in flight, min_k is a register minimum over the lane's values and a butterfly
//    over the wavefront (wave_fmin, csrc/wave.h), k ± 1 come from the neighbouring lanes (the lane at a 64-plane
//    boundary reads the neighbouring register's end lane), and L_r(p, ·) goes to the direction's own slab.  Lanes
//    at or beyond K hold +inf, which no minimum takes and no sum turns into NaN.  No LDS.
//  * k_sgm_finish<PATHS> — the workgroup of k_sgm_cost in reverse: sums the slabs in direction order with the lanes
//    over planes, 1 − S / paths, NaN where the cell has no scored plane, transposed back through LDS.
// No atomics anywhere: each (cell, plane, direction) is written by exactly one lane.
#include <cmath>

#include "common.h"
#include "ground.h"

#pragma clang fp contract(off)

#include "../../include/spnerf_amd_sgm.h"
#include "sweep_pick.h"
#include "wave.h"

namespace spn {

constexpr int kSgmTile = SPNERF_SGM_TILE;
constexpr int kSgmThreads = 256;
constexpr int kSgmRows = kSgmTile / (kSgmThreads / 64);   // tile rows per wavefront
static_assert(kSgmTile == 64 && kSgmRows == 16, "a tile is 64 cells x 64 planes, 16 rows per wavefront of a 256-thread workgroup");
constexpr unsigned kSgmMaxBlocks = 1u << 20;              // the transposing kernels stride over the tiles beyond this
constexpr unsigned kSgmMaxPathBlocks = 1u << 16;

// the header's directions, (dj, di)
__device__ __forceinline__ void sgm_direction(int d, int& dj, int& di) {
    dj = d < 2 ? 0 : (d & 1) ? -1 : 1;
    di = d < 2 ? (d == 0 ? 1 : -1) : d < 4 ? 0 : (d == 4 || d == 7) ? 1 : -1;
}

//   volume [K][cells]; cost [cells][K]; scored [cells]
__global__ __launch_bounds__(kSgmThreads) void k_sgm_cost(const float* __restrict__ volume, int K, int64_t cells, float unscored,
                                                          float* __restrict__ cost, uint8_t* __restrict__ scored) {
    __shared__ float tile[kSgmTile][kSgmTile + 1];
    __shared__ int any_of[kSgmThreads / 64][64];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t tiles = (cells + kSgmTile - 1) / kSgmTile;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t c0 = t * kSgmTile;
        int any = 0;
        for (int k0 = 0; k0 < K; k0 += kSgmTile) {
            for (int r = 0; r < kSgmRows; ++r) {   // lanes over cells
                const int kk = wave * kSgmRows + r, k = k0 + kk;
                if (k < K && c0 + lane < cells) {
                    const float v = volume[k * cells + c0 + lane];
                    const bool fin = isfinite(v);
                    any |= fin ? 1 : 0;
                    tile[kk][lane] = fin ? 1.0f - v : unscored;
                }
            }
            __syncthreads();
            for (int r = 0; r < kSgmRows; ++r) {   // lanes over planes
                const int cc = wave * kSgmRows + r;
                if (c0 + cc < cells && k0 + lane < K) cost[(c0 + cc) * K + k0 + lane] = tile[lane][cc];
            }
            __syncthreads();
        }
        any_of[wave][lane] = any;
        __syncthreads();
        if (wave == 0 && c0 + lane < cells) scored[c0 + lane] = (uint8_t)(any_of[0][lane] | any_of[1][lane] | any_of[2][lane] | any_of[3][lane]);
        __syncthreads();
    }
}

// the values of lane l of a wavefront register, as a scalar
__device__ __forceinline__ float lane_value(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

template <int NC>
__device__ __forceinline__ void load_costs(const float* __restrict__ cost, int64_t cell, int K, int lane, float (&c)[NC]) {
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        const int k = ch * 64 + lane;
        c[ch] = k < K ? cost[cell * K + k] : INFINITY;
    }
}

//   cost [cells][K]; slabs [paths][cells][K]; grid: x strides over the paths of direction blockIdx.y, 4 per block
template <int NC>
__global__ __launch_bounds__(kSgmThreads) void k_sgm_paths(const float* __restrict__ cost, int K, int H, int W, float p1, float p2,
                                                           float* __restrict__ slabs) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int d = (int)blockIdx.y;
    int dj, di;
    sgm_direction(d, dj, di);
    const int64_t cells = (int64_t)H * W;
    const int64_t n_paths = dj == 0 ? H : di == 0 ? W : (int64_t)W + H - 1;
    float* __restrict__ L_out = slabs + (int64_t)d * K * cells;
    for (int64_t t = (int64_t)blockIdx.x * (kSgmThreads / 64) + wave; t < n_paths; t += (int64_t)gridDim.x * (kSgmThreads / 64)) {
        // the path's first cell: the one whose predecessor lies outside the grid
        int j, i;
        if (dj == 0) {
            j = (int)t;
            i = di > 0 ? 0 : W - 1;
        } else if (di == 0 || t < W) {
            j = dj > 0 ? 0 : H - 1;
            i = (int)t;
        } else {
            j = (int)(t - W) + (dj > 0 ? 1 : 0);
            i = di > 0 ? 0 : W - 1;
        }
        float L[NC], c[NC], cn[NC];
        int64_t cell = (int64_t)j * W + i;
        load_costs<NC>(cost, cell, K, lane, c);
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            L[ch] = c[ch];
            if (ch * 64 + lane < K) L_out[cell * K + ch * 64 + lane] = L[ch];
        }
        j += dj;
        i += di;
        bool inside = j >= 0 && j < H && i >= 0 && i < W;
        if (inside) load_costs<NC>(cost, (int64_t)j * W + i, K, lane, cn);
        while (inside) {
            cell = (int64_t)j * W + i;
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) c[ch] = cn[ch];
            j += dj;
            i += di;
            inside = j >= 0 && j < H && i >= 0 && i < W;
            if (inside) load_costs<NC>(cost, (int64_t)j * W + i, K, lane, cn);   // in flight under this step

            float M = L[0];
#pragma unroll
            for (int ch = 1; ch < NC; ++ch) M = fminf(M, L[ch]);
            M = wave_fmin(M);
            const float jump = M + p2;
            float next[NC];
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) {
                float below = __shfl_up(L[ch], 1, 64), above = __shfl_down(L[ch], 1, 64);
                const float before = ch > 0 ? lane_value(L[ch > 0 ? ch - 1 : 0], 63) : INFINITY;
                const float after = ch < NC - 1 ? lane_value(L[ch < NC - 1 ? ch + 1 : ch], 0) : INFINITY;
                if (lane == 0) below = before;
                if (lane == 63) above = after;
                const float m = fminf(fminf(L[ch], below + p1), fminf(above + p1, jump));
                next[ch] = c[ch] + (m - M);
            }
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) {
                L[ch] = next[ch];
                if (ch * 64 + lane < K) L_out[cell * K + ch * 64 + lane] = L[ch];
            }
        }
    }
}

//   slabs [PATHS][cells][K]; scored [cells]; out [K][cells]
template <int PATHS>
__global__ __launch_bounds__(kSgmThreads) void k_sgm_finish(const float* __restrict__ slabs, const uint8_t* __restrict__ scored, int K,
                                                            int64_t cells, float* __restrict__ out) {
    __shared__ float tile[kSgmTile][kSgmTile + 1];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int64_t tiles = (cells + kSgmTile - 1) / kSgmTile, slab = (int64_t)K * cells;
    const float inv = 1.0f / (float)PATHS;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t c0 = t * kSgmTile;
        for (int k0 = 0; k0 < K; k0 += kSgmTile) {
            for (int r = 0; r < kSgmRows; ++r) {   // lanes over planes
                const int cc = wave * kSgmRows + r;
                const int64_t cell = c0 + cc;
                if (cell < cells && k0 + lane < K) {
                    const float* at = slabs + cell * K + k0 + lane;
                    float S = at[0];
#pragma unroll
                    for (int d = 1; d < PATHS; ++d) S = S + at[d * slab];
                    tile[lane][cc] = scored[cell] ? 1.0f - S * inv : NAN;
                }
            }
            __syncthreads();
            for (int r = 0; r < kSgmRows; ++r) {   // lanes over cells
                const int kk = wave * kSgmRows + r, k = k0 + kk;
                if (k < K && c0 + lane < cells) out[k * cells + c0 + lane] = tile[kk][lane];
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSgmThreads) void k_sgm_pick(const float* __restrict__ aggregated, const float* __restrict__ volume, int K,
                                                          int64_t cells, double alt_lo, double step, float* __restrict__ altitude,
                                                          float* __restrict__ score, int32_t* __restrict__ index,
                                                          float* __restrict__ photo) {
    const int64_t cell = blockIdx.x * (int64_t)kSgmThreads + threadIdx.x;
    if (cell >= cells) return;
    Pick p;
    for (int k = 0; k < K; ++k) p.plane(k, aggregated[k * cells + cell], 0);
    altitude[cell] = p.altitude(K, alt_lo, step);
    score[cell] = p.best;
    index[cell] = p.index;
    float raw = NAN;
    if (p.index >= 0) {
        const float v = volume[p.index * cells + cell];
        if (isfinite(v)) raw = v;
    }
    photo[cell] = raw;
}

static int32_t check_sizes(const char* who, int32_t n_planes, int32_t ysize, int32_t xsize, int32_t paths) {
    SPN_ARG(n_planes >= 1 && n_planes <= SPNERF_SGM_MAX_PLANES, "%s: n_planes %d outside [1, %d]", who, n_planes, SPNERF_SGM_MAX_PLANES);
    SPN_TRY(check_cells(who, ysize, xsize));
    SPN_ARG(paths == 4 || paths == 8, "%s: paths %d must be 4 or 8", who, paths);
    return SPNERF_OK;
}

static int64_t workspace_of(int32_t n_planes, int64_t cells, int32_t paths) { return (int64_t)(1 + paths) * n_planes * cells * 4 + cells; }

static bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

template <int NC>
static void launch_paths(dim3 grid, hipStream_t st, const float* cost, int K, int H, int W, float p1, float p2, float* slabs) {
    hipLaunchKernelGGL(k_sgm_paths<NC>, grid, dim3(kSgmThreads), 0, st, cost, K, H, W, p1, p2, slabs);
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_sgm_abi_version(void) { return SPNERF_SGM_ABI_VERSION; }

extern "C" int32_t spnerf_sgm_workspace_bytes(int32_t n_planes, int32_t ysize, int32_t xsize, int32_t paths, int64_t* bytes) {
    SPN_ARG(bytes, "sgm_workspace_bytes: NULL bytes");
    SPN_TRY(check_sizes("sgm_workspace_bytes", n_planes, ysize, xsize, paths));
    *bytes = workspace_of(n_planes, (int64_t)xsize * ysize, paths);
    return SPNERF_OK;
}

extern "C" int32_t spnerf_sgm_aggregate(const float* volume, int32_t n_planes, int32_t ysize, int32_t xsize, float p1, float p2,
                                        float unscored, int32_t paths, float* out, void* workspace, int64_t workspace_bytes,
                                        void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(volume && out && workspace, "sgm: NULL volume, out or workspace");
    SPN_TRY(check_sizes("sgm", n_planes, ysize, xsize, paths));
    SPN_ARG(std::isfinite(p1) && p1 >= 0.0f, "sgm: p1 %g must be finite and >= 0", (double)p1);
    SPN_ARG(std::isfinite(p2) && p2 >= p1, "sgm: p2 %g must be finite and >= p1 %g", (double)p2, (double)p1);
    SPN_ARG(std::isfinite(unscored), "sgm: unscored %g is not finite", (double)unscored);
    const int64_t cells = (int64_t)xsize * ysize, entries = (int64_t)n_planes * cells, need = workspace_of(n_planes, cells, paths);
    SPN_ARG(workspace_bytes >= need, "sgm: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    SPN_ARG(!overlap(out, entries * 4, volume, entries * 4), "sgm: out overlaps volume");
    SPN_ARG(!overlap(workspace, need, volume, entries * 4) && !overlap(workspace, need, out, entries * 4),
            "sgm: workspace overlaps volume or out");
    SPN_ARG((uintptr_t)workspace % 4 == 0, "sgm: workspace is not 4-byte aligned");
    float* cost = (float*)workspace;
    float* slabs = cost + entries;
    uint8_t* scored = (uint8_t*)(slabs + (int64_t)paths * entries);
    const int64_t tiles = (cells + kSgmTile - 1) / kSgmTile;
    const unsigned blocks = (unsigned)(tiles < (int64_t)kSgmMaxBlocks ? tiles : (int64_t)kSgmMaxBlocks);
    {
        ProfScope prof("sgm_cost", st, (double)entries, (double)entries * 8.0 + (double)cells);
        hipLaunchKernelGGL(k_sgm_cost, dim3(blocks), dim3(kSgmThreads), 0, st, volume, n_planes, cells, unscored, cost, scored);
        SPN_HIP(hipGetLastError());
    }
    {
        const int64_t most = paths == 4 ? (xsize > ysize ? xsize : ysize) : (int64_t)xsize + ysize - 1;
        const int64_t groups = (most + kSgmThreads / 64 - 1) / (kSgmThreads / 64);
        const dim3 grid((unsigned)(groups < (int64_t)kSgmMaxPathBlocks ? groups : (int64_t)kSgmMaxPathBlocks), (unsigned)paths);
        ProfScope prof("sgm_paths", st, (double)paths * (double)entries * 8.0, (double)paths * (double)entries * 8.0);
        if (n_planes <= 64) launch_paths<1>(grid, st, cost, n_planes, ysize, xsize, p1, p2, slabs);
        else if (n_planes <= 128) launch_paths<2>(grid, st, cost, n_planes, ysize, xsize, p1, p2, slabs);
        else if (n_planes <= 256) launch_paths<4>(grid, st, cost, n_planes, ysize, xsize, p1, p2, slabs);
        else launch_paths<8>(grid, st, cost, n_planes, ysize, xsize, p1, p2, slabs);
        SPN_HIP(hipGetLastError());
    }
    {
        ProfScope prof("sgm_finish", st, (double)paths * (double)entries, (double)entries * (4.0 * paths + 4.0) + (double)cells);
        if (paths == 4) hipLaunchKernelGGL(k_sgm_finish<4>, dim3(blocks), dim3(kSgmThreads), 0, st, slabs, scored, n_planes, cells, out);
        else hipLaunchKernelGGL(k_sgm_finish<8>, dim3(blocks), dim3(kSgmThreads), 0, st, slabs, scored, n_planes, cells, out);
        SPN_HIP(hipGetLastError());
    }
    return SPNERF_OK;
}

extern "C" int32_t spnerf_sgm_pick(const float* aggregated, const float* volume, int32_t n_planes, int64_t cells, double alt_lo,
                                   double step, float* altitude, float* score, int32_t* index, float* photo, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(aggregated && volume && altitude && score && index && photo,
            "sgm_pick: NULL aggregated, volume, altitude, score, index or photo");
    SPN_ARG(cells >= 1 && cells <= ((int64_t)1 << 32), "sgm_pick: cells %lld outside [1, 2^32]", (long long)cells);
    SPN_ARG(n_planes >= 1 && n_planes <= SPNERF_SGM_MAX_PLANES, "sgm_pick: n_planes %d outside [1, %d]", n_planes, SPNERF_SGM_MAX_PLANES);
    SPN_ARG(std::isfinite(alt_lo), "sgm_pick: alt_lo %g is not finite", alt_lo);
    SPN_ARG(step > 0.0 && std::isfinite(step), "sgm_pick: step %g must be finite and > 0", step);
    ProfScope prof("sgm_pick", st, 0.0, (double)cells * (n_planes * 4.0 + 20.0));
    hipLaunchKernelGGL(k_sgm_pick, dim3((unsigned)((cells + kSgmThreads - 1) / kSgmThreads)), dim3(kSgmThreads), 0, st, aggregated, volume,
                       n_planes, cells, alt_lo, step, altitude, score, index, photo);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
