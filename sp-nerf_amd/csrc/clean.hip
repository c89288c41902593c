// DSM cleaning (include/staged/spnerf_amd_clean.h): the speckle filter, the median and the hole fill of an
// (H, W) fp32 raster.  Nothing here rounds — compares, selections and one fp32 subtraction that is only
// compared — so there is nothing to contract; the pragma below keeps it that way.
//
// THE LABELLING is a union-find on an int32 parent plane.  The invariant every kernel keeps and checks:
// parent[i] <= i, parent[i] is a cell of i's component, and a value stored in parent[i] only ever
// decreases (the stores are the initial i, atomicMin, and nothing else).  A root is a cell with
// parent[i] == i; once no union is in flight a component has one root, its smallest index.
//  * find(i) follows parent links.  Each step goes to a strictly smaller index — a link that does not is
//    refused and raises the flag — so it ends within i + 1 steps, whatever other threads store meanwhile,
//    and also if it reads a stale value: every value parent[i] ever held is a smaller cell of the component.
//  * unite(a, b): order the pair so that a > b, old = atomicMin(&parent[a], b).  If old == a, a was a root
//    and now hangs under b: done.  Otherwise a already hung under old < a; parent[a] is now min(old, b),
//    still a cell of the component, and the union that remains is that of old and b: retry with a = old.
//    max(a, b) is strictly lower in every retry, so the loop ends within max(a, b) + 1 rounds.
//  Both loops still count their iterations against H·W (the local pass: against the tile's cells) and set
//  the flag when the count runs out: a defect shows as SPNERF_CLEAN_E_BOUND, never as a kernel that spins.
//  * k_clean_local — one workgroup per TILE x TILE tile, one thread per cell, the same two loops on an LDS
//    plane of tile-local indices (row-major, so the order of local indices is the order of the global ones),
//    then every cell's local root as a global index into parent.
//  * k_clean_merge — one thread per pair of cells across a tile border (east-west pairs of every border column,
//    then north-south pairs of every border row).  Reads of parent are agent-scope atomic loads, the unions
//    device-scope atomicMin: no plain load has to see another workgroup's store inside this launch.
//  * k_clean_flatten — a launch of its own, so plain loads see the merged plane: label = find(i), and the root's
//    count + 1, one integer add per wavefront where all its cells share the first lane's root.
//  * k_clean_apply — size = count[label], out.
//
// THE MEDIAN stages a tile and its halo in LDS with every hole as NaN; a thread counts the finite values of
// its window, then looks for the value v with  #(w < v) <= k < #(w <= v), k = (n - 1) / 2: the value of rank k.
// The window stays in LDS (no register array, no scratch).  THE FILL is eight bounded walks per hole.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "../../include/staged/spnerf_amd_clean.h"

namespace spn {

constexpr int kCleanTile = SPNERF_CLEAN_TILE;
constexpr int kCleanThreads = kCleanTile * kCleanTile;
static_assert(kCleanThreads == 256, "a tile is one 256-thread workgroup, one thread per cell");
constexpr int kCleanMaxCells = 0x7fffffff;

// both finite cells: joined?  (b NaN: NaN <= x is false; b ±inf or an overflowing difference: inf <= x is false)
__device__ __forceinline__ bool clean_joined(float a, float b, float max_diff) { return fabsf(a - b) <= max_diff; }

// ---- union-find on an LDS plane (workgroup scope) and on the global plane (agent scope) ---------------------

// how a parent plane is read: an LDS plane other threads of the workgroup are uniting on; the global plane while other
// workgroups unite on it (agent-scope atomic loads, so no plain load has to see another workgroup's store); the global
// plane after the launch that united it has ended (plain loads: the launch boundary made it visible, nothing stores)
enum class Plane { kLds, kGlobalLive, kGlobalSettled };

template <Plane P>
__device__ __forceinline__ int uf_load(const int* p) {
    if constexpr (P == Plane::kLds) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else if constexpr (P == Plane::kGlobalLive) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// the root above cell i (i >= 0); `bad` is raised by a link that does not point downwards or when `limit` steps did not reach a root
template <Plane P>
__device__ __forceinline__ int uf_find(const int* parent, int i, int limit, bool& bad) {
    for (int it = 0; it < limit; ++it) {
        const int p = uf_load<P>(parent + i);
        if (p == i) return i;
        if ((unsigned)p > (unsigned)i) break;   // also a negative p: never followed, so no read leaves the plane
        i = p;
    }
    bad = true;
    return i;
}

template <Plane P>
__device__ __forceinline__ void uf_unite(int* parent, int a, int b, int limit, bool& bad) {
    for (int it = 0; it < limit; ++it) {
        a = uf_find<P>(parent, a, limit, bad);
        b = uf_find<P>(parent, b, limit, bad);
        if (a == b || bad) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        if ((unsigned)old > (unsigned)a) break;
        a = old;
    }
    bad = true;
}

// tiles are numbered row-major in a 1-D grid (a grid of one column has more tile rows than gridDim.y holds)
__device__ __forceinline__ void clean_tile_origin(int tiles_x, int& x0, int& y0) {
    const int tile = (int)blockIdx.x;
    y0 = (tile / tiles_x) * kCleanTile;
    x0 = (tile % tiles_x) * kCleanTile;
}

__global__ __launch_bounds__(kCleanThreads) void k_clean_local(const float* __restrict__ dsm, int H, int W, int tiles_x, float max_diff,
                                                               int* __restrict__ parent, int* __restrict__ flag) {
    __shared__ float val[kCleanThreads];
    __shared__ int lab[kCleanThreads];
    int x0, y0;
    clean_tile_origin(tiles_x, x0, y0);
    const int t = (int)threadIdx.x, lx = t % kCleanTile, ly = t / kCleanTile;
    const int x = x0 + lx, y = y0 + ly;
    const bool inside = x < W && y < H;
    const float v = inside ? dsm[(int64_t)y * W + x] : NAN;
    const bool fin = isfinite(v);
    val[t] = v;
    lab[t] = fin ? t : -1;
    __syncthreads();
    bool bad = false;
    if (fin) {
        if (lx + 1 < kCleanTile && clean_joined(v, val[t + 1], max_diff)) uf_unite<Plane::kLds>(lab, t, t + 1, kCleanThreads, bad);
        if (ly + 1 < kCleanTile && clean_joined(v, val[t + kCleanTile], max_diff)) uf_unite<Plane::kLds>(lab, t, t + kCleanTile, kCleanThreads, bad);
    }
    __syncthreads();
    if (inside) {
        int root = -1;
        if (fin) {
            const int r = uf_find<Plane::kLds>(lab, t, kCleanThreads, bad);
            root = (y0 + r / kCleanTile) * W + x0 + r % kCleanTile;
        }
        parent[(int64_t)y * W + x] = root;
    }
    if (bad) *flag = 1;
}

//   pairs: the (tiles_x - 1)·H east-west pairs, then the (tiles_y - 1)·W north-south pairs
__global__ __launch_bounds__(256) void k_clean_merge(const float* __restrict__ dsm, int H, int W, int tiles_x, int64_t pairs, float max_diff,
                                                     int* __restrict__ parent, int limit, int* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pairs) return;
    const int64_t ew = (int64_t)(tiles_x - 1) * H;
    int a, b;
    if (e < ew) {
        const int x = ((int)(e / H) + 1) * kCleanTile - 1, y = (int)(e % H);   // x + 1 <= (tiles_x - 1)·TILE < W
        a = y * W + x;
        b = a + 1;
    } else {
        const int64_t s = e - ew;
        const int y = ((int)(s / W) + 1) * kCleanTile - 1, x = (int)(s % W);   // y + 1 <= (tiles_y - 1)·TILE < H
        a = y * W + x;
        b = a + W;
    }
    const float va = dsm[a], vb = dsm[b];
    if (!isfinite(va) || !clean_joined(va, vb, max_diff)) return;
    bool bad = false;
    uf_unite<Plane::kGlobalLive>(parent, a, b, limit, bad);
    if (bad) *flag = 1;
}

__global__ __launch_bounds__(256) void k_clean_flatten(const int* __restrict__ parent, int cells, int limit, int32_t* __restrict__ label,
                                                       int* __restrict__ count, int* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool inside = i < cells;
    bool bad = false;
    int root = -1;
    if (inside && parent[i] >= 0) root = uf_find<Plane::kGlobalSettled>(parent, (int)i, limit, bad);
    if (inside) label[i] = root;
    // every lane is here: one add for the lanes that share the first lane's root, one each for the others
    const int first = __builtin_amdgcn_readfirstlane(root);
    const bool shares = root >= 0 && root == first;
    const unsigned long long group = __ballot(shares);
    if (shares) {
        if (((int)threadIdx.x & 63) == __ffsll((long long)group) - 1) atomicAdd(count + first, __popcll(group));
    } else if (root >= 0) {
        atomicAdd(count + root, 1);
    }
    if (bad) *flag = 1;
}

__global__ __launch_bounds__(256) void k_clean_apply(const float* __restrict__ dsm, const int32_t* __restrict__ label, const int* __restrict__ count,
                                                     int cells, int max_size, float* __restrict__ out, int32_t* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const int root = label[i];
    const int n = root >= 0 ? count[root] : 0;
    size[i] = n;
    out[i] = n >= 1 && n <= max_size ? NAN : dsm[i];
}

// ---- the median -------------------------------------------------------------------------------------------------

template <int R>
__global__ __launch_bounds__(kCleanThreads) void k_clean_median(const float* __restrict__ dsm, int H, int W, int tiles_x, int min_count, int fill,
                                                                float* __restrict__ out) {
    constexpr int S = kCleanTile + 2 * R;
    __shared__ float halo[S][S + 1];
    int x0, y0;
    clean_tile_origin(tiles_x, x0, y0);
    for (int k = (int)threadIdx.x; k < S * S; k += kCleanThreads) {
        const int hy = k / S, hx = k % S, y = y0 + hy - R, x = x0 + hx - R;
        float v = NAN;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            v = dsm[(int64_t)y * W + x];
            if (!isfinite(v)) v = NAN;
        }
        halo[hy][hx] = v;
    }
    __syncthreads();
    const int lx = (int)threadIdx.x % kCleanTile, ly = (int)threadIdx.x / kCleanTile;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const int64_t cell = (int64_t)y * W + x;
    if (!fill && halo[ly + R][lx + R] != halo[ly + R][lx + R]) {
        out[cell] = dsm[cell];   // a hole keeps its own bytes
        return;
    }
    int n = 0;
    for (int j = 0; j <= 2 * R; ++j)
        for (int i = 0; i <= 2 * R; ++i) n += halo[ly + j][lx + i] == halo[ly + j][lx + i] ? 1 : 0;
    float result = NAN;
    if (n >= min_count) {   // min_count >= 1: there is a finite value
        const int k = (n - 1) / 2;
        for (int c = 0; c < (2 * R + 1) * (2 * R + 1); ++c) {
            const float v = halo[ly + c / (2 * R + 1)][lx + c % (2 * R + 1)];
            if (v != v) continue;
            int less = 0, leq = 0;
            for (int j = 0; j <= 2 * R; ++j)
                for (int i = 0; i <= 2 * R; ++i) {
                    const float w = halo[ly + j][lx + i];
                    less += w < v ? 1 : 0;
                    leq += w <= v ? 1 : 0;
                }
            if (less <= k && k < leq) {
                result = v + 0.0f;   // -0 comes out as +0
                break;
            }
        }
    }
    out[cell] = result;
}

// ---- the fill ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_clean_fill(const float* __restrict__ dsm, int H, int W, int reach, int mode, int min_dirs,
                                                    float* __restrict__ out, uint8_t* __restrict__ filled) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= (int64_t)H * W) return;
    const float own = dsm[cell];
    if (isfinite(own)) {
        out[cell] = own;
        filled[cell] = 0;
        return;
    }
    const int y = (int)(cell / W), x = (int)(cell % W);
    int found = 0, best_d2 = 0;
    float best = NAN;
    for (int d = 0; d < 8; ++d) {   // E, NE, N, NW, W, SW, S, SE; north is towards row 0
        const int dx = (d == 0 || d == 1 || d == 7) ? 1 : (d >= 3 && d <= 5) ? -1 : 0;
        const int dy = (d >= 1 && d <= 3) ? -1 : (d >= 5) ? 1 : 0;
        int yy = y, xx = x;
        for (int n = 1; n <= reach; ++n) {
            yy += dy;
            xx += dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) break;
            const float v = dsm[(int64_t)yy * W + xx];
            if (isfinite(v)) {
                const int d2 = (dx != 0 && dy != 0 ? 2 : 1) * n * n;   // reach <= 4096: at most 2^25
                if (found == 0 || (mode == SPNERF_CLEAN_LOWEST ? v < best : d2 < best_d2)) {
                    best = v;
                    best_d2 = d2;
                }
                ++found;
                break;
            }
        }
    }
    const bool write = found >= min_dirs;   // min_dirs >= 1
    out[cell] = write ? best : own;
    filled[cell] = write ? 1 : 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------

static int32_t clean_cells(const char* who, int32_t ysize, int32_t xsize) {
    SPN_ARG(xsize > 0 && ysize > 0, "%s: grid of %d x %d cells", who, xsize, ysize);
    SPN_ARG((int64_t)xsize * ysize <= (int64_t)kCleanMaxCells, "%s: grid of %d x %d cells is too large for one call (2^31 - 1 cells: a cell's index is an int32)", who,
            xsize, ysize);
    return SPNERF_OK;
}

static int64_t clean_workspace_of(int64_t cells) { return cells * 8 + 16; }

static bool clean_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

static unsigned clean_tiles(int32_t ysize, int32_t xsize, int& tiles_x, int& tiles_y) {
    tiles_x = (xsize + kCleanTile - 1) / kCleanTile;
    tiles_y = (ysize + kCleanTile - 1) / kCleanTile;
    return (unsigned)((int64_t)tiles_x * tiles_y);   // at most 2^31 / 16 + 1
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_clean_abi_version(void) { return SPNERF_CLEAN_ABI_VERSION; }

extern "C" int32_t spnerf_clean_workspace_bytes(int32_t ysize, int32_t xsize, int64_t* bytes) {
    SPN_ARG(bytes, "clean_workspace_bytes: NULL bytes");
    SPN_TRY(clean_cells("clean_workspace_bytes", ysize, xsize));
    *bytes = clean_workspace_of((int64_t)xsize * ysize);
    return SPNERF_OK;
}

extern "C" int32_t spnerf_clean_speckle(const float* dsm, int32_t ysize, int32_t xsize, float max_diff, int32_t max_size, float* out,
                                        int32_t* label, int32_t* size, void* workspace, int64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(dsm && out && label && size && workspace, "clean_speckle: NULL dsm, out, label, size or workspace");
    SPN_TRY(clean_cells("clean_speckle", ysize, xsize));
    SPN_ARG(std::isfinite(max_diff) && max_diff >= 0.0f, "clean_speckle: max_diff %g must be finite and >= 0", (double)max_diff);
    SPN_ARG(max_size >= 0, "clean_speckle: max_size %d must be >= 0", max_size);
    const int64_t cells = (int64_t)xsize * ysize, plane = cells * 4, need = clean_workspace_of(cells);
    SPN_ARG(workspace_bytes >= need, "clean_speckle: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    SPN_ARG((uintptr_t)workspace % 4 == 0, "clean_speckle: workspace is not 4-byte aligned");
    SPN_ARG(!clean_overlap(out, plane, dsm, plane), "clean_speckle: out overlaps dsm");
    SPN_ARG(!clean_overlap(label, plane, dsm, plane) && !clean_overlap(size, plane, dsm, plane), "clean_speckle: label or size overlaps dsm");
    SPN_ARG(!clean_overlap(workspace, need, dsm, plane) && !clean_overlap(workspace, need, out, plane) && !clean_overlap(workspace, need, label, plane) &&
                !clean_overlap(workspace, need, size, plane),
            "clean_speckle: workspace overlaps dsm, out, label or size");
    SPN_ARG(!clean_overlap(out, plane, label, plane) && !clean_overlap(out, plane, size, plane) && !clean_overlap(label, plane, size, plane),
            "clean_speckle: out, label and size overlap one another");
    int* parent = (int*)workspace;
    int* count = parent + cells;
    int* flag = count + cells;
    int tiles_x, tiles_y;
    const unsigned tiles = clean_tiles(ysize, xsize, tiles_x, tiles_y);
    const int64_t pairs = (int64_t)(tiles_x - 1) * ysize + (int64_t)(tiles_y - 1) * xsize;
    const unsigned blocks = blocks_of(cells, 256);
    const int limit = (int)cells;
    SPN_HIP(hipMemsetAsync(count, 0, (size_t)plane + 16, st));   // the counts and the flag's 16 bytes
    {
        ProfScope prof("clean_local", st, 0.0, (double)cells * 8.0);
        hipLaunchKernelGGL(k_clean_local, dim3(tiles), dim3(kCleanThreads), 0, st, dsm, ysize, xsize, tiles_x, max_diff, parent, flag);
        SPN_HIP(hipGetLastError());
    }
    if (pairs > 0) {
        ProfScope prof("clean_merge", st, 0.0, (double)pairs * 16.0);
        hipLaunchKernelGGL(k_clean_merge, dim3(blocks_of(pairs, 256)), dim3(256), 0, st, dsm, ysize, xsize, tiles_x, pairs, max_diff, parent, limit, flag);
        SPN_HIP(hipGetLastError());
    }
    {
        ProfScope prof("clean_flatten", st, 0.0, (double)cells * 12.0);
        hipLaunchKernelGGL(k_clean_flatten, dim3(blocks), dim3(256), 0, st, parent, (int)cells, limit, label, count, flag);
        SPN_HIP(hipGetLastError());
    }
    {
        ProfScope prof("clean_apply", st, 0.0, (double)cells * 20.0);
        hipLaunchKernelGGL(k_clean_apply, dim3(blocks), dim3(256), 0, st, dsm, label, count, (int)cells, max_size, out, size);
        SPN_HIP(hipGetLastError());
    }
    int ran_out = 0;
    SPN_HIP(hipMemcpyAsync(&ran_out, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    SPN_HIP(hipStreamSynchronize(st));
    if (ran_out != 0) {
        set_error("clean_speckle: a bounded loop of the labelling ran out on a grid of %d x %d cells: a defect of the kernels, the outputs are not valid", xsize,
                  ysize);
        return SPNERF_CLEAN_E_BOUND;
    }
    return SPNERF_OK;
}

extern "C" int32_t spnerf_clean_median(const float* dsm, int32_t ysize, int32_t xsize, int32_t radius, int32_t min_count, int32_t fill,
                                       float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(dsm && out, "clean_median: NULL dsm or out");
    SPN_TRY(clean_cells("clean_median", ysize, xsize));
    SPN_ARG(radius >= 1 && radius <= SPNERF_CLEAN_MAX_RADIUS, "clean_median: radius %d outside [1, %d]", radius, SPNERF_CLEAN_MAX_RADIUS);
    const int window = (2 * radius + 1) * (2 * radius + 1);
    SPN_ARG(min_count >= 1 && min_count <= window, "clean_median: min_count %d outside [1, %d]", min_count, window);
    SPN_ARG(fill == 0 || fill == 1, "clean_median: fill %d must be 0 or 1", fill);
    const int64_t cells = (int64_t)xsize * ysize;
    SPN_ARG(!clean_overlap(out, cells * 4, dsm, cells * 4), "clean_median: out overlaps dsm");
    int tiles_x, tiles_y;
    const unsigned tiles = clean_tiles(ysize, xsize, tiles_x, tiles_y);
    ProfScope prof("clean_median", st, 0.0, (double)cells * 8.0);
    if (radius == 1) hipLaunchKernelGGL(k_clean_median<1>, dim3(tiles), dim3(kCleanThreads), 0, st, dsm, ysize, xsize, tiles_x, min_count, fill, out);
    else if (radius == 2) hipLaunchKernelGGL(k_clean_median<2>, dim3(tiles), dim3(kCleanThreads), 0, st, dsm, ysize, xsize, tiles_x, min_count, fill, out);
    else hipLaunchKernelGGL(k_clean_median<3>, dim3(tiles), dim3(kCleanThreads), 0, st, dsm, ysize, xsize, tiles_x, min_count, fill, out);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_clean_fill(const float* dsm, int32_t ysize, int32_t xsize, int32_t reach, int32_t mode, int32_t min_dirs,
                                     float* out, uint8_t* filled, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(dsm && out && filled, "clean_fill: NULL dsm, out or filled");
    SPN_TRY(clean_cells("clean_fill", ysize, xsize));
    SPN_ARG(reach >= 1 && reach <= SPNERF_CLEAN_MAX_REACH, "clean_fill: reach %d outside [1, %d]", reach, SPNERF_CLEAN_MAX_REACH);
    SPN_ARG(mode == SPNERF_CLEAN_LOWEST || mode == SPNERF_CLEAN_NEAREST, "clean_fill: mode %d is neither 0 (lowest) nor 1 (nearest)", mode);
    SPN_ARG(min_dirs >= 1 && min_dirs <= 8, "clean_fill: min_dirs %d outside [1, 8]", min_dirs);
    const int64_t cells = (int64_t)xsize * ysize;
    SPN_ARG(!clean_overlap(out, cells * 4, dsm, cells * 4), "clean_fill: out overlaps dsm");
    SPN_ARG(!clean_overlap(filled, cells, dsm, cells * 4) && !clean_overlap(filled, cells, out, cells * 4), "clean_fill: filled overlaps dsm or out");
    ProfScope prof("clean_fill", st, 0.0, (double)cells * 9.0);
    hipLaunchKernelGGL(k_clean_fill, dim3(blocks_of(cells, 256)), dim3(256), 0, st, dsm, ysize, xsize, reach, mode, min_dirs, out, filled);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
