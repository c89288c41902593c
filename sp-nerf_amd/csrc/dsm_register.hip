// DSM registration by multiscale normalised cross correlation (the reference's modules/dsmr.py:
// downsample2x, mean_std / ncc, compute_ncc, recursive_ncc, apply_shift_) on the GPU in fp64, and
// the registered error map with its sums (utils.dsm_pointwise_diff / the MAE).  Images are
// row-major [H][W]; non-finite pixels are missing; a shift (dx, dy) pairs u[j][i] with
// v[j + dy][i + dx].
//  * k_dsm_pivot — one block: the first finite pixel of u and of v, subtracted from every pixel
//    before the one-pass moments accumulate (mean, deviation and covariance are invariant to it;
//    it only keeps Σx² − (Σx)²/n away from cancellation).  0 when an image has no finite pixel.
//  * k_dsm_down2x — downsample2x.  The reference stores, for every source pixel (j, i), the mean
//    of the finite pixels of the 2x2 block starting there at out[j/2][i/2]; the value written
//    last stands, i.e. the block starting at (min(2J+1, H−1), min(2I+1, W−1)), summed in the
//    reference's order so the result is bit-equal.
//  * k_dsm_ncc_moments — a workgroup owns a 32x32 tile of u.  It stages the (32 + 2·irange)²
//    halo of v around the tile displaced by the window centre in LDS (pivoted, NaN = missing);
//    every wave holds the whole tile of u in registers (16 pixels per lane) and takes every 4th
//    shift of the window: per shift 16 LDS reads per lane (conflict-free: a half-wave reads 32
//    consecutive doubles), six masked sums (count, Σu, Σv, Σu², Σv², Σuv), a __shfl_xor
//    reduction, and one 48-byte store to partial[block][shift][6].  The window centre comes
//    from device memory (the level below's result, doubled), so a whole pyramid is enqueued
//    without a host sync.
//  * k_dsm_ncc_pick — one workgroup per level: sums the partials over blocks in block order (no
//    atomics: bit-reproducible), forms mean_std's moments and ncc = xcorr / (sigu·sigv) per
//    shift, and scans them like compute_ncc (y outer, x inner, strictly greater wins, a NaN
//    never does, the centre stands when nothing wins).
//  * k_dsm_apply_shift_err / k_dsm_err_finish — out = a·v[j+dy][i+dx] + b (NaN out of range),
//    err = out − u, and the two-stage sums of |err| and of the finite count (fixed grid, fixed
//    order).  The reference's "+ c·i + d·j" is left out: it is identically zero there (c is
//    shadowed by the channel loop's index, 0 for a one-channel DSM, and d defaults to 0).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../../include/spnerf_amd_eval.h"
#include "common.h"
#include "wave.h"

namespace spn {

constexpr int kRegTile = 32;        // tile side of u per workgroup
constexpr int kRegPix = 16;         // pixels of the tile per lane (32·32 / 64)
constexpr int kRegWaves = 4;
constexpr int kRegMaxShifts = (2 * SPNERF_EVAL_DSM_MAX_IRANGE + 1) * (2 * SPNERF_EVAL_DSM_MAX_IRANGE + 1);
constexpr int kErrBlocks = (SPNERF_EVAL_DSM_SUMS_DOUBLES - 2) / 2;

__global__ __launch_bounds__(256) void k_dsm_pivot(const double* u, const double* v, int n, double* pivot) {
    __shared__ int s_first[2];
    if (threadIdx.x < 2) s_first[threadIdx.x] = n;
    __syncthreads();
    for (int img = 0; img < 2; ++img) {
        const double* p = img ? v : u;
        for (int k = threadIdx.x; k < n; k += 256)
            if (isfinite(p[k])) {
                atomicMin(&s_first[img], k);   // LDS integer minimum: order-independent
                break;
            }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = s_first[threadIdx.x];
        pivot[threadIdx.x] = k < n ? (threadIdx.x ? v : u)[k] : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_dsm_down2x(const double* in, int H, int W, double* out, int oh, int ow) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= oh * ow) return;
    const int J = k / ow, I = k - J * ow;
    const int j0 = min(2 * J + 1, H - 1), i0 = min(2 * I + 1, W - 1);
    double s = 0.0;
    int n = 0;
#pragma unroll
    for (int di = 0; di < 2; ++di)
#pragma unroll
        for (int dj = 0; dj < 2; ++dj) {
            const int j = j0 + dj, i = i0 + di;
            if (j < H && i < W) {
                const double t = in[(int64_t)j * W + i];
                if (isfinite(t)) {
                    s += t;
                    ++n;
                }
            }
        }
    out[k] = n > 0 ? s / (double)n : NAN;
}

struct NccArgs {
    const double* u;
    const double* v;
    int H, W, r;
    const int* centre;   // the level below's (dx, dy), doubled here; null: (cx0, cy0)
    int cx0, cy0;
    const double* pivot;
    double* partial;     // [blocks][shifts][6]
};

__device__ __forceinline__ void window_centre(const int* centre, int cx0, int cy0, int* cx, int* cy) {
    *cx = centre ? 2 * centre[0] : cx0;
    *cy = centre ? 2 * centre[1] : cy0;
}

__global__ __launch_bounds__(256) void k_dsm_ncc_moments(NccArgs g) {
    extern __shared__ double s_v[];   // [hw][hw]: v − pivot around the displaced tile, NaN = missing
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int side = 2 * g.r + 1, hw = kRegTile + 2 * g.r, S = side * side;
    int cx, cy;
    window_centre(g.centre, g.cx0, g.cy0, &cx, &cy);
    const int tx0 = blockIdx.x * kRegTile, ty0 = blockIdx.y * kRegTile;
    const double pu = g.pivot[0], pv = g.pivot[1];
    for (int e = tid; e < hw * hw; e += 256) {
        const int hy = e / hw, hx = e - hy * hw;
        const int64_t jj = (int64_t)ty0 + cy - g.r + hy, ii = (int64_t)tx0 + cx - g.r + hx;
        double val = NAN;
        if (jj >= 0 && jj < g.H && ii >= 0 && ii < g.W) {
            const double t = g.v[jj * g.W + ii];
            if (isfinite(t)) val = t - pv;
        }
        s_v[e] = val;
    }
    // the wave's copy of the tile: lane (lx, ly0) holds rows ly0, ly0 + 2, ... of column lx
    const int lx = lane & 31, ly0 = lane >> 5;
    double uu[kRegPix];
#pragma unroll
    for (int k = 0; k < kRegPix; ++k) {
        const int j = ty0 + ly0 + 2 * k, i = tx0 + lx;
        double val = NAN;
        if (j < g.H && i < g.W) {
            const double t = g.u[(int64_t)j * g.W + i];
            if (isfinite(t)) val = t - pu;
        }
        uu[k] = val;
    }
    __syncthreads();
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int s = wave; s < S; s += kRegWaves) {
        const int sy = s / side, sx = s - sy * side;
        const double* col = s_v + (ly0 + sy) * hw + lx + sx;
        double n = 0.0, su = 0.0, sv = 0.0, suu = 0.0, svv = 0.0, suv = 0.0;
#pragma unroll
        for (int k = 0; k < kRegPix; ++k) {
            const double vv = col[2 * k * hw];
            const bool ok = uu[k] == uu[k] && vv == vv;
            const double a = ok ? uu[k] : 0.0, b = ok ? vv : 0.0;
            n += ok ? 1.0 : 0.0;
            su += a;
            sv += b;
            suu += a * a;
            svv += b * b;
            suv += a * b;
        }
        n = wave_sum(n);
        su = wave_sum(su);
        sv = wave_sum(sv);
        suu = wave_sum(suu);
        svv = wave_sum(svv);
        suv = wave_sum(suv);
        if (lane < 6) {
            const double o = lane == 0 ? n : lane == 1 ? su : lane == 2 ? sv : lane == 3 ? suu : lane == 4 ? svv : suv;
            g.partial[(blk * S + s) * 6 + lane] = o;
        }
    }
}

struct PickArgs {
    const double* partial;
    int nb, r;
    const int* centre;
    int cx0, cy0;
    const double* pivot;
    int* shift_out;                   // this level's (dx, dy)
    double* table;                    // null, or [shifts + 2]: ncc in scan order, then dx, dy
    spnerf_eval_dsm_shift* result;    // null below the finest level
};

__global__ __launch_bounds__(256) void k_dsm_ncc_pick(PickArgs g) {
    __shared__ double s_m[kRegMaxShifts][7];   // muu, muv, sigu, sigv, xcorr, count, ncc
    const int side = 2 * g.r + 1, S = side * side;
    const double pu = g.pivot[0], pv = g.pivot[1];
    for (int s = threadIdx.x; s < S; s += 256) {
        double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < g.nb; ++b) {
            const double* p = g.partial + ((int64_t)b * S + s) * 6;
#pragma unroll
            for (int q = 0; q < 6; ++q) t[q] += p[q];
        }
        // mean_std from one-pass sums of the pivoted pixels; 0 / 0 = NaN without a pair
        const double n = t[0], mu = t[1] / n, mv = t[2] / n;
        const double uu = t[3] / n, vv = t[4] / n;
        double var_u = uu - mu * mu, var_v = vv - mv * mv;
        // a deviation below the rounding of its own sums (n·ε relative to the raw moment) is the
        // reference's exact 0 of a constant image: ncc = 0 / 0 there, which never wins
        const double tiny = n * 2.220446049250313e-16;
        if (var_u <= tiny * uu) var_u = 0.0;
        if (var_v <= tiny * vv) var_v = 0.0;
        const double su = sqrt(var_u), sv = sqrt(var_v);
        const double xc = (var_u == 0.0 || var_v == 0.0) ? 0.0 : t[5] / n - mu * mv;
        const double c = xc / (su * sv);
        s_m[s][0] = pu + mu;
        s_m[s][1] = pv + mv;
        s_m[s][2] = su;
        s_m[s][3] = sv;
        s_m[s][4] = xc;
        s_m[s][5] = n;
        s_m[s][6] = c;
        if (g.table) g.table[s] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int cx, cy;
        window_centre(g.centre, g.cx0, g.cy0, &cx, &cy);
        int best = g.r * side + g.r;
        double maxv = -INFINITY;
        for (int s = 0; s < S; ++s)
            if (s_m[s][6] > maxv) {
                maxv = s_m[s][6];
                best = s;
            }
        const int dx = cx - g.r + best % side, dy = cy - g.r + best / side;
        g.shift_out[0] = dx;
        g.shift_out[1] = dy;
        if (g.table) {
            g.table[S] = (double)dx;
            g.table[S + 1] = (double)dy;
        }
        if (g.result) {
            g.result->dx = dx;
            g.result->dy = dy;
            g.result->muu = s_m[best][0];
            g.result->muv = s_m[best][1];
            g.result->sigu = s_m[best][2];
            g.result->sigv = s_m[best][3];
            g.result->xcorr = s_m[best][4];
            g.result->count = (int64_t)s_m[best][5];
        }
    }
}

// a·x + b with two roundings like the reference's numpy expression: hipcc contracts a * x + b into
// one fused multiply-add by default (and its __dmul_rn / __dadd_rn are plain operators)
__device__ __forceinline__ double mul_then_add(double a, double x, double b) {
#pragma clang fp contract(off)
    const double p = a * x;
    return p + b;
}

struct ApplyArgs {
    const double* v;
    const double* u;
    int H, W;
    const spnerf_eval_dsm_shift* reg;
    int scaling, dx, dy;
    double a, b;
    double* out;
    double* err;
    double* sums;
};

__global__ __launch_bounds__(256) void k_dsm_apply_shift_err(ApplyArgs g) {
    __shared__ double s_part[kRegWaves][2];
    int dx = g.dx, dy = g.dy;
    double a = g.a, b = g.b;
    if (g.reg) {
        dx = g.reg->dx;
        dy = g.reg->dy;
        a = g.scaling ? g.reg->sigu / g.reg->sigv : 1.0;
        b = mul_then_add(-g.reg->muv, a, g.reg->muu);   // muu − muv·a, rounded like the host's
    }
    const int64_t n = (int64_t)g.H * g.W;
    double sum = 0.0, cnt = 0.0;
    for (int64_t k = blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) {
        const int64_t j = k / g.W, i = k - j * g.W;
        const int64_t jj = j + dy, ii = i + dx;
        double o = NAN;
        if (jj >= 0 && jj < g.H && ii >= 0 && ii < g.W) o = mul_then_add(a, g.v[jj * g.W + ii], b);
        if (g.out) g.out[k] = o;
        if (g.u) {
            const double e = o - g.u[k];
            if (g.err) g.err[k] = e;
            if (isfinite(e)) {
                sum += fabs(e);
                cnt += 1.0;
            }
        }
    }
    if (!g.sums) return;
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_part[wave][0] = sum;
        s_part[wave][1] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
        for (int w = 0; w < kRegWaves; ++w) t += s_part[w][threadIdx.x];
        g.sums[2 + 2 * blockIdx.x + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(64) void k_dsm_err_finish(double* sums, int nb) {
    if (threadIdx.x < 2) {
        double t = 0.0;
        for (int b = 0; b < nb; ++b) t += sums[2 + 2 * b + threadIdx.x];
        sums[threadIdx.x] = t;
    }
}

// ---- host: the pyramid's shapes and the workspace layout -----------------------------------
constexpr int kRegMaxLevels = 16;
struct RegPlan {
    int levels;                                   // 1 + the 2x reductions
    int h[kRegMaxLevels], w[kRegMaxLevels];
    int64_t off_u[kRegMaxLevels], off_v[kRegMaxLevels];   // bytes; level 0 is the caller's images
    int64_t off_pivot, off_shift, off_partial, bytes;
};

static int32_t reg_plan(int32_t H, int32_t W, int32_t irange, RegPlan* p) {
    SPN_ARG(H > 0 && W > 0 && H <= SPNERF_EVAL_DSM_MAX_SIDE && W <= SPNERF_EVAL_DSM_MAX_SIDE,
            "dsm_register: bad shape %d x %d (1..%d)", H, W, SPNERF_EVAL_DSM_MAX_SIDE);
    SPN_ARG(irange >= 0 && irange <= SPNERF_EVAL_DSM_MAX_IRANGE, "dsm_register: irange %d outside 0..%d", irange,
            SPNERF_EVAL_DSM_MAX_IRANGE);
    p->levels = 1;
    p->h[0] = H;
    p->w[0] = W;
    while (std::min(p->h[p->levels - 1], p->w[p->levels - 1]) > 100) {   // recursive_ncc's condition
        p->h[p->levels] = (p->h[p->levels - 1] + 1) / 2;
        p->w[p->levels] = (p->w[p->levels - 1] + 1) / 2;
        ++p->levels;
    }
    int64_t off = 0;
    p->off_pivot = off;
    off += 16;
    p->off_shift = off;
    off += ((int64_t)p->levels * 2 * sizeof(int32_t) + 15) / 16 * 16;
    p->off_u[0] = p->off_v[0] = -1;
    for (int l = 1; l < p->levels; ++l) {
        const int64_t img = ((int64_t)p->h[l] * p->w[l] * sizeof(double) + 15) / 16 * 16;
        p->off_u[l] = off;
        p->off_v[l] = off + img;
        off += 2 * img;
    }
    const int side = 2 * irange + 1;
    p->off_partial = off;
    off += (int64_t)cdiv(H, kRegTile) * cdiv(W, kRegTile) * side * side * 6 * sizeof(double);
    p->bytes = off;
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_eval_abi_version(void) { return SPNERF_EVAL_ABI_VERSION; }

extern "C" int64_t spnerf_eval_dsm_register_workspace_bytes(int32_t H, int32_t W, int32_t irange) {
    RegPlan p;
    const int32_t rc = reg_plan(H, W, irange, &p);
    return rc == SPNERF_OK ? p.bytes : (int64_t)rc;
}

extern "C" int32_t spnerf_eval_dsm_down2x(const double* in, int32_t H, int32_t W, double* out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    SPN_ARG(in && out, "dsm_down2x: NULL image");
    SPN_ARG(H > 0 && W > 0 && H <= SPNERF_EVAL_DSM_MAX_SIDE && W <= SPNERF_EVAL_DSM_MAX_SIDE,
            "dsm_down2x: bad shape %d x %d (1..%d)", H, W, SPNERF_EVAL_DSM_MAX_SIDE);
    const int oh = (H + 1) / 2, ow = (W + 1) / 2;
    hipLaunchKernelGGL(k_dsm_down2x, dim3((unsigned)cdiv((int64_t)oh * ow, 256)), dim3(256), 0, s, in, H, W, out, oh, ow);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_eval_dsm_register(const double* u, const double* v, int32_t H, int32_t W, int32_t irange,
                                            int32_t init_dx, int32_t init_dy, void* workspace, double* ncc_tables,
                                            spnerf_eval_dsm_shift* result, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    SPN_ARG(u && v && workspace && result, "dsm_register: NULL image, workspace or result");
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "dsm_register: workspace not 16-byte aligned");
    SPN_ARG(std::abs((int64_t)init_dx) <= SPNERF_EVAL_DSM_MAX_INIT && std::abs((int64_t)init_dy) <= SPNERF_EVAL_DSM_MAX_INIT,
            "dsm_register: initial shift (%d, %d) beyond +-%d", init_dx, init_dy, SPNERF_EVAL_DSM_MAX_INIT);
    RegPlan p;
    SPN_TRY(reg_plan(H, W, irange, &p));
    char* ws = (char*)workspace;
    double* pivot = (double*)(ws + p.off_pivot);
    int* shifts = (int*)(ws + p.off_shift);
    double* partial = (double*)(ws + p.off_partial);
    const int side = 2 * irange + 1, S = side * side;
    ProfScope prof("dsm_register", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_dsm_pivot, dim3(1), dim3(256), 0, s, u, v, H * W, pivot);
    const double* lu[kRegMaxLevels];
    const double* lv[kRegMaxLevels];
    lu[0] = u;
    lv[0] = v;
    for (int l = 1; l < p.levels; ++l) {
        double* du = (double*)(ws + p.off_u[l]);
        double* dv = (double*)(ws + p.off_v[l]);
        const unsigned nb = (unsigned)cdiv((int64_t)p.h[l] * p.w[l], 256);
        hipLaunchKernelGGL(k_dsm_down2x, dim3(nb), dim3(256), 0, s, lu[l - 1], p.h[l - 1], p.w[l - 1], du, p.h[l], p.w[l]);
        hipLaunchKernelGGL(k_dsm_down2x, dim3(nb), dim3(256), 0, s, lv[l - 1], p.h[l - 1], p.w[l - 1], dv, p.h[l], p.w[l]);
        lu[l] = du;
        lv[l] = dv;
    }
    // dx // 2 per level on the way down: an arithmetic shift floors negative values too
    const int top = p.levels - 1;
    const int cx0 = init_dx >> top, cy0 = init_dy >> top;
    const size_t lds = (size_t)(kRegTile + 2 * irange) * (kRegTile + 2 * irange) * sizeof(double);
    for (int l = top; l >= 0; --l) {
        const int* centre = l == top ? nullptr : shifts + 2 * (l + 1);
        const dim3 grid((unsigned)cdiv(p.w[l], kRegTile), (unsigned)cdiv(p.h[l], kRegTile));
        NccArgs m{lu[l], lv[l], p.h[l], p.w[l], irange, centre, cx0, cy0, pivot, partial};
        hipLaunchKernelGGL(k_dsm_ncc_moments, grid, dim3(256), lds, s, m);
        PickArgs k{partial, (int)(grid.x * grid.y), irange, centre, cx0, cy0, pivot, shifts + 2 * l,
                   ncc_tables ? ncc_tables + (int64_t)l * (S + 2) : nullptr, l == 0 ? result : nullptr};
        hipLaunchKernelGGL(k_dsm_ncc_pick, dim3(1), dim3(256), 0, s, k);
    }
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_eval_dsm_apply_shift(const double* v, int32_t H, int32_t W, const spnerf_eval_dsm_shift* reg,
                                               int32_t scaling, int32_t dx, int32_t dy, double a, double b,
                                               const double* u, double* out, double* err, double* sums, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    SPN_ARG(v != nullptr, "dsm_apply_shift: NULL image");
    SPN_ARG(H > 0 && W > 0 && H <= SPNERF_EVAL_DSM_MAX_SIDE && W <= SPNERF_EVAL_DSM_MAX_SIDE,
            "dsm_apply_shift: bad shape %d x %d (1..%d)", H, W, SPNERF_EVAL_DSM_MAX_SIDE);
    SPN_ARG(u || (!err && !sums), "dsm_apply_shift: err and sums need the reference image u");
    SPN_ARG(out || err || sums, "dsm_apply_shift: no output asked for");
    const int nb = std::min(cdiv((int64_t)H * W, 256), kErrBlocks);
    ApplyArgs g{v, u, H, W, reg, scaling ? 1 : 0, dx, dy, a, b, out, err, sums};
    ProfScope prof("dsm_register", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_dsm_apply_shift_err, dim3((unsigned)nb), dim3(256), 0, s, g);
    if (sums) hipLaunchKernelGGL(k_dsm_err_finish, dim3(1), dim3(64), 0, s, sums, nb);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
