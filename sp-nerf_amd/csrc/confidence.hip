// Confidence of a pick from its score volume (include/staged/spnerf_amd_confidence.h).  One launch, one thread
// per cell, consecutive lanes on consecutive cells: every plane's read is one coalesced row of the plane-major
// volume [K][cells], and kConfBatch planes' loads are issued before the first of them is used.
//  * Pass 1 feeds spn::Pick (sweep_pick.h) — an unscored entry as NaN — and counts the scored planes.
//  * Everything else is stated relative to best and index: `support` and `peaks` compare every plane with
//    best − tau, the sums of mlm and spread are taken around best and index.  No single pass has them without
//    keeping the column, and a column of up to 512 values does not fit a lane's registers, so pass 2 reads the
//    column again (what that costs: DESIGN.md §8.21).  It walks the planes with a lag of one, so that a plane is
//    judged a local maximum when the one above it has arrived.
// The template leaves pass 2 out (SECOND) when none of its planes is asked for, and its exp (EXP) when neither mlm
// nor spread is.  No LDS, no atomics, nothing but registers.  The whole file is compiled without contraction:
// the exact planes have no product to fuse, and the fp64 sums are then what the header writes.
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "../../include/staged/spnerf_amd_confidence.h"
#include "sweep_pick.h"

namespace spn {

constexpr int kConfThreads = 256;
constexpr int kConfBatch = 8;   // planes whose loads are in flight per lane

struct ConfOut {
    int32_t *scored, *index;
    float *margin, *peak_margin;
    int32_t *peaks, *support;
    float *curvature, *mlm, *spread;
};

// planes k0 .. k0 + kConfBatch − 1 of one cell, NaN beyond K and for an unscored entry
__device__ __forceinline__ void conf_load(const float* __restrict__ column, int64_t cells, int k0, int K, float (&v)[kConfBatch]) {
#pragma unroll
    for (int u = 0; u < kConfBatch; ++u) v[u] = k0 + u < K ? column[(int64_t)(k0 + u) * cells] : NAN;
#pragma unroll
    for (int u = 0; u < kConfBatch; ++u) v[u] = isfinite(v[u]) ? v[u] : NAN;
}

// the local maxima of the header, fed the planes in order; plane j is judged when plane j + 1 (or the end) arrives
struct ConfPeaks {
    float before = NAN, at = NAN;   // planes j − 1 and j, NaN where unscored or outside
    float other = NAN;              // the largest local maximum that is not the pick
    int peaks = 0;
    __device__ __forceinline__ void judge(int j, float after, int index, double floor_) {
        const bool is_peak = at == at && !(before == before && !(at > before)) && !(after == after && !(at >= after));
        if (is_peak) {
            if (j != index && !(other >= at)) other = at;
            if ((double)at >= floor_) ++peaks;
        }
    }
    __device__ __forceinline__ void plane(int k, float s, int index, double floor_) {
        if (k > 0) judge(k - 1, s, index, floor_);
        before = at;
        at = s;
    }
};

//   volume [K][cells]; every plane of `out` [cells] or NULL
template <bool SECOND, bool EXP>
__global__ __launch_bounds__(kConfThreads) void k_conf_volume(const float* __restrict__ volume, int K, int64_t cells, double step, float tau,
                                                              float temperature, int exclude, ConfOut out) {
    const int64_t cell = blockIdx.x * (int64_t)kConfThreads + threadIdx.x;
    if (cell >= cells) return;
    const float* __restrict__ column = volume + cell;
    Pick p;
    int scored = 0;
    for (int k0 = 0; k0 < K; k0 += kConfBatch) {
        float v[kConfBatch];
        conf_load(column, cells, k0, K, v);
#pragma unroll
        for (int u = 0; u < kConfBatch; ++u) {
            if (k0 + u < K) {
                p.plane(k0 + u, v[u], 0);
                scored += v[u] == v[u] ? 1 : 0;
            }
        }
    }
    const int index = p.index;
    const float best = p.best;
    if (out.scored) out.scored[cell] = scored;
    if (out.index) out.index[cell] = index;
    if (out.curvature) {
        float c = NAN;
        if (index > 0 && index < K - 1 && p.below == p.below && p.above == p.above)
            c = (float)(-(((double)p.below - 2.0 * (double)best) + (double)p.above));
        out.curvature[cell] = c;
    }
    if (!SECOND) return;

    float second = NAN;
    int support = 0;
    double Z = 0.0, V = 0.0;
    ConfPeaks pk;
    if (index >= 0) {
        const double floor_ = (double)best - (double)tau;
        for (int k0 = 0; k0 < K; k0 += kConfBatch) {
            float v[kConfBatch];
            conf_load(column, cells, k0, K, v);
#pragma unroll
            for (int u = 0; u < kConfBatch; ++u) {
                const int k = k0 + u;
                if (k < K) {
                    const float s = v[u];
                    pk.plane(k, s, index, floor_);
                    if (s == s) {
                        const int d = k - index;
                        if ((d > exclude || -d > exclude) && !(second >= s)) second = s;
                        if ((double)s >= floor_) ++support;
                        if (EXP) {
                            const double e = exp(((double)s - (double)best) / (double)temperature);
                            Z += e;
                            V += e * (double)(d * d);
                        }
                    }
                }
            }
        }
        pk.judge(K - 1, NAN, index, floor_);
    }
    if (out.margin) out.margin[cell] = second == second ? best - second : NAN;
    if (out.peak_margin) out.peak_margin[cell] = pk.other == pk.other ? best - pk.other : NAN;
    if (out.peaks) out.peaks[cell] = pk.peaks;
    if (out.support) out.support[cell] = support;
    if (EXP) {
        const double mlm = 1.0 / Z;
        if (out.mlm) out.mlm[cell] = index >= 0 ? (float)mlm : NAN;
        if (out.spread) out.spread[cell] = index >= 0 ? (float)(step * sqrt(V * mlm)) : NAN;
    }
}

static bool conf_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_conf_abi_version(void) { return SPNERF_CONF_ABI_VERSION; }

extern "C" int32_t spnerf_conf_volume(const float* volume, int32_t n_planes, int64_t cells, double alt_lo, double step, float tau,
                                      float temperature, int32_t exclude, int32_t* scored, int32_t* index, float* margin,
                                      float* peak_margin, int32_t* peaks, int32_t* support, float* curvature, float* mlm, float* spread,
                                      void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SPN_ARG(volume, "conf_volume: NULL volume");
    SPN_ARG(n_planes >= 1 && n_planes <= SPNERF_CONF_MAX_PLANES, "conf_volume: n_planes %d outside [1, %d]", n_planes, SPNERF_CONF_MAX_PLANES);
    SPN_ARG(cells >= 1 && cells <= ((int64_t)1 << 32), "conf_volume: cells %lld outside [1, 2^32]", (long long)cells);
    SPN_ARG(std::isfinite(alt_lo), "conf_volume: alt_lo %g is not finite", alt_lo);
    SPN_ARG(step > 0.0 && std::isfinite(step), "conf_volume: step %g must be finite and > 0", step);
    SPN_ARG(std::isfinite(tau) && tau >= 0.0f, "conf_volume: tau %g must be finite and >= 0", (double)tau);
    SPN_ARG(std::isfinite(temperature) && temperature > 0.0f, "conf_volume: temperature %g must be finite and > 0", (double)temperature);
    SPN_ARG(exclude >= 1, "conf_volume: exclude %d must be >= 1", exclude);
    const void* planes[SPNERF_CONF_OUTPUTS] = {scored, index, margin, peak_margin, peaks, support, curvature, mlm, spread};
    int written = 0;
    for (const void* q : planes) {
        if (!q) continue;
        ++written;
        SPN_ARG(!conf_overlap(q, cells * 4, volume, (int64_t)n_planes * cells * 4), "conf_volume: an output overlaps volume");
    }
    SPN_ARG(written > 0, "conf_volume: every output is NULL");
    const bool exps = mlm || spread, second = exps || margin || peak_margin || peaks || support;
    const double entries = (double)n_planes * (double)cells;
    ProfScope prof("conf_volume", st, exps ? entries : 0.0, entries * 4.0 + (double)cells * 4.0 * written);
    const ConfOut out{scored, index, margin, peak_margin, peaks, support, curvature, mlm, spread};
    const dim3 grid((unsigned)((cells + kConfThreads - 1) / kConfThreads)), block(kConfThreads);
    if (exps) hipLaunchKernelGGL((k_conf_volume<true, true>), grid, block, 0, st, volume, n_planes, cells, step, tau, temperature, exclude, out);
    else if (second) hipLaunchKernelGGL((k_conf_volume<true, false>), grid, block, 0, st, volume, n_planes, cells, step, tau, temperature, exclude, out);
    else hipLaunchKernelGGL((k_conf_volume<false, false>), grid, block, 0, st, volume, n_planes, cells, step, tau, temperature, exclude, out);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
