// The march of include/spnerf_amd_shadow.h, shared by the shadow cast (shadow.hip) and the visibility
// floor (occlusion.hip): one direction prepared on the host, the workgroup's hmax from the partial
// maxima, and the DDA of one cell along the direction's major axis.  Stated once, so the cast and the
// floor visit the same steps, read the same heights and stop at the same bound.
#pragma once
#include <cmath>

#include "common.h"
#include "wave.h"

namespace spn {

constexpr int kShadowThreads = 256;
constexpr int kShadowTileW = 64, kShadowTileH = kShadowThreads / kShadowTileW;   // a wavefront per row of the tile
constexpr int kShadowMaxParts = 256;      // partial maxima: 2 KiB, reduced by the first wavefront of every marching workgroup

// the partial maxima of the non-NaN heights, one launch into `part` (shadow.hip); hmax_parts entries
int hmax_parts(int64_t cells);
void launch_shadow_hmax(const double* dsm, int64_t cells, double* part, hipStream_t st);

// One direction's march, prepared on the host: axis 0 steps along the columns, 1 along the rows,
// -1 takes no step (a = b = 0); sgn is the step's sign along that axis.
struct ShadowDir {
    double q, rho;
    int32_t axis, sgn;
};

// s = (east, north, up) as the header takes it
inline ShadowDir shadow_dir(const float* s, double resolution) {
    const double a = (double)s[0], b = -(double)s[1], u = (double)s[2];
    ShadowDir d{};
    if (a == 0.0 && b == 0.0) {
        d.axis = -1;
    } else if (std::fabs(a) >= std::fabs(b)) {
        d.axis = 0; d.sgn = a > 0.0 ? 1 : -1;
        d.q = b / std::fabs(a); d.rho = resolution * u / std::fabs(a);
    } else {
        d.axis = 1; d.sgn = b > 0.0 ? 1 : -1;
        d.q = a / std::fabs(b); d.rho = resolution * u / std::fabs(b);
    }
    return d;
}

// hmax of the grid from the partial maxima, by the first wavefront of the workgroup; ends in a barrier
__device__ __forceinline__ double block_hmax(const double* __restrict__ part, int nparts, double* s_hmax) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        double v = -INFINITY;
        for (int p = tid; p < nparts; p += 64) v = fmax(v, part[p]);
        v = wave_max(v);
        if (tid == 0) *s_hmax = v;
    }
    __syncthreads();
    return *s_hmax;
}

// The march of cell (j, i) against the reference height h: the maximum over the contributing steps of
// ((height - h) - m·rho), -inf when there is none.  It stops once the bound (hmax - h) - m·rho is <= the
// running maximum; with want == false also at the first positive value or once the bound is <= 0.
// h = 0 gives max(height - m·rho): x - 0 is x, so nothing is rounded that the floor does not state.
__device__ __forceinline__ double shadow_march(const double* __restrict__ dsm, int H, int W, int j, int i, const ShadowDir d, double hmax,
                                               double h, bool want) {
#pragma clang fp contract(off)
    double run = -INFINITY;
    if (d.axis >= 0) {
        // major: the axis the march steps along; minor: the one it interpolates along
        const int maj0 = d.axis ? j : i, min0 = d.axis ? i : j;
        const int nmaj = d.axis ? H : W, nmin = d.axis ? W : H;
        const int64_t smaj = d.axis ? W : 1, smin = d.axis ? 1 : W;
        const double top = hmax - h, last = (double)(nmin - 1);
        for (int m = 1;; ++m) {
            const int c = maj0 + m * d.sgn;
            if (c < 0 || c >= nmaj) break;
            const double dm = (double)m;
            const double drop = dm * d.rho;
            // no step from m on exceeds top - drop; without `want` a non-positive value changes nothing
            const double bound = top - drop;
            if (bound <= run || (!want && bound <= 0.0)) break;
            const double y = (double)min0 + dm * d.q;
            if (!(y >= 0.0 && y <= last)) break;   // y is monotone in m: it has left for good
            const double fl = floor(y), f = y - fl;
            const double* p = dsm + (int64_t)c * smaj + (int64_t)fl * smin;   // rows floor(y) [+ 1]: inside, see above
            double hs = p[0];
            if (f != 0.0) {   // then y < nmin - 1, so floor(y) + 1 is inside
                const double h1 = p[smin];
                if (hs != hs || h1 != h1) continue;
                const double t = hs + f * (h1 - hs);
                hs = fmin(fmax(t, fmin(hs, h1)), fmax(hs, h1));
            } else if (hs != hs) {
                continue;
            }
            const double e = (hs - h) - drop;
            run = fmax(run, e);
            if (!want && e > 0.0) break;
        }
    }
    return run;
}

}  // namespace spn
