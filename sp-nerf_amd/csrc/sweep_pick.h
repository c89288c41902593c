// The pick of include/spnerf_amd_sweep.h, shared by the plane sweep (sweep.hip) and the semi-global
// aggregation (sgm.hip): the running best of a cell and the scores of its two neighbouring planes, fed
// plane by plane — from a stored volume (k_sweep_pick, k_sgm_pick) or as the planes are scored (k_sweep).
#pragma once
#include <cmath>

#include "common.h"

namespace spn {

// the pick of the header, fed the planes of one cell in order
struct Pick {
    float best = NAN, prev = NAN, below = NAN, above = NAN;
    int index = -1, m = 0;
    __device__ __forceinline__ void plane(int k, float s, int views) {
        if (index >= 0 && k == index + 1) above = s;
        if (s == s && (index < 0 || (double)s > (double)best)) {
            best = s;
            index = k;
            below = prev;
            above = NAN;
            m = views;
        }
        prev = s;
    }
    __device__ __forceinline__ float altitude(int K, double alt_lo, double step) const {
        if (index < 0) return NAN;
        double off = 0.0;
        if (index > 0 && index < K - 1 && below == below && above == above) {
            const double sm = (double)below, s0 = (double)best, sp = (double)above;
            const double den = (sm - 2.0 * s0) + sp;
            if (den < 0.0) {
                off = 0.5 * (sm - sp) / den;
                off = off < -0.5 ? -0.5 : off > 0.5 ? 0.5 : off;
            }
        }
        return (float)(alt_lo + ((double)index + off) * step);
    }
};

}  // namespace spn
