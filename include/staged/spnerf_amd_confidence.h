/* Confidence exports of libspnerf_amd.so (gfx950): how unambiguous each cell's pick is, read from the
 * (K, H, W) score volume the plane sweep (spnerf_amd_sweep.h) or the semi-global aggregation
 * (spnerf_amd_sgm.h) leaves.  `score` and `photo` of the picks are the height of the peak; the planes here
 * say whether the peak stands alone.  The measures are those the stereo literature derives from a cost
 * volume alone (Hu & Mordohai 2012): the naive and the local-maximum margin, the count of near-winners,
 * the curvature at the pick, and the maximum-likelihood measure with the spread of its distribution.
 * STAGED: this header lives in include/staged/ (and its ctypes table in _confidence_abi.py, outside
 * _lib.BINDING_MODULES) because tests/test_abi_tables.py pins the list of headers in include/; both move to
 * include/spnerf_amd_confidence.h / _confidence_lib.py in the first change that may touch that test.
 * The conventions are those of spnerf_amd_sgm.h: every function returns SPNERF_OK or a negative SPNERF_E_*
 * code with the text in spnerf_last_error, pointers are device pointers, `stream` is a hipStream_t, and no
 * call synchronises with the host, allocates, or uses atomics — results are bit-reproducible from run to run.
 *
 * THE DEFINITION, per cell.  volume [K][cells] fp32, plane-major, higher is better; an entry that is NaN,
 * +inf or -inf is UNSCORED, and s_k below are the scored ones (k their plane).  tau and temperature are
 * fp32, on the score scale; tau is finite and >= 0, temperature finite and > 0; exclude >= 1.
 *
 *   scored       int32  the number of scored planes.
 *   index        int32  the lowest plane holding the largest scored value, -1 if there is none: the pick of
 *                       spnerf_amd_sweep.h (csrc/sweep_pick.h) fed NaN for every unscored entry, so where
 *                       the volume holds no ±inf these are the bytes of spnerf_sweep_pick / spnerf_sgm_pick.
 *                       best = s_index.
 * When index is -1 every fp32 plane below is NaN (0x7fc00000) and every int32 plane is 0.  Otherwise:
 *   margin       fp32   best - second, one fp32 subtraction; second is the largest scored value over the
 *                       planes with |k - index| > exclude, NaN if there is none.  The naive peak-ratio
 *                       margin: the `exclude` planes on either side of the pick belong to the same peak.
 *   peak_margin  fp32   best - s_j, one fp32 subtraction, s_j the largest LOCAL MAXIMUM with j != index; NaN if
 *                       there is none.  s_j is a local maximum if it is scored, and s_j > s_(j-1) unless
 *                       that entry is unscored or j = 0, and s_j >= s_(j+1) unless that entry is unscored
 *                       or j = K - 1.  A plateau therefore counts once, at its lowest plane, and the pick
 *                       is always a local maximum.
 *   peaks        int32  the number of local maxima with (double)s_j >= (double)best - (double)tau; the pick
 *                       is among them, so peaks >= 1.
 *   support      int32  the number of scored planes with (double)s_k >= (double)best - (double)tau: how
 *                       wide the set of near-winners is.
 *   curvature    fp32   -((below - 2·best) + above) in fp64 in that order, below and above the entries at
 *                       index - 1 and index + 1 (the denominator of the pick's parabola), cast once; NaN if
 *                       index is 0 or K - 1 or either neighbour is unscored.
 *   mlm          fp32   1 / Z,  Z = sum over the scored planes, in plane order, of
 *                       e_k = exp(((double)s_k - (double)best) / (double)temperature), everything fp64, cast
 *                       once: the maximum-likelihood measure, in (0, 1]; 1 is a lone winner.
 *   spread       fp32   step · sqrt(sum_k p_k (k - index)^2),  p_k = e_k / Z, in fp64, cast once: the RMS
 *                       distance in metres of that distribution from the pick.  Every term is
 *                       non-negative, so nothing cancels.  Meant as the `std` a depth prior carries.
 * Everything but mlm and spread is exact: compares, counts, and single roundings without a product that
 * could be contracted.  mlm and spread are held to the fp64 statement (tests/confidence_numpy.py) within
 * 4 fp32 ulps and 1e-5 relative + 1e-5·step: what an fp64 exp and the order of an fp64 sum of K <= 512
 * non-negative terms can move lies orders of magnitude below either.
 */
#ifndef SPNERF_AMD_CONFIDENCE_H
#define SPNERF_AMD_CONFIDENCE_H

#include "../spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_CONF_ABI_VERSION 1
#define SPNERF_CONF_MAX_PLANES 512
#define SPNERF_CONF_OUTPUTS 9 /* scored, index, margin, peak_margin, peaks, support, curvature, mlm, spread */

int32_t spnerf_conf_abi_version(void);

/* One launch, one thread per cell, consecutive lanes on consecutive cells.  A first pass over the planes
 * feeds the pick; everything else is stated relative to best and index, so a second pass over the same
 * column takes the margins, the counts and the fp64 sums.  The second pass is left out when only scored,
 * index and curvature are asked for, and its exp when neither mlm nor spread is.
 *   volume   [n_planes][cells] fp32, 1 <= n_planes <= 512, 1 <= cells <= 2^32
 *   alt_lo, step   the planes' altitudes, as the picks take them: finite, step > 0.  Only step enters a
 *            result (spread); alt_lo is checked and otherwise unused
 *   scored, index, peaks, support  [cells] int32;  margin, peak_margin, curvature, mlm, spread  [cells] fp32.
 *            Any of the nine may be NULL and is then not written, but not all of them; none may overlap
 *            volume */
int32_t spnerf_conf_volume(const float* volume, int32_t n_planes, int64_t cells, double alt_lo, double step, float tau,
                           float temperature, int32_t exclude, int32_t* scored, int32_t* index, float* margin, float* peak_margin,
                           int32_t* peaks, int32_t* support, float* curvature, float* mlm, float* spread, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_CONFIDENCE_H */
