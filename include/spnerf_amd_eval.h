/* Evaluation-side exports of libspnerf_amd.so (gfx950): DSM registration by multiscale
 * normalised cross correlation (the reference's modules/dsmr.py) and the registered error map.
 * A separate header from spnerf_amd.h so that the render / training ABI stays as it is; the
 * conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code with
 * the text in spnerf_last_error, pointers are device pointers unless noted, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics on global
 * memory — results are bit-reproducible from run to run.
 *
 * Images are row-major fp64 [H][W]; non-finite pixels are missing data.  A shift (dx, dy) pairs
 * u[j][i] with v[j + dy][i + dx].
 */
#ifndef SPNERF_AMD_EVAL_H
#define SPNERF_AMD_EVAL_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_EVAL_ABI_VERSION 1
#define SPNERF_EVAL_DSM_MAX_IRANGE 8   /* the search window is (2·irange + 1)² shifts per level   */
#define SPNERF_EVAL_DSM_MAX_SIDE 32768 /* H, W                                                    */
#define SPNERF_EVAL_DSM_MAX_INIT 65536 /* |initial dx|, |initial dy|                              */
/* doubles behind `sums` of the apply call: [0] Σ|err|, [1] finite count, the rest block partials */
#define SPNERF_EVAL_DSM_SUMS_DOUBLES (2 + 2 * 256)

/* What a registration leaves on the device (56 bytes): the shift, then mean_std at that shift
 * over the finest level — the means and (population) deviations of the paired pixels of u and v,
 * their covariance, and the number of pairs.  The moments are NaN when count is 0. */
typedef struct spnerf_eval_dsm_shift {
    int32_t dx, dy;
    double muu, muv, sigu, sigv, xcorr;
    int64_t count;
} spnerf_eval_dsm_shift;

int32_t spnerf_eval_abi_version(void);

/* Pyramid levels of an H x W pair: 1 + the number of 2x reductions (ceil) made while
 * min(H, W) > 100.  Bytes of workspace a registration of that shape needs, or a negative code. */
int64_t spnerf_eval_dsm_register_workspace_bytes(int32_t H, int32_t W, int32_t irange);

/* downsample2x of modules/dsmr.py, one pyramid step: out[ceil(H/2)][ceil(W/2)], each cell the mean
 * of the finite pixels of a 2x2 block of `in` (NaN when it has none), bit-equal to the reference
 * — whose loop leaves in cell (J, I) the block starting at (min(2J+1, H−1), min(2I+1, W−1)). */
int32_t spnerf_eval_dsm_down2x(const double* in, int32_t H, int32_t W, double* out, void* stream);

/* recursive_ncc + mean_std of modules/dsmr.py: the integer shift of v onto u that maximises the
 * normalised cross correlation, searched over (centre) ± irange at every level of a 2x pyramid,
 * coarsest first, each level's centre being twice the level below's result (read on the device)
 * and the coarsest's the initial shift floor-divided by 2 per level.  Ties keep the first shift
 * in scan order (y outer, x inner), a NaN correlation (no finite pair, zero deviation) never
 * wins, and the centre stands when nothing wins.
 *   u, v            [H][W] fp64
 *   workspace       at least ..._workspace_bytes(H, W, irange) bytes, 16-byte aligned
 *   ncc_tables      NULL, or [levels][(2·irange+1)² + 2] fp64, finest level first: the
 *                   correlations in scan order, then that level's chosen dx, dy as doubles
 *   result          one spnerf_eval_dsm_shift */
int32_t spnerf_eval_dsm_register(const double* u, const double* v, int32_t H, int32_t W, int32_t irange,
                                 int32_t init_dx, int32_t init_dy, void* workspace, double* ncc_tables,
                                 spnerf_eval_dsm_shift* result, void* stream);

/* apply_shift_ of modules/dsmr.py fused with the error map and its sums:
 *   out[j][i] = a · v[j + dy][i + dx] + b, NaN where the source pixel is out of range;
 *   err = out − u; sums[0] = Σ|err| and sums[1] = the count over finite err (MAE = their ratio).
 * The transform is (dx, dy, a, b), or — with `reg` non-NULL — read from a registration's result
 * on the device: its dx, dy, a = sigu / sigv if `scaling` else 1, b = muu − muv · a.
 *   v [H][W]; u NULL or [H][W]; out, err NULL or [H][W] (err needs u);
 *   sums NULL or SPNERF_EVAL_DSM_SUMS_DOUBLES doubles (needs u) */
int32_t spnerf_eval_dsm_apply_shift(const double* v, int32_t H, int32_t W, const spnerf_eval_dsm_shift* reg,
                                    int32_t scaling, int32_t dx, int32_t dy, double a, double b, const double* u,
                                    double* out, double* err, double* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_EVAL_H */
