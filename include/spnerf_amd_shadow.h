/* Geometric-shadow exports of libspnerf_amd.so (gfx950): a ground-grid DSM cast under K sun
 * directions — a cell is shadowed when the terrain between it and the sun rises above the sun ray
 * — and the agreement of a learnt sun plane (relight_ortho's "sun") with those shadows.  No MLP is
 * involved: the DSM may be render_ortho's, the lidar truth or any registered raster.
 * A separate header so that the ABIs of spnerf_amd.h and its siblings stay as they are; the
 * conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code with
 * the text in spnerf_last_error, pointers are device pointers unless said otherwise, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics on global memory
 * — results are bit-reproducible from run to run.  All arithmetic is fp64.
 */
#ifndef SPNERF_AMD_SHADOW_H
#define SPNERF_AMD_SHADOW_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_SHADOW_ABI_VERSION 1
#define SPNERF_SHADOW_MAX_DIRS 65535 /* K of one call (a grid dimension of the launches) */

/* What spnerf_shadow_agreement leaves on the device, one per direction.  A cell counts when its
 * shadow is 0 or 1 and its sun is finite; the learnt prediction of "shadowed" is sun < 0.5. */
typedef struct spnerf_shadow_agreement_result {
    double sum_sun_lit;    /* sum of sun over the counted cells with shadow 0 */
    double sum_sun_shadow; /* ... with shadow 1 */
    double sum_abs;        /* sum of |sun - (1 - shadow)| over the counted cells */
    int64_t n_lit, n_shadow;
    int64_t tp, fp, fn;    /* shadow 1 & sun < 0.5;  shadow 0 & sun < 0.5;  shadow 1 & not sun < 0.5 */
} spnerf_shadow_agreement_result;

int32_t spnerf_shadow_abi_version(void);

/* Bytes of workspace spnerf_shadow_cast needs for an H x W grid, or a negative code. */
int64_t spnerf_shadow_workspace_bytes(int32_t height, int32_t width);

/* Cast the DSM under K sun directions, one thread per (direction, cell).  For cell (j, i) of height
 * h and direction s = (e, n, u) — east, north, up, pointing from the ground towards the sun, u > 0 —
 * let a = e (along the columns) and b = -n (along the rows, which run south).  With a = b = 0 no step
 * is taken.  Otherwise the major axis is the columns when |a| >= |b|, else the rows; stated for the
 * columns (the rows are the transpose): step m = 1, 2, ... visits column i' = i + m·sign(a) at row
 * position y = j + m·q, q = b/|a|.  The height there is dsm[floor(y)][i'] when y is whole, else
 *   h0 + f·(h1 - h0),  h0 = dsm[floor(y)][i'], h1 = dsm[floor(y) + 1][i'], f = y - floor(y),
 * kept within [min(h0, h1), max(h0, h1)]; a step that needs a NaN height contributes nothing.  The
 * march ends when i' leaves the grid or y leaves [0, H - 1].  The sun ray stands at h + m·rho,
 * rho = resolution·u/|a|, and
 *   excess = max over the contributing steps of ((height - h) - m·rho),  -inf when there is none,
 *   shadow = 1 where excess > 0, else 0;   where h is NaN: excess NaN, shadow 255.
 * Every product and sum is rounded once (nothing is fused), q and rho are computed on the host.
 *
 * The march of a cell stops early, without changing either output: a max reduction of the heights
 * that are not NaN (a launch of its own, into `workspace`) gives hmax, no step from m on can exceed
 * (hmax - h) - m·rho, and that bound falls with m.  With `excess` the march stops once the bound is
 * <= the running maximum; without it also at the first positive excess or once the bound is <= 0.
 *   dsm        [height][width] fp64, row 0 the northernmost
 *   dirs       HOST pointer, [n_dirs][3] fp32; every component finite, up > 0
 *   workspace  at least ..._workspace_bytes(height, width) bytes, 16-byte aligned
 *   shadow     [n_dirs][height][width] uint8
 *   excess     NULL, or [n_dirs][height][width] fp64 (metres) */
int32_t spnerf_shadow_cast(const double* dsm, int32_t height, int32_t width, double resolution, const float* dirs,
                           int32_t n_dirs, void* workspace, uint8_t* shadow, double* excess, void* stream);

/* Bytes of workspace spnerf_shadow_agreement needs, or a negative code. */
int64_t spnerf_shadow_agreement_workspace_bytes(int64_t cells, int32_t n_dirs);

/* One pass over a learnt sun plane and a shadow plane, then a single-workgroup finish: fp64 sums and
 * int64 counts per direction, per-workgroup partials summed in workgroup order.
 *   sun        [n_dirs][cells] fp32
 *   shadow     [n_dirs][cells] uint8 (spnerf_shadow_cast's: 0 lit, 1 shadowed, anything else is skipped)
 *   workspace  at least ..._workspace_bytes(cells, n_dirs) bytes, 16-byte aligned
 *   result     [n_dirs] spnerf_shadow_agreement_result */
int32_t spnerf_shadow_agreement(const float* sun, const uint8_t* shadow, int64_t cells, int32_t n_dirs, void* workspace,
                                spnerf_shadow_agreement_result* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_SHADOW_H */
