/* Occlusion exports of libspnerf_amd.so (gfx950): the visibility floor of a ground-grid DSM under V
 * lines of sight, and the plane sweep of spnerf_amd_sweep.h with its views gated by that floor.  The
 * sweep on its own lets a view that sees a cell's plane position behind higher terrain take part in
 * that cell's score; with a prior DSM — a first sweep's, the lidar's, any registered raster — the
 * views that cannot see a cell at a plane are taken out of that plane's score.
 * A separate header so that the ABIs of spnerf_amd.h and its siblings stay as they are; the
 * conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code with the
 * text in spnerf_last_error, pointers are device pointers unless said otherwise, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics — results are
 * bit-reproducible from run to run.
 *
 * THE FLOOR.  For a direction d = (e, n, u) — east, north, up, pointing from the ground towards the
 * camera, u > 0 — floor_d(j, i) is the lowest altitude at cell (j, i) from which the camera is still
 * seen over the DSM.  The march is spnerf_shadow_cast's (spnerf_amd_shadow.h), in its words: let
 * a = e (along the columns) and b = -n (along the rows, which run south).  With a = b = 0 no step
 * is taken.  Otherwise the major axis is the columns when |a| >= |b|, else the rows; stated for the
 * columns (the rows are the transpose): step m = 1, 2, ... visits column i' = i + m·sign(a) at row
 * position y = j + m·q, q = b/|a|.  The height there is dsm[floor(y)][i'] when y is whole, else
 *   h0 + f·(h1 - h0),  h0 = dsm[floor(y)][i'], h1 = dsm[floor(y) + 1][i'], f = y - floor(y),
 * kept within [min(h0, h1), max(h0, h1)]; a step that needs a NaN height contributes nothing.  The
 * march ends when i' leaves the grid or y leaves [0, H - 1].  With rho = resolution·u/|a|,
 *   floor = max over the contributing steps of (height - m·rho),  -inf when there is none,
 * in fp64, every product and difference rounded once (nothing is fused), q and rho computed on the
 * host, the result cast once to fp32.  Step m = 0 is not taken: the DSM's own altitude at the cell
 * does not gate it, and the cell's own height is not read — a NaN cell still gets a floor.  With
 * a = b = 0 every floor is -inf.
 * The march of a cell stops early, without changing the output: a max reduction of the heights that
 * are not NaN (spnerf_shadow_cast's launch, into `workspace`) gives hmax, no step from m on can exceed
 * hmax - m·rho, that bound falls with m, and the march stops once it is <= the running maximum.
 *
 * THE GATE.  At a plane of altitude alt, view v at cell w is gated when
 *   (alt + slack) < (double)floor[v][w]
 * — the sum rounded once in fp64, the comparison strict, so a NaN floor gates nothing; slack is
 * finite and >= 0.  A gated (view, cell) is invalid for that plane exactly as a read outside the
 * image is: its valid byte is 0 and its grey is NaN.  Nothing else of spnerf_amd_sweep.h changes: a
 * view is usable at a cell only when it is valid on the whole window, so a view drops out within
 * `radius` cells of its occlusion boundary.
 */
#ifndef SPNERF_AMD_OCCLUSION_H
#define SPNERF_AMD_OCCLUSION_H

#include "spnerf_amd_sweep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_OCCLUSION_ABI_VERSION 1
#define SPNERF_OCCLUSION_MAX_VIEWS 16 /* V of one call: SPNERF_SWEEP_MAX_VIEWS */

int32_t spnerf_occlusion_abi_version(void);

/* Bytes of workspace spnerf_occlusion_floor needs for an H x W grid, or a negative code. */
int64_t spnerf_occlusion_workspace_bytes(int32_t height, int32_t width);

/* The floor of the DSM under V directions, one thread per (view, cell), after the max reduction.
 *   dsm        [height][width] fp64, row 0 the northernmost
 *   dirs       HOST pointer, [n_views][3] fp32; every component finite, up > 0; 1 <= n_views <= 16
 *   workspace  at least ..._workspace_bytes(height, width) bytes, 16-byte aligned
 *   floor      [n_views][height][width] fp32 (metres; -inf where nothing stands towards the camera) */
int32_t spnerf_occlusion_floor(const double* dsm, int32_t height, int32_t width, double resolution, const float* dirs,
                               int32_t n_views, void* workspace, float* floor, void* stream);

/* The gate on a stored grey / valid pair of one plane (as spnerf_sweep_grey writes it), in place, one
 * thread per (view, cell): a gated entry gets grey NaN and valid 0, every other entry is left as it is.
 *   grey       [n_views][cells] fp32
 *   valid      [n_views][cells] uint8
 *   floor      [n_views][cells] fp32 */
int32_t spnerf_occlusion_gate(float* grey, uint8_t* valid, const float* floor, int32_t n_views, int64_t cells, double alt,
                              double slack, void* stream);

/* spnerf_sweep with the gate applied at every plane, in one launch: the same tile, halo, LDS greys,
 * score and pick.  The floors of tile and halo are read once per tile into LDS (4·V·(16 + 2r)² bytes
 * more), a gated lane neither projects nor reads the image, and a wavefront whose 64 halo cells of one
 * view are all gated skips them.  The results have the bytes of the staged chain spnerf_sweep_grey →
 * spnerf_occlusion_gate → spnerf_sweep_score per plane → spnerf_sweep_pick; with every floor -inf or
 * NaN they are spnerf_sweep's.
 *   floor      [n_views][ysize][xsize] fp32 */
int32_t spnerf_occlusion_sweep(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                               int32_t n_views, int32_t channels, double alt_lo, double step, int32_t n_planes, int32_t radius,
                               int32_t min_views, double min_std, const float* floor, double slack, float* altitude, float* score,
                               int32_t* index, uint8_t* views, float* volume, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_OCCLUSION_H */
