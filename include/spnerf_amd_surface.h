/* Surface-sweep exports of libspnerf_amd.so (gfx950): the plane sweep of spnerf_amd_sweep.h around a base
 * surface instead of around horizontal planes.  Every sweep of spnerf_amd_sweep.h and its siblings takes K
 * planes alt_lo + k·step shared by all cells; here surface k lies at base + (off_lo + k·step), `base` a raster
 * on the ground grid: a coarser sweep's altitude resampled to this grid (the second half of a coarse-to-fine
 * pyramid), a trained network's DSM, a lidar.  A separate header so that the ABIs of spnerf_amd_sweep.h and
 * its siblings stay as they are; the conventions are theirs: every function returns SPNERF_OK or a negative
 * SPNERF_E_* code with the text in spnerf_last_error, pointers are device pointers, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics — results are
 * bit-reproducible from run to run.  Cameras, images and the grid are the tables of spnerf_amd_rectify.h.
 *
 * THE DEFINITION.  Everything below is fp64 unless it says otherwise, every product, sum, quotient and
 * square root is rounded once (nothing is fused), in exactly the stated order.
 *
 * Surface grey.  base [ysize][xsize] fp32.  The altitude of cell (j, i) at the offset `offset` is
 *   alt(j, i) = (double)base[j][i] + offset,
 * one sum.  grey[v][j][i] and valid[v][j][i] are spnerf_sweep_grey's with alt(j, i) in the place of its one
 * altitude: the same inverse UTM, projection, bilinear read, channel mean and cast.  Where base[j][i] is not
 * finite (NaN or ±inf) no view is projected: valid is 0 and grey NaN, exactly as for a read outside the image.
 *
 * Surface sweep.  Surface k lies at the offset off_k = off_lo + (double)k·step, k = 0..K-1 (a product, then a
 * sum), so cell (j, i) has the altitude (double)base[j][i] + off_k there.  The score of a cell at a surface
 * is spnerf_sweep_score's over the surface greys, the pick spnerf_sweep_pick's over the K scores with
 * alt_lo = off_lo, which gives index, score, views and a relative altitude rel (fp32, NaN at index -1);
 *   altitude = lift(base, rel).
 *
 * Lift.  out = (float)((double)base + (double)rel), elementwise: the one place where an offset becomes an
 * altitude.  NaN propagates from either side.
 *
 * Upsample.  coarse [hc][wc] fp32 lies on the grid coarsened by the integer factor f in 1..8 — the same
 * xoff, ytop and zone, cells of f·res, hc = ceil(H / f), wc = ceil(W / f) — and out [H][W] fp32 on the fine
 * grid.  For the fine cell (j, i):
 *   y = ((double)j + 0.5) / (double)f - 0.5,  j0 = floor(y),  t = y - j0;
 *   x = ((double)i + 0.5) / (double)f - 0.5,  i0 = floor(x),  s = x - i0;
 * rows ja = clamp(j0, 0, hc - 1), jb = clamp(j0 + 1, 0, hc - 1), columns ia, ib likewise from i0 and wc; the
 * four entries h = coarse[ja][ia], coarse[ja][ib], coarse[jb][ia], coarse[jb][ib] widened to fp64 with the
 * weights w = (1 - t)·(1 - s), (1 - t)·s, t·(1 - s), t·s, in that order.  Starting from num = 0 and den = 0,
 * every finite entry, in that order, adds w·h to num (a product, then a sum) and w to den;
 *   out = (float)(num / den) when den > 0, NaN otherwise
 * — that is, NaN when no finite entry has a weight above 0.  Non-finite entries (NaN, ±inf) are left out and
 * the weights of the others renormalised; at f = 1, t = s = 0 and the result is coarse[j][i] where that is
 * finite.
 */
#ifndef SPNERF_AMD_SURFACE_H
#define SPNERF_AMD_SURFACE_H

#include "spnerf_amd_sweep.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_SURFACE_ABI_VERSION 1
#define SPNERF_SURFACE_MAX_FACTOR 8

int32_t spnerf_surface_abi_version(void);

/* grey and valid of every view on the surface base + offset, one thread per cell looping over the views.
 * grid->supersample is not read.
 *   cameras  [n_views][90] fp64
 *   images   [n_views] spnerf_rectify_image
 *   base     [ysize][xsize] fp32
 *   grey     [n_views][ysize][xsize] fp32 (NaN where the read is invalid or the base not finite)
 *   valid    [n_views][ysize][xsize] uint8 */
int32_t spnerf_surface_grey(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                            int32_t n_views, int32_t channels, const float* base, double offset, float* grey, uint8_t* valid,
                            void* stream);

/* out[e] = (float)((double)base[e] + (double)rel[e]), e < count, one thread per entry; out may be base or rel. */
int32_t spnerf_surface_lift(const float* base, const float* rel, int64_t count, float* out, void* stream);

/* coarse [ceil(ysize / factor)][ceil(xsize / factor)] fp32 -> out [ysize][xsize] fp32, one thread per fine cell. */
int32_t spnerf_surface_upsample(const float* coarse, int32_t factor, int32_t ysize, int32_t xsize, float* out, void* stream);

/* The surface sweep in one launch: spnerf_sweep's kernel with the bases of a tile and its halo read once
 * into LDS as fp32 (4·(16 + 2·radius)² B more; NaN outside the grid); per surface, a lane whose base is not
 * finite writes NaN without projecting or reading the image.  The results have the bytes of
 * spnerf_surface_grey, spnerf_sweep_score per surface, spnerf_sweep_pick with alt_lo = off_lo and
 * spnerf_surface_lift.  Arguments are checked as spnerf_sweep checks them (off_lo as its alt_lo).  `volume`
 * may be NULL; otherwise it receives the K score planes, [n_planes][ysize][xsize] fp32. */
int32_t spnerf_surface_sweep(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                             int32_t n_views, int32_t channels, const float* base, double off_lo, double step, int32_t n_planes,
                             int32_t radius, int32_t min_views, double min_std, float* altitude, float* score, int32_t* index,
                             uint8_t* views, float* volume, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_SURFACE_H */
