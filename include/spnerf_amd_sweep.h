/* Plane-sweep exports of libspnerf_amd.so (gfx950): a photo-consistency DSM on the UTM ground grid,
 * made from the camera images alone.  For K horizontal planes every view is put on the grid at that
 * altitude, the views are scored against each other around each cell, and the best plane per cell
 * is kept.  No MLP and no outside depth is involved: the result is a model-free altitude to hold a
 * learnt DSM against, and it feeds spnerf_rectify and spnerf_shadow_cast unchanged.
 * Occlusion is not modelled, as in any plane sweep: a view that sees a cell's plane position behind
 * higher terrain still takes part in that cell's score.
 * A separate header so that the ABIs of spnerf_amd.h and its siblings stay as they are; the
 * conventions are those of spnerf_amd_rectify.h: every function returns SPNERF_OK or a negative
 * SPNERF_E_* code with the text in spnerf_last_error, pointers are device pointers, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics — results are
 * bit-reproducible from run to run.  Cameras and images are the tables of spnerf_amd_rectify.h.
 *
 * THE DEFINITION.  Everything below is fp64 unless it says otherwise, every product, sum, quotient
 * and square root is rounded once (nothing is fused), in exactly the stated order.
 *
 * Inputs: V images [h][w][C] fp32, 2 <= V <= 16, C <= 4; V cameras; a ground grid; the planes
 * alt_k = alt_lo + k·step, k = 0..K-1, 1 <= K <= 4096, step > 0; a window radius r in 1..4, the
 * window being the (2r + 1)² cells around a cell, clipped to the grid; min_views in 2..V;
 * min_std >= 0.
 *
 * Grey.  grey[v][j][i] at plane k: the centre of cell (j, i) — easting xoff + (i + 1/2)·res,
 * northing ytop - (j + 1/2)·res, as spnerf_rectify_project states it — goes through the inverse
 * UTM once, then through camera v's RPC projection at altitude alt_k; the image is read there
 * bilinearly exactly as spnerf_rectify_sample states (same validity rule, same operation order,
 * one cast to fp32 per channel).  The C fp32 values are widened to fp64, summed in channel order
 * (c0 + c1, + c2, ...), divided by C and cast once to fp32.  valid[v][j][i] is 1 when the read is
 * valid and the grey is finite, else 0.
 *
 * Score of a cell at one plane.  Let the window hold n in-grid cells, visited in row-major order.
 * View v is usable at the cell when n >= 2, v is valid at every one of the n cells, and it passes
 * the contrast test: with mu = (sum of its window greys) / n and ss = sum of (g - mu)·(g - mu),
 * ss > n·(min_std·min_std) — strictly; with min_std = 0 that is ss > 0.  Let m be the number of
 * usable views.  If m < min_views the score is NaN.  Otherwise, with p_v(w) = (g_v(w) - mu_v) /
 * sqrt(ss_v) and S(w) = sum over the usable views, in view order, of p_v(w),
 *   score = (sum over w of S(w)·S(w) - m) / (m·(m - 1)),
 * cast once to fp32: the mean pairwise zero-normalised cross-correlation (ZNCC) of the usable
 * views, at O(V·window) instead of O(V²·window).
 *
 * Pick.  Over the fp32 scores of a cell widened to fp64: index is the lowest k whose score is the
 * largest non-NaN one (a later plane wins only by strict >), -1 where every plane is NaN.  When
 * 0 < index < K - 1, both neighbours s- and s+ of s0 = score[index] are non-NaN and
 * den = (s- - 2·s0) + s+ is < 0, offset = 0.5·(s- - s+) / den clamped to [-0.5, 0.5]; otherwise 0.
 *   altitude = (float)(alt_lo + (index + offset)·step), NaN at index -1;
 *   score = the fp32 score at index, NaN at index -1;
 *   views = m at index (uint8), 0 at index -1.
 */
#ifndef SPNERF_AMD_SWEEP_H
#define SPNERF_AMD_SWEEP_H

#include "spnerf_amd_rectify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_SWEEP_ABI_VERSION 1
#define SPNERF_SWEEP_MIN_VIEWS 2
#define SPNERF_SWEEP_MAX_VIEWS 16
#define SPNERF_SWEEP_MAX_PLANES 4096
#define SPNERF_SWEEP_MAX_RADIUS 4
#define SPNERF_SWEEP_TILE 16 /* a workgroup of the fused kernel owns TILE x TILE cells */

int32_t spnerf_sweep_abi_version(void);

/* grey and valid of every view at one altitude, one thread per cell looping over the views.
 * grid->supersample is not read.
 *   cameras  [n_views][90] fp64
 *   images   [n_views] spnerf_rectify_image
 *   grey     [n_views][ysize][xsize] fp32 (what the read and the channel mean give; NaN where the read is invalid)
 *   valid    [n_views][ysize][xsize] uint8 */
int32_t spnerf_sweep_grey(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                          int32_t n_views, int32_t channels, double alt, float* grey, uint8_t* valid, void* stream);

/* The score of every cell from a stored grey / valid pair (valid: 1 counts, anything else does
 * not), one thread per cell.  views is m, the number of usable views, whatever min_views is.
 *   grey     [n_views][ysize][xsize] fp32
 *   valid    [n_views][ysize][xsize] uint8
 *   score    [ysize][xsize] fp32
 *   views    [ysize][xsize] uint8 */
int32_t spnerf_sweep_score(const float* grey, const uint8_t* valid, int32_t n_views, int32_t ysize, int32_t xsize,
                           int32_t radius, int32_t min_views, double min_std, float* score, uint8_t* views, void* stream);

/* The pick over K stored score planes, one thread per cell.
 *   volume     [n_planes][cells] fp32
 *   views_vol  [n_planes][cells] uint8
 *   altitude, score [cells] fp32; index [cells] int32; views [cells] uint8 */
int32_t spnerf_sweep_pick(const float* volume, const uint8_t* views_vol, int32_t n_planes, int64_t cells, double alt_lo,
                          double step, float* altitude, float* score, int32_t* index, uint8_t* views, void* stream);

/* The three steps above in one launch, with nothing but the four result planes written: one
 * workgroup of 256 threads owns a 16 x 16 tile of cells, computes the inverse UTM of the tile and
 * its halo of `radius` cells once, and per plane fills the greys of tile and halo for all views in
 * LDS, scores its cells from there and keeps the running best in registers.  The results have the
 * bytes of the staged calls.  `volume` may be NULL; otherwise it receives the K score planes,
 * [n_planes][ysize][xsize] fp32. */
int32_t spnerf_sweep(const spnerf_ortho_grid* grid, const double* cameras, const spnerf_rectify_image* images,
                     int32_t n_views, int32_t channels, double alt_lo, double step, int32_t n_planes, int32_t radius,
                     int32_t min_views, double min_std, float* altitude, float* score, int32_t* index, uint8_t* views,
                     float* volume, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_SWEEP_H */
