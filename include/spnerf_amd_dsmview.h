/* DSM-view exports of libspnerf_amd.so (gfx950): a ground-grid DSM seen from a camera.  Every other export
 * that joins the grid and the images maps grid -> image (a cell is projected and the image read there);
 * these map image -> grid: for pixel (col, row) of a camera, the point of the DSM its line of sight meets
 * first.  With it a DSM (a sweep's, a lidar's, a trained network's) becomes an altitude and a depth image of a
 * camera, any raster on the grid can be read at the hits, and a swept DSM with its score becomes the
 * per-pixel depth priors the trainer is supervised by.  A separate header so that the ABIs of
 * spnerf_amd_surface.h and its siblings stay as they are; the conventions are theirs: every function
 * returns SPNERF_OK (or a byte count) or a negative SPNERF_E_* code with the text in spnerf_last_error,
 * pointers are device pointers, `stream` is a hipStream_t, and no call synchronises with the host,
 * allocates, or uses atomics — results are bit-reproducible from run to run.  The grid and the camera are
 * the tables of spnerf_amd_rectify.h: a camera is 90 packed doubles, already rescaled to its image.
 *
 * THE DEFINITION.  Everything below is fp64 unless it says otherwise, every product, sum, quotient and
 * square root is rounded once (nothing is fused), in exactly the stated order.
 *
 * Lattice.  Entry (r, c) of every output plane, r < n_rows, c < n_cols, is image pixel
 *   col = (double)col0 + (double)c·(double)stride,   row = (double)row0 + (double)r·(double)stride
 * (whole pixels; the image's size is not known here: any whole pixel has a line of sight).
 *
 * Localisation.  With cn = (col - col_offset) / col_scale, rn = (row - row_offset) / row_scale and
 * an = (alt - alt_offset) / alt_scale, the normalised (lon, lat) start at (-1, -1) with eps = 2.  An
 * iteration projects (lat, lon, an), (lat, lon + eps, an) and (lat + eps, lon, an) by the RPC00B quotients
 * of spnerf_amd_rectify.h to (x0, y0), (x1, y1), (x2, y2); with e1 = (x1 - x0, y1 - y0), e2 = (x2 - x0,
 * y2 - y0) and u = (cn - x0, rn - y0),
 *   lon += (u·e1) / (e1·e1) · eps,   lat += (u·e2) / (e2·e2) · eps,   then eps = 0.1.
 * The first iteration whose squared residual (x0 - cn)² + (y0 - rn)² is below 1e-18 is followed by two
 * more updates; the iteration after those (it also needs a residual below 1e-18) returns without an update,
 * and so does the 101st in any case.  Degrees are lon·lon_scale + lon_offset, lat·lat_scale + lat_offset.
 * This is the iteration of spnerf_rpc_rays.
 *
 * Segment.  The pixel is localised at alt_hi and at alt_lo, both points go through the forward transverse
 * Mercator projection of the grid's zone (Krüger's series to 6th order in n, as spnerf_dsm's) to
 * (E_hi, N_hi) and (E_lo, N_lo), and the line of sight is the straight segment between them in
 * (E, N, alt): the point at parameter t in [0, 1] is (E_hi + t·dE, N_hi + t·dN, alt_hi + t·dA) with
 * dE = E_lo - E_hi, dN = N_lo - N_hi, dA = alt_lo - alt_hi.  Its length is L = sqrt((dE·dE + dN·dN) + dA·dA).
 * In grid coordinates, where cell centres lie at whole numbers,
 *   x = (E - xoff) / res - 0.5 (columns),   y = (ytop - N) / res - 0.5 (rows, which run south),
 * the ends are (x_hi, y_hi), (x_lo, y_lo) and dx = x_lo - x_hi, dy = y_lo - y_hi.  A pixel one of whose
 * four end coordinates is not finite or exceeds 2^31 in magnitude is a miss.
 *
 * Walk.  With dx = dy = 0 the segment stands in the cell i = floor(x_hi + 0.5), j = floor(y_hi + 0.5): a
 * miss when that cell is outside the grid, h = dsm[j][i] is not finite or h < alt_lo; otherwise a hit at
 * t* = 0 when h >= alt_hi, else at t* = (alt_hi - h) / (alt_hi - alt_lo).  Otherwise the major axis is the
 * columns when |dx| >= |dy|, else the rows; stated for the columns (the rows are the transpose), with
 * a = |dx| and s = sign(dx): the first cell-centre line is c_0 = ceil(x_hi) for s > 0, floor(x_hi) for
 * s < 0, step m = 0, 1, ... stands on column c_m = c_0 + s·m at
 *   u_m = (c_m - x_hi)·s,   t_m = u_m / a,   y_m = y_hi + t_m·dy,   z_m = alt_hi + t_m·dA,
 * and the walk ends after the first step with u_m > a: that step, on the segment's line beyond its alt_lo
 * end (t_m > 1), is still taken, so that the last part of the segment is bracketed as every other part is —
 * a step of a steep line of sight descends many metres, and a surface met after the last centre line
 * inside the segment would otherwise be lost.  A step contributes when 0 <= c_m <= xsize - 1,
 * 0 <= y_m <= ysize - 1 and the height under it is finite: dsm[floor(y_m)][c_m] widened to fp64 when y_m is
 * whole, else
 *   h0 + f·(h1 - h0),  h0 = dsm[floor(y_m)][c_m], h1 = dsm[floor(y_m) + 1][c_m], f = y_m - floor(y_m),
 * kept within [min(h0, h1), max(h0, h1)], both finite — the height of spnerf_shadow_cast's march; a step
 * over a NaN or ±inf entry contributes nothing: such cells are transparent.  Its excess is
 * e_m = z_m - height.  The hit is the first contributing step k with e_k <= 0.  When an earlier step
 * contributed, p the last one (e_p > 0),
 *   t* = t_p + (t_k - t_p)·(e_p / (e_p - e_k));
 * when none did, t* = t_k.  The walk stops there.  A crossing with t* > 1 lies below alt_lo and is a miss, and
 * so is a walk without such a step: it left the grid, or reached alt_lo.  A segment that crosses no
 * cell-centre line of its major axis has one step, the one beyond its end, and is a miss.
 *
 * Outputs at a hit:
 *   altitude = (float)(alt_hi + t*·dA)
 *   ground   = (E_hi + t*·dE, N_hi + t*·dN)
 *   cell     = ((float)min(max(x_hi + t*·dx, 0), xsize - 1), (float)min(max(y_hi + t*·dy, 0), ysize - 1))
 *   depth    = (float)(t*·L)   — metres along the segment from its alt_hi end, in the (E, N, alt) metric
 * and at a miss hit = 0 and every other entry NaN.
 *
 * The walk of a pixel skips, without changing any output, the steps that stand above every height: a max
 * reduction of the finite heights (a launch of its own, into `workspace`) gives hmax, z_m does not rise
 * with m, and a step with z_m > hmax has a positive excess or none.
 *
 * Sample.  A raster on the grid read at a `cell` entry (x, y), both widened to fp64.  The result is NaN
 * unless 0 <= x <= xsize - 1 and 0 <= y <= ysize - 1 (a miss's NaN fails that).  Mode SPNERF_DSMVIEW_NEAREST
 * is raster[floor(y + 0.5)][floor(x + 0.5)], whatever it holds.  Mode SPNERF_DSMVIEW_BILINEAR: x0 = floor(x),
 * s = x - x0, y0 = floor(y), t = y - y0, columns ia = x0, ib = min(x0 + 1, xsize - 1), rows ja, jb likewise;
 * the four entries h = raster[ja][ia], raster[ja][ib], raster[jb][ia], raster[jb][ib] widened to fp64 with
 * the weights w = (1 - t)·(1 - s), (1 - t)·s, t·(1 - s), t·s, in that order.  Starting from num = 0 and
 * den = 0, every finite entry, in that order, adds w·h to num (a product, then a sum) and w to den;
 *   out = (float)(num / den) when den > 0, NaN otherwise:
 * non-finite entries are left out and the weights of the others renormalised.
 *
 * ECEF.  (E, N) goes through the inverse transverse Mercator projection of spnerf_ortho_rays (Krüger's
 * series and Newton steps) to (lat, lon) in degrees, and with the altitude widened to fp64 through
 *   N' = A / sqrt(1 - e2·sin²(lat)),  e2 = 1 - B²/A²,  A = 6378137, B = 6356752.314245,
 *   X = (N' + alt)·cos(lat)·cos(lon),  Y = (N' + alt)·cos(lat)·sin(lon),  Z = ((B²/A²)·N' + alt)·sin(lat),
 * the geodetic-to-ECEF formula of spnerf_rpc_rays.  NaN propagates.
 */
#ifndef SPNERF_AMD_DSMVIEW_H
#define SPNERF_AMD_DSMVIEW_H

#include "spnerf_amd_rectify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_DSMVIEW_ABI_VERSION 1
#define SPNERF_DSMVIEW_NEAREST 0
#define SPNERF_DSMVIEW_BILINEAR 1

int32_t spnerf_dsmview_abi_version(void);

/* Bytes of workspace spnerf_dsmview_cast needs for a grid of ysize x xsize cells, or a negative code. */
int64_t spnerf_dsmview_workspace_bytes(int32_t ysize, int32_t xsize);

/* The cast: one thread per pixel of the lattice, a workgroup on a 16 x 16 patch of it.
 * grid->supersample is not read.
 *   dsm        [ysize][xsize] fp32, row 0 the northernmost
 *   camera     [90] fp64
 *   alt_lo, alt_hi   finite, alt_hi > alt_lo
 *   col0, row0, stride >= 1, n_cols, n_rows >= 1   the lattice; its last pixel must fit an int32
 *   workspace  at least ..._workspace_bytes(ysize, xsize) bytes, 16-byte aligned
 *   hit        [n_rows][n_cols] uint8: 1 hit, 0 miss
 *   altitude   [n_rows][n_cols] fp32
 *   ground     [n_rows][n_cols][2] fp64 (E, N)
 *   cell       [n_rows][n_cols][2] fp32 (x, y)
 *   depth      [n_rows][n_cols] fp32 */
int32_t spnerf_dsmview_cast(const spnerf_ortho_grid* grid, const float* dsm, const double* camera, double alt_lo, double alt_hi,
                            int32_t col0, int32_t row0, int32_t stride, int32_t n_cols, int32_t n_rows, void* workspace,
                            uint8_t* hit, float* altitude, double* ground, float* cell, float* depth, void* stream);

/* raster [ysize][xsize] fp32 read at cell [count][2] fp32 into out [count] fp32, one thread per entry. */
int32_t spnerf_dsmview_sample(const float* raster, int32_t ysize, int32_t xsize, const float* cell, int64_t count, int32_t mode,
                              float* out, void* stream);

/* ground [count][2] fp64 (E, N) in UTM `zone` (south != 0: the southern hemisphere) and altitude [count] fp32
 * to ecef [count][3] fp64, one thread per entry. */
int32_t spnerf_dsmview_ecef(const double* ground, const float* altitude, int64_t count, int32_t zone, int32_t south, double* ecef,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_DSMVIEW_H */
