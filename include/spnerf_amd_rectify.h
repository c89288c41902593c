/* Orthorectification exports of libspnerf_amd.so (gfx950): camera images put onto a UTM ground grid
 * over a DSM.  Every cell centre, at its DSM altitude, goes through the inverse transverse Mercator
 * projection and a camera's RPC projection to a pixel position; the image is read there bilinearly.
 * With it an ortho product can be held against the pixels it was trained on, a DSM checked for
 * photo-consistency across views, and the true orthophoto of the source imagery made (the occlusion
 * mask is spnerf_shadow_cast with a camera's line of sight in place of the sun's).  No MLP is involved.
 * A separate header so that the ABIs of spnerf_amd.h and its siblings stay as they are; the
 * conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code with
 * the text in spnerf_last_error, pointers are device pointers, `stream` is a hipStream_t, and no
 * call synchronises with the host, allocates, or uses atomics — results are bit-reproducible from
 * run to run.  Geometry is fp64 throughout.
 *
 * A camera is the 90 packed doubles of an RPC00B model, already rescaled to its image's downscale:
 *   row_offset col_offset lat_offset lon_offset alt_offset row_scale col_scale lat_scale lon_scale
 *   alt_scale, row_num[20], row_den[20], col_num[20], col_den[20].
 * A pixel position (col, row) with whole coordinates is the sample position of that pixel.  Camera
 * tables and image tables live in device memory: 64 cameras do not fit in kernel arguments.
 */
#ifndef SPNERF_AMD_RECTIFY_H
#define SPNERF_AMD_RECTIFY_H

#include "spnerf_amd_ortho.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_RECTIFY_ABI_VERSION 1
#define SPNERF_RECTIFY_MAX_VIEWS 64   /* V of one call */
#define SPNERF_RECTIFY_MAX_CHANNELS 4 /* C of the images */
#define SPNERF_RECTIFY_CAMERA_DOUBLES 90

#define SPNERF_RECTIFY_MEAN 0
#define SPNERF_RECTIFY_MEDIAN 1

/* One image of a call's table: [height][width][channels] fp32, channels the call's. */
typedef struct spnerf_rectify_image {
    const float* pixels;
    int32_t height, width;
} spnerf_rectify_image;

int32_t spnerf_rectify_abi_version(void);

/* pix[v][j][i] = (col, row) of the centre of cell (j, i) — easting xoff + (i + 1/2)·res, northing
 * ytop - (j + 1/2)·res — at altitude dsm[j][i] in camera v: the inverse UTM of the centre, once per
 * cell, then per view the RPC projection on normalised coordinates,
 *   col = P_cn(lat, lon, alt) / P_cd(...) · col_scale + col_offset,   row likewise.
 * One thread per cell loops over the views.  Both entries are NaN where the DSM is NaN.
 * grid->supersample is not read.
 *   dsm      [ysize][xsize] fp64, row 0 the northernmost
 *   cameras  [n_views][90] fp64
 *   pix      [n_views][ysize][xsize][2] fp64 */
int32_t spnerf_rectify_project(const double* dsm, const spnerf_ortho_grid* grid, const double* cameras, int32_t n_views,
                               double* pix, void* stream);

/* Read image v at pix[v]: one thread per cell loops over the views.  A cell is valid when both
 * entries of its pix are finite, 0 <= col <= width - 1 and 0 <= row <= height - 1.  With
 * x0 = floor(col), fx = col - x0, x1 = min(x0 + 1, width - 1), and y0, fy, y1 likewise,
 *   value = ((1 - fx)·p[y0][x0] + fx·p[y0][x1])·(1 - fy) + ((1 - fx)·p[y1][x0] + fx·p[y1][x1])·fy
 * per channel, the pixels widened to fp64, every product and sum rounded once (nothing is fused), in
 * exactly this order, then one cast to fp32.  An invalid cell is NaN in every channel.
 *   images   [n_views] spnerf_rectify_image
 *   pix      [n_views][cells][2] fp64
 *   rgb      [n_views][cells][channels] fp32
 *   valid    [n_views][cells] uint8: 1 valid, 0 not */
int32_t spnerf_rectify_sample(const spnerf_rectify_image* images, int32_t n_views, int32_t channels, const double* pix,
                              int64_t cells, float* rgb, uint8_t* valid, void* stream);

/* spnerf_rectify_project and spnerf_rectify_sample in one launch, the pixel positions kept in
 * registers: the bytes of the two-step path.  `pix` may be NULL; otherwise it is written as
 * spnerf_rectify_project writes it. */
int32_t spnerf_rectify(const double* dsm, const spnerf_ortho_grid* grid, const double* cameras,
                       const spnerf_rectify_image* images, int32_t n_views, int32_t channels, float* rgb, uint8_t* valid,
                       double* pix, void* stream);

/* One line of sight per view, in the form spnerf_shadow_cast takes its directions: at a ground
 * point (E, N), project (E, N, alt_lo) into the camera, localise that pixel at alt_hi (the iterative
 * inverse of csrc/rpc.h), bring the result back to UTM (E', N'), and normalise
 * (E' - E, N' - N, alt_hi - alt_lo): east, north, up from the ground towards the camera, up > 0.
 * dirs[v] is that vector at the grid's centre (xoff + xsize·res/2, ytop - ysize·res/2), cast to fp32.
 * spread[v] is the largest absolute component difference, in fp64 before the cast, between the
 * vector at any of the four grid corners and the one at the centre: what one direction per view costs.
 *   cameras  [n_views][90] fp64
 *   dirs     [n_views][3] fp32
 *   spread   [n_views] fp32 */
int32_t spnerf_rectify_view_dirs(const spnerf_ortho_grid* grid, const double* cameras, int32_t n_views, double alt_lo,
                                 double alt_hi, float* dirs, float* spread, void* stream);

/* Combine the views of every cell, one thread per cell.  Over the views whose `usable` is 1, in
 * view order, per channel in fp64: SPNERF_RECTIFY_MEAN is sum / count; SPNERF_RECTIFY_MEDIAN the
 * middle value of the sorted ones (a NaN sorts last), for an even count (a + b) / 2 of the two
 * middle values; one cast to fp32.  spread is sqrt(sum of (x - mean_c)² / (count·channels)) over
 * the usable views and the channels, channel by channel and in view order, mean_c = sum / count in
 * fp64, nothing fused, one cast: 0 for a count of 1.  A cell with count 0 is NaN in both float planes.
 *   rgb      [n_views][cells][channels] fp32
 *   usable   [n_views][cells] uint8: 1 counts, anything else does not
 *   mosaic   [cells][channels] fp32
 *   count    [cells] int32
 *   spread   [cells] fp32 */
int32_t spnerf_rectify_mosaic(const float* rgb, const uint8_t* usable, int32_t n_views, int64_t cells, int32_t channels,
                              int32_t mode, float* mosaic, int32_t* count, float* spread, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_RECTIFY_H */
