/* Ground-grid exports of libspnerf_amd.so (gfx950): one vertical ray per cell of a UTM grid, the
 * route of S-NeRF / EO-NeRF to a DSM and to true-ortho products.  A cell's altitude, albedo, class
 * and shadow are read straight off the grid the lidar ROI and the ground-truth rasters live on:
 * no per-view point cloud, no rasteriser, no holes.
 * A separate header so that the ABIs of spnerf_amd.h and its siblings stay as they are; the
 * conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code with
 * the text in spnerf_last_error, pointers are device pointers unless said otherwise, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics — results are
 * bit-reproducible from run to run.  All arithmetic is fp64 up to one final cast.
 */
#ifndef SPNERF_AMD_ORTHO_H
#define SPNERF_AMD_ORTHO_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_ORTHO_ABI_VERSION 1
#define SPNERF_ORTHO_MAX_SUPERSAMPLE 4

int32_t spnerf_ortho_abi_version(void);

/* A north-up grid of square cells in WGS-84 UTM metres: cell (j, i) — row j from the top, column
 * i from the left — covers eastings [xoff + i·res, xoff + (i + 1)·res) and northings
 * (ytop − (j + 1)·res, ytop − j·res]. */
typedef struct spnerf_ortho_grid {
    double xoff;          /* easting of the left edge */
    double ytop;          /* northing of the top edge */
    double resolution;    /* cell size, > 0 */
    int32_t xsize, ysize; /* columns, rows */
    int32_t zone;         /* UTM zone, 1..60 */
    int32_t south;        /* 0: northern false northing (0 m); 1: southern (10 000 000 m) */
    int32_t supersample;  /* s in 1..SPNERF_ORTHO_MAX_SUPERSAMPLE: s x s sub-rays per cell */
    int32_t reserved[3];
} spnerf_ortho_grid;

/* The rays of grid rows [row0, row0 + n_rows), n = n_rows·xsize·s² of them, one thread per ray.
 * Ray ((j·xsize + i)·s + a)·s + b — the s² sub-rays of a cell are contiguous — stands at
 *   E = xoff + (i + (b + ½)/s)·res,   N = ytop − (j + (a + ½)/s)·res,
 * goes to (lat, lon) by the inverse of the transverse Mercator projection (Krüger's series to n⁶,
 * then Newton steps on tan(lat) to fp64 convergence), to the two ECEF points p_max, p_min at
 * max_alt and min_alt on the ellipsoid normal (the constants of the reference's geodetic_to_ecef),
 * and is written as
 *   o = (p_max − center) / range,  d = unit(p_min − p_max),  near = 0,  far = ‖p_min − p_max‖ / range
 * in columns 0..7; with ray_stride 11 columns 8..10 hold `sun`.  One cast to fp32, at the store:
 * the fp32 rounding of ECEF that the camera rays reproduce (half a metre) is not made here.
 *   grid, center, sun  host pointers; center: 3 doubles holding the scene's fp32 values, as
 *                      spnerf_dsm_points takes them; sun: 3 floats, NULL with ray_stride 8
 *   rays               [n][ray_stride] fp32, ray_stride 8 or 11 */
int32_t spnerf_ortho_rays(const spnerf_ortho_grid* grid, int32_t row0, int32_t n_rows, double min_alt, double max_alt,
                          const double* center, double range, const float* sun, float* rays, int32_t ray_stride,
                          void* stream);

/* Box filter of the s² contiguous sub-rays of every cell, one thread per output value:
 *   out[m][c][w] = (in[m][c·s² + 0][w] + in[m][c·s² + 1][w] + …) / s²
 * summed in fp64 in ascending sub-ray order, one division, one cast to the planes' type.
 *   in   [n_images][cells·s²][width],  out  [n_images][cells][width]
 *   dtype 0: fp32 planes; 1: fp64 planes (the altitude)
 * With supersample 1 there is nothing to reduce: nothing is launched, `out` is not written and the
 * caller keeps its input planes. */
int32_t spnerf_ortho_reduce(const void* in, void* out, int64_t n_images, int64_t cells, int32_t width,
                            int32_t supersample, int32_t dtype, void* stream);

/* The class of every cell from its (already reduced) mean logits, by the rule of the sem_class
 * plane (spnerf_amd_view.h): the first index of the maximum, a NaN counting as the maximum.
 *   logits [cells][n_classes] fp32,  labels [cells] int32 */
int32_t spnerf_ortho_classes(const float* logits, int64_t cells, int32_t n_classes, int32_t* labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_ORTHO_H */
