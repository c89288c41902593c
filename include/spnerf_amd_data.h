/* Training-set exports of libspnerf_amd.so (gfx950): the per-keypoint and per-pixel arithmetic of
 * the reference's dataset construction (datasets/satellite_scene.py load_depth_data :223-297,
 * init_scaling_params :391-413, load_semantic_data :299-389), which produces the tensors that
 * render_rays (valid_depth, target_depths, target_std), the fused training loss and the batch
 * gather consume.  Reading the files stays with the caller.
 * A separate header from spnerf_amd.h and the eval / view / image / loss headers so that those ABIs
 * stay as they are; the conventions are the same: every function returns SPNERF_OK or a negative
 * SPNERF_E_* code with the text in spnerf_last_error, pointers are device pointers unless noted,
 * `stream` is a hipStream_t, and no call synchronises with the host or allocates.  The only
 * atomics are integer min / max on the fold buffers, so results are bit-reproducible.
 *
 * `rpc` is the HOST array of 90 doubles of spnerf_rpc_rays (spnerf_amd.h), and rays are localised
 * exactly as there: fp64 localisation at max / min altitude, WGS-84 ECEF, origin rounded to fp32.
 */
#ifndef SPNERF_AMD_DATA_H
#define SPNERF_AMD_DATA_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_DATA_ABI_VERSION 1
#define SPNERF_DATA_WORKSPACE_BYTES 4096 /* spnerf_depth_priors: the partial correl minima / maxima */
#define SPNERF_DATA_VOID_LABEL (-100)    /* the label of an unmapped or unsupervised pixel         */

int32_t spnerf_data_abi_version(void);

/* spnerf_rpc_rays with the pixel list as (n_pixels, 2) [col, row] DOUBLES: rays at fractional
 * pixels (the reference localises depth keypoints at pts2d / img_downscale).  Every other argument
 * as in spnerf_rpc_rays; an integer-valued pixel gives the bits the int32 list gives. */
int32_t spnerf_rpc_rays_f64(const double* rpc, double downscale, double min_alt, double max_alt,
                            const double* pixels, int64_t n_pixels, const float* center, float range,
                            const float* sun, float* rays, int32_t ray_stride, void* stream);

/* Depth priors of one image (load_depth_data :241-279 at img_downscale 1).  Per keypoint k, in the
 * reference's fp32 arithmetic:
 *   ray    = the normalised ray of pixel pixels[k] (origin (fp32(ECEF) - center) / range)
 *   p      = (pts3d[k] - center) / range
 *   depth  = |p - o|_2, accumulated as fma(z, z, fma(y, y, x * x)) like torch's CPU vector norm
 *   w      = (correl[k] - min correl) / (max correl - min correl)   (min, max over this image)
 *   std    = stdscale * (1 - w) + margin                            (multiply, then add: not fused)
 * scattered to row r = row * width + col of the planes, which the call first sets to zero:
 *   deprays [HW][8], depths [HW][2] = [depth, w], valid_depth [HW] = 1, depth_std [HW] = std.
 * depth_range is two floats (min, max) that the call folds the image's depths into; start it at
 * (+inf, -inf), pass it to every image, and scale depth_std by (max - min) after the last (:295).
 *   pixels      (K, 2) [col, row] doubles, integer-valued, inside the image and DISTINCT (two
 *               keypoints on one pixel would race; the reference needs them strictly increasing in
 *               row * width + col, which the caller checks on the host)
 *   K           >= 1
 *   workspace   SPNERF_DATA_WORKSPACE_BYTES bytes, 8-byte aligned
 * Constant correl gives w = std = NaN at every keypoint (0 / 0), as in the reference. */
int32_t spnerf_depth_priors(const double* rpc, double min_alt, double max_alt, int32_t height, int32_t width,
                            const float* center, float range, const double* pixels, const float* pts3d,
                            const float* correl, int64_t K, float stdscale, float margin, float* deprays,
                            float* depths, float* valid_depth, float* depth_std, float* depth_range,
                            void* workspace, void* stream);

/* Scene bounds of one image (init_scaling_params :397-406): for every pixel of [0, n_rows) x
 * [0, n_cols) of the camera rescaled by 1 / downscale, the un-normalised ray is generated without
 * being stored, near = o and far_pt = o + far * d are formed in fp32 (multiply, then add), and the
 * per-axis minimum and maximum over both point sets are folded into
 *   bounds   6 floats [min x, min y, min z, max x, max y, max z]; start at (+inf x3, -inf x3) and
 *            pass the same buffer for every image of the scene. */
int32_t spnerf_scene_bounds(const double* rpc, double downscale, double min_alt, double max_alt, int32_t n_rows,
                            int32_t n_cols, float* bounds, void* stream);

/* Semantic supervision of one image (load_semantic_data :316-375).
 *   raster        [Hs][Ws] class codes as read from the CLS raster, uint8 (raster_is_i32 = 0) or
 *                 int32 (1); a code outside [0, 256) maps to SPNERF_DATA_VOID_LABEL
 *   lut           256 int32: code -> label, SPNERF_DATA_VOID_LABEL where unmapped
 *   sem_downscale >= 1
 *   dense         0: nearest resize to (height, width); valid = 1 where row % sem_downscale == 0,
 *                    col % sem_downscale == 0 and the label is not void; labels elsewhere are void
 *                 1: nearest resize to (Hs / sem_downscale, Ws / sem_downscale) (both >= 1), then to
 *                    (height, width); valid = label is not void
 *   labels        [height * width] int64,  valid [height * width] float 0 / 1
 * "Nearest" is F.interpolate(mode='nearest'): source = min(floor(dst * (float)in / (float)out), in - 1)
 * with the product in fp32. */
int32_t spnerf_semantic_labels(const void* raster, int32_t raster_is_i32, int32_t Hs, int32_t Ws, const int32_t* lut,
                               int32_t height, int32_t width, int32_t sem_downscale, int32_t dense, int64_t* labels,
                               float* valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_DATA_H */
