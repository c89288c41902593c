/* Image-score exports of libspnerf_amd.so (gfx950): the structural similarity the reference's
 * validation step logs as val/ssim (modules/metrics.py ssim :210-215 -> kornia.losses.ssim of
 * kornia 0.5.3 with window_size 3; eval.py:120-125), evaluated in fp64 on fp32 images.
 * A separate header from spnerf_amd.h, spnerf_amd_eval.h and spnerf_amd_view.h so that those ABIs
 * stay as they are; the conventions are the same: every function returns SPNERF_OK or a negative
 * SPNERF_E_* code with the text in spnerf_last_error, pointers are device pointers unless noted,
 * `stream` is a hipStream_t, and no call synchronises with the host, allocates, or uses atomics on
 * global memory — results are bit-reproducible from run to run.
 *
 * The definition, for images x, y of C channels of H x W values, an odd window size ws and
 * r = ws / 2:
 *   g[i]  = exp(-(i - r)^2 / (2 * 1.5^2)) normalised to sum 1; the window is outer(g, g)
 *   f(.)  = the correlation with that window per channel, the border mirrored without repeating
 *           the edge value (torch's 'reflect' padding of r)
 *   mu1 = f(x), mu2 = f(y), s1 = f(x x) - mu1^2, s2 = f(y y) - mu2^2, s12 = f(x y) - mu1 mu2
 *   C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2
 *   map = ((2 mu1 mu2 + C1) (2 s12 + C2)) / ((mu1^2 + mu2^2 + C1) (s1 + s2 + C2) + 1e-12)
 * and the score is the mean of the map over its C * H * W values.
 */
#ifndef SPNERF_AMD_IMAGE_H
#define SPNERF_AMD_IMAGE_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_IMAGE_ABI_VERSION 1
#define SPNERF_IMAGE_MAX_CHANNELS 4
#define SPNERF_IMAGE_MAX_WINDOW 11 /* ws is odd and in [3, 11] */

/* What spnerf_image_ssim leaves on the device. */
typedef struct spnerf_image_ssim_result {
    double ssim;                                    /* mean of the map over C * H * W values      */
    double channel_mean[SPNERF_IMAGE_MAX_CHANNELS]; /* mean over each channel's H * W; 0 past C   */
    int64_t n;                                      /* C * H * W                                  */
} spnerf_image_ssim_result;

int32_t spnerf_image_abi_version(void);

/* Bytes of workspace spnerf_image_ssim needs for that image, or a negative code. */
int64_t spnerf_image_ssim_workspace_bytes(int32_t C, int32_t H, int32_t W, int32_t ws);

/* SSIM of two fp32 images that share one layout: value (c, i, j) of either image is at element
 * c * channel_stride + i * row_stride + j * pixel_stride of its pointer, so planar CHW is
 * (H * W, W, 1), interleaved HWC is (1, W * C, C), and rows may be padded.  Strides are in
 * elements and not negative.  One workgroup per output tile per channel evaluates the map in fp64
 * and stores the tile's sum; one workgroup then sums the tiles in a fixed order.
 *   C             in [1, SPNERF_IMAGE_MAX_CHANNELS]
 *   H, W          both greater than ws / 2 (a mirrored border needs that many interior values)
 *   ws            3, 5, 7, 9 or 11
 *   max_val       the dynamic range of the images (1 for images in [0, 1])
 *   workspace     at least ..._workspace_bytes(C, H, W, ws) bytes, 16-byte aligned
 *   map           NULL, or [C][H][W] fp64: the map itself
 *   result        one spnerf_image_ssim_result, 8-byte aligned
 * A NaN anywhere in either image makes the score NaN. */
int32_t spnerf_image_ssim(const float* x, const float* y, int32_t C, int32_t H, int32_t W, int64_t channel_stride,
                          int64_t row_stride, int64_t pixel_stride, int32_t ws, double max_val, void* workspace,
                          double* map, spnerf_image_ssim_result* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_IMAGE_H */
