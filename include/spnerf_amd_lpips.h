/* Perceptual-distance exports of libspnerf_amd.so (gfx950): the LPIPS score the reference's offline
 * evaluation prints per view (eval.py:20,128-135,399: lpips.LPIPS(net='alex') of the `lpips` package
 * 0.1, spatial=False, one image pair), in fp32 with fp64 final sums.
 * A separate header from spnerf_amd_image.h and the others so that those ABIs stay as they are; the
 * conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code with the
 * text in spnerf_last_error, pointers are device pointers unless noted, `stream` is a hipStream_t,
 * and no call synchronises with the host, allocates, or uses atomics on global memory — results are
 * bit-reproducible from run to run.
 *
 * The definition, for two images x, y of 3 channels of H x W values in [-1, 1]:
 *   scaling   v <- (v - shift[c]) / scale[c], shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
 *   features  five taps of AlexNet, each after its ReLU (zero padding, floor output sizes, biases):
 *               conv1 3->64 k11 s4 p2 | pool 3/2, conv2 64->192 k5 p2 | pool 3/2, conv3 192->384 k3 p1
 *               | conv4 384->256 k3 p1 | conv5 256->256 k3 p1
 *   distance  n(f) = f / (sqrt(sum_c f^2) + 1e-10) at every position of a tap;
 *             d_l = mean over positions of sum_c lin_l[c] (n(f_x) - n(f_y))^2
 *   score     sum_l d_l
 * The weights are data the caller brings (the `lpips` package's state_dict); the library holds none.
 *
 * How it runs: each convolution is an im2col gather into the workspace followed by the library's
 * fp32 MFMA GEMM, both images in one launch (rows of image x, then rows of image y), activations
 * NHWC.  A ReLU is applied by whoever reads an activation.  When the workspace is smaller than the
 * largest gather, the rows of a convolution are processed in bands; every output value is the same
 * dot product in the same order whatever the band, so the result has the same bits.
 */
#ifndef SPNERF_AMD_LPIPS_H
#define SPNERF_AMD_LPIPS_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_LPIPS_ABI_VERSION 1
#define SPNERF_LPIPS_TAPS 5
#define SPNERF_LPIPS_MIN_SIDE 31   /* taps of 7, 3, 1, 1, 1 on a side; at 30 the second pool has no window */
#define SPNERF_LPIPS_MAX_SIDE 8192

/* What spnerf_lpips leaves on the device (88 bytes). */
typedef struct spnerf_lpips_result {
    double lpips;                     /* sum of layer[]                                   */
    double layer[SPNERF_LPIPS_TAPS];  /* d_l of each tap                                   */
    int32_t h[SPNERF_LPIPS_TAPS];     /* rows of each tap                                  */
    int32_t w[SPNERF_LPIPS_TAPS];     /* columns of each tap                               */
} spnerf_lpips_result;

int32_t spnerf_lpips_abi_version(void);

/* Floats of one packed weight buffer: per tap l the convolution weights [C_out][Kp] with
 * k = (ky * kw + kx) * C_in + c and Kp = C_in * k * k rounded up to 32 (zero filled: the GEMM's
 * K-step), then the C_out biases, then the C_out lin weights. */
int64_t spnerf_lpips_weights_floats(void);

/* Packs the weights into `packed` (spnerf_lpips_weights_floats() floats, 16-byte aligned).  The
 * three arguments are HOST arrays of 5 DEVICE pointers: conv_w[l] the convolution weights of tap l
 * as torch holds them (OIHW, contiguous fp32), conv_b[l] its C_out biases, lin[l] its C_out lin
 * weights. */
int32_t spnerf_lpips_pack_weights(const float* const* conv_w, const float* const* conv_b, const float* const* lin,
                                  float* packed, void* stream);

/* Bytes of workspace for an H x W pair, or a negative code.  max_bytes <= 0: the size at which no
 * convolution is split.  Otherwise the largest useful size not above max_bytes, or — when max_bytes
 * is below the minimum (all activations, the partial sums and a gather band of 32 rows) — that
 * minimum.  spnerf_lpips takes any size from the minimum up and bands accordingly. */
int64_t spnerf_lpips_workspace_bytes(int32_t H, int32_t W, int64_t max_bytes);

/* HOST output: bands[l] = the number of row bands convolution l runs in with that workspace. */
int32_t spnerf_lpips_bands(int32_t H, int32_t W, int64_t workspace_bytes, int32_t* bands);

/* Floats of features_out for an H x W pair, or a negative code. */
int64_t spnerf_lpips_features_floats(int32_t H, int32_t W);

/* LPIPS of two fp32 images that share one layout: value (c, i, j) of either image is at element
 * c * channel_stride + i * row_stride + j * pixel_stride of its pointer, as in spnerf_image_ssim
 * (planar CHW is (H * W, W, 1), interleaved HWC is (1, W * 3, 3), rows may be padded).
 *   H, W            both in [SPNERF_LPIPS_MIN_SIDE, SPNERF_LPIPS_MAX_SIDE]
 *   normalize       not 0: the images are in [0, 1] and are mapped with 2 v - 1 first (eval.py:131-132)
 *   packed_weights  what spnerf_lpips_pack_weights wrote
 *   workspace       workspace_bytes bytes, 16-byte aligned
 *   features_out    NULL, or spnerf_lpips_features_floats(H, W) floats: the ten post-ReLU feature
 *                   maps, tap after tap, each [2][h_l][w_l][C_l] (image x, then image y; channels
 *                   innermost)
 *   result          one spnerf_lpips_result, 8-byte aligned
 * A NaN anywhere in either image makes the score NaN.  Swapping x and y gives the same bits. */
int32_t spnerf_lpips(const float* x, const float* y, int32_t H, int32_t W, int64_t channel_stride, int64_t row_stride,
                     int64_t pixel_stride, int32_t normalize, const float* packed_weights, void* workspace,
                     int64_t workspace_bytes, float* features_out, spnerf_lpips_result* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_LPIPS_H */
