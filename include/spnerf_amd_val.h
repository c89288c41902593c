/* Validation-loss exports of libspnerf_amd.so (gfx950): the solar-correction march of a rendered
 * view reduced to two numbers per ray (the reference's solar_correction, modules/metrics.py:17-24,
 * on the solar pass of rendering.py:171-177), and the loss its validation step logs
 * (SNerfLoss / SatNerfLoss, modules/metrics.py:27-65) in one pass over the view's image planes.
 * A separate header so that the ABIs of spnerf_amd.h, spnerf_amd_view.h and their siblings stay as
 * they are; the conventions are the same: every function returns SPNERF_OK or a negative
 * SPNERF_E_* code with the text in spnerf_last_error, pointers are device pointers, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics on global
 * memory — results are bit-reproducible from run to run.
 */
#ifndef SPNERF_AMD_VAL_H
#define SPNERF_AMD_VAL_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_VAL_ABI_VERSION 1

/* What spnerf_val_loss leaves on the device.  A term whose planes were not given is 0 and is not
 * part of `loss`. */
typedef struct spnerf_val_loss_result {
    double n;            /* the number of rays                                                      */
    double color;        /* mean (rgb - t)^2 over the 3N values; with beta: mean (rgb - t)^2 / (2 b^2),
                            b = beta + beta_min (uncertainty_aware_loss, metrics.py:10-14)          */
    double color_coarse; /* mean (rgb_coarse - t)^2 over the 3N values                              */
    double logbeta;      /* (3 + mean log b) / 2                                                    */
    double sc_term2;     /* lambda_sc / 3 * mean term2                                              */
    double sc_term3;     /* lambda_sc / 3 * mean term3                                              */
    double loss;         /* the sum of the terms present                                            */
} spnerf_val_loss_result;

int32_t spnerf_val_abi_version(void);

/* The sibling of spnerf_view_composite_products for the solar pass: marches rays [0, n_rays) of one
 * chunk over the rows of the sun-only forward exactly as spnerf_composite_forward does (alpha,
 * transparency T and weights w are bit for bit its `transparency` / `weights` on the same out, z
 * and noise; sigma is column 3 of a row) and writes, per ray,
 *   term2[ray_begin + r] = sum_s (T_s - sun_s)^2        term3[ray_begin + r] = 1 - sum_s w_s * sun_s
 * as fp32 sums of rounded products: a lane's samples in index order, then across the wavefront.
 * Nothing per sample is stored.  `noise` / `noise_std` / `rng` mean what they mean for
 * spnerf_composite_forward, draw for draw.
 *   z        [n_rays][n_samples]               n_samples in [1, 256]
 *   out      [n_rays * n_samples][out_stride]  out_stride >= 4, n_samples * out_stride * 4 <= 32 KiB
 *   sun_col  column of out holding the sun visibility, in [0, out_stride) */
int32_t spnerf_val_solar_terms(int64_t n_rays, int32_t n_samples, const float* z, const float* out, int32_t out_stride,
                               int32_t sun_col, const float* noise, float noise_std, int64_t ray_begin, float* term2,
                               float* term3, const spnerf_rng* rng, void* stream);

/* Bytes of workspace spnerf_val_loss needs for that view, or a negative code. */
int64_t spnerf_val_loss_workspace_bytes(int64_t n_rays);

/* One pass over the planes of a rendered view, then a single-workgroup finish: fp64 sums, the
 * per-workgroup partials summed in workgroup order.
 *   rgb, target_rgb  [n_rays][3] fp32
 *   rgb_coarse       NULL, or [n_rays][3]: the coarse model's image beside a fine model's rgb
 *   beta             NULL, or [n_rays]: sum w * beta (the view's "beta" plane); not with rgb_coarse
 *   term2, term3     both NULL, or [n_rays] each (spnerf_val_solar_terms)
 *   workspace        at least ..._workspace_bytes(n_rays) bytes, 16-byte aligned
 *   result           one spnerf_val_loss_result */
int32_t spnerf_val_loss(int64_t n_rays, const float* rgb, const float* target_rgb, const float* rgb_coarse,
                        const float* beta, const float* term2, const float* term3, double lambda_sc, double beta_min,
                        void* workspace, spnerf_val_loss_result* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_VAL_H */
