/* Whole-view exports of libspnerf_amd.so (gfx950): the image products of a rendered view
 * (the reference's save_nerf_output_to_images, eval.py:27-101) composited straight into
 * caller-owned image planes, and the scores its validation step logs (modules/metrics.py:
 * psnr :206, miou :218, overall_accuracy :239) in one pass over a rendered view.
 * A separate header from spnerf_amd.h and spnerf_amd_eval.h so that those ABIs stay as they are;
 * the conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code
 * with the text in spnerf_last_error, pointers are device pointers unless noted, `stream` is a
 * hipStream_t, and no call synchronises with the host, allocates, or uses atomics on global
 * memory — results are bit-reproducible from run to run.
 */
#ifndef SPNERF_AMD_VIEW_H
#define SPNERF_AMD_VIEW_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_VIEW_ABI_VERSION 1
#define SPNERF_VIEW_MAX_CLASSES 32 /* n_classes of the metrics; n_sem of the products' argmax is
                                      bounded by the row width only */

/* The image planes of a view (a HOST struct of device pointers), each row-major over the view's
 * N rays.  Any pointer may be NULL: that plane is skipped. */
typedef struct spnerf_view_planes {
    float* rgb;         /* [N][3]      clamp(sum w * albedo * (sun + (1 - sun) * sky), 0, 1)      */
    float* depth;       /* [N]         sum w * z                                                   */
    float* sun;         /* [N]         sum w * sun          (eval.py:76)                           */
    float* albedo;      /* [N][3]      sum w * albedo       (eval.py:80)                           */
    float* sky;         /* [N][3]      sum w * sky          (eval.py:99)                           */
    float* beta;        /* [N]         sum w * beta         (eval.py:94; needs beta_col >= 0)      */
    float* sem_logits;  /* [N][n_sem]  the unweighted mean over the samples, as the composite's    */
    int32_t* sem_class; /* [N]         first index of that mean's maximum; a NaN is the maximum    */
} spnerf_view_planes;

/* What spnerf_view_metrics leaves on the device.  `table` is the row-major
 * (n_classes + 1) x n_classes confusion table [ground-truth label][predicted class]; labels
 * outside [0, n_classes) (the loss's ignore index -100 among them) are counted in the last row,
 * predictions outside [0, n_classes) in no cell.  Only its first (n_classes + 1) * n_classes
 * entries are written.  `correct` is the table's trace, `n` the number of rays. */
typedef struct spnerf_view_metrics_result {
    double mse, psnr; /* mean of (rgb - target)^2 over the 3N values; -10 * log10(mse)            */
    int64_t n, correct;
    int64_t table[(SPNERF_VIEW_MAX_CLASSES + 1) * SPNERF_VIEW_MAX_CLASSES];
} spnerf_view_metrics_result;

int32_t spnerf_view_abi_version(void);

/* The inference-only sibling of spnerf_composite_forward: composites rays [0, n_rays) of one
 * chunk and writes per-ray values only, ray r of the chunk to entry ray_begin + r of each plane.
 * rgb and depth are bit-identical to spnerf_composite_forward's on the same out, z and noise
 * (`noise` / `noise_std` / `rng` mean what they mean there, draw for draw); no weights or
 * transparency are stored.  The four weighted planes are fp32 sums, a lane's samples in index
 * order, then across the wavefront.
 *   z        [n_rays][n_samples]            n_samples in [1, 256]
 *   out      [n_rays * n_samples][n_out]    n_out >= 8, n_samples * n_out * 4 <= 32 KiB
 *   sem_col, n_sem   columns [sem_col, sem_col + n_sem) of out are the semantic logits
 *   beta_col         column of out holding beta, or -1
 *   planes           HOST pointer */
int32_t spnerf_view_composite_products(int64_t n_rays, int32_t n_samples, const float* z, const float* out,
                                       int32_t n_out, const float* noise, float noise_std, int32_t sem_col,
                                       int32_t n_sem, int32_t beta_col, int64_t ray_begin,
                                       const spnerf_view_planes* planes, const spnerf_rng* rng, void* stream);

/* Bytes of workspace spnerf_view_metrics needs for that view, or a negative code. */
int64_t spnerf_view_metrics_workspace_bytes(int64_t n_rays, int32_t n_classes);

/* One pass over a rendered view and its targets, then a single-workgroup finish: the squared
 * error summed in fp64 and the confusion table, per-workgroup partials summed in workgroup order.
 *   rgb, target_rgb  [n_rays][3] fp32
 *   sem_class        NULL, or [n_rays] int32 (the products' sem_class plane)
 *   labels           NULL, or [n_rays] int64
 *   n_classes        in [0, SPNERF_VIEW_MAX_CLASSES]; the table is counted when it is > 0 and
 *                    sem_class and labels are given, and not written otherwise
 *   workspace        at least ..._workspace_bytes(n_rays, n_classes) bytes, 16-byte aligned
 *   result           one spnerf_view_metrics_result */
int32_t spnerf_view_metrics(int64_t n_rays, const float* rgb, const float* target_rgb, const int32_t* sem_class,
                            const int64_t* labels, int32_t n_classes, void* workspace,
                            spnerf_view_metrics_result* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_VIEW_H */
