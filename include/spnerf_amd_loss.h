/* Training-loss exports of libspnerf_amd.so (gfx950): every loss form the reference trainer
 * combines (main.py:125-174 over modules/metrics.py) and all of their upstream gradients, for the
 * coarse pass and, when the render has one, the fine pass, in two launches forward and one
 * backward.  A separate header from spnerf_amd.h, spnerf_amd_eval.h, spnerf_amd_view.h and
 * spnerf_amd_image.h so that those ABIs stay as they are (spnerf_render_loss_* of spnerf_amd.h
 * remains the one-configuration entry it was); the conventions are the same: every function
 * returns SPNERF_OK or a negative SPNERF_E_* code with the text in spnerf_last_error, pointers are
 * device pointers unless noted, `stream` is a hipStream_t, and no call synchronises with the host,
 * allocates, or uses atomics on global memory — results are bit-reproducible from run to run and a
 * step can be captured in a HIP graph.
 *
 * The terms, for B rays, pass p with S_p samples per ray (B_ = (float)B):
 *   colour, plain   color  = Σ_rc (rgb - t)^2 / (3 B_)                               metrics.py:36,41
 *   colour, β       b_r    = Σ_s w_rs β_rs + 0.05   (β of the COARSE pass in either pass)   :10-14
 *                   color  = Σ_rc (rgb - t)^2 / (2 b_r^2) / (3 B_)
 *                   logbeta = (3 + Σ_r log b_r / B_) / 2
 *   solar           sc2 = λ_sc/3 · Σ_rs (T_sc - sun)^2 / B_,  sc3 = λ_sc/3 · Σ_r (1 - Σ_s w_sc sun) / B_
 *                   (T_sc, w_sc constants: only sun_sc takes a gradient)                     :17-24
 *   depth           σ_r = sqrt(Σ_s w_rs (z_rs - d_r)^2);  applied = valid_r > 0 and
 *                   (|d_r - t_r| > σt_r or σ_r > σt_r), no gradient through the selection     :78-80
 *     subset MSE    ds = λ_ds/3 · Σ_applied tw_r (d_r - t_r)^2 / B_                          :125-132
 *     subset GNLL   ds = λ_ds/3 · Σ_applied ½ (log σc + (d_r - t_r)^2 / σc) / B_, σc = max(σ_r, 1e-6)
 *                   with the clamp invisible to the gradient (torch.nn.GaussianNLLLoss handed the
 *                   standard deviation as its variance, :129-130); gradients to depth (direct and
 *                   through σ) and to weights, none to z_vals; a ray left out contributes exactly 0
 *     all rays      ds = λ_ds/3 · Σ_r tw_r (d_r - t_r)^2 / B_                                :141,156
 *   semantic        ss = λ_ss · Σ_{label ≠ -100} nll_r / (n_valid_global / world)            :162-183
 *                   a label outside [0, C) other than -100 makes ss, the loss and that ray's logit
 *                   gradients NaN; no valid label in the global batch makes ss NaN (torch's mean
 *                   over nothing) with zero logit gradients
 *   loss            the sum of the terms above over the passes; a depth or semantic term flagged
 *                   term-only is reported but neither added nor differentiated (ds_drop / ss_drop,
 *                   main.py:163,172)
 */
#ifndef SPNERF_AMD_LOSS_H
#define SPNERF_AMD_LOSS_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_LOSS_ABI_VERSION 1

/* spnerf_train_loss_opts.flags */
#define SPNERF_LOSS_BETA 1            /* β colour form (needs opts.beta and pass.weights)          */
#define SPNERF_LOSS_DEPTH_TERM_ONLY 2 /* depth term reported, not added, zero gradient             */
#define SPNERF_LOSS_SEM_TERM_ONLY 4   /* semantic term reported, not added, zero gradient          */

/* spnerf_train_loss_opts.depth_form */
#define SPNERF_LOSS_DEPTH_NONE 0
#define SPNERF_LOSS_DEPTH_SUBSET_MSE 1
#define SPNERF_LOSS_DEPTH_SUBSET_GNLL 2
#define SPNERF_LOSS_DEPTH_ALL 3

/* The result block: SPNERF_LOSS_RESULT_FLOATS floats.
 *   [0] loss   [1] the semantic denominator n_valid_global / world (read back by the backward)
 *   [2 + 8 p + k] term k of pass p (0 coarse, 1 fine); 0 where the term is not formed */
#define SPNERF_LOSS_RESULT_FLOATS 18
#define SPNERF_LOSS_PASS_BASE 2
#define SPNERF_LOSS_PASS_TERMS 8
#define SPNERF_LOSS_TERM_COLOR 0
#define SPNERF_LOSS_TERM_LOGBETA 1
#define SPNERF_LOSS_TERM_SC2 2
#define SPNERF_LOSS_TERM_SC3 3
#define SPNERF_LOSS_TERM_DS 4
#define SPNERF_LOSS_TERM_SS 5
#define SPNERF_LOSS_TERM_MSE 6  /* Σ_rc (rgb - t)^2 / (3 B_) whatever the colour form            */
#define SPNERF_LOSS_TERM_PSNR 7 /* -10 log10 of it (train/psnr, main.py:179-181)                  */

/* One pass of the render.  NULL where the configuration does not need the tensor; the d_* members
 * are read by spnerf_train_loss_backward alone. */
typedef struct spnerf_train_loss_pass {
    int32_t n_samples;            /* S_p >= 1                                                      */
    int32_t ld_sun;               /* sun_sc[(r S_p + s) ld_sun]: a column of the MLP output        */
    const float* rgb;             /* (B, 3)    required                                            */
    const float* weights;         /* (B, S_p)  β form, subset depth forms                          */
    const float* z_vals;          /* (B, S_p)  subset depth forms                                  */
    const float* depth;           /* (B)       any depth form                                      */
    const float* sun_sc;          /* strided   λ_sc > 0                                            */
    const float* transparency_sc; /* (B, S_p)  λ_sc > 0                                            */
    const float* weights_sc;      /* (B, S_p)  λ_sc > 0                                            */
    const float* sem_logits;      /* (B, C)    λ_ss > 0                                            */
    float* d_rgb;                 /* (B, 3)    required                                            */
    float* d_weights;             /* (B, S_p)  dense; β form, or GNLL added to the loss; else NULL */
    float* d_depth;               /* (B)       a depth form added to the loss; else NULL           */
    float* d_sun;                 /* (B, S_p)  dense; λ_sc > 0                                     */
    float* d_logits;              /* (B, C)    λ_ss > 0 and added to the loss; else NULL           */
} spnerf_train_loss_pass;

/* The shared targets and options. */
typedef struct spnerf_train_loss_opts {
    int64_t n_rays;               /* B >= 1                                                        */
    int32_t n_classes;            /* C in [1, 64] when λ_ss > 0                                    */
    int32_t flags;                /* SPNERF_LOSS_*                                                 */
    int32_t depth_form;           /* SPNERF_LOSS_DEPTH_*                                           */
    int32_t world;                /* data-parallel ranks (>= 1) sharing labels_global              */
    float lambda_sc, lambda_ds, lambda_ss; /* a term is formed when its λ > 0 (depth: and a form)  */
    int32_t ld_beta;              /* beta[(r S_0 + s) ld_beta]                                     */
    int32_t ld_td;                /* target_depth[r ld_td], target_weight[r ld_td]                 */
    int32_t reserved;
    const float* target;          /* (B, 3)                                                        */
    const float* beta;            /* strided; β form: S_1 must equal S_0                           */
    const float* target_depth;    /* strided   any depth form                                      */
    const float* target_weight;   /* strided   subset MSE and all-rays forms                       */
    const int64_t* valid;         /* (B)       subset forms (> 0 = the ray has a prior)            */
    const float* target_std;      /* (B)       subset forms                                        */
    const int64_t* labels;        /* (B)       λ_ss > 0                                            */
    const int64_t* labels_global; /* (n_global) λ_ss > 0, forward only                             */
    int64_t n_global;
    float* d_beta;                /* (B, S_0) dense; β form, backward only                         */
} spnerf_train_loss_opts;

int32_t spnerf_loss_abi_version(void);

/* Bytes of workspace spnerf_train_loss_forward needs for that batch, or a negative code. */
int64_t spnerf_train_loss_workspace_bytes(int64_t n_rays);

/* The loss and its terms into `result` (SPNERF_LOSS_RESULT_FLOATS floats).  `opts`, `coarse` and
 * `fine` are host pointers, read before the call returns; `fine` is NULL for a render without the
 * fine keys.  Two launches: a wavefront per ray leaves per-block partial sums
 * in the workspace, one block adds them in block order. */
int32_t spnerf_train_loss_forward(const spnerf_train_loss_opts* opts, const spnerf_train_loss_pass* coarse,
                                  const spnerf_train_loss_pass* fine, void* workspace, float* result, void* stream);

/* Every upstream gradient times *g_loss (a device scalar) into the d_* members, one launch.
 * `result` is the block the forward of the same arguments left. */
int32_t spnerf_train_loss_backward(const spnerf_train_loss_opts* opts, const spnerf_train_loss_pass* coarse,
                                   const spnerf_train_loss_pass* fine, const float* result, const float* g_loss,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_LOSS_H */
