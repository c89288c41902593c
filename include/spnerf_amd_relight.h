/* Relighting exports of libspnerf_amd.so (gfx950): a view under K sun directions from one pass over
 * its geometry.  Of SPNeRF.forward (models/spnerf.py:332-356) only sun_v_net and sky_color read the
 * sun direction, and sun_v_net.0 splits into W0[:, :feat]·xyz_features + b0 (once per point) plus
 * W0[:, feat:]·d_k (one H-vector per direction).  The final-pass forward therefore runs once with
 * SPNERF_MLP_KEEP_FEAT (spnerf_amd.h), which leaves xyz_features in the MLP workspace; the entry
 * points below evaluate the rest of sun_v_net per direction and composite the K images.
 * A separate header so that the ABIs of spnerf_amd.h and its siblings stay as they are; the
 * conventions are the same: every function returns SPNERF_OK or a negative SPNERF_E_* code with
 * the text in spnerf_last_error, pointers are device pointers, `stream` is a hipStream_t, and no
 * call synchronises with the host, allocates, or uses atomics on global memory — results are
 * bit-reproducible from run to run.
 */
#ifndef SPNERF_AMD_RELIGHT_H
#define SPNERF_AMD_RELIGHT_H

#include "spnerf_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPNERF_RELIGHT_ABI_VERSION 1

int32_t spnerf_relight_abi_version(void);

/* Bytes of the per-direction terms of n_dirs directions (spnerf_relight_directions), or a negative
 * code: SPNERF_E_UNSUPPORTED for a model the relight launches do not run — a width above 256 or
 * not a multiple of 64 (H = width / 2 must be 32, 64, 96 or 128) — whose caller renders each
 * direction in full instead. */
int64_t spnerf_relight_workspace_bytes(const spnerf_model_cfg* cfg, int32_t n_dirs);

/* The terms that depend on the direction alone, in fp32, one workgroup per direction:
 *   sky_color(d_k) (3 inputs -> H -> 3, ReLU, sigmoid) and
 *   v_k = sun_v_net.0.weight[:, feat:] · d_k + sun_v_net.0.bias,
 * into `workspace` ([n_dirs][4] sky, then [n_dirs][H] v; 16-byte aligned).
 *   sun_dirs  [n_dirs][3] fp32 */
int32_t spnerf_relight_directions(const spnerf_model_cfg* cfg, const void* packed, const float* sun_dirs, int32_t n_dirs,
                                  void* workspace, void* stream);

/* The sun visibility of every point of one forward under every direction:
 *   sun_v[p][k] = sigmoid(w6 · sin(W4 · sin(W2 · sin(W0f · xyz_features_p + v_k) + b2) + b4) + b6)
 * `mlp_workspace` is the workspace of the MLP forward of those n_rays x n_samples points with
 * flags SPNERF_MLP_KEEP_FEAT alone, whose G buffer holds xyz_features.  The bf16 model runs one launch:
 * 128-point tiles, the three weight matrices resident in LDS as bf16, W0f·xyz_features formed once
 * per tile and kept in registers, then per direction two MFMA layers; the fp32 model (the parity
 * path) runs the same arithmetic in fp32 on the vector units.
 *   sun_v  [n_rays * n_samples][n_dirs] fp32 */
int32_t spnerf_relight_sun(const spnerf_model_cfg* cfg, const void* packed, const void* mlp_workspace, int64_t n_rays,
                           int32_t n_samples, const void* dir_workspace, int32_t n_dirs, float* sun_v, void* stream);

/* The K images of one chunk: marches rays [0, n_rays) exactly as spnerf_composite_forward does
 * (sigma and the albedo are columns 3 and 0..2 of a row of `out`; `noise` / `noise_std` / `rng` mean
 * what they mean there, draw for draw) and writes, per direction k and ray r, at entry
 * k * plane_rays + ray_begin + r of each plane that is not NULL:
 *   rgb  [n_dirs][plane_rays][3]  sum w·albedo·(s + (1 - s)·sky_k), clamped to [0, 1]
 *   sun  [n_dirs][plane_rays]     sum w·s
 *   sky  [n_dirs][plane_rays][3]  sum w·sky_k
 * with s = sun_v[p][k].  One wavefront per ray, a lane's samples in index order, then across the
 * wavefront: a plane does not depend on n_dirs, on k's position or on the chunking.
 *   n_samples in [1, 256], 2 * n_samples * n_out * 4 <= 64 KiB */
int32_t spnerf_relight_composite(int64_t n_rays, int32_t n_samples, const float* z, const float* out, int32_t n_out,
                                 const float* noise, float noise_std, const spnerf_rng* rng, int32_t n_dirs,
                                 const float* sun_v, const void* dir_workspace, int64_t ray_begin, int64_t plane_rays,
                                 float* rgb, float* sun, float* sky, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPNERF_AMD_RELIGHT_H */
