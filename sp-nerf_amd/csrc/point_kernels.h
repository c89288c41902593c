// The per-ray and per-point kernels of the MLP passes (point_kernels.hip): argument structs and one
// host launch function per kernel.  Each launch function opens the kernel's profiling class.
#pragma once
#include "common.h"
#include "mlp_layout.h"

namespace spn {

struct RayFwdArgs {
    const float* rays; int rs;
    const int64_t* labels; const float* temb;
    const float* packed; PackedOffs k; Dims d;
    float *rb0, *rb4, *rbQ, *skyh, *sky;
    int sem_on, need_q, need_sky;
};

template <typename T>
struct HeadsArgs {
    const float* packed; Dims d;
    const T *HL, *G, *Q, *S3;
    const float* sky;
    float* out; float* hsave;
    int64_t P; int S; int mode;  // mode: 0 full, 1 sigma only, 2 sigma + sun
};

template <typename T>
struct HeadsBwdArgs {
    const float* packed; Dims d;
    const float *d_out, *hsave;
    const T *DQ, *DG, *DS3;
    float* hpre;
    T *dZQ, *dZG, *dS3;
    int64_t P; int mode;
    int emu = 0;  // precision study (fp32 only): the dX outputs rounded to bf16
};

struct RayBwdArgs {
    const float* packed; PackedOffs k; Dims d;
    const float *sky, *skyh, *R0, *R4, *RQ;
    const float* d_out; int NO, S;   // the points' output gradients (sky columns 5..7)
    const int64_t* labels;
    float *skyd, *skydh, *gemb, *embr, *grad_t;
    int sem_on, beta_on, sky_on;
};

#pragma GCC visibility push(hidden)  // launch functions: internal to the library
// class "ray_terms": k_ray_fwd, k_ray_bwd (one block per ray), k_class_sum
int32_t ray_fwd(const RayFwdArgs& a, int64_t n_rays, hipStream_t s);
int32_t ray_bwd(const RayBwdArgs& a, int64_t n_rays, hipStream_t s);
int32_t class_sum(int64_t B, const float* gemb, int sd, const int64_t* labels, int C, float* out, int accumulate,
                  hipStream_t s);
// class "encode": k_encode over P points; each of X0 / X0b / X0s is written when non-null
int32_t encode(const float* rays, int rs, int dir_off, const float* z, int S, int ldz, int64_t P, int K0, int K0p,
               float* X0, bf16* X0b, bf16* X0s, hipStream_t s);
// class "heads_fwd": the wave-per-point narrow heads (k_heads_fwd_v by W, or k_heads_fwd: option
// heads_variant 0); sig_done: the σ pre-activation is in hsave already (W = 512)
int32_t heads_fwd(const HeadsArgs<float>& a, const PackedOffs& k, bool sig_done, hipStream_t s);
int32_t heads_fwd(const HeadsArgs<bf16>& a, const PackedOffs& k, bool sig_done, hipStream_t s);
// class "heads_bwd": k_heads_bwd_v by H, or k_heads_bwd
int32_t heads_bwd(const HeadsBwdArgs<float>& a, const PackedOffs& k, hipStream_t s);
int32_t heads_bwd(const HeadsBwdArgs<bf16>& a, const PackedOffs& k, hipStream_t s);
// class "ray_rowsum": per-ray sums of a point-major buffer (see k_ray_rowsum) ...
int32_t ray_rowsum(const float* in, int ld, int c0, int N, int S, int64_t n_rays, float* out, int ldo, hipStream_t s);
int32_t ray_rowsum(const bf16* in, int ld, int c0, int N, int S, int64_t n_rays, float* out, int ldo, hipStream_t s);
// ... and of a 512-wide bf16 dZ by 64-point tiles (S % 64 == 0): the tiles' column sums of dZ into
// part (dZ = nullptr: the fused dX chain wrote them), then each ray's tiles added in tile order;
// the pair adds two part / out pairs in one launch
int32_t ray_tiles_sum(const bf16* dZ, float* part, int64_t P, int S, int64_t n_rays, float* out, hipStream_t s);
int32_t ray_tiles_sum_pair(const float* part0, float* out0, const float* part1, float* out1, int64_t P, int S,
                           int64_t n_rays, hipStream_t s);
// class "zero"
int32_t zero_fill(float* p, int64_t n, hipStream_t s);
#pragma GCC visibility pop

}  // namespace spn
