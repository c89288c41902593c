// Relighting kernels (include/spnerf_amd_relight.h): a view under K sun directions from one pass
// over its geometry.
//
//  * k_relight_dirs — what depends on the direction alone, fp32, one workgroup per direction:
//    sky_color(d_k) and v_k = W0[:, feat:]·d_k + b0 of sun_v_net.0.
//  * k_relight_sun_bf16 — the bf16 model's launch.  A persistent grid over 128-point tiles, four
//    wavefronts of 32 points each; W0f = sun_v_net.0.weight[:, :feat], sun_v_net.2 and .4 stay in
//    LDS as bf16 (rows padded by 16 B).  Every product is computed transposed, Xᵀ = W · actᵀ with
//    mfma_f32_32x32x16_bf16: the result has its point on the lane and its neurons in the 16
//    registers, which is the B operand of the next layer's product with no LDS round trip — only
//    the k order inside a 16-step is permuted, and the weight fragment is read in that same order.
//    baseᵀ = W0f·Fᵀ is formed once per tile (F = xyz_features from the MLP workspace's G rows) and
//    kept in registers; per direction: sin(base + v_k), two MFMA layers with sin, the H→1 dot and
//    the sigmoid.  Activations are rounded to bf16 where the layer-by-layer heads round them.
//  * k_relight_sun_f32 — the fp32 model (the parity path): the same arithmetic in fp32 on the
//    vector units, 8 points per workgroup.
//  * k_relight_composite — one wavefront per ray: the march of composite.h once, then per
//    direction the sums Σ w·albedo·(s + (1 − s)·sky_k), Σ w·s and Σ w·sky_k through shade_colour;
//    fixed order, no atomics.
#include <algorithm>

#include "../../include/spnerf_amd_relight.h"
#include "composite.h"
#include "mlp_layout.h"

namespace spn {

typedef __bf16 rl_bf16x8 __attribute__((ext_vector_type(8)));

// the per-direction terms in the caller's workspace: [K][4] sky, then [K][H] v
__host__ __device__ inline size_t dir_sky_bytes(int K) { return (size_t)K * 4 * sizeof(float); }

struct RelightW {   // offsets (floats / bf16 elements) of the packed weights the launches read
    int64_t WQ, bQ, Wsun, Ws2, bs2, Ws3, bs3, ws4, bs4, Wk1, bk1, Wk2, bk2, WQ16, Ws2_16, Ws3_16;
};

static RelightW relight_w(const Packed& k) {
    return RelightW{k.WQ, k.bQ, k.Wsun, k.Ws2, k.bs2, k.Ws3, k.bs3, k.ws4, k.bs4, k.Wk1, k.bk1, k.Wk2, k.bk2,
                    k.WQ16, k.Ws2_16, k.Ws3_16};
}

__global__ __launch_bounds__(128) void k_relight_dirs(const float* __restrict__ P, RelightW k, int H,
                                                      const float* __restrict__ dirs, float* __restrict__ sky,
                                                      float* __restrict__ vec) {
    __shared__ float red[3][128];
    const int dk = blockIdx.x, tid = threadIdx.x;
    const float s0 = dirs[dk * 3], s1 = dirs[dk * 3 + 1], s2 = dirs[dk * 3 + 2];
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
    for (int n = tid; n < H; n += 128) {
        const float* ws = P + k.Wsun + n * 3;
        vec[dk * H + n] = P[k.bQ + n] + (ws[0] * s0 + ws[1] * s1 + ws[2] * s2);
        const float* w = P + k.Wk1 + n * 3;
        const float hv = fmaxf(P[k.bk1 + n] + (w[0] * s0 + w[1] * s1 + w[2] * s2), 0.f);
        acc0 += P[k.Wk2 + n] * hv;
        acc1 += P[k.Wk2 + H + n] * hv;
        acc2 += P[k.Wk2 + 2 * H + n] * hv;
    }
    red[0][tid] = acc0;
    red[1][tid] = acc1;
    red[2][tid] = acc2;
    __syncthreads();
    for (int st = 64; st > 0; st >>= 1) {
        if (tid < st)
            for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + st];
        __syncthreads();
    }
    if (tid < 3) sky[dk * 4 + tid] = sigmoidf_(red[tid][0] + P[k.bk2 + tid]);
    if (tid == 3) sky[dk * 4 + 3] = 0.f;
}

// ---- bf16: the MFMA launch ------------------------------------------------------------------------

// row of the 32 x 32 accumulator tile that register `reg` of lane half `h` holds
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// 16 neurons (registers 8·half .. 8·half + 7 of a 32-row block) of sin(acc + bias) as the next
// product's B fragment; element j is row 16·half + 8(j >> 2) + 4h + (j & 3) of the block
__device__ __forceinline__ rl_bf16x8 sin_frag(const f32x16& acc, int half, const float* bias_blk, int h) {
    float f[8];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(bias_blk + 16 * half + 8 * q + 4 * h);
#pragma unroll
        for (int i = 0; i < 4; ++i) f[4 * q + i] = fast_sin(acc[8 * half + 4 * q + i] + b[i]);
    }
    return __builtin_bit_cast(rl_bf16x8, pack8(f));
}

// the weight fragment matching sin_frag's k order: row `row` of a [.][ld] bf16 LDS image, columns
// 16s + 4h .. + 3 and 16s + 8 + 4h .. + 3
__device__ __forceinline__ rl_bf16x8 perm_frag(const bf16* w, int ld, int row, int s, int h) {
    const bf16* p = w + row * ld + 16 * s + 4 * h;
    const u32x2 lo = *reinterpret_cast<const u32x2*>(p), hi = *reinterpret_cast<const u32x2*>(p + 8);
    return __builtin_bit_cast(rl_bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
}

template <int MB>
struct RelightGeo {
    static constexpr int H = 32 * MB, W = 2 * H;
    static constexpr int LD0 = W + 8, LD2 = H + 8;          // bf16 row strides: 16 B of padding
    static constexpr int W0_OFF = 0, W2_OFF = H * LD0, W4_OFF = W2_OFF + H * LD2, W_END = W4_OFF + H * LD2;
    static constexpr int F_OFF = W_END * 2;                   // fp32 from here (bytes): b2, b4 and sun_v_net.6's row
    static constexpr int LDS = F_OFF + 3 * H * 4;
};

struct RelightSunArgs {
    const void* G;   // [P][ldG] activations (bf16 or fp32), xyz_features in columns [0, W)
    int ldG;
    int64_t P;
    const float* packed;
    RelightW k;
    const float* vec;   // [K][H]
    int K;
    float* sv;          // [P][K]
};

template <int MB>
__global__ __launch_bounds__(256) void k_relight_sun_bf16(RelightSunArgs a, int ntiles) {
    using Geo = RelightGeo<MB>;
    constexpr int H = Geo::H, W = Geo::W;
    __shared__ __attribute__((aligned(16))) char smem[Geo::LDS];
    bf16* wl = reinterpret_cast<bf16*>(smem);
    float* fl = reinterpret_cast<float*>(smem + Geo::F_OFF);   // b2 [H], b4 [H], w4 [H]
    const int tid = threadIdx.x;
    const bf16* P16 = reinterpret_cast<const bf16*>(a.packed);
    // the three matrices, 16 B at a time, into the padded rows
    for (int i = tid; i < H * (W / 8); i += 256) {
        const int r = i / (W / 8), c = i % (W / 8);
        *reinterpret_cast<u32x4*>(wl + Geo::W0_OFF + r * Geo::LD0 + 8 * c) = ldg16(P16 + a.k.WQ16 + (int64_t)r * W + 8 * c);
    }
    for (int i = tid; i < H * (H / 8); i += 256) {
        const int r = i / (H / 8), c = i % (H / 8);
        *reinterpret_cast<u32x4*>(wl + Geo::W2_OFF + r * Geo::LD2 + 8 * c) = ldg16(P16 + a.k.Ws2_16 + (int64_t)r * H + 8 * c);
        *reinterpret_cast<u32x4*>(wl + Geo::W4_OFF + r * Geo::LD2 + 8 * c) = ldg16(P16 + a.k.Ws3_16 + (int64_t)r * H + 8 * c);
    }
    for (int i = tid; i < H; i += 256) {
        fl[i] = a.packed[a.k.bs2 + i];
        fl[H + i] = a.packed[a.k.bs3 + i];
        fl[2 * H + i] = a.packed[a.k.ws4 + i];
    }
    __syncthreads();
    const float b6 = a.packed[a.k.bs4];
    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const bf16* G = reinterpret_cast<const bf16*>(a.G);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t p = (int64_t)tile * 128 + wave * 32 + r;
        const int64_t pc = p < a.P ? p : a.P - 1;   // clamped: unconditional loads, the store is guarded
        const bf16* frow = G + pc * a.ldG + 8 * h;
        // (lane indices the compiler cannot see through: the LDS-resident weights are the same for
        // every tile and direction, and their fragment reads must not be hoisted into registers)
        const int rt = opaque(r);
        // baseᵀ = W0f · Fᵀ, natural k order on both operands
        f32x16 base[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) base[m][e] = 0.f;
#pragma unroll 4
        for (int s = 0; s < W / 16; ++s) {
            const rl_bf16x8 fb = __builtin_bit_cast(rl_bf16x8, ldg16(frow + 16 * s));
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const rl_bf16x8 wa = __builtin_bit_cast(
                    rl_bf16x8, *reinterpret_cast<const u32x4*>(wl + Geo::W0_OFF + (32 * m + rt) * Geo::LD0 + 16 * s + 8 * h));
                base[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, fb, base[m], 0, 0, 0);
            }
        }
        for (int dk = 0; dk < a.K; ++dk) {
            const float* v = a.vec + (int64_t)dk * H;
            const int rd = opaque(r), hd = opaque(h);
            rl_bf16x8 x[2 * MB];
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                x[2 * m] = sin_frag(base[m], 0, v + 32 * m, h);
                x[2 * m + 1] = sin_frag(base[m], 1, v + 32 * m, h);
            }
#pragma unroll
            for (int layer = 0; layer < 2; ++layer) {
                const bf16* wm = wl + (layer == 0 ? Geo::W2_OFF : Geo::W4_OFF);
                f32x16 acc[MB];
#pragma unroll
                for (int m = 0; m < MB; ++m) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
#pragma unroll
                    for (int s = 0; s < 2 * MB; ++s)
                        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(perm_frag(wm, Geo::LD2, 32 * m + rd, s, hd), x[s], acc[m],
                                                                         0, 0, 0);
                }
                if (layer == 0) {
#pragma unroll
                    for (int m = 0; m < MB; ++m) {
                        x[2 * m] = sin_frag(acc[m], 0, fl + 32 * m, hd);
                        x[2 * m + 1] = sin_frag(acc[m], 1, fl + 32 * m, hd);
                    }
                } else {
                    // sun_v_net.6 on the bf16-rounded sin, as the heads read S3: this lane's 16·MB
                    // neurons, then the other lane half's
                    float t = 0.f;
#pragma unroll
                    for (int m = 0; m < MB; ++m)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int row = 32 * m + 8 * g + 4 * hd;
                            const f32x4 b = *reinterpret_cast<const f32x4*>(fl + H + row);
                            const f32x4 w = *reinterpret_cast<const f32x4*>(fl + 2 * H + row);
#pragma unroll
                            for (int i = 0; i < 4; ++i) t += (float)(bf16)fast_sin(acc[m][4 * g + i] + b[i]) * w[i];
                        }
                    t += __shfl_xor(t, 32, 64);
                    if (h == 0 && p < a.P) a.sv[p * a.K + dk] = sigmoidf_(t + b6);
                }
            }
        }
    }
}

// ---- fp32: the parity path ------------------------------------------------------------------------

constexpr int kRelightPT = 8;   // points per workgroup

__global__ __launch_bounds__(256) void k_relight_sun_f32(RelightSunArgs a, int W, int H) {
    __shared__ float x[kRelightPT * 256], base[kRelightPT * 128], ha[kRelightPT * 128], hb[kRelightPT * 128];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * kRelightPT;
    const float* G = reinterpret_cast<const float*>(a.G);
    const float* Pk = a.packed;
    for (int i = tid; i < kRelightPT * W; i += 256) {
        const int64_t p = p0 + i / W;
        x[i] = p < a.P ? G[p * a.ldG + i % W] : 0.f;
    }
    __syncthreads();
    const int nh = kRelightPT * H;
    for (int i = tid; i < nh; i += 256) {
        const int n = i % H, q = i / H;
        const float* w = Pk + a.k.WQ + (int64_t)n * W;
        float acc = 0.f;
        for (int c = 0; c < W; ++c) acc += x[q * W + c] * w[c];
        base[i] = acc;
    }
    __syncthreads();
    for (int dk = 0; dk < a.K; ++dk) {
        for (int i = tid; i < nh; i += 256) ha[i] = sinf(base[i] + a.vec[(int64_t)dk * H + i % H]);
        __syncthreads();
        for (int i = tid; i < nh; i += 256) {
            const int n = i % H, q = i / H;
            const float* w = Pk + a.k.Ws2 + (int64_t)n * H;
            float acc = 0.f;
            for (int c = 0; c < H; ++c) acc += ha[q * H + c] * w[c];
            hb[i] = sinf(acc + Pk[a.k.bs2 + n]);
        }
        __syncthreads();
        for (int i = tid; i < nh; i += 256) {
            const int n = i % H, q = i / H;
            const float* w = Pk + a.k.Ws3 + (int64_t)n * H;
            float acc = 0.f;
            for (int c = 0; c < H; ++c) acc += hb[q * H + c] * w[c];
            ha[i] = sinf(acc + Pk[a.k.bs3 + n]);
        }
        __syncthreads();
        // sun_v_net.6: a wavefront per point, two points per wavefront
        const int wave = tid >> 6, lane = tid & 63;
        for (int q = wave; q < kRelightPT; q += 4) {
            float t = 0.f;
            for (int c = lane; c < H; c += 64) t += ha[q * H + c] * Pk[a.k.ws4 + c];
            t = wave_sum(t);
            const int64_t p = p0 + q;
            if (lane == 0 && p < a.P) a.sv[p * a.K + dk] = sigmoidf_(t + Pk[a.k.bs4]);
        }
        __syncthreads();
    }
}

// ---- the K images of a chunk ----------------------------------------------------------------------

struct RelightCompArgs {
    CompArgs c;   // what march() reads
    int K;
    const float *sv, *sky;   // [P][K], [K][4]
    int64_t ray_begin, plane_rays;
    float *rgb, *sun, *skyp;
};

template <int EPL>
__global__ __launch_bounds__(256) void k_relight_composite(RelightCompArgs v) {
    extern __shared__ __attribute__((aligned(16))) float sh_rows[];
    const CompArgs& a = v.c;
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= a.B) return;  // wave-uniform; the LDS slices are wave-private (no block barrier)
    const int S = a.S, NO = a.NO, K = v.K;
    float* rows = sh_rows + (threadIdx.x >> 6) * (S * NO);
    stage_rows(a.out + ray * (int64_t)(S * NO), rows, S * NO, lane);
    RayState<EPL> st;
    march<EPL>(a, ray, lane, rows, st);
    const int64_t px = v.ray_begin + ray;
    for (int dk = 0; dk < K; ++dk) {
        const float k0 = v.sky[dk * 4], k1 = v.sky[dk * 4 + 1], k2 = v.sky[dk * 4 + 2];
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, su = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            const int e = lane * EPL + j;
            if (e >= S) continue;
            const float* o = rows + e * NO;
            const float w = st.w[j];
            const float s = v.sv[(ray * S + e) * K + dk];
            const float oo[8] = {o[0], o[1], o[2], 0.f, s, k0, k1, k2};
            shade_colour(w, oo, c0, c1, c2);
            su += w * s;
            s0 += w * k0;
            s1 += w * k1;
            s2 += w * k2;
        }
        c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
        su = wave_sum(su);
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) {
            const int64_t e = (int64_t)dk * v.plane_rays + px;
            if (v.rgb) {
                v.rgb[e * 3] = fminf(fmaxf(c0, 0.f), 1.f);
                v.rgb[e * 3 + 1] = fminf(fmaxf(c1, 0.f), 1.f);
                v.rgb[e * 3 + 2] = fminf(fmaxf(c2, 0.f), 1.f);
            }
            if (v.sun) v.sun[e] = su;
            if (v.skyp) {
                v.skyp[e * 3] = s0;
                v.skyp[e * 3 + 1] = s1;
                v.skyp[e * 3 + 2] = s2;
            }
        }
    }
}

template <int EPL>
static int32_t launch_relight_composite(const RelightCompArgs& v, hipStream_t s) {
    const size_t per_wave = (size_t)v.c.S * v.c.NO * sizeof(float);
    const int wpb = comp_waves_per_block(per_wave);
    const dim3 grid((unsigned)((v.c.B + wpb - 1) / wpb)), block(64 * wpb);
    hipLaunchKernelGGL(k_relight_composite<EPL>, grid, block, per_wave * wpb, s, v);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

static int32_t relight_dims(const spnerf_model_cfg* cfg, Dims* d) {
    SPN_ARG(cfg, "relight: NULL cfg");
    SPN_TRY(make_dims(cfg, d));
    if (d->W > 256 || d->W % 64 != 0) {
        set_error("relight: width %d is not one of 64, 128, 192, 256 (render each direction in full)", d->W);
        return SPNERF_E_UNSUPPORTED;
    }
    return SPNERF_OK;
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_relight_abi_version(void) { return SPNERF_RELIGHT_ABI_VERSION; }

extern "C" int64_t spnerf_relight_workspace_bytes(const spnerf_model_cfg* cfg, int32_t n_dirs) {
    Dims d;
    SPN_TRY(relight_dims(cfg, &d));
    SPN_ARG(n_dirs >= 1, "relight_workspace_bytes: n_dirs %d must be positive", n_dirs);
    return (int64_t)(dir_sky_bytes(n_dirs) + (size_t)n_dirs * d.H * sizeof(float));
}

extern "C" int32_t spnerf_relight_directions(const spnerf_model_cfg* cfg, const void* packed, const float* sun_dirs,
                                             int32_t n_dirs, void* workspace, void* stream) {
    Dims d;
    SPN_TRY(relight_dims(cfg, &d));
    SPN_ARG(packed && sun_dirs && workspace, "relight_directions: NULL packed, sun_dirs or workspace");
    SPN_ARG(n_dirs >= 1, "relight_directions: n_dirs %d must be positive", n_dirs);
    SPN_ARG(((uintptr_t)workspace & 15) == 0, "relight_directions: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* sky = (float*)workspace;
    float* vec = (float*)((char*)workspace + dir_sky_bytes(n_dirs));
    ProfScope prof("relight_dirs", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_relight_dirs, dim3(n_dirs), dim3(128), 0, s, (const float*)packed, relight_w(packed_layout(d)), d.H,
                       sun_dirs, sky, vec);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_relight_sun(const spnerf_model_cfg* cfg, const void* packed, const void* mlp_workspace,
                                      int64_t n_rays, int32_t n_samples, const void* dir_workspace, int32_t n_dirs,
                                      float* sun_v, void* stream) {
    Dims d;
    SPN_TRY(relight_dims(cfg, &d));
    SPN_ARG(packed && mlp_workspace && dir_workspace && sun_v, "relight_sun: NULL packed, workspace or sun_v");
    SPN_ARG(n_rays >= 0 && n_samples >= 1, "relight_sun: bad sizes (n_rays %lld, n_samples %d)", (long long)n_rays, n_samples);
    SPN_ARG(n_dirs >= 1, "relight_sun: n_dirs %d must be positive", n_dirs);
    SPN_ARG(((uintptr_t)dir_workspace & 15) == 0 && ((uintptr_t)mlp_workspace & 15) == 0, "relight_sun: workspace not 16-byte aligned");
    const int64_t P = n_rays * n_samples;
    if (P == 0) return SPNERF_OK;
    SPN_ARG(P < (1ll << 31) / std::max(d.NQ, d.NG), "relight_sun: too many points (%lld) for one call", (long long)P);
    const Packed k = packed_layout(d);
    const WS w = ws_layout(d, n_rays, n_samples, 0);
    RelightSunArgs a{};
    a.G = (const float*)mlp_workspace + w.G;
    a.ldG = d.NG;
    a.P = P;
    a.packed = (const float*)packed;
    a.k = relight_w(k);
    a.vec = (const float*)((const char*)dir_workspace + dir_sky_bytes(n_dirs));
    a.K = n_dirs;
    a.sv = sun_v;
    hipStream_t s = (hipStream_t)stream;
    const double flop = 2.0 * P * ((double)d.H * d.W + (double)n_dirs * (2.0 * d.H * d.H + d.H));
    const double bytes = (d.bf ? 2.0 : 4.0) * P * d.W + 4.0 * P * n_dirs;
    if (d.bf) {
        const int ntiles = (int)((P + 127) / 128);
        const dim3 grid(std::min(ntiles, num_cus())), block(256);
        ProfScope prof("relight_sun_bf16", s, flop, bytes);
        switch (d.H / 32) {
            case 1: hipLaunchKernelGGL(k_relight_sun_bf16<1>, grid, block, 0, s, a, ntiles); break;
            case 2: hipLaunchKernelGGL(k_relight_sun_bf16<2>, grid, block, 0, s, a, ntiles); break;
            case 3: hipLaunchKernelGGL(k_relight_sun_bf16<3>, grid, block, 0, s, a, ntiles); break;
            default: hipLaunchKernelGGL(k_relight_sun_bf16<4>, grid, block, 0, s, a, ntiles);
        }
    } else {
        ProfScope prof("relight_sun_f32", s, flop, bytes);
        hipLaunchKernelGGL(k_relight_sun_f32, dim3((unsigned)((P + kRelightPT - 1) / kRelightPT)), dim3(256), 0, s, a, d.W, d.H);
    }
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_relight_composite(int64_t n_rays, int32_t n_samples, const float* z, const float* out,
                                            int32_t n_out, const float* noise, float noise_std, const spnerf_rng* rng,
                                            int32_t n_dirs, const float* sun_v, const void* dir_workspace, int64_t ray_begin,
                                            int64_t plane_rays, float* rgb, float* sun, float* sky, void* stream) {
    SPN_ARG(z && out, "relight_composite: NULL z or out");
    SPN_ARG(sun_v && dir_workspace, "relight_composite: NULL sun_v or dir_workspace");
    SPN_ARG(n_rays >= 0, "relight_composite: n_rays %lld is negative", (long long)n_rays);
    SPN_ARG(n_samples >= 1 && n_samples <= 256, "relight_composite: n_samples %d must be in [1, 256]", n_samples);
    SPN_ARG(n_out >= 8, "relight_composite: n_out %d is below 8", n_out);
    SPN_ARG((size_t)2 * n_samples * n_out * sizeof(float) <= 64 * 1024, "relight_composite: n_samples x n_out = %d x %d too large",
            n_samples, n_out);
    SPN_ARG(n_dirs >= 1, "relight_composite: n_dirs %d must be positive", n_dirs);
    SPN_ARG(ray_begin >= 0 && plane_rays >= ray_begin + n_rays, "relight_composite: rays [%lld, %lld) outside a plane of %lld",
            (long long)ray_begin, (long long)(ray_begin + n_rays), (long long)plane_rays);
    if (n_rays == 0) return SPNERF_OK;
    RelightCompArgs v{};
    v.c.B = n_rays; v.c.S = n_samples; v.c.NO = n_out;
    v.c.z = z; v.c.out = out; v.c.noise = noise; v.c.noise_std = noise_std;
    if (!noise && rng && noise_std != 0.f) v.c.rng = *rng;
    v.K = n_dirs;
    v.sv = sun_v;
    v.sky = (const float*)dir_workspace;
    v.ray_begin = ray_begin;
    v.plane_rays = plane_rays;
    v.rgb = rgb; v.sun = sun; v.skyp = sky;
    hipStream_t s = (hipStream_t)stream;
    const double P = (double)n_rays * n_samples;
    ProfScope prof("relight_composite", s, 0.0,
                   P * (n_out * 4.0 + 4.0 + 4.0 * n_dirs) + 4.0 * n_rays * n_dirs * ((rgb ? 3 : 0) + (sun ? 1 : 0) + (sky ? 3 : 0)));
    if (n_samples <= 64) return launch_relight_composite<1>(v, s);
    if (n_samples <= 128) return launch_relight_composite<2>(v, s);
    return launch_relight_composite<4>(v, s);
}
