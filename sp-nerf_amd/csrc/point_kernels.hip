// The small per-ray and per-point kernels around the MLP's GEMMs (positional encoding, per-ray
// terms, the wave-per-point narrow heads and their backward, per-ray row sums, zeroing) and their
// launch functions (point_kernels.h).
#include <algorithm>
#include <type_traits>

#include "point_kernels.h"
#include "mlp_options.h"
#include "trunk.h"
#include "wave.h"

namespace spn {

// X0[p][c]: positional encoding of xyz = o + dir*z (rendering.py:147; spnerf.py:32-37), one
// output element per thread.  Each of the fp32 row X0, its bf16 copy X0b and its split planes
// X0s = [hi | lo | hi | lo] (hi = bf16(v), lo = bf16(v − hi), row length 4·K0p) is written when
// non-null.  o + dir*z is evaluated as two rounded ops like the reference
// (no FMA contraction: sin(2^9 x) amplifies a 1-ulp difference in x by 512).
__global__ void k_encode(const float* __restrict__ rays, int rs, int dir_off, const float* __restrict__ z, int S, int ldz,
                         int64_t P, int n_freq, int K0, int K0p, float* __restrict__ X0, bf16* __restrict__ X0b,
                         bf16* __restrict__ X0s) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= P * K0p) return;
    const int64_t p = i / K0p;
    const int c = (int)(i % K0p);
    const int64_t r = p / S;
    const float v = c < K0 ? pe_value(rays + r * rs, dir_off, z[r * ldz + (p - r * S)], c, n_freq, K0) : 0.f;
    if (X0) X0[i] = v;
    const bf16 hi = (bf16)v;
    if (X0b) X0b[i] = hi;
    if (X0s) {
        bf16* r = X0s + p * 4 * K0p + c;
        const bf16 lo = (bf16)(v - (float)hi);
        r[0] = hi;
        r[K0p] = lo;
        r[2 * K0p] = hi;
        r[3 * K0p] = lo;
    }
}

// Per-ray terms: semantic bias rows of fc_net.0 / fc_net.<skip>, sun / t bias rows of the Q
// GEMM, and the sky_color MLP (spnerf.py:244-249,355).  One 256-thread block per ray.
__global__ __launch_bounds__(256) void k_ray_fwd(RayFwdArgs a) {
    const int64_t ray = blockIdx.x;
    const int tid = threadIdx.x;
    const Dims& d = a.d;
    const float* P = a.packed;
    const float* r = a.rays + ray * a.rs;
    const float s0 = r[8], s1 = r[9], s2 = r[10];
    if (a.sem_on) {
        int64_t lab = a.labels[ray];
        if (lab == -100) lab = d.C;
        const float* e = P + a.k.emb + lab * d.sd;
        for (int n = tid; n < d.W; n += blockDim.x) {
            float v0 = 0.f, v4 = 0.f;
            for (int j = 0; j < d.sd; ++j) {
                v0 += P[a.k.Wsem0 + (int64_t)n * d.sd + j] * e[j];
                v4 += P[a.k.Wsem4 + (int64_t)n * d.sd + j] * e[j];
            }
            a.rb0[ray * d.W + n] = v0;
            a.rb4[ray * d.W + n] = v4;
        }
    }
    if (a.need_q) {
        for (int n = tid; n < d.NQ; n += blockDim.x) {
            float v = 0.f;
            if (n < d.H) {
                const float* w = P + a.k.Wsun + n * 3;
                v = w[0] * s0 + w[1] * s1 + w[2] * s2;
            } else if (n >= 2 * d.H) {
                const float* w = P + a.k.Wtt + (int64_t)(n - 2 * d.H) * d.td;
                const float* t = a.temb + ray * d.td;
                for (int j = 0; j < d.td; ++j) v += w[j] * t[j];
            }
            a.rbQ[ray * d.NQ + n] = v;
        }
    }
    if (a.need_sky) {
        __shared__ float red[3][256];
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
        for (int n = tid; n < d.H; n += blockDim.x) {
            const float* w = P + a.k.Wk1 + n * 3;
            const float hv = fmaxf(P[a.k.bk1 + n] + (w[0] * s0 + w[1] * s1 + w[2] * s2), 0.f);
            a.skyh[ray * d.H + n] = hv;
            acc0 += P[a.k.Wk2 + n] * hv;
            acc1 += P[a.k.Wk2 + d.H + n] * hv;
            acc2 += P[a.k.Wk2 + 2 * d.H + n] * hv;
        }
        red[0][tid] = acc0;
        red[1][tid] = acc1;
        red[2][tid] = acc2;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st)
                for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + st];
            __syncthreads();
        }
        if (tid < 3) a.sky[ray * 4 + tid] = sigmoidf_(red[tid][0] + P[a.k.bk2 + tid]);
    }
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// lane-partial dot product of a row with a weight vector, columns 4*lane + 256*i
template <typename T>
__device__ __forceinline__ float pdot(const T* __restrict__ x, const float* __restrict__ w, int n, int lane) {
    float s = 0.f;
    for (int k = 4 * lane; k < n; k += 256) {
        const f32x4 a = ld4(x + k);
        const f32x4 b = *reinterpret_cast<const f32x4*>(w + k);
        s += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
    }
    return s;
}

// Narrow output heads (spnerf.py:333-367): σ = softplus, albedo = sigmoid·1.002−0.001,
// sun = sigmoid, β = softplus, semantic logits; sky broadcast per ray.  One wavefront per
// point: every row read is a coalesced 1-KiB sweep, dot products end in a DPP reduction.
template <typename T>
__global__ __launch_bounds__(256) void k_heads_fwd(HeadsArgs<T> a, PackedOffs k) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const Dims& d = a.d;
    const float* Pk = a.packed;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.P; p += nw) {
        float* o = a.out + p * d.NO;
        float* hs = a.hsave + p * 8;
        const float spre = wsum(pdot(a.HL + p * d.W, Pk + k.wsig, d.W, lane)) + Pk[k.bsig];
        float sun = 0.f, rgb[3] = {0.f, 0.f, 0.f}, bpre = 0.f;
        if (a.mode != 1) sun = sigmoidf_(wsum(pdot(a.S3 + p * d.H, Pk + k.ws4, d.H, lane)) + Pk[k.bs4]);
        if (a.mode == 0) {
            const T* R1 = a.Q + p * d.NQ + d.H;
            for (int c = 0; c < 3; ++c) rgb[c] = sigmoidf_(wsum(pdot(R1, Pk + k.Wr2 + c * d.H, d.H, lane)) + Pk[k.br2 + c]);
            if (d.beta) bpre = wsum(pdot(a.Q + p * d.NQ + 2 * d.H, Pk + k.wb2, d.H, lane)) + Pk[k.bb2];
            if (d.sem) {
                const T* M1 = a.G + p * d.NG + d.W;
                for (int c = 0; c < d.C; ++c) {
                    const float v = wsum(pdot(M1, Pk + k.Wm2 + c * d.H, d.H, lane)) + Pk[k.bm2 + c];
                    if (lane == 0) o[d.sem_col + c] = v;
                }
            }
        }
        if (lane == 0) {
            o[3] = softplusf_(spre);
            hs[0] = spre;
            if (a.mode == 1) continue;
            o[4] = sun;
            hs[4] = sun;
            if (a.mode == 2) {
                o[0] = o[1] = o[2] = o[5] = o[6] = o[7] = 0.f;
                for (int c = 8; c < d.NO; ++c) o[c] = 0.f;
                continue;
            }
            for (int c = 0; c < 3; ++c) {
                hs[1 + c] = rgb[c];
                o[c] = __fsub_rn(__fmul_rn(rgb[c], 1.002f), 0.001f);
            }
            const float* sk = a.sky + (p / a.S) * 4;
            o[5] = sk[0];
            o[6] = sk[1];
            o[7] = sk[2];
            if (d.beta) {
                hs[5] = bpre;
                o[8] = softplusf_(bpre);
            }
        }
    }
}

int g_heads_variant = 1;  // 0 = the one-point-at-a-time k_heads_fwd (ablation)

template <typename T> struct RawOf;
template <> struct RawOf<float> { using type = f32x4; };
template <> struct RawOf<bf16> { using type = u32x2; };
template <typename T>
__device__ __forceinline__ typename RawOf<T>::type ld_raw(const T* p) {
    return *reinterpret_cast<const typename RawOf<T>::type*>(p);
}

// The rows one point's heads read: its last trunk row (σ), sun_v.3 output, rgb / β hidden
// (Q) and semantic hidden (G); lane `l` holds columns 4l + 256i.
template <typename T, int NC, int NH>
struct HeadRows {
    typename RawOf<T>::type hl[NC], s3[NH], r1[NH], b1[NH], m1[NH];
    float sp;  // k_heads_fwd_v<…, SIGB>: the σ pre-activation from hsave
};

// Narrow output heads (spnerf.py:333-367): σ = softplus, albedo = sigmoid·1.002−0.001,
// sun = sigmoid, β = softplus, semantic logits; sky broadcast per ray.  One wavefront per
// point, W ≤ 256·NC.  HBM-latency bound, so the rows of point p + nw are in flight while
// point p's dot products and DPP reductions run: two register sets in turn (no copies, which
// would wait on the loads), a fixed number of row loads per point (rows a mode does not use
// are re-reads of the σ row, so the wait counts are static), and every other operand in
// registers or LDS (σ / sun / rgb / β weights in VGPRs, semantic weights staged in LDS) so no
// vector-memory load is issued behind the prefetch.  A point's output row leaves as one
// coalesced store.
// SIGB: the σ pre-activation comes from hsave[p·8], written by the fused training trunk with this
// kernel's own arithmetic (TrunkArgs::sig_hsave) — no H_L row is loaded
template <typename T, int NC, bool SIGB = false>
__global__ __launch_bounds__(256) void k_heads_fwd_v(HeadsArgs<T> a, PackedOffs k) {
    constexpr int NH = (NC + 1) / 2;
    extern __shared__ float wsem[];  // [C][H] semantic weights + [C] biases (mode 0, semantic model)
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const Dims& d = a.d;
    const float* Pk = a.packed;
    const int W = d.W, H = d.H;
    const bool sun_on = a.mode != 1, full = a.mode == 0, beta = full && d.beta, sem = full && d.sem;
    if (sem) {
        for (int i = threadIdx.x; i < d.C * H; i += 256) wsem[i] = Pk[k.Wm2 + i];
        if (threadIdx.x < d.C) wsem[d.C * H + threadIdx.x] = Pk[k.bm2 + threadIdx.x];
        __syncthreads();
    }
    int cw[NC], ch[NH];
    bool vw[NC], vh[NH];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        vw[i] = 4 * lane + 256 * i < W;
        cw[i] = vw[i] ? 4 * lane + 256 * i : 0;
    }
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        vh[i] = 4 * lane + 256 * i < H;
        ch[i] = vh[i] ? 4 * lane + 256 * i : 0;
    }
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 wsg[NC], w4[NH], wr[3][NH], wb[NH];
#pragma unroll
    for (int i = 0; i < NC; ++i) wsg[i] = vw[i] ? ld4(Pk + k.wsig + cw[i]) : z4;
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        w4[i] = vh[i] && sun_on ? ld4(Pk + k.ws4 + ch[i]) : z4;
        for (int c = 0; c < 3; ++c) wr[c][i] = vh[i] && full ? ld4(Pk + k.Wr2 + c * H + ch[i]) : z4;
        wb[i] = vh[i] && beta ? ld4(Pk + k.wb2 + ch[i]) : z4;
    }
    const float bsig = Pk[k.bsig];
    const float bs4 = sun_on ? Pk[k.bs4] : 0.f;
    const float br0 = full ? Pk[k.br2] : 0.f, br1 = full ? Pk[k.br2 + 1] : 0.f, br2 = full ? Pk[k.br2 + 2] : 0.f;
    const float bb = beta ? Pk[k.bb2] : 0.f;

    // row bases of point p; unused rows alias the σ row (SIGB: the Q row)
    auto load = [&](int64_t p, HeadRows<T, NC, NH>& r) {
        const T* q = a.Q + p * d.NQ;
        const T* hl = SIGB ? q : a.HL + p * W;
        const T* s3 = sun_on ? a.S3 + p * H : hl;
        const T* r1 = full ? q + H : hl;
        const T* b1 = beta ? q + 2 * H : hl;
        const T* m1 = sem ? a.G + p * d.NG + W : hl;
        if constexpr (SIGB) {
            r.sp = a.hsave[p * 8];
        } else {
#pragma unroll
            for (int i = 0; i < NC; ++i) r.hl[i] = ld_raw(hl + cw[i]);
        }
#pragma unroll
        for (int i = 0; i < NH; ++i) {
            r.s3[i] = ld_raw(s3 + ch[i]);
            r.r1[i] = ld_raw(r1 + ch[i]);
            r.b1[i] = ld_raw(b1 + ch[i]);
            r.m1[i] = ld_raw(m1 + ch[i]);
        }
    };

    auto body = [&](int64_t p, const HeadRows<T, NC, NH>& cur, HeadRows<T, NC, NH>& nxt) {
        // this point's sky colour before the prefetch, so waiting on it leaves the prefetch in flight
        float sky = 0.f;
        if (full && lane >= 5 && lane <= 7) sky = a.sky[(int64_t)((int)p / a.S) * 4 + lane - 5];
        load(std::min(p + nw, a.P - 1), nxt);
        // lane-partial dot products (masked columns carry zero weights)
        float ps = 0.f, pu = 0.f, pr0 = 0.f, pr1 = 0.f, pr2 = 0.f, pb = 0.f;
        if constexpr (!SIGB) {
#pragma unroll
            for (int i = 0; i < NC; ++i) ps += dot4(raw_f32(cur.hl[i]), wsg[i]);
        }
#pragma unroll
        for (int i = 0; i < NH; ++i) {
            pu += dot4(raw_f32(cur.s3[i]), w4[i]);
            const f32x4 r = raw_f32(cur.r1[i]);
            pr0 += dot4(r, wr[0][i]);
            pr1 += dot4(r, wr[1][i]);
            pr2 += dot4(r, wr[2][i]);
            pb += dot4(raw_f32(cur.b1[i]), wb[i]);
        }
        const float spre = SIGB ? cur.sp : wave_total(ps) + bsig;
        float ov = lane == 3 ? softplusf_(spre) : 0.f;  // this lane's output column
        float hv = spre;                                // this lane's hsave column (lane 0: σ pre-activation)
        float* o = a.out + p * d.NO;
        float* hs = a.hsave + p * 8;
        if (!sun_on) {
            if (lane == 3) o[3] = ov;
            if (lane == 0) hs[0] = hv;
            return;
        }
        const float sun = sigmoidf_(wave_total(pu) + bs4);
        if (lane == 4) ov = hv = sun;
        if (full) {
            const float g0 = sigmoidf_(wave_total(pr0) + br0), g1 = sigmoidf_(wave_total(pr1) + br1),
                        g2 = sigmoidf_(wave_total(pr2) + br2);
            const float g = lane == 0 ? g0 : lane == 1 ? g1 : g2;
            if (lane < 3) ov = __fsub_rn(__fmul_rn(g, 1.002f), 0.001f);
            if (lane >= 1 && lane <= 3) hv = lane == 1 ? g0 : lane == 2 ? g1 : g2;  // hsave[1 + c] = rgb c
            if (lane >= 5 && lane <= 7) ov = sky;
            if (beta) {
                const float bpre = wave_total(pb) + bb;
                if (lane == 8) ov = softplusf_(bpre);
                if (lane == 5) hv = bpre;
            }
            if (sem) {
                for (int c = 0; c < d.C; ++c) {
                    float pm = 0.f;
#pragma unroll
                    for (int i = 0; i < NH; ++i)
                        pm += dot4(raw_f32(cur.m1[i]), vh[i] ? *reinterpret_cast<const f32x4*>(wsem + c * H + ch[i]) : z4);
                    const float v = wave_total(pm) + wsem[d.C * H + c];
                    if (lane == d.sem_col + c) ov = v;
                }
            }
        }
        if (lane < d.NO) o[lane] = ov;
        if (lane == 0 || lane == 4 || (full && (lane <= 3 || (lane == 5 && d.beta)))) hs[lane] = hv;
    };

    // the point index is wave-uniform: keep it (and every row address) in scalar registers;
    // P < 2^31 (spnerf_mlp_forward checks it)
    int64_t p = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (p >= a.P) return;
    // two register sets in turn (a third, prefetching two points ahead, measured no faster)
    HeadRows<T, NC, NH> ra, rb;
    load(p, ra);
    for (;;) {
        body(p, ra, rb);
        if ((p += nw) >= a.P) break;
        body(p, rb, ra);
        if ((p += nw) >= a.P) break;
    }
}

// Backward of the narrow heads, one wavefront per point: per-point pre-activation gradients
// (hpre, reduced over points into the head weights by the skinny reduction) and the
// gradients of the hidden layers feeding them (dX = dY·W, × sin' saved in D*), written as
// coalesced rows.
template <typename T>
__global__ __launch_bounds__(256) void k_heads_bwd(HeadsBwdArgs<T> a, PackedOffs k) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const Dims& d = a.d;
    const float* Pk = a.packed;
    const int H = d.H;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.P; p += nw) {
        const float* g = a.d_out + p * d.NO;
        const float* hs = a.hsave + p * 8;
        float* hp = a.hpre + p * d.HP;
        const float dsig = softplus_grad(g[3], hs[0]);
        float dys = 0.f, dy[3] = {0.f, 0.f, 0.f}, db = 0.f;
        if (a.mode != 1) {
            const float s = hs[4];
            dys = g[4] * (1.f - s) * s;
        }
        if (a.mode == 0) {
            for (int c = 0; c < 3; ++c) {
                const float s = hs[1 + c];
                dy[c] = g[c] * 1.002f * (1.f - s) * s;
            }
            if (d.beta) db = softplus_grad(g[8], hs[5]);
        }
        for (int c = lane; c < d.HP; c += 64) {
            float v = 0.f;
            if (c == 0) v = dsig;
            else if (c <= 3) v = dy[c - 1];
            else if (c == 4) v = dys;
            else if (c == 5) v = db;
            else if (a.mode == 0) v = g[d.sem_col + c - 6];
            hp[c] = v;
        }
        if (a.mode == 1) continue;
        for (int c = 4 * lane; c < H; c += 256) {
            const f32x4 D = ld4(a.DS3 + p * H + c);
            const f32x4 w = *reinterpret_cast<const f32x4*>(Pk + k.ws4 + c);
            st4(a.dS3 + p * H + c, (dys * w) * D);
        }
        if (a.mode == 2) continue;
        for (int c = 4 * lane; c < H; c += 256) {
            const f32x4 D = ld4(a.DQ + p * d.NQ + H + c);
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(Pk + k.Wr2 + c);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(Pk + k.Wr2 + H + c);
            const f32x4 w2 = *reinterpret_cast<const f32x4*>(Pk + k.Wr2 + 2 * H + c);
            st4(a.dZQ + p * d.NQ + H + c, (dy[0] * w0 + dy[1] * w1 + dy[2] * w2) * D);
            if (d.beta) {
                const f32x4 Db = ld4(a.DQ + p * d.NQ + 2 * H + c);
                const f32x4 wb = *reinterpret_cast<const f32x4*>(Pk + k.wb2 + c);
                st4(a.dZQ + p * d.NQ + 2 * H + c, (db * wb) * Db);
            }
            if (d.sem) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int j = 0; j < d.C; ++j)
                    acc += g[d.sem_col + j] * *reinterpret_cast<const f32x4*>(Pk + k.Wm2 + j * H + c);
                const f32x4 Dm = ld4(a.DG + p * d.NG + d.W + c);
                st4(a.dZG + p * d.NG + d.W + c, acc * Dm);
            }
        }
    }
}

// k_heads_bwd with the latency structure of k_heads_fwd_v: the d_out row, the hsave row and
// the D rows of point p + nw load into a second register set while point p computes (two sets
// in turn), the d_out / hsave values come from one coalesced load each (lane c holds column c,
// read back with readlane), the head weights sit in VGPRs / LDS.  Same arithmetic per element
// as k_heads_bwd (bit-identical).  H ≤ 256·NH.
template <typename T, int NH>
__global__ __launch_bounds__(256) void k_heads_bwd_v(HeadsBwdArgs<T> a, PackedOffs k) {
    extern __shared__ float wsem[];  // [C][H] semantic weights (mode 0, semantic model)
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const Dims& d = a.d;
    const float* Pk = a.packed;
    const int H = d.H;
    const bool sun_on = a.mode != 1, full = a.mode == 0, beta = full && d.beta, sem = full && d.sem;
    if (sem) {
        for (int i = threadIdx.x; i < d.C * H; i += 256) wsem[i] = Pk[k.Wm2 + i];
        __syncthreads();
    }
    int ch[NH];
    bool vh[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        vh[i] = 4 * lane + 256 * i < H;
        ch[i] = vh[i] ? 4 * lane + 256 * i : 0;
    }
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 w4[NH], wr[3][NH], wb[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        w4[i] = vh[i] && sun_on ? ld4(Pk + k.ws4 + ch[i]) : z4;
        for (int c = 0; c < 3; ++c) wr[c][i] = vh[i] && full ? ld4(Pk + k.Wr2 + c * H + ch[i]) : z4;
        wb[i] = vh[i] && beta ? ld4(Pk + k.wb2 + ch[i]) : z4;
    }
    struct Rows {
        float g, h;  // lane c: d_out[c] (c < NO), hsave[c] (c < 8)
        typename RawOf<T>::type s3[NH], qr[NH], qb[NH], gm[NH];
    };
    auto load = [&](int64_t p, Rows& r) {
        r.g = a.d_out[p * d.NO + min(lane, d.NO - 1)];
        r.h = a.hsave[p * 8 + (lane & 7)];
        if (sun_on) {
#pragma unroll
            for (int i = 0; i < NH; ++i) r.s3[i] = ld_raw(a.DS3 + p * H + ch[i]);
        }
        if (full) {
#pragma unroll
            for (int i = 0; i < NH; ++i) {
                r.qr[i] = ld_raw(a.DQ + p * d.NQ + H + ch[i]);
                if (beta) r.qb[i] = ld_raw(a.DQ + p * d.NQ + 2 * H + ch[i]);
                if (sem) r.gm[i] = ld_raw(a.DG + p * d.NG + d.W + ch[i]);
            }
        }
    };
    auto col = [](float v, int c) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), c)); };
    auto body = [&](int64_t p, const Rows& cur, Rows& nxt) {
        load(std::min(p + nw, a.P - 1), nxt);
        const float dsig = softplus_grad(col(cur.g, 3), col(cur.h, 0));
        float dys = 0.f, dy[3] = {0.f, 0.f, 0.f}, db = 0.f;
        if (sun_on) {
            const float s = col(cur.h, 4);
            dys = col(cur.g, 4) * (1.f - s) * s;
        }
        if (full) {
            for (int c = 0; c < 3; ++c) {
                const float s = col(cur.h, 1 + c);
                dy[c] = col(cur.g, c) * 1.002f * (1.f - s) * s;
            }
            if (d.beta) db = softplus_grad(col(cur.g, 8), col(cur.h, 5));
        }
        // hpre row [dσ, drgb3, dsun, dβ, dsem C]: lane c; the semantic gradients are d_out's
        // columns sem_col + c - 6, shifted across lanes
        const float gs = __shfl(cur.g, min(d.sem_col + lane - 6 + 64, 63 + 64) - 64, 64);
        if (lane < d.HP) {
            float v = 0.f;
            if (lane == 0) v = dsig;
            else if (lane <= 3) v = dy[lane - 1];
            else if (lane == 4) v = dys;
            else if (lane == 5) v = db;
            else if (full) v = gs;
            a.hpre[p * d.HP + lane] = v;
        }
        if (!sun_on) return;
        auto st = [&](T* q, f32x4 v) {
            if (a.emu)
                for (int e = 0; e < 4; ++e) v[e] = (float)(bf16)v[e];
            st4(q, v);
        };
#pragma unroll
        for (int i = 0; i < NH; ++i)
            if (vh[i]) st(a.dS3 + p * H + ch[i], (dys * w4[i]) * raw_f32(cur.s3[i]));
        if (!full) return;
#pragma unroll
        for (int i = 0; i < NH; ++i) {
            if (!vh[i]) continue;
            st(a.dZQ + p * d.NQ + H + ch[i], (dy[0] * wr[0][i] + dy[1] * wr[1][i] + dy[2] * wr[2][i]) * raw_f32(cur.qr[i]));
            if (d.beta) st(a.dZQ + p * d.NQ + 2 * H + ch[i], (db * wb[i]) * raw_f32(cur.qb[i]));
            if (d.sem) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int j = 0; j < d.C; ++j)
                    acc += col(cur.g, d.sem_col + j) * *reinterpret_cast<const f32x4*>(wsem + j * H + ch[i]);
                st(a.dZG + p * d.NG + d.W + ch[i], acc * raw_f32(cur.gm[i]));
            }
        }
    };
    int64_t p = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (p >= a.P) return;
    Rows ra, rb;
    load(p, ra);
    for (;;) {
        body(p, ra, rb);
        if ((p += nw) >= a.P) break;
        body(p, rb, ra);
        if ((p += nw) >= a.P) break;
    }
}

// out[ray][n] = Σ_{s<S} in[(ray*S + s)*ld + c0 + n]
template <typename T>
__global__ void k_ray_rowsum(const T* __restrict__ in, int ld, int c0, int N, int S, float* __restrict__ out,
                             int ldo) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ray = blockIdx.y;
    if (n >= N) return;
    const T* p = in + ray * S * (int64_t)ld + c0 + n;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += ld1(p + (int64_t)i * ld);
    out[ray * ldo + n] = s;
}

// Same sum for bf16 rows with N, ld, c0 multiples of 8: one block per ray, a thread owns 8
// columns (16-B loads) in one of 256/(N/8) row phases; phases combined in a fixed order.  A
// thread's rows load 8 at a time before they are summed (in the same order): one HBM latency per
// 8 rows instead of one per row (two launches per step: C4 0.138 -> 0.135 ms, C4@512 0.044 ->
// 0.037 ms, bit-identical; the same batching in the skinny reductions measured level)
__global__ __launch_bounds__(256) void k_ray_rowsum16(const bf16* __restrict__ in, int ld, int c0, int N, int S,
                                                      float* __restrict__ out, int ldo) {
    __shared__ float part[256 * 8];
    const int64_t ray = blockIdx.x;
    const int nq = N >> 3;                   // column chunks (<= 256)
    const int ph = threadIdx.x / nq, q = threadIdx.x % nq;
    const int nph = 256 / nq;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ph < nph) {
        const bf16* p = in + ray * S * (int64_t)ld + c0 + 8 * q;
        for (int i0 = ph; i0 < S; i0 += 8 * nph) {
            u32x4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * nph;
                v[u] = i < S ? ldg16(p + (int64_t)i * ld) : u32x4{0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u * nph < S) {
                    float f[8];
                    unpack8(v[u], f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += f[e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[threadIdx.x * 8 + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < nq) {
        float r[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = part[threadIdx.x * 8 + e];
        for (int k = 1; k < nph; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] += part[(k * nq + threadIdx.x) * 8 + e];
#pragma unroll
        for (int e = 0; e < 8; ++e) out[ray * ldo + 8 * threadIdx.x + e] = r[e];
    }
}

// The per-ray sums of the 512-wide trunk dZ in the fused backward's order (S % 64 == 0): per
// 64-point tile the column sums of tile_colsum_part / _final (trunk.h), read from HBM here (the
// layer-by-layer backward; k_trunk_bwd_bf16 forms them from its LDS image) ...
__global__ __launch_bounds__(512) void k_tile_rowsum16(const bf16* __restrict__ in, float* __restrict__ part_out) {
    __shared__ float part[8 * 512];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bf16* src = in + ((int64_t)blockIdx.x * 64 + 8 * w) * 512 + 8 * lane;
    u32x4 rows[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) rows[r] = ldg16(src + r * 512);
    float a[8];
    tile_colsum_part(rows, a);
    *reinterpret_cast<f32x4*>(part + w * 512 + lane * 8) = f32x4{a[0], a[1], a[2], a[3]};
    *reinterpret_cast<f32x4*>(part + w * 512 + lane * 8 + 4) = f32x4{a[4], a[5], a[6], a[7]};
    __syncthreads();
    part_out[(int64_t)blockIdx.x * 512 + tid] = tile_colsum_final(part, tid);
}

// ... and the T tiles of a ray added in tile order: out[ray][c] = Σ_t part[ray·T + t][c]
// (blockIdx.y = 1: the second part / output pair — layer 0 and the skip layer in one launch)
__global__ __launch_bounds__(256) void k_ray_tiles_sum(const float* __restrict__ part0, int T, int64_t n_rays,
                                                       float* __restrict__ out0, const float* __restrict__ part1,
                                                       float* __restrict__ out1) {
    const float* part = blockIdx.y ? part1 : part0;
    float* out = blockIdx.y ? out1 : out0;
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_rays * 512) return;
    const int64_t ray = i >> 9;
    const int c = (int)(i & 511);
    const float* p = part + ray * T * 512 + c;
    float s = p[0];
    for (int t = 1; t < T; ++t) s += p[t * 512];
    out[i] = s;
}

// Per-ray backward pieces: sky MLP pre-activation grads, the semantic-embedding input grad
// and the time-embedding input grad.  One 256-thread block per ray.  The sky colour's gradient
// is the sum of d_out's sky columns over the ray's samples (the sky is per ray, broadcast to every
// sample: spnerf.py:244-249): wave c sums column c, its lanes strided over the samples (a separate
// one-thread-per-column launch walked the 128 samples serially: 50 us per C4 step).
__global__ __launch_bounds__(256) void k_ray_bwd(RayBwdArgs a) {
    const int64_t ray = blockIdx.x;
    const int tid = threadIdx.x;
    const Dims& d = a.d;
    const float* P = a.packed;
    if (a.sky_on) {
        __shared__ float dsk[3];
        if ((tid >> 6) < 3) {
            const int c = tid >> 6, lane = tid & 63;
            const float* q = a.d_out + ray * a.S * (int64_t)a.NO + 5 + c;
            float v = 0.f;
            for (int s = lane; s < a.S; s += 64) v += q[(int64_t)s * a.NO];
            v = wave_sum(v);
            if (lane == 0) dsk[c] = v;
        }
        __syncthreads();
        float dp[3];
        for (int c = 0; c < 3; ++c) {
            const float s = a.sky[ray * 4 + c];
            dp[c] = dsk[c] * (1.f - s) * s;
        }
        if (tid < 3) a.skyd[ray * 4 + tid] = dp[tid];
        for (int n = tid; n < d.H; n += blockDim.x) {
            const float hv = a.skyh[ray * d.H + n];
            const float g = dp[0] * P[a.k.Wk2 + n] + dp[1] * P[a.k.Wk2 + d.H + n] + dp[2] * P[a.k.Wk2 + 2 * d.H + n];
            a.skydh[ray * d.H + n] = hv > 0.f ? g : 0.f;
        }
    }
    __shared__ float red[256];
    if (a.sem_on) {
        int64_t lab = a.labels[ray];
        if (lab == -100) lab = d.C;
        for (int j = tid; j < d.sd; j += blockDim.x) a.embr[ray * d.sd + j] = P[a.k.emb + lab * d.sd + j];
        for (int j = 0; j < d.sd; ++j) {
            float acc = 0.f;
            for (int n = tid; n < d.W; n += blockDim.x)
                acc += a.R0[ray * d.W + n] * P[a.k.Wsem0 + (int64_t)n * d.sd + j] +
                       a.R4[ray * d.W + n] * P[a.k.Wsem4 + (int64_t)n * d.sd + j];
            red[tid] = acc;
            __syncthreads();
            for (int st = 128; st > 0; st >>= 1) {
                if (tid < st) red[tid] += red[tid + st];
                __syncthreads();
            }
            if (tid == 0) a.gemb[ray * d.sd + j] = red[0];
            __syncthreads();
        }
    }
    if (a.beta_on && a.grad_t) {
        for (int j = 0; j < d.td; ++j) {
            float acc = 0.f;
            for (int n = tid; n < d.H; n += blockDim.x)
                acc += a.RQ[ray * d.NQ + 2 * d.H + n] * P[a.k.Wtt + (int64_t)n * d.td + j];
            red[tid] = acc;
            __syncthreads();
            for (int st = 128; st > 0; st >>= 1) {
                if (tid < st) red[tid] += red[tid + st];
                __syncthreads();
            }
            if (tid == 0) a.grad_t[ray * d.td + j] = red[0];
            __syncthreads();
        }
    }
}

// d_emb[c][j] = Σ_{rays with label c} gemb[ray][j]; the padding row (−100 → C) gets none
// (nn.Embedding padding_idx, spnerf.py:191-194).
// One block per (class, j): rays strided over 256 threads, then a fixed-order tree in LDS.
__global__ __launch_bounds__(256) void k_class_sum(int64_t B, const float* __restrict__ gemb, int sd,
                                                   const int64_t* __restrict__ labels, int C, float* __restrict__ out,
                                                   int accumulate) {
    __shared__ float red[256];
    const int c = blockIdx.x / sd, j = blockIdx.x % sd;
    float s = 0.f;
    if (c < C)
        for (int64_t r = threadIdx.x; r < B; r += 256)
            if (labels[r] == c) s += gemb[r * sd + j];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = accumulate ? out[blockIdx.x] + red[0] : red[0];
}

// Zeroing with a kernel of our own instead of hipMemsetAsync: inside a captured HIP graph the
// runtime's memset node (a blit kernel) did not survive later eager memsets on this ROCm —
// replays then left every 4th float of the range stale (tests/test_gpu_graph.py).
__global__ void k_zero(float* __restrict__ p, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0.f;
}

// ------------------------------------------------------------------------------------------
// launch functions
// ------------------------------------------------------------------------------------------

int32_t zero_fill(float* p, int64_t n, hipStream_t s) {
    if (n <= 0) return SPNERF_OK;
    ProfScope prof("zero", s, 0.0, 4.0 * n);
    hipLaunchKernelGGL(k_zero, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, s, p, n);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

int32_t ray_fwd(const RayFwdArgs& a, int64_t n_rays, hipStream_t s) {
    ProfScope prof("ray_terms", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_ray_fwd, dim3((unsigned)n_rays), dim3(256), 0, s, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

int32_t ray_bwd(const RayBwdArgs& a, int64_t n_rays, hipStream_t s) {
    ProfScope prof("ray_terms", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_ray_bwd, dim3((unsigned)n_rays), dim3(256), 0, s, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

int32_t class_sum(int64_t B, const float* gemb, int sd, const int64_t* labels, int C, float* out, int accumulate,
                  hipStream_t s) {
    ProfScope prof("ray_terms", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_class_sum, dim3((C + 1) * sd), dim3(256), 0, s, B, gemb, sd, labels, C, out, accumulate);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

int32_t encode(const float* rays, int rs, int dir_off, const float* z, int S, int ldz, int64_t P, int K0, int K0p,
               float* X0, bf16* X0b, bf16* X0s, hipStream_t s) {
    const int64_t n = P * K0p;
    // the planes (10 B per element) stand in for the fp32 rows; the bf16 copy goes with either
    ProfScope prof("encode", s, 0.0, (X0s ? 10.0 : 4.0 + (X0b ? 2.0 : 0.0)) * n);
    hipLaunchKernelGGL(k_encode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rays, rs, dir_off, z, S, ldz, P,
                       K0 == 3 ? 0 : K0 / 6, K0, K0p, X0, X0b, X0s);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

template <typename T>
static int32_t heads_fwd_t(const HeadsArgs<T>& a, const PackedOffs& k, bool sig_done, hipStream_t s) {
    const Dims& d = a.d;
    const int64_t P = a.P;
    const int W = d.W, H = d.H, mode = a.mode;
    const int grid = (int)std::min<int64_t>(cdiv(P, 4), 8192);
    ProfScope prof("heads_fwd", s, 2.0 * P * ((sig_done ? 0 : W) + (mode != 1 ? 4 * H + H * d.C : 0)),
                   (d.bf ? 2.0 : 4.0) * P * ((sig_done ? 0 : W) + 3 * H) + 4.0 * P * (d.NO + (sig_done ? 1 : 0)));
    const int nc = g_heads_variant == 0 ? 0 : cdiv(W, 256);
    const size_t lds = mode == 0 && d.sem ? sizeof(float) * d.C * (H + 1) : 0;  // C × 257 floats (8 224 B at C = 8; the kernel runs for any C the LDS limit allows)
    if (sig_done && nc == 2) {  // σ from hsave (W = 512, bf16)
        hipLaunchKernelGGL((k_heads_fwd_v<T, 2, true>), dim3(grid), dim3(256), lds, s, a, k);
    } else {
        switch (nc) {
            case 1: hipLaunchKernelGGL((k_heads_fwd_v<T, 1>), dim3(grid), dim3(256), lds, s, a, k); break;
            case 2: hipLaunchKernelGGL((k_heads_fwd_v<T, 2>), dim3(grid), dim3(256), lds, s, a, k); break;
            case 3: hipLaunchKernelGGL((k_heads_fwd_v<T, 3>), dim3(grid), dim3(256), lds, s, a, k); break;
            case 4: hipLaunchKernelGGL((k_heads_fwd_v<T, 4>), dim3(grid), dim3(256), lds, s, a, k); break;
            default: hipLaunchKernelGGL(k_heads_fwd<T>, dim3(grid), dim3(256), 0, s, a, k);
        }
    }
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
int32_t heads_fwd(const HeadsArgs<float>& a, const PackedOffs& k, bool sig_done, hipStream_t s) {
    return heads_fwd_t(a, k, sig_done, s);
}
int32_t heads_fwd(const HeadsArgs<bf16>& a, const PackedOffs& k, bool sig_done, hipStream_t s) {
    return heads_fwd_t(a, k, sig_done, s);
}

template <typename T>
static int32_t heads_bwd_t(const HeadsBwdArgs<T>& a, const PackedOffs& k, hipStream_t s) {
    const Dims& d = a.d;
    const int64_t P = a.P;
    const int H = d.H;
    const double eb = std::is_same<T, bf16>::value ? 2.0 : 4.0;
    ProfScope prof("heads_bwd", s, 2.0 * P * 4 * H, 4.0 * P * (d.NO + d.HP) + eb * P * 6 * H);
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv(P, 4), 8192);
    const int nh = g_heads_variant == 0 ? 0 : cdiv(H, 256);
    const size_t lds = a.mode == 0 && d.sem ? sizeof(float) * d.C * H : 0;
    if (nh == 1) hipLaunchKernelGGL((k_heads_bwd_v<T, 1>), dim3(grid), dim3(256), lds, s, a, k);
    else if (nh == 2) hipLaunchKernelGGL((k_heads_bwd_v<T, 2>), dim3(grid), dim3(256), lds, s, a, k);
    else hipLaunchKernelGGL(k_heads_bwd<T>, dim3(grid), dim3(256), 0, s, a, k);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
int32_t heads_bwd(const HeadsBwdArgs<float>& a, const PackedOffs& k, hipStream_t s) { return heads_bwd_t(a, k, s); }
int32_t heads_bwd(const HeadsBwdArgs<bf16>& a, const PackedOffs& k, hipStream_t s) { return heads_bwd_t(a, k, s); }

int32_t ray_tiles_sum(const bf16* dZ, float* part, int64_t P, int S, int64_t n_rays, float* out, hipStream_t s) {
    ProfScope prof("ray_rowsum", s, 0.0, (dZ ? 2.0 * P * 512 : 0.0) + 4.0 * (P / 64 + n_rays) * 512);
    if (dZ) {
        hipLaunchKernelGGL(k_tile_rowsum16, dim3((unsigned)(P / 64)), dim3(512), 0, s, dZ, part);
        SPN_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ray_tiles_sum, dim3((unsigned)cdiv(n_rays * 512, 256)), dim3(256), 0, s, part, S / 64, n_rays,
                       out, nullptr, nullptr);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

int32_t ray_tiles_sum_pair(const float* part0, float* out0, const float* part1, float* out1, int64_t P, int S,
                           int64_t n_rays, hipStream_t s) {
    ProfScope prof("ray_rowsum", s, 0.0, 2.0 * 4.0 * (P / 64 + n_rays) * 512);
    hipLaunchKernelGGL(k_ray_tiles_sum, dim3((unsigned)cdiv(n_rays * 512, 256), 2), dim3(256), 0, s, part0, S / 64,
                       n_rays, out0, part1, out1);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

template <typename T>
static int32_t ray_rowsum_t(const T* in, int ld, int c0, int N, int S, int64_t n_rays, float* out, int ldo, hipStream_t s) {
    ProfScope prof("ray_rowsum", s, 0.0, (double)n_rays * (S * (double)N * sizeof(T) + 4.0 * N));
    if constexpr (std::is_same<T, bf16>::value) {
        if (N % 8 == 0 && N <= 2048 && ld % 8 == 0 && c0 % 8 == 0) {
            hipLaunchKernelGGL(k_ray_rowsum16, dim3((unsigned)n_rays), dim3(256), 0, s, in, ld, c0, N, S, out, ldo);
            SPN_HIP(hipGetLastError());
            return SPNERF_OK;
        }
    }
    hipLaunchKernelGGL(k_ray_rowsum<T>, dim3(cdiv(N, 256), (unsigned)n_rays), dim3(256), 0, s, in, ld, c0, N, S, out, ldo);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
int32_t ray_rowsum(const float* in, int ld, int c0, int N, int S, int64_t n_rays, float* out, int ldo, hipStream_t s) {
    return ray_rowsum_t(in, ld, c0, N, S, n_rays, out, ldo, s);
}
int32_t ray_rowsum(const bf16* in, int ld, int c0, int N, int S, int64_t n_rays, float* out, int ldo, hipStream_t s) {
    return ray_rowsum_t(in, ld, c0, N, S, n_rays, out, ldo, s);
}

}  // namespace spn
