// Every loss form the reference trainer combines (main.py:125-174 over modules/metrics.py) with
// all upstream gradients, for the coarse and the fine pass of a render; the formulas are stated in
// include/spnerf_amd_loss.h.  Same structure as loss.hip, which keeps its one configuration:
//   k_tl_rays   one wavefront per ray (lanes stride the samples) handles both passes of the ray; a
//               block of 4 waves walks a fixed ray range and writes its 2 x 8 partial sums
//   k_tl_final  one block adds the partials in block order, counts the global valid labels and
//               writes the result block (loss, terms, raw MSE and PSNR per pass)
//   k_tl_grad   one wavefront per ray recomputes the ray's scalars and writes every gradient x dL
//               (device scalar).  β of the coarse pass weights both passes' colour: the wave that
//               owns the ray adds the two contributions to d_beta itself, so nothing is atomic.
// No atomics, no host synchronisation, fixed summation order: deterministic and graph-capturable.
#include "../../include/spnerf_amd_loss.h"
#include "common.h"
#include "wave.h"

namespace spn {

constexpr int kTlWaves = 4;
constexpr int kTlParts = 8;  // per pass: colour, squared error, log b, sc2, sc3, depth, nll, out-of-range labels
constexpr float kBetaMin = 0.05f;   // metrics.py:10
constexpr float kNllEps = 1e-6f;    // torch.nn.GaussianNLLLoss eps

struct TlArgs {
    spnerf_train_loss_opts o;
    spnerf_train_loss_pass p[2];
    int npass;
    float* partial;  // [nblocks][2 * kTlParts]
    int nblocks;
    float* result;   // SPNERF_LOSS_RESULT_FLOATS
    const float* g;  // dL (device scalar) for the gradients
};

__device__ __forceinline__ bool tl_beta(const TlArgs& a) { return (a.o.flags & SPNERF_LOSS_BETA) != 0; }
__device__ __forceinline__ bool tl_solar(const TlArgs& a) { return a.o.lambda_sc > 0.f; }
__device__ __forceinline__ int tl_form(const TlArgs& a) { return a.o.lambda_ds > 0.f ? a.o.depth_form : SPNERF_LOSS_DEPTH_NONE; }
__device__ __forceinline__ bool tl_sem(const TlArgs& a) { return a.o.lambda_ss > 0.f; }
__device__ __forceinline__ bool tl_subset(int form) {
    return form == SPNERF_LOSS_DEPTH_SUBSET_MSE || form == SPNERF_LOSS_DEPTH_SUBSET_GNLL;
}

// per-ray quantities of one pass, shared by the loss and its gradient (every lane holds them)
struct TlRay {
    float sq;            // Σ_c (rgb - t)^2
    float b;             // Σ_s w β + 0.05 (β form)
    float sc2, sc3;
    float dep;           // the ray's depth term, 0 when the selection leaves it out
    float sigma, diff;   // sqrt(Σ w (z - d)^2) unclamped (subset forms), d - t
    bool apply;
    float nll, bad;
};

__device__ __forceinline__ TlRay tl_ray(const TlArgs& a, const spnerf_train_loss_pass& P, int64_t r, int lane,
                                         float* sm_logit) {
    const int S = P.n_samples, form = tl_form(a);
    const bool beta = tl_beta(a), solar = tl_solar(a), subset = tl_subset(form);
    TlRay o{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, false, 0.f, 0.f};
    float c = 0.f;
    if (lane < 3) {
        const float d = P.rgb[r * 3 + lane] - a.o.target[r * 3 + lane];
        c = d * d;
    }
    o.sq = wave_sum(c);
    const float d = form ? P.depth[r] : 0.f;
    float sb = 0.f, s2 = 0.f, s3 = 0.f, v = 0.f;
    for (int s = lane; s < S; s += 64) {
        const int64_t i = r * S + s;
        const float w = (beta || subset) ? P.weights[i] : 0.f;
        if (beta) sb += w * a.o.beta[i * (int64_t)a.o.ld_beta];
        if (solar) {
            const float sun = P.sun_sc[i * (int64_t)P.ld_sun];
            const float dt = P.transparency_sc[i] - sun;
            s2 += dt * dt;
            s3 += P.weights_sc[i] * sun;
        }
        if (subset) {
            const float e = P.z_vals[i] - d;
            v += e * e * w;
        }
    }
    if (beta) o.b = wave_sum(sb) + kBetaMin;
    if (solar) {
        o.sc2 = wave_sum(s2);
        o.sc3 = 1.f - wave_sum(s3);
    }
    if (form) {
        o.diff = d - a.o.target_depth[r * (int64_t)a.o.ld_td];
        if (form == SPNERF_LOSS_DEPTH_ALL) {
            o.apply = true;
        } else {
            const float ts = a.o.target_std[r];
            o.sigma = sqrtf(wave_sum(v));
            o.apply = a.o.valid[r] > 0 && (fabsf(o.diff) > ts || o.sigma > ts);
        }
        if (o.apply) {
            if (form == SPNERF_LOSS_DEPTH_SUBSET_GNLL) {
                const float sc = fmaxf(o.sigma, kNllEps);
                o.dep = 0.5f * (logf(sc) + o.diff * o.diff / sc);
            } else {
                o.dep = a.o.target_weight[r * (int64_t)a.o.ld_td] * o.diff * o.diff;
            }
        }
    }
    if (tl_sem(a)) {
        const int C = a.o.n_classes;
        const int64_t lab = a.o.labels[r];
        if (lab != -100 && (lab < 0 || lab >= C)) o.bad = 1.f;
        if (lab != -100) {
            // log-softmax over C classes (lane c holds logit c; C ≤ 64)
            const float x = lane < C ? P.sem_logits[r * C + lane] : -INFINITY;
            float m = x;
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
            const float lse = m + logf(wave_sum(lane < C ? expf(x - m) : 0.f));
            const float xl = __shfl(x, (int)min<int64_t>(max<int64_t>(lab, 0), C - 1), 64);
            o.nll = lse - xl;
            if (sm_logit) *sm_logit = lane < C ? expf(x - lse) : 0.f;
        }
    }
    return o;
}

__global__ __launch_bounds__(64 * kTlWaves) void k_tl_rays(TlArgs a) {
    __shared__ float part[kTlWaves][2 * kTlParts];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t per = (a.o.n_rays + a.nblocks - 1) / a.nblocks;
    const int64_t r0 = blockIdx.x * per, r1 = min(a.o.n_rays, r0 + per);
    const bool beta = tl_beta(a);
    float acc[2 * kTlParts];
    for (int k = 0; k < 2 * kTlParts; ++k) acc[k] = 0.f;
    // (the pass is named, not indexed: a run-time index would put the arguments into scratch)
    auto pass = [&](const spnerf_train_loss_pass& P, float* q, int64_t r) {
        const TlRay o = tl_ray(a, P, r, lane, nullptr);
        q[0] += beta ? o.sq / (2.f * o.b * o.b) : o.sq;
        q[1] += o.sq;
        q[2] += beta ? logf(o.b) : 0.f;
        q[3] += o.sc2; q[4] += o.sc3; q[5] += o.dep; q[6] += o.nll; q[7] += o.bad;
    };
    for (int64_t r = r0 + wv; r < r1; r += kTlWaves) {
        pass(a.p[0], acc, r);
        if (a.npass > 1) pass(a.p[1], acc + kTlParts, r);
    }
    if (lane == 0)
        for (int k = 0; k < 2 * kTlParts; ++k) part[wv][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 2 * kTlParts) {
        float s = 0.f;
        for (int v = 0; v < kTlWaves; ++v) s += part[v][threadIdx.x];
        a.partial[(int64_t)blockIdx.x * (2 * kTlParts) + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void k_tl_final(TlArgs a) {
    constexpr int N = 2 * kTlParts;
    __shared__ float red[N + 1][256];
    const int t = threadIdx.x;
    float s[N];
    for (int k = 0; k < N; ++k) s[k] = 0.f;
    for (int b = t; b < a.nblocks; b += 256)
        for (int k = 0; k < N; ++k) s[k] += a.partial[(int64_t)b * N + k];
    float nv = 0.f;
    if (tl_sem(a))
        for (int64_t i = t; i < a.o.n_global; i += 256) nv += a.o.labels_global[i] != -100 ? 1.f : 0.f;
    for (int k = 0; k < N; ++k) red[k][t] = s[k];
    red[N][t] = nv;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (t < st)
            for (int k = 0; k <= N; ++k) red[k][t] += red[k][t + st];
        __syncthreads();
    }
    if (t == 0) {
        const float B = (float)a.o.n_rays;
        const bool beta = tl_beta(a), solar = tl_solar(a), sem = tl_sem(a);
        const int form = tl_form(a);
        // CE mean over the global batch's valid labels, per rank: Σ nll / (n_valid_global / world)
        const float den = red[N][0] / (float)a.o.world;
        float colour = 0.f, ds = 0.f, ss = 0.f;
        for (int k = 0; k < SPNERF_LOSS_RESULT_FLOATS; ++k) a.result[k] = 0.f;
        for (int p = 0; p < a.npass; ++p) {
            const int q = p * kTlParts;
            float* out = a.result + SPNERF_LOSS_PASS_BASE + p * SPNERF_LOSS_PASS_TERMS;
            const float col = red[q + 0][0] / (3.f * B);
            const float lb = beta ? (3.f + red[q + 2][0] / B) / 2.f : 0.f;
            const float sc2 = solar ? a.o.lambda_sc / 3.f * (red[q + 3][0] / B) : 0.f;
            const float sc3 = solar ? a.o.lambda_sc / 3.f * (red[q + 4][0] / B) : 0.f;
            const float dep = form ? a.o.lambda_ds / 3.f * red[q + 5][0] / B : 0.f;
            float ce = 0.f;
            if (sem) ce = (den > 0.f && red[q + 7][0] == 0.f) ? a.o.lambda_ss * (red[q + 6][0] / den) : NAN;
            const float mse = red[q + 1][0] / (3.f * B);
            out[SPNERF_LOSS_TERM_COLOR] = col; out[SPNERF_LOSS_TERM_LOGBETA] = lb;
            out[SPNERF_LOSS_TERM_SC2] = sc2; out[SPNERF_LOSS_TERM_SC3] = sc3;
            out[SPNERF_LOSS_TERM_DS] = dep; out[SPNERF_LOSS_TERM_SS] = ce;
            out[SPNERF_LOSS_TERM_MSE] = mse; out[SPNERF_LOSS_TERM_PSNR] = -10.f * log10f(mse);
            colour += ((col + lb) + sc2) + sc3;
            ds += dep;
            ss += ce;
        }
        if (a.o.flags & SPNERF_LOSS_DEPTH_TERM_ONLY) ds = 0.f;
        if (a.o.flags & SPNERF_LOSS_SEM_TERM_ONLY) ss = 0.f;
        a.result[1] = den;
        a.result[0] = (colour + ds) + ss;
    }
}

// the gradients of one pass of ray r; returns dL/db_r (β form), which d_beta needs from both passes
__device__ __forceinline__ float tl_grad_pass(const TlArgs& a, const spnerf_train_loss_pass& P, int64_t r, int lane) {
    const float g = *a.g, B = (float)a.o.n_rays;
    const bool beta = tl_beta(a), solar = tl_solar(a);
    const bool sem = tl_sem(a) && !(a.o.flags & SPNERF_LOSS_SEM_TERM_ONLY);
    const int form = (a.o.flags & SPNERF_LOSS_DEPTH_TERM_ONLY) ? SPNERF_LOSS_DEPTH_NONE : tl_form(a);
    const bool gnll = form == SPNERF_LOSS_DEPTH_SUBSET_GNLL;
    const int S = P.n_samples, C = a.o.n_classes;
    float sm = 0.f, db = 0.f;
    const TlRay o = tl_ray(a, P, r, lane, sem ? &sm : nullptr);
    if (lane < 3) {
        const float d = P.rgb[r * 3 + lane] - a.o.target[r * 3 + lane];
        P.d_rgb[r * 3 + lane] = beta ? g * (d / (o.b * o.b * 3.f * B)) : g * (2.f * d / (3.f * B));
    }
    if (beta) db = g * (-o.sq / (3.f * B * o.b * o.b * o.b) + 1.f / (2.f * B * o.b));
    if (solar) {
        const float k = g * (a.o.lambda_sc / 3.f) / B;
        for (int s = lane; s < S; s += 64) {
            const int64_t i = r * S + s;
            const float sun = P.sun_sc[i * (int64_t)P.ld_sun];
            P.d_sun[i] = k * (-2.f * (P.transparency_sc[i] - sun) - P.weights_sc[i]);
        }
    }
    float kw = 0.f;  // dL/d(Σ w (z - d)^2): the GNLL term through σ, 0 on a ray left out
    if (form) {
        const float k = g * (a.o.lambda_ds / 3.f) / B;
        float dd = 0.f;
        if (gnll) {
            const float d = P.depth[r];
            float m1 = 0.f;
            for (int s = lane; s < S; s += 64) m1 += P.weights[r * S + s] * (P.z_vals[r * S + s] - d);
            m1 = wave_sum(m1);
            if (o.apply) {
                // the clamp of σ is invisible to the gradient: d term / dσ at σc, dσ / dvar at σ
                const float sc = fmaxf(o.sigma, kNllEps);
                kw = k * (0.5f * (1.f / sc - o.diff * o.diff / (sc * sc))) * (0.5f / o.sigma);
                dd = k * (o.diff / sc) + kw * (-2.f * m1);
            }
        } else if (o.apply) {
            dd = k * 2.f * a.o.target_weight[r * (int64_t)a.o.ld_td] * o.diff;
        }
        if (lane == 0) P.d_depth[r] = dd;
    }
    if (beta || gnll) {
        const float d = gnll ? P.depth[r] : 0.f;
        for (int s = lane; s < S; s += 64) {
            const int64_t i = r * S + s;
            float gw = 0.f;
            if (beta) gw = db * a.o.beta[i * (int64_t)a.o.ld_beta];
            if (gnll && o.apply) {
                const float e = P.z_vals[i] - d;
                gw += kw * (e * e);
            }
            P.d_weights[i] = gw;
        }
    }
    if (sem && lane < C) {
        const int64_t lab = a.o.labels[r];
        const float den = a.result[1];
        float d = 0.f;
        if (o.bad != 0.f) d = NAN;
        else if (lab != -100 && den > 0.f) d = g * a.o.lambda_ss * (sm - (lane == lab ? 1.f : 0.f)) / den;
        P.d_logits[r * C + lane] = d;
    }
    return db;
}

__global__ __launch_bounds__(64 * kTlWaves) void k_tl_grad(TlArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kTlWaves + (threadIdx.x >> 6);
    if (r >= a.o.n_rays) return;  // wave-uniform
    const float db0 = tl_grad_pass(a, a.p[0], r, lane);
    const float db1 = a.npass > 1 ? tl_grad_pass(a, a.p[1], r, lane) : 0.f;
    if (tl_beta(a)) {
        const int S = a.p[0].n_samples;  // = the fine pass's under β
        for (int s = lane; s < S; s += 64) {
            const int64_t i = r * S + s;
            float gb = db0 * a.p[0].weights[i];
            if (a.npass > 1) gb += db1 * a.p[1].weights[i];
            a.o.d_beta[i] = gb;
        }
    }
}

}  // namespace spn

using namespace spn;

static int32_t tl_check(const spnerf_train_loss_opts* o, const spnerf_train_loss_pass* coarse,
                        const spnerf_train_loss_pass* fine, bool backward) {
    SPN_ARG(o && coarse, "train_loss: NULL opts / coarse pass");
    SPN_ARG(o->n_rays > 0, "train_loss: bad size B=%lld", (long long)o->n_rays);
    SPN_ARG(o->target, "train_loss: NULL target");
    const bool beta = (o->flags & SPNERF_LOSS_BETA) != 0, solar = o->lambda_sc > 0.f, sem = o->lambda_ss > 0.f;
    SPN_ARG((o->flags & ~(SPNERF_LOSS_BETA | SPNERF_LOSS_DEPTH_TERM_ONLY | SPNERF_LOSS_SEM_TERM_ONLY)) == 0,
            "train_loss: unknown flags %d", o->flags);
    SPN_ARG(o->depth_form >= SPNERF_LOSS_DEPTH_NONE && o->depth_form <= SPNERF_LOSS_DEPTH_ALL,
            "train_loss: unknown depth form %d", o->depth_form);
    const int form = o->lambda_ds > 0.f ? o->depth_form : SPNERF_LOSS_DEPTH_NONE;
    const bool subset = form == SPNERF_LOSS_DEPTH_SUBSET_MSE || form == SPNERF_LOSS_DEPTH_SUBSET_GNLL;
    const bool g_depth = form && !(o->flags & SPNERF_LOSS_DEPTH_TERM_ONLY);
    const bool g_sem = sem && !(o->flags & SPNERF_LOSS_SEM_TERM_ONLY);
    SPN_ARG(!beta || (o->beta && o->ld_beta > 0), "train_loss: NULL beta / bad stride");
    SPN_ARG(!beta || !fine || fine->n_samples == coarse->n_samples,
            "train_loss: the β form weights the fine colour by beta_coarse: %d fine samples, %d coarse",
            fine ? fine->n_samples : 0, coarse->n_samples);
    SPN_ARG(!form || (o->target_depth && o->ld_td > 0), "train_loss: NULL depth targets / bad stride");
    SPN_ARG(!subset || (o->valid && o->target_std), "train_loss: NULL valid / target_std (subset depth forms)");
    SPN_ARG(!form || form == SPNERF_LOSS_DEPTH_SUBSET_GNLL || o->target_weight, "train_loss: NULL target_weight");
    SPN_ARG(!sem || (o->labels && o->n_classes >= 1 && o->n_classes <= 64), "train_loss: NULL labels / classes outside [1, 64]");
    SPN_ARG(!sem || backward || (o->labels_global && o->n_global >= 0 && o->world >= 1), "train_loss: NULL labels_global / bad world");
    SPN_ARG(!backward || !beta || o->d_beta, "train_loss_backward: NULL d_beta");
    const spnerf_train_loss_pass* ps[2] = {coarse, fine};
    for (int p = 0; p < 2; ++p) {
        const spnerf_train_loss_pass* P = ps[p];
        if (!P) continue;
        const char* nm = p ? "fine" : "coarse";
        SPN_ARG(P->n_samples >= 1 && P->n_samples <= (1 << 20), "train_loss: %s pass: bad size S=%d", nm, P->n_samples);
        SPN_ARG(P->rgb, "train_loss: %s pass: NULL rgb", nm);
        SPN_ARG(!(beta || subset) || P->weights, "train_loss: %s pass: NULL weights", nm);
        SPN_ARG(!subset || P->z_vals, "train_loss: %s pass: NULL z_vals", nm);
        SPN_ARG(!form || P->depth, "train_loss: %s pass: NULL depth", nm);
        SPN_ARG(!solar || (P->sun_sc && P->transparency_sc && P->weights_sc && P->ld_sun > 0),
                "train_loss: %s pass: NULL solar inputs / bad stride", nm);
        SPN_ARG(!sem || P->sem_logits, "train_loss: %s pass: NULL sem_logits", nm);
        if (backward) {
            SPN_ARG(P->d_rgb && (!solar || P->d_sun) && (!g_depth || P->d_depth) && (!g_sem || P->d_logits) &&
                        (!(beta || (g_depth && form == SPNERF_LOSS_DEPTH_SUBSET_GNLL)) || P->d_weights),
                    "train_loss_backward: %s pass: NULL gradient pointer", nm);
        }
    }
    return SPNERF_OK;
}

static TlArgs tl_args(const spnerf_train_loss_opts* o, const spnerf_train_loss_pass* coarse,
                      const spnerf_train_loss_pass* fine) {
    TlArgs a{};
    a.o = *o;
    a.p[0] = *coarse;
    a.npass = 1;
    if (fine) {
        a.p[1] = *fine;
        a.npass = 2;
    }
    return a;
}

// a block of 4 waves per 4 rays, at most 4096 blocks (as loss.hip: a wave per ray, the per-ray
// terms are a chain of dependent loads and wave sums)
static int tl_blocks(int64_t n_rays) {
    return (int)std::min<int64_t>(std::max<int64_t>((n_rays + kTlWaves - 1) / kTlWaves, 1), 4096);
}

extern "C" int32_t spnerf_loss_abi_version(void) { return SPNERF_LOSS_ABI_VERSION; }

extern "C" int64_t spnerf_train_loss_workspace_bytes(int64_t n_rays) {
    if (n_rays < 0) return -1;
    return 2 * kTlParts * (int64_t)tl_blocks(n_rays) * (int64_t)sizeof(float);
}

extern "C" int32_t spnerf_train_loss_forward(const spnerf_train_loss_opts* opts, const spnerf_train_loss_pass* coarse,
                                             const spnerf_train_loss_pass* fine, void* workspace, float* result,
                                             void* stream) {
    SPN_TRY(tl_check(opts, coarse, fine, false));
    SPN_ARG(workspace && result, "train_loss: NULL workspace / result");
    TlArgs a = tl_args(opts, coarse, fine);
    a.nblocks = tl_blocks(opts->n_rays);
    a.partial = (float*)workspace;
    a.result = result;
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_loss", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_tl_rays, dim3(a.nblocks), dim3(64 * kTlWaves), 0, s, a);
    SPN_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_tl_final, dim3(1), dim3(256), 0, s, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

extern "C" int32_t spnerf_train_loss_backward(const spnerf_train_loss_opts* opts, const spnerf_train_loss_pass* coarse,
                                              const spnerf_train_loss_pass* fine, const float* result,
                                              const float* g_loss, void* stream) {
    SPN_TRY(tl_check(opts, coarse, fine, true));
    SPN_ARG(result && g_loss, "train_loss_backward: NULL result / g_loss");
    TlArgs a = tl_args(opts, coarse, fine);
    a.result = const_cast<float*>(result);
    a.g = g_loss;
    const int64_t nb = (opts->n_rays + kTlWaves - 1) / kTlWaves;
    SPN_ARG(nb <= 0x7fffffffLL, "train_loss_backward: too many rays B=%lld", (long long)opts->n_rays);
    hipStream_t s = (hipStream_t)stream;
    ProfScope prof("train_loss", s, 0.0, 0.0);
    hipLaunchKernelGGL(k_tl_grad, dim3((unsigned)nb), dim3(64 * kTlWaves), 0, s, a);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}
