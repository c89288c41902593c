// The backward pass's orchestration (spnerf_mlp_backward) and the deferred weight gradients over
// one or two passes' points (spnerf_mlp_trunk_wgrad).  Each weight gradient is stated once, below.
#include "grad_marks.h"
#include "mlp_ctx.h"
#include "point_kernels.h"

namespace spn {

int g_tile_rowsum = 1;  // 1 = per-ray dZ sums by 64-point tiles (fused into the dX chain); 0 = k_ray_rowsum16
int g_tn_split_tail = 1;  // option "tn_split_tail": see tn_grad
// option "tn_group": deferred weight-gradient GEMMs per launch (trunk_wgrad; 1 = one launch each).
// All 9 of a W = 512 model (sun_v_net.4 / .2, trunk layers 7 .. 1) in one launch: C4 at 512 rays
// 4.252 / 4.288 -> 4.033 / 4.036 ms, at 4 096 rays 26.57 / 26.49 -> 26.50 / 26.45 (same call; the
// slab reductions 0.35 -> 0.22 ms per step)
int g_tn_group = 9;
// option "tn_group_rounds": a group launch's blocks per CU (≤ kTnGroupRounds); 0 = 2 when a block
// would otherwise take ≥ 64 K points (C4 at 4 096 rays: 26.29 / 26.32 -> 26.25 / 26.26 ms), else 1
// (at 512 rays 2 rounds measured 3.976 / 3.977 against 3.963 / 3.964 ms)
int g_tn_group_rounds = 0;
int g_tn_group_last = 0;   // option "tn_group_last" (bench.py sets 2 when N > 1): the last group's size cap
// option "defer_heads": under deferred trunk weight gradients the output heads' G / Q weight
// gradients run in trunk_wgrad too (one GEMM over every pass's points, inside the group launch)
// — 1 always, 0 never, 2 (default) for passes of at most 2^18 points: C4 at 512 rays 3.970 / 3.973
// -> 3.926 / 3.917 ms, while at 4 096 rays the per-pass GEMMs overlapping the dX chain on the side
// stream are worth more (26.04 / 26.14 against 26.16 / 26.19 ms deferred; same call)
int g_defer_heads = 2;
int g_tn_k64_pair = 1;  // option "tn_k64_pair": the skip layer's PE tail and fc_net.0 in one narrow launch
int g_ray_tiles_pair = 1;  // option "ray_tiles_pair": the per-ray dZ sums of layer 0 and the skip layer in one launch

#ifndef SPN_DEFER_SUNV
#define SPN_DEFER_SUNV 1  // sun_v_net.2 / .4's weight gradients deferred with the trunk's (0: A/B builds)
#endif

namespace {
// each parameter's slot of the flat gradient
struct Grads {
    PIdx x;
    std::vector<PSpec> specs;
    float* grad;
    Grads(const Dims& d, float* g) : specs(param_specs(d, &x)), grad(g) {}
    float* operator()(int pi) const { return grad + specs[pi].off; }
    int ld(int pi) const { return (int)specs[pi].ld(); }
};
}  // namespace

// ---- the weight gradients, one GEMM (tn_grad) each: dW = dZᵀ · input over a pass's points; the
// backward and the ungrouped arms of trunk_wgrad issue the same calls (bitwise-equal gradients) ----

// Q's rows: sun_v_net.0, with every head rgb.0 and beta.0 too = dZ_Qᵀ · feat
template <typename T>
static int32_t q_wgrad(const Ctx& c, int mode, const Grads& gp, hipStream_t s) {
    const Dims& d = c.d;
    const PIdx& x = gp.x;
    const int W = d.W, H = d.H;
    std::vector<ReduceArgs> r{red(0, H, W, gp(x.s1W), gp.ld(x.s1W), gp(x.s1b))};
    if (mode == 0) {
        r.push_back(red(H, H, W, gp(x.r1W), gp.ld(x.r1W), gp(x.r1b)));
        if (d.beta) r.push_back(red(2 * H, H, W, gp(x.b1W), gp.ld(x.b1W), gp(x.b1b)));
    }
    return tn_grad<T>(c, Gemms<T>::buf(c, c.w.dZQ), d.NQ, mode == 0 ? d.NQ : H, Gemms<T>::buf(c, c.w.G), d.NG, nullptr, 0,
                      W, W, s, r);
}

// G's rows: feat, with every head of a semantic model its hidden layer too = dZ_Gᵀ · H_L
template <typename T>
static int32_t g_wgrad(const Ctx& c, int mode, const Grads& gp, hipStream_t s) {
    const Dims& d = c.d;
    const PIdx& x = gp.x;
    const int W = d.W, H = d.H;
    const bool sem = mode == 0 && d.sem;
    std::vector<ReduceArgs> r{red(0, W, W, gp(x.featW), W, gp(x.featb))};
    if (sem) r.push_back(red(W, H, W, gp(x.m1W), W, gp(x.m1b)));
    return tn_grad<T>(c, Gemms<T>::buf(c, c.w.dZG), d.NG, sem ? d.NG : W, Gemms<T>::buf(c, c.w.Hb[d.L - 1]), W, nullptr, 0,
                      W, W, s, r);
}

// sun_v_net.<layer> (4: dZ_S3ᵀ · S2; 2: dZ_S2ᵀ · Q[:, :H]), over c2's points too when given
template <typename T>
static int32_t sunv_wgrad(const Ctx& c, int layer, const Grads& gp, hipStream_t s, const Ctx* c2 = nullptr) {
    const PIdx& x = gp.x;
    const int H = c.d.H;
    const bool l4 = layer == 4;
    auto dz = [&](const Ctx& q) { return l4 ? q.w.dS3 : q.w.dS2; };
    auto in = [&](const Ctx& q) { return l4 ? q.w.S2 : q.w.Q; };
    TnSeg sg;
    if (c2) sg = {c2->hb(dz(*c2)), c2->hb(in(*c2)), nullptr, c2->w.P};
    return tn_grad<T>(c, Gemms<T>::buf(c, dz(c)), H, H, Gemms<T>::buf(c, in(c)), l4 ? H : c.d.NQ, nullptr, 0, H, H, s,
                      {red(0, H, H, gp(l4 ? x.s3W : x.s2W), H, gp(l4 ? x.s3b : x.s2b))}, false, c2 ? &sg : nullptr);
}

// trunk layer i = dZ_iᵀ · in (the skip layer: [in | PE rows]; layer 0: the PE rows); zin: `in` holds a saved Z
template <typename T>
static int32_t layer_wgrad(const Ctx& c, int i, const T* dZ, const T* in, bool zin, const Grads& gp, hipStream_t s,
                           const TnSeg* sg = nullptr) {
    const Dims& d = c.d;
    const PIdx& x = gp.x;
    const int W = d.W;
    const int kreal = i == 0 ? d.K0 : (i == d.skip ? W + d.K0 : W);
    const std::vector<ReduceArgs> r{red(0, W, kreal, gp(x.fcW[i]), gp.ld(x.fcW[i]), gp(x.fcb[i]))};
    if (i == d.skip) {
        const T* X0 = Gemms<T>::buf(c, std::is_same<T, bf16>::value ? c.w.X0b : c.w.X0);
        return tn_grad<T>(c, dZ, W, W, in, W, X0, d.K0p, W, W + d.K0p, s, r, zin, sg);
    }
    return tn_grad<T>(c, dZ, W, W, in, i == 0 ? d.K0p : W, nullptr, 0, c.k.Kp[i], c.k.Kp[i], s, r, zin, sg);
}

// Backward of the per-point network (steps 1-6): narrow heads, head / sun_v / feat / trunk
// weight gradients (split-P TN GEMMs + fixed-order slab reduction), dX GEMMs with the saved
// sin' as Dmul, and the per-ray sums R0 / R4 / RQ feeding the per-ray parameters.
template <typename T>
static int32_t backward_points(const Ctx& c, int mode, const float* packed, const float* d_out, int64_t n_rays,
                               const Grads& gp, hipStream_t s, hipStream_t s2, Side* sd) {
    using G = Gemms<T>;
    using NT = typename G::NT;
    constexpr bool BF = std::is_same<T, bf16>::value;
    const bool zs = BF && g_zsave;  // the forward saved Z for the trunk layers >= 1 (forward_gemms)
    const Dims& d = c.d;
    const PIdx& x = gp.x;
    const int64_t P = c.w.P;
    const int W = d.W, H = d.H, S = c.S;
    auto buf = [&](int64_t off) { return G::buf(c, off); };

    T* HL = buf(c.w.Hb[d.L - 1]);
    T* Gb = buf(c.w.G);
    T* Qb = buf(c.w.Q);
    T* dZG = buf(c.w.dZG);
    T* dZQ = buf(c.w.dZQ);
    T* dS3 = buf(c.w.dS3);
    T* dS2 = buf(c.w.dS2);
    float* hpre = c.at(c.w.hpre);

    // 1. narrow heads
    {
        HeadsBwdArgs<T> a{packed, d, d_out, c.at(c.w.hsave), buf(c.w.DQ), buf(c.w.DG), buf(c.w.DS3), hpre, dZQ, dZG, dS3,
                          P, mode, (!BF && (g_emu_bf16 & 2)) ? 1 : 0};
        SPN_TRY(heads_bwd(a, c.k, s));
    }
    // from here on: dX chain on s, weight gradients on s2 (each after a fork from s)
    SPN_TRY(stream_dep(sd, s, s2));
    // 2. narrow-head weights: reductions over points (one launch + one reduction launch)
    {
        SkinnyBatch sb(c);
        SPN_TRY(sb.add(P, hpre + 0, d.HP, 1, HL, W, W, gp(x.sigW), W, 0, gp(x.sigb), nullptr));
        SPN_TRY(sb.add(P, hpre + 4, d.HP, 1, buf(c.w.S3), H, H, gp(x.s4W), H, 0, gp(x.s4b), nullptr));
        if (mode == 0) {
            SPN_TRY(sb.add(P, hpre + 1, d.HP, 3, Qb + H, d.NQ, H, gp(x.r2W), H, 0, gp(x.r2b), nullptr));
            if (d.beta) SPN_TRY(sb.add(P, hpre + 5, d.HP, 1, Qb + 2 * H, d.NQ, H, gp(x.b2W), H, 0, gp(x.b2b), nullptr));
            if (d.sem) SPN_TRY(sb.add(P, hpre + 6, d.HP, d.C, Gb + W, d.NG, H, gp(x.m2W), H, 0, gp(x.m2b), nullptr));
        }
        SPN_TRY(sb.run(s2));
    }
    // 3 - 5 (their dX GEMMs): the training heads' fused dX chain (heads_dx_bf16.hip, option
    // fused_heads_bwd) — dS2, dZQ's sun half, dZG's feat half and dZ_{L-1} in ONE launch, bit for bit
    // the four GEMMs below; their weight gradients then follow on s2 as before.  It runs only where
    // the forward recorded D_{L-1} tile-ordered (the launch reads nothing else); the ×D GEMM of step
    // 5 refuses such a buffer (the option changed between the forward and its backward)
    const int NQ = mode == 0 ? d.NQ : H;
    const int NG = mode == 0 ? d.NG : W;
    bool hdx = false;
    if constexpr (BF) {
        HeadsDxArgs h;
        h.dS3 = dS3; h.DS2 = buf(c.w.DS2); h.DQ = buf(c.w.DQ); h.DL = buf(c.w.Db[d.L - 1]);
        h.dS2 = dS2; h.dZQ = dZQ; h.dZG = dZG; h.dZL = buf(c.w.dZa);
        h.hpre = hpre; h.wsig = c.pk(c.k.wsig); h.packed16 = c.pk16(0);
        h.Bs3 = c.k.Bs3_16; h.Bs2 = c.k.Bs2_16; h.BQ = c.k.BQ16; h.BG = c.k.BG16;
        h.P = P; h.ldQ = d.NQ; h.ldG = d.NG; h.HP = d.HP; h.kQ = d.NQ; h.kG = d.NG;
        h.mode = mode; h.sem = d.sem ? 1 : 0;
        h.dl_tiled = (dtile_get(c.ws) >> (d.L - 1)) & 1;
        hdx = g_fused_heads_bwd && h.dl_tiled && heads_dx_shape(c, mode) && heads_dx_bf16_ok(h);
        if (hdx) {
            const double flop = 2.0 * P * ((double)H * H * 2 + (double)NQ * W + (double)NG * W);
            const double in = 2.0 * P * (3.0 * H + (mode == 0 ? H : 0) + (mode == 0 && d.sem ? H : 0) + W) + 4.0 * P;
            const double out = 2.0 * P * (2.0 * H + 2.0 * W);
            SPN_TRY(heads_dx_bf16(h, s, flop, in + out));
            SPN_TRY(stream_dep(sd, s, s2));
        }
    }
    // 3. sun_v_net chain: dZ_S2 = (dZ_S3 · Ws3) ⊙ DS2 ; dZ_S1 = (dZ_S2 · Ws2) ⊙ DQ[:, :H]
    {
        // deferred (SPNERF_MLP_DEFER_TRUNK_WGRAD): sun_v_net.4 / .2's weight gradients run in
        // spnerf_mlp_trunk_wgrad too — every pass of a render has them
        const bool sunv_now = !c.defer || !SPN_DEFER_SUNV;
        if (sunv_now) SPN_TRY(sunv_wgrad<T>(c, 4, gp, s2));
        NT g;
        g.A = dS3; g.lda = H; g.K1 = H; g.B = G::w(c, c.k.Ws3T, c.k.Ws3T16); g.ldb = H; g.C = dS2; g.ldc = H;
        g.M = (int)P; g.N = H; g.K = H; g.Dmul = buf(c.w.DS2); g.ld_dmul = H;
        if (!hdx) {
            SPN_TRY(G::nt(g, s));
            SPN_TRY(stream_dep(sd, s, s2));
        }
        if (sunv_now) SPN_TRY(sunv_wgrad<T>(c, 2, gp, s2));
        NT g2 = g;
        g2.A = dS2; g2.B = G::w(c, c.k.Ws2T, c.k.Ws2T16); g2.C = dZQ; g2.ldc = d.NQ; g2.Dmul = buf(c.w.DQ); g2.ld_dmul = d.NQ;
        if (!hdx) {
            SPN_TRY(G::nt(g2, s));
            SPN_TRY(stream_dep(sd, s, s2));
        }
    }
    // 4. feat: dF = dZ_Q · WQ → dZG[:, :W];  dWQ = dZ_Q^T · feat
    // deferred (SPNERF_MLP_DEFER_TRUNK_WGRAD, option defer_heads): the G / Q weight gradients run in
    // spnerf_mlp_trunk_wgrad, over every pass's points in one GEMM each
    const bool heads_def = c.defer && defer_heads_for(P);
    {
        if (!heads_def) SPN_TRY(q_wgrad<T>(c, mode, gp, s2));
        // per-ray sums of dZ_Q feed the sun-direction / time-embedding columns (sun_v.0's and β.0's
        // blocks of RQ; rgb.0 has no per-ray input, so its block is not summed without β)
        SPN_TRY(ray_rowsum(dZQ, d.NQ, 0, d.beta ? NQ : H, S, n_rays, c.at(c.w.RQ), d.NQ, s2));
        NT g;
        g.A = dZQ; g.lda = d.NQ; g.K1 = NQ; g.B = G::w(c, c.k.WQT, c.k.WQT16); g.ldb = d.NQ; g.C = dZG; g.ldc = d.NG;
        g.M = (int)P; g.N = W; g.K = NQ;
        if (!hdx) {
            SPN_TRY(G::nt(g, s));
            SPN_TRY(stream_dep(sd, s, s2));
        }
    }
    // 5. H_L: dH_L = dZ_G · WG + dσ ⊗ w_σ ;  dZ_{L-1} = dH_L ⊙ D_L ;  dWG = dZ_G^T · H_L
    // trunk dZ buffers in rotation: the dX GEMM of layer i writes the buffer whose dZ_{i+2} the
    // side stream's weight gradient of layer i+2 read (it waits for that, not for layer i+1's)
    T* dzb[3] = {buf(c.w.dZa), buf(c.w.dZb), buf(c.w.dZc)};
    std::vector<hipEvent_t> tn_done(d.L + 2, nullptr);
    int cur = 0;
    T* dZ = dzb[cur];
    {
        if (!heads_def) SPN_TRY(g_wgrad<T>(c, mode, gp, s2));
        // every output head's gradient is final (spnerf_grad_marks) — unless sun_v_net.2 / .4's
        // are deferred: then spnerf_mlp_trunk_wgrad records the mark once they are
        if (!c.defer || (!SPN_DEFER_SUNV && !heads_def)) SPN_TRY(grad_mark(0, s2));
        NT g;
        g.A = dZG; g.lda = d.NG; g.K1 = NG; g.B = G::w(c, c.k.WGT, c.k.WGT16); g.ldb = d.NG; g.C = dZ; g.ldc = W;
        g.M = (int)P; g.N = W; g.K = NG;
        g.r1_a = hpre; g.r1_lda = d.HP; g.r1_v = c.pk(c.k.wsig);
        g.Dmul = buf(c.w.Db[d.L - 1]); g.ld_dmul = W;
        if constexpr (BF) g.dmul_z = zs ? 1 : 0;
        if (!hdx) {
            if constexpr (BF)
                SPN_ARG(((dtile_get(c.ws) >> (d.L - 1)) & 1) == 0, "backward: D_{L-1} is tile-ordered; the xD head GEMM reads row-major D");
            g_heads_bwd_path |= 2;
            SPN_TRY(G::nt(g, s));
            SPN_TRY(stream_dep(sd, s, s2));
        }
    }
    // 6. trunk, top to bottom
    const T* X0 = BF ? buf(c.w.X0b) : buf(c.w.X0);
    // the per-ray sums of dZ_0 / dZ_skip (semantic columns) by 64-point tiles: the fused dX chain
    // forms the tiles' column sums from its LDS image (no re-read of dZ), the layer-by-layer chain
    // from HBM in the same order (bit-identical), then one launch adds each ray's tiles
    const bool tsum = BF && g_tile_rowsum && d.sem && W == 512 && S % 64 == 0;
    // both layers' tile sums written by the fused chain: one launch adds both, after the chain
    bool pair_tiles = false;
    bool parts_in_bwd = false;  // the fused chain wrote the tile sums
    // layer i's weight gradient (and the per-ray sums of its dZ at layer 0 / the skip layer)
    auto layer_grads = [&](int i, const T* dZi) -> int32_t {
        // dZi holds dL/d(pre-activation of layer i).  The input of layer i >= 2 is saved as Z
        // (option zsave): staged as sin(Z) by the TN
        const bool zin = zs && i >= 2;
        const T* In = i == 0 ? X0 : buf(zin ? c.w.Db[i - 1] : c.w.Hb[i - 1]);
        // deferred: spnerf_mlp_trunk_wgrad computes it later, over this and other passes' points
        if (!c.defer) SPN_TRY(layer_wgrad<T>(c, i, dZi, In, zin, gp, s2));
        if (d.sem && (i == 0 || i == d.skip) && !pair_tiles) {
            float* R = c.at(i == 0 ? c.w.R0 : c.w.R4);
            if (tsum)  // (bf16 only)
                SPN_TRY(ray_tiles_sum(parts_in_bwd ? nullptr : reinterpret_cast<const bf16*>(dZi),
                                      c.at(i == 0 ? c.w.Rp0 : c.w.Rp4), P, S, n_rays, R, s2));
            else
                SPN_TRY(ray_rowsum(dZi, W, 0, W, S, n_rays, R, W, s2));
        }
        // a mark is recorded only once its gradients are final: deferred layers get theirs from
        // spnerf_mlp_trunk_wgrad
        return c.defer ? SPNERF_OK : grad_mark(1 + (d.L - 1 - i), s2);
    };
    if (BF && !zs && g_fused_bwd && !c.k.Wb16.empty() && c.k.Wb16[1] >= 0) {
        // the whole dX chain in one launch (k_trunk_bwd_bf16): dZ_{i-1} overwrites D_{i-1} in
        // place (the workspace serves one backward: spnerf_mlp_backward consumes it), then the
        // weight gradients of every layer
        TrunkBwdArgs a;
        a.dZtop = reinterpret_cast<const bf16*>(dZ);
        for (int i = 1; i < d.L; ++i) {
            a.Wb[i] = c.pk16(c.k.Wb16[i]);
            a.D[i - 1] = c.hb(c.w.Db[i - 1]);
            a.dZ[i - 1] = c.hb(c.w.Db[i - 1]);
        }
        a.P = P; a.L = d.L;
        a.dtile = dtile_get(c.ws) & ((1 << (d.L - 1)) - 1);  // as the forward wrote each layer's D (D_{L-1}: the heads')
        if (tsum && d.skip > 0 && d.skip < d.L) {
            a.Rsum[0] = c.at(c.w.Rp0); a.rs_layer[0] = 0;
            a.Rsum[1] = c.at(c.w.Rp4); a.rs_layer[1] = d.skip;
            parts_in_bwd = true;
        }
        // algorithmic HBM bytes: dZ_{L-1} in, per layer D_{i-1} in and dZ_{i-1} out
        SPN_TRY(trunk_bwd_bf16(a, s, 2.0 * P * W * W * (d.L - 1), 2.0 * P * W * (1.0 + 2.0 * (d.L - 1))));
        SPN_TRY(stream_dep(sd, s, s2));
        pair_tiles = parts_in_bwd && g_ray_tiles_pair;
        if (pair_tiles)
            SPN_TRY(ray_tiles_sum_pair(c.at(c.w.Rp0), c.at(c.w.R0), c.at(c.w.Rp4), c.at(c.w.R4), P, S, n_rays, s2));
        for (int i = d.L - 1; i >= 0; --i) SPN_TRY(layer_grads(i, i == d.L - 1 ? dZ : buf(c.w.Db[i])));
        return SPNERF_OK;
    }
    if constexpr (BF) SPN_ARG(dtile_get(c.ws) == 0, "backward: the forward saved tile-ordered D (mask %x), which the layer-by-layer "
                                                    "dX chain cannot read (set fused_bwd before the forward)", dtile_get(c.ws));
    for (int i = d.L - 1; i >= 0; --i) {
        // dZ (buffer cur) holds dL/d(pre-activation of layer i); the side stream has it
        SPN_TRY(layer_grads(i, dZ));
        if (sd && s2 != s) {   // this layer's reads of buffer `cur` are issued on s2
            tn_done[i] = sd->ev[sd->next];
            sd->next = (sd->next + 1) % 64;
            SPN_HIP(hipEventRecord(tn_done[i], s2));
        }
        if (i > 0) {
            const int nxt = (cur + 1) % 3;
            // buffer nxt last held dZ_{i+2}: its weight gradient (layer i+2) must be done
            if (i + 2 <= d.L - 1 && tn_done[i + 2]) SPN_HIP(hipStreamWaitEvent(s, tn_done[i + 2], 0));
            NT g;
            g.A = dZ; g.lda = W; g.K1 = W; g.B = G::w(c, c.k.WTt[i], BF ? c.k.WTt16[i] : -1); g.ldb = W; g.C = dzb[nxt];
            g.ldc = W; g.M = (int)P; g.N = W; g.K = W; g.Dmul = buf(c.w.Db[i - 1]); g.ld_dmul = W;
            if constexpr (BF) g.dmul_z = zs && i >= 2;   // Db[i - 1] holds Z for layers >= 1
            SPN_TRY(G::nt(g, s));
            SPN_TRY(stream_dep(sd, s, s2));
            cur = nxt;
            dZ = dzb[cur];
        }
    }
    return SPNERF_OK;
}

// The trunk layers' weight gradients (fc_net.2i weight / bias, without the per-ray semantic
// columns, which each backward adds itself) and sun_v_net.2 / .4's over the points of up to two
// deferred backwards' workspaces per GEMM, added into grad (spnerf_mlp_trunk_wgrad).
static int32_t trunk_wgrad(const Dims& d, int n_seg, void* const* wss, const int64_t* n_rays, const int32_t* S,
                           const int32_t* flags, float* grad, hipStream_t s) {
    const Grads gp(d, grad);
    const PIdx& x = gp.x;
    auto ld = [&](int pi) { return gp.ld(pi); };
    const int W = d.W;
    for (int j = 0; j < n_seg; j += 2) {
        auto ctx = [&](int k) {
            const int fl = flags[k] & ~(SPNERF_MLP_ACCUMULATE | SPNERF_MLP_DEFER_TRUNK_WGRAD);
            Ctx c{d, packed_layout(d), ws_layout(d, n_rays[k], S[k], fl), nullptr, static_cast<float*>(wss[k]), S[k]};
            c.acc = 1;
            return c;
        };
        const Ctx c = ctx(j);
        SPN_ARG(wss[j] && (flags[j] & SPNERF_MLP_SAVE) && trunk_wgrad_ok(c), "spnerf_mlp_trunk_wgrad: bad segment");
        const bool two = j + 1 < n_seg;
        Ctx c2 = two ? ctx(j + 1) : c;
        if (two) SPN_ARG(wss[j + 1] && (flags[j + 1] & SPNERF_MLP_SAVE), "spnerf_mlp_trunk_wgrad: bad segment");
        if (c.w.P + (two ? c2.w.P : 0) == 0) continue;
        auto dzl = [&](const Ctx& q, int i) { return q.hb(i == d.L - 1 ? q.w.dZa : q.w.Db[i]); };
        const int64_t Pt = c.w.P + (two ? c2.w.P : 0);
        const int H = d.H;
        // option tn_group (> 1): the output heads' G / Q weight gradients (defer_heads), sun_v_net.4
        // / .2 and the trunk layers L-1 .. 1 (the skip layer's H part; its PE tail on the narrow
        // kernel) run g_tn_group GEMMs per launch of the DMA kernel, splits in proportion to each
        // GEMM's points (equal points per block), the slab shared out among them
        struct Item {
            TN16Args t;
            ReduceArgs r[3];
            int nr, mark, layer;
        };
        std::vector<Item> items;
        bool sunv_grouped = false, heads_grouped = false, grouped[16] = {};
        const int mode_a = mode_of(flags[j]);
        const int mode_b = two ? mode_of(flags[j + 1]) : -1;
        // segment a (c) and / or b (c2) of one GEMM: A / B pointers of each, nullptr = not in it
        struct Seg2 {
            const bf16 *A1, *B1;
            int64_t P1;
            const bf16 *A2, *B2;
            int64_t P2;
        };
        auto seg2 = [&](const bf16* Aa, const bf16* Ba, bool in_a, const bf16* Ab, const bf16* Bb, bool in_b) {
            Seg2 g{nullptr, nullptr, 0, nullptr, nullptr, 0};
            if (in_a) g = {Aa, Ba, c.w.P, nullptr, nullptr, 0};
            if (in_b) {
                if (in_a) g.A2 = Ab, g.B2 = Bb, g.P2 = c2.w.P;
                else g = {Ab, Bb, c2.w.P, nullptr, nullptr, 0};
            }
            return g;
        };
        auto item_ok = [&](const Seg2& g, int N, int K) {
            return g.P1 + g.P2 > 0 && tn_group_ok((int)(g.P1 + g.P2), N, K) && (g.P2 == 0 || g.P1 % 32 == 0);
        };
        auto add = [&](const Seg2& g, int lda, int N, int ldb, int K, const std::vector<ReduceArgs>& reds, int mark,
                       int layer) {
            Item it;
            it.t.A = g.A1; it.t.lda = lda; it.t.B = g.B1; it.t.ldb = ldb; it.t.K1 = K;
            it.t.P = (int)(g.P1 + g.P2); it.t.N = N; it.t.K = K;
            it.t.ld_slab = K; it.t.slab_stride = (int64_t)N * K;
            if (g.P2) second_segment(it.t, g.P1, g.A2, g.B2);
            it.nr = 0;
            for (const ReduceArgs& r : reds) it.r[it.nr++] = r;
            it.mark = mark;
            it.layer = layer;
            items.push_back(it);
        };
        const bool grp = g_tn_group > 1;
        const bool hda = defer_heads_for(c.w.P), hdb = two && defer_heads_for(c2.w.P), hd = hda || hdb;
        if (grp && hda && (!two || hdb)) {
            // feat (+ the semantic hidden rows) = dZ_Gᵀ · H_L; sun_v_net.0 (+ rgb / beta rows) = dZ_Qᵀ · G[:, :W]
            const bool m0a = mode_a == 0, m0b = mode_b == 0;
            const Seg2 gf = seg2(c.hb(c.w.dZG), c.hb(c.w.Hb[d.L - 1]), true, c2.hb(c2.w.dZG), c2.hb(c2.w.Hb[d.L - 1]), two);
            const Seg2 gm = seg2(c.hb(c.w.dZG) + W, c.hb(c.w.Hb[d.L - 1]), m0a, c2.hb(c2.w.dZG) + W, c2.hb(c2.w.Hb[d.L - 1]),
                                 m0b);
            const Seg2 qs = seg2(c.hb(c.w.dZQ), c.hb(c.w.G), true, c2.hb(c2.w.dZQ), c2.hb(c2.w.G), two);
            const Seg2 qr = seg2(c.hb(c.w.dZQ) + H, c.hb(c.w.G), m0a, c2.hb(c2.w.dZQ) + H, c2.hb(c2.w.G), m0b);
            const int nqr = d.beta ? 2 * H : H;
            const bool any0 = m0a || m0b;
            if (item_ok(gf, W, W) && item_ok(qs, H, W) && (!any0 || ((!d.sem || item_ok(gm, H, W)) && item_ok(qr, nqr, W)))) {
                add(gf, d.NG, W, W, W, {red(0, W, W, gp(x.featW), W, gp(x.featb))}, 0, -1);
                add(qs, d.NQ, H, d.NG, W, {red(0, H, W, gp(x.s1W), ld(x.s1W), gp(x.s1b))}, 0, -1);
                if (any0) {
                    if (d.sem) add(gm, d.NG, H, W, W, {red(0, H, W, gp(x.m1W), W, gp(x.m1b))}, 0, -1);
                    std::vector<ReduceArgs> rq{red(0, H, W, gp(x.r1W), ld(x.r1W), gp(x.r1b))};
                    if (d.beta) rq.push_back(red(H, H, W, gp(x.b1W), ld(x.b1W), gp(x.b1b)));
                    add(qr, d.NQ, nqr, d.NG, W, rq, 0, -1);
                }
                heads_grouped = true;
            }
        }
        if (grp && SPN_DEFER_SUNV) {
            const Seg2 g3 = seg2(c.hb(c.w.dS3), c.hb(c.w.S2), true, c2.hb(c2.w.dS3), c2.hb(c2.w.S2), two);
            const Seg2 g2 = seg2(c.hb(c.w.dS2), c.hb(c.w.Q), true, c2.hb(c2.w.dS2), c2.hb(c2.w.Q), two);
            if (item_ok(g3, H, H) && item_ok(g2, H, H)) {
                add(g3, H, H, H, H, {red(0, H, H, gp(x.s3W), H, gp(x.s3b))}, 0, -1);
                add(g2, H, H, d.NQ, H, {red(0, H, H, gp(x.s2W), H, gp(x.s2b))}, 0, -1);
                sunv_grouped = true;
            }
        }
        if (grp)
            for (int i = d.L - 1; i >= 1; --i) {
                const Seg2 g = seg2(dzl(c, i), c.hb(c.w.Hb[i - 1]), true, dzl(c2, i), c2.hb(c2.w.Hb[i - 1]), two);
                if ((c.k.Kp[i] == W || i == d.skip) && i < 16 && item_ok(g, W, W)) {
                    add(g, W, W, W, W, {red(0, W, W, gp(x.fcW[i]), ld(x.fcW[i]), gp(x.fcb[i]))}, 1 + (d.L - 1 - i), i);
                    grouped[i] = true;
                }
            }
        // the skip layer's PE tail and fc_net.0 (both N = W, K = K0p over the PE rows X0b) share one
        // launch of the narrow kernel at the end, with half the splits each
        // (not with tn_group_last: the skip layer's tail then runs right after its group, so its mark
        // fires a launch earlier instead of with fc_net.0's at the very end)
        const bool pair_tail = g_tn_k64_pair && g_tn_group_last == 0 && tn_k64_ok(W, d.K0p) && d.skip >= 1 && d.skip < 16 &&
                               grouped[d.skip] && c.k.Kp[0] == d.K0p;
        bool tail_pending = false;
        for (size_t g0 = 0; g0 < items.size();) {
            size_t g1 = std::min(items.size(), g0 + (size_t)std::min(g_tn_group, kTnGroup));
            // option tn_group_last: the final group at most that many GEMMs (the ones before it one
            // launch more), so the marks of all but the lowest layers fire a group earlier and their
            // all-reduce overlaps the last group (data parallelism: a smaller exposed last bucket)
            if (g_tn_group_last > 0 && g1 == items.size() && g1 - g0 > (size_t)g_tn_group_last)
                g1 = items.size() - (size_t)g_tn_group_last;
            // one split count per point: GEMM q takes sp · P_q / Pt splits, rounds x the CUs' worth
            // of blocks, within the workspace's slab capacity
            double tiles = 0, nk = 0, nn = 0;
            for (size_t q = g0; q < g1; ++q) {
                const double w = (double)items[q].t.P / (double)Pt;
                tiles += w * tn_tiles_bf16(items[q].t.N, items[q].t.K);
                nk += w * items[q].t.N * items[q].t.K;
                nn += w * items[q].t.N;
            }
            const int64_t sp1 = std::max<int64_t>(1, (int64_t)(split_cus() / tiles));
            const int rounds = g_tn_group_rounds > 0 ? std::min(g_tn_group_rounds, kTnGroupRounds)
                                                     : (Pt / sp1 >= 65536 ? 2 : 1);
            const int64_t sp = std::max<int64_t>(1, std::min({(int64_t)(rounds * split_cus() / tiles), (int64_t)cdiv(Pt, g_tn16_min_points),
                                                             (int64_t)(c.w.slab_n / nk), (int64_t)(c.w.slab_b_n / nn)}));
            TN16Args t[kTnGroup];
            int spl[kTnGroup];
            std::vector<ReduceArgs> r;
            int64_t off = 0, off_b = 0;
            bool skip_in = false, mark0 = false;
            for (size_t q = g0; q < g1; ++q) {
                Item& it = items[q];
                const int sq = (int)std::max<int64_t>(1, sp * it.t.P / Pt);
                it.t.slab = c.at(c.w.slab) + off;
                it.t.slab_b = c.at(c.w.slab_b) + off_b;
                off += sq * it.t.slab_stride;
                off_b += (int64_t)sq * it.t.N;
                for (int k = 0; k < it.nr; ++k) {
                    bind_slab(it.r[k], it.t.slab, it.t.N, it.t.K, sq, it.t.slab_b, c.acc);
                    r.push_back(it.r[k]);
                }
                t[q - g0] = it.t;
                spl[q - g0] = sq;
                skip_in = skip_in || it.layer == d.skip;
                mark0 = mark0 || it.layer < 0;
            }
            SPN_ARG(off <= c.w.slab_n && off_b <= c.w.slab_b_n, "trunk_wgrad: slab capacity for a group of %d GEMMs",
                    (int)(g1 - g0));
            SPN_TRY(gemm_tn_bf16_group(t, (int)(g1 - g0), spl, s));
            for (size_t q = 0; q < r.size(); q += kReduceMulti)
                SPN_TRY(reduce_slabs_multi(r.data() + q, (int)std::min<size_t>(kReduceMulti, r.size() - q), s));
            if (skip_in && pair_tail) {
                tail_pending = true;   // with fc_net.0's, one launch of the narrow kernel (below)
            } else if (skip_in) {  // the skip layer's PE columns: N = W, K = K0p (the narrow kernel)
                const int l = d.skip;
                const TnSeg st{dzl(c2, l), c2.hb(c2.w.X0b), nullptr, c2.w.P};
                SPN_TRY(tn_grad<bf16>(c, dzl(c, l), W, W, c.hb(c.w.X0b), d.K0p, nullptr, 0, d.K0p, d.K0p, s,
                                      {red(0, W, d.K0, gp(x.fcW[l]) + W, ld(x.fcW[l]), nullptr)}, false, two ? &st : nullptr));
            }
            // mark 0 (the output heads) once the last group holding one of them is done
            bool later0 = false;
            for (size_t q = g1; q < items.size(); ++q) later0 = later0 || items[q].layer < 0;
            if (mark0 && !later0 && (sunv_grouped || !SPN_DEFER_SUNV) && (heads_grouped || !hd))
                SPN_TRY(grad_mark(0, s));
            for (size_t q = g0; q < g1; ++q)
                if (items[q].layer >= 0 && !(tail_pending && items[q].layer == d.skip)) SPN_TRY(grad_mark(items[q].mark, s));
            g0 = g1;
        }
        // the heads' G / Q weight gradients not grouped: per segment, as the backward computes them
        if (hd && !heads_grouped) {
            for (int k = 0; k < (two ? 2 : 1); ++k) {
                const Ctx& q = k ? c2 : c;
                if (!(k ? hdb : hda)) continue;
                SPN_TRY(q_wgrad<bf16>(q, k ? mode_b : mode_a, gp, s));
                SPN_TRY(g_wgrad<bf16>(q, k ? mode_b : mode_a, gp, s));
            }
            if (sunv_grouped || !SPN_DEFER_SUNV) SPN_TRY(grad_mark(0, s));
        }
        // sun_v_net.4 and .2 (sun-visibility head, in every pass): dW = dZᵀ · input over all points
        if (SPN_DEFER_SUNV && !sunv_grouped) {
            SPN_TRY(sunv_wgrad<bf16>(c, 4, gp, s, two ? &c2 : nullptr));
            SPN_TRY(sunv_wgrad<bf16>(c, 2, gp, s, two ? &c2 : nullptr));
            SPN_TRY(grad_mark(0, s));   // the heads' gradients are final again
        }
        for (int i = d.L - 1; i >= 0; --i) {
            if (i < 16 && grouped[i]) continue;
            if (i == 0 && tail_pending) {
                const int l = d.skip;
                TN16Args t[2];
                int spl[2];
                ReduceArgs r[2];
                const int sp = std::max(1, tn_splits_bf16((int)Pt, W, d.K0p) / 2);
                for (int q = 0; q < 2; ++q) {
                    TN16Args& a = t[q];
                    const int li = q ? l : 0;
                    a.A = dzl(c, li); a.lda = W; a.B = c.hb(c.w.X0b); a.ldb = d.K0p; a.K1 = d.K0p;
                    a.P = (int)Pt; a.N = W; a.K = d.K0p;
                    a.slab = c.at(c.w.slab) + (int64_t)q * sp * W * d.K0p; a.ld_slab = d.K0p; a.slab_stride = (int64_t)W * d.K0p;
                    a.slab_b = q ? nullptr : c.at(c.w.slab_b);
                    if (two) second_segment(a, c.w.P, dzl(c2, li), c2.hb(c2.w.X0b));
                    spl[q] = sp;
                    r[q] = q ? red(0, W, d.K0, gp(x.fcW[l]) + W, ld(x.fcW[l]), nullptr)
                             : red(0, W, d.K0, gp(x.fcW[0]), ld(x.fcW[0]), gp(x.fcb[0]));
                    bind_slab(r[q], a.slab, W, d.K0p, sp, a.slab_b, c.acc);
                }
                SPN_ARG(2 * sp * (int64_t)W * d.K0p <= c.w.slab_n && sp * (int64_t)W <= c.w.slab_b_n, "trunk_wgrad: slab capacity");
                SPN_TRY(gemm_tn_bf16_k64_group(t, 2, spl, s));
                SPN_TRY(reduce_slabs_multi(r, 2, s));
                SPN_TRY(grad_mark(1 + (d.L - 1 - l), s));
                SPN_TRY(grad_mark(d.L, s));
                continue;
            }
            auto in = [&](const Ctx& q) { return q.hb(i == 0 ? q.w.X0b : q.w.Hb[i - 1]); };
            const TnSeg sg{dzl(c2, i), in(c2), c2.hb(c2.w.X0b), c2.w.P};
            SPN_TRY(layer_wgrad<bf16>(c, i, dzl(c, i), in(c), false, gp, s, two ? &sg : nullptr));
            SPN_TRY(grad_mark(1 + (d.L - 1 - i), s));
        }
    }
    return grad_mark(d.L + 1, s);
}

static int32_t mlp_backward(const Dims& d, const float* packed, const float* rays, int rs, int64_t n_rays, int S,
                            const int64_t* labels, const float* temb, int flags, float* ws, const float* d_out,
                            float* grad, float* grad_t, hipStream_t s) {
    SPN_ARG(flags & SPNERF_MLP_SAVE, "backward needs a workspace written with SPNERF_MLP_SAVE");
    SPN_ARG(!(flags & SPNERF_MLP_SIGMA_ONLY), "backward of a sigma-only pass is not supported");
    Ctx c{d, packed_layout(d), ws_layout(d, n_rays, S, flags & ~(SPNERF_MLP_ACCUMULATE | SPNERF_MLP_DEFER_TRUNK_WGRAD)),
          packed, ws, S};
    c.acc = (flags & SPNERF_MLP_ACCUMULATE) ? 1 : 0;
    c.defer = (flags & SPNERF_MLP_DEFER_TRUNK_WGRAD) ? 1 : 0;
    SPN_ARG(!c.defer || trunk_wgrad_ok(c), "backward: SPNERF_MLP_DEFER_TRUNK_WGRAD needs the bf16 MLP's fused dX chain "
                                           "(spnerf_mlp_trunk_wgrad with n_seg = 0 tells)");
    const int mode = mode_of(flags);
    const int64_t P = n_rays * S;
    const int W = d.W, H = d.H;
    const Grads gp(d, grad);
    const PIdx& x = gp.x;
    auto ld = [&](int pi) { return gp.ld(pi); };
    const int64_t total = gp.specs.back().off + gp.specs.back().numel();
    if (!c.acc) SPN_TRY(zero_fill(grad, total, s));
    if (grad_t && d.beta) SPN_TRY(zero_fill(grad_t, n_rays * d.td, s));
    if (P == 0) return SPNERF_OK;
    Side* sd = g_bwd_streams >= 2 ? side_stream() : nullptr;
    hipStream_t s2 = sd ? sd->s : s;
    if (d.bf) SPN_TRY(backward_points<bf16>(c, mode, packed, d_out, n_rays, gp, s, s2, sd));
    else SPN_TRY(backward_points<float>(c, mode, packed, d_out, n_rays, gp, s, s2, sd));
    SPN_TRY(stream_dep(sd, s, s2));   // step 7 reads d_out and the workspace written on s
    const hipStream_t s_main = s;
    s = s2;                           // step 7 (per-ray parameters) runs on the side stream
    // 7. per-ray parameters: sun-direction columns, t columns, sky MLP, semantic embedding
    {
        const int sky_on = mode == 0;
        RayBwdArgs a{packed, c.k, d, c.at(c.w.sky), c.at(c.w.skyh), c.at(c.w.R0), c.at(c.w.R4),
                     c.at(c.w.RQ), d_out, (int)d.NO, (int)S, labels, c.at(c.w.skyd), c.at(c.w.skydh), c.at(c.w.gemb), c.at(c.w.embr), grad_t,
                     d.sem ? 1 : 0, (d.beta && mode == 0) ? 1 : 0, sky_on};
        SPN_TRY(ray_bwd(a, n_rays, s));
        const float* sun = rays + 8;
        const int64_t B = n_rays;
        SkinnyBatch sb(c);
        // sun_v_net.0 sun-direction columns: dW[n][W+j] = Σ_ray RQ[ray][n] sun[ray][j]
        SPN_TRY(sb.add(B, sun, rs, 3, c.at(c.w.RQ), d.NQ, H, gp(x.s1W) + W, ld(x.s1W), 1, nullptr, nullptr));
        if (sky_on) {
            SPN_TRY(sb.add(B, sun, rs, 3, c.at(c.w.skydh), H, H, gp(x.k1W), 3, 1, nullptr, gp(x.k1b)));
            SPN_TRY(sb.add(B, c.at(c.w.skyd), 4, 3, c.at(c.w.skyh), H, H, gp(x.k2W), H, 0, gp(x.k2b), nullptr));
        }
        if (d.beta && mode == 0) {
            if (d.td <= 8)
                SPN_TRY(sb.add(B, temb, d.td, d.td, c.at(c.w.RQ) + 2 * H, d.NQ, H, gp(x.b1W) + W, ld(x.b1W), 1, nullptr,
                               nullptr));
            else
                SPN_TRY(skinny(c, B, temb, d.td, d.td, c.at(c.w.RQ) + 2 * H, d.NQ, H, gp(x.b1W) + W, ld(x.b1W), 1,
                               nullptr, nullptr, s));
        }
        if (d.sem) {
            SPN_TRY(sb.add(B, c.at(c.w.embr), d.sd, d.sd, c.at(c.w.R0), W, W, gp(x.fcW[0]) + d.K0, ld(x.fcW[0]), 1,
                           nullptr, nullptr));
            SPN_TRY(sb.add(B, c.at(c.w.embr), d.sd, d.sd, c.at(c.w.R4), W, W, gp(x.fcW[d.skip]) + W + d.K0,
                           ld(x.fcW[d.skip]), 1, nullptr, nullptr));
        }
        SPN_TRY(sb.run(s));
        if (d.sem) SPN_TRY(class_sum(n_rays, c.at(c.w.gemb), d.sd, labels, d.C, gp(x.emb), c.acc, s));
    }
    SPN_TRY(stream_dep(sd, s2, s_main));  // join: the caller's stream sees every gradient
    return grad_mark(d.L + 1, s_main);
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_mlp_trunk_wgrad(const spnerf_model_cfg* cfg, int32_t n_seg, void* const* workspaces,
                                          const int64_t* n_rays, const int32_t* n_samples, const int32_t* flags,
                                          float* grad_flat, void* stream) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    if (n_seg == 0) {   // capability query: may a backward defer under the current options?
        Ctx c{d, packed_layout(d), WS{}, nullptr, nullptr, 0};
        return trunk_wgrad_ok(c) ? 1 : 0;
    }
    SPN_ARG(n_seg > 0 && workspaces && n_rays && n_samples && flags && grad_flat, "spnerf_mlp_trunk_wgrad: NULL argument");
    return trunk_wgrad(d, n_seg, workspaces, n_rays, n_samples, flags, grad_flat, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int32_t spnerf_mlp_backward(const spnerf_model_cfg* cfg, const void* packed, const float* rays,
                                       int32_t ray_stride, int64_t n_rays, int32_t n_samples, const int64_t* labels,
                                       const float* t_emb, int32_t flags, void* workspace, const float* d_out,
                                       float* grad_flat, float* grad_t_emb, void* stream) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    SPN_ARG(packed && rays && workspace && d_out && grad_flat, "mlp_backward: NULL pointer");
    SPN_ARG(!d.sem || labels, "mlp_backward: semantic model needs labels");
    SPN_ARG(!d.beta || mode_of(flags) != 0 || t_emb, "mlp_backward: beta model needs t_emb");
    return mlp_backward(d, (const float*)packed, rays, ray_stride, n_rays, n_samples, labels, t_emb, flags,
                        (float*)workspace, d_out, grad_flat, grad_t_emb, (hipStream_t)stream);
}
