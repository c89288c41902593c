// SP-NeRF per-point network on gfx950: SPNeRF.forward (models/spnerf.py:273-369) and its
// backward, as a sequence of fp32 MFMA GEMMs (gemm_f32.hip) with fused epilogues plus small
// per-point / per-ray kernels.
//
// Algebraic re-layout (exact up to fp32 summation order):
//  * the semantic embedding, the sun direction and the time embedding are constant along a
//    ray, so their input columns of fc_net.0 / fc_net.<2*skip> / sun_v_net.0 / beta_from_xyz.0
//    become per-RAY bias rows (k_ray_fwd) added in the GEMM epilogue — no repeat_interleave,
//    no K padding for 63/575/515 wide inputs;
//  * sky_color depends only on sun_d → evaluated once per ray, broadcast to the points;
//  * sibling heads that read the same activation are one GEMM: G = H_L·[feat; sem hidden]^T,
//    Q = feat·[sun hidden 1; rgb hidden; beta hidden]^T;
//  * N ≤ C-wide output heads (σ, rgb, sun, β, semantic logits) are per-point dot products.
//
// This unit: the forward pass's orchestration (mlp_backward.hip: the backward's; the small
// kernels: point_kernels.hip; what both directions share: mlp_ctx.h).
#include <mutex>
#include <unordered_map>

#include "mlp_ctx.h"
#include "point_kernels.h"

namespace spn {

int g_l0_split = 1;       // bf16 MLP: fc_net.0 on bf16 hi/lo planes (0 = fp32 MFMA GEMM)
int g_trunk_l0 = 2;       // ... and inside the fused trunk launch: 1 = when nothing is saved (inference),
                          // 2 = also when saving (the default since round 4: the 64-point register-D training
                          // trunk with layer 0 against the separate hi/lo-plane GEMM + k_encode's planes:
                          // C4 26.56 / 26.58 -> 26.44 / 26.36 ms, C4@512 4.248 -> 4.202 ms, same call; it had
                          // measured 400 us slower on the round-2 trunk)
// option "heads_epi": the training forward's narrow heads (rgb, sun, beta, semantic logits; σ and the
// sky columns with the sun) in the epilogues of the G / Q / sun_v.3 GEMMs instead of k_heads_fwd_v:
// C4 26.39 / 26.35 -> 26.13 / 26.08 ms (heads_fwd's 0.58 ms for +0.31 ms of epilogue), C4@512
// 3.950 / 3.945 -> 3.919 / 3.921 ms (same call).  2: the whole training heads (G, Q, sun_v 2 / 3
// with their saved activations, and the narrow heads) in one LDS-resident launch after the trunk
// (k_heads_train_bf16, train_heads_on), the epilogue GEMMs where the shape does not fit: the same
// step time (C4 25.34 / 25.39 against 25.32 / 25.37 ms, C4@512 3.712 / 3.709 ms, pairs in one
// call), 2.5 GB fewer HBM bytes per C4 step (PMC 88.3 against 90.8 GB) and 6 fewer launches
int g_heads_epi = 2;

// Trunk + G/Q/sun_v GEMMs of the forward (spnerf.py:323-355).  In the bf16 MLP, layer 0 stays
// an fp32 GEMM (sin(30·x) amplifies operand rounding 30x) that writes bf16 H_1 / D_1.
// bf16 MLP: layer 0 runs inside the fused trunk launch (reading the fp32 PE rows itself)
// bf16 trunk layers 1 .. L-1 (w0 = 1) compute H = sin(Z) with Z = fp16(pre-activation), and the
// training forward saves Z alone for layers 1 .. L-2 (Z and H for the last): the backward stages
// sin(Z) for the weight gradients and multiplies by cos(Z) in the dX epilogues, so the forward
// writes one [P][512] tensor per layer instead of H and D (option "zsave"; must not change
// between a forward and its backward).  Off by default: measured on C4 (tools/gpu_ab_opt.sh) the
// trunk saves 0.9 ms per step but the weight gradients' sin staging costs 1.25 ms (31.3 vs 31.9 ms)
int g_zsave = 0;

// the D-layout record of the saving passes' workspaces (mlp_ctx.h)
static std::mutex g_dtile_mu;
static std::unordered_map<const void*, int> g_dtile_rec;
void dtile_set(const void* ws, int mask) {
    std::lock_guard<std::mutex> lk(g_dtile_mu);
    if (mask) g_dtile_rec[ws] = mask;
    else g_dtile_rec.erase(ws);
}
int dtile_get(const void* ws) {
    std::lock_guard<std::mutex> lk(g_dtile_mu);
    const auto it = g_dtile_rec.find(ws);
    return it == g_dtile_rec.end() ? 0 : it->second;
}
int g_pe_inline = 1;  // option "pe_inline": inference trunk with layer 0 encodes o + dir·z itself (no k_encode)

static HeadsFusedArgs heads_args(const Ctx& c, int mode, int64_t hl, double* flop, double* bytes);
// the training heads' arguments: what they store, and their counted work (the wide layers as
// computed — the solar pass's Q runs all 2H columns — and the narrow heads; stored: feat (+ the
// semantic hidden and its D), Q and DQ, S2 / S3 and their D, the output rows, the gates)
static HeadsFusedArgs train_heads_args(const Ctx& c, int mode, int64_t hl, double* flop, double* bytes) {
    const Dims& d = c.d;
    const int64_t P = c.w.P;
    const int W = d.W, H = d.H;
    HeadsFusedArgs h = heads_args(c, mode, hl, flop, bytes);
    h.G = c.hb(c.w.G); h.DG = d.sem ? c.hb(c.w.DG) : nullptr; h.ldG = d.NG;
    h.Q = c.hb(c.w.Q); h.DQ = c.hb(c.w.DQ); h.ldQ = d.NQ;
    h.S2 = c.hb(c.w.S2); h.DS2 = c.hb(c.w.DS2); h.S3 = c.hb(c.w.S3); h.DS3 = c.hb(c.w.DS3);
    h.hsave = c.at(c.w.hsave);
    const bool m0 = mode == 0, sm = m0 && d.sem;
    *flop = 2.0 * P * ((double)W * W + 2.0 * H * W + 2.0 * H * H + (sm ? (double)H * W + H * d.C : 0.0) + (m0 ? 3.0 * H : 0.0) + H);
    *bytes = 2.0 * P * (W + (sm ? 2.0 * H : 0.0) + 2.0 * (m0 ? 2 * H : H) + 4.0 * H) + 4.0 * P * (d.NO + (m0 ? 4 : 1));
    return h;
}

// the fused heads' arguments and counted work (k_heads_bf16, or inside the inference trunk)
static HeadsFusedArgs heads_args(const Ctx& c, int mode, int64_t hl, double* flop, double* bytes) {
    const Dims& d = c.d;
    const int64_t P = c.w.P;
    const int W = d.W, H = d.H;
    HeadsFusedArgs a;
    a.HL = hl >= 0 ? c.hb(hl) : nullptr; a.packed = c.P; a.rbQ = c.at(c.w.rbQ); a.sky = c.at(c.w.sky); a.out = c.out;
    a.P = P; a.S = c.S; a.NO = d.NO; a.C = d.sem ? d.C : 0; a.sem_col = d.sem_col; a.mode = mode;
    *flop = mode == 1 ? 2.0 * P * W
                      : 2.0 * P * ((double)W * (W + 2 * H) + 2.0 * H * H + (d.sem ? (double)H * W + H * d.C : 0.0) + W + 4.0 * H);
    *bytes = 2.0 * P * W + 4.0 * P * (mode == 1 ? 1 : d.NO);
    return a;
}

template <typename T>
static int32_t forward_gemms(const Ctx& c, bool save, int mode, hipStream_t s, bool* sig_done) {
    using G = Gemms<T>;
    using NT = typename G::NT;
    const Dims& d = c.d;
    const int64_t P = c.w.P;
    const int W = d.W, H = d.H, S = c.S;
    constexpr bool BF = std::is_same<T, bf16>::value;
    const T* X0 = BF ? G::buf(c, c.w.X0b) : G::buf(c, c.w.X0);
    const T* h = nullptr;
    T* HL = nullptr;
    const bool fused = BF && fused_trunk_on(c);
    const bool zs = BF && g_zsave;
    const int first = fused && trunk_l0_on(c, save) ? 0 : 1;  // first layer of the fused launch
    for (int i = 0; i < d.L; ++i) {
        if (fused && i == first) {
            // layers first .. L-1 in one persistent launch, activations resident in LDS
            TrunkArgs a;
            a.H1 = reinterpret_cast<const bf16*>(h);
            a.X0b = c.hb(c.w.X0b);
            if (first == 0) {
                if (pe_inline_on(c, save)) {
                    a.rays = c.rays; a.rs = c.rs; a.dir_off = c.dir_off; a.z = c.z; a.ldz = c.ldz;
                    a.n_freq = d.K0 == 3 ? 0 : d.K0 / 6; a.K0 = d.K0;
                    if (save) a.X0b_out = c.hb(c.w.X0b);
                } else {
                    a.X0 = c.at(c.w.X0);
                }
                a.rb0 = d.sem ? c.at(c.w.rb0) : nullptr;
            }
            double ksum = 0.0;
            for (int l = first; l < d.L; ++l) {
                a.Wf[l] = c.pk16(c.k.Wf16[l]);
                a.bias[l] = c.pk(c.k.bt[l]);
                const bool zonly = zs && l >= 1 && l < d.L - 1;  // Z alone (in Db) for the backward
                a.Hs[l] = save ? (zonly ? nullptr : c.hb(c.w.Hb[l])) : (l == d.L - 1 ? c.hb(c.w.Hb[l & 1]) : nullptr);
                a.Ds[l] = save ? c.hb(c.w.Db[l]) : nullptr;
                ksum += l == 0 ? d.K0p : c.k.Kp[l];   // algorithmic K (layer 0 runs 4·K0p on hi/lo planes)
            }
            a.rb_skip = d.sem ? c.at(c.w.rb4) : nullptr;
            a.P = P; a.S = S; a.L = d.L; a.skip = d.skip; a.K0p = d.K0p;
            a.zround = zs ? 1 : 0;
            // the σ head's pre-activation from the last layer's LDS image (the wave-per-point
            // heads then skip H_L); option trunk_sigma
            if (sig_done && !heads_fused_on(c, save, mode) && g_heads_variant != 0 && W == 512 && trunk_sigma_ok(a, save)) {
                a.sig_hsave = c.at(c.w.hsave);
                a.wsig = c.pk(c.k.wsig);
                a.bsig = c.pk(c.k.bsig);
                *sig_done = true;
            }
            // tile-ordered D (fused_bwd >= 2) of the layers the dX chain reads (and D_{L-1} where the
            // fused heads dX launch reads it), when the saving 128-point instance runs and no 64-point block
            // straddles two windows: the window starts on a block boundary and ends on one (or ends
            // the workspace).  A pass's later windows follow its first one's record.
            if (save) {
                const int64_t pb = c.win_p0, pe = c.win_p0 + P, pt = c.total_P < 0 ? P : c.total_P;
                const bool aligned = pb % kDtileRows == 0 && (pe % kDtileRows == 0 || pe == pt);
                int mask = 0;
                if (pb == 0) {
                    if (g_fused_bwd >= 2 && aligned && trunk_dtile_ok(a)) {
                        for (int l = first; l < d.L - 1; ++l) mask |= 1 << l;
                        // D_{L-1} too when, and only when, the fused heads dX launch will consume it
                        // (option fused_heads_bwd; the four head GEMMs read it row-major)
                        if (g_fused_heads_bwd && heads_dx_shape(c, mode)) mask |= 1 << (d.L - 1);
                    }
                    dtile_set(c.ws, mask);
                } else {
                    mask = dtile_get(c.ws);
                    SPN_ARG(mask == 0 || (aligned && trunk_dtile_ok(a) && (mask & ((1 << first) - 1)) == 0),
                            "mlp_forward_window: the pass's D is tile-ordered (mask %x); this window cannot follow it", mask);
                }
                a.dtile = mask;
            }
            // algorithmic HBM bytes: the first layer's input (fp32 PE, or H_1 and the bf16 PE)
            // in; out when saving H and D of every layer, or Z of every layer and the last H
            const double in = first == 0 ? (a.rays ? 4.0 * P : 4.0 * P * d.K0p) : 2.0 * P * (W + (d.skip > 0 ? d.K0p : 0));
            const double nout = !save ? 1.0 : (zs ? d.L - first + 1.0 : 2.0 * (d.L - first));
            const double bytes = in + 2.0 * P * W * nout + (a.X0b_out ? 2.0 * P * d.K0p : 0.0);
            if constexpr (BF) {
                // inference: the fused heads on the trunk's last LDS image (no H_L in HBM)
                if (c.heads_done && c.out && heads_fused_on(c, save, mode) &&
                    // (the two-workgroup ablation kernel's heads: one class group only)
                    (trunk1_heads_ok(a) || (trunk2_heads_ok(a) && (!d.sem || d.C <= 4)))) {
                    double hflop = 0.0, hbytes = 0.0;
                    const HeadsFusedArgs h = heads_args(c, mode, -1, &hflop, &hbytes);
                    // algorithmic bytes: the trunk's input, the output rows (H_L never leaves)
                    if (trunk1_heads_ok(a))
                        SPN_TRY(trunk1_heads_bf16(a, h, c.k, s, 2.0 * P * W * ksum + hflop, in + (hbytes - 2.0 * P * W)));
                    else
                        SPN_TRY(trunk2_heads_bf16(a, h, c.k, s, 2.0 * P * W * ksum + hflop, in + (hbytes - 2.0 * P * W)));
                    *c.heads_done = true;
                    return SPNERF_OK;
                }
            }
            SPN_TRY(trunk_bf16(a, s, 2.0 * P * W * ksum, bytes));
            HL = reinterpret_cast<T*>(a.Hs[d.L - 1]);
            break;
        }
        T* dst = save ? G::buf(c, c.w.Hb[i]) : G::buf(c, c.w.Hb[i & 1]);
        T* dd = save ? G::buf(c, c.w.Db[i]) : nullptr;
        const float* rb = (d.sem && (i == 0 || i == d.skip)) ? c.at(i == 0 ? c.w.rb0 : c.w.rb4) : nullptr;
        if (i == 0 && BF && g_l0_split) {
            // fc_net.0 on MFMA bf16 as (x_hi + x_lo)·(w_hi + w_lo), K = 4·K0p: relative error
            // ≈ 2^-17 per product (the split's remainder) against the fp32 GEMM's 2^-24, far
            // inside the bf16 output's 2^-9, at bf16 MFMA rates instead of fp32 ones
            NT16Args g;
            g.A = c.hb(c.w.X0s); g.lda = 4 * d.K0p; g.K1 = 4 * d.K0p;
            g.B = c.pk16(c.k.W0s16); g.ldb = 4 * d.K0p;
            g.C = reinterpret_cast<bf16*>(dst); g.ldc = W;
            g.M = (int)P; g.N = W; g.K = 4 * d.K0p;
            g.bias = c.pk(c.k.bt[0]);
            if (rb) { g.rowbias = rb; g.ld_rb = W; g.rows_per_ray = S; }
            g.act = 1; g.w0 = 30.f; g.n_lin = 0;
            if (save) { g.Dout = reinterpret_cast<bf16*>(dd); g.ld_dout = W; }
            g.k_alg = d.K0p;   // FLOPs counted at the layer's own K (the split's 4x MFMA work is overhead)
            SPN_TRY(gemm_nt_bf16(g, s));
        } else if (i == 0) {
            NTArgs g;
            g.A = c.at(c.w.X0); g.lda = d.K0p; g.K1 = d.K0p;
            g.B = c.pk(c.k.Wt[0]); g.ldb = d.K0p;
            g.ldc = W;
            g.M = (int)P; g.N = W; g.K = d.K0p;
            g.bias = c.pk(c.k.bt[0]);
            if (rb) { g.rowbias = rb; g.ld_rb = W; g.rows_per_ray = S; }
            g.act = 1; g.w0 = 30.f; g.n_lin = 0;
            g.ld_dout = W;
            if constexpr (BF) { g.C16 = dst; g.D16 = dd; }
            else { g.C = dst; g.Dout = dd; }
            SPN_TRY(gemm_nt(g, s));
        } else {
            NT g;
            g.A = h; g.lda = W; g.K1 = W;
            if (i == d.skip) { g.A2 = X0; g.lda2 = d.K0p; }
            g.B = G::w(c, c.k.Wt[i], BF ? c.k.Wt16[i] : -1); g.ldb = c.k.Kp[i];
            g.C = dst; g.ldc = W;
            g.M = (int)P; g.N = W; g.K = c.k.Kp[i];
            g.bias = c.pk(c.k.bt[i]);
            if (rb) { g.rowbias = rb; g.ld_rb = W; g.rows_per_ray = S; }
            g.act = 1; g.w0 = 1.f; g.n_lin = 0;
            if (save) { g.Dout = dd; g.ld_dout = W; }
            if constexpr (BF) {
                g.zround = zs ? 1 : 0;
                g.dout_z = zs ? 1 : 0;
            }
            SPN_TRY(G::nt(g, s));
        }
        h = dst;
        HL = dst;
    }
    if (mode == 1) return SPNERF_OK;
    if (BF && heads_fused_on(c, save, mode)) return SPNERF_OK;  // G, Q, sun_v 2/3 inside the fused heads
    if constexpr (BF) {
        // option heads_epi 2: the training heads as one launch after the trunk (H_L from HBM)
        if (save && train_heads_on(c, mode) && sig_done && *sig_done) {
            double hflop = 0.0, hbytes = 0.0;
            const HeadsFusedArgs h = train_heads_args(c, mode, c.w.Hb[d.L - 1], &hflop, &hbytes);
            if (heads_train_bf16_ok(h, c.k)) {
                SPN_TRY(heads_train_bf16(h, c.k, s, hflop, hbytes + 2.0 * P * W));
                *c.heads_done = true;
                return SPNERF_OK;
            }
        }
    }
    T* S2buf = save ? G::buf(c, c.w.S2) : G::buf(c, c.w.Hb[((d.L - 1) & 1) ^ 1]);
    T* S3buf = save ? G::buf(c, c.w.S3) : G::buf(c, c.w.Hb[2]);
    // option heads_epi: the narrow heads in the G / Q / sun_v.3 epilogues (bf16 DMA NT with the
    // bias / per-ray-row epilogue; σ from the trunk's hsave column); its epilogue holds three
    // outputs per head in registers, so C <= 3 here (more classes: the wave-per-point heads below)
    const bool hepi = BF && g_heads_epi && g_nt16_epi && (g_nt16_ip_gen == 2 || g_nt16_ip_gen == 3) && !zs && g_nt16_variant == 8 && save &&
                      sig_done && *sig_done && c.out && c.heads_epi_done &&
                      W == 512 && H == 256 && (!d.sem || d.C <= 3) && S % 32 == 0 && mode != 1 &&
                      d.NG % 256 == 0 && d.NQ % 256 == 0;
    NTHeads hbase;
    if (hepi) {
        hbase.out = c.out; hbase.NO = d.NO; hbase.sem_col = d.sem_col;
        hbase.hsave = c.at(c.w.hsave); hbase.sky = c.at(c.w.sky); hbase.S = S; hbase.full = mode == 0 ? 1 : 0;
    }
    auto head = [&](NTHeads& hd, int col0, int nout, int kind, int64_t w, int ldw, int64_t b) {
        hd.col0[hd.n] = col0; hd.nout[hd.n] = nout; hd.kind[hd.n] = kind;
        hd.w[hd.n] = c.pk(w); hd.ldw[hd.n] = ldw; hd.b[hd.n] = c.pk(b);
        ++hd.n;
    };
    // G = H_L · [feat ; sem hidden]^T   (feat linear, sem hidden sin)
    NT g;
    g.A = HL; g.lda = W; g.K1 = W;
    g.B = G::w(c, c.k.WG, c.k.WG16); g.ldb = W;
    g.C = G::buf(c, c.w.G); g.ldc = d.NG;
    g.M = (int)P; g.N = mode == 0 ? d.NG : W; g.K = W;
    g.bias = c.pk(c.k.bG);
    g.act = 1; g.w0 = 1.f; g.n_lin = W;
    if (save) { g.Dout = G::buf(c, c.w.DG); g.ld_dout = d.NG; }
    if constexpr (BF)
        if (hepi && mode == 0 && d.sem) {
            g.hd = hbase;
            head(g.hd, W, d.C, 3, c.k.Wm2, H, c.k.bm2);
        }
    SPN_TRY(G::nt(g, s));
    // Q = feat · [sun1 ; rgb1 ; beta1]^T + per-ray (sun_d / t) rows, all sin
    NT q;
    q.A = G::buf(c, c.w.G); q.lda = d.NG; q.K1 = W;
    q.B = G::w(c, c.k.WQ, c.k.WQ16); q.ldb = W;
    q.C = G::buf(c, c.w.Q); q.ldc = d.NQ;
    q.M = (int)P; q.N = mode == 0 ? d.NQ : H; q.K = W;
    q.bias = c.pk(c.k.bQ);
    q.rowbias = c.at(c.w.rbQ); q.ld_rb = d.NQ; q.rows_per_ray = S;
    q.act = 1; q.w0 = 1.f;
    if (save) { q.Dout = G::buf(c, c.w.DQ); q.ld_dout = d.NQ; }
    if constexpr (BF)
        if (hepi && mode == 0) {
            q.hd = hbase;
            head(q.hd, H, 3, 0, c.k.Wr2, H, c.k.br2);
            if (d.beta) head(q.hd, 2 * H, 1, 2, c.k.wb2, H, c.k.bb2);
        }
    SPN_TRY(G::nt(q, s));
    // sun_v_net layers 2 and 3
    NT s2;
    s2.A = G::buf(c, c.w.Q); s2.lda = d.NQ; s2.K1 = H;
    s2.B = G::w(c, c.k.Ws2, c.k.Ws2_16); s2.ldb = H;
    s2.C = S2buf; s2.ldc = H;
    s2.M = (int)P; s2.N = H; s2.K = H;
    s2.bias = c.pk(c.k.bs2); s2.act = 1; s2.w0 = 1.f;
    if (save) { s2.Dout = G::buf(c, c.w.DS2); s2.ld_dout = H; }
    SPN_TRY(G::nt(s2, s));
    NT s3 = s2;
    s3.A = S2buf; s3.lda = H;
    s3.B = G::w(c, c.k.Ws3, c.k.Ws3_16);
    s3.C = S3buf;
    s3.bias = c.pk(c.k.bs3);
    s3.Dout = save ? G::buf(c, c.w.DS3) : nullptr;
    if constexpr (BF)
        if (hepi) {
            s3.hd = hbase;
            head(s3.hd, 0, 1, 1, c.k.ws4, H, c.k.bs4);
        }
    SPN_TRY(G::nt(s3, s));
    if (hepi) *c.heads_epi_done = true;
    return SPNERF_OK;
}

static int32_t mlp_forward(const Dims& d, const float* packed, const float* rays, int rs, int dir_off,
                           int64_t n_rays, int S, const float* z, const int64_t* labels, const float* temb, int flags,
                           float* ws, float* out, hipStream_t s, int64_t n_total = -1, int64_t r0 = 0, int ldz = 0) {
    // n_total >= 0: rays [r0, r0 + n_rays) of a workspace laid out for n_total rays (forward_window)
    Ctx c{d, packed_layout(d),
          n_total < 0 ? ws_layout(d, n_rays, S, flags) : ws_window(d, ws_layout(d, n_total, S, flags), r0, n_rays, S),
          packed, ws, S};
    const bool save = flags & SPNERF_MLP_SAVE;
    const int mode = mode_of(flags);
    const int64_t P = n_rays * S;
    if (P == 0) return SPNERF_OK;
    SPN_ARG(P < (1ll << 31) / std::max(d.NQ, d.NG), "too many points (%lld) for one call", (long long)P);
    SPN_ARG(!(flags & SPNERF_MLP_KEEP_FEAT) || (!save && mode == 0 && n_total < 0),
            "SPNERF_MLP_KEEP_FEAT goes with a whole non-saving forward of every head");
    c.keep_feat = (flags & SPNERF_MLP_KEEP_FEAT) ? 1 : 0;
    SPN_ARG(!d.sem || labels, "semantic model needs labels");
    SPN_ARG(!d.beta || mode != 0 || temb, "beta model needs t_emb");

    // per-ray terms
    {
        RayFwdArgs a{rays, rs, labels, temb, packed, c.k, d, c.at(c.w.rb0), c.at(c.w.rb4), c.at(c.w.rbQ),
                     c.at(c.w.skyh), c.at(c.w.sky), d.sem ? 1 : 0, mode != 1, mode == 0};
        if (!d.beta || mode != 0) {
            a.d.beta = false;
            a.d.td = 0;
        }
        if (d.sem || mode != 1) SPN_TRY(ray_fwd(a, n_rays, s));
    }
    // positional encoding (fp32 for layer 0, plus a bf16 copy for the skip layer / dW_0); the
    // fused inference trunk with layer 0 computes it in its staging instead
    c.rays = rays; c.rs = rs; c.dir_off = dir_off; c.z = z; c.ldz = ldz > 0 ? ldz : S;
    if (!pe_inline_on(c, save)) {
        // bf16 MLP, layer 0 on bf16 planes: a separate GEMM reads the planes X0s; inside the
        // fused trunk it splits the fp32 rows itself
        const bool planes = d.bf && g_l0_split && !trunk_l0_on(c, save);
        SPN_TRY(encode(rays, rs, dir_off, z, S, c.ldz, P, d.K0, d.K0p, planes ? nullptr : c.at(c.w.X0),
                       d.bf ? c.hb(c.w.X0b) : nullptr, planes ? c.hb(c.w.X0s) : nullptr, s));
    }
    // the trunk D layout record of this pass (forward_gemms sets it where the fused trunk tiles D)
    c.win_p0 = n_total < 0 ? 0 : r0 * S;
    c.total_P = n_total < 0 ? -1 : n_total * S;
    if (save && d.bf) {
        if (c.win_p0 == 0) dtile_set(ws, 0);
        else SPN_ARG(fused_trunk_on(c) || dtile_get(ws) == 0, "mlp_forward_window: the pass's D is tile-ordered; this window runs layer by layer");
    }
    bool sig_done = false;  // hsave[p·8] (σ pre-activation) written by the fused trunk
    bool heads_done = false;  // the trunk launch ran the fused heads
    bool heads_epi_done = false;  // the head GEMMs' epilogues wrote the narrow heads
    c.out = out;
    c.heads_done = &heads_done;
    c.heads_epi_done = &heads_epi_done;
    if (d.bf) SPN_TRY(forward_gemms<bf16>(c, save, mode, s, &sig_done));
    else SPN_TRY(forward_gemms<float>(c, save, mode, s, nullptr));
    if (heads_done || heads_epi_done) return SPNERF_OK;
    if (heads_fused_on(c, save, mode)) {
        double flop = 0.0, bytes = 0.0;
        const HeadsFusedArgs a = heads_args(c, mode, c.w.Hb[(d.L - 1) & 1], &flop, &bytes);
        SPN_TRY(heads_bf16(a, c.k, s, flop, bytes));
        return SPNERF_OK;
    }
    {
        const int64_t L = d.L - 1;
        const int64_t hl = save ? c.w.Hb[L] : c.w.Hb[L & 1];
        const int64_t s3 = save ? c.w.S3 : c.w.Hb[2];
        if (d.bf)
            return heads_fwd(HeadsArgs<bf16>{packed, d, c.hb(hl), c.hb(c.w.G), c.hb(c.w.Q), c.hb(s3), c.at(c.w.sky), out, c.at(c.w.hsave), P, S, mode},
                             c.k, sig_done, s);
        return heads_fwd(HeadsArgs<float>{packed, d, c.at(hl), c.at(c.w.G), c.at(c.w.Q), c.at(s3), c.at(c.w.sky), out, c.at(c.w.hsave), P, S, mode},
                         c.k, sig_done, s);
    }
}

}  // namespace spn

using namespace spn;

extern "C" int64_t spnerf_mlp_workspace_bytes(const spnerf_model_cfg* cfg, int64_t n_rays, int32_t n_samples, int32_t flags) {
    Dims d;
    if (make_dims(cfg, &d) != SPNERF_OK || n_rays < 0 || n_samples <= 0) return -1;
    return ws_layout(d, n_rays, n_samples, flags).total * (int64_t)sizeof(float);
}

extern "C" int32_t spnerf_mlp_forward(const spnerf_model_cfg* cfg, const void* packed, const float* rays, int32_t ray_stride,
                                      int32_t dir_offset, int64_t n_rays, int32_t n_samples, const float* z,
                                      const int64_t* labels, const float* t_emb, int32_t flags, void* workspace, float* out,
                                      void* stream) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    SPN_ARG(packed && rays && z && workspace && out, "mlp_forward: NULL pointer");
    SPN_ARG(n_rays >= 0 && n_samples > 0 && ray_stride >= 11, "mlp_forward: bad sizes");
    SPN_ARG(dir_offset == 3 || dir_offset == 8, "mlp_forward: dir_offset must be 3 (view) or 8 (sun)");
    return mlp_forward(d, (const float*)packed, rays, ray_stride, dir_offset, n_rays, n_samples, z, labels, t_emb, flags,
                       (float*)workspace, out, (hipStream_t)stream);
}

extern "C" int32_t spnerf_mlp_forward_window(const spnerf_model_cfg* cfg, const void* packed, const float* rays,
                                             int32_t ray_stride, int32_t dir_offset, int64_t n_rays_total,
                                             int64_t ray_begin, int64_t n_rays, int32_t n_samples, const float* z,
                                             int32_t z_stride, const int64_t* labels, const float* t_emb, int32_t flags,
                                             void* workspace, float* out, void* stream) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    SPN_ARG(packed && rays && z && workspace && out, "mlp_forward_window: NULL pointer");
    SPN_ARG(n_rays >= 0 && n_samples > 0 && ray_stride >= 11, "mlp_forward_window: bad sizes");
    SPN_ARG(ray_begin >= 0 && n_rays_total >= ray_begin + n_rays, "mlp_forward_window: rays [%lld, %lld) outside %lld",
            (long long)ray_begin, (long long)(ray_begin + n_rays), (long long)n_rays_total);
    SPN_ARG(n_rays_total * n_samples < (1ll << 31) / std::max(d.NQ, d.NG), "mlp_forward_window: too many points");
    SPN_ARG(dir_offset == 3 || dir_offset == 8, "mlp_forward_window: dir_offset must be 3 (view) or 8 (sun)");
    SPN_ARG(z_stride == 0 || z_stride >= n_samples, "mlp_forward_window: z_stride %d < n_samples %d", z_stride, n_samples);
    return mlp_forward(d, (const float*)packed, rays, ray_stride, dir_offset, n_rays, n_samples, z, labels, t_emb, flags,
                       (float*)workspace, out, (hipStream_t)stream, n_rays_total, ray_begin, z_stride);
}
