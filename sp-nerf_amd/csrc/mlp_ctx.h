// What the forward (mlp_forward.hip) and the backward (mlp_backward.hip) orchestration share: the
// pass context, the dtype dispatch of the GEMM sequence, the weight-gradient GEMM + slab reduction
// helpers, the D-layout record and the predicates that pick a pass's kernels.
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "gemm_bf16.h"
#include "gemm_f32.h"
#include "heads_dx.h"
#include "mlp_layout.h"
#include "mlp_options.h"
#include "trunk.h"

namespace spn {
#pragma GCC visibility push(hidden)  // internal to the library

// a pass's heads: 0 every head, 1 σ only, 2 σ + sun (the solar pass)
inline int mode_of(int flags) { return (flags & SPNERF_MLP_SIGMA_ONLY) ? 1 : ((flags & SPNERF_MLP_SUN_ONLY) ? 2 : 0); }

struct Ctx {
    Dims d;
    Packed k;
    WS w;
    const float* P;  // packed
    float* ws;       // workspace base
    int S;
    int acc = 0;     // backward: gradient reductions add into the flat gradient
    int defer = 0;   // backward: the trunk layers' weight gradients are left to spnerf_mlp_trunk_wgrad
    int keep_feat = 0;  // forward (SPNERF_MLP_KEEP_FEAT): the heads in launches of their own, G left in the workspace
    // the forward's ray inputs (the fused inference trunk encodes layer 0's input itself)
    const float* rays = nullptr;
    const float* z = nullptr;
    int rs = 0, dir_off = 0;
    int ldz = 0;                    // z's row stride per ray (S: contiguous rows)
    float* out = nullptr;           // the forward's output rows (the fused trunk + heads write them)
    bool* heads_done = nullptr;     // set when the trunk launch ran the fused heads too
    bool* heads_epi_done = nullptr;  // set when the head GEMMs' epilogues wrote the narrow heads
    // forward_window: the window's first point in the workspace and the workspace's points (-1: no window)
    int64_t win_p0 = 0, total_P = -1;
    float* at(int64_t off) const { return ws + off; }
    const float* pk(int64_t off) const { return P + off; }
    bf16* hb(int64_t off) const { return reinterpret_cast<bf16*>(ws + off); }          // bf16 workspace buffer
    const bf16* pk16(int64_t off) const { return reinterpret_cast<const bf16*>(P) + off; }  // bf16 packed weights
};

// dtype dispatch for the GEMM sequence: fp32 (NTArgs / TNArgs) or bf16 (NT16Args / TN16Args,
// same field names); T is the activation element type.
template <typename T>
struct Gemms;
template <>
struct Gemms<float> {
    using NT = NTArgs;
    using TN = TNArgs;
    static float* buf(const Ctx& c, int64_t off) { return c.at(off); }
    static const float* w(const Ctx& c, int64_t off32, int64_t) { return c.pk(off32); }
    static int32_t nt(const NT& a, hipStream_t s) { return gemm_nt(a, s); }
    static int splits(int P, int N, int K) { return tn_splits(P, N, K); }
    static int32_t tn(const TN& a, int sp, hipStream_t s) { return gemm_tn(a, sp, s); }
};
template <>
struct Gemms<bf16> {
    using NT = NT16Args;
    using TN = TN16Args;
    static bf16* buf(const Ctx& c, int64_t off) { return c.hb(off); }
    static const bf16* w(const Ctx& c, int64_t, int64_t off16) { return c.pk16(off16); }
    static int32_t nt(const NT& a, hipStream_t s) { return gemm_nt_bf16(a, s); }
    static int splits(int P, int N, int K) { return tn_splits_bf16(P, N, K); }
    static int32_t tn(const TN& a, int sp, hipStream_t s) { return gemm_tn_bf16(a, sp, s); }
};

// ---- which kernels a pass runs (both directions must agree) --------------------------------

inline bool fused_trunk_on(const Ctx& c) {
    return c.d.bf && g_fused_trunk && !c.k.Wf16.empty() && c.k.Wf16[1] >= 0;
}
// inference (nothing saved) of the full or the σ-only heads: the fused heads kernel after the trunk
inline bool heads_fused_on(const Ctx& c, bool save, int mode) {
    return !c.keep_feat && !save && (mode == 0 || mode == 1) && c.d.bf && c.k.Ffeat16 >= 0 && heads_bf16_supported(c.d);
}
inline bool trunk_l0_on(const Ctx& c, bool save) {
    return fused_trunk_on(c) && g_l0_split && (g_trunk_l0 == 2 || (g_trunk_l0 == 1 && !save)) && c.k.Wf16[0] >= 0 &&
           trunk_l0_supported(c.d.K0p, save, c.d.bf && g_zsave);
}
// (training too since round 4: the trunk then writes the bf16 PE rows X0b the weight gradients read,
// and no k_encode runs)
inline bool pe_inline_on(const Ctx& c, bool save) { return g_pe_inline && trunk_l0_on(c, save); }

// option heads_epi 2: the training forward's heads (k_heads_train_bf16) as one launch after the
// saving trunk, where the shape allows: W = 512, H = 256, no β head, C <= kHeadsMaxC (8: one kernel
// instance per group count of four classes); a larger C falls back to the layer-by-layer heads
inline bool train_heads_shape(const Ctx& c, int mode) {
    const Dims& d = c.d;
    return d.bf && (mode == 0 || mode == 2) && d.W == 512 && d.H == 256 && !d.beta && (!d.sem || d.C <= kHeadsMaxC) &&
           c.k.Ffeat16 >= 0 && c.k.Fnar16 >= 0 && c.out && c.heads_done && !g_zsave;
}
inline bool train_heads_on(const Ctx& c, int mode) { return g_heads_epi == 2 && train_heads_shape(c, mode); }
// the shapes the fused heads dX launch (heads_dx_bf16.hip) runs: W = 512, H = 256, no β, every head
// or the solar pass, and the packed layout carries its weight streams
inline bool heads_dx_shape(const Ctx& c, int mode) {
    const Dims& d = c.d;
    return d.bf && !g_zsave && (mode == 0 || mode == 2) && d.W == 512 && d.H == 256 && !d.beta && c.k.BG16 >= 0;
}

// Deferred trunk weight gradients need every layer's dZ to outlive the backward: the fused dX
// chain of the bf16 MLP leaves dZ_i in Db[i] (and dZ_{L-1} in dZa) — the layer-by-layer chain
// rotates three buffers.
inline bool trunk_wgrad_ok(const Ctx& c) {
    return c.d.bf && !g_zsave && g_fused_bwd && !c.k.Wb16.empty() && c.k.Wb16[1] >= 0;
}
inline bool defer_heads_for(int64_t P) { return g_defer_heads == 1 || (g_defer_heads == 2 && P <= (1 << 18)); }

// Layout record of a saving pass's trunk D buffers, kept per workspace (the backward picks its
// kernels on the host, so the record lives beside the workspace, keyed by its base address): bit l
// set = Db[l] is tile-ordered (trunk.h dtile_off).  The forward that writes a workspace's first
// points sets it, later windows of the pass follow it, the backward reads it (never the option).
// (the map itself: mlp_forward.hip)
void dtile_set(const void* ws, int mask);
int dtile_get(const void* ws);

// ---- weight gradients: split-P TN GEMM into slabs + fixed-order slab reduction --------------

inline ReduceArgs red(int row0, int nrows, int ncols, float* dst, int ld_dst, float* dst_b) {
    ReduceArgs r;
    r.row0 = row0; r.nrows = nrows; r.ncols = ncols; r.dst = dst; r.ld_dst = ld_dst; r.dst_b = dst_b;
    return r;
}

// r reads the `splits` partial [N][K] slabs of one GEMM (and their row sums slab_b)
inline void bind_slab(ReduceArgs& r, const float* slab, int N, int K, int splits, const float* slab_b, int accumulate) {
    r.slab = slab; r.ld_slab = K; r.slab_stride = (int64_t)N * K; r.splits = splits; r.N = N;
    r.slab_b = slab_b;
    r.accumulate = accumulate;
}

// rows p >= P1 of t come from a second point segment: its pointers shifted back by P1 rows
// (t's leading dimensions are set)
inline void second_segment(TN16Args& t, int64_t P1, const bf16* A, const bf16* B, const bf16* B2 = nullptr) {
    t.P1 = P1;
    t.A_s2 = A - P1 * t.lda;
    t.B_s2 = B - P1 * t.ldb;
    t.B2_s2 = B2 ? B2 - P1 * t.ldb2 : nullptr;
}

// A second point segment of a weight gradient: the same operands in another pass's workspace
// (spnerf_mlp_trunk_wgrad: the main and the solar pass of a render in one GEMM per layer)
struct TnSeg {
    const bf16 *A = nullptr, *B = nullptr, *B2 = nullptr;
    int64_t P = 0;
};

template <typename T>
inline int32_t tn_grad(const Ctx& c, const T* A, int lda, int N, const T* B, int ldb, const T* B2, int ldb2, int K1,
                       int K, hipStream_t s, const std::vector<ReduceArgs>& outs, bool b_sin = false,
                       const TnSeg* sg = nullptr) {
    using G = Gemms<T>;
    const int P1 = (int)c.w.P;
    const int P = P1 + (sg ? (int)sg->P : 0);
    // bf16 skip layer ([H | x0], K = 512 + K0p): the K = 576 GEMM has no 256-wide tiling and ran
    // on the 128x128 kernel at 710 us per 524 288 points; split into the wide K = 512 part and
    // the K0p tail (two passes over dZ, the tail's slab reduced into columns K1..) it is ≈470.
    // Below 2^18 points the single launch is as fast
    // (with the narrow N = 512, K = 64 kernel for the tail, tn_bf16_k64, splitting below 2^18
    // points measured level too: C4 at 512 rays 4.468 / 4.491 against 4.469 / 4.465 ms)
    bool split = std::is_same<T, bf16>::value && g_tn_split_tail && B2 && K > K1 && P >= (1 << 18) &&
                 N % 256 == 0 && K1 % 256 == 0 && (N / 256) * (K1 / 256) >= 4;
    for (const ReduceArgs& r : outs) split = split && !r.transpose;
    if (split) {
        std::vector<ReduceArgs> head, tail;
        for (ReduceArgs r : outs) {
            ReduceArgs h = r;
            h.ncols = std::min(r.ncols, K1);
            head.push_back(h);
            if (r.ncols > K1) {
                ReduceArgs t = r;
                t.dst = r.dst + K1;
                t.ncols = r.ncols - K1;
                t.dst_b = nullptr;  // the column sums come with the head
                tail.push_back(t);
            }
        }
        TnSeg sh, st;
        if (sg) {
            sh = {sg->A, sg->B, nullptr, sg->P};
            st = {sg->A, sg->B2, nullptr, sg->P};
        }
        SPN_TRY(tn_grad<T>(c, A, lda, N, B, ldb, nullptr, 0, K1, K1, s, head, b_sin, sg ? &sh : nullptr));
        if (!tail.empty())
            SPN_TRY(tn_grad<T>(c, A, lda, N, B2, ldb2, nullptr, 0, K - K1, K - K1, s, tail, false, sg ? &st : nullptr));
        return SPNERF_OK;
    }
    // the slab buffer is sized for this workspace's points: a longer (two-segment) GEMM takes
    // no more splits than that
    const int splits = std::min(G::splits(P, N, K), G::splits(P1, N, K));
    typename G::TN t;
    t.A = A; t.lda = lda;
    t.B = B; t.ldb = ldb; t.B2 = B2; t.ldb2 = ldb2; t.K1 = K1;
    if constexpr (std::is_same<T, bf16>::value) t.b_sin = b_sin ? 1 : 0;  // B[:, :K1] holds a saved Z
    t.slab = c.at(c.w.slab); t.ld_slab = K; t.slab_stride = (int64_t)N * K;
    t.slab_b = c.at(c.w.slab_b);
    t.P = P; t.N = N; t.K = K;
    if (sg) {
        if constexpr (std::is_same<T, bf16>::value) second_segment(t, P1, sg->A, sg->B, sg->B2);
        else SPN_ARG(false, "tn_grad: two point segments need the bf16 MLP");
    }
    SPN_TRY(G::tn(t, splits, s));
    std::vector<ReduceArgs> rs;
    for (ReduceArgs r : outs) {
        bind_slab(r, t.slab, N, K, splits, t.slab_b, c.acc);
        rs.push_back(r);
    }
    for (size_t i = 0; i < rs.size(); i += kReduceMulti)
        SPN_TRY(reduce_slabs_multi(rs.data() + i, (int)std::min<size_t>(kReduceMulti, rs.size() - i), s));
    return SPNERF_OK;
}

// One skinny reduction over `rows` rows (points or rays) and the reductions of its slabs:
// out[m][k] = Σ_r A[r*lda+m] · B[r*ldb+k], written to dst (row-major, or dst[k][m] with
// `transpose`); dst_b[m] = Σ_r A[r][m]; dst_ones[k] = Σ_r B[r][k].
struct SkinnyJob {
    SkinnyArgs k;
    ReduceArgs r[2];
    int nr = 0;
    int64_t chunks = 0;
};
template <typename TB>
inline SkinnyJob skinny_job(const Ctx& c, int64_t rows, const float* A, int lda, int Ma, const TB* B, int ldb, int K,
                            float* dst, int ld_dst, int transpose, float* dst_b, float* dst_ones, float* slab,
                            float* slab_b) {
    SkinnyJob j;
    SkinnyArgs& k = j.k;
    k.A = A; k.lda = lda; k.Ma = Ma; k.ldb = ldb; k.K = K; k.P = rows; k.ones = dst_ones ? 1 : 0;
    if constexpr (std::is_same<TB, bf16>::value) k.B16 = B;
    else k.B = B;
    k.slab = slab; k.slab_b = slab_b;
    j.chunks = rows > 0 ? cdiv(rows, skinny_chunk(rows)) : 0;
    const int Mt = Ma + k.ones;
    ReduceArgs r = red(0, Ma, K, dst, ld_dst, dst_b);
    bind_slab(r, slab, Mt, K, (int)j.chunks, slab_b, c.acc);
    r.transpose = transpose;
    if (dst) j.r[j.nr++] = r;
    if (dst_ones) {
        ReduceArgs o = r;
        o.row0 = Ma; o.nrows = 1; o.dst = dst_ones; o.ld_dst = K; o.dst_b = nullptr; o.transpose = 0;
        j.r[j.nr++] = o;
    }
    return j;
}

// a launch of its own (tn_skinny + one reduction launch)
template <typename TB>
inline int32_t skinny(const Ctx& c, int64_t rows, const float* A, int lda, int Ma, const TB* B, int ldb, int K,
                      float* dst, int ld_dst, int transpose, float* dst_b, float* dst_ones, hipStream_t s) {
    const SkinnyJob j = skinny_job(c, rows, A, lda, Ma, B, ldb, K, dst, ld_dst, transpose, dst_b, dst_ones,
                                   c.at(c.w.sk_slab), c.at(c.w.sk_slab_b));
    SPN_TRY(tn_skinny(j.k, s));
    return reduce_slabs_multi(j.r, j.nr, s);
}
#pragma GCC visibility pop

// Skinny reductions with fp32 rows batched into ONE launch (tn_skinny_multi) plus one reduction
// launch per kReduceMulti outputs — the per-ray parameter gradients of a backward (step 7) were
// a dozen launches of a few microseconds of work each.  Same arithmetic as skinny().
struct SkinnyBatch {
    const Ctx& c;
    std::vector<SkinnyArgs> tasks;
    std::vector<ReduceArgs> reds;
    int64_t off = 0, off_b = 0;
    explicit SkinnyBatch(const Ctx& cc) : c(cc) {}
    template <typename TB>
    int32_t add(int64_t rows, const float* A, int lda, int Ma, const TB* B, int ldb, int K, float* dst, int ld_dst,
                int transpose, float* dst_b, float* dst_ones) {
        const SkinnyJob j = skinny_job(c, rows, A, lda, Ma, B, ldb, K, dst, ld_dst, transpose, dst_b, dst_ones,
                                       c.at(c.w.sk_slab) + off, c.at(c.w.sk_slab_b) + off_b);
        const int64_t n = j.chunks * (Ma + j.k.ones) * K, n_b = j.chunks * Ma;
        SPN_ARG(off + n <= c.w.sk_slab_n && off_b + n_b <= c.w.sk_slab_b_n && (int)tasks.size() < kSkinnyMulti,
                "skinny batch: slab capacity");
        off += n;
        off_b += n_b;
        tasks.push_back(j.k);
        for (int i = 0; i < j.nr; ++i) reds.push_back(j.r[i]);
        return SPNERF_OK;
    }
    int32_t run(hipStream_t s) {
        SPN_TRY(tn_skinny_multi(tasks.data(), (int)tasks.size(), s));
        for (size_t i = 0; i < reds.size(); i += kReduceMulti)
            SPN_TRY(reduce_slabs_multi(reds.data() + i, (int)std::min<size_t>(kReduceMulti, reds.size() - i), s));
        return SPNERF_OK;
    }
};

}  // namespace spn
