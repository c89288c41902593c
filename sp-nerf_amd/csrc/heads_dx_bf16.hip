// The training heads' dX chain in ONE persistent launch (bf16 MLP, W = 512, H = 256, no β) —
// the backward of models/spnerf.py:332-369 from the narrow heads' gradients to the trunk's top
// pre-activation gradient, a 128-point tile resident in ONE LDS image from the first GEMM to the last:
//
//   dS2  = (dS3 · Ws3) ⊙ DS2                     [256]   sun_v_net.4 → .2   (spnerf.py:358-360)
//   dZQs = (dS2 · Ws2) ⊙ DQ[:, :H]               [256]   sun_v_net.2 → .0
//   dF   = [dZQs | dZQ_rgb] · WQ                 [512]   Q = [sun_v.0 ; rgb.0] → feat (linear)
//   dZL  = ([dF | dZG_sem] · WG + dσ ⊗ w_σ) ⊙ D_L [512]  G = [feat ; semantic hidden] → H_L
//
// (the solar pass: K of Q = H, of G = W).  The layer-by-layer path runs these as four DMA GEMMs
// (k_gemm_nt_bf16d, two with the ×D epilogue, one with the rank-1 σ term), each writing its output
// to HBM and the next reading it back (≈ 3.5 KB per point of re-reads); here every intermediate
// stays in LDS and only what the weight gradients read (dS2, dZQ's sun half, dF) and dZL leave.
// The arithmetic is the GEMMs': the same 32x32x16 bf16 MFMAs over the K-steps of 16 in ascending
// order (weights and activations in swapped operand roles, as the fused forward heads), the
// epilogues' (acc + 0) [+ dσ·w_σ] [· D] in fp32, RNE to bf16 — bit for bit the GEMMs' outputs.
//
// The forward's 128-point geometry (512 threads, 4 point tiles per wave): one [128][512] bf16 image
// (128 KB), its column halves L = [0, 256) and R = [256, 512) taking turns as MFMA B operand and as
// the target of an IN-PLACE epilogue (a lane multiplies by, and overwrites, exactly its own 8-byte
// pieces, so the saved derivative needs no image of its own and no barrier of its own):
//   top   image ← [dS3 | DS2]
//   P1    dS3 (L) → R = dS2 (× DS2 in place);            L ← DQ_s once every wave has read dS3
//   P2    dS2 (R) → L = dZQs (× DQ_s in place); dS2 leaves;  R ← dZQ_rgb once every wave has read dS2
//   P3    dZQ (L | R) → the image = dF; dZQ's sun half leaves
//   P4    dF (k-steps 0..31: L then R, each half leaving while the k-loop reads it), then — a 768-wide
//         dZG does not fit one image — dZG_sem into L once every wave is past L's 16 k-steps, and
//         k-steps 32..47 from there; × D_L from the lane's own TILE-ORDERED fragments (trunk.h
//         dtile_off, as the saving trunk wrote them: two b128 loads per accumulator, whole KBs per
//         wave, no D image) → the image = dZL, which leaves before the next tile's top.
// Each row-major input is loaded into registers one phase ahead.  D_L's a = 0 half loads after P4's
// first 16 k-steps (into the registers dZG_sem has left) and rides through the rest of the k-loop,
// its a = 1 half after the k-loop into the registers bc / bn leave free (the dX chain's staging,
// k_trunk_bwd_bf16 T128).  The weights (transposed, fragment order: PackedOffs Bs3_16 / Bs2_16 /
// BQ16 / BG16) stream from L2 through a register ring as the A operand, the ring running on into
// the next phase's stream where both phases share it.
#include <algorithm>
#include <type_traits>

#include "heads_dx.h"
#include "trunk.h"

namespace spn {

// option "fused_heads_bwd": 1 (default) = this launch where the shape fits and the forward wrote D_L
// tile-ordered; 0 = the four GEMMs
int g_fused_heads_bwd = 1;
// read-back (option "heads_bwd_path"): or-ed since last zeroed, 1 = the fused launch ran, 2 = the four GEMMs
int g_heads_bwd_path = 0;

namespace hx {

constexpr int TM = 128;                // points per tile
constexpr int NJ = TM / 32;            // 32-point MFMA tiles per wave
constexpr int IMG = TM * 1024;         // the [128][512] bf16 image
constexpr int HW = 512, HH = 256;
constexpr int D1 = 8, D2 = 4;          // weight-ring depths of the 256-wide (NA 1) and 512-wide (NA 2) layers
constexpr int LDS_BYTES = IMG + (HW + 2 * TM) * 4;
static_assert(LDS_BYTES <= 160 * 1024, "the image, w_σ and two tiles' dσ in 160 KB of LDS");
static_assert(TM == 2 * kDtileRows, "a tile is two adjacent blocks of the tile-ordered D_L");
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int img_off(int row, int ch) { return row * 1024 + ((ch ^ (row & 15)) << 4); }
// the 8-byte piece of 4 consecutive features f0.. (f0 % 4 == 0) of one row
__device__ __forceinline__ int img4(int row, int f0) { return img_off(row, f0 >> 3) + 8 * ((f0 >> 2) & 1); }

template <int NA, int DEPTH>
__device__ __forceinline__ void prime(const bf16* __restrict__ wsrc, u32x4 (&ring)[DEPTH][NA]) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
        for (int a = 0; a < NA; ++a) ring[d][a] = ldg16(wsrc + (d * NA + a) * 512);
}

// acc[a][j] += Σ W-fragment(ks) · image columns over the k-steps [ks_begin, ks_end) of this wave's
// stream wsrc (nks k-steps of NA fragments of 512 bf16), k-step ks reading the image's k-step
// ks + kk_shift.  The ring holds the stream's next DEPTH k-steps on entry and on exit; past the
// stream's end it runs on into wnext's first DEPTH k-steps (null: the last slice again, unused).
// drain(group) runs after the refills of each group of DEPTH k-steps (group = ks / DEPTH).
template <int NA, int DEPTH, typename Drain>
__device__ __forceinline__ void kloop(const bf16* __restrict__ wsrc, const bf16* __restrict__ wnext, int ks_begin, int ks_end,
                                      int nks, int kk_shift, const char* img, int lane, f32x16 (&acc)[NA][NJ],
                                      u32x4 (&ring)[DEPTH][NA], Drain&& drain) {
    const int r32 = lane & 31, h = lane >> 5, sw = r32 & 15;
    const char* brow = img + r32 * 1024;
#pragma unroll 1
    for (int ks0 = ks_begin; ks0 < ks_end; ks0 += DEPTH) {
        const int kk0 = ks0 + kk_shift;
        const bf16* rsrc = ks0 + DEPTH < nks ? wsrc + (ks0 + DEPTH) * NA * 512 : (wnext ? wnext : wsrc + (nks - DEPTH) * NA * 512);
        bf16x8 bc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bc[j] = *reinterpret_cast<const bf16x8*>(brow + j * 32768 + (((2 * kk0 + h) ^ sw) << 4));
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            const int kk = kk0 + d;
            bf16x8 bn[NJ];
            if (d + 1 < DEPTH) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) bn[j] = *reinterpret_cast<const bf16x8*>(brow + j * 32768 + (((2 * (kk + 1) + h) ^ sw) << 4));
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int a = 0; a < NA; ++a)
                    acc[a][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ring[d][a]), bc[j], acc[a][j], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < NA; ++a) ring[d][a] = ldg16(rsrc + (d * NA + a) * 512);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, NA, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x020, NA, 0);
            if (d + 1 < DEPTH) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) bc[j] = bn[j];
            }
        }
        drain(ks0 / DEPTH);
    }
}

template <int NA>
__device__ __forceinline__ void zero(f32x16 (&acc)[NA][NJ]) {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][j][r] = 0.f;
}

}  // namespace hx

using namespace hx;

__global__ __launch_bounds__(512) void k_heads_dx128_bf16(HeadsDxArgs g, int ntiles) {
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    float* const wsg = reinterpret_cast<float*>(smem + IMG);  // w_σ [512]
    float* const hs0 = wsg + HW;   // the tile's dσ [128], double-buffered by tile parity (the next tile's top
                                   // writes its rows while slower waves still read this tile's)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool full = g.mode == 0, semk = full && g.sem;
    const int nksQ = full ? g.kQ / 16 : HH / 16;   // Q's K: [sun_v.0 | rgb.0] or sun_v.0 alone
    const int nksG = semk ? g.kG / 16 : HW / 16;   // G's K: [feat | semantic hidden] or feat alone
    // this wave's weight streams, computed where they are used (opaque: not kept live, nor the lane
    // addresses derived from them, across the phases)
    auto wstream = [&](int64_t off, int nksw, int na) { return g.packed16 + off + (int64_t)w * nksw * na * 512 + opaque(lane) * 8; };
    auto s3f = [&]() { return wstream(g.Bs3, HH / 16, 1); };
    auto s2f = [&]() { return wstream(g.Bs2, HH / 16, 1); };
    auto sqf = [&]() { return wstream(g.BQ, g.kQ / 16, 2); };
    auto sgf = [&]() { return wstream(g.BG, g.kG / 16, 2); };
    for (int i = tid; i < HW; i += 512) wsg[i] = g.wsig[i];

    // the tile's rows of a [P][ld] bf16 tensor as a buffer resource: rows past P are dropped by the
    // hardware (stores), loads read a clamped row; off (or a null base): an empty resource, every
    // access dropped — no branch around a load or a store, whose vmcnt accounting would make the
    // later weight-refill waits wait for everything in flight
    auto rsrc = [&](const bf16* base, int ld, int64_t p0, bool on) {
        const int rows = (int)std::min<int64_t>(TM, g.P - p0);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(base ? base + p0 * ld : g.dZL), 0,
                                                 base && on ? rows * ld * 2 : 0, 0x00020000);
    };
    // chunk c (16 B) of the tile's rows from column c0, NCH chunks per row
    auto ld_rows = [&](__amdgpu_buffer_rsrc_t rs, int ld, int c0, int64_t p0, int nch, int c) -> u32x4 {
        const int rows = (int)std::min<int64_t>(TM, g.P - p0);
        const int row = std::min(c / nch, rows - 1), ch = c % nch;
        return __builtin_amdgcn_raw_buffer_load_b128(rs, (row * ld + c0 + ch * 8) * 2, 0, 3);
    };
    // image columns [8·ch0, 8·(ch0 + nch)) to columns [c0, ..) of the rows: chunks q0 .. q0 + n of this thread
    auto out_rows = [&](__amdgpu_buffer_rsrc_t rs, int ld, int c0, int ch0, int nch, int q0, auto kn) {
        constexpr int n = decltype(kn)::value;
        const int t = opaque(tid);
        u32x4 v[n];
#pragma unroll
        for (int q = 0; q < n; ++q) {
            const int c = t + 512 * (q0 + q), row = c / nch, ch = c % nch;
            v[q] = *reinterpret_cast<const u32x4*>(smem + img_off(row, ch0 + ch));
        }
#pragma unroll
        for (int q = 0; q < n; ++q) {
            const int c = t + 512 * (q0 + q), row = c / nch, ch = c % nch;
            __builtin_amdgcn_raw_buffer_store_b128(v[q], rs, (row * ld + c0 + ch * 8) * 2, 0, 3);
        }
    };
    // 8 register chunks per thread into an image half (32 chunks per row from chunk ch0)
    auto stage_half = [&](const u32x4 (&r)[8], int ch0) {
        const int t = opaque(tid);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int c = t + 512 * q;
            *reinterpret_cast<u32x4*>(smem + img_off(c >> 5, ch0 + (c & 31))) = r[q];
        }
    };
    const std::integral_constant<int, 1> K1{};
    const std::integral_constant<int, 2> K2{};
    const std::integral_constant<int, 4> K4{};

    int tile = xcd_remap(blockIdx.x, gridDim.x);
    if (tile >= ntiles) return;  // block-uniform
    // the next tile's [dS3 | DS2] rows (128 rows x 64 chunks: 16 per thread)
    u32x4 rA[16];
    auto load_top = [&](int64_t q0) {
        const auto r3 = rsrc(g.dS3, HH, q0, true), rD = rsrc(g.DS2, HH, q0, true);
        const int t = opaque(tid);
#pragma unroll
        for (int q = 0; q < 8; ++q) {   // chunk c & 31 of row c >> 5: rA[q] from dS3 (L), rA[8 + q] from DS2 (R)
            rA[q] = ld_rows(r3, HH, 0, q0, 32, t + 512 * q);
            rA[8 + q] = ld_rows(rD, HH, 0, q0, 32, t + 512 * q);
        }
    };
    load_top((int64_t)tile * TM);
    u32x4 ring1[D1][1];
    prime<1, D1>(s3f(), ring1);
    for (int it = 0; tile < ntiles; tile += gridDim.x, ++it) {
        const int64_t p0 = (int64_t)tile * TM;
        float* const hs = hs0 + (it & 1) * TM;
        const int64_t next = std::min(tile + (int)gridDim.x, ntiles - 1);
        {
            const int t = opaque(tid);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int c = t + 512 * (q & 7);
                *reinterpret_cast<u32x4*>(smem + img_off(c >> 5, (q >> 3) * 32 + (c & 31))) = rA[q];
            }
            if (t < TM) hs[t] = g.hpre[std::min<int64_t>(p0 + t, g.P - 1) * g.HP];
        }
        __syncthreads();  // the image = [dS3 | DS2]
        // ---- P1: dS2 = (dS3 · Ws3) ⊙ DS2, in place over DS2 (R); L ← DQ_s
        {
            u32x4 rq[8];
            const auto rsQ = rsrc(g.DQ, g.ldQ, p0, true);
#pragma unroll
            for (int q = 0; q < 8; ++q) rq[q] = ld_rows(rsQ, g.ldQ, 0, p0, 32, opaque(tid) + 512 * q);
            f32x16 acc[1][NJ];
            zero<1>(acc);
            kloop<1, D1>(s3f(), s2f(), 0, HH / 16, HH / 16, 0, smem, opaque(lane), acc, ring1, [&](int) {});
            __syncthreads();  // every wave is done reading dS3 (L)
            const int el = opaque(lane), er32 = el & 31, eh = el >> 5;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int f0 = 32 * w + 8 * gq + 4 * eh, row = 32 * j + er32;
                    char* const o = smem + img4(row, HH + f0);
                    const f32x4 m = ld4(reinterpret_cast<const bf16*>(o));
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (acc[0][j][4 * gq + e] + 0.f) * m[e];
                    *reinterpret_cast<u32x2*>(o) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
                }
            stage_half(rq, 0);
        }
        __syncthreads();  // the image = [DQ_s | dS2]
        // ---- P2: dZQs = (dS2 · Ws2) ⊙ DQ_s, in place over DQ_s (L); dS2 leaves; R ← dZQ_rgb
        u32x4 ring2[D2][2];
        {
            u32x4 rr[8];
            const auto rsR = rsrc(g.dZQ, g.ldQ, p0, full);
#pragma unroll
            for (int q = 0; q < 8; ++q) rr[q] = ld_rows(rsR, g.ldQ, HH, p0, 32, opaque(tid) + 512 * q);
            f32x16 acc[1][NJ];
            zero<1>(acc);
            const auto rsS2 = rsrc(g.dS2, HH, p0, true);
            // 8 chunks per thread over the 2 k-step groups
            kloop<1, D1>(s2f(), nullptr, 0, HH / 16, HH / 16, HH / 16, smem, opaque(lane), acc, ring1,
                         [&](int grp) { out_rows(rsS2, HH, 0, 32, 32, 4 * grp, K4); });
            prime<2, D2>(sqf(), ring2);
            const int el = opaque(lane), er32 = el & 31, eh = el >> 5;
            // in place over L, which no k-step of this phase reads
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int f0 = 32 * w + 8 * gq + 4 * eh, row = 32 * j + er32;
                    char* const o = smem + img4(row, f0);
                    const f32x4 m = ld4(reinterpret_cast<const bf16*>(o));
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (acc[0][j][4 * gq + e] + 0.f) * m[e];
                    *reinterpret_cast<u32x2*>(o) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
                }
            __syncthreads();  // every wave is done reading dS2 (R), its copy-out included
            if (full) stage_half(rr, 32);  // block-uniform
        }
        __syncthreads();  // the image = [dZQs | dZQ_rgb]
        // ---- P3: dF = dZQ · WQ → the image; dZQ's sun half leaves
        u32x4 rs[8];
        {
            f32x16 acc[2][NJ];
            zero<2>(acc);
            const auto rsQ = rsrc(g.dZQ, g.ldQ, p0, true);
            // 8 chunks per thread over the nksQ / D2 = 8 (solar pass: 4) k-step groups
            if (full)
                kloop<2, D2>(sqf(), sgf(), 0, nksQ, nksQ, 0, smem, opaque(lane), acc, ring2, [&](int grp) { out_rows(rsQ, g.ldQ, 0, 0, 32, grp, K1); });
            else
                kloop<2, D2>(sqf(), sgf(), 0, nksQ, nksQ, 0, smem, opaque(lane), acc, ring2, [&](int grp) { out_rows(rsQ, g.ldQ, 0, 0, 32, 2 * grp, K2); });
            // dZG's semantic half (row-major [:, W:]) rides through the epilogue and P4's first 16 k-steps
            const auto rsS = rsrc(g.dZG, g.ldG, p0, semk);
#pragma unroll
            for (int q = 0; q < 8; ++q) rs[q] = ld_rows(rsS, g.ldG, HW, p0, 32, opaque(tid) + 512 * q);
            __syncthreads();  // every wave is done reading dZQ, its copy-out included
            const int el = opaque(lane), er32 = el & 31, eh = el >> 5;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int f0 = 64 * w + 32 * a + 8 * gq + 4 * eh, row = 32 * j + er32;
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[a][j][4 * gq + e] + 0.f;
                        *reinterpret_cast<u32x2*>(smem + img4(row, f0)) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
                    }
        }
        __syncthreads();  // the image = dF
        // ---- P4: dZL = ([dF | dZG_sem] · WG + dσ ⊗ w_σ) ⊙ D_L → the image; dF leaves
        {
            f32x16 acc[2][NJ];
            zero<2>(acc);
            const auto rsF = rsrc(g.dZG, g.ldG, p0, true);
            // the lane's fragments of D_L's feature tile a (dh[2j + q]: half q of accumulator (a, j))
            // through a resource over the tile's two blocks — round_up(P, 64) rows are allocated, so
            // a last tile's absent block reads as dropped, a partial block from the buffer's padding
            const int64_t pad = (g.P + kDtileRows - 1) / kDtileRows * kDtileRows;
            const __amdgpu_buffer_rsrc_t rsD = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<bf16*>(g.DL) + p0 * HW, 0, (int)std::min<int64_t>(TM, pad - p0) * HW * 2, 0x00020000);
            auto load_dh = [&](u32x4 (&dh)[2 * NJ], int a) {
                const int base = dtile_frag_off(w, a, 0, 0, opaque(lane));
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        dh[2 * j + q] = __builtin_amdgcn_raw_buffer_load_b128(
                            rsD, (j >> 1) * kDtileBlockBytes + dtile_frag_off(0, 0, j & 1, q, 0) + base, 0, 3);
            };
            // dF's L half under k-steps 0..15, its R half under 16..31: 8 chunks per thread each, 2 per group
            const bf16* const sg = sgf();
            kloop<2, D2>(sg, nullptr, 0, HH / 16, nksG, 0, smem, opaque(lane), acc, ring2,
                         [&](int grp) { out_rows(rsF, g.ldG, 0, 0, 32, 2 * grp, K2); });
            if (semk) {  // block-uniform
                __syncthreads();  // every wave is past dF's L half, its copy-out included
                stage_half(rs, 0);
            }
            u32x4 d0[2 * NJ];
            load_dh(d0, 0);
            kloop<2, D2>(sg, nullptr, HH / 16, HW / 16, nksG, 0, smem, opaque(lane), acc, ring2,
                         [&](int grp) { out_rows(rsF, g.ldG, HH, 32, 32, 2 * (grp - HH / 16 / D2), K2); });
            if (semk) {
                __syncthreads();  // L = dZG_sem
                kloop<2, D2>(sg, nullptr, HW / 16, nksG, nksG, -HW / 16, smem, opaque(lane), acc, ring2, [&](int) {});
            }
            u32x4 d1[2 * NJ];
            load_dh(d1, 1);
            __syncthreads();  // every wave is done reading the image, dF's copy-out included
            const int el = opaque(lane), er32 = el & 31, eh = el >> 5;
            auto half = [&](const u32x4 (&dh)[2 * NJ], int a) {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int f0 = 64 * w + 32 * a + 8 * gq + 4 * eh;
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(wsg + f0);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int row = 32 * j + er32;
                        const u32x4 dq = dh[2 * j + (gq >> 1)];
                        const f32x4 m = raw_f32(u32x2{dq[(gq & 1) * 2], dq[(gq & 1) * 2 + 1]});
                        const float hv = hs[row];
                        float v[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            v[e] = acc[a][j][4 * gq + e] + 0.f;
                            v[e] += hv * wv[e];
                            v[e] *= m[e];
                        }
                        *reinterpret_cast<u32x2*>(smem + img4(row, f0)) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            half(d0, 0);
            half(d1, 1);
        }
        // the next tile's [dS3 | DS2] rows (past the last tile: this tile's rows again, never used) and
        // its P1 stream, ahead of this tile's last copy-out
        load_top(next * TM);
        prime<1, D1>(s3f(), ring1);
        __syncthreads();  // the image = dZL
        {
            const auto rsL = rsrc(g.dZL, HW, p0, true);
#pragma unroll
            for (int q0 = 0; q0 < 16; q0 += 4) out_rows(rsL, HW, 0, 0, 64, q0, K4);
        }
        __syncthreads();  // the next tile restages the image
    }
}

bool heads_dx_bf16_ok(const HeadsDxArgs& a) {
    return a.packed16 && a.Bs3 >= 0 && a.Bs2 >= 0 && a.BQ >= 0 && a.BG >= 0 && (a.mode == 0 || a.mode == 2) &&
           a.kQ == 2 * HH && a.kG == (a.sem ? HW + HH : HW) && a.ldQ == a.kQ && a.ldG == a.kG && a.dS3 && a.DS2 && a.DQ &&
           a.dS2 && a.dZQ && a.dZG && a.dZL && a.DL && a.hpre && a.wsig && a.dl_tiled;
}

int32_t heads_dx_bf16(const HeadsDxArgs& a, hipStream_t s, double flop, double bytes) {
    SPN_ARG(heads_dx_bf16_ok(a), "heads_dx_bf16: bad arguments (the launch reads a tile-ordered D_L)");
    if (a.P == 0) return SPNERF_OK;
    SPN_ARG(a.P < (1ll << 31) / (HW + HH), "heads_dx_bf16: too many points (%lld)", (long long)a.P);
    const int ntiles = cdiv(a.P, TM);
    ProfScope prof("heads_dx", s, flop, bytes);
    g_heads_bwd_path |= 1;
    hipLaunchKernelGGL(k_heads_dx128_bf16, dim3(std::min(ntiles, num_cus())), dim3(512), 0, s, a, ntiles);
    SPN_HIP(hipGetLastError());
    return SPNERF_OK;
}

}  // namespace spn
