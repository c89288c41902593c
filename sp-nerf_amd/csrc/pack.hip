// Re-packing the model's parameters into the layouts the kernels read (mlp_layout.h Packed): the
// pack kernels, the device-resident piece tables, and spnerf_pack_params with the parameter queries.
#include <cstring>
#include <deque>
#include <mutex>
#include <vector>

#include "common.h"
#include "gemm_f32.h"
#include "mlp_layout.h"
#include "mlp_options.h"
#include "trunk.h"

namespace spn {

struct PackPiece {
    const float* src;
    // bf: 1 = bf16 destination (dst in bf16 units); 2 = bf16 in the fused trunk's MFMA fragment
    // order (trunk_frag_off, dst_ld = the layer's padded K; transposed: element [c][r]); 5 = the same for 32 features per
    // wave (frag_off NA = 1: the fused heads' 256-wide layers); 7 = frag_off NA = 2 (64 features per wave; the
    // heads' dX chain, transposed only); 3 = split into bf16 planes
    // [hi | hi | lo | lo] of width dst_ld / 4 each (hi = bf16(v), lo = bf16(v − hi)); 4 = the
    // same planes in the fused trunk's fragment order (dst_ld = 4·K0p); 6 = a narrow head's
    // [32][cols] hi/lo-row A operand (PackedOffs::Fnar16; rows = 32, nsrc source rows)
    int src_ld, src_c0, rows, cols, dst_ld, transpose, bf;
    int src_idx;   // the parameter's index (device-resident tables: src comes from PackSrcs)
    int64_t dst;
    int nsrc = 0;  // bf = 6: source rows
    int rnd = 0;   // fp32 destination rounded to bf16 (precision study, option emu_bf16 & 4)
};
static_assert(sizeof(PackPiece) == 56, "PackArgs must stay within the 4 KB kernel-argument segment");
constexpr int kPackParams = 64;
struct PackSrcs {
    const float* p[kPackParams];
};
constexpr int kMaxPieces = 64;
constexpr int kPackTR = 32, kPackTC = 64;  // a block re-lays one 32 x 64 tile of a piece
struct PackArgs {
    PackPiece p[kMaxPieces];
    int tile0[kMaxPieces + 1];  // prefix of the pieces' tile counts (block ranges)
    int n;
    float* packed;
};

// One launch for up to kMaxPieces pieces: block b re-lays tile (b - tile0[piece]) of its piece,
// 8 elements per thread.  Transposed pieces (fp32 or bf16) go through an LDS tile so both the
// read (rows of the source) and the write (rows of the transpose) are coalesced.
// block b re-lays tile t of piece pc into packed
__device__ __forceinline__ void pack_block(const PackPiece pc, int t, float* packed) {
    __shared__ float tileT[kPackTC][kPackTR + 1];
    const int tcols = (pc.cols + kPackTC - 1) / kPackTC;
    const int r0 = (t / tcols) * kPackTR, c0 = (t % tcols) * kPackTC;
    const int tid = threadIdx.x;
    if (pc.transpose && (pc.bf <= 2 || pc.bf == 5 || pc.bf == 7)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int rr = (tid >> 6) + 4 * e, cc = tid & 63;
            const int r = r0 + rr, c = c0 + cc;
            tileT[cc][rr] = (r < pc.rows && c < pc.cols) ? pc.src[(int64_t)r * pc.src_ld + pc.src_c0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int rr = tid & 31, cc = (tid >> 5) + 8 * e;
            const int r = r0 + rr, c = c0 + cc;
            if (r < pc.rows && c < pc.cols) {
                const int64_t o = pc.dst + (pc.bf == 2   ? trunk_frag_off(c, r, pc.dst_ld)
                                            : pc.bf == 5 ? frag_off(c, r, pc.dst_ld, 1)
                                            : pc.bf == 7 ? frag_off(c, r, pc.dst_ld, 2)
                                                         : (int64_t)c * pc.dst_ld + r);
                if (pc.bf) reinterpret_cast<bf16*>(packed)[o] = (bf16)tileT[cc][rr];
                else packed[o] = pc.rnd ? (float)(bf16)tileT[cc][rr] : tileT[cc][rr];
            }
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int r = r0 + (tid >> 6) + 4 * e, c = c0 + (tid & 63);
        if (r >= pc.rows || c >= pc.cols) continue;
        if (pc.bf == 6) {  // destination row r: source row sr's hi (r even) or lo (r odd) plane
            const int sr = r < 2 ? 0 : r < 4 ? 1 : (r == 8 || r == 9) ? 2 : -1;
            bf16 o = (bf16)0.f;
            if (sr >= 0 && sr < pc.nsrc) {
                const float v = pc.src[(int64_t)sr * pc.src_ld + pc.src_c0 + c];
                const bf16 hi = (bf16)v;
                o = (r & 1) ? (bf16)(v - (float)hi) : hi;
            }
            reinterpret_cast<bf16*>(packed)[pc.dst + frag_off(r, c, pc.dst_ld, 1)] = o;
            continue;
        }
        const float v = pc.src[(int64_t)r * pc.src_ld + pc.src_c0 + c];
        if (pc.bf == 3 || pc.bf == 4) {
            bf16* dst = reinterpret_cast<bf16*>(packed) + pc.dst;
            const int kp = pc.dst_ld / 4;
            const bf16 hi = (bf16)v, lo = (bf16)(v - (float)hi);
            const bf16 pl[4] = {hi, hi, lo, lo};
            for (int j = 0; j < 4; ++j)
                dst[pc.bf == 4 ? trunk_frag_off(r, c + j * kp, pc.dst_ld) : (int64_t)r * pc.dst_ld + c + j * kp] = pl[j];
            continue;
        }
        const int64_t o = pc.dst + (pc.bf == 2        ? trunk_frag_off(r, c, pc.dst_ld)
                                    : pc.bf == 5   ? frag_off(r, c, pc.dst_ld, 1)
                                    : pc.transpose ? (int64_t)c * pc.dst_ld + r
                                                   : (int64_t)r * pc.dst_ld + c);
        if (pc.bf) reinterpret_cast<bf16*>(packed)[o] = (bf16)v;
        else packed[o] = pc.rnd ? (float)(bf16)v : v;
    }
}

__global__ __launch_bounds__(256) void k_pack(PackArgs a) {
    const int b = blockIdx.x;
    int pi = 0;
    while (pi + 1 < a.n && a.tile0[pi + 1] <= b) ++pi;  // block-uniform
    pack_block(a.p[pi], b - a.tile0[pi], a.packed);
}

// The same for a piece table resident in device memory (pack_table: one launch for any number
// of pieces — the bf16 MLP's ~90 pieces took two kernarg-table launches per re-pack).  blk[b] =
// {piece, tile} of block b, one load (a binary search over the tile prefix was 7 dependent loads
// ahead of every block's work: 24 us per re-pack)
__global__ __launch_bounds__(256) void k_pack_dev(const PackPiece* __restrict__ pcs, const int2* __restrict__ blk,
                                                  float* packed, PackSrcs srcs) {
    const int2 bt = blk[blockIdx.x];
    PackPiece pc = pcs[bt.x];
    pc.src = srcs.p[pc.src_idx];
    pack_block(pc, bt.y, packed);
}

// Device-resident piece tables, one per distinct model layout (the parameters' addresses go in
// the launch's kernarg PackSrcs, so every model of one configuration shares a table), built on
// first use outside a stream capture and never freed (a captured graph may hold one); option
// pack_table 0 = the kernarg tables only
int g_pack_table = 1;
struct PackTable {
    int dev;
    std::vector<PackPiece> key;
    PackPiece* d_pcs;
    int2* d_blk;   // per block: {piece, tile of the piece}
    int tiles;
};
static std::mutex g_pack_mu;
static std::deque<PackTable> g_pack_tables;   // deque: the returned pointers stay valid

static const PackTable* pack_table(const std::vector<PackPiece>& pieces0, hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::vector<PackPiece> pieces = pieces0;   // the key: layout only
    for (PackPiece& p : pieces) {
        if (p.src_idx < 0 || p.src_idx >= kPackParams) return nullptr;
        p.src = nullptr;
    }
    std::lock_guard<std::mutex> lk(g_pack_mu);
    for (const PackTable& t : g_pack_tables)
        if (t.dev == dev && t.key.size() == pieces.size() &&
            std::memcmp(t.key.data(), pieces.data(), pieces.size() * sizeof(PackPiece)) == 0)
            return &t;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    if (g_pack_tables.size() >= 64) return nullptr;
    std::vector<int2> blk;
    for (size_t i = 0; i < pieces.size(); ++i) {
        const int nt = cdiv(pieces[i].rows, kPackTR) * cdiv(pieces[i].cols, kPackTC);
        for (int t = 0; t < nt; ++t) blk.push_back(make_int2((int)i, t));
    }
    if (blk.empty()) return nullptr;
    PackTable t{dev, pieces, nullptr, nullptr, (int)blk.size()};
    if (hipMalloc(&t.d_pcs, pieces.size() * sizeof(PackPiece)) != hipSuccess) return nullptr;
    if (hipMalloc(&t.d_blk, blk.size() * sizeof(int2)) != hipSuccess ||
        hipMemcpy(t.d_pcs, pieces.data(), pieces.size() * sizeof(PackPiece), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(t.d_blk, blk.data(), blk.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(t.d_pcs);
        if (t.d_blk) (void)hipFree(t.d_blk);
        return nullptr;
    }
    g_pack_tables.push_back(t);
    return &g_pack_tables.back();
}

static int32_t launch_pack(const std::vector<PackPiece>& pieces, float* packed, hipStream_t s) {
    if (g_pack_table && pieces.size() > (size_t)kMaxPieces) {
        if (const PackTable* t = pack_table(pieces, s)) {
            PackSrcs srcs{};
            for (const PackPiece& p : pieces) srcs.p[p.src_idx] = p.src;
            ProfScope prof("pack", s, 0.0, 0.0);
            hipLaunchKernelGGL(k_pack_dev, dim3(t->tiles), dim3(256), 0, s, t->d_pcs, t->d_blk, packed, srcs);
            SPN_HIP(hipGetLastError());
            return SPNERF_OK;
        }
    }
    for (size_t b = 0; b < pieces.size(); b += kMaxPieces) {
        PackArgs a{};
        a.packed = packed;
        int n = 0, tiles = 0;
        for (size_t i = b; i < pieces.size() && n < kMaxPieces; ++i, ++n) {
            a.p[n] = pieces[i];
            a.tile0[n] = tiles;
            tiles += cdiv(pieces[i].rows, kPackTR) * cdiv(pieces[i].cols, kPackTC);
        }
        a.tile0[n] = tiles;
        a.n = n;
        ProfScope prof("pack", s, 0.0, 0.0);
        hipLaunchKernelGGL(k_pack, dim3(tiles), dim3(256), 0, s, a);
        SPN_HIP(hipGetLastError());
    }
    return SPNERF_OK;
}

static int32_t pack_params(const Dims& d, const float* const* prm, float* packed, hipStream_t s) {
    PIdx x;
    auto specs = param_specs(d, &x);
    const Packed k = packed_layout(d);
    std::vector<PackPiece> v;
    auto piece = [&](int pi, int c0, int rows, int cols, int64_t dst, int dst_ld, int tr, int bf = 0) {
        SPN_ARG(prm[pi] != nullptr, "parameter %s is NULL", specs[pi].name.c_str());
        v.push_back(PackPiece{prm[pi], (int)specs[pi].ld(), c0, rows, cols, dst_ld, tr, bf, pi, dst});
        return SPNERF_OK;
    };
    const int W = d.W, H = d.H;
    // precision study: the fp32 MLP's GEMM weights rounded to bf16 (as the bf16 MLP packs them)
    const bool rnd16 = !d.bf && (g_emu_bf16 & 4);
    auto mark = [&]() { v.back().rnd = rnd16 ? 1 : 0; };
    for (int i = 0; i < d.L; ++i) {
        const int kreal = i == 0 ? d.K0 : (i == d.skip ? W + d.K0 : W);
        SPN_TRY(piece(x.fcW[i], 0, W, kreal, k.Wt[i], k.Kp[i], 0));
        if (i > 0) mark();
        SPN_TRY(piece(x.fcb[i], 0, 1, W, k.bt[i], W, 0));
        if (i > 0) {
            SPN_TRY(piece(x.fcW[i], 0, W, W, k.WTt[i], W, 1));
            mark();
        }
    }
    if (d.sem) {
        SPN_TRY(piece(x.fcW[0], d.K0, W, d.sd, k.Wsem0, d.sd, 0));
        SPN_TRY(piece(x.fcW[d.skip], W + d.K0, W, d.sd, k.Wsem4, d.sd, 0));
        SPN_TRY(piece(x.emb, 0, d.C + 1, d.sd, k.emb, d.sd, 0));
        SPN_TRY(piece(x.m1W, 0, H, W, k.WG + (int64_t)W * W, W, 0));
        mark();
        SPN_TRY(piece(x.m1b, 0, 1, H, k.bG + W, H, 0));
        SPN_TRY(piece(x.m1W, 0, H, W, k.WGT + W, d.NG, 1));
        mark();
        SPN_TRY(piece(x.m2W, 0, d.C, H, k.Wm2, H, 0));
        SPN_TRY(piece(x.m2b, 0, 1, d.C, k.bm2, d.C, 0));
    }
    SPN_TRY(piece(x.featW, 0, W, W, k.WG, W, 0));
    mark();
    SPN_TRY(piece(x.featb, 0, 1, W, k.bG, W, 0));
    SPN_TRY(piece(x.featW, 0, W, W, k.WGT, d.NG, 1));
    mark();
    SPN_TRY(piece(x.s1W, 0, H, W, k.WQ, W, 0));
    mark();
    SPN_TRY(piece(x.r1W, 0, H, W, k.WQ + (int64_t)H * W, W, 0));
    mark();
    SPN_TRY(piece(x.s1b, 0, 1, H, k.bQ, H, 0));
    SPN_TRY(piece(x.r1b, 0, 1, H, k.bQ + H, H, 0));
    SPN_TRY(piece(x.s1W, 0, H, W, k.WQT, d.NQ, 1));
    mark();
    SPN_TRY(piece(x.r1W, 0, H, W, k.WQT + H, d.NQ, 1));
    mark();
    SPN_TRY(piece(x.s1W, W, H, 3, k.Wsun, 3, 0));
    if (d.beta) {
        SPN_TRY(piece(x.b1W, 0, H, W, k.WQ + (int64_t)2 * H * W, W, 0));
        SPN_TRY(piece(x.b1b, 0, 1, H, k.bQ + 2 * H, H, 0));
        SPN_TRY(piece(x.b1W, 0, H, W, k.WQT + 2 * H, d.NQ, 1));
        SPN_TRY(piece(x.b1W, W, H, d.td, k.Wtt, d.td, 0));
        SPN_TRY(piece(x.b2W, 0, 1, H, k.wb2, H, 0));
        SPN_TRY(piece(x.b2b, 0, 1, 1, k.bb2, 1, 0));
    }
    SPN_TRY(piece(x.s2W, 0, H, H, k.Ws2, H, 0));
    mark();
    SPN_TRY(piece(x.s2b, 0, 1, H, k.bs2, H, 0));
    SPN_TRY(piece(x.s2W, 0, H, H, k.Ws2T, H, 1));
    mark();
    SPN_TRY(piece(x.s3W, 0, H, H, k.Ws3, H, 0));
    mark();
    SPN_TRY(piece(x.s3b, 0, 1, H, k.bs3, H, 0));
    SPN_TRY(piece(x.s3W, 0, H, H, k.Ws3T, H, 1));
    mark();
    SPN_TRY(piece(x.sigW, 0, 1, W, k.wsig, W, 0));
    SPN_TRY(piece(x.sigb, 0, 1, 1, k.bsig, 1, 0));
    SPN_TRY(piece(x.r2W, 0, 3, H, k.Wr2, H, 0));
    SPN_TRY(piece(x.r2b, 0, 1, 3, k.br2, 3, 0));
    SPN_TRY(piece(x.s4W, 0, 1, H, k.ws4, H, 0));
    SPN_TRY(piece(x.s4b, 0, 1, 1, k.bs4, 1, 0));
    SPN_TRY(piece(x.k1W, 0, H, 3, k.Wk1, 3, 0));
    SPN_TRY(piece(x.k1b, 0, 1, H, k.bk1, H, 0));
    SPN_TRY(piece(x.k2W, 0, 3, H, k.Wk2, H, 0));
    SPN_TRY(piece(x.k2b, 0, 1, 3, k.bk2, 3, 0));
    if (d.bf) {  // bf16 GEMM operands (same shapes as their fp32 counterparts above)
        SPN_TRY(piece(x.fcW[0], 0, W, d.K0, k.W0s16, 4 * k.Kp[0], 0, 3));
        if (k.Wf16[0] >= 0) SPN_TRY(piece(x.fcW[0], 0, W, d.K0, k.Wf16[0], 4 * k.Kp[0], 0, 4));
        for (int i = 1; i < d.L; ++i) {
            const int kreal = i == d.skip ? W + d.K0 : W;
            SPN_TRY(piece(x.fcW[i], 0, W, kreal, k.Wt16[i], k.Kp[i], 0, 1));
            SPN_TRY(piece(x.fcW[i], 0, W, W, k.WTt16[i], W, 1, 1));
            if (k.Wf16[i] >= 0) SPN_TRY(piece(x.fcW[i], 0, W, kreal, k.Wf16[i], k.Kp[i], 0, 2));
            if (k.Wb16[i] >= 0) SPN_TRY(piece(x.fcW[i], 0, W, W, k.Wb16[i], W, 1, 2));
        }
        if (d.sem) {
            SPN_TRY(piece(x.m1W, 0, H, W, k.WG16 + (int64_t)W * W, W, 0, 1));
            SPN_TRY(piece(x.m1W, 0, H, W, k.WGT16 + W, d.NG, 1, 1));
        }
        SPN_TRY(piece(x.featW, 0, W, W, k.WG16, W, 0, 1));
        SPN_TRY(piece(x.featW, 0, W, W, k.WGT16, d.NG, 1, 1));
        SPN_TRY(piece(x.s1W, 0, H, W, k.WQ16, W, 0, 1));
        SPN_TRY(piece(x.r1W, 0, H, W, k.WQ16 + (int64_t)H * W, W, 0, 1));
        SPN_TRY(piece(x.s1W, 0, H, W, k.WQT16, d.NQ, 1, 1));
        SPN_TRY(piece(x.r1W, 0, H, W, k.WQT16 + H, d.NQ, 1, 1));
        if (d.beta) {
            SPN_TRY(piece(x.b1W, 0, H, W, k.WQ16 + (int64_t)2 * H * W, W, 0, 1));
            SPN_TRY(piece(x.b1W, 0, H, W, k.WQT16 + 2 * H, d.NQ, 1, 1));
        }
        SPN_TRY(piece(x.s2W, 0, H, H, k.Ws2_16, H, 0, 1));
        SPN_TRY(piece(x.s2W, 0, H, H, k.Ws2T16, H, 1, 1));
        SPN_TRY(piece(x.s3W, 0, H, H, k.Ws3_16, H, 0, 1));
        SPN_TRY(piece(x.s3W, 0, H, H, k.Ws3T16, H, 1, 1));
        if (k.Ffeat16 >= 0) {  // the fused inference heads' fragment streams
            if (d.sem) SPN_TRY(piece(x.m1W, 0, H, W, k.Fsem16, W, 0, 5));
            SPN_TRY(piece(x.featW, 0, W, W, k.Ffeat16, W, 0, 2));
            SPN_TRY(piece(x.s1W, 0, H, W, k.FQ16, W, 0, 2));
            SPN_TRY(piece(x.r1W, 0, H, W, k.FQ16 + (int64_t)H * W, W, 0, 2));  // rows H.. of Q (64-row waves)
            SPN_TRY(piece(x.s2W, 0, H, H, k.Fs2_16, H, 0, 5));
            SPN_TRY(piece(x.s3W, 0, H, H, k.Fs3_16, H, 0, 5));
            SPN_TRY(piece(x.s1W, 0, H, W, k.FQs16, W, 0, 5));   // the solar pass's Q (sun_v.0 alone)
            auto narrow = [&](int pi, int nsrc, int K, int64_t dst) {
                SPN_TRY(piece(pi, 0, 32, K, dst, K, 0, 6));
                v.back().nsrc = nsrc;
                return SPNERF_OK;
            };
            SPN_TRY(narrow(x.sigW, 1, W, k.Fnar16));
            SPN_TRY(narrow(x.r2W, 3, H, k.Fnar16 + (int64_t)32 * W));
            SPN_TRY(narrow(x.s4W, 1, H, k.Fnar16 + (int64_t)32 * (W + H)));
        }
        if (k.BG16 >= 0) {  // the heads' fused dX chain: transposed, fragment order
            SPN_TRY(piece(x.s3W, 0, H, H, k.Bs3_16, H, 1, 5));
            SPN_TRY(piece(x.s2W, 0, H, H, k.Bs2_16, H, 1, 5));
            // K index q of Q: sun_v.0 rows, then rgb.0 rows (k += H: (H / 16) k-steps of 2 · 512)
            SPN_TRY(piece(x.s1W, 0, H, W, k.BQ16, d.NQ, 1, 7));
            SPN_TRY(piece(x.r1W, 0, H, W, k.BQ16 + (int64_t)(H / 16) * 2 * 512, d.NQ, 1, 7));
            SPN_TRY(piece(x.featW, 0, W, W, k.BG16, d.NG, 1, 7));
            if (d.sem) SPN_TRY(piece(x.m1W, 0, H, W, k.BG16 + (int64_t)(W / 16) * 2 * 512, d.NG, 1, 7));
        }
    }
    return launch_pack(v, packed, s);
}

}  // namespace spn

using namespace spn;

extern "C" int32_t spnerf_param_count(const spnerf_model_cfg* cfg) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    return (int32_t)param_specs(d, nullptr).size();
}

extern "C" int32_t spnerf_param_info(const spnerf_model_cfg* cfg, int32_t idx, char* name, int32_t cap, int64_t* rows,
                                     int64_t* cols) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    auto v = param_specs(d, nullptr);
    SPN_ARG(idx >= 0 && idx < (int)v.size(), "param index %d out of range", idx);
    if (name && cap > 0) {
        snprintf(name, cap, "%s", v[idx].name.c_str());
    }
    if (rows) *rows = v[idx].rows;
    if (cols) *cols = v[idx].cols;
    return SPNERF_OK;
}

extern "C" int64_t spnerf_packed_bytes(const spnerf_model_cfg* cfg) {
    Dims d;
    if (make_dims(cfg, &d) != SPNERF_OK) return -1;
    return packed_layout(d).total * (int64_t)sizeof(float);
}

extern "C" int32_t spnerf_pack_params(const spnerf_model_cfg* cfg, const float* const* params, void* packed, void* stream) {
    Dims d;
    SPN_TRY(make_dims(cfg, &d));
    SPN_ARG(params && packed, "pack: NULL pointer");
    return pack_params(d, params, (float*)packed, (hipStream_t)stream);
}
