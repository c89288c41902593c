// Fragment of gemm_bf16.hip, included there under SPN_ABLATIONS after k_gemm_tn_bf16d (it uses that
// file's static helpers and constants); abl_launch_tn_bf16d (launch_tn_bf16d.inc) launches these.
// Weight-gradient kernels measured slower than k_gemm_tn_bf16d in the C4 step (DESIGN.md §6): the
// 16x16x32 pipelined kernels (8 and 16 waves) and the quad-wave kernel — compiled only into
// -DSPN_ABLATIONS builds (tools/tn_lab, the A/B variant libraries).
// Weight gradients on v_mfma_f32_16x16x32_bf16 (option tn_bf16_m16): k_gemm_tn_bf16d's 256 x 256
// block tile, 32-point LDS-DMA stages and bias sums, but a wave's 128 x 64 is 8 x 4 accumulators
// of 16 x 16 and one stage is exactly one 32-point k-step.  The same LDS bytes per FLOP as the
// 32x32x16 form (a fragment is 8 points of one feature per lane either way), at a lower energy
// per FLOP (MI355X_MICROARCH.md, DVFS item 7: 1.12-1.15x the FLOP/s of 32x32x16 at equal cycles).
// The fragments are software-pipelined: a[i + 2]'s transposed reads are issued before a[i]'s four
// MFMAs, each group waits only for its own fragment (counted lgkmcnt, LDS returns in order), and
// the stage barrier sits before the last two groups, so the next stage's B and first two A
// fragments are read under this stage's last MFMAs — no group waits for a read issued in its own
// gap, and no wave drains its LDS queue at the barrier.  The DMA of stage st + NSTG - 1 is issued
// right after stage st's barrier into the slot stage st - 1 used (every wave has consumed it).
// Each output element sums its points in 32-point MFMA blocks in point order: fixed and
// deterministic, but not k_gemm_tn_bf16d's 16-point blocks, so the fp32 slabs round differently.
template <int NSTG>
__global__ __launch_bounds__(512) void k_gemm_tn_bf16m(TN16Group G) {
    static_assert(NSTG == 4 || NSTG == 5, "4 or 5 DMA stages (5 x 32 KB = the whole LDS)");
    __shared__ __attribute__((aligned(16))) char smem[NSTG * TD_STG];  // [stage][A0|A1|B0|B1]
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    typedef __attribute__((address_space(1))) void* gbl_ptr_t;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    int gi = 0;
    while (gi + 1 < G.n && wg >= G.start[gi + 1]) ++gi;
    const int w = wg - G.start[gi];
    const TN16Args& g = G.g[gi];
    const int nK = (g.K + TW - 1) / TW;
    const int ntiles = cdiv(g.N, TW) * nK;
    const int split = w / ntiles, t = w % ntiles;
    const int n0 = (t / nK) * TW, k0 = (t % nK) * TW;
    const int p_beg = split * g.p_per_split;
    const int p_end = min(g.P, p_beg + g.p_per_split);
    const bool bsplit = g.bias_split && nK == 2;
    const int kt = t % nK;
    const bool do_bias = g.slab_b != nullptr && (bsplit || k0 == 0);
    const int ns = p_end > p_beg ? (p_end - p_beg) / TD_STEP : 0;  // whole steps (host-checked)

    // DMA sources: as k_gemm_tn_bf16d
    const bf16* src[4];
    int64_t dl[4];
    int ld[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = wid + 8 * i, X = q >> 4, hf = (q >> 3) & 1, rg = q & 7;
        const int row = rg * 4 + (lane >> 4);
        const int chl = (lane & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3));
        const int f = (X ? k0 : n0) + hf * 128 + 8 * chl;
        if (X == 0) {
            src[i] = g.A + (int64_t)row * g.lda + min(f, g.N - 8);
            dl[i] = (int64_t)((intptr_t)g.A_s2 - (intptr_t)g.A);
            ld[i] = g.lda;
        } else {
            const int kc = min(f, g.K - 8);
            const bool s2 = __builtin_amdgcn_readfirstlane(kc >= g.K1 ? 1 : 0) != 0;
            ld[i] = s2 ? g.ldb2 : g.ldb;
            src[i] = (s2 ? g.B2 + (kc - g.K1) : g.B + kc) + (int64_t)row * ld[i];
            dl[i] = s2 ? (int64_t)((intptr_t)g.B2_s2 - (intptr_t)g.B2) : (int64_t)((intptr_t)g.B_s2 - (intptr_t)g.B);
        }
    }
    const int64_t P1 = g.P1;
    auto issue = [&](int st, int stg) {
        const int64_t p0 = p_beg + (int64_t)TD_STEP * st;
        const bool sg2 = p0 >= P1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = wid + 8 * i;
            const char* a = reinterpret_cast<const char*>(src[i] + p0 * ld[i]) + (sg2 ? dl[i] : 0);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)a, (lds_ptr_t)(smem + stg * TD_STG + q * 1024), 16, 0, 0);
        }
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wa = wid >> 2, wb = wid & 3;
    const int g16 = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;
    constexpr int HALF = TD_STEP * 256;
    // 16x16x32 operand of 16 features (cols 16m .. 16m + 15 of a half image) x 32 points: lane l
    // holds feature 16m + l % 16, points 8 (l / 16) .. + 7 — the 16-lane group g reads rows
    // 8g .. 8g + 3 (lo) and 8g + 4 .. 8g + 7 (hi) transposed; lane 4q + p of the group addresses
    // row + q, columns 16m + 4p .. + 3 (cdna_hip_programming.md T10: a half's two blocks 8 rows
    // apart in the same columns, conflict-free).  In tn_off's swizzle, column block m only flips
    // address bits 5..7: off(m) = off(0) ^ 32m, so a read is one v_xor from a per-stage lane address
    // (24 hoisted per-fragment addresses spilled, and a spill reload's vmcnt(0) drains the DMA ring)
    const int rlo = 8 * g16 + q4;
    const int olo = tn_off(rlo, pp >> 1) + 8 * (pp & 1), ohi = tn_off(rlo + 4, pp >> 1) + 8 * (pp & 1);
    auto lds_addr = [&](int stg, int half, int o) -> uint32_t {
        return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)(smem + stg * TD_STG + half * HALF) +
               (uint32_t)opaque(o);
    };
    auto trd = [](uint32_t base, int m) -> s16x4 {
        s16x4 v;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(base ^ (uint32_t)(32 * m)) : "memory");
        return v;
    };
    auto join = [](s16x4 lo, s16x4 hi) -> bf16x8 {
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8, v);
    };
    const int mb = (wb & 1) * 4;  // B column blocks of this wave: 4 (wb & 1) + j
    auto readB = [&](s16x4& bl, s16x4& bh, int stg, int j) {
        bl = trd(lds_addr(stg, 2 + (wb >> 1), olo), mb + j);
        bh = trd(lds_addr(stg, 2 + (wb >> 1), ohi), mb + j);
    };
    auto readA = [&](s16x4& al, s16x4& ah, int stg, int i) {
        al = trd(lds_addr(stg, wa, olo), i);
        ah = trd(lds_addr(stg, wa, ohi), i);
    };
    auto mma = [&](int i, s16x4 al, s16x4 ah, int j, s16x4 bl, s16x4 bh) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(join(al, ah), join(bl, bh), acc[i][j], 0, 0, 0);
    };
#define TNM_WAIT(N, x, y) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(x), "+v"(y) : : "memory")

    // bias: thread (chunk ch of 32, row phase lrow of 16) sums rows lrow, lrow + 16 of each stage;
    // bsplit: thread (chunk ch of the tile's 16, row phase lrow of 32) sums row lrow — read by asm
    // (ordered among the fragment reads; consumed behind a later fragment wait)
    const int ch = bsplit ? 16 * kt + (tid & 15) : tid & 31, lrow = bsplit ? tid >> 4 : tid >> 5;
    float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto brd = [&](int stg, int row) -> u32x4 {
        const uint32_t addr = lds_addr(stg, ch >> 4, tn_off(row, ch & 15));
        u32x4 v;
        asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
        return v;
    };
    auto badd = [&](u32x4 v) {
        float f[8];
        unpack8(v, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) bs[e] += f[e];
    };

    if (ns > 0) {  // block-uniform
#pragma unroll
        for (int s = 0; s < NSTG - 1; ++s) issue(min(s, ns - 1), s);  // past the end: re-reads, never consumed
        if constexpr (NSTG == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // stage 0 landed (own DMAs)
        else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        s16x4 bl[4], bh[4], al[8], ah[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) readB(bl[j], bh[j], 0, j);
        readA(al[0], ah[0], 0, 0);
        readA(al[1], ah[1], 0, 1);
        for (int st = 0; st < ns; ++st) {
            const int stg = st % NSTG;
            u32x4 bv0 = u32x4{0u, 0u, 0u, 0u}, bv1 = u32x4{0u, 0u, 0u, 0u};
            // i = 0 .. 5: a[i + 2] read, a[i] waited (4 younger reads — the bias reads, older than
            // a[2], only make the wait stricter), four MFMAs
            if (do_bias) {  // block-uniform
                bv0 = brd(stg, lrow);
                if (!bsplit) bv1 = brd(stg, lrow + 16);
            }
            readA(al[2], ah[2], stg, 2);
            asm volatile("s_waitcnt lgkmcnt(4)"
                         : "+v"(al[0]), "+v"(ah[0]), "+v"(bl[0]), "+v"(bl[1]), "+v"(bl[2]), "+v"(bl[3]), "+v"(bh[0]),
                           "+v"(bh[1]), "+v"(bh[2]), "+v"(bh[3])
                         :
                         : "memory");
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(0, al[0], ah[0], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            readA(al[3], ah[3], stg, 3);
            TNM_WAIT(4, al[1], ah[1]);
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(1, al[1], ah[1], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            readA(al[4], ah[4], stg, 4);
            asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(al[2]), "+v"(ah[2]), "+v"(bv0), "+v"(bv1) : : "memory");
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(2, al[2], ah[2], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            if (do_bias) {
                badd(bv0);
                if (!bsplit) badd(bv1);
            }
            readA(al[5], ah[5], stg, 5);
            TNM_WAIT(4, al[3], ah[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(3, al[3], ah[3], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            readA(al[6], ah[6], stg, 6);
            TNM_WAIT(4, al[4], ah[4]);
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(4, al[4], ah[4], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            readA(al[7], ah[7], stg, 7);
            TNM_WAIT(4, al[5], ah[5]);
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(5, al[5], ah[5], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            const bool more = st + 1 < ns;
            if (more) {  // block-uniform
                // stage st + 1 landed (own DMAs: at most NSTG - 3 younger stages outstanding); the
                // barrier publishes it and retires every wave's reads of slot (st - 1) % NSTG
                if constexpr (NSTG == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                issue(min(st + NSTG - 1, ns - 1), (st + NSTG - 1) % NSTG);
            }
            // the last two groups column by column: b[j] is free after (a6, bj), (a7, bj), and the
            // next stage's b[j] is read into it (then its a[0], a[1])
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(al[6]), "+v"(ah[6]), "+v"(al[7]), "+v"(ah[7]) : : "memory");
            const int nstg = (st + 1) % NSTG;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mma(6, al[6], ah[6], j, bl[j], bh[j]);
                mma(7, al[7], ah[7], j, bl[j], bh[j]);
                __builtin_amdgcn_sched_barrier(0);
                if (more) readB(bl[j], bh[j], nstg, j);
            }
            if (more) {
                readA(al[0], ah[0], nstg, 0);
                readA(al[1], ah[1], nstg, 1);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing may land in the reused LDS
        __builtin_amdgcn_s_barrier();
    }
#undef TNM_WAIT

    float* slab = g.slab + (int64_t)split * g.slab_stride;
    const int c16 = lane & 15;
    // (N and K are multiples of 256 on this kernel: tn_wide, host-checked)
    const int64_t lds_ = g.ld_slab;
    float* sp = slab + (int64_t)(n0 + wa * 128 + 4 * g16) * lds_ + k0 + wb * 64 + c16;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) sp[(int64_t)(i * 16 + r) * lds_ + j * 16] = acc[i][j][r];
    if (do_bias && bsplit) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);  // [32 phases][128 features]
        const int cl = ch & 15;
#pragma unroll
        for (int e = 0; e < 8; ++e) red[lrow * 128 + 8 * cl + e] = bs[e];
        __syncthreads();
        const int n = n0 + 128 * kt + tid;
        if (tid < 128 && n < g.N) {
            float s = 0.f;
            for (int ph = 0; ph < 32; ++ph) s += red[ph * 128 + tid];
            g.slab_b[(int64_t)split * g.N + n] = s;
        }
    } else if (do_bias) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);  // [16 phases][256 features]
#pragma unroll
        for (int e = 0; e < 8; ++e) red[lrow * 256 + 8 * ch + e] = bs[e];
        __syncthreads();
        if (tid < 256 && n0 + tid < g.N) {
            float s = 0.f;
            for (int ph = 0; ph < 16; ++ph) s += red[ph * 256 + tid];
            g.slab_b[(int64_t)split * g.N + n0 + tid] = s;
        }
    }
}

// Weight gradients with 16 waves per block (option tn_bf16_m16 3 / 4): the 256 x 256 block tile and
// 32-point LDS-DMA stages of k_gemm_tn_bf16d (the L2 -> CU bytes per FLOP of a 256 x 256 tile), but
// 16 waves of 64 x 64 (4 x 4 accumulators of v_mfma_f32_16x16x32_bf16, 64 registers): four waves
// per SIMD instead of two, so a wave waiting on its LDS reads, the DMA or the barrier leaves three
// others to issue MFMAs.  Per stage a wave reads its 4 B fragments once and streams its A
// fragments one ahead (counted lgkmcnt); the barrier sits before the last A fragment's MFMAs, which
// run column by column so each freed B register pair takes the next stage's fragment at once.
// The bias sums ride along: one 16-B row chunk per thread and stage, read among the fragments.
template <int NSTG>
__global__ __launch_bounds__(1024) void k_gemm_tn_bf16x(TN16Group G) {
    static_assert(NSTG == 4 || NSTG == 5, "4 or 5 DMA stages");
    __shared__ __attribute__((aligned(16))) char smem[NSTG * TD_STG];  // [stage][A0|A1|B0|B1]
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    typedef __attribute__((address_space(1))) void* gbl_ptr_t;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    int gi = 0;
    while (gi + 1 < G.n && wg >= G.start[gi + 1]) ++gi;
    const int w = wg - G.start[gi];
    const TN16Args& g = G.g[gi];
    const int nK = (g.K + TW - 1) / TW;
    const int ntiles = cdiv(g.N, TW) * nK;
    const int split = w / ntiles, t = w % ntiles;
    const int n0 = (t / nK) * TW, k0 = (t % nK) * TW;
    const int p_beg = split * g.p_per_split;
    const int p_end = min(g.P, p_beg + g.p_per_split);
    const bool bsplit = g.bias_split && nK == 2;
    const int kt = t % nK;
    // bias: !bsplit — thread (row tid / 32, chunk tid % 32) of the stage's 32 x 256 A rows;
    // bsplit — threads < 512: (row tid / 16, chunk 16 kt + tid % 16), the tile's 128-feature half
    const bool do_bias = g.slab_b != nullptr && (bsplit || k0 == 0);
    const bool t_bias = do_bias && (!bsplit || tid < 512);  // wave-uniform
    const int ns = p_end > p_beg ? (p_end - p_beg) / TD_STEP : 0;  // whole steps (host-checked)

    // DMA: instruction q = wid + 16 i (i = 0: A, 1: B) fills 4 rows x 256 B of one half image
    const bf16* src[2];
    int64_t dl[2];
    int ld[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = wid + 16 * i, hf = (q >> 3) & 1, rg = q & 7;
        const int row = rg * 4 + (lane >> 4);
        const int chl = (lane & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3));
        const int f = (i ? k0 : n0) + hf * 128 + 8 * chl;
        if (i == 0) {
            src[i] = g.A + (int64_t)row * g.lda + min(f, g.N - 8);
            dl[i] = (int64_t)((intptr_t)g.A_s2 - (intptr_t)g.A);
            ld[i] = g.lda;
        } else {
            const int kc = min(f, g.K - 8);
            const bool s2 = __builtin_amdgcn_readfirstlane(kc >= g.K1 ? 1 : 0) != 0;
            ld[i] = s2 ? g.ldb2 : g.ldb;
            src[i] = (s2 ? g.B2 + (kc - g.K1) : g.B + kc) + (int64_t)row * ld[i];
            dl[i] = s2 ? (int64_t)((intptr_t)g.B2_s2 - (intptr_t)g.B2) : (int64_t)((intptr_t)g.B_s2 - (intptr_t)g.B);
        }
    }
    const int64_t P1 = g.P1;
    auto issue = [&](int st, int stg) {
        const int64_t p0 = p_beg + (int64_t)TD_STEP * st;
        const bool sg2 = p0 >= P1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int q = wid + 16 * i;
            const char* a = reinterpret_cast<const char*>(src[i] + p0 * ld[i]) + (sg2 ? dl[i] : 0);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)a, (lds_ptr_t)(smem + stg * TD_STG + q * 1024), 16, 0, 0);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wa = wid >> 2, wb = wid & 3;
    const int g16 = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;
    constexpr int HALF = TD_STEP * 256;
    // fragment reads as k_gemm_tn_bf16m: off(column block m) = off(0) ^ 32 m
    const int rlo = 8 * g16 + q4;
    const int olo = tn_off(rlo, pp >> 1) + 8 * (pp & 1), ohi = tn_off(rlo + 4, pp >> 1) + 8 * (pp & 1);
    auto lds_addr = [&](int stg, int half, int o) -> uint32_t {
        return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)(smem + stg * TD_STG + half * HALF) +
               (uint32_t)opaque(o);
    };
    auto trd = [](uint32_t base, int m) -> s16x4 {
        s16x4 v;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(base ^ (uint32_t)(32 * m)) : "memory");
        return v;
    };
    auto join = [](s16x4 lo, s16x4 hi) -> bf16x8 {
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8, v);
    };
    // A: features wa * 64 + 16 i (half wa / 2, column block 4 (wa & 1) + i); B likewise with wb
    auto readB = [&](s16x4& bl, s16x4& bh, int stg, int j) {
        bl = trd(lds_addr(stg, 2 + (wb >> 1), olo), 4 * (wb & 1) + j);
        bh = trd(lds_addr(stg, 2 + (wb >> 1), ohi), 4 * (wb & 1) + j);
    };
    auto readA = [&](s16x4& al, s16x4& ah, int stg, int i) {
        al = trd(lds_addr(stg, wa >> 1, olo), 4 * (wa & 1) + i);
        ah = trd(lds_addr(stg, wa >> 1, ohi), 4 * (wa & 1) + i);
    };
    auto mma = [&](int i, s16x4 al, s16x4 ah, int j, s16x4 bl, s16x4 bh) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(join(al, ah), join(bl, bh), acc[i][j], 0, 0, 0);
    };

    const int brow = bsplit ? (tid >> 4) & 31 : tid >> 5;
    const int bch = bsplit ? 16 * kt + (tid & 15) : tid & 31;
    float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto brd = [&](int stg) -> u32x4 {
        const uint32_t addr = lds_addr(stg, bch >> 4, tn_off(brow, bch & 15));
        u32x4 v;
        asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
        return v;
    };

    if (ns > 0) {  // block-uniform
#pragma unroll
        for (int s = 0; s < NSTG - 1; ++s) issue(min(s, ns - 1), s);  // past the end: re-reads, never consumed
        if constexpr (NSTG == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // stage 0 landed (own DMAs)
        else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        s16x4 bl[4], bh[4], al[4], ah[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) readB(bl[j], bh[j], 0, j);
        readA(al[0], ah[0], 0, 0);
        for (int st = 0; st < ns; ++st) {
            const int stg = st % NSTG;
            readA(al[1], ah[1], stg, 1);
            asm volatile("s_waitcnt lgkmcnt(2)"
                         : "+v"(al[0]), "+v"(ah[0]), "+v"(bl[0]), "+v"(bl[1]), "+v"(bl[2]), "+v"(bl[3]), "+v"(bh[0]),
                           "+v"(bh[1]), "+v"(bh[2]), "+v"(bh[3])
                         :
                         : "memory");
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(0, al[0], ah[0], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            readA(al[2], ah[2], stg, 2);
            asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(al[1]), "+v"(ah[1]) : : "memory");
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(1, al[1], ah[1], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            u32x4 bv = u32x4{0u, 0u, 0u, 0u};
            if (t_bias) bv = brd(stg);  // wave-uniform; older than a[3]: covered by the next wait
            readA(al[3], ah[3], stg, 3);
            asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(al[2]), "+v"(ah[2]), "+v"(bv) : : "memory");
#pragma unroll
            for (int j = 0; j < 4; ++j) mma(2, al[2], ah[2], j, bl[j], bh[j]);
            __builtin_amdgcn_sched_barrier(0);
            if (t_bias) {
                float f[8];
                unpack8(bv, f);
#pragma unroll
                for (int e = 0; e < 8; ++e) bs[e] += f[e];
            }
            const bool more = st + 1 < ns;
            if (more) {  // block-uniform
                // stage st + 1 landed (own DMAs: at most NSTG - 3 younger stages outstanding); the
                // barrier publishes it and retires every wave's reads of slot (st - 1) % NSTG
                if constexpr (NSTG == 4) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                issue(min(st + NSTG - 1, ns - 1), (st + NSTG - 1) % NSTG);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(al[3]), "+v"(ah[3]) : : "memory");
            const int nstg = (st + 1) % NSTG;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                mma(3, al[3], ah[3], j, bl[j], bh[j]);
                __builtin_amdgcn_sched_barrier(0);
                if (more) readB(bl[j], bh[j], nstg, j);
            }
            if (more) readA(al[0], ah[0], nstg, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing may land in the reused LDS
        __builtin_amdgcn_s_barrier();
    }

    float* slab = g.slab + (int64_t)split * g.slab_stride;
    const int c16 = lane & 15;
    // (N and K are multiples of 256 on this kernel: tn_wide, host-checked)
    const int64_t lds_ = g.ld_slab;
    float* sp = slab + (int64_t)(n0 + wa * 64 + 4 * g16) * lds_ + k0 + wb * 64 + c16;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) sp[(int64_t)(i * 16 + r) * lds_ + j * 16] = acc[i][j][r];
    if (do_bias) {  // block-uniform
        const int nf = bsplit ? 128 : 256;  // features summed by this tile
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);  // [32 row phases][nf features]
        if (t_bias) {
            const int cl = bsplit ? (bch & 15) : bch;
#pragma unroll
            for (int e = 0; e < 8; ++e) red[brow * nf + 8 * cl + e] = bs[e];
        }
        __syncthreads();
        const int n = n0 + (bsplit ? 128 * kt : 0) + tid;
        if (tid < nf) {
            float s = 0.f;
            for (int ph = 0; ph < 32; ++ph) s += red[ph * nf + tid];
            g.slab_b[(int64_t)split * g.N + n] = s;
        }
    }
}

// Quad-wave DMA weight-gradient GEMM (option tn_bf16_quad): the 256x256 tile and LDS-DMA ring
// of k_gemm_tn_bf16d, but 4 waves (one per SIMD) of 128x128 each (4 x 4 32x32 accumulators, 256
// registers): 16 MFMAs per 16 fragment reads instead of 8 per 12, and the next k-step's fragments
// read while the current k-step's MFMAs run (two register sets) — a single wave per SIMD has no
// partner to hide its LDS latency. Same per-element k-order as k_gemm_tn_bf16d (bit-identical).
__global__ __launch_bounds__(256) void k_gemm_tn_bf16q(TN16Group G) {
    __shared__ __attribute__((aligned(16))) char smem[TD_STAGES * TD_STG];  // [stage][A0|A1|B0|B1]
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    typedef __attribute__((address_space(1))) void* gbl_ptr_t;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    int gi = 0;
    while (gi + 1 < G.n && wg >= G.start[gi + 1]) ++gi;
    const int w = wg - G.start[gi];
    const TN16Args& g = G.g[gi];
    const int nK = (g.K + TW - 1) / TW;
    const int ntiles = cdiv(g.N, TW) * nK;
    const int split = w / ntiles, t = w % ntiles;
    const int n0 = (t / nK) * TW, k0 = (t % nK) * TW;
    const int p_beg = split * g.p_per_split;
    const int p_end = min(g.P, p_beg + g.p_per_split);
    const bool bsplit = g.bias_split && nK == 2;
    const int kt = t % nK;
    const bool do_bias = g.slab_b != nullptr && (bsplit || k0 == 0);
    const int ns = p_end > p_beg ? (p_end - p_beg) / TD_STEP : 0;

    // this lane's 8 DMA sources (wave-instructions q = wid + 4 i of the stage's 32)
    const bf16* src[8];
    int64_t dl[8];
    int ld[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int q = wid + 4 * i, X = q >> 4, hf = (q >> 3) & 1, rg = q & 7;
        const int row = rg * 4 + (lane >> 4);
        const int chl = (lane & 15) ^ (((row & 3) << 2) | ((row >> 2) & 3));
        const int f = (X ? k0 : n0) + hf * 128 + 8 * chl;
        if (X == 0) {
            src[i] = g.A + (int64_t)row * g.lda + min(f, g.N - 8);
            dl[i] = (int64_t)((intptr_t)g.A_s2 - (intptr_t)g.A);
            ld[i] = g.lda;
        } else {
            const int kc = min(f, g.K - 8);
            const bool s2 = __builtin_amdgcn_readfirstlane(kc >= g.K1 ? 1 : 0) != 0;
            ld[i] = s2 ? g.ldb2 : g.ldb;
            src[i] = (s2 ? g.B2 + (kc - g.K1) : g.B + kc) + (int64_t)row * ld[i];
            dl[i] = s2 ? (int64_t)((intptr_t)g.B2_s2 - (intptr_t)g.B2) : (int64_t)((intptr_t)g.B_s2 - (intptr_t)g.B);
        }
    }
    const int64_t P1 = g.P1;
    auto issue = [&](int st, int stg) {
        const int64_t p0 = p_beg + (int64_t)TD_STEP * st;
        const bool sg2 = p0 >= P1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = wid + 4 * i;
            const char* a = reinterpret_cast<const char*>(src[i] + p0 * ld[i]) + (sg2 ? dl[i] : 0);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)a, (lds_ptr_t)(smem + stg * TD_STG + q * 1024), 16, 0, 0);
        }
    };

    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wa = wid >> 1, wb = wid & 1, h = lane >> 5, grp = (lane >> 4) & 1;
    const int q4 = (lane & 15) >> 2, pp = lane & 3;
    auto trd = [&](const char* base, int r0, int col) -> s16x4 {
        const int o = tn_off(r0 + q4, (col >> 3) + (pp >> 1)) + 8 * (pp & 1);
        const uint32_t addr = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)(base + o);
        s16x4 v;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
        return v;
    };
    auto join = [](s16x4 lo, s16x4 hi) -> bf16x8 {
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8, v);
    };
    constexpr int HALF = TD_STEP * 256;
    struct Frag {
        s16x4 al[4], ah[4], bl[4], bh[4];
    };
    auto fread = [&](Frag& f, int stg, int ks) {
        const char* sA = smem + stg * TD_STG + wa * HALF;
        const char* sB = smem + stg * TD_STG + (2 + wb) * HALF;
        const int r0 = 16 * ks + 8 * h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f.bl[j] = trd(sB, r0, 32 * j + 16 * grp);
            f.bh[j] = trd(sB, r0 + 4, 32 * j + 16 * grp);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f.al[i] = trd(sA, r0, 32 * i + 16 * grp);
            f.ah[i] = trd(sA, r0 + 4, 32 * i + 16 * grp);
        }
    };
    // at most 15 LDS operations (the other set's reads, issued after f's) left in flight
    auto fwait = [](Frag& f, auto cnt) {
        if constexpr (decltype(cnt)::value == 15)
            asm volatile("s_waitcnt lgkmcnt(15)"
                         : "+v"(f.al[0]), "+v"(f.al[1]), "+v"(f.al[2]), "+v"(f.al[3]), "+v"(f.ah[0]), "+v"(f.ah[1]),
                           "+v"(f.ah[2]), "+v"(f.ah[3]), "+v"(f.bl[0]), "+v"(f.bl[1]), "+v"(f.bl[2]), "+v"(f.bl[3]),
                           "+v"(f.bh[0]), "+v"(f.bh[1]), "+v"(f.bh[2]), "+v"(f.bh[3])
                         :
                         : "memory");
        else
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(f.al[0]), "+v"(f.al[1]), "+v"(f.al[2]), "+v"(f.al[3]), "+v"(f.ah[0]), "+v"(f.ah[1]),
                           "+v"(f.ah[2]), "+v"(f.ah[3]), "+v"(f.bl[0]), "+v"(f.bl[1]), "+v"(f.bl[2]), "+v"(f.bl[3]),
                           "+v"(f.bh[0]), "+v"(f.bh[1]), "+v"(f.bh[2]), "+v"(f.bh[3])
                         :
                         : "memory");
    };
    auto fmma = [&](const Frag& f) {
        bf16x8 a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = join(f.bl[j], f.bh[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = join(f.al[i], f.ah[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    };
    // bias: the per-phase sums of k_gemm_tn_bf16d in the same order (bit-identical), two phases per
    // thread: bsplit: chunk ch of the tile's 16, phases lrow and lrow + 16 (row = phase);
    // else chunk ch of 32, phases lrow and lrow + 8 (rows phase and phase + 16)
    const int ch = bsplit ? 16 * kt + (tid & 15) : tid & 31, lrow = bsplit ? tid >> 4 : tid >> 5;
    float bs[2][8] = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
    auto bias_rows = [&](int stg) {
        const char* sA = smem + stg * TD_STG + (ch >> 4) * HALF;
        if (bsplit) {  // block-uniform
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float f[8];
                unpack8(*reinterpret_cast<const u32x4*>(sA + tn_off(lrow + 16 * i, ch & 15)), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) bs[i][e] += f[e];
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float f[8];
                unpack8(*reinterpret_cast<const u32x4*>(sA + tn_off(lrow + 8 * i + 16 * r, ch & 15)), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) bs[i][e] += f[e];
            }
    };
    using I0 = std::integral_constant<int, 0>;

    if (ns > 0) {  // block-uniform
        issue(0, 0);
        issue(min(1, ns - 1), 1);  // past the end: re-reads of the last step, never consumed
        issue(min(2, ns - 1), 2);
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // step 0 landed (own DMAs)
        __builtin_amdgcn_s_barrier();
        Frag f0, f1;
        fread(f0, 0, 0);
        // each set is waited for (lgkmcnt(0): issued a whole MFMA burst earlier) just before the
        // other set's reads are issued, so they run under this set's MFMAs
        for (int st = 0; st < ns; ++st) {
            const int stg = st % TD_STAGES;
            fwait(f0, I0{});
            fread(f1, stg, 1);
            fmma(f0);
            if (do_bias) bias_rows(stg);
            // step st+1 landed (own DMAs of st+1, st+2 outstanding); the barrier publishes it and
            // retires every wave's reads of stage (st+3) % 4 = (st-1) % 4 before it is refilled
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            issue(min(st + 3, ns - 1), (st + 3) % TD_STAGES);
            fwait(f1, I0{});
            if (st + 1 < ns) fread(f0, (st + 1) % TD_STAGES, 0);
            fmma(f1);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing may land in the reused LDS
        __builtin_amdgcn_s_barrier();
    }

    float* slab = g.slab + (int64_t)split * g.slab_stride;
    const int r32 = lane & 31;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + wb * 128 + j * 32 + r32;
        if (k >= g.K) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wa * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < g.N) slab[(int64_t)n * g.ld_slab + k] = acc[i][j][r];
            }
    }
    if (do_bias && bsplit) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);  // [32 phases][128 features]
        const int cl = ch & 15;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[(lrow + 16 * i) * 128 + 8 * cl + e] = bs[i][e];
        __syncthreads();
        const int n = n0 + 128 * kt + tid;
        if (tid < 128 && n < g.N) {
            float s = 0.f;
            for (int ph = 0; ph < 32; ++ph) s += red[ph * 128 + tid];
            g.slab_b[(int64_t)split * g.N + n] = s;
        }
    } else if (do_bias) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);  // [16 phases][256 features]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[(lrow + 8 * i) * 256 + 8 * ch + e] = bs[i][e];
        __syncthreads();
        if (n0 + tid < g.N) {
            float s = 0.f;
            for (int ph = 0; ph < 16; ++ph) s += red[ph * 256 + tid];
            g.slab_b[(int64_t)split * g.N + n0 + tid] = s;
        }
    }
}
