// Implicit-GEMM convolution, scalar-addressed variant ("conv_gemm_kernel"), for layers whose K tiles never straddle a
// filter tap (cinp % BK == 0) and whose input is read at its own resolution.  Same math and epilogue as
// conv_mfma_kernel (conv_mfma.hip) — results are bit-identical — but built around what bounds an implicit GEMM on
// gfx950: the L2 -> LDS fill path (~56 B/clk/CU) and the instruction stream next to the MFMAs.
//
//   * every LDS-DMA is `buffer_load_dwordx4 v_off, s[rsrc], s_off offen lds`: the per-lane part of the address
//     (row of the tile, 16-byte k-vector) is a 32-bit VGPR computed ONCE per block; the per-K-step part (filter tap
//     offset + channel offset, or the weight tile offset) is one SGPR updated by SALU.  No 64-bit vector address
//     arithmetic, no divergent branches in the loop.
//   * zero padding / M tail / cout tail come from the buffer descriptor's bounds check: an invalid lane's offset gets
//     bit 31 set, the load is out of range and the DMA writes zeros (no zero page, no select on pointers).  The
//     validity of (row, tap) is one bit of a per-row tap mask: v_bfe_u32 + v_lshl_or_b32 per load.
//   * BK = 64 configurations fetch whole 128-byte lines per row (one wave instruction = 8 rows x 128 B) and tiles of
//     256 pixels x 128/256 couts raise the flops per fetched byte over the 128 x 128 x 32 tile of conv_mfma_kernel.
//   * the ring is unrolled by stage, so every ds_read_b128 is `per-thread VGPR + immediate`.
//   * the unmasked form can take the column sums of what it stores for the global-average pool record behind it (gap_part, a runtime
//     branch of the epilogue; conv_gap_select in conv_select.hip decides per plan): that pool's pass over the tensor is then not run.
//
// Eligibility and the tile configuration (kCfg, conv_common.h) are decided by conv_select(); everything else stays on conv_mfma_kernel.

#include <type_traits>
#include "conv_common.h"

// The LDS-DMAs are builtins: as asm statements (counted lgkmcnt waits survive) they measured 1-3 % SLOWER — the kernel is bound by
// the DMA stream, and the asm form adds issue slots.

// BM x BN block tile (pixels x couts), WM x WN waves, BKT-deep K tiles in an ST-stage LDS ring.
// MASK = 0: 1x1, no padding, K % 64 == 0 -> every (row, k) of a valid row is a real element, no tap mask.
// MASK = 1: up to 31 taps, one validity bit per tap and row.
// blocks per CU the LDS ring allows -> waves per SIMD the register allocation has to leave room for
constexpr int gemm_waves_per_simd(int bm, int bn, int bkt, int st, int nw) {
    const int rpi = 64 / (bkt / 8);
    const int bnr = (bn + rpi * nw - 1) / (rpi * nw) * (rpi * nw);
    const int blocks = (160 * 1024) / (st * (bm + bnr) * bkt * 2 + bn * 4);
    const int w = blocks * nw / 4;
    return w < 1 ? 1 : (w > 4 ? 4 : w);
}

// v + (the value of the lane the DPP control names), all lanes active
template <int CTRL> __device__ __forceinline__ float gap_dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

template <int BM, int BN, int WM, int WN, int BKT, int ST, int MASK>
__global__ __launch_bounds__(64 * WM * WN, gemm_waves_per_simd(BM, BN, BKT, ST, WM * WN))
void conv_gemm_kernel(const ConvParams p) {
    constexpr int NW = WM * WN;                 // waves per block
    constexpr int KV = BKT / 8;                 // 16-byte k-vectors per LDS row (4 or 8)
    constexpr int RPI = 64 / KV;                // tile rows one wave instruction (1 KiB) covers
    constexpr int ROWB = BKT * 2;               // bytes per LDS row
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int KS = BKT / 16;                // MFMA k sub-steps per tile
    constexpr int BNR = (BN + RPI * NW - 1) / (RPI * NW) * (RPI * NW);   // weight rows staged (whole wave instructions)
    constexpr int NA = BM / (RPI * NW);         // LDS-DMA instructions per wave per stage, activations
    constexpr int NB = BNR / (RPI * NW);        // ... weights
    constexpr int LPT = NA + NB;
    constexpr int STAGE_HALFS = (BM + BNR) * BKT;
    static_assert(BKT == 32 || BKT == 64, "BK");
    static_assert(ST >= 2 && ST <= 5 && (ST - 2) * LPT <= 16, "ring depth");
    static_assert(TM >= 1 && TN >= 1 && NA >= 1 && NB >= 1 && BM % (RPI * NW) == 0 && BNR % (RPI * NW) == 0, "tile shape");
    static_assert(ST * STAGE_HALFS * 2 + BN * 4 <= 160 * 1024, "LDS");

    __shared__ __attribute__((aligned(16))) half_t lds[ST * STAGE_HALFS + BN * 2];   // ring + BN floats of bias
    float* const sbias = reinterpret_cast<float*>(lds + ST * STAGE_HALFS);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    // XCD-aware tile order, identical to conv_mfma_kernel
    const unsigned logical = xcd_block(blockIdx.x, gridDim.x);
    const unsigned mtile = logical / p.ntn, ntile = logical - mtile * p.ntn;
    // F_IMGW (per-image weights): M tiles are aligned to images, so that one tile has one weight matrix
    // ... and so are they when the block sums the global-average pool's partials (gap_part): a tile then belongs to one image, and an
    // image's rows are grouped the same way wherever it sits in the batch
    long m0 = (long)mtile * BM;
    long mend = p.M;                                 // rows at or beyond it do not exist
    const half_t* wsrc = p.w;
    const bool gap = MASK == 0 && p.gap_part != nullptr;
    unsigned img = 0, ti = 0;
    if ((p.flags & F_IMGW) || gap) {
        img = mtile / (unsigned)p.tiles_img;
        ti = mtile - img * (unsigned)p.tiles_img;
        m0 = (long)img * p.hw_img + (long)ti * BM;
        mend = (long)(img + 1) * p.hw_img;
        if (p.flags & F_IMGW) wsrc += (long)img * p.wimg_stride;
    }
    const int n0 = ntile * BN;

    // LDS image: row-major [row][BKT halfs], 16-byte slots XOR-swizzled by the row so that the MFMA fragment reads
    // (32 consecutive rows, one logical slot) are bank-conflict free: BK=32: slot ^ (row>>2 & 3); BK=64: slot ^ (row>>1 & 7)
    auto swz = [](int r) { return BKT == 32 ? (r >> 2) & 3 : (r >> 1) & 7; };

    // ---- block-uniform descriptors ------------------------------------------------------------------------
    // activations: base = address of tap (0,0), channel 0 of the block's first output pixel (may lie before the tensor
    // for padded borders; it is only ever used with offsets that land inside).  Input pixel index is monotone in m
    // (checked at launch: kh >= 2*ph + 1, kw >= 2*pw), so every row's offset from this base is >= 0.
    long pix0;
    {
        const int ow = (int)(m0 % p.OW);
        const long t = m0 / p.OW;
        const int oh = (int)(t % p.OH);
        const long n = t / p.OH;
        pix0 = (n * p.Hs + (long)oh * p.sh - p.ph) * p.Ws + (long)ow * p.sw - p.pw;
    }
    const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.in + pix0 * p.in_ld), 0, 0x7fffffff, 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)(wsrc + (long)n0 * ((p.flags & F_WK32) ? 32 : 64)), 0, 0x7fffffff, 0x00020000);

    // ---- per-thread, loop-invariant offsets ------------------------------------------------------------------
    // wave instruction j of this wave covers tile rows (j*NW + wave)*RPI .. +RPI-1; lane l -> row + l/KV, physical
    // 16-byte slot l%KV, i.e. logical k-vector (l%KV) ^ swz(row)  (source-side swizzle; the LDS image is lane-linear)
    const int rsub = lane / KV;
    unsigned voffA[NA], ntap[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int r = (j * NW + wave) * RPI + rsub;
        const int kv = (lane % KV) ^ swz(r);
        const long m = m0 + r;
        voffA[j] = OOB;
        ntap[j] = 0xffffffffu;
        if (m < mend) {
            const int ow = (int)(m % p.OW);
            const long t = m / p.OW;
            const int oh = (int)(t % p.OH);
            const long n = t / p.OH;
            const int ih0 = oh * p.sh - p.ph, iw0 = ow * p.sw - p.pw;
            const long pix = (n * p.Hs + ih0) * p.Ws + iw0;
            voffA[j] = (unsigned)((pix - pix0) * p.in_ld * 2 + kv * 16);
            if constexpr (MASK) {
                unsigned okm = 0;
                for (int dy = 0; dy < p.kh; ++dy)
                    for (int dx = 0; dx < p.kw; ++dx)
                        okm |= (unsigned)(ih0 + dy >= 0 && ih0 + dy < p.H && iw0 + dx >= 0 && iw0 + dx < p.W) << (dy * p.kw + dx);
                ntap[j] = ~okm;
            }
        }
    }
    const bool wk32 = p.flags & F_WK32;
    unsigned voffW[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int r = (j * NW + wave) * RPI + rsub;
        const int kv = (lane % KV) ^ swz(r);
        // weights tiled [Kp/64][Np][64], or (F_WK32, BK 32 only) [Kp/32][Np][32]: a wave DMA then covers 1 KiB of
        // CONTIGUOUS memory = 8 whole 128-byte lines instead of 16 half lines (half the L2 requests of the weight stream)
        // (BK 64 over 32-deep tiles: k-vectors 4..7 of a row come from the next tile, Np * 64 bytes further)
        voffW[j] = !(r < BN && n0 + r < p.Np) ? OOB
                 : wk32 ? (unsigned)((kv >> 2) * p.Np * 64 + r * 64 + (kv & 3) * 16) : (unsigned)(r * 128 + kv * 16);
    }
    const unsigned wstep = (unsigned)p.Np * (wk32 ? 64u : 128u);       // bytes per weight K tile

    // ---- block-uniform K walk (SALU) ---------------------------------------------------------------------------
    int kc = 0, dx = 0, dy = 0, tap = 0;
    auto issue = [&](int kt, int st) {
        half_t* base = lds + st * STAGE_HALFS;
        const int soffA = ((dy * p.Ws + dx) * p.in_ld + kc) * 2;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            unsigned off = voffA[j];
            if constexpr (MASK) off |= __builtin_amdgcn_ubfe(ntap[j], (unsigned)tap, 1u) << 31;   // v_bfe_u32 + v_lshl_or_b32
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (ldsv_t)(base + (j * NW + wave) * RPI * BKT), 16, (int)off, soffA, 0, 0);
        }
        const int soffW = wk32 ? (int)((unsigned)kt * (BKT / 32) * wstep)
                         : BKT == 64 ? (int)((unsigned)kt * wstep) : (int)((unsigned)(kt >> 1) * wstep + (unsigned)(kt & 1) * 64u);
#pragma unroll
        for (int j = 0; j < NB; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (ldsv_t)(base + BM * BKT + (j * NW + wave) * RPI * BKT), 16, (int)voffW[j], soffW, 0, 0);
        kc += BKT;
        if (kc >= p.cinp) {
            kc = 0;
            ++tap;
            if (++dx == p.kw) { dx = 0; ++dy; }
        }
        if (kt + 1 == p.nkh) { kc = 0; dx = 0; dy = 0; tap = 0; }      // F_HILO: second pass (lo weight tiles), same activations
    };

    float16v acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    conv_stage_consts(sbias, p.bias, p.zero, n0, BN, p.Np, wave, lane);
#pragma unroll
    for (int s = 0; s < ST - 1; ++s)
        if (s < p.nk) issue(s, s);

    // fragment addresses inside a stage: row*ROWB + swizzled 16-byte slot; tiles of one wave are 32 rows apart, which
    // keeps swz(row), so tile i / stage S are immediates on top of one per-thread VGPR per k sub-step and operand
    const int frow = lane & 31, fj = lane >> 5;
    const char* xptr[KS];
    const char* wptr[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int rx = wm * WTM + frow, rw = wn * WTN + conv_wrow(frow);
        xptr[ks] = (const char*)lds + rx * ROWB + (((ks * 2 + fj) ^ swz(rx)) << 4);
        wptr[ks] = (const char*)lds + BM * ROWB + rw * ROWB + (((ks * 2 + fj) ^ swz(rw)) << 4);
    }

    int kt = 0;
    auto step = [&](auto stage_c) {
        constexpr int S = decltype(stage_c)::value;
        // WAR on the ring slot refilled below: it was read during step kt-1, and those ds_reads were retired by the
        // lgkmcnt waits in front of that step's last MFMAs — keep this step's barrier behind them (no hoisting)
        __builtin_amdgcn_sched_barrier(0);
        // tile kt has landed once only the loads of the ST-2 tiles behind it can be outstanding (vmcnt retires in order)
        const int rem = p.nk - 1 - kt;
        if (rem >= ST - 2) wait_vm<(ST - 2) * LPT>();
        else if (ST >= 5 && rem == 2) wait_vm<2 * LPT>();
        else if (ST >= 4 && rem == 1) wait_vm<LPT>();
        else wait_vm<0>();
        __builtin_amdgcn_s_barrier();              // every thread's part of tile kt is in LDS; compute(kt-1) is over
        asm volatile("" ::: "memory");
        if (kt + ST - 1 < p.nk) issue(kt + ST - 1, (S + ST - 1) % ST);
        // fragment reads in groups of KG k sub-steps (<= 16 ds_read_b128 in flight), each followed by its MFMAs
        // (16-wave tiles run 4 waves per SIMD = 128 VGPRs: at most 8 fragments = 32 VGPRs in flight beside the accumulators)
        constexpr int FCAP = NW >= 16 ? 8 : 16;
        constexpr int KG = (KS * (TM + TN) <= FCAP) ? KS : (KS / 2 * (TM + TN) <= FCAP ? KS / 2 : 1);
#pragma unroll
        for (int k0 = 0; k0 < KS; k0 += KG) {
            half8 wf[KG][TN], xf[KG][TM];
#pragma unroll
            for (int ks = 0; ks < KG; ++ks) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    wf[ks][j] = *reinterpret_cast<const half8*>(wptr[k0 + ks] + (S * STAGE_HALFS + j * 32 * BKT) * 2);
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    xf[ks][i] = *reinterpret_cast<const half8*>(xptr[k0 + ks] + (S * STAGE_HALFS + i * 32 * BKT) * 2);
            }
#pragma unroll
            for (int ks = 0; ks < KG; ++ks)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks][j], xf[ks][i], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, KG * (TM + TN), 0);   // this group's ds_reads ...
            __builtin_amdgcn_sched_group_barrier(0x008, KG * TM * TN, 0);     // ... then its MFMAs
        }
    };
    // whole ring revolutions without exits (keeps the accumulators in place), then a tail of at most ST-1 steps
    for (; kt + ST <= p.nk;) {
        step(std::integral_constant<int, 0>{}); ++kt;
        step(std::integral_constant<int, 1>{}); ++kt;
        if constexpr (ST >= 3) { step(std::integral_constant<int, 2>{}); ++kt; }
        if constexpr (ST >= 4) { step(std::integral_constant<int, 3>{}); ++kt; }
        if constexpr (ST >= 5) { step(std::integral_constant<int, 4>{}); ++kt; }
    }
    if (kt < p.nk) {
        step(std::integral_constant<int, 0>{}); ++kt;
        if constexpr (ST >= 3) {
            if (kt < p.nk) { step(std::integral_constant<int, 1>{}); ++kt; }
        }
        if constexpr (ST >= 4) {
            if (kt < p.nk) { step(std::integral_constant<int, 2>{}); ++kt; }
        }
        if constexpr (ST >= 5) {
            if (kt < p.nk) { step(std::integral_constant<int, 3>{}); ++kt; }
        }
    }

    // ---- epilogue + column sums for the global-average pool behind this conv (conv_gap_select: plain epilogue, 16-byte stores) ------
    // The sums are taken over the values AS STORED (after the activation, rounded to fp16), rows at or beyond mend left out, in a fixed
    // order: the wave's row tiles in the lane, the 16 lanes of a DPP row, then — through LDS, the ring is free — the 2 WM half-tiles of
    // the block in order.  Slot (tile of the image) % gap_splits takes the block's sums: a plain store, or with gap_atomic an atomic add
    // to a zeroed slot that has at most two contributors (fp32 addition commutes, so the order of arrival does not show).
    if (gap) {
        __syncthreads();                               // every wave has left the K loop: the ring is free
        float* const red = reinterpret_cast<float*>(lds);      // [2 * WM][BN]
        long mrow[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) mrow[i] = m0 + wm * WTM + i * 32 + (lane & 31);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float bias[16];
            conv_epilogue_consts(sbias, wn * WTN + j * 32, lane, bias);
            const int cb = wn * WTN + j * 32 + (lane >> 5) * 8;      // first cout of this lane's run 0, inside the block's tile
            float cs[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) cs[e] = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float v[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] = acc[i][j][e] + bias[e];
                vse_act_n(v, p.act, p.act_a, p.act_b);
                if (p.post_a != 1.f || p.post_b != 0.f) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] = v[e] * p.post_a + p.post_b;
                }
                vse_act_n(v, p.act2, 0.f, 0.f);
                const bool live = mrow[i] < mend;
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const float* w = v + g * 8;
                    const half8 h8 = half8{(half_t)w[0], (half_t)w[1], (half_t)w[2], (half_t)w[3],
                                           (half_t)w[4], (half_t)w[5], (half_t)w[6], (half_t)w[7]};
                    if (live && n0 + cb + g * 16 < p.Np)
                        *reinterpret_cast<half8*>(reinterpret_cast<half_t*>(p.out) + mrow[i] * p.out_ld + n0 + cb + g * 16) = h8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) cs[g * 8 + e] += live ? (float)h8[e] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                cs[e] = gap_dpp_add<0xB1>(cs[e]);      // quad_perm [1, 0, 3, 2]
                cs[e] = gap_dpp_add<0x4E>(cs[e]);      // quad_perm [2, 3, 0, 1]
                cs[e] = gap_dpp_add<0x141>(cs[e]);     // row_half_mirror
                cs[e] = gap_dpp_add<0x140>(cs[e]);     // row_mirror: every lane holds the sum of its row of 16
            }
            if ((lane & 15) == 0) {
                float* r = red + (wm * 2 + ((lane >> 4) & 1)) * BN + cb;
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int e = 0; e < 8; ++e) r[g * 16 + e] = cs[g * 8 + e];
            }
        }
        __syncthreads();
        if (tid < BN && n0 + tid < p.gap_c) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 2 * WM; ++r) s += red[r * BN + tid];
            float* dst = p.gap_part + ((long)img * p.gap_splits + (int)(ti % (unsigned)p.gap_splits)) * p.gap_c + n0 + tid;
            if (p.gap_atomic) atomicAdd(dst, s);
            else *dst = s;
        }
        return;
    }

    // ---- epilogue (shared with conv_mfma_kernel) ---------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const long m = m0 + wm * WTM + i * 32 + (lane & 31);
        if (m >= mend) continue;
        const int ow = (int)(m % p.OW);
        const long t = m / p.OW;
        const int oh = (int)(t % p.OH);
        const long n = t / p.OH;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float bias[16];
            conv_epilogue_consts(sbias, wn * WTN + j * 32, lane, bias);
            conv_epilogue_tile(p, acc[i][j], bias, m, n, oh, ow, n0 + wn * WTN + j * 32, lane);
        }
    }
}

// arg = the kCfg configuration, MASK.  GEMM_INST spells the configuration's numbers (the kernel's name) and refuses to compile where
// they are not kCfg[I]'s.  (The kernels lie in the code object in the order of their entries: configuration 0 has always come last.)
template <int I, int BM, int BN, int WM, int WN, int BKT, int ST>
constexpr int gemm_cfg_is() {
    static_assert(kCfg[I].bm == BM && kCfg[I].bn == BN && kCfg[I].wm == WM && kCfg[I].wn == WN && kCfg[I].bk == BKT && kCfg[I].st == ST,
                  "GEMM_INST: the spelled template arguments are not kCfg[I]");
    return I;
}
#define GEMM_INST(I, ...) CONV_INST((gemm_cfg_is<I, __VA_ARGS__>()), 1, 0, conv_gemm_kernel<__VA_ARGS__, 1>), \
                          CONV_INST((gemm_cfg_is<I, __VA_ARGS__>()), 0, 0, conv_gemm_kernel<__VA_ARGS__, 0>)
static const ConvInst kGemmInst[] = {
    GEMM_INST(1, 256, 64, 4, 1, 32, 3),  GEMM_INST(2, 256, 32, 4, 1, 32, 3),  GEMM_INST(3, 256, 128, 4, 2, 32, 3), GEMM_INST(4, 256, 256, 4, 4, 32, 3),
    GEMM_INST(5, 256, 192, 8, 2, 32, 3), GEMM_INST(6, 256, 256, 4, 4, 64, 2), GEMM_INST(7, 256, 192, 8, 2, 64, 2), GEMM_INST(0, 128, 128, 2, 2, 32, 3),
};

static int launch_conv_gemm(const ConvParams& pin, const ConvKernel& k, hipStream_t st) {
    const ConvInst* inst = conv_inst(conv_gemm_family(), k);
    if (!inst) return VSE_E_UNSUPPORTED;
    ConvParams p = pin;
    const GemmCfg& g = kCfg[k.arg[0]];
    p.ntn = (unsigned)((p.Np + g.bn - 1) / g.bn);
    p.nkh = p.nkh * 32 / g.bk;               // (nkh = Kp / 32 on entry)
    p.nk = p.nkh;
    if (p.flags & F_HILO) p.nk *= 2;
    unsigned long long tiles = (unsigned long long)((p.M + g.bm - 1) / g.bm) * p.ntn;
    if (p.gap_part && (k.arg[1] != 0 || p.hw_img <= 0 || p.M % p.hw_img || p.gap_splits < 1 || g.bn > 64 * g.wm * g.wn)) return VSE_E_INVAL;
    if ((p.flags & F_IMGW) || p.gap_part) {
        p.tiles_img = (p.hw_img + g.bm - 1) / g.bm;
        tiles = (unsigned long long)(p.M / p.hw_img) * p.tiles_img * p.ntn;
    }
    // a slot takes one tile by a plain store, or two by atomic adds to the zeroed buffer (conv_gap_select decided for this row tile)
    if (p.gap_part && (p.tiles_img > 2 * p.gap_splits || (p.gap_atomic != 0) != (p.tiles_img > p.gap_splits))) return VSE_E_INVAL;
    if (tiles == 0 || tiles > 0x7fffffffull) return VSE_E_INVAL;
    hipLaunchKernelGGL(inst->fn, dim3((unsigned)tiles), dim3(64 * g.wm * g.wn), 0, st, p);
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}
ConvFamily conv_gemm_family() { return conv_family(launch_conv_gemm, kGemmInst); }
