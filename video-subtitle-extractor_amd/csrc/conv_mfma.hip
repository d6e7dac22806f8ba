// Implicit-GEMM convolution on the CDNA4 matrix cores (gfx950), NHWC fp16 in, fp32 accumulate.
//
// GEMM view:  D[cout][pixel] = sum_k  Wt[cout][k] * X[pixel][k],   k = (tap_y, tap_x, cin)
//   * "A" MFMA operand = weights (rows = cout), "B" operand = gathered activations (cols = pixel), so each
//     lane ends up holding 4 *consecutive output channels* of one pixel per accumulator quad -> 8-byte
//     NHWC stores, per-channel bias as a float4, residual loads of the same shape.
//   * v_mfma_f32_32x32x16_f16: lane l supplies row/col (l&31) and k-slice 8*(l>>5)..+7 of both operands.
//   * block = 256 threads = 4 waves arranged WM x WN over a BM(pixels) x BN(couts) tile, BK = 64 per step
//     (16 MFMAs per wave between barriers), one LDS stage with 144-byte rows (conflict-free b128 reads and
//     writes); the next K tile is prefetched into registers under the MFMAs and written after the barrier.
//   * activations are gathered as one 16-byte vector per (pixel, tap, 8-channel group): cin is padded to a
//     multiple of 8 by the compiler, so a vector never straddles taps; image borders, K padding and the
//     M tail are predicated to zero.  A nearest-upsampled input (FPN) is gathered with (y>>s, x>>s).
//   * weights arrive pre-tiled [K/64][Np][64] so a BN x 64 tile is one contiguous, fully coalesced chunk.
//   * epilogue: + bias (BN folded) -> activation -> scalar affine -> (+ residual, optionally upsampled)
//     -> activation2 -> fp16 (or fp32) store; 2x2/stride-2 transposed conv = same GEMM with a
//     pixel-shuffle store.

#include "conv_common.h"

#define BK 32          // K elements per pipeline stage
#define STAGES 3       // LDS ring: tile k is consumed while tiles k+1 and k+2 are in flight
#define ROWB 64        // bytes per LDS row (BK halfs, no padding: LDS-DMA writes are lane-linear)

template <int BM, int BN, int WM, int WN, bool UPS>
__global__ __launch_bounds__(256, (BM + (BN < 64 ? 64 : BN)) <= 256 ? 3 : 2) void conv_mfma_kernel(const ConvParams p) {   // 3 / 2 blocks per CU by LDS
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int BNR = BN < 64 ? 64 : BN;      // weight rows staged per tile (>= one wave instruction per wave)
    constexpr int NA = BM / 64;                 // LDS-DMA instructions per wave per stage, activations
    constexpr int NB = BNR / 64;                // ... weights
    constexpr int LPT = NA + NB;                // VMEM ops per thread per stage (vmcnt bookkeeping)
    constexpr int STAGE_HALFS = (BM + BNR) * BK;
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1, "tile shape");

    __shared__ __attribute__((aligned(16))) half_t lds[STAGES * STAGE_HALFS + BN * 2];   // the ONLY LDS object: ring + bias
    float* const sbias = reinterpret_cast<float*>(lds + STAGES * STAGE_HALFS);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    // XCD-aware tile order: the dispatcher places block b on XCD b % 8 (each XCD has a private 4 MiB L2).  Give every
    // XCD one CONTIGUOUS range of logical tiles (bijective for any tile count) and walk the N tiles of one pixel
    // tile first, so the kh x kw halo rows shared by neighbouring pixel tiles and the re-read of the activation
    // tile by the other cout tiles hit the same L2 instead of being fetched once per XCD.  Speed only: any
    // placement computes the same result.
    const unsigned logical = xcd_block(blockIdx.x, gridDim.x);
    const unsigned mtile = logical / p.ntn, ntile = logical - mtile * p.ntn;
    const long m0 = (long)mtile * BM;
    const int n0 = ntile * BN;

    // ---- per-thread gather state ---------------------------------------------------------------------------
    // wave instruction j of this wave covers tile rows (j*4 + wave)*16 .. +15; lane l -> row +(l>>2), physical slot
    // l&3, i.e. logical k-vector kv = (l&3) ^ ((l>>4)&3)  (row>>2 & 3 == l>>4 & 3 because the 16-row base is 16-aligned)
    const int kv = (lane & 3) ^ ((lane >> 4) & 3);
    const int rsub = lane >> 2;
    // Gather addressing is incremental: per row one base pointer (tap (0,0), channel 0) and two validity bitmasks
    // (bit dy / bit dx set when that tap row / column is inside the image); per K step the thread computes ONE tap
    // offset shared by its rows.  The nearest-upsampled input (UPS) keeps the explicit (y>>s, x>>s) form.
    int ih0[NA], iw0[NA];
    long pbase[NA];
    const half_t* rowptr[NA];
    unsigned rmask[NA], cmask[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const long m = m0 + (j * 4 + wave) * 16 + rsub;
        ih0[j] = 0; iw0[j] = 0; pbase[j] = 0; rowptr[j] = p.zero; rmask[j] = 0; cmask[j] = 0;
        if (m < p.M) {
            const int ow = (int)(m % p.OW);
            const long t = m / p.OW;
            const int oh = (int)(t % p.OH);
            const long n = t / p.OH;
            ih0[j] = oh * p.sh - p.ph;
            iw0[j] = ow * p.sw - p.pw;
            pbase[j] = n * p.Hs * p.Ws;
            if constexpr (!UPS) {
                rowptr[j] = p.in + (pbase[j] + (long)ih0[j] * p.Ws + iw0[j]) * p.in_ld;
                for (int d = 0; d < p.kh; ++d) rmask[j] |= (unsigned)(ih0[j] + d >= 0 && ih0[j] + d < p.H) << d;
                for (int d = 0; d < p.kw; ++d) cmask[j] |= (unsigned)(iw0[j] + d >= 0 && iw0[j] + d < p.W) << d;
            }
        } else if constexpr (UPS) {
            ih0[j] = -(1 << 28);
        }
    }
    int kc = kv * 8, dy = 0, dx = 0;
    while (kc >= p.cinp) {
        kc -= p.cinp;
        if (++dx == p.kw) { dx = 0; ++dy; }
    }
    const half_t* wrow[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int n = n0 + (j * 4 + wave) * 16 + rsub;
        const bool ok = ((j * 4 + wave) * 16 + rsub < BN) && (n < p.Np);
        wrow[j] = ok ? p.w + (long)n * 64 + kv * 8 : nullptr;        // weights are tiled [Kp/64][Np][64]
    }
    const long wstep = (long)p.Np * 64;

    // issue the LDS-DMAs of K tile `kt` into ring slot `st` (always exactly LPT VMEM ops per thread)
    auto issue = [&](int kt, int st) {
        half_t* base = lds + st * STAGE_HALFS;
        if constexpr (UPS) {
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int ih = ih0[j] + dy, iw = iw0[j] + dx;
                const bool ok = (dy < p.kh) && (ih >= 0) && (ih < p.H) && (iw >= 0) && (iw < p.W);
                const half_t* src = p.zero;
                if (ok) src = p.in + (pbase[j] + (long)(ih >> p.inshift) * p.Ws + (iw >> p.inshift)) * p.in_ld + kc;
                glds16(src, base + (j * 4 + wave) * 16 * BK);
            }
        } else {
            const long toff = (long)(dy * p.Ws + dx) * p.in_ld + kc;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const bool ok = (rmask[j] >> dy) & (cmask[j] >> dx) & 1u;     // bits >= kh / kw are never set
                glds16(ok ? rowptr[j] + toff : p.zero, base + (j * 4 + wave) * 16 * BK);
            }
        }
        const long woff = (long)(kt >> 1) * wstep + (kt & 1) * 32;
#pragma unroll
        for (int j = 0; j < NB; ++j) glds16(wrow[j] ? wrow[j] + woff : p.zero, base + BM * BK + (j * 4 + wave) * 16 * BK);
        kc += BK;
        while (kc >= p.cinp) {
            kc -= p.cinp;
            if (++dx == p.kw) { dx = 0; ++dy; }
        }
        if (kt + 1 == p.nkh) {                   // F_HILO: the walk over the taps starts again for the lo weight tiles
            kc = kv * 8; dy = 0; dx = 0;
            while (kc >= p.cinp) {
                kc -= p.cinp;
                if (++dx == p.kw) { dx = 0; ++dy; }
            }
        }
    };

    float16v acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    conv_stage_consts(sbias, p.bias, p.zero, n0, BN, p.Np, wave, lane);
    issue(0, 0);
    if (p.nk > 1) issue(1, 1);

    const int frow = lane & 31;
    const int fj = lane >> 5;                      // logical k-vector within a 16-wide k sub-step
    // fragment byte offsets inside a stage (row*64 + swizzled slot*16), fixed per thread
    int xoff[TM][2], woff[TN][2];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int r = wm * WTM + i * 32 + frow;
            xoff[i][ks] = r * BK + (((ks * 2 + fj) ^ ((r >> 2) & 3)) << 3);
        }
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int r = wn * WTN + j * 32 + conv_wrow(frow);
            woff[j][ks] = BM * BK + r * BK + (((ks * 2 + fj) ^ ((r >> 2) & 3)) << 3);
        }

    int st = 0;
    for (int kt = 0; kt < p.nk; ++kt) {
        // tile kt has landed once at most the LPT ops of tile kt+1 are still outstanding (vmcnt counts in order)
        if (kt + 1 < p.nk) {
            if constexpr (LPT == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else if constexpr (LPT == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
            else if constexpr (LPT == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if constexpr (LPT == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();              // every thread's part of tile kt is in LDS; compute(kt-1) is over
        asm volatile("" ::: "memory");
        if (kt + 2 < p.nk) {
            int s2 = st + 2;
            if (s2 >= STAGES) s2 -= STAGES;
            issue(kt + 2, s2);                     // refill the slot compute(kt-1) just released
        }
        const half_t* base = lds + st * STAGE_HALFS;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            half8 wf[TN], xf[TM];
#pragma unroll
            for (int j = 0; j < TN; ++j) wf[j] = *reinterpret_cast<const half8*>(base + woff[j][ks]);
#pragma unroll
            for (int i = 0; i < TM; ++i) xf[i] = *reinterpret_cast<const half8*>(base + xoff[i][ks]);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
        }
        if (++st == STAGES) st = 0;
    }

    // ---- epilogue ----------------------------------------------------------------------------------
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const long m = m0 + wm * WTM + i * 32 + (lane & 31);
        if (m >= p.M) continue;
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

// arg = BN, UPS (the input is read through a nearest-neighbour up-sampling: inshift)
static const ConvInst kMfmaInst[] = {
    CONV_INST(128, 1, 0, conv_mfma_kernel<128, 128, 2, 2, true>),  CONV_INST(64, 1, 0, conv_mfma_kernel<256, 64, 4, 1, true>),
    CONV_INST(32, 1, 0, conv_mfma_kernel<256, 32, 4, 1, true>),    CONV_INST(128, 0, 0, conv_mfma_kernel<128, 128, 2, 2, false>),
    CONV_INST(64, 0, 0, conv_mfma_kernel<256, 64, 4, 1, false>),   CONV_INST(32, 0, 0, conv_mfma_kernel<256, 32, 4, 1, false>),
};

static int launch_conv_mfma(const ConvParams& pin, const ConvKernel& k, hipStream_t st) {
    const ConvInst* inst = conv_inst(conv_mfma_family(), k);
    if (!inst) return VSE_E_UNSUPPORTED;
    ConvParams p = pin;
    const int bn = k.arg[0], bm = bn == 128 ? 128 : 256;
    p.ntn = (unsigned)((p.Np + bn - 1) / bn);
    const unsigned long long tiles = (unsigned long long)((p.M + bm - 1) / bm) * p.ntn;
    if (tiles == 0 || tiles > 0x7fffffffull) return VSE_E_INVAL;
    hipLaunchKernelGGL(inst->fn, dim3((unsigned)tiles), dim3(256), 0, st, p);
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}
ConvFamily conv_mfma_family() { return conv_family(launch_conv_mfma, kMfmaInst); }
