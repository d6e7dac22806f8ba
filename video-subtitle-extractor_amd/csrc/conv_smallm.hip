// 1x1 convolution over a HANDFUL of pixels (M <= 256): the SE / ESE gate convs — one pixel per image behind a global average
// pool, 256 .. 1024 channels in and out (gfx950 / CDNA4).
//
// conv_gemm_kernel gives such a layer Np / 128 blocks of a 128 x 128 tile (2 .. 8 blocks on 256 CUs), each walking all of K through
// its LDS ring: 22 - 29 us per layer, five layers per recogniser launch sequence and per detector pass.  The layer is a GEMV-shaped
// weight stream (Np x K x 2 bytes, L2-resident) against a tiny activation matrix, so here
//   wave   = one block = 32 couts x 32 pixels (one accumulator tile); grid = Np / 32 x ceil(M / 32) waves all over the chip;
//   K loop = 16-channel slices, both MFMA operands straight from global memory (the weight fragment of lane (cout row, k half) is
//            one 16-byte load from the [K / KT][Np][KT] tiles conv_gemm_kernel reads; the activation fragment of lane (pixel, k half)
//            one 16-byte NHWC load), eight slices of loads in flight;
//   order  = k ascending, one fp32 accumulator — conv_gemm_kernel's order, so the bits are identical;
//   epilogue = conv_epilogue_tile (bias, activation, residual, ragged mask, fp16 / fp32 stores), as everywhere.
// No LDS but the 32 bias values, no barrier in the K loop.
#include "conv_common.h"

#define SM_UNROLL 8

template <int KT, bool HILO>       // HILO (round 5, the mobile detectors' SE convs): the lo weight tiles follow the hi tiles; K is walked twice
__device__ __forceinline__ void conv_smallm_body(const ConvParams& p, float* sbias) {
    const int lane = threadIdx.x;
    const int fx = lane & 31, fj = lane >> 5;
    const int n0 = blockIdx.x * 32;                          // first cout of this wave
    const long m0 = (long)blockIdx.y * 32;                   // first pixel
    if (lane < 32) sbias[lane] = (n0 + lane < p.Np) ? p.bias[n0 + lane] : 0.f;

    const int co = n0 + conv_wrow(fx);                       // the cout whose weights this lane supplies
    const bool wok = co < p.Np;
    const half_t* wl = p.w + (long)(wok ? co : 0) * KT + fj * 8;
    const long wstep = (long)p.Np * KT;                      // elements between K tiles
    const long m = m0 + fx;                                  // the pixel whose activations this lane supplies
    const bool xok = m < p.M;
    const half_t* xl = p.in + (xok ? m : 0) * (long)p.in_ld + fj * 8;

    float16v acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const half8 zero8 = half8{0, 0, 0, 0, 0, 0, 0, 0};
    const int nslice = (p.cinp + 15) >> 4;                   // (cinp % 16 == 8: the upper half of the last slice lies behind the pixel's channels: zeros)
    // (hi pass, then lo pass over the same activations into the same accumulator: conv_gemm_kernel's two-pass K walk, identical bits)
#pragma unroll 1
    for (int pass = 0; pass < (HILO ? 2 : 1); ++pass) {
        const half_t* wp = wl + (long)pass * p.nkh * wstep;
        for (int s0 = 0; s0 < nslice; s0 += SM_UNROLL) {
            half8 wf[SM_UNROLL], xf[SM_UNROLL];
#pragma unroll
            for (int u = 0; u < SM_UNROLL; ++u) {
                const int k = (s0 + u) << 4;
                const bool live = k + fj * 8 < p.cinp;
                wf[u] = (live && wok) ? *reinterpret_cast<const half8*>(wp + (long)(k / KT) * wstep + (k % KT)) : zero8;
                xf[u] = (live && xok) ? *reinterpret_cast<const half8*>(xl + k) : zero8;
            }
#pragma unroll
            for (int u = 0; u < SM_UNROLL; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[u], xf[u], acc, 0, 0, 0);
        }
    }
    __syncthreads();
    if (xok) {
        const int hw = p.OH * p.OW;
        const long n = m / hw;
        const int r = (int)(m - n * hw);
        float bias[16];
        conv_epilogue_consts(sbias, 0, lane, bias);
        conv_epilogue_tile(p, acc, bias, m, n, r / p.OW, r % p.OW, n0, lane);
    }
}

template <int KT>
__global__ __launch_bounds__(64) void conv_smallm_kernel(const ConvParams p) {
    __shared__ float sbias[32];
    conv_smallm_body<KT, false>(p, sbias);
}
template <int KT>
__global__ __launch_bounds__(64) void conv_smallm_hl_kernel(const ConvParams p) {
    __shared__ float sbias[32];
    conv_smallm_body<KT, true>(p, sbias);
}

// arg = KT, hi + lo; which layers it serves: conv_select() (conv_select.hip)
static const ConvInst kSmallmInst[] = {
    CONV_INST(32, 1, 0, conv_smallm_hl_kernel<32>), CONV_INST(64, 1, 0, conv_smallm_hl_kernel<64>),
    CONV_INST(32, 0, 0, conv_smallm_kernel<32>), CONV_INST(64, 0, 0, conv_smallm_kernel<64>),
};

static int launch_conv_smallm(const ConvParams& pin, const ConvKernel& k, hipStream_t st) {
    const ConvInst* inst = conv_inst(conv_smallm_family(), k);
    if (!inst) return VSE_E_UNSUPPORTED;
    ConvParams p = pin;
    p.nkh = p.nkh * 32 / k.arg[0];           // K tiles of one weight pass (nkh = Kp / 32 on entry)
    if ((p.M + 31) / 32 > 65535) return VSE_E_UNSUPPORTED;
    const dim3 grid((unsigned)((p.Np + 31) / 32), (unsigned)((p.M + 31) / 32)), block(64);
    hipLaunchKernelGGL(inst->fn, grid, block, 0, st, p);
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}
ConvFamily conv_smallm_family() { return conv_family(launch_conv_smallm, kSmallmInst); }
