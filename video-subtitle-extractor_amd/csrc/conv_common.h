// Shared by the conv kernels (conv_*.hip) and the host code that chooses and launches them (conv_select.hip).
#pragma once
#include "common.h"

// Tile and table limits that a kernel and conv_select() both use
#define PTW 32                  // conv_patch_kernel: output tile width
#define CTW 32                  // conv_col_kernel: output tile width
#define CPW 48                  // conv_col_kernel: patch row stride in pixels
#define C3BN 64                 // conv_c3_kernel: couts per block
#define PW_MAXN 256             // conv_pw_kernel: staged weight rows (couts)
#define PW_MAXN_HILO 128        // ... with hi + lo weight tables
#define DWPW_ROWS_MAX_KS 3      // conv_dwpw_rows_kernel: 16-channel slices at stride 2
#define DWPW_ROWS_MAX_KS_S1 3   // ... at stride 1

struct ConvParams {
    const half_t* in;
    const half_t* w;
    const float* bias;
    const half_t* res;
    const half_t* zero;      // 4 KiB of zeros: gather target for padding / out-of-range lanes
    void* out;
    int H, W, Hs, Ws, in_ld, cinp, inshift;
    int OH, OW;
    long M;
    int kh, kw, sh, sw, ph, pw;
    int Np, nk;
    int nkh;                // F_HILO: K tiles of ONE pass over the taps (nk = 2 * nkh: hi weights, then lo weights); else = nk
    int out_ld, out_f32;
    int res_ld, resshift, res_hs, res_ws;
    int act, act2;
    float act_a, act_b, post_a, post_b;
    int flags, coutp;
    unsigned ntn;       // number of cout tiles
    unsigned ntiles;    // conv_head_up2r_kernel: tiles of the launch (the persistent blocks share them out); conv_dwpw_rows_kernel: row stride
    int tiles_h, tiles_w;   // patch kernel: output tile grid per image
    const float* dotw;      // F_DOT1: per-cout weights of the fused 1-channel projection
    float dotb;
    int dotact, dot_f32, dot_ld;
    void* dot_out;
    const half_t* in2;      // F_SRC2: channels [nv0*8, cinp) come from this tensor (own pixel grid / shift / stride)
    int in2_ld, in2_shift, in2_hs, in2_ws, nv0;
    unsigned long long* trace;   // -DVSE_TRACE builds only: per-block phase stamps
    int vec16;              // output (and residual) rows allow 16-byte accesses at every 8-channel group
    long wimg_stride;       // F_IMGW: weight elements per image (Kp * Np); M tiles are then aligned to images
    int hw_img, tiles_img;  // F_IMGW: output pixels per image, M tiles per image
    const int* wl_out;      // ragged plans: per-image output width; pixels at ow >= wl_out[n] are stored as zeros
    int in_lo_off;          // F_DWPRE: != 0: the INPUT is an fp16 hi + lo pair (both halves are filtered)
    int res_lo_off;         // != 0: the residual is an fp16 hi + lo pair: its lo half sits res_lo_off channels behind the hi half
    int lo_off;             // != 0: fp16 hi + lo pair output: fp16(v - fp16(v)) goes lo_off channels behind the hi value
    const half_t* ogate;    // F_OGATE: per-(image, cout) gate [n][ogate_ld] fp16; the value is multiplied by (1 + gate) ahead of the residual
    int ogate_ld;
    int wnp;                // conv_c3_kernel: weight rows per tap of a ring stage (= Np; F_HLSUM: 64 = hi 32 | lo 32 while Np stays 32)
    const uint8_t* u8src;   // F_U8SRC (stem): uint8 BGR frames [n][u8_h][u8_w][3], row pitch / frame stride in bytes
    int u8_h, u8_w;
    long u8_pitch, u8_fstride;
    // conv_c3_kernel / conv_col_kernel: pack_g images of the batch share one virtual row band of pack_g * OW output columns that the
    // tiles cover densely (conv_pack_group); 1 = every image is tiled on its own.  Set by the launchers.
    int pack_g, nimg;                    // images per group, images of the launch
    unsigned pack_mag_ow, pack_mag_d;    // conv_pack_magic(OW), conv_pack_magic(W + pw); 0 when pack_g == 1 (every quotient is 0)
    // conv_c3pool_kernel: a block walks pool_seg tile rows of one column strip, pool_nseg strips cover the map's tiles_h.  Set by the launcher.
    int pool_seg, pool_nseg;
    // conv_gemm_kernel with the global-average pool behind it (conv_gap_select): != nullptr: M tiles are aligned to images (hw_img, tiles_img
    // as for F_IMGW) and every block adds the column sums of the fp16 values it stores into slot (tile of the image) % gap_splits of
    // gap_part[image][slot][gap_c] (fp32); gap_atomic: an image has more tiles than slots, the buffer was zeroed and the blocks add atomically.
    float* gap_part;
    int gap_splits, gap_c, gap_atomic;
};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// One 16-byte LDS-DMA per lane: global -> LDS without touching VGPRs.  The LDS destination of a wave instruction
// is wave-uniform base + lane*16 (1 KiB), so any bank-conflict swizzle is applied on the SOURCE side.
__device__ __forceinline__ void glds16(const void* g, half_t* l) {
    __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)l, 16, 0, 0);
}

// The same DMA as an asm statement, hidden from hipcc's s_waitcnt bookkeeping: with the builtin inside a loop, hipcc
// (ROCm 7.2) drains lgkmcnt to 0 in front of every DMA and degrades every LDS wait of the loop to lgkmcnt(0), which
// defeats fragment prefetching.  The caller counts completion itself (s_waitcnt vmcnt(N) + barrier before the ds_reads)
// and guarantees that no ds_read of the destination is outstanding.  M0 (destination base) is saved and restored.
__device__ __forceinline__ void glds16_asm(const void* g, half_t* l) {
    unsigned keep;
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)l);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(dst) : "memory");
}

// Buffer-addressed LDS-DMA helpers (conv_gemm.hip): an offset with bit 31 set is out of range for the
// 2 GiB descriptors these kernels build, so the DMA writes zeros.
#define OOB 0x80000000u
typedef __attribute__((address_space(3))) void* ldsv_t;

template <int N> __device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N <= 16, "vmcnt literal");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 13) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
    else if constexpr (N == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
    else if constexpr (N == 15) asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
}

// Accumulator tile layout.  v_mfma_f32_32x32x16_f16 leaves lane l with rows 8q + 4(l>>5) + e (q, e in 0..3; register
// 4q + e) of column l & 31.  Columns are pixels; rows are couts THROUGH THE PERMUTATION "swap bits 2 and 3": the lane
// that supplies weight row f of a 32-cout tile reads cout conv_wrow(f), so lane l ends up with the 16 couts
//     cbase + 16g + 8(l>>5) + {0..7},  g = 0, 1      (registers 8g .. 8g+7 in order)
// i.e. two runs of 8 consecutive channels = 16-byte NHWC stores (the natural order gives 4-channel / 8-byte runs, and
// the 8-byte partial-line writes cost ~30 % of a whole 1x1 layer).  The permutation keeps the weight-fragment
// ds_read_b128 bank-conflict free under both LDS swizzles (64-byte and 128-byte rows).
// Flattened output pixel -> (image, row, column) by 32-BIT unsigned divisions: a 64-bit division by a runtime value expands to ~100
// instructions, and the small-K streaming kernels (conv_pw, conv_dwpw) do two of them per 32-pixel tile.  Their launchers refuse M >= 2^31.
__device__ __forceinline__ void conv_pix_coords(const ConvParams& p, long m, long& n, int& oh, int& ow) {
    const unsigned mu = (unsigned)m, t = mu / (unsigned)p.OW, nn = t / (unsigned)p.OH;
    ow = (int)(mu - t * (unsigned)p.OW);
    oh = (int)(t - nn * (unsigned)p.OH);
    n = (long)nn;
}

__device__ __forceinline__ int conv_wrow(int f) { return (f & ~12) | ((f & 4) << 1) | ((f & 8) >> 1); }

// Per-cout epilogue constants (bias, F_DOT1 projection weights) are staged ONCE per block in LDS (conv_stage_consts;
// visible after the K loop's first wait + barrier) and read back per accumulator
// tile in the lane's register order.  Reading them from global memory inside the epilogue costs one dependent memory
// round trip per 8 couts (s_memtime trace: 7 us of a 20 us tile on the detector's last layer); holding them in
// registers across the K loop costs the occupancy the ring was sized for.
// The staging itself is a 4-byte-per-lane LDS-DMA issued BEFORE the prologue DMAs: it is then the oldest entry of the
// issuing wave's vmcnt queue, so every counted wait of the K loop covers it without changing a literal, no VGPR is
// involved and the compiler adds no wait of its own.  Wave w stages couts 64w .. 64w+63 of the block's cout tile.
// ASM = true issues it as an asm statement (kernels whose other DMAs are glds16_asm: ONE builtin LDS-DMA anywhere in a
// kernel is enough for hipcc to drop counted lgkmcnt waits everywhere in it).
template <bool ASM = false>
__device__ __forceinline__ void conv_stage_consts(float* dst, const float* src, const half_t* zero, int n0, int bn, int Np,
                                                  int wave, int lane) {
    if (wave >= 0 && wave * 64 < bn) {
        const int c = wave * 64 + lane;
        const void* g = (c < bn && n0 + c < Np) ? (const void*)(src + n0 + c) : (const void*)zero;
        if constexpr (ASM) {
            unsigned keep;
            const unsigned d = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lptr_t)(dst + wave * 64));
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(g), "s"(d) : "memory");
        } else {
            __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(dst + wave * 64), 4, 0, 0);
        }
    }
}
// `tab` = the staged table of this block's cout tile, `c` = first cout of the 32-cout accumulator tile inside it
__device__ __forceinline__ void conv_epilogue_consts(const float* tab, int c, int lane, float (&out)[16]) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const float* q = tab + c + g * 16 + (lane >> 5) * 8;
        const float4v a = *reinterpret_cast<const float4v*>(q), b = *reinterpret_cast<const float4v*>(q + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { out[g * 8 + e] = a[e]; out[g * 8 + 4 + e] = b[e]; }
    }
}

// Epilogue of one 32(cout) x 32(pixel) accumulator tile: lane l owns pixel (l & 31) — passed in as (m, n, oh, ow).
//   + bias (BN folded) -> activation -> scalar affine -> (+ residual, optionally nearest-upsampled) -> activation2
//   -> fp16 / fp32 store; F_PIXSHUF scatters a 2x2-stride-2 transposed conv.
__device__ __forceinline__ void conv_epilogue_tile(const ConvParams& p, const float16v& acc, const float (&bias)[16], long m,
                                                   long n, int oh, int ow, int cbase, int lane) {
    const bool pixshuf = p.flags & F_PIXSHUF;
    const bool has_res = p.flags & F_RES;
    long res_pix = m;
    if (has_res && p.resshift) res_pix = (n * p.res_hs + (oh >> p.resshift)) * p.res_ws + (ow >> p.resshift);
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = acc[e] + bias[e];
    vse_act_n(v, p.act, p.act_a, p.act_b);
    // the scalar affine after the activation is the identity for all but a handful of layers: one uniform branch instead of
    // 16 multiply-adds per accumulator tile (the epilogue is VALU-bound)
    if (p.post_a != 1.f || p.post_b != 0.f) {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = v[e] * p.post_a + p.post_b;
    }
    long opix[2];
    int oc[2];
    bool live[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int c0 = cbase + g * 16 + (lane >> 5) * 8;
        live[g] = c0 < p.Np;
        opix[g] = m;
        oc[g] = c0;
        if (pixshuf) {                                   // coutp % 8 == 0: a run of 8 never straddles two quads
            const int quad = c0 / p.coutp;
            oc[g] = c0 - quad * p.coutp;
            opix[g] = (n * (2 * p.OH) + 2 * oh + (quad >> 1)) * (2L * p.OW) + 2 * ow + (quad & 1);
        }
    }
    if (p.ogate != nullptr) {
        // an SE block with shortcut behind a 1x1 conv, x + x * gate(mean(x)), folded into the conv: the gate comes from the mean
        // of the conv's INPUT (the mean commutes with a 1x1 conv), so x itself is never written (compiler.py _rewrite_se_laterals)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (!live[g]) continue;
            const half8 g8 = *reinterpret_cast<const half8*>(p.ogate + n * p.ogate_ld + oc[g]);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[g * 8 + e] *= 1.0f + (float)g8[e];
        }
    }
    if (has_res) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            if (!live[g]) continue;
            const half_t* rp = p.res + res_pix * p.res_ld + oc[g];
            if (p.vec16) {
                const half8 r8 = *reinterpret_cast<const half8*>(rp);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[g * 8 + e] += (float)r8[e];
                if (p.res_lo_off) {
                    const half8 l8 = *reinterpret_cast<const half8*>(rp + p.res_lo_off);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[g * 8 + e] += (float)l8[e];
                }
            } else {
                const half4 r0 = *reinterpret_cast<const half4*>(rp), r1 = *reinterpret_cast<const half4*>(rp + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[g * 8 + e] += (float)r0[e]; v[g * 8 + 4 + e] += (float)r1[e]; }
            }
        }
    }
    vse_act_n(v, p.act2, 0.f, 0.f);
    if (p.wl_out != nullptr && ow >= p.wl_out[n]) {
        // ragged batch: this pixel lies right of its sample's own width — the next layer must see what zero padding would
        // have given it there
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = 0.f;
    }
    if (p.flags & F_ONECH) {
        // pixel-shuffle conv to ONE channel, fp32 map out (ld = 1): this lane's 8-channel run g is one quad; its first value is the pixel
#pragma unroll
        for (int g = 0; g < 2; ++g)
            if (live[g]) reinterpret_cast<float*>(p.out)[opix[g]] = v[g * 8];
        return;
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        if (!live[g]) continue;
        const float* w = v + g * 8;
        if (p.out_f32) {
            float* op = reinterpret_cast<float*>(p.out) + opix[g] * p.out_ld + oc[g];
            *reinterpret_cast<float4v*>(op) = float4v{w[0], w[1], w[2], w[3]};
            *reinterpret_cast<float4v*>(op + 4) = float4v{w[4], w[5], w[6], w[7]};
        } else {
            half_t* op = reinterpret_cast<half_t*>(p.out) + opix[g] * p.out_ld + oc[g];
            if (p.vec16) {
                const half8 hi8 = half8{(half_t)w[0], (half_t)w[1], (half_t)w[2], (half_t)w[3],
                                        (half_t)w[4], (half_t)w[5], (half_t)w[6], (half_t)w[7]};
                *reinterpret_cast<half8*>(op) = hi8;
                if (p.lo_off) {          // the tensor feeds an OP_CHAIN: what fp16 dropped travels beside it (launch_conv checks vec16)
                    half8 lo8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) lo8[e] = (half_t)(w[e] - (float)hi8[e]);
                    *reinterpret_cast<half8*>(op + p.lo_off) = lo8;
                }
            } else {
                *reinterpret_cast<half4*>(op) = half4{(half_t)w[0], (half_t)w[1], (half_t)w[2], (half_t)w[3]};
                *reinterpret_cast<half4*>(op + 4) = half4{(half_t)w[4], (half_t)w[5], (half_t)w[6], (half_t)w[7]};
            }
        }
    }
}

// Ragged batches: an output tile that lies entirely right of its sample's width holds zeros by definition — the block writes
// them (one 16-byte store per pixel and 8-channel group) and skips its prologue, K loop and epilogue.  Call before the first
// DMA / barrier; the decision is block-uniform.  TH x TW = the tile, bn = couts of the block's tile.
template <int TH, int TW>
__device__ __forceinline__ bool conv_tile_right_of_sample(const ConvParams& p, long img, int oy0, int ox0, int n0, int bn) {
    if (p.wl_out == nullptr || p.out_f32 || (p.flags & (F_DOT1 | F_PIXSHUF)) || !p.vec16) return false;
    if (ox0 < p.wl_out[img]) return false;
    const int c1 = min(n0 + bn, p.Np);
    for (int i = threadIdx.x; i < TH * TW; i += blockDim.x) {
        const int oy = oy0 + i / TW, ox = ox0 + i % TW;
        if (oy >= p.OH || ox >= p.OW) continue;
        half_t* op = reinterpret_cast<half_t*>(p.out) + ((img * p.OH + oy) * p.OW + ox) * (long)p.out_ld;
        for (int c = n0; c < c1; c += 8) *reinterpret_cast<half8*>(op + c) = half8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    return true;
}

// Column packing (conv_c3_kernel, conv_col_kernel).  A map whose width is not a multiple of the tile width leaves the last column tile of
// every row band partly empty, and a 32-lane fragment cannot be shortened: the detector's 240 / 120 / 60-wide maps cost 1/16 more
// MFMAs than their outputs need.  So G images form one VIRTUAL row band: output column v = g * OW + ox (g = image of the group), tiled
// by the same TW-wide tiles.  The input rows of the group are pictured as one AUGMENTED row: pw zero columns in front of every image,
//     n = g * (W + pw) + pw + ix        (ix = the image's own column; n % (W + pw) < pw is a gap),
// one shared gap between neighbours being enough, since pw is the conv's horizontal padding.  A tile's LDS patch is a plain window
// of that row starting at n0 = ox0 + pw * (ox0 / OW), and the lane that owns output column v reads patch columns
//     (v - ox0) + pw * (v / OW - ox0 / OW) + dx:
// every seam between ox0 and v shifts it by one gap.  Each output pixel sees the values and the K order it sees unpacked.
// The quotients are taken with a multiply-high: conv_pack_magic(d) is exact for dividends < 2^16 and d <= 2^16 (conv_pack_group
// refuses larger maps).
static inline unsigned conv_pack_magic(unsigned d) { return (unsigned)(0x100000000ull / d + 1); }
struct ConvPackTile {
    long img0;          // first image of the block's group
    int vw;             // live virtual columns of the group (a short last group has fewer than pack_g * OW)
    int vlast;          // last live virtual column of the tile
    int g0;             // image (of the group) of the tile's first column
    int n0;             // augmented column of patch column 0
    int used;           // patch columns the tile's fragments read
};
// grp = the block's image group, ox0 = first virtual column of its tile, TW = tile width, KW = filter width.  Block-uniform.
__device__ __forceinline__ ConvPackTile conv_pack_tile(const ConvParams& p, int grp, int ox0, int TW, int KW) {
    ConvPackTile t;
    t.img0 = (long)grp * p.pack_g;
    t.vw = min(p.pack_g, p.nimg - grp * p.pack_g) * p.OW;
    t.vlast = min(ox0 + TW, t.vw) - 1;
    t.g0 = (int)__umulhi((unsigned)ox0, p.pack_mag_ow);
    t.n0 = ox0 + p.pw * t.g0;
    t.used = TW + KW - 1 + p.pw * ((int)__umulhi((unsigned)max(t.vlast, 0), p.pack_mag_ow) - t.g0);
    return t;
}
// Patch column px of the tile -> (image of the group, input column); false: a gap or outside the group's live images
__device__ __forceinline__ bool conv_pack_src(const ConvParams& p, const ConvPackTile& t, int px, int& g, int& ix) {
    const unsigned n = (unsigned)(t.n0 + px);
    g = (int)__umulhi(n, p.pack_mag_d);
    ix = (int)n - g * (p.W + p.pw) - p.pw;
    return px < t.used && ix >= 0 && ix < p.W && (long)g * p.OW < t.vw;
}
// Fragment column of the lane that owns virtual output column v (lanes right of the tile's live columns read what the last one reads)
__device__ __forceinline__ int conv_pack_fragcol(const ConvParams& p, const ConvPackTile& t, int ox0, int v) {
    return v - ox0 + p.pw * ((int)__umulhi((unsigned)max(min(v, t.vlast), 0), p.pack_mag_ow) - t.g0);
}

// F_DOT1 variant: returns this lane's partial  sum_c y[c] * dotw[c]  over the couts it owns in one accumulator tile
// (y = the full epilogue value); nothing is stored.  Padded couts carry zero weights.
__device__ __forceinline__ float conv_epilogue_dot(const ConvParams& p, const float16v& acc, const float (&bias)[16],
                                                   const float (&dotw)[16]) {
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = acc[e] + bias[e];
    vse_act_n(v, p.act, p.act_a, p.act_b);
    if (p.post_a != 1.f || p.post_b != 0.f) {        // as conv_epilogue_tile: the affine is the identity almost everywhere
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = v[e] * p.post_a + p.post_b;
    }
    vse_act_n(v, p.act2, 0.f, 0.f);
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) part += v[e] * dotw[e];
    return part;
}

// ---- which kernel serves a conv record (conv_select.hip) -------------------------------------------------------------------
// conv_select() answers it from the record's parameters alone (no pointer, no HIP call); launch_conv() launches that answer and
// vse_op_kernel_name() names it.  arg[] selects one instantiation of the family: what each slot means, and which instantiations exist,
// is the family's table next to its launcher (conv_*.hip, CONV_INST).  CK_C3POOL = a conv record + the max-pool record behind it
// (conv_pool_select).
enum { CK_NONE = 0, CK_GEMM, CK_SMALLM, CK_MFMA, CK_PATCH, CK_COL, CK_C3, CK_PW, CK_DWPW, CK_HEAD, CK_STEM, CK_C3POOL, CK_FAMILIES };
struct ConvKernel {
    int family;     // CK_NONE: refused before any launcher
    int rc;         // != VSE_OK: refused with this code (a CK_PW refusal is reported by its launcher, after the launcher's own checks)
    int arg[3];
};

// One kernel instantiation: the arg[] it serves, the kernel, and its name as rocprofv3 reports the symbol (without "void " and the
// parameter list).  CONV_INST writes kernel and name from the same tokens, so spell EVERY template argument, defaulted ones too,
// separated by ", ", booleans as true / false:  CONV_INST(9, 64, 0, conv_col_kernel<9, 64>).
struct ConvInst {
    int arg[3];
    void (*fn)(const ConvParams);
    const char* name;
};
#define CONV_INST(a0, a1, a2, ...) {{a0, a1, a2}, __VA_ARGS__, #__VA_ARGS__}
// A family: its launcher (grid, block, LDS, parameter fix-ups, what only a launch can check) and its instantiations.  The launcher
// launches conv_inst()'s entry and answers VSE_E_UNSUPPORTED when there is none; conv_kernel_name() prints the same entry's name.
struct ConvFamily {
    int (*launch)(const ConvParams& p, const ConvKernel& k, hipStream_t st);
    const ConvInst* inst;
    int n;
};
template <int N>
static inline ConvFamily conv_family(int (*launch)(const ConvParams&, const ConvKernel&, hipStream_t), const ConvInst (&inst)[N]) {
    return ConvFamily{launch, inst, N};
}
static inline const ConvInst* conv_inst(const ConvFamily& f, const ConvKernel& k) {
    for (const ConvInst* e = f.inst; e != f.inst + f.n; ++e)
        if (e->arg[0] == k.arg[0] && e->arg[1] == k.arg[1] && e->arg[2] == k.arg[2]) return e;
    return nullptr;
}
// Defined beside the kernels (conv_gemm.hip ... conv_c3pool.hip), indexed by CK_* in conv_select.hip.  (Functions, not objects: a const
// object of this type would be emitted into the device code as well.)
ConvFamily conv_gemm_family(), conv_smallm_family(), conv_mfma_family(), conv_patch_family(), conv_col_family(), conv_c3_family(),
    conv_pw_family(), conv_dwpw_family(), conv_head_family(), conv_stem_family(), conv_c3pool_family();

// conv_gemm_kernel tile configurations (BM x BN, waves WM x WN, BK, stages).  Measured and dropped on MI355X (tools/bench_conv.py,
// DESIGN.md): BK = 64 rings with 2-3 stages (fewer bytes in flight per CU, -5..-25 %), 4-stage 128 x 128 (2 blocks/CU, -10 %),
// 512 x 128, 8-wave 256 x 256 (VGPR spills), and a persistent one-block-per-slot variant of every shape (-5..-15 %: the hardware
// already overlaps one block's store tail with its neighbours' K loops, and stores share vmcnt with the LDS-DMAs); 4-stage rings for
// the 16-wave tiles (128 / 112 KiB, 0..-12 %: more bytes in flight do not help, tools/ubench/fill.hip shows why: the L2 takes ~1
// request per channel clock, i.e. ~32 B/clk/CU of 64-byte row segments chip-wide, HBM streams at ~10 B/clk/CU, and a stream that
// mixes both gets ~15 B/clk/CU), BK 64 / 2 stages for 256 x 256 (8x slower: spills).
//   0: 128 x 128,  4 waves (2 x 2), BK 32, 3 stages  (48 KiB LDS, 3 blocks/CU)  — the conv_mfma_kernel shape
//   1: 256 x  64,  4 waves (4 x 1), BK 32, 3 stages  (60 KiB, 2 blocks/CU)
//   2: 256 x  32,  4 waves (4 x 1), BK 32, 3 stages
//   3: 256 x 128,  8 waves (4 x 2), BK 32, 3 stages  (72 KiB, 2 blocks/CU)
//   4: 256 x 256, 16 waves (4 x 4), BK 32, 3 stages  (96 KiB, 1 block/CU)
//   5: 256 x 192, 16 waves (8 x 2), BK 32, 3 stages  (96 KiB, 1 block/CU; weight rows staged as 256)
//   6 / 7: the same two tiles with BK 64 and 2 stages (128 KiB) for layers with cin % 64 == 0
struct GemmCfg { int bm, bn, wm, wn, bk, st; };
constexpr GemmCfg kCfg[] = {{128, 128, 2, 2, 32, 3}, {256, 64, 4, 1, 32, 3}, {256, 32, 4, 1, 32, 3}, {256, 128, 4, 2, 32, 3},
                            {256, 256, 4, 4, 32, 3}, {256, 192, 8, 2, 32, 3}, {256, 256, 4, 4, 64, 2}, {256, 192, 8, 2, 64, 2}};

// geometry of the uint8 source frames of one run (F_U8SRC plans)
struct SrcGeom { int h, w; long pitch, fstride; };
// The parameters of a conv record: in / res / in2 / out / dot_out = its resolved in0 / in1 / in2 / out / out2 views, wts = the weight
// blob, u8src = the frames of an F_U8SRC stem.  Naming passes null pointers: only the shapes count.
ConvParams conv_params(const vse_op& o, const TView& in, const TView& res, const TView& in2, const TView& out, const TView& dot_out,
                       const char* wts, const half_t* zero, const int* wl_out, const uint8_t* u8src, const SrcGeom& src);
ConvKernel conv_select(const ConvParams& p, int Kp);       // Kp = the record's P_KTOT
int conv_kernel_name(const ConvKernel& k, char* buf, size_t n);
int launch_conv(const vse_op& o, const TView& in, const TView& res, const TView& in2, const TView& out, const TView& dot_out,
                const char* wts, const half_t* zero, const int* wl_out, const uint8_t* u8src, const SrcGeom& src, hipStream_t st);
// A 3x3 conv whose only reader is the 3x3 / stride-2 max-pool record behind it runs with that pool as ONE kernel (conv_c3pool.hip): the
// conv's output tensor is then never written.  conv_pool_select() answers from the plan's records alone whether ops[i], ops[i + 1] are
// such a pair (family CK_C3POOL, else CK_NONE); vse_plan_create asks once per plan, launch_conv_pool() launches the answer with the
// conv's input view and the POOL's output view.
ConvKernel conv_pool_select(const vse_op* ops, int n_ops, int i);
int launch_conv_pool(const vse_op& conv, const ConvKernel& k, const TView& in, const TView& pool_out, const char* wts, const half_t* zero,
                     hipStream_t st);
// A 1x1 conv of conv_gemm_kernel's unmasked form whose output feeds the global-average pool record behind it sums the pool's partials in
// its own epilogue (conv_gemm.hip): the pool's pass over the tensor is not run, only its gap_finish_kernel.  conv_gap_select() answers
// from the plan's records alone whether ops[i], ops[i + 1] are such a pair; vse_plan_create asks once per plan.  The partials go to the
// pool's scratch view (in2) unless the compiler laid that over the conv's own input or output: then to `part_off`, bytes of the workspace
// that are dead while the pair runs (the output of a later record that nothing touches before that record overwrites it).
struct ConvGap {
    int fused;          // 0: two launches, as the records say
    int bm;             // row tile of the conv's configuration
    int tiles_img;      // M tiles per image
    int slots;          // slots gap_finish_kernel adds: min(splits, tiles_img)
    int atomic;         // an image has more tiles than slots (at most twice as many): zero the partial buffer in front of the conv
    int64_t part_off;   // workspace offset of the partial buffer [n][splits][c] fp32
    int64_t part_bytes;
};
ConvGap conv_gap_select(const vse_op* ops, int n_ops, int i);
// launch_conv for such a pair: `part` = the resolved partial buffer
int launch_conv_gap(const vse_op& o, const ConvGap& g, const TView& in, const TView& out, const char* wts, const half_t* zero, float* part,
                    int splits, hipStream_t st);
// An SE gate multiply (OP_SCALE) directly followed by the residual add (OP_BINARY) that reads its product runs as one pass
// (scale_add_kernel, simple_ops.hip) when the product is dead behind the add: 0 = two launches, 1 / 2 = fused, the add's in1 / in0 is
// the residual.  Decided per plan like the pairs above; ragged plans included (element-wise: no summation order is involved).
int scale_add_select(const vse_op* ops, int n_ops, int i);
// images of a launch (M = images x OH x OW)
static inline long conv_images(const ConvParams& p) { return p.OH && p.OW ? p.M / ((long)p.OH * p.OW) : 0; }
// Images per virtual row band for TW-wide tiles whose patch has `spare` unused columns and a `gap` of zero columns between images:
// G from {1, 2, 4, 8, 16} (<= images) with the fewest live tiles, the smaller G on ties; a G whose worst tile holds more seams than
// the spare columns take is left out.  1 when OW is a multiple of TW already.
int conv_pack_group(long images, int OW, int TW, int spare, int gap);
// fills p.pack_*, p.nimg and p.tiles_w for TW-wide tiles; `spare` as above.  Ragged plans and convs that change the width stay unpacked.
void conv_pack_plan(ConvParams& p, int TW, int spare);
