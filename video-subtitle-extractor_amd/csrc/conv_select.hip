// Which kernel serves an OP_CONV record, decided in one place (host code only): the record -> ConvParams step, the selector with
// the shape rules of every conv kernel family, the name of its answer, and launch_conv(), which checks the record, asks the
// selector and hands the answer to the family's launcher.  The kernels, their launchers and the tables of their instantiations stay
// in their own files.
#include <stdlib.h>
#include <cstdio>
#include "conv_common.h"

// ---- shape rules of the kernel families -------------------------------------------------------------------------------------

// conv_gemm_kernel: 0 = not eligible; 1 = masked variant; 2 = unmasked 1x1 variant.  (Mirrored by conv_route.py, gemm_ok: F_WK32.)
static int conv_gemm_mode(int kh, int kw, int sh, int sw, int ph, int pw, int cinp, int Kp, int inshift, int flags) {
    (void)sh; (void)sw;
    if (inshift || (flags & (F_PATCH | F_DOT1 | F_SRC2))) return 0;
    if (cinp % 32) return 0;
    if (kh * kw > 31) return 0;
    if (kh < 2 * ph + 1 || kw < 2 * pw) return 0;
    if (kh == 1 && kw == 1 && ph == 0 && pw == 0 && Kp == cinp) return 2;
    return 1;
}
// 32-bit offsets: the rows of one block span at most BM output pixels (+ one image seam), the tap walk kh rows
static bool conv_gemm_span_ok(const ConvParams& p, int Kp) {
    const double span = ((double)512 * p.sw + (512.0 / p.OW + 3) * p.sh * p.Ws + (double)p.kh * p.Ws + p.kw) * p.in_ld * 2;
    return !(span > 1.9e9 || (double)Kp * p.Np * 2 > 1.9e9);
}

// Which kCfg configuration serves a layer.  The kernel is bound by the L2 -> LDS fill (ablation: MFMAs and fragment reads
// are free, the DMA stream and the store tail are not), so the choice minimises fetched bytes: one cout tile when the
// couts fit 192 / 256 (the activation tile is then fetched once instead of 2-3 times), 256-pixel tiles (weights re-read
// half as often), as long as the grid still fills the 256 CUs.  Zero-padded couts cost MFMA issue slots only.
static int conv_gemm_config(int Np, int cinp, long M) {
    auto ntn = [&](int bn) { return (long)((Np + bn - 1) / bn); };
    // the 16-wave tiles run 64-deep K tiles in a 2-stage ring where the channels allow it (whole 128-byte lines per
    // activation row and half the barriers; A/B on one box: -2..-4 %); the 8-wave 256 x 128 tile loses its second block per CU
    auto deep = [&](int c) { return cinp % 64 == 0 ? c + 2 : c; };          // 4 -> 6, 5 -> 7
    if (Np <= 32) return 2;
    if (Np <= 64) return 1;
    const long mt = (M + 255) / 256;
    if (Np <= 128) return mt >= 256 ? 3 : 0;
    if (Np <= 192) return mt >= 192 ? deep(5) : (mt >= 128 ? 3 : 0);
    const double w256 = (double)ntn(256) * 256 / Np, w192 = (double)ntn(192) * 192 / Np;
    const bool pick256 = ntn(256) < ntn(192) || (ntn(256) == ntn(192) && w256 <= w192);
    if (pick256 && mt * ntn(256) >= 192 && w256 <= 1.34) return deep(4);
    if (mt * ntn(192) >= 192 && w192 <= 1.34) return deep(5);
    if (mt * ntn(256) >= 192 && w256 <= 1.34) return deep(4);
    return mt * ntn(128) >= 512 ? 3 : 0;
}

// conv_smallm_kernel: conv_gemm_kernel's unmasked 1x1 mode (mode 2) at stride 1 with at most 256 pixels, one weight stream.
static bool conv_smallm_ok(const ConvParams& p, int mode, bool same_hw) {
    return mode == 2 && p.M <= 256 && p.sh == 1 && p.sw == 1 && same_hw && !(p.flags & (F_IMGW | F_PIXSHUF | F_DOT1 | F_SRC2))
           && (p.cinp & 15) == 0;
}
// ... and (round 5) SMALL 1x1 PROBLEMS whatever their route would be: <= 256 input channels (any multiple of 8: the SVTR necks' 120 / 240
// are not multiples of 32 and ran on the 128 x 128 tile of conv_mfma_kernel), <= 4096 (32-cout x 32-pixel) wave tiles — a recogniser
// sequence's [crops, 1, T, 120] layers.  Such a launch is a handful of K steps behind a prologue and in front of an epilogue on 13-50 of
// 256 CUs (13-23 us launch to launch); there every wave is its own block with ALL its loads in flight at once.  Same K order, same bits.
static bool conv_smallk_ok(const ConvParams& p, bool same_hw) {
    return p.kh == 1 && p.kw == 1 && p.sh == 1 && p.sw == 1 && p.ph == 0 && p.pw == 0 && !p.inshift && same_hw && p.cinp > 0 && p.cinp <= 256
           && (p.cinp & 7) == 0
           && !(p.flags & (F_IMGW | F_PIXSHUF | F_DOT1 | F_SRC2 | F_PATCH | F_COL | F_PW | F_STEM | F_UP2HEAD | F_DWPRE | F_ONECH | F_TAIL2 | F_HLSUM))
           && p.M > 0 && ((p.M + 31) / 32) * ((p.Np + 31) / 32) <= 4096;
}

// conv_mfma_kernel tile: minimise padded-N waste, prefer the widest tile on ties
static int conv_tile_bn(int Np) {
    auto padded = [&](int bn) { return ((Np + bn - 1) / bn) * bn; };
    if (Np <= 32) return 32;
    if (padded(64) < padded(128)) return 64;
    return 128;
}

// conv_patch_kernel (mirrored by conv_route.py — patch_fits, patch_th, route_conv — for the compiler, which packs the weight stream for it):
//   mode 2 (LIGHT, 8-row tiles, 64 or 128 couts, two blocks per CU) when the halo patch of an 8 x 32 tile fits 352 pixels
//   (3x3, 1xk) and no 1-channel projection is fused (that needs all couts of a pixel in one wave);
//   else 64 couts per tile, 16-row tiles when they fit the 960-pixel patch (mode 1 above 640 pixels), else 8-row tiles.
// Tile height: 16 rows when the halo patch fits the LDS patch buffer (960 pixels) and the map tiles at least as well as with
// 8 rows.  (Measured twice: a 16-row x 128-cout tile — 64 px x 128 couts per wave, one block per CU, 3 or 4 taps per step,
// pipelined fast step, 254 VGPRs — is 7-20 % slower than LIGHT's two 8-row blocks: a 3x3 K loop is too short to amortise an
// un-overlapped prologue + 128-cout epilogue.)
static int conv_patch_th(int kh, int kw, int OH) {
    if ((16 + kh - 1) * (PTW + kw - 1) > 960) return 8;
    const int pad16 = (OH + 15) / 16 * 16, pad8 = (OH + 7) / 8 * 8;
    return pad16 * 100 <= pad8 * 112 ? 16 : 8;      // accept <= 12 % extra row padding for the denser wave tile
}
static void conv_patch_plan(int kh, int kw, int OH, int Np, int flags, int* th, int* bn, int* mode) {
    const bool fits = (8 + kh - 1) * (PTW + kw - 1) <= 352 && !(flags & (F_DOT1 | F_SRC2));
    if (fits) {
        *th = 8; *bn = Np > 64 ? 128 : 64; *mode = 2;
        return;
    }
    *bn = 64;
    *th = conv_patch_th(kh, kw, OH);
    *mode = (*th == 16 && (16 + kh - 1) * (PTW + kw - 1) > 640) ? 1 : 0;
    if (*mode == 1 && Np <= 32 && !(flags & F_DOT1)) *bn = 32;      // half the MFMAs and weight DMAs of a 64-cout tile
}

// conv_col_kernel (mirrored by conv_route.py, col_ok; the compiler packs the weight stream for it, F_COL)
static int conv_col_bn(int Np) { return Np > 32 ? 64 : 32; }
static bool conv_col_ok(int kh, int kw, int sh, int sw, int cinp, int Np, int flags) {
    return sh == 1 && sw == 1 && (kh == 9 || kh == 7 || kh == 5) && kw >= 3 && CTW + kw - 1 <= CPW && (cinp & 15) == 0 && Np <= 64
           && !(flags & (F_SRC2 | F_PIXSHUF | F_DOT1));
}

// conv_c3_kernel tile shape per map: estimated cost (in full tiles) of covering OH x OW with (2 RW) x (32 CW) tiles when waves outside
// the map idle (a partial tile costs ~0.35 + 0.65 * live waves / 8 of a full one).  Mirrored by conv_route.py (c3_tile_eff).
static double c3_axis_cost(int n, int unit, int waves) {      // n pixels along an axis covered by tiles of `waves` x `unit`
    const int tile = unit * waves, full = n / tile, rem = n - full * tile;
    return full + (rem ? 0.35 + 0.65 * ((rem + unit - 1) / unit) / (double)waves : 0.0);
}
static double conv_c3_plan(int OH, int OW, int* rw_out) {
    double best = 0;
    int brw = 8;
    for (int rw = 8; rw >= 2; rw >>= 1) {
        const int cw = 8 / rw;
        // partial tiles in both directions: live fraction multiplies; approximate by the product of the axis costs
        const double cost = c3_axis_cost(OH, 2, rw) * c3_axis_cost(OW, 32, cw) * 512.0;
        const double eff = (double)OH * OW / cost;
        if (eff > best + 1e-9) { best = eff; brw = rw; }
    }
    if (rw_out) *rw_out = brw;
    return best;
}
// (mirrored by conv_route.py, c3_ok)
static bool conv_c3_ok(int kh, int kw, int sh, int sw, int ph, int pw, int cinp, int flags) {
    return kh == 3 && kw == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && (cinp & 15) == 0
           && !(flags & (F_SRC2 | F_PIXSHUF | F_DOT1));
}

// Column packing of conv_c3_kernel / conv_col_kernel (conv_common.h)
int conv_pack_group(long images, int OW, int TW, int spare, int gap) {
    if (OW <= 0 || OW % TW == 0 || images < 2 || spare < 0) return 1;
    if (16L * (OW + gap) + TW + 64 >= 65536) return 1;                      // conv_pack_magic: dividends < 2^16
    auto tiles = [&](long cols) { return (cols + TW - 1) / TW; };
    long best = images * tiles(OW);
    int bg = 1;
    for (int G = 2; G <= 16 && G <= images; G *= 2) {
        int seams = 0;                                                      // worst tile of a full group
        for (long x0 = 0; x0 < (long)G * OW; x0 += TW) {
            const long x1 = (x0 + TW < (long)G * OW ? x0 + TW : (long)G * OW) - 1;
            seams = (int)(x1 / OW - x0 / OW) > seams ? (int)(x1 / OW - x0 / OW) : seams;
        }
        if (seams * gap > spare) continue;
        const long cost = images / G * tiles((long)G * OW) + tiles(images % G * OW);      // live tiles: those of a short last group's empty
        if (cost < best) { best = cost; bg = G; }                                        // columns return at once
    }
    return bg;
}
void conv_pack_plan(ConvParams& p, int TW, int spare) {
    p.nimg = (int)conv_images(p);
    const bool same_w = p.sw == 1 && p.OW == p.W && p.kw == 2 * p.pw + 1;
    p.pack_g = (p.wl_out != nullptr || !same_w) ? 1 : conv_pack_group(p.nimg, p.OW, TW, spare, p.pw);
    p.pack_mag_ow = p.pack_g > 1 ? conv_pack_magic((unsigned)p.OW) : 0u;
    p.pack_mag_d = p.pack_g > 1 ? conv_pack_magic((unsigned)(p.W + p.pw)) : 0u;
    p.tiles_w = (int)(((long)p.pack_g * p.OW + TW - 1) / TW);
}

// (mirrored by conv_route.py, pw_ok)
static bool conv_pw_ok(int kh, int kw, int sh, int sw, int ph, int pw, int cinp, int Np, int inshift, int flags) {
    return kh == 1 && kw == 1 && sh == 1 && sw == 1 && ph == 0 && pw == 0 && inshift == 0 && (cinp & 7) == 0
           && cinp <= ((flags & F_HILO) ? 96 : 64)      // (hi + lo nets: a 48-channel PAIR tensor is 96 input channels — round 5)
           && Np <= ((flags & F_HILO) ? PW_MAXN_HILO : PW_MAXN) && !(flags & (F_SRC2 | F_DOT1 | F_PATCH | F_COL));
}

// conv_dwpw: 5 x 5 filters stay on two launches (25 taps per lane: 0.21 against 0.09 + 0.04 ms, and the unrolled form spills)
static bool conv_dwpw_ok(int k, int s, int cinp, int Np, int flags) {
    return k == 3 && (s == 1 || s == 2) && (cinp & 7) == 0 && cinp <= 96 && Np <= 192 && (flags & F_HILO)
           && !(flags & (F_SRC2 | F_DOT1 | F_PATCH | F_COL | F_PIXSHUF | F_IMGW | F_STEM));
}
// Stride of the row-streaming form (conv_dwpw_rows_kernel), 0 = the tile form.  The row-streaming form takes 3 x 3 'same' filters
// (pad 1) over <= 3 slices of 16 channels: there the row-invariant depthwise weights stay in registers (see LAUNDER in the kernel).
// Wider units measured SLOWER than the tile form with the weight reads left in the row loop (96 -> 192 @34 x 60, stride 2: 0.208 vs
// 0.168 ms) and spill with them hoisted: they keep the tile form.  Only PAIR inputs take it: on plain fp16 inputs (the layer-by-layer
// programs) the tile form measures the same or better (16 -> 32 @272 x 480: 0.373 vs 0.365 ms, 48 -> 48 @136 x 240: 0.215 vs 0.286) —
// half the gathers and half the multiply-adds per pixel leave little for the strip walk to save.
static int conv_dwpw_rows_stride(int k, int pad, int s, int cinp, int lo_in) {
    const int ks = (cinp + 15) / 16;
    return (lo_in != 0 && k == 3 && pad == 1 && ((s == 1 && ks <= DWPW_ROWS_MAX_KS_S1) || (s == 2 && ks <= DWPW_ROWS_MAX_KS))) ? s : 0;
}

// ---- record -> parameters -----------------------------------------------------------------------------------------------------

ConvParams conv_params(const vse_op& o, const TView& in, const TView& res, const TView& in2, const TView& out, const TView& dot_out,
                       const char* wts, const half_t* zero, const int* wl_out, const uint8_t* u8src, const SrcGeom& src) {
    auto blob = [&](long off) { return wts ? wts + off : nullptr; };
    const int flags = o.flags;
    ConvParams p{};
    p.in = reinterpret_cast<const half_t*>(in.ptr);
    p.w = reinterpret_cast<const half_t*>((flags & F_IMGW) ? in2.ptr : blob(o.w_off));     // F_IMGW: per-image weights in the workspace
    p.bias = reinterpret_cast<const float*>(blob(o.b_off));
    p.res = reinterpret_cast<const half_t*>(res.ptr);
    p.out = out.ptr;
    p.zero = zero;
    p.inshift = o.p[P_INSHIFT];
    p.Hs = in.h;
    p.Ws = in.w;
    p.H = in.h << p.inshift;
    p.W = in.w << p.inshift;
    p.in_ld = in.ld;
    p.cinp = o.p[P_CINP];
    p.kh = o.p[P_KH]; p.kw = o.p[P_KW]; p.sh = o.p[P_SH]; p.sw = o.p[P_SW]; p.ph = o.p[P_PH]; p.pw = o.p[P_PW];
    p.OH = (p.H + 2 * p.ph - p.kh) / p.sh + 1;
    p.OW = (p.W + 2 * p.pw - p.kw) / p.sw + 1;
    p.M = (long)in.n * p.OH * p.OW;
    p.Np = o.p[P_COUT];
    p.nk = o.p[P_KTOT] / 32;                  // conv_mfma_kernel's 32-deep K tiles (the other launchers derive theirs from nkh)
    p.nkh = p.nk;
    if (flags & F_HILO) p.nk *= 2;            // second pass over the same activations with the lo weight tiles
    p.out_ld = out.ld;
    p.out_f32 = (flags & F_OUT_F32) ? 1 : 0;
    p.res_ld = res.ld;
    p.resshift = o.p[P_RESSHIFT];
    p.res_hs = res.h;
    p.res_ws = res.w;
    p.act = o.p[P_ACT]; p.act2 = o.p[P_ACT2];
    p.act_a = o.f[FS_ACT_A]; p.act_b = o.f[FS_ACT_B]; p.post_a = o.f[FS_POST_A]; p.post_b = o.f[FS_POST_B];
    p.flags = flags;
    p.coutp = (flags & F_PIXSHUF) ? p.Np / 4 : p.Np;
    p.vec16 = ((reinterpret_cast<uintptr_t>(out.ptr) & 15) == 0 && ((long)out.ld * out.esize) % 16 == 0 &&
               (!(flags & F_RES) || ((reinterpret_cast<uintptr_t>(res.ptr) & 15) == 0 && (res.ld & 7) == 0))) ? 1 : 0;
    p.dotw = reinterpret_cast<const float*>(blob(o.aux_off));
    p.dotb = o.f[FS_PRE_B]; p.dotact = o.p[P_DOTACT];
    p.dot_out = dot_out.ptr; p.dot_f32 = dot_out.esize == 4; p.dot_ld = dot_out.ld;
    p.in2 = reinterpret_cast<const half_t*>(in2.ptr); p.in2_ld = in2.ld; p.in2_shift = o.p[P_IN2SHIFT];
    p.in2_hs = in2.h; p.in2_ws = in2.w; p.nv0 = in.c >> 3;
    if (flags & F_IMGW) {
        p.wimg_stride = (long)o.p[P_KTOT] * p.Np;
        p.hw_img = p.OH * p.OW;
    }
    p.wl_out = wl_out;
    p.lo_off = o.p[P_LO_OUT];
    p.res_lo_off = (flags & F_RES) ? o.p[P_LO_RES] : 0;
    p.in_lo_off = (flags & F_DWPRE) ? o.p[P_LO_IN] : 0;
    if (flags & F_OGATE) {                    // (in2 carries the gate)
        p.ogate = reinterpret_cast<const half_t*>(in2.ptr);
        p.ogate_ld = in2.ld;
    }
    if (flags & F_U8SRC) {
        p.u8src = u8src;
        p.u8_h = src.h; p.u8_w = src.w; p.u8_pitch = src.pitch; p.u8_fstride = src.fstride;
    }
    return p;
}

// ---- the selector -------------------------------------------------------------------------------------------------------------

static bool head_resident() {
    // the persistent resident-weight form unless VSE_HEAD_RESIDENT is a number that reads as 0
    static const bool resident = [] { const char* e = getenv("VSE_HEAD_RESIDENT"); return e && e[0] ? atoi(e) != 0 : true; }();
    return resident;
}

ConvKernel conv_select(const ConvParams& p, int Kp) {
    auto refuse = [](int rc) { return ConvKernel{CK_NONE, rc, {0, 0, 0}}; };
    auto pick = [](int family, int a0, int a1 = 0, int a2 = 0) { return ConvKernel{family, VSE_OK, {a0, a1, a2}}; };
    const int f = p.flags;
    const bool hilo = (f & F_HILO) != 0;
    if (f & F_IMGW) {
        // per-image weights (an SE gate folded into a 1x1 consumer): the unmasked conv_gemm_kernel only, M tiles aligned to images
        if (p.kh != 1 || p.kw != 1 || (f & (F_SRC2 | F_DOT1 | F_PATCH | F_COL | F_PW | F_HILO | F_PIXSHUF))) return refuse(VSE_E_UNSUPPORTED);
        const int mode = conv_gemm_mode(p.kh, p.kw, p.sh, p.sw, p.ph, p.pw, p.cinp, Kp, p.inshift, f);
        if (mode != 2 || !conv_gemm_span_ok(p, Kp) || p.hw_img <= 0 || p.M % p.hw_img) return refuse(VSE_E_UNSUPPORTED);
        return pick(CK_GEMM, conv_gemm_config(p.Np, p.cinp, p.M), 0);
    }
    if (f & F_DWPRE) {
        if (!(f & F_PW) || p.inshift || (p.in_lo_off && ((p.in_lo_off & 7) || p.in_ld < p.in_lo_off + p.cinp))) return refuse(VSE_E_INVAL);
        if (!conv_dwpw_ok(p.kh, p.sh, p.cinp, p.Np, f) || p.kh != p.kw || p.sh != p.sw || p.ph != p.pw) return refuse(VSE_E_UNSUPPORTED);
        return pick(CK_DWPW, (p.cinp + 15) / 16, p.in_lo_off != 0, conv_dwpw_rows_stride(p.kh, p.ph, p.sh, p.cinp, p.in_lo_off));
    }
    if ((f & (F_DOT1 | F_SRC2)) && !(f & (F_PATCH | F_COL))) return refuse(VSE_E_UNSUPPORTED);
    if (f & F_UP2HEAD) return pick(CK_HEAD, head_resident());
    if (f & F_STEM) return pick(CK_STEM, p.sh == 2 ? 2 : 1, hilo, (f & F_U8SRC) != 0);
    if (f & F_PW) {
        if (!conv_pw_ok(p.kh, p.kw, p.sh, p.sw, p.ph, p.pw, p.cinp, p.Np, p.inshift, f)) return refuse(VSE_E_UNSUPPORTED);
        const int ks = (p.cinp + 15) / 16;
        ConvKernel k = pick(CK_PW, ks, hilo, (f & F_TAIL2) != 0);
        if ((f & F_TAIL2) && ks != 2 && ks != 4) k.rc = VSE_E_UNSUPPORTED;      // (the tail is built for 32 and 64 input channels)
        return k;
    }
    if (f & F_COL) {
        if (p.kh == 3 && p.kw == 3) {
            if (!conv_c3_ok(p.kh, p.kw, p.sh, p.sw, p.ph, p.pw, p.cinp, f)) return refuse(VSE_E_UNSUPPORTED);
            int rw;
            conv_c3_plan(p.OH, p.OW, &rw);
            return pick(CK_C3, rw, p.Np <= 32 && !(f & F_HLSUM));     // F_HLSUM: the 64-row form (hi | lo)
        }
        if (!conv_col_ok(p.kh, p.kw, p.sh, p.sw, p.cinp, p.Np, f)) return refuse(VSE_E_UNSUPPORTED);
        return pick(CK_COL, p.kh, conv_col_bn(p.Np));
    }
    if (f & F_PATCH) {
        int th, bn, mode;
        conv_patch_plan(p.kh, p.kw, p.OH, p.Np, f, &th, &bn, &mode);
        return pick(CK_PATCH, th, bn, mode);
    }
    if (Kp % 64) return refuse(VSE_E_INVAL);
    const int kt = (f & F_WK32) ? 32 : 64;
    const bool same_hw = p.H == p.OH && p.W == p.OW && p.Hs == p.H && p.Ws == p.W;
    if (conv_smallk_ok(p, same_hw)) return pick(CK_SMALLM, kt, hilo);        // a small 1x1 problem: one wave per 32 x 32 tile
    const int mode = conv_gemm_mode(p.kh, p.kw, p.sh, p.sw, p.ph, p.pw, p.cinp, Kp, p.inshift, f);
    if (mode && conv_smallm_ok(p, mode, same_hw)) return pick(CK_SMALLM, kt, hilo);   // a handful of pixels (SE gates)
    if (mode && conv_gemm_span_ok(p, Kp)) return pick(CK_GEMM, conv_gemm_config(p.Np, p.cinp, p.M), mode == 1);
    if (f & F_WK32) return refuse(VSE_E_UNSUPPORTED);     // 32-deep weight tiles are read by conv_gemm_kernel and conv_smallm only
    return pick(CK_MFMA, conv_tile_bn(p.Np), p.inshift != 0);
}

// ---- the families: launcher and instantiations of each (defined beside the kernels), by CK_* ---------------------------------------

static const ConvFamily& conv_family_of(int family) {
    static const ConvFamily fam[CK_FAMILIES] = {
        ConvFamily{nullptr, nullptr, 0}, conv_gemm_family(), conv_smallm_family(), conv_mfma_family(), conv_patch_family(), conv_col_family(),
        conv_c3_family(), conv_pw_family(), conv_dwpw_family(), conv_head_family(), conv_stem_family(), conv_c3pool_family()};
    return fam[family > CK_NONE && family < CK_FAMILIES ? family : CK_NONE];
}

// a family outside the registry is refused like a choice outside the family's table
static int conv_launch(const ConvParams& p, const ConvKernel& k, hipStream_t st) {
    const ConvFamily& f = conv_family_of(k.family);
    return f.launch ? f.launch(p, k, st) : VSE_E_UNSUPPORTED;
}

// The instantiation `k` names: the name in its table entry, which is the kernel the family's launcher launches for `k`.
int conv_kernel_name(const ConvKernel& k, char* buf, size_t n) {
    if (k.rc != VSE_OK) return snprintf(buf, n, "(refused: %d)", k.rc);
    const ConvFamily& f = conv_family_of(k.family);
    const ConvInst* inst = conv_inst(f, k);
    if (!inst) return snprintf(buf, n, "(no instantiation: family %d<%d, %d, %d>)", k.family, k.arg[0], k.arg[1], k.arg[2]);
    return snprintf(buf, n, "%s", inst->name);
}

// ---- conv + max-pool pairs that run as one kernel ------------------------------------------------------------------------------

// byte range [lo, hi) a view spans in its arena (channel slices of one buffer count as overlapping: conservative)
static void view_span(const vse_view& v, int64_t* lo, int64_t* hi) {
    *lo = v.off;
    *hi = v.off + (((int64_t)v.n * v.h * v.w - 1) * v.ld + v.c) * v.esize;
}
static bool views_overlap(const vse_view& a, const vse_view& b) {
    if (a.n == 0 || b.n == 0 || a.arena != b.arena) return false;
    int64_t a0, a1, b0, b1;
    view_span(a, &a0, &a1);
    view_span(b, &b0, &b1);
    return a0 < b1 && b0 < a1;
}
static bool same_view(const vse_view& a, const vse_view& b) {
    return a.off == b.off && a.arena == b.arena && a.n == b.n && a.h == b.h && a.w == b.w && a.c == b.c && a.ld == b.ld && a.esize == b.esize;
}

// ops[i] = a 3x3 / stride-1 / pad-1 conv of conv_patch_kernel's LIGHT family with a plain epilogue (bias / BN / activation), ops[i + 1] = a
// 3x3 / stride-2 / pad-1 max-pool whose one input is exactly the conv's output view, neither of them ragged; and the conv's output is DEAD
// behind the pool: fused, that tensor is never written, so walking the later records, the first one that touches its bytes must write them
// without reading them (or none touches them).  The fused kernel reads the conv's input while it writes the pool's output, which the
// unfused pair never does at the same time: those two views must not share bytes either.
ConvKernel conv_pool_select(const vse_op* ops, int n_ops, int i) {
    const ConvKernel no{CK_NONE, VSE_OK, {0, 0, 0}};
    if (!ops || i < 0 || i + 1 >= n_ops) return no;
    const vse_op &c = ops[i], &q = ops[i + 1];
    if (c.kind != OP_CONV || q.kind != OP_POOL) return no;
    if (c.flags != F_PATCH || c.p[P_KH] != 3 || c.p[P_KW] != 3 || c.p[P_SH] != 1 || c.p[P_SW] != 1 || c.p[P_PH] != 1 || c.p[P_PW] != 1) return no;
    if (c.p[P_INSHIFT] || c.p[P_LO_OUT] || c.p[P_WLIN] || c.p[P_WLOUT] || q.p[P_WLIN] || q.p[P_WLOUT]) return no;
    if (c.in1.n || c.in2.n || c.out2.n || q.in1.n || q.in2.n || q.out2.n) return no;
    if (!q.p[P_POOL_MAX] || q.p[P_KH] != 3 || q.p[P_KW] != 3 || q.p[P_SH] != 2 || q.p[P_SW] != 2 || q.p[P_PH] != 1 || q.p[P_PW] != 1) return no;
    if (c.out.arena != 0 || c.out.esize != 2 || c.in0.esize != 2 || !same_view(c.out, q.in0)) return no;
    if (c.out.n != c.in0.n || c.out.h != c.in0.h || c.out.w != c.in0.w || c.out.c != c.p[P_COUT] || (c.p[P_COUT] & 7)) return no;
    if (q.out.esize != 2 || q.out.n != c.out.n || q.out.h != (c.out.h - 1) / 2 + 1 || q.out.w != (c.out.w - 1) / 2 + 1 || q.out.c != c.out.c ||
        (q.out.ld & 7) || (q.out.off & 15))
        return no;
    if (views_overlap(c.in0, q.out) || views_overlap(c.out, q.out) || views_overlap(c.out, c.in0)) return no;
    int th, bn, mode;
    conv_patch_plan(3, 3, c.out.h, c.p[P_COUT], c.flags, &th, &bn, &mode);
    if (mode != 2) return no;
    for (int j = i + 2; j < n_ops; ++j) {
        const vse_op& o = ops[j];
        // (in2 and out2 carry an output of some kinds and an input of others: whichever, touching the tensor there counts as reading it)
        if (views_overlap(o.in0, c.out) || views_overlap(o.in1, c.out) || views_overlap(o.in2, c.out) || views_overlap(o.out2, c.out)) return no;
        if (views_overlap(o.out, c.out)) break;
    }
    return ConvKernel{CK_C3POOL, VSE_OK, {bn, 0, 0}};
}

int launch_conv_pool(const vse_op& conv, const ConvKernel& k, const TView& in, const TView& pool_out, const char* wts, const half_t* zero,
                     hipStream_t st) {
    if (k.family != CK_C3POOL || !in.ptr || !pool_out.ptr || !zero) return VSE_E_INVAL;
    const TView none{nullptr, 0, 0, 0, 0, 0, 0};
    // the conv's own output view is only a shape here: the kernel stores through the pool's
    const TView shape{nullptr, conv.out.n, conv.out.h, conv.out.w, conv.out.c, conv.out.ld, conv.out.esize};
    ConvParams p = conv_params(conv, in, none, none, shape, none, wts, zero, nullptr, nullptr, SrcGeom{0, 0, 0, 0});
    if (in.c != p.cinp || (in.ld & 7)) return VSE_E_INVAL;
    p.out = pool_out.ptr;
    p.out_ld = pool_out.ld;
    return conv_launch(p, k, st);
}

// ---- 1x1 conv + global-average pool pairs: the conv sums the pool's partials -------------------------------------------------------

static bool touches_range(const vse_view& v, int64_t lo, int64_t hi) {          // workspace bytes [lo, hi)
    if (v.n == 0 || v.arena != 0) return false;
    int64_t a, b;
    view_span(v, &a, &b);
    return a < hi && lo < b;
}
static bool reads_range(const vse_op& o, int64_t lo, int64_t hi) {              // (in2 / out2: as in conv_pool_select)
    return touches_range(o.in0, lo, hi) || touches_range(o.in1, lo, hi) || touches_range(o.in2, lo, hi) || touches_range(o.out2, lo, hi);
}

// ops[i] = a 1x1 / stride-1 conv that conv_select sends to conv_gemm_kernel's unmasked form, with a plain epilogue (bias / BN / activation,
// fp16, 16-byte stores), ops[i + 1] = a global-average pool over exactly the conv's output view with an fp32 scratch view [n][splits][c],
// neither of them ragged, and an image has at most two row tiles per slot (two contributors to a zeroed slot add in either order to the
// same bits; three would not).
// The fused conv WRITES the partials while its other blocks still read its input, which the unfused pair never does: the compiler is free
// to lay the pool's scratch over the conv's input, dead behind the conv (the server detector's second, third and last stage do).  Then the
// partials go to other workspace bytes that are dead while the pair runs: the head of a later record's dense output (a view without
// padding, rewritten whole) that no record from the pool to that one touches and that that record overwrites without reading it, or an
// end of an earlier record's that nothing touches any more.  No such bytes: two launches.
ConvGap conv_gap_select(const vse_op* ops, int n_ops, int i) {
    const ConvGap no{0, 0, 0, 0, 0, 0, 0};
    if (!ops || i < 0 || i + 1 >= n_ops) return no;
    const vse_op &c = ops[i], &q = ops[i + 1];
    if (c.kind != OP_CONV || q.kind != OP_GAP) return no;
    if ((c.flags & ~F_WK32) || c.p[P_KH] != 1 || c.p[P_KW] != 1 || c.p[P_SH] != 1 || c.p[P_SW] != 1 || c.p[P_PH] || c.p[P_PW]) return no;
    if (c.p[P_INSHIFT] || c.p[P_LO_OUT] || c.p[P_WLIN] || c.p[P_WLOUT] || q.p[P_WLIN] || q.p[P_WLOUT]) return no;
    if (c.in1.n || c.in2.n || c.out2.n || q.in1.n || q.out2.n) return no;
    if (c.in0.arena != 0 || c.out.arena != 0 || c.out.esize != 2 || c.in0.esize != 2 || !same_view(c.out, q.in0)) return no;
    if (c.out.n < 1 || c.out.n != c.in0.n || c.out.h != c.in0.h || c.out.w != c.in0.w || c.out.c != c.p[P_COUT] || (c.out.ld & 7) || (c.out.off & 15))
        return no;
    const vse_view& s = q.in2;
    if (s.arena != 0 || s.n != c.out.n || s.esize != 4 || s.h < 1 || s.w != 1 || s.c != c.out.c || s.ld != s.c || (s.off & 3)) return no;
    if (q.out.arena != 0 || q.out.n != c.out.n || q.out.c != c.out.c || q.out.esize != 2) return no;
    auto shape = [](const vse_view& v) { return TView{nullptr, v.n, v.h, v.w, v.c, v.ld, v.esize}; };
    const TView none{nullptr, 0, 0, 0, 0, 0, 0};
    const ConvParams p = conv_params(c, shape(c.in0), none, none, shape(c.out), none, nullptr, nullptr, nullptr, nullptr, SrcGeom{0, 0, 0, 0});
    const ConvKernel k = conv_select(p, c.p[P_KTOT]);
    if (k.family != CK_GEMM || k.rc != VSE_OK || k.arg[1] != 0 || c.in0.c != p.cinp) return no;
    ConvGap g = no;
    g.bm = kCfg[k.arg[0]].bm;
    const long hw = (long)c.out.h * c.out.w;
    if (hw < 1 || hw > 0x7fffffffl) return no;
    g.tiles_img = (int)((hw + g.bm - 1) / g.bm);
    if (g.tiles_img > 2 * s.h) return no;
    g.slots = g.tiles_img < s.h ? g.tiles_img : s.h;
    g.atomic = g.tiles_img > s.h;
    g.part_bytes = (int64_t)s.n * s.h * s.c * 4;
    auto free_of_the_pair = [&](int64_t lo, int64_t hi) {
        return !touches_range(c.in0, lo, hi) && !touches_range(c.out, lo, hi) && !touches_range(q.out, lo, hi);
    };
    if (free_of_the_pair(s.off, s.off + g.part_bytes)) {
        g.part_off = s.off;
        g.fused = 1;
        return g;
    }
    for (int j = i + 2; j < n_ops && !g.fused; ++j) {
        const vse_view& r = ops[j].out;
        int64_t lo, hi;
        if (r.n == 0 || r.arena != 0 || r.ld != r.c || (r.off & 15)) continue;
        view_span(r, &lo, &hi);
        if (hi - lo < g.part_bytes) continue;
        hi = lo + g.part_bytes;
        if (!free_of_the_pair(lo, hi) || reads_range(ops[j], lo, hi)) continue;
        if (ops[j].kind == OP_CONV && conv_pool_select(ops, n_ops, j).family == CK_C3POOL) continue;      // (never writes that view)
        bool dead = true;
        for (int m = i + 2; m < j && dead; ++m) dead = !reads_range(ops[m], lo, hi) && !touches_range(ops[m].out, lo, hi);
        if (!dead) continue;
        g.part_off = lo;
        g.fused = 1;
    }
    // ... or the head or the tail of an EARLIER record's dense output that no record from the conv on touches again.  The next run finds
    // the partials there: walking its records up to the conv, the first that touches those bytes must overwrite them whole without reading
    // them.  (A conv that runs with its max-pool as one kernel never writes its output view and that pool never reads it: neither counts.)
    auto runs_pooled = [&](int m) { return ops[m].kind == OP_CONV && conv_pool_select(ops, n_ops, m).family == CK_C3POOL; };
    auto dead_from_here = [&](int64_t lo, int64_t hi) {
        if (!free_of_the_pair(lo, hi)) return false;
        for (int m = i; m < n_ops; ++m)
            if (reads_range(ops[m], lo, hi) || touches_range(ops[m].out, lo, hi)) return false;
        for (int m = 0; m < i; ++m) {
            const bool pooled = runs_pooled(m);
            if (m > 0 && ops[m].kind == OP_POOL && runs_pooled(m - 1)) {                  // (launches nothing; stores through its out)
                if (touches_range(ops[m].in1, lo, hi) || touches_range(ops[m].in2, lo, hi) || touches_range(ops[m].out2, lo, hi)) return false;
            } else if (reads_range(ops[m], lo, hi)) {
                return false;
            }
            if (!touches_range(ops[m].out, lo, hi) || pooled) continue;
            int64_t a, b;
            view_span(ops[m].out, &a, &b);
            return ops[m].out.ld == ops[m].out.c && a <= lo && hi <= b;
        }
        return true;
    };
    for (int j = 0; j < i && !g.fused; ++j) {
        const vse_view& r = ops[j].out;
        int64_t lo, hi;
        if (r.n == 0 || r.arena != 0 || r.ld != r.c || (r.off & 15)) continue;
        view_span(r, &lo, &hi);
        if (hi - lo < g.part_bytes) continue;
        const int64_t tail = (hi - g.part_bytes) & ~(int64_t)15;
        if (dead_from_here(lo, lo + g.part_bytes)) g.part_off = lo, g.fused = 1;
        else if (tail >= lo && dead_from_here(tail, tail + g.part_bytes)) g.part_off = tail, g.fused = 1;
    }
    return g.fused ? g : no;
}

int launch_conv_gap(const vse_op& o, const ConvGap& g, const TView& in, const TView& out, const char* wts, const half_t* zero, float* part,
                    int splits, hipStream_t st) {
    if (!g.fused || !in.ptr || !out.ptr || !part || !zero || splits < 1) return VSE_E_INVAL;
    const TView none{nullptr, 0, 0, 0, 0, 0, 0};
    ConvParams p = conv_params(o, in, none, none, out, none, wts, zero, nullptr, nullptr, SrcGeom{0, 0, 0, 0});
    if (in.c != p.cinp || in.esize != 2 || (in.ld & 7) || (p.Np & 7) || !p.vec16 || out.h != p.OH || out.w != p.OW || out.n != in.n) return VSE_E_INVAL;
    const ConvKernel k = conv_select(p, o.p[P_KTOT]);
    if (k.family != CK_GEMM || k.rc != VSE_OK || k.arg[1] != 0 || kCfg[k.arg[0]].bm != g.bm) return VSE_E_INVAL;
    p.hw_img = p.OH * p.OW;
    p.gap_part = part;
    p.gap_splits = splits;
    p.gap_c = out.c;
    p.gap_atomic = g.atomic;
    return conv_launch(p, k, st);
}

// ---- SE gate multiply + residual add pairs that run as one pass ---------------------------------------------------------------------

// ops[i] = an OP_SCALE without F_RES (x * gate), ops[i + 1] = an OP_BINARY add at the same resolution one of whose operands is exactly
// the scale's output view, all four tensors of one shape, both records on the same width levels (the kernels of neither look at them);
// and the product is DEAD behind the add (conv_pool_select's walk): fused, it is never written.  The fused pass reads x and the
// residual while it writes the add's output, so that output may be x or the residual ITSELF (element for element) but may not
// overlap them, or the gate, in any other way.  -> 0: two launches; 1 / 2: the add's in1 / in0 is the residual.
int scale_add_select(const vse_op* ops, int n_ops, int i) {
    if (!ops || i < 0 || i + 1 >= n_ops) return 0;
    const vse_op &s = ops[i], &b = ops[i + 1];
    if (s.kind != OP_SCALE || b.kind != OP_BINARY || s.flags || b.flags || b.p[0] || b.p[1]) return 0;
    if (s.p[P_WLIN] != b.p[P_WLIN] || s.p[P_WLOUT] != b.p[P_WLOUT]) return 0;
    const int which = same_view(s.out, b.in0) ? 1 : (same_view(s.out, b.in1) ? 2 : 0);
    if (!which || s.out.arena != 0) return 0;
    const vse_view &x = s.in0, &gate = s.in1, &res = which == 1 ? b.in1 : b.in0, &out = b.out;
    const vse_view* big[4] = {&x, &s.out, &res, &out};
    for (const vse_view* v : big)
        if (v->n != x.n || v->h != x.h || v->w != x.w || v->c != x.c || v->esize != 2 || (v->ld & 7) || (v->off & 15) || v->n < 1) return 0;
    if ((x.c & 7) || gate.n != x.n || gate.h != 1 || gate.w != 1 || gate.c != x.c || gate.esize != 2 || (gate.ld & 7) || (gate.off & 15)) return 0;
    if (same_view(res, s.out)) return 0;                                        // (t + t)
    if ((views_overlap(out, x) && !same_view(out, x)) || (views_overlap(out, res) && !same_view(out, res)) || views_overlap(out, gate)) return 0;
    if (same_view(out, s.out)) return which;              // the add in place over the product: the same bytes hold the same sums afterwards
    if (views_overlap(out, s.out)) return 0;
    for (int j = i + 2; j < n_ops; ++j) {
        const vse_op& o = ops[j];
        if (views_overlap(o.in0, s.out) || views_overlap(o.in1, s.out) || views_overlap(o.in2, s.out) || views_overlap(o.out2, s.out)) return 0;
        if (views_overlap(o.out, s.out)) break;
    }
    return which;
}

// ---- launch -----------------------------------------------------------------------------------------------------------------

int launch_conv(const vse_op& o, const TView& in, const TView& res, const TView& in2, const TView& out, const TView& dot_out,
                const char* wts, const half_t* zero, const int* wl_out, const uint8_t* u8src, const SrcGeom& src, hipStream_t st) {
    const ConvParams p = conv_params(o, in, res, in2, out, dot_out, wts, zero, wl_out, u8src, src);
    const int f = p.flags, Np = p.Np, cinp = p.cinp;
    if (f & F_SRC2) {
        if (!in2.ptr || in2.esize != 2 || (in2.ld & 7) || in.c + in2.c != cinp) return VSE_E_INVAL;
        if ((in2.h << p.in2_shift) != p.H || (in2.w << p.in2_shift) != p.W) return VSE_E_INVAL;
    } else if (in.c != cinp) {
        return VSE_E_INVAL;
    }
    // (F_UP2HEAD reads ONE channel of in0 at pixel stride ld: the dense map of an F_TAIL2 producer has ld = 1)
    if (in.esize != 2 || ((in.ld & 7) && !((f & F_UP2HEAD) && in.ld == 1)) || (cinp & 7)) return VSE_E_INVAL;
    if ((f & F_RES) && (res.esize != 2 || (res.ld & 3))) return VSE_E_INVAL;
    if ((!(f & (F_DOT1 | F_ONECH)) && (out.ld & 3)) || (Np & 7)) return VSE_E_INVAL;
    if ((f & F_ONECH) && (!(f & F_PIXSHUF) || !(f & F_OUT_F32) || Np != 32 || out.ld != 1 || out.esize != 4 || (f & F_RES)))
        return VSE_E_INVAL;
    // sanity on the output view: [n, OH(*2), OW(*2)]
    const int mul = (f & F_PIXSHUF) ? 2 : 1;
    if (out.h != p.OH * mul || out.w != p.OW * mul || out.n != in.n) return VSE_E_INVAL;
    if (p.res_lo_off && (!p.vec16 || p.resshift || (p.res_lo_off & 7))) return VSE_E_INVAL;
    if (p.lo_off && (!p.vec16 || (f & (F_OUT_F32 | F_ONECH | F_DOT1 | F_UP2HEAD)) || (p.lo_off & 7) || out.ld < p.lo_off + Np / ((f & F_PIXSHUF) ? 4 : 1)))
        return VSE_E_INVAL;
    if ((f & F_OGATE) && ((f & (F_SRC2 | F_IMGW | F_PIXSHUF | F_DOT1 | F_UP2HEAD)) || !in2.ptr || in2.esize != 2 || in2.n != in.n || in2.h != 1
                          || in2.w != 1 || in2.c < Np || (in2.ld & 7) || (reinterpret_cast<uintptr_t>(in2.ptr) & 15)))
        return VSE_E_INVAL;
    if ((f & F_U8SRC) && (!(f & F_STEM) || !p.u8src || p.u8_h <= 0 || p.u8_w <= 0)) return VSE_E_INVAL;
    if (p.wl_out && (f & (F_DOT1 | F_SRC2 | F_UP2HEAD | F_PIXSHUF))) return VSE_E_UNSUPPORTED;   // no per-sample width in these forms
    const ConvKernel k = conv_select(p, o.p[P_KTOT]);
    if (k.family == CK_NONE) return k.rc;
    if (!p.zero && !(f & (F_IMGW | F_DWPRE))) return VSE_E_INVAL;
    return conv_launch(p, k, st);
}
