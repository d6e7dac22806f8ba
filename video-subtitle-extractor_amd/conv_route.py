"""Which kernel family a dense conv layer is flagged and packed for: the compiler's half of the kernel choice.

The library picks the kernel of an OP_CONV record in conv_select() (csrc/conv_select.hip) from the record's flags and shape.  The
compiler decides what the record says: the family flag (F_PATCH, F_COL, F_PW, F_STEM, F_WK32 ...), how the weight stream is packed
and the P_KTOT it carries — and the packing must match the variant the library picks later.  route_conv() makes that decision from
plain values, without compiler state; the rules of the library it depends on are restated in the helpers below, one helper per C
function (tests/test_kernel_names.py holds the two sides together).  conv_select itself is NOT restated: which tile shape or
instantiation serves a record is the library's business unless packing or flags depend on it."""
from dataclasses import dataclass

from . import ir


def rup(x, m):
    return (x + m - 1) // m * m


@dataclass(frozen=True)
class RouteLimits:
    """Thresholds of the routing.  Compiled programs use the defaults; tools/bench_conv.py passes other values (compile_model /
    engine.Net `limits`) to time one layer on several families."""
    patch_min_k: int = 500              # shortest K (taps x channels) worth a conv_patch_kernel launch
    # most couts sent to the patch kernel: with more than 64 couts the 256-pixel implicit-GEMM tiles (conv_gemm.hip, activation tile
    # fetched once for 128-256 couts) measure 15-50 % faster than the patch kernel on MI355X
    patch_max_cout: int = 64
    patch_min_tile_eff: float = 0.5     # smallest useful fraction of a tile grid (8/16 x 32 output pixels) for the patch kernel; below it the map is too ragged
    # conv_col_kernel (one filter column per step, 9x9 / 7x7 / 5x5 layers): below this tile efficiency the 8-row tiles of
    # conv_patch_kernel win (measured: 17x30 map 0.163 vs 0.203 ms, 34x60 0.50 vs 0.43)
    col_min_tile_eff: float = 0.75
    # conv_c3_kernel (3x3, two blocks per CU); cout / tile-efficiency limits from per-layer A/B runs
    col3_max_cout: int = 192            # per-layer A/B (tools/bench_conv.py --cfgs d,p,c): 224-cout layers tie or lose
    col3_min_k: int = 250               # 3x3 32->32 @136x240 (K = 288): 0.180 ms on the implicit GEMM, 0.115 ms here
    col3_wide_min_cin: int = 128        # layers with more than 64 couts (two+ cout tiles refetch the patch) only from 128 input channels on
    col3_min_tile_eff: float = 0.8
    pw_max_cout: int = 64               # conv_pw_kernel for 1x1 convs (and 2x2 s2 transposed convs) over <= 64 input channels


# ---- rules of the library, restated ------------------------------------------------------------------------------------------
def patch_fits(th, kh, kw, pixels):
    """The halo patch of a th x 32 output tile fits `pixels` (conv_patch_plan / conv_patch_th / launch_conv_patch: 352 for the LIGHT
    form's 8-row tiles, 640 for the plain 8-row tiles, 960 for the 16-row tiles)."""
    return (th + kh - 1) * (32 + kw - 1) <= pixels


def patch_th(kh, kw, oh):
    """conv_patch_th: 16-row tiles when their patch fits and the map tiles at most 12 % worse in rows than with 8-row tiles."""
    if not patch_fits(16, kh, kw, 960):
        return 8
    return 16 if rup(oh, 16) * 100 <= rup(oh, 8) * 112 else 8


def _axis_cost(n, unit, waves):
    """c3_axis_cost: full tiles along an axis of n pixels covered by `waves` x `unit`; a partial tile costs 0.35 + 0.65 x its live waves."""
    full, rem = divmod(n, unit * waves)
    return full + ((0.35 + 0.65 * -(-rem // unit) / waves) if rem else 0.0)


def c3_tile_eff(oh, ow):
    """conv_c3_plan: best tile efficiency over the 16x32 / 8x64 / 4x128 tile shapes when waves outside the map idle."""
    return max(oh * ow / (_axis_cost(oh, 2, rw) * _axis_cost(ow, 32, 8 // rw) * 512.0) for rw in (8, 4, 2))


def col_ok(kh, kw, sh, sw, cinp, coutp):
    """conv_col_ok, for a record without F_SRC2 / F_DOT1 (the route sets neither on a column layer)."""
    return (sh, sw) == (1, 1) and kh in (5, 7, 9) and 3 <= kw <= 17 and cinp % 16 == 0 and coutp <= 64


def c3_ok(kh, kw, sh, sw, ph, pw, cinp):
    """conv_c3_ok, for a record without F_SRC2 / F_DOT1."""
    return (kh, kw, sh, sw, ph, pw) == (3, 3, 1, 1, 1, 1) and cinp % 16 == 0


def gemm_ok(kh, kw, ph, pw, cinp, inshift):
    """conv_gemm_mode != 0, for a record without F_PATCH / F_DOT1 / F_SRC2: the layer runs on conv_gemm_kernel (or conv_smallm), the
    readers of 32-deep weight tiles.  The selector refuses an F_WK32 record it cannot send there, so a drift between the two rules
    fails loudly instead of computing garbage."""
    return not inshift and cinp % 32 == 0 and kh * kw <= 31 and kh >= 2 * ph + 1 and kw >= 2 * pw


def pw_ok(kh, kw, sh, sw, ph, pw, cinp, coutp, inshift, hilo, limits):
    """conv_pw_ok, with the compiler's own cout limit.  (hi + lo nets: the alternative is the generic kernel with K padded to 64 and
    walked twice — any cout count conv_pw_kernel can hold is faster there.)"""
    return ((kh, kw, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0) and not inshift and cinp % 8 == 0 and cinp <= (96 if hilo else 64)
            and coutp <= (128 if hilo else limits.pw_max_cout))


# ---- the compiler's own measures ---------------------------------------------------------------------------------------------
def grid_eff(oh, ow, th):
    """Live fraction of the th x 32 tile grid that covers an oh x ow map."""
    return oh * ow / float(rup(oh, th) * rup(ow, 32))


def col_tile_eff(oh, ow):
    """... of conv_col_kernel's 16 x 32 tiles, whose waves below the map idle (the cost model of conv_c3_plan)."""
    return oh * ow / float(_axis_cost(oh, 2, 8) * 16 * rup(ow, 32))


# ---- the route ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConvRoute:
    family: str                 # head | pw | c3 | c3_hlsum | col | patch_light | patch_std | stem | gemm_wk32 | generic
    flags: int                  # the flags the family implies (F_RES, F_IMGW, F_OGATE, F_U8SRC are the lowering's)
    ktot: int                   # P_KTOT
    ptaps: int = 0              # patch families: taps of the weight stream (whole kernel steps)
    th: int = 0                 # patch families: rows of a tile
    may_fuse_dot1: bool = False # the lowering may try to fuse the 1-channel projection behind the layer; if it does, it routes again with dot1_fused


def route_conv(kh, kw, sh, sw, ph, pw, cin, cinp, coutp, oh, ow, hilo, concat=False, inshift=0, offsets_fit=True, residual=False, dot1_next=False,
               limits=RouteLimits(), dot1_fused=False, head_input=False) -> ConvRoute:
    """The family of a dense conv layer.  cin: real input channels, cinp: as stored (View.span); ow: the width the selection sees
    (Compiler.sel_width: a nominal sample's in a ragged plan); concat: the input is a virtual concat of two views; inshift: upsample shift of
    an input read in place; offsets_fit: 32-bit in-image offsets reach the whole input image (launch_conv_c3 checks the same); dot1_next:
    the only reader is a 1x1 conv to ONE channel, which conv_patch_kernel could fuse.
    dot1_fused: that projection WAS fused (the first answer said may_fuse_dot1); head_input: the two parts of the concat are then a
    1-channel full-resolution map and a 64-channel map at half resolution (Compiler._head_input)."""
    unit = (sh, sw) == (1, 1)
    taps, k = kh * kw, kh * kw * cin
    ktot = rup(taps * cinp, ir.KT)
    hl = ir.F_HILO if hilo else 0
    # column kernels: not on a virtual concat, and never in front of a projection conv_patch_kernel could fuse
    if not concat and not dot1_next:
        if (c3_ok(kh, kw, sh, sw, ph, pw, cinp) and k >= min(limits.patch_min_k, limits.col3_min_k) and coutp <= limits.col3_max_cout
                and (coutp <= 64 or cinp >= limits.col3_wide_min_cin) and offsets_fit and c3_tile_eff(oh, ow) >= limits.col3_min_tile_eff):
            if hilo and coutp <= 32:
                # the 32-cout tile of conv_c3_kernel walks K twice for a hi + lo net with half its MFMA tile empty: ONE pass over a
                # 64-row stage [hi 32 | lo 32] instead, the two accumulator tiles added in the epilogue
                return ConvRoute("c3_hlsum", ir.F_COL | ir.F_HLSUM, taps * cinp)
            return ConvRoute("c3", ir.F_COL | hl, taps * cinp)
        if col_ok(kh, kw, sh, sw, cinp, coutp) and k >= limits.patch_min_k and col_tile_eff(oh, ow) >= limits.col_min_tile_eff:
            return ConvRoute("col", ir.F_COL | hl, taps * cinp)
    # k x k stride-1 convs on maps that tile well into 8/16 x 32 output patches: the LDS-resident-patch kernel, which has no two-pass
    # K walk for hi + lo weights (one block per CU: the fixed prologue / epilogue only amortises over a long enough K loop)
    if unit and taps >= 5 and k >= limits.patch_min_k and not hilo:
        th = patch_th(kh, kw, oh)
        std = patch_fits(8, kh, kw, 640) and grid_eff(oh, ow, th) >= limits.patch_min_tile_eff and coutp <= limits.patch_max_cout
        # LIGHT form (conv_patch_plan): 8-row tiles whose patch fits 352 pixels (3x3, 1xk), 64 or 128 couts per tile, two blocks per CU;
        # not combined with a virtual concat or the fused projection (that needs all couts of a pixel in one wave)
        light = patch_fits(8, kh, kw, 352) and grid_eff(oh, ow, 8) >= limits.patch_min_tile_eff and coutp <= 128 and not concat and not dot1_fused
        # (the fused projection: 16-row tiles, one cout tile, no residual — launch_conv_patch refuses the rest)
        fuse = dot1_next and std and th == 16 and coutp <= 64 and not residual
        assert fuse or not dot1_fused
        flags = ir.F_PATCH | (ir.F_SRC2 if concat else 0) | (ir.F_DOT1 if dot1_fused else 0)
        if dot1_fused and head_input and concat and (kh, kw, ph, pw) == (3, 3, 1, 1) and cinp == 72:
            # DB head of the PP-OCRv4 server detector: the 3x3 evaluated on the low-res grid with folded 2x2 taps (conv_head.hip)
            return ConvRoute("head", flags | ir.F_UP2HEAD, 2 * 4 * 4 * 32 + 32)
        if std or light:
            ptaps = rup(taps, 2 if light else 4)        # taps padded to whole kernel steps (2 in the LIGHT form, else 4), channels to 32
            return ConvRoute("patch_light" if light else "patch_std", flags, ptaps * rup(cinp, 32), ptaps, 8 if light else th, fuse and not dot1_fused)
    if concat:
        inshift = 0          # (a virtual concat is copied for the families below, upsampled parts with it)
    if pw_ok(kh, kw, sh, sw, ph, pw, cinp, coutp, inshift, hilo, limits):
        return ConvRoute("pw", ir.F_PW | hl, rup(cinp, 16))         # weight rows are whole 16-channel K slices
    if (kh, kw, ph, pw) == (3, 3, 1, 1) and (sh, sw) in ((1, 1), (2, 2)) and cinp == 8 and cin <= 4 and coutp <= 64 and not inshift:
        return ConvRoute("stem", ir.F_STEM | hl, ktot)              # an image-like input (conv_stem.hip)
    if gemm_ok(kh, kw, ph, pw, cinp, inshift):
        return ConvRoute("gemm_wk32", ir.F_WK32 | hl, ktot)         # 32-deep weight tiles (contiguous wave DMAs)
    return ConvRoute("generic", hl, ktot)
