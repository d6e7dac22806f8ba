"""One-record OP_CONV cases: every instantiation of every conv kernel family (the CONV_INST / GEMM_INST tables of csrc/conv_*.hip) at the
smallest shapes that reach it, derived from the rules of csrc/conv_select.hip, and the branches of conv_epilogue_tile (conv_common.h).
tests/test_gpu_conv_ops.py runs them on the GPU, tests/test_conv_records.py on the emulator; both through op_harness.run_case.

A case is a Spec (spec(...)): the record's geometry, flags and views.  case(spec) turns it into TWO runs of the same record:

  * the EXACT run.  Inputs, bias, residual, gate, affine on a dyadic grid ({-2 .. 2} / 2; the lo half of a pair tensor {-1, 0, 1} / 4: the
    kernels add the halves, whatever their size), weights sparse in {+-1, +-1/2} (hi + lo streams: {+-(1 + 2^-12), +-(1/2 + 2^-12)}, so the lo stream carries information), at most NNZ
    non-zero weights per cout at random (tap, channel) positions, so that a swapped tap, channel chunk, cout tile or pixel changes some
    output.  The condition — asserted from the generated tensors by every exact check (exact_cap) — is that the record evaluated on the ABSOLUTE values,
    in units of the product of the grids, stays below 2^24: then every partial sum in any order is exact in fp32 (fp16 x fp16 products
    are), and the stored value is the one rounding of an exact number.  The check is equality of bit patterns with float16(ref64) /
    float32(ref64).  Activations none / relu only.
  * the REAL run.  Seeded normal inputs, weights scaled 1 / sqrt(K), the nonlinear activations; held to op_harness.ratio with e32 from
    op_harness.conv_reference (the larger of the library and the strictly sequential float32 evaluation of ref_conv).

Both runs check that the bytes of the output buffers outside the output view are the pre-fill (NaN), and the zeros right of a ragged
sample's width by bit pattern.  build(spec, mode, mutate=...) hands a MUTATED matrix / record to the packer and the kernel and the
unmutated one to the reference (tests/test_conv_records.py: the checks must fail)."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import op_harness as H
from vse_amd import ir

NNZ = 24                        # non-zero weights per cout in the exact run
F16_NAN = 0x7E00
ACTS_REAL = (ir.ACT_HSWISH, ir.ACT_SWISH, ir.ACT_SIGMOID, ir.ACT_HSIGMOID)
MUTATIONS = ("taps", "chunk", "cout", "res", "bias", "width")


def rup(x, m):
    return (x + m - 1) // m * m


@dataclass(frozen=True)
class Spec:
    name: str
    expect: Optional[str]               # the instantiation the case was written for; None: the record must be refused
    fam: str                            # conv_pack family
    n: int
    h: int                              # stored input map (in0), before inshift
    w: int
    cin: int                            # stored channels of in0 (P_CINP = cin + the second source's)
    np_: int                            # P_COUT
    k: Tuple[int, int] = (1, 1)
    s: Tuple[int, int] = (1, 1)
    pad: Optional[Tuple[int, int]] = None          # default: 'same' (k // 2)
    hilo: bool = False
    flags: int = 0                      # flags beyond the family's, F_HILO, and those the fields below imply
    act: int = ir.ACT_RELU              # activation of the REAL run is `real_act`; the exact run uses this one (none / relu)
    real_act: int = ir.ACT_HSWISH
    act2: int = ir.ACT_NONE
    post: bool = False                  # a scalar affine behind the activation
    inshift: int = 0
    src2: Optional[Tuple[int, int]] = None         # (channels, shift) of the second source of a virtual concat (F_SRC2)
    res: Optional[dict] = None          # dict(shift=0, lo=False, ld_extra=0, off=0): residual (F_RES)
    gate: bool = False                  # F_OGATE
    pixshuf: bool = False
    out_f32: bool = False
    onech: bool = False
    lo_out: bool = False
    out_ld_extra: int = 8               # the output view is a channel slice of a buffer this much wider
    out_off: int = 0                    # ... starting this many ELEMENTS into it
    widths: Optional[Tuple[int, ...]] = None       # ragged: per-sample output widths
    dot: Optional[dict] = None          # dict(f32=True, ld=1): F_DOT1
    tail2: bool = False                 # F_TAIL2
    dwpre: Optional[dict] = None        # dict(lo_in=True): F_DWPRE (k / s / pad = the depthwise conv's)
    imgw: bool = False                  # F_IMGW
    in_ld_extra: int = 0                # the input view is a channel slice of a buffer this much wider
    ptaps: int = 0                      # patch: taps of the stream
    ktot: Optional[int] = None          # override of P_KTOT (refusals; F_IMGW with 32-deep K)
    real_ch: Optional[int] = None       # stem: real input channels (the others carry zeros and zero weights)
    u_ld: int = 8                       # head: pixel stride of the 1-channel source
    nnz: int = NNZ                      # non-zero weights per cout of the exact run
    rc: Optional[int] = None            # refused: the code the library must answer

    @property
    def padv(self):
        return self.pad if self.pad is not None else (self.k[0] // 2, self.k[1] // 2)


def spec(name, expect, fam, n, h, w, cin, np_, **kw):
    return Spec(name, expect, fam, n, h, w, cin, np_, **kw)


# ---------------------------------------------------------------------------------------------------------------- tensors
def _grid(rng, shape, lo=-4, hi=4, unit=0.5):
    return rng.integers(lo, hi + 1, shape).astype(np.float64) * unit


def _gen_x(rng, shape, mode, pair=False):
    """-> (hi fp16, lo fp16 or None, float64 value)"""
    if mode == "exact":
        hi = _grid(rng, shape).astype(np.float16)
        lo = (rng.integers(-1, 2, shape) / 4.0).astype(np.float16) if pair else None
    else:
        v = rng.normal(0, 1, shape)
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float64)).astype(np.float16) if pair else None
    return hi, lo, hi.astype(np.float64) + (lo.astype(np.float64) if pair else 0.0)


def _gen_w(rng, npad, K, mode, hilo, live=None, grid_bits=None, nnz=NNZ):
    """The float64 matrix handed to conv_pack.  live: boolean mask [K] of the positions that may carry a weight."""
    live = np.ones(K, bool) if live is None else live
    pos = np.flatnonzero(live)
    w = np.zeros((npad, K), np.float64)
    if mode == "exact":
        for co in range(npad):
            sel = rng.choice(pos, size=min(nnz, len(pos)), replace=False)
            w[co, sel] = rng.choice([1.0, -1.0, 0.5, -0.5], size=len(sel)) + (2.0 ** -12 if hilo else 0.0) * rng.choice([1.0, -1.0], size=len(sel))
    else:
        w[:, pos] = rng.normal(0, 1, (npad, len(pos))) / np.sqrt(len(pos))
        if grid_bits is not None:
            w = np.round(w * 2.0 ** grid_bits) / 2.0 ** grid_bits
    return w


def _buffer(shape_pix, c, ld, off, dtype, fill_nan=True):
    """A flat buffer holding a [pixels][ld] tensor `off` elements in, 8 elements of slack behind; -> (flat array, view of the [.., c] slice)."""
    npix = int(np.prod(shape_pix))
    flat = np.zeros(off + npix * ld + 8, dtype)
    if fill_nan:
        if dtype == np.float16:
            flat.view(np.uint16)[:] = F16_NAN
        else:
            flat[:] = np.nan
    return flat


def _slice(flat, shape_pix, c, ld, off, coff=0):
    npix = int(np.prod(shape_pix))
    return flat[off:off + npix * ld].reshape(tuple(shape_pix) + (ld,))[..., coff:coff + c]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same_bits(got, ref64, what):
    want = ref64.astype(got.dtype)
    ok = _bits(got) == _bits(want)
    assert ok.all(), (what, "not bit-identical at", tuple(int(v) for v in np.argwhere(~ok)[0]), "of", got.shape, "got",
                      float(got[tuple(np.argwhere(~ok)[0])]), "want", float(want[tuple(np.argwhere(~ok)[0])]), int((~ok).sum()), "differ")


# ---------------------------------------------------------------------------------------------------------------- one run
@dataclass
class Built:
    run: H.Run
    rec: np.ndarray
    check: object                       # check(arenas) -> worst error / bound (exact run: 0.0)
    exact_cap: object = None            # exact run: asserts the condition of the exact run, -> the bound in grid units


def build(sp: Spec, mode: str, mutate: Optional[str] = None) -> Built:
    """mode: "exact" | "real".  mutate (see MUTATIONS): the kernel's side is mutated, the reference's is not."""
    exact = mode == "exact"
    rng = np.random.default_rng(sum(map(ord, sp.name)) * 7 + (1 if exact else 2))
    (kh, kw), (sh, sw), (ph, pw) = sp.k, sp.s, sp.padv
    n, Np = sp.n, sp.np_
    H_, W_ = sp.h << sp.inshift, sp.w << sp.inshift
    oh, ow = (H_ + 2 * ph - kh) // sh + 1, (W_ + 2 * pw - kw) // sw + 1
    cinp = sp.cin + (sp.src2[0] if sp.src2 else 0)
    head = sp.fam == "head"
    flags = sp.flags | H.CONV_FAMILY_FLAGS[sp.fam] | (ir.F_HILO if sp.hilo and sp.fam != "hlsum" else 0)
    act = (sp.act if exact else sp.real_act)
    act_a, act_b = (0.25, 0.5) if act == ir.ACT_HSIGMOID else (0.0, 0.0)
    post_a, post_b = ((0.5, 1.0) if exact else (0.75, -0.125)) if sp.post else (1.0, 0.0)
    units = 0.5 * 0.5                                        # x, w   (the bias shares the product's grid)
    if sp.hilo:
        units *= 2.0 ** -12
    pixshuf = sp.pixshuf or sp.tail2
    if sp.post:
        units *= 0.5
    blob, tensors = H.Blob(), []
    pair_in = bool(sp.dwpre and sp.dwpre.get("lo_in"))
    if pair_in:
        units *= 0.5

    # ---- inputs
    in_ld = (2 * sp.cin if pair_in else sp.cin) + sp.in_ld_extra
    xhi, xlo, x64 = _gen_x(rng, (n, sp.h, sp.w, sp.cin), mode, pair_in)
    if sp.real_ch is not None:
        xhi[..., sp.real_ch:] = 0
        x64[..., sp.real_ch:] = 0
    if head:
        # the 1-channel full-resolution source: [n, H, W] at pixel stride u_ld, nominal span 8
        xb = _buffer((n, sp.h, sp.w), 1, sp.u_ld, 0, np.float16, fill_nan=False)
        _slice(xb, (n, sp.h, sp.w), 1, sp.u_ld, 0)[...] = xhi[..., :1]
        x64 = np.concatenate([x64[..., :1], np.zeros(x64.shape[:3] + (7,))], axis=3)
        in0 = H.view(H.ext(0), n, sp.h, sp.w, 8, ld=sp.u_ld)
    else:
        xb = _buffer((n, sp.h, sp.w), sp.cin, in_ld, 0, np.float16, fill_nan=False)
        _slice(xb, (n, sp.h, sp.w), sp.cin, in_ld, 0)[...] = xhi
        if pair_in:
            _slice(xb, (n, sp.h, sp.w), sp.cin, in_ld, 0, coff=sp.cin)[...] = xlo
        in0 = H.view(H.ext(0), n, sp.h, sp.w, sp.cin, ld=in_ld)
    tensors.append(xb)

    # ---- output
    oc = Np // 4 if pixshuf else Np
    mul = 2 if pixshuf else 1
    oshape = (n, oh * mul, ow * mul)
    odt = np.float32 if sp.out_f32 else np.float16
    if sp.onech:
        oc_view, out_ld = 1, 1
    else:
        oc_view, out_ld = oc, (2 * oc if sp.lo_out else oc) + sp.out_ld_extra
    ob = _buffer(oshape, oc_view, out_ld, sp.out_off, odt)
    out = H.view(H.ext(1), *oshape, oc_view, ld=out_ld, esize=ob.itemsize, off=sp.out_off * ob.itemsize)
    tensors.append(ob)

    # ---- residual
    res_v, res64, lo_res = None, None, 0
    if sp.res is not None:
        rs = sp.res.get("shift", 0)
        rh, rw_ = (oshape[1] + (1 << rs) - 1) >> rs, (oshape[2] + (1 << rs) - 1) >> rs
        rpair = bool(sp.res.get("lo"))
        r_ld = (2 * oc if rpair else oc) + sp.res.get("ld_extra", 0)
        r_off = sp.res.get("off", 0)
        rhi, rlo, res64 = _gen_x(rng, (n, rh, rw_, oc), mode, rpair)
        if rpair:
            units *= 0.5
        rk = np.roll(rhi, 1, axis=2) if mutate == "res" else rhi
        rb = _buffer((n, rh, rw_), oc, r_ld, r_off, np.float16, fill_nan=False)
        _slice(rb, (n, rh, rw_), oc, r_ld, r_off)[...] = rk
        if rpair:
            _slice(rb, (n, rh, rw_), oc, r_ld, r_off, coff=oc)[...] = rlo
            lo_res = oc
        res_v = H.view(H.ext(2), n, rh, rw_, oc, ld=r_ld, off=r_off * 2)
        flags |= ir.F_RES
        tensors.append(rb)
    else:
        tensors.append(np.zeros(8, np.float16))

    # ---- weights (and what rides in in2)
    K = kh * kw * cinp
    live = None
    if sp.fam == "stem":
        live = np.tile(np.arange(8) < (sp.real_ch or 4), 9)
    if head:
        live = np.tile(np.r_[True, np.zeros(7, bool), np.ones(64, bool)], 9)
    if sp.dwpre:
        K = cinp
    wk = _gen_w(rng, Np, K, mode, sp.hilo, live, grid_bits=10 if head else None, nnz=sp.nnz)
    w_seen = H.conv_seen_weights(wk, sp.hilo)
    if head:                                                  # (the packer sums the taps that fold onto one low-res pixel in fp64, then rounds once)
        w_seen = wk
    w_kernel = wk
    if mutate == "taps":
        if kh * kw < 2 or sp.dwpre:
            raise ValueError("taps: the conv has one tap")
        w_kernel = wk.copy().reshape(Np, kh * kw, cinp)
        w_kernel[:, [0, 1]] = w_kernel[:, [1, 0]]
        w_kernel = w_kernel.reshape(Np, K)
    elif mutate == "chunk":
        w_kernel = wk.copy().reshape(Np, -1, cinp)
        w_kernel[:, :, (cinp - 1) // 16 * 16:] = 0
        w_kernel = w_kernel.reshape(Np, K)
    elif mutate == "cout":
        if Np <= 32:
            raise ValueError("cout: no rows on both sides of a 32-boundary")
        w_kernel = wk.copy()
        w_kernel[[31, 32]] = w_kernel[[32, 31]]
    pk = (1, 1) if sp.dwpre else (kh, kw)
    stream, ktot = H.conv_pack(sp.fam, w_kernel, pk[0], pk[1], cinp, hilo=sp.hilo, ptaps=sp.ptaps)
    in2_v, x2_64, gate64, wimg64 = None, None, None, None
    in2shift = 0
    if sp.imgw:
        wi = np.stack([_gen_w(rng, Np, K, mode, False) for _ in range(n)])
        if mutate == "chunk":
            wik = wi.copy()
            wik[:, :, (cinp - 1) // 16 * 16:] = 0
        elif mutate == "cout":
            wik = wi.copy()
            wik[:, [31, 32]] = wik[:, [32, 31]]
        else:
            wik = wi
        packs = [H.conv_pack(sp.fam, wik[b], kh, kw, cinp) for b in range(n)]
        ktot = packs[0][1]
        kp_rec = sp.ktot or ktot
        tensors.append(np.stack([p_[0][:kp_rec * Np] for p_ in packs]).astype(np.float16))
        in2_v = H.view(H.ext(3), n, 1, 1, kp_rec * Np)
        wimg64 = wi.astype(np.float16).astype(np.float64)
        flags |= ir.F_IMGW
    elif sp.src2:
        c2, in2shift = sp.src2
        h2, w2 = H_ >> in2shift, W_ >> in2shift
        x2hi, _, x2_64 = _gen_x(rng, (n, h2, w2, c2), mode)
        tensors.append(x2hi)
        in2_v = H.view(H.ext(3), n, h2, w2, c2)
        flags |= ir.F_SRC2
    elif sp.gate:
        g_ld = rup(Np, 8) + 8
        g = (_grid(rng, (n, Np), -1, 2) if exact else rng.normal(0, 0.5, (n, Np))).astype(np.float16)
        units *= 0.5
        gb = np.zeros((n, g_ld), np.float16)
        gb[:, :Np] = g
        gate64 = g.astype(np.float64)
        tensors.append(gb)
        in2_v = H.view(H.ext(3), n, 1, 1, Np, ld=g_ld)
        flags |= ir.F_OGATE
    else:
        tensors.append(np.zeros(8, np.float16))
    w_off = blob.add(stream)
    bias = (_grid(rng, Np) if exact else rng.normal(0, 0.5, Np)).astype(np.float32)
    b_off = blob.add(np.roll(bias, 1) if mutate == "bias" else bias)

    # ---- the 1-channel map behind it / the depthwise conv in front
    out2_v, aux_off, dotact, pre_b, dot_ref, tail_ref, dw_ref = None, 0, ir.ACT_NONE, 0.0, None, None, None
    lo_in = 0
    if sp.dot is not None:
        dw = (_grid(rng, Np, -2, 2) if exact else rng.normal(0, 1, Np) / np.sqrt(Np)).astype(np.float32)
        units *= 0.5
        pre_b = 0.5 if exact else 0.3
        dotact = ir.ACT_NONE if exact else ir.ACT_SIGMOID
        aux_off = blob.add(dw)
        f32, d_ld = sp.dot.get("f32", True), sp.dot.get("ld", 1)
        o2 = _buffer(oshape, 1, d_ld, 0, np.float32 if f32 else np.float16)
        out2_v = H.view(H.ext(4), *oshape, 1, ld=d_ld, esize=o2.itemsize)
        tensors.append(o2)
        dot_ref = (dw, pre_b, dotact)
        flags |= ir.F_DOT1
    elif sp.tail2:
        cp = Np // 4
        w2 = (_grid(rng, (cp, 2, 2), -2, 2) if exact else rng.normal(0, 1, (cp, 2, 2)) / np.sqrt(cp)).astype(np.float16).astype(np.float64)
        units *= 0.5
        pre_b = 0.5 if exact else 0.3
        dotact = ir.ACT_RELU if exact else ir.ACT_SIGMOID
        from vse_amd import compiler
        aux_off = blob.add(compiler.Compiler.tail2_fragments(w2, cp))
        o2 = _buffer((n, 4 * oh, 4 * ow), 1, 1, 0, np.float16)
        out2_v = H.view(H.ext(4), n, 4 * oh, 4 * ow, 8, ld=1)
        tensors.append(o2)
        tail_ref = (w2, pre_b, dotact)
        flags |= ir.F_TAIL2
    elif sp.dwpre:
        from vse_amd import compiler
        wd = (_grid(rng, (cinp, kh * kw), -2, 2) if exact else rng.normal(0, 1, (cinp, kh * kw)) / 3.0).astype(np.float32)
        dshift = (_grid(rng, cinp) if exact else rng.normal(0, 0.5, cinp)).astype(np.float32)
        units *= 0.5
        dact = ir.ACT_RELU if exact else ir.ACT_HSWISH
        aux_off = blob.add(compiler.Compiler.dwpre_table(wd.astype(np.float64), dshift, rup(cinp, 16), kh, sh, ph, dact))
        dw_ref = (wd, dshift, dact, 0.0, 0.0, 1.0, 0.0)
        lo_in = sp.cin if pair_in else 0
        flags |= ir.F_DWPRE
        tensors.append(np.zeros(8, np.float16))
    else:
        tensors.append(np.zeros(8, np.float16))
    if pixshuf:
        flags |= ir.F_PIXSHUF
    if sp.out_f32:
        flags |= ir.F_OUT_F32
    if sp.onech:
        flags |= ir.F_ONECH

    if (mutate == "res" and sp.res is None) or (mutate == "width" and sp.widths is None) or mutate not in (None,) + MUTATIONS:
        raise ValueError(f"{mutate}: does not apply to {sp.name}")
    widths = None if sp.widths is None else np.asarray(sp.widths, np.int64)
    wk_widths = widths
    if mutate == "width":
        wk_widths = widths.copy()
        wk_widths[0] -= 1
    rec = H.conv_op(in0, out, sp.k, sp.s, sp.padv, Np, sp.ktot or ktot, cinp, w_off, b_off, flags=flags, act=act, act2=sp.act2, act_a=act_a,
                    act_b=act_b, post_a=post_a, post_b=post_b, inshift=sp.inshift, res=res_v, resshift=sp.res.get("shift", 0) if sp.res else 0,
                    in2=in2_v, in2shift=in2shift, out2=out2_v, aux_off=aux_off, dotact=dotact, pre_b=pre_b, lo_out=oc if sp.lo_out else 0,
                    lo_res=lo_res, lo_in=lo_in, wl=(0, 1) if widths is not None else (0, 0))
    run = H.Run(rec, blob.array(), tensors, None if widths is None else wk_widths[None].astype(np.int32))

    # ---- the reference
    ref_w = w_seen

    def ref(dt, seq, absolute=False):
        a = np.abs if absolute else (lambda v: v)
        kw_ = dict(dt=dt, seq=seq, x2=None if x2_64 is None else a(x2_64), inshift=sp.inshift, in2shift=in2shift,
                   act=ir.ACT_NONE if absolute else act, act_a=act_a, act_b=act_b, post_a=abs(post_a) if absolute else post_a,
                   post_b=abs(post_b) if absolute else post_b, gate=None if gate64 is None else a(gate64), pixshuf=pixshuf,
                   res=None if res64 is None else a(res64), resshift=sp.res.get("shift", 0) if sp.res else 0,
                   act2=ir.ACT_NONE if absolute else sp.act2, wl_out=widths,
                   dot=None if dot_ref is None else (a(dot_ref[0]), abs(dot_ref[1]), ir.ACT_NONE if absolute else dot_ref[2]),
                   tail2=None if tail_ref is None else (a(tail_ref[0]), abs(tail_ref[1]), ir.ACT_NONE if absolute else tail_ref[2]),
                   dwpre=None if dw_ref is None else (a(dw_ref[0]), a(dw_ref[1]), ir.ACT_NONE if absolute else dw_ref[2]) + dw_ref[3:],
                   wimg=None if wimg64 is None else a(wimg64))
        r = H.ref_conv(a(x64), a(ref_w), a(bias), sp.k, sp.s, sp.padv, **kw_)
        if sp.onech:
            r = r[..., :1]
        return r

    memo = {}

    def references():
        """(float64 results, e32 per result; None in the exact run), computed once, when the first check asks."""
        if not memo:
            if exact:
                r = ref(np.float64, False)
                memo["r"] = (r if isinstance(r, tuple) else (r,)), None
            else:
                memo["r"] = H.conv_reference(ref)
        return memo["r"]

    def exact_cap():
        """The condition of the exact run: the record on the absolute values, in units of the product of the grids, stays below 2^24."""
        bound = ref(np.float64, False, absolute=True)
        cap = max(float(np.max(b)) for b in (bound if isinstance(bound, tuple) else (bound,))) / units
        assert cap < 2.0 ** 24, (sp.name, "the exact run's inputs do not meet the condition: sum |x w| in grid units", cap)
        return cap

    def untouched(flat, shape_pix, c, ld, off, what, lo=0):
        keep = np.ones(flat.shape, bool)
        _slice(keep, shape_pix, c, ld, off)[...] = False
        if lo:
            _slice(keep, shape_pix, c, ld, off, coff=lo)[...] = False
        pre = F16_NAN if flat.dtype == np.float16 else 0x7FC00000
        assert (_bits(flat)[keep] == pre).all(), (sp.name, mode, what, "bytes outside the output view were written")

    def hold(got, want64, e, what, pair=False):
        if exact:
            _same_bits(got, want64, (sp.name, "exact", what))
            return 0.0
        return H.ratio(got, want64, e, (sp.name, "real", what), pair=pair)

    def check(arenas):
        worst = 0.0
        r64, e32 = references()
        if exact:
            exact_cap()
        if sp.dot is not None:
            f32, d_ld = sp.dot.get("f32", True), sp.dot.get("ld", 1)
            o2 = arenas[4].reshape(-1)
            worst = hold(_slice(o2, oshape, 1, d_ld, 0), r64[0], None if exact else e32[0], "out2")
            untouched(o2, oshape, 1, d_ld, 0, "out2")
            assert (_bits(arenas[1].reshape(-1)) == F16_NAN).all(), (sp.name, "F_DOT1 must not store the wide tensor")
            return worst
        flat = arenas[1].reshape(-1)
        got = _slice(flat, oshape, oc_view, out_ld, sp.out_off)
        y64 = r64[0]
        if sp.lo_out:
            lo = _slice(flat, oshape, oc, out_ld, sp.out_off, coff=oc)
            if exact:
                hi64 = y64.astype(np.float16).astype(np.float64)
                _same_bits(got, y64, (sp.name, "exact", "hi half"))
                _same_bits(lo, y64 - hi64, (sp.name, "exact", "lo half"))
            else:
                worst = H.ratio(got.astype(np.float64) + lo.astype(np.float64), y64, e32[0], (sp.name, "real", "hi + lo"), pair=True)
        else:
            worst = hold(got, y64, None if exact else e32[0], "out")
        untouched(flat, oshape, oc_view, out_ld, sp.out_off, "out", lo=oc if sp.lo_out else 0)
        if widths is not None:
            for b, wn in enumerate(widths):
                assert not _bits(np.ascontiguousarray(got[b, :, int(wn):])).any(), (sp.name, mode, "right of sample", b, "not +0 bit patterns")
        if sp.tail2:
            o2 = arenas[4].reshape(-1)
            z = _slice(o2, (n, 4 * oh, 4 * ow), 1, 1, 0)
            # stage B reads the fp16 values stage A stored: held to the reference of stage B on THOSE values
            if exact:
                _same_bits(z, r64[1], (sp.name, "exact", "out2"))
            else:
                z64, ez = H.reference(lambda dt: H.ref_tail2(np.ascontiguousarray(got), *tail_ref, dt=dt))
                worst = max(worst, H.ratio(z, z64[0], ez[0], (sp.name, "real", "out2")))
            assert (_bits(o2[n * 16 * oh * ow:]) == F16_NAN).all(), (sp.name, "out2: bytes behind the map were written")
        return worst

    return Built(run, rec, check, exact_cap if exact else None)


def case(sp: Spec, mutate=None, modes=("exact", "real")):
    """The op_harness.Case of a spec: asserts the instantiation the record names, then both runs."""
    built = [build(sp, m, mutate) for m in modes]
    if sp.expect is None:
        return H.Case(sp.name, [built[0].run], refused=True, note={"want_rc": sp.rc})

    def check(outs):
        return max(b.check(o) for b, o in zip(built, outs))
    c = H.Case(sp.name, [b.run for b in built], check, note={"expect": sp.expect})
    return c


def selected(sp: Spec):
    """The instantiation the record of a spec names (vse_op_kernel_name)."""
    return H.conv_name(build(sp, "exact").rec)


# ---------------------------------------------------------------------------------------------------------------- the groups
# Shapes follow the rules of csrc/conv_select.hip (the thresholds named in the comments), not the models.  `expect` is asserted against the
# library's own answer (op_harness.conv_name) by both test files.
A = ir
_G = "conv_gemm_kernel<%s>"
_CFG = {0: "128, 128, 2, 2, 32, 3", 1: "256, 64, 4, 1, 32, 3", 2: "256, 32, 4, 1, 32, 3", 3: "256, 128, 4, 2, 32, 3", 4: "256, 256, 4, 4, 32, 3",
        5: "256, 192, 8, 2, 32, 3", 6: "256, 256, 4, 4, 64, 2", 7: "256, 192, 8, 2, 64, 2"}


def gemm(cfg, mask):
    return _G % f"{_CFG[cfg]}, {mask}"


def _gemm():
    """conv_gemm_config: Np <= 32 -> 2, <= 64 -> 1, <= 128 -> 0 (3 from 65 281 pixels), 129 .. 192 from 48 897 pixels -> 5 (7 at cinp % 64
    == 0), 193 .. 256 -> 4 (6).  Unmasked = a 1x1 filter without padding whose K is the stored channels (Kp == cinp); a small 1x1 problem
    goes to conv_smallm first (conv_smallk_ok: <= 256 channels at stride 1), so the small unmasked cases have 320 channels or stride 2.
    The selector refuses Kp % 64 != 0 — but only behind the F_IMGW branch, which asks for the unmasked mode alone: per-image weights with
    Kp = cinp = 96 reach the unmasked forms of the 32-deep configurations 4 and 5 (no compiled program does: P_KTOT is a multiple of 64)."""
    return [
        # image seam inside a 256-pixel tile (2 x 99 pixels), M tail, N tail (24 of 32)
        spec("gemm2 masked 3x3 seam", gemm(2, 1), "tile32", 2, 9, 11, 32, 24, k=(3, 3)),
        spec("gemm2 masked 3x3 hilo", gemm(2, 1), "tile32", 2, 9, 11, 32, 32, k=(3, 3), hilo=True, real_act=A.ACT_SWISH),
        spec("gemm2 unmasked 320ch", gemm(2, 0), "tile32", 1, 15, 20, 320, 32, real_act=A.ACT_SIGMOID),
        spec("gemm2 unmasked s2 kt64", gemm(2, 0), "tile64", 2, 9, 11, 64, 24, s=(2, 2), pad=(0, 0)),
        spec("gemm1 masked 2x2 s2", gemm(1, 1), "tile32", 2, 10, 14, 32, 64, k=(2, 2), s=(2, 2), pad=(0, 0)),
        spec("gemm1 unmasked", gemm(1, 0), "tile32", 1, 15, 20, 320, 48, real_act=A.ACT_HSIGMOID),
        spec("gemm1 unmasked imgw", gemm(1, 0), "tile32", 3, 8, 8, 64, 40, imgw=True),          # an image ends inside every 256-pixel tile
        spec("gemm0 masked 3x3 s2", gemm(0, 1), "tile32", 2, 19, 23, 32, 72, k=(3, 3), s=(2, 2)),
        spec("gemm0 masked 1x5 kt64", gemm(0, 1), "tile64", 1, 9, 40, 32, 128, k=(1, 5)),
        spec("gemm0 unmasked hilo", gemm(0, 0), "tile32", 1, 15, 20, 320, 104, hilo=True),
        spec("gemm0 unmasked imgw 2 tiles", gemm(0, 0), "tile32", 2, 12, 16, 64, 72, imgw=True),    # 192 pixels per image: 128 + 64
    ]


# The big-M configurations: one image of 256 x 256 (65 536 >= 65 281 pixels) or 192 x 256 (49 152 >= 48 897), 32 .. 96 channels, a 1x1 filter
# (masked through a zero-padded K tile: cinp 32 or 96 in Kp 64 or 128) or a 1x2 filter (masked at cinp % 64 == 0).
def _gemm_m65k():
    return [spec("gemm3 masked", gemm(3, 1), "tile32", 1, 256, 256, 32, 72),
            spec("gemm3 unmasked", gemm(3, 0), "tile32", 1, 256, 256, 64, 128, real_act=A.ACT_SWISH)]


def _gemm_n192():
    return [spec("gemm5 masked", gemm(5, 1), "tile32", 1, 192, 256, 32, 136),
            spec("gemm5 unmasked imgw K96", gemm(5, 0), "tile32", 1, 192, 256, 96, 192, imgw=True, ktot=96),
            spec("gemm7 masked 1x2", gemm(7, 1), "tile32", 1, 192, 256, 64, 136, k=(1, 2), pad=(0, 0), real_act=A.ACT_SIGMOID),
            spec("gemm7 unmasked", gemm(7, 0), "tile32", 1, 192, 256, 64, 192, res=dict(), act2=A.ACT_RELU)]


def _gemm_n256():
    return [spec("gemm4 masked K96", gemm(4, 1), "tile32", 1, 192, 256, 96, 200),
            spec("gemm4 unmasked imgw K96", gemm(4, 0), "tile32", 1, 192, 256, 96, 256, imgw=True, ktot=96),
            spec("gemm6 masked 1x2", gemm(6, 1), "tile32", 1, 192, 256, 64, 256, k=(1, 2), pad=(0, 0)),
            spec("gemm6 unmasked", gemm(6, 0), "tile32", 1, 192, 256, 64, 200, real_act=A.ACT_HSIGMOID)]


def _smallm():
    """conv_smallk_ok (a 1x1 over <= 256 channels and <= 4096 32 x 32 wave tiles) and conv_smallm_ok (M <= 256, any channel count)."""
    sm, hl = "conv_smallm_kernel<%d>", "conv_smallm_hl_kernel<%d>"
    return [
        # cinp 120: the last 16-channel slice is half masked; 40 couts: a tail of 8; 35 pixels: a pixel tail
        spec("smallk 120ch kt32", sm % 32, "tile32", 1, 5, 7, 120, 40),
        spec("smallk 72ch kt64", sm % 64, "tile64", 1, 5, 7, 72, 40, real_act=A.ACT_SWISH),
        spec("smallk 120ch hilo kt32", hl % 32, "tile32", 1, 5, 7, 120, 40, hilo=True),
        spec("smallk 72ch hilo kt64", hl % 64, "tile64", 1, 5, 7, 72, 72, hilo=True, res=dict(), act2=A.ACT_RELU),
        spec("smallm SE gate 320ch", sm % 32, "tile32", 3, 1, 1, 320, 80, real_act=A.ACT_HSIGMOID),
        spec("smallm SE gate 320ch hilo", hl % 32, "tile32", 3, 1, 1, 320, 80, hilo=True, real_act=A.ACT_HSIGMOID),
        # (M + 31) / 32 * (Np + 31) / 32 = 512 * 8 = 4096: the last small problem; one pixel tile more selects another family
        spec("smallk 4096 wave tiles", sm % 64, "tile64", 1, 128, 128, 8, 256),
        spec("smallk 4104 wave tiles", "conv_mfma_kernel<128, 128, 2, 2, false>", "tile64", 1, 129, 128, 8, 256),
    ]


def _mfma():
    """conv_tile_bn: Np <= 32 -> 32; 72 -> 128 (padded 128 both ways: the wider tile); 192 -> 64.  24 channels keep the layer off
    conv_gemm_kernel (cinp % 32), as does inshift."""
    m = "conv_mfma_kernel<%s, %s>"
    t = {32: "256, 32, 4, 1", 128: "128, 128, 2, 2", 64: "256, 64, 4, 1"}
    out = []
    for np_, bn in ((32, 32), (72, 128), (192, 64)):
        out.append(spec(f"mfma Np{np_}", m % (t[bn], "false"), "tile64", 2, 9, 15, 24, np_, k=(3, 3), in_ld_extra=8))
        out.append(spec(f"mfma Np{np_} up", m % (t[bn], "true"), "tile64", 2, 5, 8, 24, np_, k=(3, 3), inshift=1, res=dict()))
    out.append(spec("mfma 5x5 s(1,2) K tail", m % (t[32], "false"), "tile64", 1, 9, 21, 24, 24, k=(5, 5), s=(1, 2), real_act=A.ACT_SWISH))
    out.append(spec("mfma 32ch up hilo", m % (t[128], "true"), "tile64", 1, 5, 8, 32, 72, k=(3, 3), inshift=1, hilo=True))
    return out


def _patch():
    """conv_patch_plan: LIGHT (mode 2, 8-row tiles) when the patch of an 8 x 32 tile fits 352 pixels and neither F_DOT1 nor F_SRC2 is set; else
    64 couts, 16-row tiles where their patch fits 960 pixels and the rows tile well (mode 1 above 640 pixels, and then 32 couts for Np <= 32).
    A 5x5 filter's 16-row patch has 720 pixels: it runs on <16, 64, 1>; <16, 64, 0> serves the 3x3 with a second source or a fused
    projection (612 pixels)."""
    pk = "conv_patch_kernel<%d, %d, %d>"
    return [
        spec("patch 3x3 light", pk % (8, 64, 2), "patch", 2, 9, 40, 32, 64, k=(3, 3), ptaps=10),
        spec("patch 3x3 light 128", pk % (8, 128, 2), "patch", 1, 9, 40, 24, 72, k=(3, 3), ptaps=10, res=dict(), act2=A.ACT_RELU),
        spec("patch 1x7 light", pk % (8, 64, 2), "patch", 1, 9, 40, 32, 40, k=(1, 7), ptaps=8),
        spec("patch 1x7 light 128", pk % (8, 128, 2), "patch", 1, 9, 40, 32, 128, k=(1, 7), ptaps=8, real_act=A.ACT_SWISH),
        spec("patch 9x9 OH16", pk % (16, 64, 1), "patch", 1, 16, 40, 32, 64, k=(9, 9), ptaps=84),
        spec("patch 9x9 OH40", pk % (8, 64, 0), "patch", 1, 40, 33, 32, 40, k=(9, 9), ptaps=84),
        spec("patch 5x5", pk % (16, 64, 1), "patch", 2, 16, 33, 24, 64, k=(5, 5), ptaps=28),
        spec("patch 9x9 Np24", pk % (16, 32, 1), "patch", 1, 16, 33, 32, 24, k=(9, 9), ptaps=84),
        spec("patch 7x7 49 taps", pk % (16, 64, 1), "patch", 1, 16, 33, 32, 64, k=(7, 7), ptaps=52),      # 13 steps of 4: the last holds one tap
        spec("patch 3x3 src2 shift0", pk % (16, 64, 0), "patch", 1, 16, 40, 32, 64, k=(3, 3), ptaps=12, src2=(32, 0)),
        spec("patch 3x3 src2 shift1", pk % (16, 64, 0), "patch", 2, 16, 40, 24, 40, k=(3, 3), ptaps=12, src2=(40, 1)),
        spec("patch 5x5 src2 shift1", pk % (16, 64, 1), "patch", 1, 16, 40, 32, 64, k=(5, 5), ptaps=28, src2=(32, 1)),
        spec("patch 3x3 dot1 f32", pk % (16, 64, 0), "patch", 2, 16, 40, 32, 64, k=(3, 3), ptaps=12, dot=dict(f32=True, ld=1)),
        spec("patch 9x9 dot1 f16 ld8", pk % (16, 64, 1), "patch", 1, 32, 33, 32, 40, k=(9, 9), ptaps=84, dot=dict(f32=False, ld=8)),
    ]


def _col():
    """conv_col_ok: stride 1, kh 9 / 7 / 5, 3 <= kw <= 17 (CTW + kw - 1 <= CPW), 16-channel chunks, <= 64 couts (conv_col_bn: 32 up to 32)."""
    ck = "conv_col_kernel<%d, %d>"
    return [
        spec("col 9x9", ck % (9, 64), "col", 1, 18, 40, 32, 64, k=(9, 9)),
        spec("col 9x3 one chunk", ck % (9, 32), "col", 1, 18, 33, 16, 24, k=(9, 3)),
        spec("col 7x17 widest", ck % (7, 64), "col", 1, 17, 40, 16, 40, k=(7, 17)),
        spec("col 7x7 16 chunks", ck % (7, 32), "col", 1, 9, 33, 256, 32, k=(7, 7), real_act=A.ACT_SWISH),
        spec("col 5x5 up + res", ck % (5, 64), "col", 2, 9, 20, 32, 64, k=(5, 5), inshift=1, res=dict(), act2=A.ACT_RELU),
        spec("col 5x3 ragged", ck % (5, 32), "col", 3, 9, 50, 16, 32, k=(5, 3), widths=(50, 7, 33)),         # (ragged: not packed)
        spec("col 5x5 packed batch", ck % (5, 64), "col", 3, 9, 20, 16, 64, k=(5, 5)),                      # OW % 32 != 0, n >= 2: side by side
        spec("col 9x9 hilo packed", ck % (9, 64), "col", 2, 17, 12, 16, 40, k=(9, 9), hilo=True),
    ]


def _c3():
    """conv_c3_plan picks the tile (2 rw rows x 32 (8 / rw) columns) that covers the map best: 32 x 40 -> rw 8, 21 x 70 -> rw 4, 9 x 165 -> rw 2
    (the smallest maps with two or three tiles per axis that the plan gives to each shape).  Np <= 32 without F_HLSUM: the 32-cout form."""
    c, c32 = "conv_c3_kernel<%d, %d>", "conv_c3n32_kernel<%d, %d>"
    maps = {8: (32, 40), 4: (21, 70), 2: (9, 165)}
    out = []
    for rw, (h, w) in maps.items():
        out.append(spec(f"c3 rw{rw} 96 couts", c % (rw, 8 // rw), "col", 1, h, w, 48, 96, k=(3, 3)))          # 3 chunks, a cout tail: 64 + 32
        out.append(spec(f"c3n32 rw{rw}", c32 % (rw, 8 // rw), "col", 1, h, w, 16, 24, k=(3, 3), res=dict(), act2=A.ACT_RELU))
    out += [
        spec("c3 hilo 16 chunks", c % (8, 1), "col", 1, 16, 32, 256, 64, k=(3, 3), hilo=True, nnz=16),
        spec("c3 hlsum", c % (8, 1), "hlsum", 2, 32, 40, 48, 24, k=(3, 3), hilo=True),
        spec("c3 hlsum rw4", c % (4, 2), "hlsum", 1, 21, 70, 32, 32, k=(3, 3), hilo=True, real_act=A.ACT_SWISH),
        spec("c3n32 hilo", c32 % (8, 1), "col", 1, 32, 40, 32, 32, k=(3, 3), hilo=True),
        spec("c3 packed batch", c % (8, 1), "col", 3, 16, 20, 32, 64, k=(3, 3)),
        spec("c3n32 packed batch rw4", c32 % (4, 2), "col", 4, 8, 40, 16, 32, k=(3, 3)),
        # ragged: sample 1 ends left of the second 32-column tile (conv_tile_right_of_sample), sample 2 inside it
        spec("c3 ragged", c % (8, 1), "col", 3, 16, 70, 32, 64, k=(3, 3), widths=(70, 20, 45)),
        spec("c3n32 ragged rw2", c32 % (2, 4), "col", 2, 4, 260, 16, 16, k=(3, 3), widths=(260, 100)),
    ]
    return out


def _pw():
    """conv_pw_ok: a 1x1 over <= 64 channels (96 with hi + lo weights) in 16-channel slices, <= PW_MAXN 256 (hi + lo: 128) couts."""
    pk = "conv_pw_kernel<%d, %s>"
    out = []
    for ks in (1, 2, 3, 4):
        out.append(spec(f"pw ks{ks}", pk % (ks, "false"), "pw", 2, 5, 27, 16 * ks - (8 if ks in (1, 3) else 0), 40 if ks < 4 else 256,
                        real_act=ACTS_REAL[ks - 1]))
    for ks in (1, 2, 3, 4, 5, 6):
        out.append(spec(f"pw ks{ks} hilo", pk % (ks, "true"), "pw", 1, 9, 31, 16 * ks - (8 if ks in (2, 5) else 0), 72 if ks < 6 else 128,
                        hilo=True, real_act=ACTS_REAL[ks % 4]))
    out += [
        spec("pw pixshuf", pk % (2, "false"), "pw", 2, 5, 27, 32, 96, pixshuf=True, in_ld_extra=16),
        spec("pw pixshuf hilo", pk % (3, "true"), "pw", 1, 5, 27, 48, 64, pixshuf=True, hilo=True, real_act=A.ACT_SWISH),
        spec("pw pixshuf onech f32", pk % (2, "false"), "pw", 2, 5, 27, 32, 32, pixshuf=True, onech=True, out_f32=True, real_act=A.ACT_SIGMOID),
        spec("pw pair out", pk % (2, "true"), "pw", 1, 5, 27, 32, 40, hilo=True, lo_out=True),
        spec("pw tail ks2", "conv_pw_tail_kernel<2>", "pw", 2, 5, 27, 32, 64, tail2=True),
        spec("pw tail ks4", "conv_pw_tail_kernel<4>", "pw", 1, 9, 31, 64, 96, tail2=True, real_act=A.ACT_RELU),
    ]
    return out


def _stem():
    sk = "conv_stem_kernel<%d, %d, %s, false>"
    return [
        spec("stem s1 3ch 16 couts", sk % (1, 1, "false"), "stem", 2, 9, 35, 8, 16, k=(3, 3), real_ch=3),
        spec("stem s1 hilo 4ch 40 couts", sk % (1, 1, "true"), "stem", 1, 11, 33, 8, 40, k=(3, 3), real_ch=4, hilo=True),
        spec("stem s2 4ch 64 couts", sk % (2, 2, "false"), "stem", 2, 17, 67, 8, 64, k=(3, 3), s=(2, 2), real_ch=4, real_act=A.ACT_SWISH),
        spec("stem s2 hilo 3ch 40 couts", sk % (2, 2, "true"), "stem", 1, 19, 65, 8, 40, k=(3, 3), s=(2, 2), real_ch=3, hilo=True),
        spec("stem s2 even map ragged", sk % (2, 2, "false"), "stem", 2, 16, 66, 8, 16, k=(3, 3), s=(2, 2), real_ch=3, widths=(33, 9)),
    ]


def _dwpw():
    """conv_dwpw_ok: a 3x3 depthwise conv (stride 1 / 2) over <= 96 channels in front of a 1x1 with hi + lo weights.  conv_dwpw_rows_stride: a PAIR
    input, pad 1 and <= DWPW_ROWS_MAX_KS(_S1) = 3 slices take the row-streaming form; one slice more, a plain input, or pad 0 the tile form."""
    rows, tile = "conv_dwpw_rows_kernel<%d, true, %d>", "conv_dwpw_kernel<%d, 3, %s>"
    out = []
    for ks in (1, 2, 3):
        for s in (1, 2):
            out.append(spec(f"dwpw rows ks{ks} s{s}", rows % (ks, s), "pw", 2 if ks == 1 else 1, 9, 35, 16 * ks - (8 if ks == 2 else 0), 40, k=(3, 3),
                            s=(s, s), hilo=True, dwpre=dict(lo_in=True), nnz=8, res=dict() if ks == 3 else None))
    for ks in (1, 2, 3, 4, 5, 6):
        cin = 16 * ks - (8 if ks in (1, 4) else 0)
        out.append(spec(f"dwpw tile ks{ks} plain", tile % (ks, "false"), "pw", 1, 9, 35, cin, 40 if ks < 6 else 192, k=(3, 3),
                        s=(1 + ks % 2,) * 2, hilo=True, dwpre=dict(lo_in=False), nnz=8))
        # a pair input on the tile form: one slice above the row form's limit — or no padding
        out.append(spec(f"dwpw tile ks{ks} pair", tile % (ks, "true"), "pw", 1, 9, 35, cin, 72, k=(3, 3), s=(1 + (ks + 1) % 2,) * 2,
                        pad=None if ks > 3 else (0, 0), hilo=True, dwpre=dict(lo_in=True), nnz=8, lo_out=(ks == 5)))
    # one slice above DWPW_ROWS_MAX_KS_S1 at stride 1 (the loop's ks 4 pair case has stride 2: above DWPW_ROWS_MAX_KS)
    out.append(spec("dwpw tile ks4 pair s1", tile % (4, "true"), "pw", 2, 7, 33, 64, 40, k=(3, 3), hilo=True, dwpre=dict(lo_in=True), nnz=8,
                    res=dict(lo=True)))
    return out


def _head():
    """conv_head_up2r_kernel (the resident form; VSE_HEAD_RESIDENT unset): in0 = the 1-channel full-resolution map, in2 = 64 channels at half
    resolution.  16 x 32 low-res tiles: 48 x 112 leaves the last column tile half empty."""
    hk = "conv_head_up2r_kernel"
    return [
        spec("head u ld1", hk, "head", 2, 32, 64, 8, 64, k=(3, 3), src2=(64, 1), dot=dict(f32=True, ld=1), u_ld=1),
        spec("head u ld8 96x224", hk, "head", 1, 96, 224, 8, 64, k=(3, 3), src2=(64, 1), dot=dict(f32=True, ld=1), u_ld=8),
        spec("head 24 couts f16 map", hk, "head", 1, 34, 66, 8, 24, k=(3, 3), src2=(64, 1), dot=dict(f32=False, ld=8), u_ld=8),
    ]


def _epilogue():
    """Every branch of conv_epilogue_tile, once, on the two cheapest kernels (conv_pw_kernel<2, false>, conv_gemm_kernel configuration 2)."""
    pw2, g2 = "conv_pw_kernel<2, false>", gemm(2, 1)
    P = lambda name, **kw: spec("ep pw " + name, pw2, "pw", 2, 5, 7, 32, kw.pop("np_", 40), **kw)                  # noqa: E731
    G = lambda name, **kw: spec("ep gemm " + name, g2, "tile32", 2, 5, 7, 32, kw.pop("np_", 24), k=(3, 3), **kw)    # noqa: E731
    out = []
    for mk in (P, G):
        out += [
            # vec16 == 0: the view starts 8 bytes into a 16-byte group / pixels 8 bytes apart modulo 16
            mk("half4 view offset 8 bytes", out_off=4),
            mk("half4 view offset 8 bytes + res", out_off=4, res=dict()),
            mk("half4 ld % 8 == 4", out_ld_extra=4),
            mk("half4 ld % 8 == 4 + res", out_ld_extra=4, res=dict(ld_extra=4), act2=A.ACT_RELU),
            mk("half4 through the residual", res=dict(off=4)),
            mk("resshift 1 odd map", res=dict(shift=1)),
            mk("pair residual", res=dict(lo=True)),
            mk("pair out", lo_out=True),
            mk("pair out + pair residual", lo_out=True, res=dict(lo=True), act2=A.ACT_RELU),
            mk("ogate", gate=True, act=A.ACT_NONE, real_act=A.ACT_NONE),
            mk("ogate + res", gate=True, act=A.ACT_NONE, real_act=A.ACT_NONE, res=dict()),
            mk("act2 after residual", res=dict(), act2=A.ACT_RELU, real_act=A.ACT_SWISH),
            mk("affine", post=True, real_act=A.ACT_HSIGMOID),
            mk("affine + res + act2", post=True, res=dict(), act2=A.ACT_RELU, real_act=A.ACT_SIGMOID),
            mk("fp32 out", out_f32=True),
            mk("fp32 out + res", out_f32=True, res=dict(), real_act=A.ACT_SWISH),
            mk("ragged widths 0 1 OW", widths=(0, 1)) if mk is G else mk("ragged widths 0 1 OW", widths=(0, 7)),
            mk("ragged widths OW 1", widths=(7, 1), res=dict()),
        ]
    return out


GROUPS = {"gemm": _gemm, "gemm_m65k": _gemm_m65k, "gemm_n192": _gemm_n192, "gemm_n256": _gemm_n256, "smallm": _smallm, "mfma": _mfma, "patch": _patch, "col": _col, "c3": _c3, "pw": _pw, "stem": _stem, "dwpw": _dwpw,
          "head": _head, "epilogue": _epilogue}


def instantiations(group):
    """The instantiation list of a group: what its cases were written for."""
    return sorted({sp.expect for sp in GROUPS[group]()})


def _refused():
    """Well-formed records but for ONE property: a negative code, no launch."""
    inval, unsup = H.VSE_E_INVAL, H.VSE_E_UNSUPPORTED
    return [
        spec("F_WK32 with 49 taps", None, "tile32", 1, 9, 11, 32, 32, k=(7, 7), rc=unsup),                  # conv_gemm_mode: <= 31 taps; no other reader of 32-deep tiles
        spec("F_IMGW on a 3x3", None, "tile32", 2, 8, 8, 64, 40, k=(3, 3), imgw=True, rc=unsup),
        spec("F_DOT1 without a patch or column family", None, "tile64", 1, 16, 40, 24, 64, k=(3, 3), dot=dict(f32=True, ld=1), rc=unsup),
        spec("Np % 8 != 0", None, "pw", 2, 5, 7, 32, 36, out_ld_extra=4, rc=inval),
        spec("P_LO_OUT with F_OUT_F32", None, "pw", 2, 5, 7, 32, 40, lo_out=True, out_f32=True, rc=inval),
        spec("wl_out with F_PIXSHUF", None, "pw", 2, 5, 7, 32, 64, pixshuf=True, widths=(14, 3), rc=unsup),
        spec("pw 264 couts", None, "pw", 1, 5, 7, 32, 264, rc=unsup),                                       # PW_MAXN + 8
        spec("pw hilo 136 couts", None, "pw", 1, 5, 7, 32, 136, hilo=True, rc=unsup),                       # PW_MAXN_HILO + 8
        spec("pw tail ks3", None, "pw", 1, 5, 7, 48, 64, tail2=True, rc=unsup),
    ]


REFUSED = {"refused": _refused}
