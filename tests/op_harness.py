"""One-record plans: run a single `vse_op` record — one HIP kernel — on tensors the test chooses, on the GPU (run_gpu) and on the
CPU emulator (run_emulator), and hold the result to a plain fp64 reference of the same operation.

A plain helper module like tests/parity.py (no fixtures, no pytest settings).  It has four parts (and, at the end, the same four for
OP_CONV: conv_op, conv_pack — the compiler's own static packers —, conv_name — the library's own answer, vse_op_kernel_name —, ref_conv and
conv_reference; the cases are tests/conv_cases.py — and for OP_CHAIN: chain_stage, chain_op, chain_form, ref_chain, ref_shuffle, with the
compiler's static chains.chain_plan / chain_pack as the packer; the cases are tests/chain_cases.py):

  * builders for ir.VIEW_DT / ir.OP_DT records (the fields follow the comments of ir.py and the checks at the top of each `case` of
    launch_simple_op, csrc/simple_ops.hip), and a weight blob with the compiler's 256-byte alignment;
  * the kernel FORM a record selects (softmax_form, dwconv_form, lstm_form, pool_form): the launcher's own conditions, restated, so that a
    test can assert that its case still reaches the path it was written for;
  * run_gpu / run_emulator: the same records and the same byte images through vse_plan_run_ragged and through oracle/ir_emul.py;
  * one reference per op, written for a numpy dtype: evaluated in float64 it is the reference, in float32 it measures `e32`, the distance
    of a plain single-precision evaluation from it — the yardstick of the error bound.  None of them calls the emulator.

The bound (never derived from what a kernel returns):
    fp16 output:  |got - ref64| <= ulp16(|ref64|) + 8 e32          fp32 output:  |got - ref64| <= 16 ulp32(|ref64|) + 8 e32
e32 = the largest |ref32 - ref64| over the tensor.  The ulp term is one rounding of a value that is itself slightly off; the factor 8
covers another fp32 summation order and the fast __expf.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from vse_amd import compiler, ir

VSE_E_INVAL, VSE_E_HIP, VSE_E_UNSUPPORTED = -1, -2, -3


# ---------------------------------------------------------------------------------------------------------------- records
def ext(k):
    """Arena id of external pointer k (tensors[k] of run_gpu / run_emulator)."""
    return ir.ARENA_EXT0 + k


def view(arena, n, h, w, c, ld=None, esize=2, off=0):
    """ir.VIEW_DT: [n,h,w] pixels of c channels, `ld` elements apart (default c), `off` BYTES into the arena."""
    v = ir.empty_view()
    v["off"], v["arena"] = off, arena
    v["n"], v["h"], v["w"], v["c"] = n, h, w, c
    v["ld"], v["esize"] = (c if ld is None else ld), esize
    return v


def op(kind, ins=(), out=None, out2=None, flags=0, p=None, f=None, w_off=0, b_off=0, aux_off=0, wl=(0, 0)):
    """One ir.OP_DT record.  ins: up to three views (None = absent); p / f: {slot: value}; wl = (P_WLIN, P_WLOUT): 1 + width level."""
    r = np.zeros(1, ir.OP_DT)
    r["kind"], r["flags"] = kind, flags
    for k, v in (p or {}).items():
        r["p"][0, k] = v
    for k, v in (f or {}).items():
        r["f"][0, k] = v
    r["p"][0, ir.P_WLIN], r["p"][0, ir.P_WLOUT] = wl
    for name, v in zip(("in0", "in1", "in2"), list(ins) + [None] * (3 - len(ins))):
        if v is not None:
            r[name] = v
    if out is not None:
        r["out"] = out
    if out2 is not None:
        r["out2"] = out2
    r["w_off"], r["b_off"], r["aux_off"] = w_off, b_off, aux_off
    return r


class Blob:
    """Weight blob of a one-record plan: every table 256-byte aligned, like compiler.WeightStore."""

    def __init__(self):
        self.buf = bytearray()

    def add(self, arr):
        off = (len(self.buf) + 255) // 256 * 256
        self.buf.extend(b"\0" * (off - len(self.buf)))
        self.buf.extend(np.ascontiguousarray(arr).tobytes())
        return off

    def array(self):
        return np.frombuffer(bytes(self.buf) + b"\0" * max(0, 16 - len(self.buf)), dtype=np.uint8).copy()


def dwconv_op(in0, out, k, s, pad, w_off, b_off, act=ir.ACT_NONE, act_a=0.0, act_b=0.0, post_a=1.0, post_b=0.0, gate=None,
              gate_res=False, lo_in=0, lo_out=0, hilo=False, wl=(0, 0)):
    """k = (kh, kw), s = (sh, sw), pad = (ph, pw); gate = SE gate view [N,1,1,C] (F_GATE; gate_res: x * g + x); lo_in / lo_out = channel
    offset of the lo half of an fp16 hi + lo pair input / output (P_LO_RES / P_LO_OUT)."""
    flags = (ir.F_GATE | (ir.F_RES if gate_res else 0) if gate is not None else 0) | (ir.F_HILO if hilo else 0)
    return op(ir.OP_DWCONV, [in0, gate], out, flags=flags, w_off=w_off, b_off=b_off, wl=wl,
              p={ir.P_KH: k[0], ir.P_KW: k[1], ir.P_SH: s[0], ir.P_SW: s[1], ir.P_PH: pad[0], ir.P_PW: pad[1], ir.P_ACT: act,
                 ir.P_LO_OUT: lo_out, ir.P_LO_RES: lo_in},
              f={ir.FS_ACT_A: act_a, ir.FS_ACT_B: act_b, ir.FS_POST_A: post_a, ir.FS_POST_B: post_b})


def pool_op(in0, out, k, s, pad, is_max, ceil=False, exclusive=True, wl=(0, 0)):
    return op(ir.OP_POOL, [in0], out, wl=wl,
              p={ir.P_KH: k[0], ir.P_KW: k[1], ir.P_SH: s[0], ir.P_SW: s[1], ir.P_PH: pad[0], ir.P_PW: pad[1],
                 ir.P_POOL_MAX: int(is_max), ir.P_POOL_CEIL: int(ceil), ir.P_POOL_EXCL: int(exclusive)})


def gap_op(in0, scratch, out, wl=(0, 0)):
    """scratch = fp32 view [n, splits, 1, c] (the ragged row form: splits = in0.h)."""
    return op(ir.OP_GAP, [in0, None, scratch], out, wl=wl)


def layernorm_op(in0, out, eps, w_off, wl=(0, 0)):
    """w_off -> fp32 [2 C]: scale, then bias."""
    return op(ir.OP_LAYERNORM, [in0], out, f={ir.FS_EPS: eps}, w_off=w_off, wl=wl)


def attn_op(qkv, out, heads, hd, scale, wl=(0, 0)):
    return op(ir.OP_ATTN, [qkv], out, p={ir.P_HEADS: heads, ir.P_HDIM: hd}, f={ir.FS_SCALE: scale}, wl=wl)


def softmax_op(in0, idx_maxp, probs, ncls, wl=(0, 0)):
    return op(ir.OP_SOFTMAX, [in0], idx_maxp, out2=probs, p={ir.P_NCLS: ncls}, wl=wl)


def lstm_op(gates, out, H, mode, w_off, mfma, wl=(0, 0)):
    """gates: one view, or [forward, reverse] for mode 2 (MFMA form only)."""
    gates = list(gates) if isinstance(gates, (list, tuple)) else [gates]
    p = {ir.P_HID: H, ir.P_REVERSE: mode}
    if mfma:
        p[ir.P_WAVES] = 16
    return op(ir.OP_LSTM, gates, out, flags=ir.F_LSTM_MFMA if mfma else 0, p=p, w_off=w_off, wl=wl)


# ---------------------------------------------------------------------------------------------------------------- kernel forms
def softmax_form(r):
    """("reg", NV): softmax_reg_kernel<T, NV>, or ("scalar", 0): softmax_kernel — the conditions of `case OP_SOFTMAX` (the base pointer
    of a tensor from torch's allocator is 16-byte aligned)."""
    r = r[0] if r.ndim else r
    es, ld, ncls = int(r["in0"]["esize"]), int(r["in0"]["ld"]), int(r["p"][ir.P_NCLS])
    vw = 16 // es
    nvec = (ncls + vw - 1) // vw
    nvt = (nvec + 255) // 256
    if int(r["in0"]["off"]) % 16 == 0 and (ld * es) % 16 == 0 and nvt <= 8 and ncls > 0 and nvec * vw <= ld:
        return "reg", next(nv for nv in (1, 2, 4, 8) if nvt <= nv)
    return "scalar", 0


def dwconv_form(r):
    """("col", nseg, rows per segment) | ("row", 0, 0) | ("generic", 0, 0): the conditions and the segment arithmetic of `case OP_DWCONV`."""
    r = r[0] if r.ndim else r
    p, i, o = r["p"], r["in0"], r["out"]
    kh, kw, sh, sw, ph, pw = (int(p[k]) for k in range(6))
    gated = bool(int(r["flags"]) & ir.F_GATE)
    if (not gated and not p[ir.P_LO_OUT] and not p[ir.P_LO_RES] and kw == kh and kw in (3, 5) and sw == 1 and sh in (1, 2)
            and ph == kw // 2 and pw == kw // 2 and int(o["w"]) == int(i["w"]) and int(o["h"]) == (int(i["h"]) + 2 * (kw // 2) - kw) // sh + 1):
        cols = int(o["n"]) * ((int(o["w"]) + 3) // 4) * (int(i["c"]) >> 1)
        nseg = max(1, min((262144 + cols - 1) // cols, (int(o["h"]) + 3) // 4))
        rs = (int(o["h"]) + nseg - 1) // nseg
        return "col", (int(o["h"]) + rs - 1) // rs, rs
    if kw in (3, 5) and sw in (1, 2):
        return "row", 0, 0
    return "generic", 0, 0


def lstm_form(r):
    """"mfma" (lstm_mfma16_kernel) | "scalar" (lstm_kernel) | "refused"."""
    r = r[0] if r.ndim else r
    H, mode = int(r["p"][ir.P_HID]), int(r["p"][ir.P_REVERSE])
    if int(r["flags"]) & ir.F_LSTM_MFMA:
        return "mfma" if H == 256 and int(r["p"][ir.P_WAVES]) == 16 else "refused"
    return "scalar" if H <= 256 and mode <= 1 else "refused"


def pool_form(r):
    """The branch of pool_kernel: "max" (packed fp16 maxima), "avg_excl" (divide by the taps inside), "avg_incl" (by the padded window)."""
    r = r[0] if r.ndim else r
    if int(r["p"][ir.P_POOL_MAX]):
        return "max"
    return "avg_excl" if int(r["p"][ir.P_POOL_EXCL]) else "avg_incl"


# ---------------------------------------------------------------------------------------------------------------- running
class OpRefused(RuntimeError):
    """vse_plan_create / vse_plan_run_ragged returned a negative code."""

    def __init__(self, rc, what, msg):
        super().__init__(f"{what} rc={rc}: {msg}")
        self.rc = rc


@dataclass
class Run:
    """One plan run: the records, the weight blob, the byte images of the external arenas (tensors[k] = arena ext(k), inputs and
    outputs alike; outputs pre-filled with NaN / -1 so that an element nobody wrote shows), the width table, the workspace size."""
    ops: np.ndarray
    blob: np.ndarray
    tensors: List[np.ndarray]
    widths: Optional[np.ndarray] = None
    ws_bytes: int = 0


@dataclass
class Case:
    """check(outs) gets, per run, the list of arenas after the run (same shapes and dtypes as Run.tensors), asserts, and returns the
    worst error / bound.  refused: every run must return a negative code.  may_refuse: VSE_E_UNSUPPORTED is a valid answer too."""
    name: str
    runs: List[Run]
    check: Optional[Callable] = None
    refused: bool = False
    may_refuse: bool = False
    note: dict = field(default_factory=dict)


def run_gpu(ctx, ops, weight_blob, tensors, widths=None, ws_bytes=0):
    """A plan of these records on ctx's device; -> the external arenas after the run (numpy, shapes and dtypes of `tensors`)."""
    t, lib = ctx.torch, ctx.lib
    blob = np.ascontiguousarray(weight_blob, np.uint8)
    if blob.nbytes < 16:
        blob = np.concatenate([blob, np.zeros(16 - blob.nbytes, np.uint8)])
    ops = np.ascontiguousarray(ops)
    dev = [t.from_numpy(np.ascontiguousarray(a).copy()).to(ctx.tdev) for a in tensors]
    ws = t.zeros(max(int(ws_bytes), 256), dtype=t.uint8, device=ctx.tdev)
    wt = None
    if widths is not None:
        wt = t.from_numpy(np.ascontiguousarray(widths, np.int32).copy()).to(ctx.tdev)
    t.cuda.synchronize(ctx.tdev)
    wid = lib.vse_weights_upload(ctx.handle, blob.ctypes.data_as(C.c_void_p), blob.nbytes)
    if wid < 0:
        raise OpRefused(wid, "vse_weights_upload", lib.vse_last_error().decode(errors="replace"))
    handle = C.c_void_p()
    try:
        rc = lib.vse_plan_create(ctx.handle, wid, ops.ctypes.data_as(C.c_void_p), len(ops), int(ws_bytes), C.byref(handle))
        if rc < 0:
            raise OpRefused(rc, "vse_plan_create", lib.vse_last_error().decode(errors="replace"))
        ptrs = (C.c_void_p * len(dev))(*[d.data_ptr() for d in dev])
        rc = lib.vse_plan_run_ragged(handle, C.c_void_p(ws.data_ptr()), ptrs, len(dev),
                                     C.c_void_p(wt.data_ptr()) if wt is not None else None, ctx.stream())
        if rc < 0:
            raise OpRefused(rc, "vse_plan_run_ragged", lib.vse_last_error().decode(errors="replace"))
        t.cuda.synchronize(ctx.tdev)
        return [d.cpu().numpy() for d in dev]
    finally:
        if handle:
            lib.vse_plan_destroy(handle)
        lib.vse_weights_free(ctx.handle, wid)


class _Weights:
    def __init__(self, blob):
        self.blob = blob

    def array(self):
        return self.blob


class _StubProgram:
    """What ir_emul.Emulator reads of a compiled Program."""

    def __init__(self, ops, blob, ws_bytes, has_widths):
        self.ops, self.ws_bytes, self.weights = ops, max(int(ws_bytes), 16), _Weights(np.ascontiguousarray(blob, np.uint8).copy())
        self.outputs, self.wlevels = [], ([] if has_widths else None)


def run_emulator(ops, weight_blob, tensors, widths=None, ws_bytes=0):
    """The same records through oracle/ir_emul.py with every stored tensor rounded where the kernels round; -> like run_gpu."""
    from oracle import ir_emul
    emu = ir_emul.Emulator(_StubProgram(ops, weight_blob, ws_bytes, widths is not None), round_f16=True)
    outs = emu.run_records(tensors, None if widths is None else np.ascontiguousarray(widths, np.int32))
    return [o.view(a.dtype).reshape(a.shape) for o, a in zip(outs, tensors)]


def run_case(case, runner):
    """runner(ops, blob, tensors, widths, ws_bytes) = run_gpu bound to a context, or run_emulator.  -> worst error / bound (None for a
    refused case)."""
    outs = []
    for r in case.runs:
        try:
            outs.append(runner(r.ops, r.blob, r.tensors, r.widths, r.ws_bytes))
        except OpRefused as e:
            if case.refused or (case.may_refuse and e.rc == VSE_E_UNSUPPORTED):
                case.note["rc"] = e.rc
                continue
            raise
        else:
            assert not case.refused, (case.name, "ran, where the library must refuse the record")
    if case.refused or (case.may_refuse and len(outs) < len(case.runs)):
        return None
    case.note["rc"] = 0
    return case.check(outs)


# ---------------------------------------------------------------------------------------------------------------- the bound
def f16(a):
    """Round to fp16 (the values a kernel gets)."""
    return np.asarray(a).astype(np.float16)


def ulp16(a):
    a = np.abs(np.asarray(a, np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -14))) - 10)


def ulp32(a):
    a = np.abs(np.asarray(a, np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -126))) - 23)


def reference(fn):
    """fn(dtype) -> array or tuple of arrays.  -> (float64 results, e32 per result)."""
    r64, r32 = fn(np.float64), fn(np.float32)
    if not isinstance(r64, tuple):
        r64, r32 = (r64,), (r32,)
    for a, b in zip(r64, r32):
        assert a.dtype == np.float64 and b.dtype == np.float32, (a.dtype, b.dtype)
    e32 = tuple(float(np.abs(b.astype(np.float64) - a).max()) if a.size else 0.0 for a, b in zip(r64, r32))
    return r64, e32


def ratio(got, ref64, e32, what, pair=False):
    """Worst |got - ref64| / bound; asserts <= 1.  got: fp16 or fp32 array (the bound follows its dtype); pair: `got` is float64 hi + lo
    of an fp16 pair tensor, held to 2^-20 relative + 8 e32."""
    got = np.asarray(got)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    if pair:
        bound = np.abs(ref64) * 2.0 ** -20 + 2.0 ** -24 + 8 * e32          # (2^-24: the smallest fp16 step, a lo half cannot carry less)
    elif got.dtype == np.float16:
        bound = ulp16(ref64) + 8 * e32
    else:
        assert got.dtype == np.float32, got.dtype
        bound = 16 * ulp32(ref64) + 8 * e32
    err = np.abs(got.astype(np.float64) - ref64)
    ok = err <= bound                    # (NaN — an element nobody wrote — compares false)
    worst = float(np.nanmax(err / bound)) if err.size else 0.0
    assert ok.all(), (what, "error / bound", worst, "at", tuple(int(v) for v in np.argwhere(~ok)[0]), "e32", e32,
                      "unwritten" if np.isnan(got.astype(np.float64)).any() else "")
    return worst


# ---------------------------------------------------------------------------------------------------------------- references
def ref_act(x, code, a=0.0, b=0.0):
    dt = x.dtype.type
    if code == ir.ACT_NONE:
        return x
    if code == ir.ACT_RELU:
        return np.maximum(x, dt(0))
    if code == ir.ACT_HSWISH:
        return x * np.clip(x + dt(3), dt(0), dt(6)) / dt(6)
    if code == ir.ACT_SWISH:
        return x / (dt(1) + np.exp(-x))
    if code == ir.ACT_SIGMOID:
        return dt(1) / (dt(1) + np.exp(-x))
    if code == ir.ACT_HSIGMOID:
        return np.clip(x * dt(np.float32(a)) + dt(np.float32(b)), dt(0), dt(1))
    raise ValueError(code)


def mask_width(y, wl):
    """Zeros right of each sample's width (what every producing kernel of a ragged plan stores there)."""
    if wl is not None:
        y = y.copy()
        for n, wn in enumerate(wl):
            y[n, :, int(wn):] = 0
    return y


def ref_dwconv(x, wk, bias, k, s, pad, act=ir.ACT_NONE, act_a=0.0, act_b=0.0, post_a=1.0, post_b=0.0, wl_out=None, dt=np.float64):
    """x [n,h,w,c] (already gated / hi + lo summed), wk fp32 [kh*kw][c], bias fp32 [c] -> [n,oh,ow,c]."""
    (kh, kw), (sh, sw), (ph, pw) = k, s, pad
    n, h, w, c = x.shape
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    xp = np.zeros((n, h + 2 * ph + sh, w + 2 * pw + sw, c), dt)
    xp[:, ph:ph + h, pw:pw + w] = x.astype(dt)
    acc = np.broadcast_to(bias.astype(dt), (n, oh, ow, c)).copy()
    for dy in range(kh):
        for dx in range(kw):
            acc += xp[:, dy:dy + sh * oh:sh, dx:dx + sw * ow:sw][:, :oh, :ow] * wk[dy * kw + dx].astype(dt)
    y = ref_act(acc, act, act_a, act_b) * dt(np.float32(post_a)) + dt(np.float32(post_b))
    return mask_width(y, wl_out)


def ref_pool(x, k, s, pad, is_max, ceil, exclusive, wl_in=None, wl_out=None, out_w=None, dt=np.float64):
    """Paddle's pool2d = F.max_pool2d / F.avg_pool2d(count_include_pad=not exclusive, ceil_mode=ceil).  wl_in: every sample is pooled
    over its own width and written left-aligned into [n, oh, out_w, c]."""
    tdt = torch.float64 if dt == np.float64 else torch.float32

    def pool(xs):
        xs = torch.from_numpy(np.ascontiguousarray(xs.astype(dt))).permute(0, 3, 1, 2)
        if is_max:
            y = F.max_pool2d(xs, k, s, pad, ceil_mode=ceil)
        else:
            y = F.avg_pool2d(xs, k, s, pad, ceil_mode=ceil, count_include_pad=not exclusive)
        return y.permute(0, 2, 3, 1).to(tdt).numpy()
    if wl_in is None:
        return mask_width(pool(x), wl_out)
    outs = [pool(x[n:n + 1, :, :int(wn)]) for n, wn in enumerate(wl_in)]
    y = np.zeros((x.shape[0], outs[0].shape[1], out_w, x.shape[3]), dt)
    for n, o in enumerate(outs):
        y[n, :, :o.shape[2]] = o[0]
    return mask_width(y, wl_out)


def ref_gap(x, wl_in=None, dt=np.float64):
    """[n,h,w,c] -> [n,1,1,c]: the mean over the map (over the sample's own width in a ragged batch)."""
    n = x.shape[0]
    y = np.zeros((n, 1, 1, x.shape[3]), dt)
    for b in range(n):
        xs = x[b].astype(dt) if wl_in is None else x[b, :, :int(wl_in[b])].astype(dt)
        y[b, 0, 0] = xs.reshape(-1, x.shape[3]).sum(0, dtype=dt) / dt(xs.shape[0] * xs.shape[1])
    return y


def ref_layernorm(x, g, b, eps, wl_out=None, dt=np.float64):
    """Two-pass mean / variance over the channels."""
    x = x.astype(dt)
    c = dt(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=dt) / c
    d = x - mean
    var = (d * d).sum(-1, keepdims=True, dtype=dt) / c
    y = d / np.sqrt(var + dt(np.float32(eps))) * g.astype(dt) + b.astype(dt)
    return mask_width(y, wl_out)


def ref_attn(qkv, heads, hd, scale, lens=None, dt=np.float64):
    """qkv [B,1,T,3C] -> [B,1,T,C]; a sample's keys and queries end at its own length (rows behind it are zeros)."""
    B, _, T, _ = qkv.shape
    Cc = heads * hd
    out = np.zeros((B, 1, T, Cc), dt)
    for b in range(B):
        tb = T if lens is None else int(lens[b])
        x = qkv[b, 0, :tb].astype(dt).reshape(tb, 3, heads, hd)
        q, k, v = x[:, 0] * dt(np.float32(scale)), x[:, 1], x[:, 2]
        s = np.einsum("thd,uhd->htu", q, k)
        s = np.exp(s - s.max(-1, keepdims=True))
        a = s / s.sum(-1, keepdims=True, dtype=dt)
        out[b, 0, :tb] = np.einsum("htu,uhd->thd", a, v).reshape(tb, Cc)
    return out


def ref_softmax(x, dt=np.float64):
    """x [rows, ncls] -> (probabilities, 1 / sum = the largest probability)."""
    x = x.astype(dt)
    e = np.exp(x - x.max(-1, keepdims=True))
    s = e.sum(-1, keepdims=True, dtype=dt)
    return e / s, (dt(1) / s)[:, 0]


def ref_lstm(g, w_hh, rev, lens=None, dt=np.float64):
    """g [B,T,4H] = x.W_ih^T + b in gate order i, f, g, o; w_hh [4H,H] -> h [B,T,H]; the reverse pass starts at the sample's own end,
    steps behind its length give zeros."""
    B, T, H4 = g.shape
    H = H4 // 4
    w = w_hh.astype(dt)
    out = np.zeros((B, T, H), dt)

    def sig(z):
        return dt(1) / (dt(1) + np.exp(-z))
    for b in range(B):
        tb = T if lens is None else int(lens[b])
        h, c = np.zeros(H, dt), np.zeros(H, dt)
        for t in (range(tb - 1, -1, -1) if rev else range(tb)):
            z = g[b, t].astype(dt) + w @ h
            c = sig(z[H:2 * H]) * c + sig(z[:H]) * np.tanh(z[2 * H:3 * H])
            h = sig(z[3 * H:]) * np.tanh(c)
            out[b, t] = h
    return out


def lstm_mfma_blob(w_hhs):
    """The MFMA kernel's W_hh stream of one or two directions (Compiler.lstm_fragments16)."""
    return np.concatenate([compiler.Compiler.lstm_fragments16(np.ascontiguousarray(w, np.float32)) for w in w_hhs])


def lstm_mfma_gates(g):
    """Gate pre-activations [.., 4H] in i, f, g, o order -> the channel order the MFMA kernel reads (Compiler.lstm_gate_order)."""
    return np.ascontiguousarray(g[..., compiler.Compiler.lstm_gate_order(g.shape[-1] // 4)])


# ---------------------------------------------------------------------------------------------------------------- OP_CONV
# One conv record = one instantiation of one conv kernel family.  The fields follow conv_params and the checks at the top of launch_conv
# (csrc/conv_select.hip); which instantiation a record selects is asked of the library (conv_name), never restated here.
def conv_op(in0, out, k, s, pad, cout, ktot, cinp, w_off, b_off, flags=0, act=ir.ACT_NONE, act2=ir.ACT_NONE, act_a=0.0, act_b=0.0,
            post_a=1.0, post_b=0.0, inshift=0, res=None, resshift=0, in2=None, in2shift=0, out2=None, aux_off=0, dotact=ir.ACT_NONE,
            pre_b=0.0, lo_out=0, lo_res=0, lo_in=0, wl=(0, 0)):
    """k = (kh, kw), s = (sh, sw), pad = (ph, pw); cout = P_COUT (GEMM N: padded couts, x 4 under F_PIXSHUF), ktot = P_KTOT (the padded K
    of the weight stream), cinp = P_CINP (stored input channels, both sources of an F_SRC2 conv).  Views: in0; res = in1 (F_RES, read through
    resshift, a hi + lo pair when lo_res); in2 = the second source (F_SRC2, in2shift), the per-image weights (F_IMGW) or the gate (F_OGATE);
    out (a pair when lo_out); out2 = the 1-channel map of F_DOT1 / F_UP2HEAD / F_TAIL2 (dotact, pre_b = its activation and bias; aux_off =
    its weights — or the depthwise table of F_DWPRE, whose geometry k / s / pad then is, with lo_in the pair offset of in0)."""
    return op(ir.OP_CONV, [in0, res, in2], out, out2=out2, flags=flags, w_off=w_off, b_off=b_off, aux_off=aux_off, wl=wl,
              p={ir.P_KH: k[0], ir.P_KW: k[1], ir.P_SH: s[0], ir.P_SW: s[1], ir.P_PH: pad[0], ir.P_PW: pad[1], ir.P_ACT: act, ir.P_ACT2: act2,
                 ir.P_COUT: cout, ir.P_KTOT: ktot, ir.P_INSHIFT: inshift, ir.P_RESSHIFT: resshift, ir.P_CINP: cinp, ir.P_DOTACT: dotact,
                 ir.P_IN2SHIFT: in2shift, ir.P_LO_OUT: lo_out, ir.P_LO_RES: lo_res, ir.P_LO_IN: lo_in},
              f={ir.FS_ACT_A: act_a, ir.FS_ACT_B: act_b, ir.FS_POST_A: post_a, ir.FS_POST_B: post_b, ir.FS_PRE_B: pre_b})


def conv_name(rec):
    """The kernel instantiation the library launches for the record (vse_op_kernel_name: no GPU), e.g. "conv_col_kernel<9, 64>"."""
    from vse_amd import engine
    return engine.op_kernel_names(np.ascontiguousarray(rec).reshape(-1)[:1])[0]


def _rup(x, m):
    return (x + m - 1) // m * m


CONV_FAMILY_FLAGS = {"tile64": 0, "tile32": ir.F_WK32, "pw": ir.F_PW, "stem": ir.F_STEM, "patch": ir.F_PATCH, "col": ir.F_COL,
                     "hlsum": ir.F_COL | ir.F_HLSUM, "head": ir.F_PATCH | ir.F_SRC2 | ir.F_DOT1 | ir.F_UP2HEAD}


def conv_pack(family, w, kh, kw, cinp, hilo=False, ptaps=0):
    """The weight stream of one conv record, by the compiler's own packers.  w: float64 [Np][kh * kw * cinp], K in (tap, channel) order (a
    hi + lo stream is split by the packer: hi = fp16(w), lo = fp16(w - hi)).  family: tile64 / tile32 ([Kp / kt][Np][kt]: conv_gemm,
    conv_smallm, conv_mfma), pw ([Np][cinp -> 16]), stem, patch (ptaps = taps padded to whole kernel steps), col (conv_col, conv_c3),
    hlsum (conv_c3 [hi 32 | lo 32]), head (conv_head_up2).  -> (the stream, P_KTOT)."""
    Cm = compiler.Compiler
    w = np.asarray(w, np.float64)
    npad, K = w.shape
    assert K == kh * kw * cinp, (K, kh, kw, cinp)

    def padded(kp):
        m = np.zeros((npad, kp), np.float64)
        m[:, :K] = w
        return m
    if family in ("tile64", "tile32"):
        kp = _rup(K, ir.KT)
        return Cm.tile_weights(padded(kp), 32 if family == "tile32" else ir.KT, hilo=hilo).reshape(-1), kp
    if family == "pw":
        assert (kh, kw) == (1, 1)
        kp = _rup(cinp, 16)
        return Cm.pw_weights(padded(kp), hilo), kp
    if family == "stem":
        return Cm.stem_weights(padded(128), hilo), 128
    if family == "patch":
        assert not hilo and ptaps >= kh * kw
        return Cm.patch_weights(padded(_rup(K, ir.KT)), kh, kw, cinp, ptaps), ptaps * _rup(cinp, 32)
    if family == "col":
        return Cm.col_weights(w, kh, kw, cinp, hilo), K
    if family == "hlsum":
        return Cm.hlsum_weights(w, kh, kw, cinp), K
    if family == "head":
        return Cm.head_up2_weights(w, cinp), 2 * 4 * 4 * 32 + 32
    raise ValueError(family)


def conv_seen_weights(w, hilo):
    """The matrix a kernel sees of the float64 matrix handed to conv_pack: fp16(w), or hi + lo summed in float64."""
    w = np.asarray(w, np.float64)
    hi = w.astype(np.float16).astype(np.float64)
    return hi + (w - hi).astype(np.float16).astype(np.float64) if hilo else hi


def _up(t, shift):
    return t if not shift else np.repeat(np.repeat(t, 1 << shift, axis=1), 1 << shift, axis=2)


def _matmul(a, w, dt, seq):
    """a [..., K] x w [N, K] -> [..., N] in dt; seq: strictly sequential over 16-channel chunks."""
    if not seq:
        return np.matmul(a, w.T)
    acc = np.zeros(a.shape[:-1] + (w.shape[0],), dt)
    for c0 in range(0, a.shape[-1], 16):
        acc = acc + np.matmul(a[..., c0:c0 + 16], w[:, c0:c0 + 16].T)
    return acc


def ref_conv(x, w, bias, k, s, pad, dt=np.float64, seq=False, x2=None, inshift=0, in2shift=0, act=ir.ACT_NONE, act_a=0.0, act_b=0.0,
             post_a=1.0, post_b=0.0, gate=None, pixshuf=False, res=None, resshift=0, act2=ir.ACT_NONE, wl_out=None, dot=None, tail2=None,
             dwpre=None, wimg=None):
    """The whole OP_CONV record, plainly.  x [n,h,w,c] (a pair tensor: hi + lo summed), x2 = the second source of a virtual concat, each read
    through its own nearest-neighbour shift; w [Np][kh * kw * cinp] = the matrix the kernel sees (conv_seen_weights), K in (tap, channel)
    order — wimg [n][Np][cinp]: one matrix per image (F_IMGW); bias fp32 [Np].  In the record's order: gather, (dwpre = (wd [c][k*k], shift
    [c], act, act_a, act_b, post_a, post_b): the depthwise conv of F_DWPRE in front, whose geometry k / s / pad then is), conv, bias, act,
    affine, (1 + gate [n, Np]), pixel-shuffle scatter (Np = 4 x couts in (dy, dx, co) order), residual (hi + lo summed, read through
    resshift), act2, zeros right of wl_out[n]; then dot = (weights fp32 [Np], bias, act): -> the 1-channel projection [n,oh,ow,1] alone
    (F_DOT1), or tail2 = (w2 [c1][2][2], bias, act): -> (y, the second 2x2 s2 transposed conv over fp16(y) [n,4h,4w,1]).
    seq: the accumulation runs strictly sequentially over taps and 16-channel chunks (the second float32 evaluation of e32)."""
    (kh, kw), (sh, sw), (ph, pw) = k, s, pad
    f32 = lambda v: dt(np.float32(v))          # noqa: E731
    x = _up(np.asarray(x).astype(dt), inshift)
    if x2 is not None:
        x = np.concatenate([x, _up(np.asarray(x2).astype(dt), in2shift)], axis=3)
    if dwpre is not None:
        wd, dshift, dact, da, db, dpa, dpb = dwpre
        d = ref_dwconv(x, np.asarray(wd).T, np.asarray(dshift), k, s, pad, dact, da, db, dpa, dpb, dt=dt)
        x, (kh, kw), (sh, sw), (ph, pw) = d, (1, 1), (1, 1), (0, 0)
    n, h, wd_, c = x.shape
    oh, ow = (h + 2 * ph - kh) // sh + 1, (wd_ + 2 * pw - kw) // sw + 1
    xp = np.zeros((n, h + 2 * ph + sh, wd_ + 2 * pw + sw, c), dt)
    xp[:, ph:ph + h, pw:pw + wd_] = x
    if wimg is not None:
        wi = np.asarray(wimg).astype(dt)
        acc = np.stack([_matmul(xp[b:b + 1, :oh, :ow], wi[b], dt, seq)[0] for b in range(n)])
        npad = wi.shape[1]
    else:
        w = np.asarray(w).astype(dt)
        npad = w.shape[0]
        assert w.shape[1] == kh * kw * c, (w.shape, kh, kw, c)
        acc = np.zeros((n, oh, ow, npad), dt)
        for dy in range(kh):
            for dx in range(kw):
                t = dy * kw + dx
                acc = acc + _matmul(xp[:, dy:dy + sh * oh:sh, dx:dx + sw * ow:sw][:, :oh, :ow], w[:, t * c:(t + 1) * c], dt, seq)
    y = acc + np.asarray(bias).astype(dt)
    y = ref_act(y, act, act_a, act_b) * f32(post_a) + f32(post_b)
    if gate is not None:
        y = y * (dt(1) + np.asarray(gate).astype(dt)[:, None, None, :npad])
    if pixshuf:
        cp = npad // 4
        y = y.reshape(n, oh, ow, 2, 2, cp).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * oh, 2 * ow, cp)
    if res is not None:
        r = _up(np.asarray(res).astype(dt), resshift)[:, :y.shape[1], :y.shape[2]]
        y = y.copy()
        y[..., :r.shape[3]] += r[..., :y.shape[3]]
    y = ref_act(y, act2)
    y = mask_width(y, wl_out)
    if dot is not None:
        dw, dbias, dact = dot
        z = (y * np.asarray(dw).astype(dt)).sum(-1, keepdims=True, dtype=dt) + f32(dbias)
        return ref_act(z, dact)
    if tail2 is not None:
        return y, ref_tail2(y.astype(np.float16), *tail2, dt=dt)
    return y


def ref_tail2(y16, w2, bias, act, dt=np.float64):
    """Stage B of F_TAIL2 on the fp16 values stage A stored: y16 [n,h,w,c1], w2 [c1][2][2] -> [n,2h,2w,1]."""
    n, h, w, c1 = y16.shape
    z = np.einsum("nhwc,cyx->nhywx", y16.astype(dt), np.asarray(w2).astype(dt)[:c1]).reshape(n, 2 * h, 2 * w, 1).astype(dt)
    return ref_act(z + dt(np.float32(bias)), act)


def conv_reference(fn):
    """reference() for a conv: fn(dtype, seq) -> array or tuple; e32 = the larger of the library float32 evaluation and the strictly
    sequential one (over taps and 16-channel chunks), each against float64.  -> (float64 results, e32 per result)."""
    r64, e_lib = reference(lambda dt: fn(dt, False))
    _, e_seq = reference(lambda dt: fn(dt, True) if dt == np.float32 else tuple(r64) if len(r64) > 1 else r64[0])
    return r64, tuple(max(a, b) for a, b in zip(e_lib, e_seq))


# ---------------------------------------------------------------------------------------------------------------- OP_CHAIN
# One chain record = one launch of chain_kernel or chain_pw2_kernel (csrc/chain.hip).  The blob comes from the compiler's own static
# planner and packer (chains.chain_plan / chains.chain_pack); the record's p[] slots follow ChainMixin._chain_emit and the comment
# above launch_chain.  The cases are tests/chain_cases.py.
def chain_stage(kind, cin, cout, k=1, s=1, act=ir.ACT_NONE, act_a=0.0, act_b=0.0, post_a=1.0, post_b=0.0, res=-1, act2=ir.ACT_NONE,
                gout=-1, shuf=0, wname=None, bias=None):
    """A stage as chains.chain_plan / chain_pack read it: kind "pw" (1x1, stride 1) or "dw" (k x k depthwise, 'same' padding, stride s);
    res = index of the channel-minor buffer the residual comes from (0 = the chain input, j + 1 = the output of stage j); gout = which
    global output the stage stores (-1: none); bias fp32 [cout] (the epilogue's shift; its scale is 1: the weights come folded)."""
    assert kind in ("pw", "dw") and (kind == "pw" or cin == cout)
    ep = dict(act=act, act_a=act_a, act_b=act_b, post_a=post_a, post_b=post_b, act2=act2, scale=np.ones(cout, np.float64),
              shift=np.zeros(cout, np.float32) if bias is None else np.asarray(bias, np.float32))
    return dict(type=kind, k=k, s=s, cin=cin, cout=cout, wname=wname, ep=ep, res_buf=res, res_abs=res, gout=gout, shuf=shuf)


def chain_op(in0, out, tiles, lds_total, nstages, img_bytes, w_off, out2=None, out3=None, pw2=0, lo_in=0, lo_out=(0, 0, 0), wl=(0, 0)):
    """The OP_CHAIN record.  tiles = (tiles_h, tiles_w) of the last stage's output; lds_total = the dynamic LDS bytes of the plan;
    img_bytes = bytes of the blob's LDS image; out3 (the third stored output) rides in the in2 slot; lo_in / lo_out[g] = channel offset of
    the lo half of a hi + lo pair input / output g (0 = plain fp16)."""
    return op(ir.OP_CHAIN, [in0, None, out3], out, out2=out2, w_off=w_off, wl=wl,
              p={ir.P_CH_TILES_H: tiles[0], ir.P_CH_TILES_W: tiles[1], ir.P_CH_LDS: lds_total, ir.P_CH_NSTAGES: nstages,
                 ir.P_CH_NBUFS: nstages + 1, ir.P_CH_PW2: pw2, ir.P_CH_IMG: img_bytes, ir.P_CH_LO_IN: lo_in,
                 ir.P_CH_LO_OUT0: lo_out[0], ir.P_CH_LO_OUT1: lo_out[1], ir.P_CH_LO_OUT2: lo_out[2]})


def chain_form(r):
    """("pw2", blocks) | ("generic", blocks per CU): the conditions of launch_chain, restated (vse_op_kernel_name answers "chain_kernel" for
    every OP_CHAIN record).  chain_pw2_kernel: P_CH_PW2, two stages, an LDS image of at most 64 KiB, at most 64 input channels."""
    r = r[0] if r.ndim else r
    p = r["p"]
    if int(p[ir.P_CH_PW2]) == 1 and int(p[ir.P_CH_NSTAGES]) == 2 and 0 < int(p[ir.P_CH_IMG]) <= 64 * 1024 and int(r["in0"]["c"]) <= 64:
        return "pw2", (int(r["in0"]["n"]) * int(r["in0"]["h"]) * int(r["in0"]["w"]) + 255) // 256
    return "generic", max(1, min(3, (160 * 1024) // (int(p[ir.P_CH_LDS]) + 2048)))


def chain_grid(r, n_cu):
    """Blocks launch_chain starts for a record of the generic kernel on a device of n_cu compute units, and the tiles they share."""
    r = r[0] if r.ndim else r
    tiles = int(r["in0"]["n"]) * int(r["p"][ir.P_CH_TILES_H]) * int(r["p"][ir.P_CH_TILES_W])
    grid = min(tiles, n_cu * chain_form(r)[1])
    return (grid & ~7 if grid > 8 else grid), tiles


def pair64(v):
    """What an fp16 hi + lo pair keeps of a value, in float64 (the kernel splits the fp32 value: hi = fp16(v), lo = fp16(v - hi))."""
    v = np.asarray(v, np.float64)
    hi = v.astype(np.float16).astype(np.float64)
    return hi + (v - hi).astype(np.float16).astype(np.float64)


def ref_chain_stage(bufs, st, dt):
    """One stage on the list of buffers so far ([n,h,w,c] arrays of dtype dt; buffer 0 = the chain input).  st: a chain_stage dict with
    st["w_ref"] = the weights the kernel sees (1x1: float64 [cout][cin] = f16(w) + f16(w - f16(w)); depthwise: fp32 [k * k][c]) and the
    fp32 bias st["ep"]["shift"]."""
    ep, x = st["ep"], bufs[-1]
    f32 = lambda v: dt(np.float32(v))          # noqa: E731
    if st["type"] == "pw":
        y = np.matmul(x, np.asarray(st["w_ref"]).astype(dt).T) + ep["shift"].astype(dt)
        y = ref_act(y, ep["act"], ep["act_a"], ep["act_b"]) * f32(ep["post_a"]) + f32(ep["post_b"])
    else:
        k, s = st["k"], st["s"]
        y = ref_dwconv(x, st["w_ref"], ep["shift"], (k, k), (s, s), (k // 2, k // 2), ep["act"], ep["act_a"], ep["act_b"], ep["post_a"],
                       ep["post_b"], dt=dt)
    if st["res_buf"] >= 0:
        y = ref_act(y + bufs[st["res_buf"]], ep["act2"])
    assert y.dtype == dt
    return y


def ref_chain(x, stages, dt=np.float64, pair=False):
    """The whole chain, plainly: no tiles, no emulator.  x [n,h,w,c] float64 (a pair input: hi + lo summed).  Nothing is rounded between
    the stages — unless pair: then every channel-minor intermediate (a stage output a 1x1 stage reads) passes through the hi + lo
    rounding of the kernel's LDS buffers (evaluated in float64: the term e_pair of the bound).  -> [x, y_1, .., y_n]."""
    bufs = [np.asarray(x).astype(dt)]
    for j, st in enumerate(stages):
        y = ref_chain_stage(bufs, st, dt)
        if pair and j + 1 < len(stages) and stages[j + 1]["type"] == "pw":
            y = pair64(y).astype(dt)
        bufs.append(y)
    return bufs


def ref_shuffle(y):
    """The pixel-shuffle store of a 16-channel stage: channel 4 r + c of input pixel (y, x) -> pixel (4 y + r, 4 x + c) of [n,4h,4w,1]."""
    n, h, w, c = y.shape
    assert c == 16
    return y.reshape(n, h, w, 4, 4).transpose(0, 1, 3, 2, 4).reshape(n, 4 * h, 4 * w, 1)
