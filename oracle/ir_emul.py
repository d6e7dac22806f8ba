"""ORACLE-SIDE TEST INFRASTRUCTURE — CPU emulator of the engine program (ir.OP_DT records).

Only tests/ may import this.  It executes a compiled `Program` op by op with numpy/torch on the CPU so that
the *graph compiler* (BN folding, fusion, concat placement, channel padding, weight tiling, buffer
allocation, attention matching) can be validated against oracle/net_ref.py without a GPU.  It doubles as
the executable specification of what each HIP kernel must compute.  It is never used by the product path:
vse_amd.engine refuses to run without the HIP library.

Arithmetic: activations are held in fp32 unless `round_f16=True`, in which case every op output is rounded
to fp16 exactly where the HIP kernels store fp16 (useful to predict the fp16 error budget).
"""
import numpy as np
import torch
import torch.nn.functional as F

import importlib
ir = importlib.import_module("vse_amd.ir")


def _act(x, code, a=0.0, b=0.0):
    if code == ir.ACT_NONE:
        return x
    if code == ir.ACT_RELU:
        return torch.relu(x)
    if code == ir.ACT_HSWISH:
        return x * torch.clamp(x + 3.0, 0.0, 6.0) / 6.0
    if code == ir.ACT_SWISH:
        return x * torch.sigmoid(x)
    if code == ir.ACT_SIGMOID:
        return torch.sigmoid(x)
    if code == ir.ACT_HSIGMOID:
        return torch.clamp(x * a + b, 0.0, 1.0)
    raise ValueError(code)


class Emulator:
    def __init__(self, prog, round_f16=False, round_ops=None):
        """round_ops (with round_f16=False): indices of the ops whose fp16 OUTPUTS are rounded to fp16 while everything else stays
        fp32 — which stored tensors' rounding moves a result (tools/act_rounding_study.py)."""
        self.prog = prog
        self.round = round_f16
        self.round_ops = set(round_ops) if round_ops is not None else None
        self.cur_op = -1
        # round_f16: byte-exact fp16 workspace.  otherwise: fp32 shadow with one float per 2 bytes.
        # poisoned with NaN: pad channels / stale buffers must never leak into results
        if round_f16:
            self.ws = np.zeros(prog.ws_bytes, dtype=np.uint8)
            self.ws.view(np.uint16)[:] = 0x7E00
        else:
            self.ws = np.full(prog.ws_bytes // 2 + 2, np.nan, dtype=np.float32)
        self.wblob = prog.weights.array()
        self.ext = {}

    # ---- view access -------------------------------------------------------------------------------
    def _arena(self, v):
        a = int(v["arena"])
        if a == ir.ARENA_WS:
            return self.ws
        if a == ir.ARENA_W:
            return self.wblob
        return self.ext[a - ir.ARENA_EXT0]

    def _shadow(self, v):
        return (not self.round) and int(v["arena"]) == ir.ARENA_WS

    def read(self, v):
        """-> float32 torch tensor [n,h,w,c]"""
        n, h, w, c, ld, es = (int(v[k]) for k in ("n", "h", "w", "c", "ld", "esize"))
        arena = self._arena(v)
        if self._shadow(v):
            st = es // 2
            idx = int(v["off"]) // 2 + (np.arange(n * h * w)[:, None] * ld + np.arange(c)[None, :]) * st
            return torch.from_numpy(arena[idx].reshape(n, h, w, c).copy())
        dt = np.float16 if es == 2 else np.float32
        base = int(v["off"])
        cnt = (n * h * w - 1) * ld + c
        flat = arena[base:base + cnt * es].view(dt)
        idx = (np.arange(n * h * w)[:, None] * ld + np.arange(c)[None, :])
        return torch.from_numpy(flat[idx].astype(np.float32).reshape(n, h, w, c))

    def masked(self, t):
        """Ragged plans: what every producing kernel does — zeros right of each sample's own output width."""
        if getattr(self, "wl_out", None) is None:
            return t
        t = t.clone()
        for n, wn in enumerate(self.wl_out):
            t[n, :, int(wn):] = 0
        return t

    def per_sample(self, x, fn):
        """Ragged plans: ops whose window / span is clipped to the sample (pooling, global pool, attention, LSTM) are evaluated
        on each sample's own slice [.., :width_in] and written left-aligned into a zero tensor of the output's shape."""
        if getattr(self, "wl_in", None) is None:
            return fn(x)
        outs = [fn(x[n:n + 1, :, :int(wn)]) for n, wn in enumerate(self.wl_in)]
        wmax = max(o.shape[2] for o in outs)
        full = torch.zeros((x.shape[0], outs[0].shape[1], wmax, outs[0].shape[3]), dtype=outs[0].dtype)
        for n, o in enumerate(outs):
            full[n, :, :o.shape[2]] = o[0]
        return full

    def write(self, v, t, as_int=False):
        n, h, w, c, ld, es = (int(v[k]) for k in ("n", "h", "w", "c", "ld", "esize"))
        if t.shape[2] < w:          # per_sample(): the widest sample of the batch is narrower than the tensor
            t = F.pad(t, (0, 0, 0, w - t.shape[2]))
        t = self.masked(t)
        arena = self._arena(v)
        arr = t.detach().numpy().reshape(n * h * w, c)
        if self._shadow(v):
            st = es // 2
            idx = int(v["off"]) // 2 + (np.arange(n * h * w)[:, None] * ld + np.arange(c)[None, :]) * st
            if self.round_ops is not None and es == 2 and self.cur_op in self.round_ops:
                arr = arr.astype(np.float16).astype(np.float32)
            arena[idx] = arr
            return
        dt = np.float16 if es == 2 else np.float32
        base = int(v["off"])
        cnt = (n * h * w - 1) * ld + c
        flat = arena[base:base + cnt * es].view(dt)
        idx = (np.arange(n * h * w)[:, None] * ld + np.arange(c)[None, :])
        flat[idx] = arr.astype(dt)

    def write_pair(self, v, lo_off, t):
        """write() of an fp16 hi + lo pair tensor (Buf.lo_off): the lo half lo_off channels behind the hi half.  The fp32 shadow
        keeps the whole value in the hi half (a pair carries ~22 bits) and a zero lo; the byte-exact mode splits like the kernels."""
        if not lo_off:
            return self.write(v, t)
        lv = v.copy()
        lv["off"] = int(lv["off"]) + lo_off * int(lv["esize"])
        if self.round:
            hi = t.half().float()
            self.write(v, hi)
            self.write(lv, t - hi)
        else:
            self.write(v, t)
            self.write(lv, torch.zeros_like(t))

    def wread(self, off, count, dt):
        return self.wblob[off:off + count * np.dtype(dt).itemsize].view(dt)

    # ---- run -----------------------------------------------------------------------------------------
    def run(self, x_nhwc8, widths=None):
        """x: float array [N,H,W,8] (fp16-representable).  Returns list of output arrays.
        widths: per-sample input widths of a ragged plan (compile_model(ragged=True)); x must be zero right of them."""
        prog = self.prog
        self.wtab = None
        if prog.wlevels is not None:
            self.wtab = prog.width_table(widths if widths is not None else [x_nhwc8.shape[2]] * x_nhwc8.shape[0])
            for n, wn in enumerate(self.wtab[0]):
                assert not np.asarray(x_nhwc8)[n, :, wn:].any(), "ragged input must be zero right of the sample's width"
        else:
            assert widths is None
        self.ext[0] = np.ascontiguousarray(x_nhwc8.astype(np.float16)).view(np.uint8).reshape(-1)
        for k, o in enumerate(prog.outputs):
            self.ext[k + 1] = np.zeros(o["n"] * o["h"] * o["w"] * o["ld"] * o["esize"], dtype=np.uint8)
        self._run_ops()
        outs = []
        for k, o in enumerate(prog.outputs):
            outs.append(self.ext[k + 1].view(np.float32).reshape(o["n"], o["h"], o["w"], o["ld"]).copy())
        return outs

    def _run_ops(self):
        for k, r in enumerate(self.prog.ops):
            self.cur_op = k
            self.wl_in = self.wl_out = None
            if self.wtab is not None:
                if int(r["p"][ir.P_WLIN]):
                    self.wl_in = self.wtab[int(r["p"][ir.P_WLIN]) - 1]
                if int(r["p"][ir.P_WLOUT]):
                    self.wl_out = self.wtab[int(r["p"][ir.P_WLOUT]) - 1]
            getattr(self, "_op%d" % int(r["kind"]))(r)

    def run_records(self, ext, wtab=None):
        """The records of `prog.ops` on caller-owned external arenas, the way vse_plan_run_ragged takes them: ext[k] = the byte
        image (any numpy array) of arena ir.ARENA_EXT0 + k, inputs and outputs alike; wtab = the int32 width table [levels][n] (None
        for an ordinary plan).  Needs the byte-exact mode (round_f16=True); prog may be any object with ops, ws_bytes and
        weights.array() (tests/op_harness.py runs single records this way).  -> the arenas after the run, as uint8 arrays."""
        assert self.round, "external arenas are byte images: round_f16=True"
        self.ext = {k: np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy() for k, a in enumerate(ext)}
        self.wtab = None if wtab is None else np.asarray(wtab, np.int32)
        self._run_ops()
        return [self.ext[k] for k in range(len(ext))]

    @staticmethod
    def _up(t, shift):
        if shift == 0:
            return t
        s = 1 << shift
        return t.repeat_interleave(s, dim=1).repeat_interleave(s, dim=2)

    def _op14(self, r):  # CHAIN (csrc/chain.hip): decoded from the blob the kernel reads — descriptor words, MFMA fragments, dw tables
        off = int(r["w_off"])
        hdr = self.wread(off, ir.CH_HDR, np.int32)
        assert int(hdr[ir.CHH_MAGIC]) == ir.CH_MAGIC
        n, nb = int(hdr[ir.CHH_NSTAGES]), int(hdr[ir.CHH_NBUFS])
        bw = self.wread(off + 4 * ir.CH_HDR, nb * ir.CH_BUF, np.int32).reshape(nb, ir.CH_BUF)
        sw = self.wread(off + 4 * (ir.CH_HDR + nb * ir.CH_BUF), n * ir.CH_STAGE, np.int32).reshape(n, ir.CH_STAGE)
        img = off + int(hdr[ir.CHH_LDSIMG_OFF])
        assert int(hdr[ir.CHH_LDS_TOTAL]) <= 160 * 1024 and int(r["p"][ir.P_CH_LDS]) == int(hdr[ir.CHH_LDS_TOTAL])

        def i2f(v):
            return float(np.asarray([v], np.int32).view(np.float32)[0])

        def pair(t):          # what a hi + lo fp16 pair keeps of an fp32 value
            if not self.round:
                return t
            hi = t.half().float()
            return hi + (t - hi).half().float()
        x = self.read(r["in0"])
        lo_in = int(r["p"][ir.P_CH_LO_IN])
        if lo_in:
            v = r["in0"].copy()
            v["off"] = int(v["off"]) + lo_in * int(v["esize"])
            x = x + self.read(v)
        assert x.shape[3] >= int(bw[0, ir.CHB_C])
        bufs = {0: x[..., :int(bw[0, ir.CHB_C])].permute(0, 3, 1, 2).contiguous()}
        gviews = [r["out"], r["out2"], r["in2"]]
        lane = np.arange(64)
        rows = np.array([(f & ~12) | ((f & 4) << 1) | ((f & 8) >> 1) for f in lane & 31])
        for j in range(n):
            s = sw[j]
            xin = bufs[int(s[ir.CHS_IN])]
            cin, cout, k, st = int(s[ir.CHS_CIN]), int(s[ir.CHS_COUT]), int(s[ir.CHS_K]), int(s[ir.CHS_S])
            assert xin.shape[1] == cin
            if int(s[ir.CHS_TYPE]) == ir.CH_PW:
                nks, nct = int(s[ir.CHS_NKS]), int(s[ir.CHS_NCT])
                fr = self.wread(img + int(s[ir.CHS_WLDS]), 2 * nct * nks * 512, np.float16).astype(np.float64).reshape(2, nct, nks, 64, 8)
                wm = np.zeros((nct * 32, nks * 16), np.float64)
                for ct in range(nct):
                    for ks in range(nks):
                        k0 = ks * 16 + 8 * (lane >> 5)
                        wm[(ct * 32 + rows)[:, None], k0[:, None] + np.arange(8)[None, :]] = fr[0, ct, ks] + fr[1, ct, ks]
                assert not wm[cout:].any() and not wm[:, cin:].any()
                bias = self.wread(img + int(s[ir.CHS_BLDS]), nct * 32, np.float32).astype(np.float64)
                y = F.conv2d(xin.double(), torch.from_numpy(wm[:cout, :cin].copy()).reshape(cout, cin, 1, 1), torch.from_numpy(bias[:cout].copy())).float()
            else:
                nrec = (k * k + 1 + 3) // 4 * 4                 # per-channel record: k*k weights, bias, padding
                rec = self.wread(img + int(s[ir.CHS_WLDS]), cin * nrec, np.float32).reshape(cin, nrec)
                assert not rec[:, k * k + 1:].any()
                wk, bk = rec[:, :k * k].reshape(cin, 1, k, k), rec[:, k * k]
                y = F.conv2d(xin, torch.from_numpy(wk.copy()), torch.from_numpy(bk.copy()), st, int(s[ir.CHS_PAD]), groups=cin)
            y = _act(y, int(s[ir.CHS_ACT]), i2f(s[ir.CHS_ACT_A]), i2f(s[ir.CHS_ACT_B]))
            y = y * i2f(s[ir.CHS_POST_A]) + i2f(s[ir.CHS_POST_B])
            if int(s[ir.CHS_RES]) >= 0:
                y = _act(y + bufs[int(s[ir.CHS_RES])], int(s[ir.CHS_ACT2]))
            ob = bw[int(s[ir.CHS_OUT])]
            assert (int(ob[ir.CHB_KIND]) == 2) == (j == n - 1)
            # the tile geometry the kernel walks: a stage's input region must be exactly what its output region needs
            ib = bw[int(s[ir.CHS_IN])]
            pad_ = int(s[ir.CHS_PAD]) if int(s[ir.CHS_TYPE]) == ir.CH_DW else 0
            for T, A, E in ((ir.CHB_TH, ir.CHB_AH, ir.CHB_EH), (ir.CHB_TW, ir.CHB_AW, ir.CHB_EW)):
                assert int(ib[T]) == int(ob[T]) * st and int(ib[A]) == int(ob[A]) * st + pad_, (j, "tile / halo")
                assert int(ib[E]) == (int(ob[E]) - 1) * st + k, (j, "extent")
            assert int(ob[ir.CHB_P]) == int(ob[ir.CHB_EH]) * int(ob[ir.CHB_EW])
            if int(ob[ir.CHB_KIND]) != 2:
                assert int(ob[ir.CHB_C]) == cout and (int(ob[ir.CHB_HIMG]), int(ob[ir.CHB_WIMG])) == tuple(y.shape[2:])
                bufs[int(s[ir.CHS_OUT])] = pair(y) if int(ob[ir.CHB_KIND]) == 0 else y
            g = int(s[ir.CHS_GOUT])
            if g >= 0 and int(s[ir.CHS_SHUF]):
                # channel 4 r + c of input pixel (y, x) = pixel (4 y + r, 4 x + c) of the 1-channel fp32 map
                nb_, _c16, hh, ww = y.shape
                assert _c16 == 16
                m = y.reshape(nb_, 4, 4, hh, ww).permute(0, 3, 1, 4, 2).reshape(nb_, 4 * hh, 4 * ww, 1)
                self.write(gviews[g], m)
            elif g >= 0:
                # the kernel stores the stage's channels that lie inside the view (8-channel runs c0 < min(cout, view c)) and nothing else:
                # a view wider than the stage keeps what it held behind them
                gv = gviews[g].copy()
                gv["c"] = min(int(gv["c"]), cout)
                self.write_pair(gv, int(r["p"][ir.P_CH_LO_OUT0 + g]), y.permute(0, 2, 3, 1)[..., :int(gv["c"])])

    def conv_wmat(self, r, kh=None, kw=None):
        """The weight matrix [Np][kh * kw * cinp] (K in (tap, channel) order, hi + lo summed) decoded from the stream of an OP_CONV record,
        whatever family it was packed for (not F_UP2HEAD: folded taps).  kh, kw: the conv's own (1, 1 behind an F_DWPRE depthwise conv)."""
        p = r["p"]
        kh, kw = (int(p[0]) if kh is None else kh), (int(p[1]) if kw is None else kw)
        Np, Kp, cinp = int(p[ir.P_COUT]), int(p[ir.P_KTOT]), int(p[ir.P_CINP])
        KT = ir.KT
        if int(r["flags"]) & ir.F_PW:
            assert (kh, kw) == (1, 1) and Kp == (cinp + 15) // 16 * 16
            wmat = self.wread(int(r["w_off"]), Np * Kp, np.float16).astype(np.float32).reshape(Np, Kp)
            if int(r["flags"]) & ir.F_HILO:           # w = hi + lo (the lo table follows the hi table)
                wmat = wmat + self.wread(int(r["w_off"]) + 2 * Np * Kp, Np * Kp, np.float16).astype(np.float32).reshape(Np, Kp)
            assert not wmat[:, cinp:].any()
            wmat = wmat[:, :cinp]
        elif int(r["flags"]) & ir.F_COL and int(r["flags"]) & ir.F_HLSUM:
            # 64-row stages [hi 32 | lo 32]: w = hi + lo (the kernel adds the two accumulator tiles)
            assert cinp % 16 == 0 and Kp == kh * kw * cinp and Np <= 32 and (kh, kw) == (3, 3) and not int(r["flags"]) & ir.F_HILO
            wt = self.wread(int(r["w_off"]), Kp * 64 + 3 * kh * 64 * 16, np.float16).astype(np.float32)
            assert not wt[Kp * 64:].any()
            w64 = np.ascontiguousarray(wt[:Kp * 64].reshape(cinp // 16, kw, kh, 64, 16).transpose(3, 2, 1, 0, 4)).reshape(64, Kp)
            wmat = (w64[:32] + w64[32:])[:Np]
        elif int(r["flags"]) & ir.F_COL:
            assert cinp % 16 == 0 and Kp == kh * kw * cinp
            npass = 2 if int(r["flags"]) & ir.F_HILO else 1          # w = hi + lo (the lo stream follows the hi stream)
            wt = self.wread(int(r["w_off"]), npass * Kp * Np + 3 * kh * Np * 16, np.float16).astype(np.float32)
            assert not wt[npass * Kp * Np:].any()           # the three zero stages of the DMA look-ahead
            ws = wt[:Kp * Np] + wt[Kp * Np:2 * Kp * Np] if npass == 2 else wt[:Kp * Np]      # (no '+ 0.0': a -0 weight stays -0)
            wmat = np.ascontiguousarray(ws.reshape(cinp // 16, kw, kh, Np, 16).transpose(3, 2, 1, 0, 4)).reshape(Np, Kp)
        elif int(r["flags"]) & ir.F_PATCH:
            taps = kh * kw
            c32 = (cinp + 31) // 32 * 32
            tp = Kp // c32                                  # taps padded to whole kernel steps by the compiler
            wt = self.wread(int(r["w_off"]), tp * c32 * Np, np.float16).astype(np.float32)
            wfull = wt.reshape(c32 // 32, tp, Np, 32).transpose(2, 1, 0, 3).reshape(Np, tp, c32)
            assert not wfull[:, taps:].any() and not wfull[:, :, cinp:].any()
            row_major = [(t % kw) * kh + t // kw for t in range(taps)]     # stream is column-major: t' = dx*kh + dy
            wmat = np.ascontiguousarray(wfull[:, :taps, :cinp][:, row_major, :]).reshape(Np, taps * cinp)
        elif int(r["flags"]) & ir.F_STEM:
            wt = self.wread(int(r["w_off"]), Np * 80, np.float16).astype(np.float32)
            if int(r["flags"]) & ir.F_HILO:
                wt = wt + self.wread(int(r["w_off"]) + 2 * Np * 80, Np * 80, np.float16).astype(np.float32)
            wt = wt.reshape(Np, 10, 8)
            assert not wt[:, 9:].any() and not wt[:, :, 4:].any() and (kh, kw, cinp) == (3, 3, 8)
            wmat = np.ascontiguousarray(wt[:, :9]).reshape(Np, 72)
        else:
            kt = 32 if int(r["flags"]) & ir.F_WK32 else KT
            cnt = (Kp // kt) * Np * kt
            wt = self.wread(int(r["w_off"]), cnt, np.float16).astype(np.float32)
            if int(r["flags"]) & ir.F_HILO:           # w = hi + lo (the lo tiles follow the hi tiles)
                wt = wt + self.wread(int(r["w_off"]) + 2 * cnt, cnt, np.float16).astype(np.float32)
            wmat = wt.reshape(Kp // kt, Np, kt).transpose(1, 0, 2).reshape(Np, Kp)[:, :kh * kw * cinp]
        return wmat

    def _op1(self, r):   # CONV
        p, f = r["p"], r["f"]
        kh, kw, sh, sw, ph, pw = (int(p[i]) for i in range(6))
        Np, Kp, cinp = int(p[ir.P_COUT]), int(p[ir.P_KTOT]), int(p[ir.P_CINP])
        v0 = r["in0"]
        if int(r["flags"]) & ir.F_UP2HEAD and int(v0["ld"]) == 1:
            # the dense 1-channel map of an F_TAIL2 conv (nominal span 8, ld = 1): the head reads channel 0 at pixel stride 1
            v0 = v0.copy()
            v0["c"] = 1
            x = F.pad(self.read(v0), (0, 7))
        else:
            x = self._up(self.read(v0), int(p[ir.P_INSHIFT]))
        if int(r["flags"]) & ir.F_SRC2:
            x = torch.cat([x, self._up(self.read(r["in2"]), int(p[ir.P_IN2SHIFT]))], dim=3)
        assert x.shape[3] == cinp
        KT = ir.KT
        if int(r["flags"]) & ir.F_UP2HEAD:
            # folded weights: [2 chunks][4 parities][4 taps][64][32] + u block [64][32]; evaluate per output parity on
            # the low-res grid exactly as conv_head_up2_kernel does, then fall through to the common epilogue
            wt = self.wread(int(r["w_off"]), 2 * 4 * 4 * 64 * 32 + 64 * 32, np.float16).astype(np.float32)
            wx = wt[:2 * 4 * 4 * 64 * 32].reshape(2, 4, 4, 64, 32)
            wu = torch.from_numpy(wt[2 * 4 * 4 * 64 * 32:].reshape(64, 32)[:Np, :9].reshape(Np, 1, 3, 3).copy())
            xl = self.read(r["in2"]).permute(0, 3, 1, 2)                      # [n,64,Hl,Wl]
            u = x[..., 0:1].permute(0, 3, 1, 2)                              # [n,1,2Hl,2Wl]
            n, _, Hl, Wl = xl.shape
            y = F.conv2d(u, wu, None, 1, 1)                                   # [n,Np,2Hl,2Wl]
            xp = F.pad(xl, (1, 1, 1, 1))
            for a_ in range(2):
                for b_ in range(2):
                    wk = np.concatenate([wx[0, a_ * 2 + b_], wx[1, a_ * 2 + b_]], axis=2)       # [4 taps][64][64 ch]
                    w4 = torch.from_numpy(np.ascontiguousarray(wk.reshape(2, 2, 64, 64).transpose(2, 3, 0, 1))[:Np])
                    z = F.conv2d(xp[:, :, a_:a_ + Hl + 1, b_:b_ + Wl + 1], w4)                     # [n,Np,Hl,Wl]
                    y[:, :, a_::2, b_::2] += z
            bias = torch.from_numpy(self.wread(int(r["b_off"]), Np, np.float32).copy())
            y = (y + bias.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
            y = _act(y, int(p[ir.P_ACT]), float(f[ir.FS_ACT_A]), float(f[ir.FS_ACT_B]))
            y = y * float(f[ir.FS_POST_A]) + float(f[ir.FS_POST_B])
            y = _act(y, int(p[ir.P_ACT2]))
            dw = torch.from_numpy(self.wread(int(r["aux_off"]), Np, np.float32).copy())
            z = (y * dw).sum(-1, keepdim=True) + float(f[ir.FS_PRE_B])
            z = _act(z, int(p[ir.P_DOTACT]))
            oc2 = int(r["out2"]["c"])
            self.write(r["out2"], z if oc2 == 1 else F.pad(z, (0, oc2 - 1)))
            return
        if int(r["flags"]) & ir.F_DWPRE:
            # depthwise conv in front of the 1x1 conv (csrc/conv_dwpw.hip): decoded from the aux blob; the 1x1 part below is a plain F_PW conv
            assert int(r["flags"]) & ir.F_PW and int(r["flags"]) & ir.F_HILO and kh == kw and sh == sw and ph == pw
            hdr = self.wread(int(r["aux_off"]), 8, np.float32)
            hi_ = hdr.view(np.int32)
            assert (int(hi_[0]), int(hi_[1]), int(hi_[2])) == (kh, sh, ph)
            tab = self.wread(int(r["aux_off"]) + 32, (kh * kw + 1) * Kp, np.float32).reshape(kh * kw + 1, Kp)
            if int(p[ir.P_LO_IN]):                # the input is an fp16 hi + lo pair
                lv = r["in0"].copy()
                lv["off"] = int(lv["off"]) + int(p[ir.P_LO_IN]) * int(lv["esize"])
                x = x + self.read(lv)
            wd = torch.from_numpy(np.ascontiguousarray(tab[:kh * kw, :cinp].T.reshape(cinp, 1, kh, kw)))
            xd = F.conv2d(x.permute(0, 3, 1, 2), wd, torch.from_numpy(tab[kh * kw, :cinp].copy()), (sh, sw), (ph, pw), groups=cinp)
            xd = _act(xd, int(hi_[3]), float(hdr[4]), float(hdr[5])) * float(hdr[6]) + float(hdr[7])
            x = xd.permute(0, 2, 3, 1)            # (the kernel keeps this as an fp16 hi + lo pair in registers: ~fp32)
            kh = kw = sh = sw = 1
            ph = pw = 0
        wmat = self.conv_wmat(r, kh, kw)
        bias = torch.from_numpy(self.wread(int(r["b_off"]), Np, np.float32).copy())
        if int(r["flags"]) & ir.F_IMGW:
            # per-image weights written by OP_WSCALE into the workspace (in2): [N][Kp/kt][Np][kt]
            assert (kh, kw) == (1, 1)
            kt = 32 if int(r["flags"]) & ir.F_WK32 else KT
            wimg = self.read(r["in2"]).reshape(x.shape[0], Kp // kt, Np, kt).permute(0, 2, 1, 3).reshape(x.shape[0], Np, Kp)[:, :, :cinp]
            y = torch.stack([F.conv2d(x[n:n + 1].permute(0, 3, 1, 2), wimg[n].reshape(Np, cinp, 1, 1).float(), bias)[0]
                             for n in range(x.shape[0])]).permute(0, 2, 3, 1)
        else:
            w4 = torch.from_numpy(np.ascontiguousarray(wmat.reshape(Np, kh, kw, cinp).transpose(0, 3, 1, 2)))
            y = F.conv2d(x.permute(0, 3, 1, 2), w4, bias, (sh, sw), (ph, pw)).permute(0, 2, 3, 1)
        y = _act(y, int(p[ir.P_ACT]), float(f[ir.FS_ACT_A]), float(f[ir.FS_ACT_B]))
        y = y * float(f[ir.FS_POST_A]) + float(f[ir.FS_POST_B])
        flags = int(r["flags"])
        if flags & ir.F_OGATE:                       # SE block with shortcut folded into the conv: y * (1 + gate[n, c])
            assert not (flags & (ir.F_SRC2 | ir.F_IMGW | ir.F_PIXSHUF))
            y = y * (1.0 + self.read(r["in2"])[..., :Np].reshape(y.shape[0], 1, 1, Np))
        if flags & ir.F_PIXSHUF:
            n, h, w, _ = y.shape
            cp = Np // 4
            y = y.reshape(n, h, w, 2, 2, cp).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, cp)
        if flags & ir.F_RES:
            res = self._up(self.read(r["in1"]), int(p[ir.P_RESSHIFT]))[:, :y.shape[1], :y.shape[2]]      # (odd maps: the last row / column of a pair)
            if int(p[ir.P_LO_RES]):           # the residual is an fp16 hi + lo pair
                lv = r["in1"].copy()
                lv["off"] = int(lv["off"]) + int(p[ir.P_LO_RES]) * int(lv["esize"])
                res = res + self.read(lv)[:, :y.shape[1], :y.shape[2]]
            y[..., :res.shape[3]] += res[..., :y.shape[3]]
        y = _act(y, int(p[ir.P_ACT2]))
        if flags & ir.F_DOT1:
            dw = torch.from_numpy(self.wread(int(r["aux_off"]), Np, np.float32).copy())
            z = (y * dw).sum(-1, keepdim=True) + float(f[ir.FS_PRE_B])
            z = _act(z, int(p[ir.P_DOTACT]))
            oc2 = int(r["out2"]["c"])
            self.write(r["out2"], z if oc2 == 1 else F.pad(z, (0, oc2 - 1)))   # pad channels (if any) are written as 0
            return
        oc = int(r["out"]["c"])
        self.write_pair(r["out"], int(p[ir.P_LO_OUT]), y[..., :oc] if y.shape[3] >= oc else F.pad(y, (0, oc - y.shape[3])))
        if flags & ir.F_TAIL2:
            # the second 2x2 s2 transposed conv (-> ONE channel) on the fp16 values just stored (csrc/conv_pw.hip, conv_pw_tail_kernel):
            # decoded from stage B's MFMA fragments [Np / 16][2][16][8] — a block-diagonal [16][Np] matrix, row 4 r + c, column
            # (2 dy + dx) * cp + co, non-zero where (r >> 1, c >> 1) = (dy, dx), value w2[co][r & 1][c & 1] in every block
            assert flags & ir.F_PW and flags & ir.F_PIXSHUF and not flags & (ir.F_HILO | ir.F_RES | ir.F_DOT1) and Np % 32 == 0
            cp, nks2 = Np // 4, Np // 16
            fr = self.wread(int(r["aux_off"]), nks2 * 2 * 16 * 8, np.float16).astype(np.float32).reshape(nks2, 2, 16, 8)
            fx = np.arange(16)
            rows = (fx & ~12) | ((fx & 4) << 1) | ((fx & 8) >> 1)
            wb = np.zeros((16, Np), np.float32)
            for s_ in range(nks2):
                for fj in range(2):
                    wb[rows, s_ * 16 + fj * 8:s_ * 16 + fj * 8 + 8] = fr[s_, fj]
            w2 = np.zeros((cp, 1, 2, 2), np.float32)
            for r_ in range(4):
                for c_ in range(4):
                    q = ((r_ >> 1) * 2 + (c_ >> 1)) * cp
                    blk = wb[4 * r_ + c_].copy()
                    if q == 0:
                        w2[:, 0, r_ & 1, c_ & 1] = blk[:cp]
                    assert np.array_equal(blk[q:q + cp], w2[:, 0, r_ & 1, c_ & 1]), "stage B is not the same 2x2 filter in every sub-pixel block"
                    blk[q:q + cp] = 0
                    assert not blk.any(), "stage B is not block-diagonal"
            yf = y.half().float() if self.round else y
            z = F.conv_transpose2d(yf.permute(0, 3, 1, 2), torch.from_numpy(w2), stride=2).permute(0, 2, 3, 1) + float(f[ir.FS_PRE_B])
            z = _act(z, int(p[ir.P_DOTACT]))
            v2 = r["out2"].copy()
            assert int(v2["ld"]) == 1 and int(v2["esize"]) == 2
            v2["c"] = 1
            self.write(v2, z)

    def _op2(self, r):   # DWCONV
        p, f = r["p"], r["f"]
        kh, kw, sh, sw, ph, pw = (int(p[i]) for i in range(6))
        x = self.read(r["in0"])
        if int(p[ir.P_LO_RES]):               # the input is an fp16 hi + lo pair
            lv = r["in0"].copy()
            lv["off"] = int(lv["off"]) + int(p[ir.P_LO_RES]) * int(lv["esize"])
            x = x + self.read(lv)
        if int(r["flags"]) & ir.F_GATE:       # SE gate applied on load, rounded to fp16 like the separate scale pass
            g = self.read(r["in1"])
            x = ((x * g + x) if int(r["flags"]) & ir.F_RES else x * g).half().float()
        cp = x.shape[3]
        wk = self.wread(int(r["w_off"]), kh * kw * cp, np.float32).copy()        # fp32 [kh * kw][cp] (hi + lo summed by the compiler)
        wk = wk.reshape(kh, kw, cp)
        w4 = torch.from_numpy(np.ascontiguousarray(wk.transpose(2, 0, 1)[:, None]))
        bias = torch.from_numpy(self.wread(int(r["b_off"]), cp, np.float32).copy())
        y = F.conv2d(x.permute(0, 3, 1, 2), w4, bias, (sh, sw), (ph, pw), groups=cp).permute(0, 2, 3, 1)
        y = _act(y, int(p[ir.P_ACT]), float(f[ir.FS_ACT_A]), float(f[ir.FS_ACT_B]))
        y = y * float(f[ir.FS_POST_A]) + float(f[ir.FS_POST_B])
        self.write_pair(r["out"], int(p[ir.P_LO_OUT]), y)

    def _op3(self, r):   # POOL
        p = r["p"]
        kh, kw, sh, sw, ph, pw = (int(p[i]) for i in range(6))
        ceil = bool(p[ir.P_POOL_CEIL])

        def pool(xs):
            xs = xs.permute(0, 3, 1, 2)
            if p[ir.P_POOL_MAX]:
                y = F.max_pool2d(xs, (kh, kw), (sh, sw), (ph, pw), ceil_mode=ceil)
            else:
                y = F.avg_pool2d(xs, (kh, kw), (sh, sw), (ph, pw), ceil_mode=ceil,
                                 count_include_pad=not bool(p[ir.P_POOL_EXCL]))
            return y.permute(0, 2, 3, 1)
        self.write(r["out"], self.per_sample(self.read(r["in0"]), pool))

    def _op4(self, r):   # GAP
        x = self.read(r["in0"])
        self.write(r["out"], self.per_sample(x, lambda xs: xs.mean((1, 2), keepdim=True)))

    def _op5(self, r):   # SCALE
        x = self.read(r["in0"])
        s = self.read(r["in1"])
        y = x * s
        if int(r["flags"]) & ir.F_RES:
            y = y + x
        self.write(r["out"], y)

    def _op6(self, r):   # BINARY
        p = r["p"]
        x = self.read(r["in0"])
        y = self._up(self.read(r["in1"]), int(p[ir.P_BIN_SHIFT]))
        z = x * y if p[ir.P_BIN_MUL] else x + y
        self.write(r["out"], _act(z, int(p[ir.P_BIN_ACT])))

    def _op7(self, r):   # RESIZE
        x = self._up(self.read(r["in0"]), int(r["p"][0]))
        oc = int(r["out"]["c"])
        flags = int(r["flags"])
        if flags & (ir.F_GATE | ir.F_SRC2):      # gated form: up(x) * (1 + gate) (F_RES) per source; F_SRC2: a second source beside it
            def gated(t, gview):
                if not (flags & ir.F_GATE):
                    return t
                g = self.read(gview)[..., :t.shape[3]]
                return t * ((1.0 if flags & ir.F_RES else 0.0) + g)
            parts = [gated(x, r["in1"])]
            if flags & ir.F_SRC2:
                parts.append(gated(self._up(self.read(r["in2"]), int(r["p"][1])), r["out2"]))
            x = torch.cat(parts, dim=3)
            assert x.shape[3] == oc
        self.write(r["out"], x[..., :oc])

    def _op8(self, r):   # UNARY
        f = r["f"]
        x = self.read(r["in0"])
        oc = int(r["out"]["c"])
        x = x[..., :oc]
        y = _act(x * float(f[ir.FS_PRE_A]) + float(f[ir.FS_PRE_B]), int(r["p"][0]), float(f[ir.FS_ACT_A]),
                 float(f[ir.FS_ACT_B]))
        self.write(r["out"], y * float(f[ir.FS_POST_A]) + float(f[ir.FS_POST_B]))

    def _op9(self, r):   # LAYERNORM
        x = self.read(r["in0"])
        c = x.shape[3]
        gb = self.wread(int(r["w_off"]), 2 * c, np.float32)
        # in float64: fp32 F.layer_norm is 5e-6 .. 9e-6 off on rows with a mean of 30 and a deviation of 0.5 (its one-pass variance
        # cancels), three times what the kernel's two-pass fp32 evaluation is off — the reference must be the more accurate side
        y = F.layer_norm(x.double(), (c,), torch.from_numpy(gb[:c].astype(np.float64)), torch.from_numpy(gb[c:].astype(np.float64)),
                         float(r["f"][ir.FS_EPS]))
        self.write(r["out"], y.float())

    def _op10(self, r):  # ATTN
        heads, hd = int(r["p"][ir.P_HEADS]), int(r["p"][ir.P_HDIM])
        scale = float(r["f"][ir.FS_SCALE])
        def attn(x):                               # [B,1,T,3*C]
            B, _, T, _ = x.shape
            qkv = x.reshape(B, T, 3, heads, hd).permute(2, 0, 3, 1, 4)   # [3,B,h,T,d]
            q, k, v = qkv[0] * scale, qkv[1], qkv[2]
            att = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
            return (att @ v).permute(0, 2, 1, 3).reshape(B, 1, T, heads * hd)
        self.write(r["out"], self.per_sample(self.read(r["in0"]), attn))

    def _op11(self, r):  # SOFTMAX
        ncls = int(r["p"][ir.P_NCLS])
        x = self.read(r["in0"])[..., :ncls]
        pr = torch.softmax(x, dim=-1)
        mx, idx = pr.max(dim=-1)
        n, h, w, _ = x.shape
        out = np.zeros((n, h, w, 2), np.float32)
        out[..., 0] = idx.numpy().astype(np.int32).view(np.float32) if False else 0
        iv = r["out"]
        arena = self._arena(iv)
        base = int(iv["off"])
        raw = arena[base:base + n * h * w * 8].view(np.int32).reshape(n, h, w, 2)
        raw[..., 0] = idx.numpy().astype(np.int32)
        raw[..., 1] = mx.numpy().astype(np.float32).view(np.int32)
        if int(r["out2"]["n"]) > 0:
            self.write(r["out2"], pr)

    def _op12(self, r):  # LSTM recurrence; in0 (/ in1) = fp32 gate pre-activations [B,1,T,4H] of one (/ the reverse) direction
        H = int(r["p"][ir.P_HID])
        mode = int(r["p"][ir.P_REVERSE])
        if int(r["flags"]) & ir.F_LSTM_MFMA:
            # W_hh^T in MFMA fragment order [dir][wave 16][slice 16][tile 2][k-half 2][gate-in-tile 2][unit 16][8] (gate = 2 * tile +
            # gate-in-tile) -> [H, 4H] per direction
            assert H == 256 and int(r["p"][ir.P_WAVES]) == 16
            ndir = 2 if mode == 2 else 1
            wt = self.wread(int(r["w_off"]), ndir * 4 * H * H, np.float16).astype(np.float32).reshape(ndir, 16, 16, 2, 2, 2, 16, 8)
            whhs = [torch.from_numpy(np.ascontiguousarray(wt[d].transpose(2, 4, 0, 5, 1, 3, 6)).reshape(4 * H, H).T.copy()) for d in range(ndir)]
            dirs = [(r["in0"], whhs[0], mode == 1)] + ([(r["in1"], whhs[1], True)] if ndir == 2 else [])
            gorder = np.arange(4 * H).reshape(4, 16, H // 16).transpose(1, 0, 2).reshape(-1)      # stored channel -> (gate, unit)
            unperm = np.argsort(gorder)
        else:
            whh = torch.from_numpy(self.wread(int(r["w_off"]), H * 4 * H, np.float16).astype(np.float32).reshape(H, 4 * H))
            dirs = [(r["in0"], whh, bool(mode))]

        def lstm(g, whh, rev):
            B, _, T, _ = g.shape
            h = torch.zeros(B, H)
            c = torch.zeros(B, H)
            out = torch.zeros(B, 1, T, H)
            for t in (range(T - 1, -1, -1) if rev else range(T)):
                # one matrix-vector product per sample: a sample's column of h . W_hh^T must not depend on the batch it rides in
                # (csrc/lstm.hip), and a batched CPU GEMM sums in an order that changes with B
                z = g[:, 0, t] + torch.stack([h[b] @ whh for b in range(B)])
                i, f_, gg, o = z.chunk(4, dim=1)
                c = torch.sigmoid(f_) * c + torch.sigmoid(i) * torch.tanh(gg)
                h = torch.sigmoid(o) * torch.tanh(c)
                # (both kernels carry fp32-grade state — lstm_kernel h in fp32, the MFMA kernel as fp16 hi + lo — and round only
                # the value they store; write() does that)
                out[:, 0, t] = h
            return out
        def gates_of(v):
            g = self.read(v)
            return g[..., torch.from_numpy(unperm)] if int(r["flags"]) & ir.F_LSTM_MFMA else g        # back to [gate][unit]
        outs = [self.per_sample(gates_of(v), lambda g, w=w, rv=rv: lstm(g, w, rv)) for v, w, rv in dirs]
        self.write(r["out"], torch.cat(outs, dim=3))

    def _op13(self, r):  # WSCALE: per-image 1x1 weights = tiled weight blob x SE gate over k, rounded to fp16 once
        p = r["p"]
        Kp, Np, kt = int(p[0]), int(p[1]), int(p[2])
        w = self.wread(int(r["w_off"]), Kp * Np, np.float16).astype(np.float32).reshape(Kp // kt, Np, kt)
        g = self.read(r["in0"]).float().reshape(-1, int(r["in0"]["c"]))               # [N, C]
        gk = torch.zeros(g.shape[0], Kp)
        gk[:, :g.shape[1]] = g
        out = torch.from_numpy(w).unsqueeze(0) * gk.reshape(-1, Kp // kt, 1, kt)       # [N, Kp/kt, Np, kt]
        self.write(r["out"], out.half().float().reshape(g.shape[0], 1, 1, Kp * Np))


def to_nhwc8(x_nchw):
    """float32 NCHW [N,3,H,W] -> fp16-rounded float NHWC with 8 physical channels."""
    n, c, h, w = x_nchw.shape
    out = np.zeros((n, h, w, 8), np.float32)
    out[..., :c] = np.transpose(np.asarray(x_nchw), (0, 2, 3, 1))
    return out.astype(np.float16).astype(np.float32)
