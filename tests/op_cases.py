"""The cases of tests/test_gpu_ops.py (GPU) and tests/test_op_records.py (the same records on the CPU emulator): per group a generator
of op_harness.Case — seeded inputs, the one-record plan, the kernel form it must select, and a check against the fp64 reference.

Shapes are the smallest that reach each path of csrc/simple_ops.hip and csrc/lstm.hip: tile and vector tails, more than one block, the
thresholds between two kernels.  Every group is a few dozen tiny launches."""
import numpy as np

import op_harness as H
from vse_amd import compiler, ir

def _nan(shape, dt=np.float16):
    return np.full(shape, np.nan, dt)


def _single(name, rec, blob, tensors, check, widths=None, ws_bytes=0, **kw):
    return H.Case(name, [H.Run(rec, blob.array() if isinstance(blob, H.Blob) else blob, tensors, widths, ws_bytes)],
                  lambda outs: check(outs[0]), **kw)


# ================================================================================================================== softmax
# (esize, ncls, ld) -> the form `case OP_SOFTMAX` must select; 3690 / 4401 / 8423 / 6625 = the shipped dictionaries
SOFTMAX = {(2, 97, 104): ("reg", 1), (2, 2049, 2056): ("reg", 2), (2, 3690, 3696): ("reg", 2), (2, 4401, 4408): ("reg", 4),
           (2, 6625, 6632): ("reg", 4), (2, 8423, 8424): ("reg", 8), (2, 16385, 16392): ("scalar", 0),
           (4, 97, 100): ("reg", 1), (4, 1025, 1028): ("reg", 2), (4, 3690, 3692): ("reg", 4), (4, 6625, 6628): ("reg", 8),
           (4, 8423, 8424): ("scalar", 0), (4, 97, 97): ("scalar", 0)}


def softmax_cases(key):
    esize, ncls, ld = key
    dt = np.float16 if esize == 2 else np.float32
    vw = 16 // esize
    for want_probs in (True, False):
        rng = np.random.default_rng(1000 * esize + ncls)
        x = rng.uniform(-30, 29, (6, ld)).astype(dt)
        x[:, ncls:] = 60000                                   # the columns between ncls and ld must be ignored
        x[0, :ncls] = 1.5                                     # equal logits: index 0
        i0 = 3 * vw + 1
        pairs = [(i0, i0 + 2),                                # inside one vector
                 (i0, min(i0 + 256 * vw, ncls - 1)),          # the same thread's next vector
                 (i0, min(i0 + 64 * vw, ncls - 1)),           # another wave
                 (0, ncls // 2),                              # at index 0
                 (ncls // 3, ncls - 1)]                       # at ncls - 1
        for r, (a, b) in enumerate(pairs, start=1):
            x[r, a] = x[r, b] = 30
        tensors = [x.reshape(2, 1, 3, ld), _nan((2, 1, 3, ncls), np.float32), np.full((2, 1, 3, 2), -1, np.int32)]
        rec = H.softmax_op(H.view(H.ext(0), 2, 1, 3, ld, ld, esize), H.view(H.ext(2), 2, 1, 3, 2, 2, 4),
                           H.view(H.ext(1), 2, 1, 3, ncls, ncls, 4) if want_probs else None, ncls)
        assert H.softmax_form(rec) == SOFTMAX[key], (key, H.softmax_form(rec))
        logits = x[:, :ncls].copy()
        (p64, inv64), (ep, ei) = H.reference(lambda d: H.ref_softmax(logits, d))

        def check(out, want_probs=want_probs, p64=p64, inv64=inv64, ep=ep, ei=ei, logits=logits):
            idx = out[2].reshape(6, 2)[:, 0]
            assert np.array_equal(idx, np.argmax(logits, axis=1)), (key, idx, np.argmax(logits, axis=1))
            worst = H.ratio(out[2].reshape(6, 2)[:, 1].copy().view(np.float32), inv64, ei, (key, "maxp = 1 / sum"))
            if want_probs:
                worst = max(worst, H.ratio(out[1].reshape(6, ncls), p64, ep, (key, "probabilities")))
            else:
                assert np.isnan(out[1]).all(), (key, "the probability row was written without being asked for")
            return worst
        yield _single(f"softmax{key}probs{int(want_probs)}", rec, H.Blob(), tensors, check)


# ================================================================================================================== layer norm
def layernorm_cases(C):
    for rows in (1, 5, 37, 260):
        for eps in (1e-6, 1e-5):
            for kind in ("n01", "m30"):
                rng = np.random.default_rng(C * 1000 + rows)
                x = rng.normal(0, 1, (1, 1, rows, C)) if kind == "n01" else rng.normal(30, 0.5, (1, 1, rows, C))
                x = H.f16(x)
                if rows > 1:
                    x[0, 0, rows - 1] = 3.5                       # a constant row: the output is the bias
                yield _ln_case(f"ln C{C} rows{rows} eps{eps} {kind}", x, eps, rng, const_row=rows - 1 if rows > 1 else None)
    # ragged: zeros at x >= width
    rng = np.random.default_rng(C)
    yield _ln_case(f"ln C{C} ragged", H.f16(rng.normal(0, 1, (3, 1, 7, C))), 1e-5, rng, widths=np.array([[7, 1, 4]], np.int32))


def _ln_case(name, x, eps, rng, const_row=None, widths=None, refused=False):
    n, h, w, C = x.shape
    g, b = rng.normal(1, 0.2, C).astype(np.float32), rng.normal(0, 0.5, C).astype(np.float32)
    blob = H.Blob()
    w_off = blob.add(np.concatenate([g, b]))
    wl = (1, 1) if widths is not None else (0, 0)
    rec = H.layernorm_op(H.view(H.ext(0), n, h, w, C), H.view(H.ext(1), n, h, w, C), eps, w_off, wl=wl)
    if refused:
        return _single(name, rec, blob, [x, _nan(x.shape)], None, refused=True)
    wl_out = None if widths is None else widths[0]
    (y64,), (e32,) = H.reference(lambda d: H.ref_layernorm(x, g, b, eps, wl_out, d))

    def check(out):
        worst = H.ratio(out[1], y64, e32, name)
        if const_row is not None:
            assert np.array_equal(out[1][0, 0, const_row], b.astype(np.float16)), (name, "constant row != bias")
        if wl_out is not None:
            for s, wn in enumerate(wl_out):
                assert not out[1][s, :, wn:].view(np.uint16).any(), (name, "values right of the sample's width")
        return worst
    return _single(name, rec, blob, [x, _nan(x.shape)], check, widths=widths)


def layernorm_refused_cases():
    rng = np.random.default_rng(136)
    yield _ln_case("ln C136", H.f16(rng.normal(0, 1, (1, 1, 4, 136))), 1e-5, rng, refused=True)


# ================================================================================================================== attention
def _attn_run(qkv, heads, hd, lens=None):
    B, _, T, _ = qkv.shape
    C = heads * hd
    scale = float(hd) ** -0.5
    widths = None if lens is None else np.asarray([lens], np.int32)
    rec = H.attn_op(H.view(H.ext(0), B, 1, T, 3 * C), H.view(H.ext(1), B, 1, T, C), heads, hd, scale,
                    wl=(1, 1) if lens is not None else (0, 0))
    return H.Run(rec, H.Blob().array(), [qkv, _nan((B, 1, T, C))], widths), scale


def _attn_case(name, qkv, heads, hd, lens=None, **kw):
    run, scale = _attn_run(qkv, heads, hd, lens)
    (y64,), (e32,) = H.reference(lambda d: H.ref_attn(qkv, heads, hd, np.float32(scale), lens, d))
    return H.Case(name, [run], lambda outs: H.ratio(outs[0][1], y64, e32, name), **kw)


def attention_cases(key):
    heads, hd = key
    C = heads * hd
    for i, T in enumerate((1, 7, 40, 256, 257, 300)):
        B = 1 + i % 3
        rng = np.random.default_rng(T * 100 + C)
        yield _attn_case(f"attn h{heads} d{hd} T{T} B{B}", H.f16(rng.normal(0, 1, (B, 1, T, 3 * C))), heads, hd)
    # ragged: the rows behind a sample's length hold +-6e4 and must change nothing; its output rows there are zeros; a sample gets the
    # same bits alone (a dense batch of one, as long as the sample) as in the batch of three
    lens = (300, 1, 129)
    rng = np.random.default_rng(C)
    qkv = H.f16(rng.normal(0, 1, (3, 1, 300, 3 * C)))
    for b, tb in enumerate(lens):
        qkv[b, 0, tb:] = H.f16(np.where(rng.random((300 - tb, 3 * C)) < 0.5, -6e4, 6e4))
    run3, scale = _attn_run(qkv, heads, hd, lens)
    alone = [_attn_run(np.ascontiguousarray(qkv[b:b + 1, :, :tb]), heads, hd)[0] for b, tb in enumerate(lens)]
    (y64,), (e32,) = H.reference(lambda d: H.ref_attn(qkv, heads, hd, np.float32(scale), lens, d))
    name = f"attn h{heads} d{hd} ragged"

    def check(outs):
        got = outs[0][1]
        worst = H.ratio(got, y64, e32, name)
        for b, tb in enumerate(lens):
            assert not got[b, 0, tb:].view(np.uint16).any(), (name, "rows behind the sample's length")
            assert np.array_equal(got[b, 0, :tb].view(np.uint16), outs[1 + b][1][0, 0].view(np.uint16)), (name, b, "alone != in the batch")
        return worst
    yield H.Case(name, [run3] + alone, check)


def attention_lds_cases():
    """T = 513: 2 x 513 x 16 floats = 65 664 bytes of dynamic LDS, the first size above 64 KiB — it must match the reference or be refused
    with VSE_E_UNSUPPORTED, never fail to launch.  T = 1280 = 160 KiB is the largest the launcher accepts (attention_refused_cases: 1281)."""
    for T in (513, 1280):
        rng = np.random.default_rng(T)
        yield _attn_case(f"attn T{T}", H.f16(rng.normal(0, 1, (1, 1, T, 3 * 32))), 4, 8, may_refuse=True)


def attention_refused_cases():
    rng = np.random.default_rng(32)
    run, _ = _attn_run(H.f16(rng.normal(0, 1, (1, 1, 4, 3 * 64))), 2, 32)
    yield H.Case("attn hd32", [run], refused=True)
    run, _ = _attn_run(H.f16(rng.normal(0, 1, (1, 1, 1281, 3 * 8))), 1, 8)
    yield H.Case("attn T1281", [run], refused=True)


# ================================================================================================================== LSTM
def _lstm_inputs(rng, B, T, H, ndir):
    """-> gate pre-activations [ndir][B,T,4H] fp32 (N(0,1), a few at +-20) and W_hh [ndir][4H,H] as the fp16 values the kernels read."""
    g = rng.normal(0, 1, (ndir, B, T, 4 * H)).astype(np.float32)
    hot = rng.random(g.shape) < 0.002
    g[hot] = np.where(rng.random(int(hot.sum())) < 0.5, -20.0, 20.0)
    w = H_f16f32(rng.normal(0, H ** -0.5, (ndir, 4 * H, H)))
    return g, w


def H_f16f32(a):
    return H.f16(a).astype(np.float32)


def _poison(g, lens):
    g = g.copy()
    if lens is not None:
        for b, tb in enumerate(lens):
            g[:, b, tb:] = np.nan                             # the gates behind a sample's length are never read
    return g


def _lstm_mfma_run(g, w, mode, lens=None):
    """g [ndir][B,T,1024] in i, f, g, o order (poisoned behind the lengths), w [ndir][1024,256]."""
    ndir, B, T, _ = g.shape
    assert ndir == (2 if mode == 2 else 1)
    blob = H.Blob()
    w_off = blob.add(H.lstm_mfma_blob(list(w)))
    gk = [H.lstm_mfma_gates(g[d]).reshape(B, 1, T, 1024) for d in range(ndir)]
    tensors = gk + [_nan((B, 1, T, 256 * ndir))]
    rec = H.lstm_op([H.view(H.ext(d), B, 1, T, 1024, 1024, 4) for d in range(ndir)], H.view(H.ext(ndir), B, 1, T, 256 * ndir), 256, mode,
                    w_off, True, wl=(1, 1) if lens is not None else (0, 0))
    assert H.lstm_form(rec) == "mfma"
    return H.Run(rec, blob.array(), tensors, None if lens is None else np.asarray([lens], np.int32))


def _lstm_ref(g, w, revs, lens):
    return H.reference(lambda d: np.concatenate([H.ref_lstm(np.nan_to_num(g[k]), w[k], rv, lens, d) for k, rv in enumerate(revs)], -1))


def _check_lstm(name, got, y64, e32, lens):
    worst = H.ratio(got, y64, e32, name)
    if lens is not None:
        for b, tb in enumerate(lens):
            assert not got[b, tb:].view(np.uint16).any(), (name, b, "steps behind the sample's length")
    return worst


def lstm_mfma_cases(mode):
    ndir = 2 if mode == 2 else 1
    revs = [False, True] if mode == 2 else [mode == 1]
    for B in (1, 31, 32, 33, 40):
        for T in (1, 2, 25):
            rng = np.random.default_rng(B * 100 + T + 7 * mode)
            g, w = _lstm_inputs(rng, B, T, 256, ndir)
            run = _lstm_mfma_run(g, w, mode)
            (y64,), (e32,) = _lstm_ref(g, w, revs, None)
            name = f"lstm mfma mode{mode} B{B} T{T}"
            yield H.Case(name, [run], lambda outs, name=name, y64=y64, e32=e32, n=ndir: _check_lstm(name, outs[0][n][:, 0], y64, e32, None))
    # ragged: lengths mix 1 and the full T; the second tile's samples are all shorter than T
    B, T = 40, 25
    rng = np.random.default_rng(4025 + mode)
    lens = [1 if b % 3 == 0 else (T if b % 3 == 1 else 1 + (7 * b) % T) for b in range(32)] + [1 + b for b in range(8)]
    g, w = _lstm_inputs(rng, B, T, 256, ndir)
    g = _poison(g, lens)
    (y64,), (e32,) = _lstm_ref(g, w, revs, lens)
    name = f"lstm mfma mode{mode} ragged"
    yield H.Case(name, [_lstm_mfma_run(g, w, mode, lens)],
                 lambda outs: _check_lstm(name, outs[0][ndir][:, 0], y64, e32, lens))
    # batch independence: one sample alone, at position 0 and at position 32 (the second tile) of B = 33
    T = 25
    g, w = _lstm_inputs(np.random.default_rng(33 + mode), 33, T, 256, ndir)
    g[:, 32] = g[:, 0]
    name2 = f"lstm mfma mode{mode} batch independence"

    def check_indep(outs):
        alone, batch = outs[0][ndir], outs[1][ndir]
        assert np.array_equal(alone[0].view(np.uint16), batch[0].view(np.uint16)), (name2, "alone != position 0 of 33")
        assert np.array_equal(alone[0].view(np.uint16), batch[32].view(np.uint16)), (name2, "alone != position 32 of 33")
        return 0.0
    yield H.Case(name2, [_lstm_mfma_run(np.ascontiguousarray(g[:, :1]), w, mode), _lstm_mfma_run(g, w, mode)], check_indep)


def lstm_scalar_cases(Hd):
    B, T = 3, 9
    for rev in (0, 1):
        for lens in (None, [9, 1, 4]):
            rng = np.random.default_rng(Hd * 10 + rev)
            g, w = _lstm_inputs(rng, B, T, Hd, 1)
            g = _poison(g, lens)
            blob = H.Blob()
            w_off = blob.add(H.f16(w[0].T))                   # W_hh^T fp16 [H][4H]
            # the output is one direction's half of a [B,1,T,2H] tensor, as the compiler lays a bidirectional layer out
            off = rev * Hd
            rec = H.lstm_op(H.view(H.ext(0), B, 1, T, 4 * Hd, 4 * Hd, 4), H.view(H.ext(1), B, 1, T, Hd, 2 * Hd, 2, off * 2), Hd, rev,
                            w_off, False, wl=(1, 1) if lens is not None else (0, 0))
            assert H.lstm_form(rec) == "scalar"
            (y64,), (e32,) = _lstm_ref(g, w, [bool(rev)], lens)
            name = f"lstm scalar H{Hd} rev{rev} ragged{int(lens is not None)}"

            def check(out, name=name, y64=y64, e32=e32, lens=lens, off=off):
                full = out[1][:, 0]
                assert np.isnan(full[..., (Hd - off):(2 * Hd - off)]).all(), (name, "wrote into the other direction's half")
                return _check_lstm(name, full[..., off:off + Hd], y64, e32, lens)
            yield _single(name, rec, blob, [g[0].reshape(B, 1, T, 4 * Hd), _nan((B, 1, T, 2 * Hd))], check,
                          widths=None if lens is None else np.asarray([lens], np.int32))


def lstm_refused_cases():
    blob = H.Blob()
    w_off = blob.add(np.zeros(16, np.float16))
    rec = H.lstm_op(H.view(H.ext(0), 1, 1, 2, 2048, 2048, 4), H.view(H.ext(1), 1, 1, 2, 512), 512, 0, w_off, False)
    assert H.lstm_form(rec) == "refused"
    yield _single("lstm H512", rec, blob, [np.zeros((1, 1, 2, 2048), np.float32), _nan((1, 1, 2, 512))], None, refused=True)


# ================================================================================================================== depthwise conv
def _dw_case(name, form, n, h, w, C, k, s, pad=None, act=ir.ACT_HSWISH, post=(0.75, 0.125), gate=0, pair_in=False, pair_out=False,
             widths=None, seed=0, expect=None):
    """gate: 0 none, 1 x * g, 2 x * g + x.  pair_in / pair_out: fp16 hi + lo tensors, the lo half C channels behind the hi half."""
    (kh, kw), (sh, sw) = k, s
    ph, pw = (kh // 2, kw // 2) if pad is None else pad
    oh, ow = (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1
    rng = np.random.default_rng(seed + 31 * h + 7 * w + C)
    x = H.f16(rng.normal(0, 1, (n, h, w, C)))
    if widths is not None:
        for b, wn in enumerate(widths):
            x[b, :, wn:] = 0                                  # a ragged tensor is zero right of each sample
    wk = H_f16f32(rng.normal(0, 0.3, (kh * kw, C)))           # the filter table: fp16 values held as fp32
    bias = rng.normal(0, 0.3, C).astype(np.float32)
    blob = H.Blob()
    w_off, b_off = blob.add(wk), blob.add(bias)
    xin = x
    x_eff = x.astype(np.float64)
    if pair_in:
        lo = H.f16(rng.normal(0, 2.0 ** -12, x.shape) * np.abs(x.astype(np.float64)))
        xin = np.concatenate([x, lo], -1)
        x_eff = x.astype(np.float64) + lo.astype(np.float64)
    tensors = [xin, _nan((n, oh, ow, C * (2 if pair_out else 1)))]
    gview = None
    if gate:
        gv = H.f16(rng.uniform(0, 1, (n, 1, 1, C)))
        tensors.append(gv)
        gview = H.view(H.ext(2), n, 1, 1, C)
        # the gate product is rounded to fp16 on load, from its fp32 value — what a separate scale pass stores
        v = x.astype(np.float32) * gv.astype(np.float32)
        x_eff = ((v + x.astype(np.float32)) if gate == 2 else v).astype(np.float16).astype(np.float64)
    rec = H.dwconv_op(H.view(H.ext(0), n, h, w, C, xin.shape[-1]), H.view(H.ext(1), n, oh, ow, C, tensors[1].shape[-1]), k, s, (ph, pw),
                      w_off, b_off, act=act, post_a=post[0], post_b=post[1], gate=gview, gate_res=gate == 2,
                      lo_in=C if pair_in else 0, lo_out=C if pair_out else 0, wl=(1, 1) if widths is not None else (0, 0))
    got_form = H.dwconv_form(rec)
    assert got_form[0] == form, (name, got_form)
    if expect is not None:
        assert expect(got_form), (name, got_form)
    wl_out = None if widths is None else np.asarray(widths)
    (y64,), (e32,) = H.reference(lambda d: H.ref_dwconv(x_eff, wk, bias, k, s, (ph, pw), act, 0.0, 0.0, post[0], post[1], wl_out, d))

    def check(out):
        o = out[1]
        if pair_out:
            return H.ratio(o[..., :C].astype(np.float64) + o[..., C:].astype(np.float64), y64, e32, name, pair=True)
        worst = H.ratio(o, y64, e32, name)
        if wl_out is not None:
            for b, wn in enumerate(wl_out):
                assert not o[b, :, wn:].view(np.uint16).any(), (name, "values right of the sample's width")
        return worst
    return _single(name, rec, blob, tensors, check, widths=None if widths is None else np.asarray([widths], np.int32))


def dwconv_col_cases(key):
    k, sh = key
    i = 0
    for w in (1, 3, 4, 5, 50):
        for h in (1, 2, 3, 12, 37):
            C = (8, 24, 240)[i % 3]
            i += 1
            expect = None
            if h == 37 and sh == 1:
                expect = lambda f: f[1] == 10 and f[2] == 4        # ten segments of four rows: the last one holds ONE row
            yield _dw_case(f"dw col k{k} sh{sh} {h}x{w} C{C}", "col", 2, h, w, C, (k, k), (sh, 1), seed=k, expect=expect)
    yield _dw_case(f"dw col k{k} sh{sh} ragged", "col", 2, 12, 50, 24, (k, k), (sh, 1), widths=[50, 17], seed=k)


def dwconv_row_cases():
    for k in (3, 5):
        yield _dw_case(f"dw row k{k} sw2", "row", 2, 9, 21, 24, (k, k), (2, 2), seed=1)
        yield _dw_case(f"dw row k{k} sw2 sh1 ragged", "row", 2, 5, 22, 8, (k, k), (1, 2), widths=[11, 4], seed=2)
        yield _dw_case(f"dw row k{k} gate", "row", 2, 7, 13, 72, (k, k), (1, 1), gate=1, seed=3)
        yield _dw_case(f"dw row k{k} gate + residual", "row", 2, 7, 13, 72, (k, k), (2, 2), gate=2, seed=4)
        yield _dw_case(f"dw row k{k} pair in / out", "row", 2, 6, 10, 16, (k, k), (1, 1), pair_in=True, pair_out=True, act=ir.ACT_NONE,
                       post=(1.0, 0.0), seed=5)
        yield _dw_case(f"dw row k{k} pair out", "row", 1, 5, 9, 8, (k, k), (2, 2), pair_out=True, seed=6)
    yield _dw_case("dw row kh5 kw3", "row", 2, 8, 11, 16, (5, 3), (1, 1), seed=7)
    yield _dw_case("dw row kh1 kw5", "row", 1, 4, 17, 8, (1, 5), (1, 1), act=ir.ACT_RELU, seed=8)


def dwconv_generic_cases():
    yield _dw_case("dw generic kw1", "generic", 2, 9, 7, 24, (3, 1), (1, 1), seed=9)
    yield _dw_case("dw generic kw7", "generic", 2, 9, 13, 16, (7, 7), (1, 1), seed=10)
    yield _dw_case("dw generic kw7 s2 gate", "generic", 1, 11, 14, 8, (7, 7), (2, 2), gate=1, seed=11)
    yield _dw_case("dw generic kw1 pair", "generic", 1, 5, 6, 8, (3, 1), (2, 1), pair_in=True, pair_out=True, seed=12)


# ================================================================================================================== pooling
def _pool_case(name, n, h, w, C, k, s, pad, is_max, ceil, excl, widths=None, seed=0):
    rng = np.random.default_rng(seed + 13 * h + w + C)
    x = H.f16(rng.normal(0, 1, (n, h, w, C)))
    oh = int(compiler.level_width(h, k[0], s[0], pad[0], ceil))
    ow = int(compiler.level_width(w, k[1], s[1], pad[1], ceil))
    wtab = wl_in = wl_out = None
    if widths is not None:
        wl_in = np.asarray(widths, np.int64)
        wl_out = np.asarray(compiler.level_width(wl_in, k[1], s[1], pad[1], ceil), np.int64)
        wtab = np.stack([wl_in, wl_out]).astype(np.int32)
        for b, wn in enumerate(wl_in):
            x[b, :, wn:] = H.f16(6e4)                          # the window is clipped to the SAMPLE: never read
    rec = H.pool_op(H.view(H.ext(0), n, h, w, C), H.view(H.ext(1), n, oh, ow, C), k, s, pad, is_max, ceil, excl,
                    wl=(1, 2) if widths is not None else (0, 0))
    assert H.pool_form(rec) == ("max" if is_max else ("avg_excl" if excl else "avg_incl")), name
    (y64,), (e32,) = H.reference(lambda d: H.ref_pool(x, k, s, pad, is_max, ceil, excl, wl_in, wl_out, ow, d))
    assert y64.shape == (n, oh, ow, C), (name, y64.shape, (n, oh, ow, C))     # torch's output size = compiler.level_width (Paddle's rule)

    def check(out):
        o = out[1]
        if is_max:
            assert np.array_equal(o.astype(np.float64), y64), (name, "max pool is not bit-exact")
            worst = 0.0
        else:
            worst = H.ratio(o, y64, e32, name)
        if wl_out is not None:
            for b, wn in enumerate(wl_out):
                assert not o[b, :, wn:].view(np.uint16).any(), (name, "values right of the sample's width")
        return worst
    return _single(name, rec, H.Blob(), [x, _nan((n, oh, ow, C))], check, widths=wtab)


def pool_cases(is_max):
    i = 0
    for k, s in (((2, 2), (2, 2)), ((3, 3), (2, 2)), ((3, 2), (2, 2)), ((2, 1), (2, 1)), ((3, 3), (1, 1))):
        for pad in (0, 1):
            for ceil in (False, True):
                for excl in ((True,) if is_max else (True, False)):
                    C = (8, 72)[i % 2]
                    i += 1
                    pd = (pad, pad if k[1] > 1 else 0)
                    yield _pool_case(f"pool max{int(is_max)} k{k} s{s} p{pd} ceil{int(ceil)} excl{int(excl)} C{C}", 2, 9, 15, C, k, s, pd,
                                     is_max, ceil, excl, seed=i)
    # ragged: per-sample input and output widths, V2's avg 2x2 / (2,1) ceil pools among them
    yield _pool_case("pool ragged 2x2 ceil", 3, 7, 21, 8, (2, 2), (2, 2), (0, 0), is_max, True, True, widths=[21, 5, 12], seed=50)
    yield _pool_case("pool ragged (2,1) ceil", 3, 7, 21, 72, (2, 1), (2, 1), (0, 0), is_max, True, True, widths=[21, 1, 12], seed=51)
    yield _pool_case("pool ragged 3x3 p1", 3, 8, 20, 8, (3, 3), (2, 2), (1, 1), is_max, False, is_max, widths=[20, 3, 11], seed=52)
    yield _pool_case("pool ragged 3x3 p1 ceil", 3, 9, 21, 8, (3, 3), (2, 2), (1, 1), is_max, True, is_max, widths=[21, 2, 12], seed=53)


# ================================================================================================================== global average
def gap_cases():
    i = 0
    for C in (8, 72, 200):
        for h, w in ((1, 1), (3, 11), (25, 40)):
            for splits in (1, 3, 7):
                i += 1
                rng = np.random.default_rng(i)
                x = H.f16(rng.normal(0.5, 1, (2, h, w, C)))
                rec = H.gap_op(H.view(H.ext(0), 2, h, w, C), H.view(ir.ARENA_WS, 2, splits, 1, C, C, 4), H.view(H.ext(1), 2, 1, 1, C))
                (y64,), (e32,) = H.reference(lambda d: H.ref_gap(x, None, d))
                name = f"gap C{C} {h}x{w} splits{splits}"
                yield _single(name, rec, H.Blob(), [x, _nan((2, 1, 1, C))],
                              lambda out, name=name, y64=y64, e32=e32: H.ratio(out[1], y64, e32, name), ws_bytes=2 * splits * C * 4)
    # the ragged row form: mixed widths (values right of a sample are never read); a sample alone = the sample in the batch, bit for bit
    for C in (8, 72, 200):
        h, w, widths = 3, 70, [70, 1, 33]
        rng = np.random.default_rng(500 + C)
        x = H.f16(rng.normal(0.5, 1, (3, h, w, C)))
        for b, wn in enumerate(widths):
            x[b, :, wn:] = H.f16(6e4)

        def run(xs, ws):
            nb, ww = xs.shape[0], xs.shape[2]
            rec = H.gap_op(H.view(H.ext(0), nb, h, ww, C), H.view(ir.ARENA_WS, nb, h, 1, C, C, 4), H.view(H.ext(1), nb, 1, 1, C), wl=(1, 0))
            return H.Run(rec, H.Blob().array(), [xs, _nan((nb, 1, 1, C))], np.asarray([ws], np.int32), nb * h * C * 4)
        runs = [run(x, widths)] + [run(np.ascontiguousarray(x[b:b + 1, :, :wn]), [wn]) for b, wn in enumerate(widths)]
        (y64,), (e32,) = H.reference(lambda d: H.ref_gap(x, widths, d))
        name = f"gap rows C{C}"

        def check(outs, name=name, y64=y64, e32=e32):
            worst = H.ratio(outs[0][1], y64, e32, name)
            for b in range(3):
                assert np.array_equal(outs[0][1][b].view(np.uint16), outs[1 + b][1][0].view(np.uint16)), (name, b, "alone != in the batch")
            return worst
        yield H.Case(name, runs, check)


# ================================================================================================================== element-wise
def elementwise_cases():
    rng = np.random.default_rng(77)
    n, h, w, C = 2, 5, 7, 24
    x = H.f16(rng.normal(0, 1, (n, h, w, C)))
    # ---- OP_SCALE
    s = H.f16(rng.uniform(0, 1, (n, 1, 1, C)))
    for res in (0, 1):
        rec = H.op(ir.OP_SCALE, [H.view(H.ext(0), n, h, w, C), H.view(H.ext(1), n, 1, 1, C)], H.view(H.ext(2), n, h, w, C),
                   flags=ir.F_RES if res else 0)
        (y64,), (e32,) = H.reference(lambda d, res=res: x.astype(d) * s.astype(d) + (x.astype(d) if res else d(0)))
        name = f"scale res{res}"
        yield _single(name, rec, H.Blob(), [x, s, _nan(x.shape)], lambda out, name=name, y64=y64, e32=e32: H.ratio(out[2], y64, e32, name))
    # ---- OP_BINARY
    for mul in (0, 1):
        for shift in (0, 1):
            for act in (ir.ACT_NONE, ir.ACT_RELU, ir.ACT_HSWISH):
                hh, ww = 6, 10
                a = H.f16(rng.normal(0, 1, (n, hh, ww, C)))
                b = H.f16(rng.normal(0, 1, (n, hh >> shift, ww >> shift, C)))
                rec = H.op(ir.OP_BINARY, [H.view(H.ext(0), n, hh, ww, C), H.view(H.ext(1), n, hh >> shift, ww >> shift, C)],
                           H.view(H.ext(2), n, hh, ww, C), p={ir.P_BIN_MUL: mul, ir.P_BIN_SHIFT: shift, ir.P_BIN_ACT: act})

                def ref(d, a=a, b=b, mul=mul, shift=shift, act=act):
                    bu = b.astype(d)
                    if shift:
                        bu = bu.repeat(2, axis=1).repeat(2, axis=2)
                    return H.ref_act(a.astype(d) * bu if mul else a.astype(d) + bu, act)
                (y64,), (e32,) = H.reference(ref)
                name = f"binary mul{mul} shift{shift} act{act}"
                yield _single(name, rec, H.Blob(), [a, b, _nan(a.shape)], lambda out, name=name, y64=y64, e32=e32: H.ratio(out[2], y64, e32, name))
    # ---- OP_RESIZE into a concat slice: channels [C, 2C) of a 3C-wide tensor, x2 nearest up-sampling; bit-exact, neighbours untouched
    rec = H.op(ir.OP_RESIZE, [H.view(H.ext(0), n, h, w, C)], H.view(H.ext(1), n, 2 * h, 2 * w, C, 3 * C, 2, C * 2), p={0: 1})

    def check_resize(out):
        o = out[1]
        assert np.array_equal(o[..., C:2 * C].view(np.uint16), x.repeat(2, axis=1).repeat(2, axis=2).view(np.uint16)), "resize into a slice"
        assert np.isnan(o[..., :C]).all() and np.isnan(o[..., 2 * C:]).all(), "resize wrote outside its concat slice"
        return 0.0
    yield _single("resize slice", rec, H.Blob(), [x, _nan((n, 2 * h, 2 * w, 3 * C))], check_resize)
    rec = H.op(ir.OP_RESIZE, [H.view(H.ext(0), n, h, w, C)], H.view(H.ext(1), n, h, w, 16), p={0: 0})     # a copy of the first 16 channels

    def check_copy(out):
        assert np.array_equal(out[1].view(np.uint16), x[..., :16].view(np.uint16)), "copy is not bit-exact"
        return 0.0
    yield _single("resize copy", rec, H.Blob(), [x, _nan((n, h, w, 16))], check_copy)
    # ---- the gated two-source form: out = [up(A) * (1 + gA) | B * (1 + gB)] into a slice
    Ca, Cb = 16, 8
    A = H.f16(rng.normal(0, 1, (n, 3, 4, Ca)))
    Bt = H.f16(rng.normal(0, 1, (n, 6, 8, Cb)))
    gA, gB = H.f16(rng.uniform(0, 1, (n, 1, 1, Ca))), H.f16(rng.uniform(0, 1, (n, 1, 1, Cb)))
    for plus1 in (1, 0):
        rec = H.op(ir.OP_RESIZE, [H.view(H.ext(0), n, 3, 4, Ca), H.view(H.ext(1), n, 1, 1, Ca), H.view(H.ext(2), n, 6, 8, Cb)],
                   H.view(H.ext(4), n, 6, 8, Ca + Cb, Ca + Cb + 8, 2, 8 * 2), out2=H.view(H.ext(3), n, 1, 1, Cb),
                   flags=ir.F_GATE | ir.F_SRC2 | (ir.F_RES if plus1 else 0), p={0: 1, 1: 0})

        def ref(d, plus1=plus1):
            ya = A.astype(d).repeat(2, axis=1).repeat(2, axis=2) * (d(plus1) + gA.astype(d))
            return np.concatenate([ya, Bt.astype(d) * (d(plus1) + gB.astype(d))], -1)
        (y64,), (e32,) = H.reference(ref)
        name = f"resize gated two sources plus{plus1}"

        def check_g(out, name=name, y64=y64, e32=e32):
            assert np.isnan(out[4][..., :8]).all(), (name, "wrote in front of its concat slice")
            return H.ratio(out[4][..., 8:], y64, e32, name)
        yield _single(name, rec, H.Blob(), [A, gA, Bt, gB, _nan((n, 6, 8, Ca + Cb + 8))], check_g)
    # ---- OP_UNARY: the vector form, ragged and plain; the scalar form (1 channel at pixel stride 8 -> dense fp32, sigmoid)
    fpar = {ir.FS_PRE_A: 1.5, ir.FS_PRE_B: -0.25, ir.FS_POST_A: 0.5, ir.FS_POST_B: 0.125, ir.FS_ACT_A: 0.2, ir.FS_ACT_B: 0.5}
    for act in (ir.ACT_HSWISH, ir.ACT_HSIGMOID, ir.ACT_SWISH):
        for widths in (None, [7, 2]):
            rec = H.op(ir.OP_UNARY, [H.view(H.ext(0), n, h, w, C)], H.view(H.ext(1), n, h, w, C), p={0: act}, f=fpar,
                       wl=(1, 1) if widths else (0, 0))

            def ref(d, act=act, widths=widths):
                y = H.ref_act(x.astype(d) * d(np.float32(1.5)) + d(np.float32(-0.25)), act, 0.2, 0.5) * d(0.5) + d(0.125)
                return H.mask_width(y, widths)
            (y64,), (e32,) = H.reference(ref)
            name = f"unary vec act{act} ragged{int(widths is not None)}"
            yield _single(name, rec, H.Blob(), [x, _nan(x.shape)], lambda out, name=name, y64=y64, e32=e32: H.ratio(out[1], y64, e32, name),
                          widths=None if widths is None else np.asarray([widths], np.int32))
    x8 = H.f16(rng.normal(0, 2, (n, h, w, 8)))
    rec = H.op(ir.OP_UNARY, [H.view(H.ext(0), n, h, w, 1, 8)], H.view(H.ext(1), n, h, w, 1, 1, 4), flags=ir.F_OUT_F32, p={0: ir.ACT_SIGMOID},
               f={ir.FS_PRE_A: 1.0, ir.FS_POST_A: 1.0})
    (y64,), (e32,) = H.reference(lambda d: H.ref_act(x8[..., :1].astype(d), ir.ACT_SIGMOID))
    yield _single("unary scalar", rec, H.Blob(), [x8, _nan((n, h, w, 1), np.float32)], lambda out: H.ratio(out[1], y64, e32, "unary scalar"))
    # ---- OP_WSCALE: per-image weights = tiled blob x gate over k; the gate is narrower than Kp (the rest of K counts as zero)
    for kt in (32, 64):
        Kp, Np, Cg = 128, 16, 72
        wt = H.f16(rng.normal(0, 0.2, (Kp // kt, Np, kt)))
        g = H.f16(rng.uniform(0, 1, (n, 1, 1, Cg)))
        blob = H.Blob()
        w_off = blob.add(wt)
        rec = H.op(ir.OP_WSCALE, [H.view(H.ext(0), n, 1, 1, Cg)], H.view(H.ext(1), n, 1, 1, Kp * Np), p={0: Kp, 1: Np, 2: kt}, w_off=w_off)

        def ref(d, wt=wt, g=g, kt=kt):
            gk = np.zeros((n, Kp), d)
            gk[:, :Cg] = g.reshape(n, Cg).astype(d)
            return (wt.astype(d)[None] * gk.reshape(n, Kp // kt, 1, kt)).reshape(n, 1, 1, Kp * Np)
        (y64,), (e32,) = H.reference(ref)
        name = f"wscale kt{kt}"
        yield _single(name, rec, blob, [g, _nan((n, 1, 1, Kp * Np))], lambda out, name=name, y64=y64, e32=e32: H.ratio(out[1], y64, e32, name))


# ================================================================================================================== the groups
GROUPS = {}
for _k in SOFTMAX:
    GROUPS["softmax-e%d-%d-ld%d" % _k] = (lambda k=_k: softmax_cases(k))
for _c in (8, 64, 120, 128):
    GROUPS["layernorm-C%d" % _c] = (lambda c=_c: layernorm_cases(c))
for _k in ((8, 15), (8, 16), (4, 8)):
    GROUPS["attention-h%d-d%d" % _k] = (lambda k=_k: attention_cases(k))
GROUPS["attention-lds"] = attention_lds_cases
for _m in (0, 1, 2):
    GROUPS["lstm-mfma-mode%d" % _m] = (lambda m=_m: lstm_mfma_cases(m))
for _h in (48, 96, 256):
    GROUPS["lstm-scalar-H%d" % _h] = (lambda h=_h: lstm_scalar_cases(h))
for _k in ((3, 1), (3, 2), (5, 1), (5, 2)):
    GROUPS["dwconv-col-k%d-sh%d" % _k] = (lambda k=_k: dwconv_col_cases(k))
GROUPS["dwconv-row"] = dwconv_row_cases
GROUPS["dwconv-generic"] = dwconv_generic_cases
GROUPS["pool-max"] = lambda: pool_cases(True)
GROUPS["pool-avg"] = lambda: pool_cases(False)
GROUPS["gap"] = gap_cases
GROUPS["elementwise"] = elementwise_cases
# records the library must answer with a negative code (GPU only: the emulator has no launcher)
REFUSED = {"layernorm-C136": layernorm_refused_cases, "attention-hd32-T1281": attention_refused_cases, "lstm-scalar-H512": lstm_refused_cases}

