"""vse_yuv_resample on the MI355X: every comparison is byte equality with the int64 restatement of the rule (tests/resample_ref.py), inside
buffers filled with 0xA5 so that a byte written outside a picture shows, and the inputs must come back unchanged.  Random tables that no
filter would produce (left off both edges, coefficients of both signs within the bound, sums that clip at both ends, every even K from 2
to 16) over random full-range words, the general kernel's shapes and the fast kernel's, for 1- and 2-byte samples and every plane layout;
padded, byte-offset and row-parity calls; the identity table; the product's own tables; what the call and the binding must refuse;
staging.Uploader over YuvFrames and InterlacedYuvFrames with resample=; and SubtitleExtractor over a squeezed Y4M against the host route."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import deinterlace_ref as D
import resample_ref as RR
import yuv_format_ref as R
from test_gpu_deinterlace import FORMATS
from test_yuv_formats import ident, product_format

pytestmark = pytest.mark.gpu

FILL = 0xA5
GENERAL_SHAPES = [(1, 1, 1), (2, 2, 3), (3, 5, 4), (5, 17, 23), (7, 34, 41), (5, 50, 37)]           # (h, w_in, w_out); the last one shrinks
# the one-store kernel's shapes: the first two have 16-byte aligned luma rows of 1-byte samples (4:4:4 and grey take that kernel; the
# 24-byte chroma rows of subsampled planar formats send those to the general one), the third 16-byte aligned chroma rows as well
FAST_SHAPES = [(4, 32, 48), (6, 64, 48), (4, 64, 96)]
FAST_SHAPES_2 = [(4, 16, 32), (6, 48, 32)]                # ... every plane's rows of the 2-byte formats, subsampled chroma included
# (name, n, stride padding in samples, base offset in samples)
VARIANTS = [("packed", 1, 0, 0), ("packed", 3, 0, 0), ("padded 16", 3, 16, 0), ("padded odd", 3, 3, 0), ("base + 1", 3, 0, 1), ("base + 2", 1, 5, 2)]
TAPS = (2, 4, 6, 8, 10, 12, 14, 16)


def run_variant(ctx, rng, fmt, h, w_in, w_out, variant, parity, luma, chroma, wild=True, planes=None):
    """One call on pictures laid out as `variant` says, through the tables given -> the reference's output planes of every frame."""
    import torch
    _name, n, pad, off = variant
    ss = 1 if fmt[3] == 8 else 2
    frame_in, frame_out = R.packed_bytes(h, w_in, fmt, parity), R.packed_bytes(h, w_out, fmt, parity)
    stride, base = frame_in + pad * ss, off * ss
    pics = planes if planes is not None else [R.random_planes(rng, h, w_in, fmt, parity, wild=wild) for _ in range(n)]
    host = np.full(base + (n + 1) * stride, FILL, np.uint8)
    for k, p in enumerate(pics):
        host[base + k * stride:base + k * stride + frame_in] = R.pack(p, fmt)
    src = torch.from_numpy(host).to(ctx.tdev)
    packed = src[base:].as_strided((n, stride), (stride, 1))
    ostride = frame_out + (pad + (16 if pad % 16 == 0 else 1)) * ss                  # its own padding: 16-byte aligned where the input's is
    obase = 16 + base
    big = torch.full((obase + (n + 1) * ostride,), FILL, dtype=torch.uint8, device=ctx.tdev)
    out = big[obase:].as_strided((n, ostride), (ostride, 1))
    got = ctx.yuv_resample(packed, n, h, w_in, product_format(fmt), RR.Tables(w_in, w_out, luma, chroma), row_parity=parity, out=out)
    assert got is out
    want = np.full(big.numel(), FILL, np.uint8)
    outs = [RR.picture(p, fmt, luma, chroma) for p in pics]
    for f, o in enumerate(outs):
        assert [q.shape for q in o] == R.plane_shapes(h, w_out, fmt, parity)
        want[obase + f * ostride:obase + f * ostride + frame_out] = R.pack(o, fmt)
    assert np.array_equal(big.cpu().numpy(), want), (fmt, h, w_in, w_out, variant, parity, luma[1].shape[1])
    assert np.array_equal(src.cpu().numpy(), host)                                   # the inputs are read only
    return outs


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_bit_for_bit_with_sentinels(ctx, fmt):
    rng = np.random.default_rng(sum(fmt) + 3)
    maxv, shift = (1 << fmt[3]) - 1, (16 - fmt[3] if fmt[4] else 0)
    calls = itertools.count()
    seen_y, seen_c, low, high, off_left, off_right = set(), set(), 0, 0, 0, 0
    for (h, w_in, w_out), variant in itertools.product(GENERAL_SHAPES + FAST_SHAPES + FAST_SHAPES_2, VARIANTS):
        for parity in ((0, 1) if fmt[1] == 1 and variant[1] == 3 and variant[2] == 0 else (0,)):
            i = next(calls)
            k_y, k_c = TAPS[i % 8], TAPS[(3 * i + 1) % 8]                             # both run through every even K, in different orders
            seen_y, seen_c = seen_y | {k_y}, seen_c | {k_c}
            luma = RR.random_table(rng, w_in, w_out, k_y)
            cw_in, cw_out = RR.chroma_width(w_in, fmt), RR.chroma_width(w_out, fmt)
            chroma = RR.random_table(rng, cw_in, cw_out, k_c) if fmt[2] else None
            outs = run_variant(ctx, rng, fmt, h, w_in, w_out, variant, parity, luma, chroma)
            values = np.concatenate([p.reshape(-1).astype(np.int64) >> shift for o in outs for p in o])
            low, high = low + int((values == 0).sum()), high + int((values == maxv).sum())
            off_left, off_right = off_left + int((luma[0] < 0).sum()), off_right + int((luma[0] + k_y > w_in).sum())
    # by the reference, both clips and both clamps were exercised, with every even K
    assert seen_y == seen_c == set(TAPS) and low > 100 and high > 100 and off_left > 20 and off_right > 20, (low, high, off_left, off_right)


@pytest.mark.parametrize("fmt", [f for f in FORMATS if f[1] == 1], ids=ident)
def test_three_rows_of_odd_parity(ctx, fmt):
    """4:2:0 rows 1..3 of their picture (two chroma rows for three luma rows), 10 -> 7 columns, two frames."""
    rng = np.random.default_rng(sum(fmt) + 107)
    run_variant(ctx, rng, fmt, 3, 10, 7, ("packed", 2, 0, 0), 1, RR.random_table(rng, 10, 7, 4), RR.random_table(rng, 5, 4, 6))


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_identity_and_filter_tables(ctx, fmt):
    """The identity table gives the input bytes (valid samples: the low bits of a high-bit word are zero); ingest.Resample's own tables,
    through the binding's cache, give the reference builder's picture."""
    from vse_amd import ingest
    rng = np.random.default_rng(sum(fmt) + 11)
    for (h, w, _), variant in itertools.product(GENERAL_SHAPES[1:] + FAST_SHAPES + FAST_SHAPES_2, (VARIANTS[1], VARIANTS[3])):
        planes = [R.random_planes(rng, h, w, fmt) for _ in range(variant[1])]
        if fmt[4]:
            planes = [tuple(p & np.uint16((0xFFFF << (16 - fmt[3])) & 0xFFFF) for p in f) for f in planes]
        tables = (RR.identity(w), RR.identity(RR.chroma_width(w, fmt)) if fmt[2] else None)
        outs = run_variant(ctx, rng, fmt, h, w, w, variant, 0, *tables, planes=planes)
        assert all(np.array_equal(a, b) for o, f in zip(outs, planes) for a, b in zip(o, f))
    import torch
    pf = product_format(fmt)
    for (h, w_in, w_out), name in zip([(7, 34, 41), (5, 50, 37), (6, 64, 48), (6, 48, 32)], ("bicubic", "lanczos", "bilinear", "bicubic")):
        r = ingest.Resample(w_in, w_out, name)
        planes = [R.random_planes(rng, h, w_in, fmt, wild=True) for _ in range(2)]
        dev = torch.from_numpy(np.concatenate([R.pack(p, fmt) for p in planes])).to(ctx.tdev)
        frame = R.packed_bytes(h, w_out, fmt)
        for _ in range(2):                                                          # the second call takes the cached device tables
            got = ctx.yuv_resample(dev, 2, h, w_in, pf, r).cpu().numpy()
            for f, p in enumerate(planes):
                assert np.array_equal(got[f, :frame], R.pack(RR.picture(p, fmt, *RR.tables(w_in, w_out, fmt, name)), fmt)), (fmt, name)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import torch
    lib = ctx.lib
    h, w_in, w_out, n = 8, 16, 24, 2
    fmt = (1, 1, 1, 10, 0, 1, 0)
    frame_in, frame_out = R.packed_bytes(h, w_in, fmt), R.packed_bytes(h, w_out, fmt)
    luma, chroma = RR.identity(w_out), RR.identity(w_out // 2)
    tabs = RR.Tables(w_in, w_out, luma, chroma).packed(None)
    table = torch.zeros(1024, dtype=torch.uint8, device=ctx.tdev)                  # luma at 0, chroma at 512
    table[:len(tabs[0])] = torch.from_numpy(np.frombuffer(tabs[0], np.uint8).copy()).to(ctx.tdev)
    table[512:512 + len(tabs[1])] = torch.from_numpy(np.frombuffer(tabs[1], np.uint8).copy()).to(ctx.tdev)
    assert len(tabs[0]) == lib.vse_yuv_resample_table_bytes(w_out, 2) == 24 * 8 and len(tabs[1]) == lib.vse_yuv_resample_table_bytes(12, 2)
    assert [lib.vse_yuv_resample_table_bytes(*a) for a in ((0, 2), (-1, 4), (8, 0), (8, 3), (8, 18), (8, 1), (8, -2), (8, 16), (1, 2))] == \
        [0, 0, 0, 0, 0, 0, 0, 8 * 36, 8]
    ok = dict(n=n, h=h, w_in=w_in, w_out=w_out, sub_x=1, sub_y=1, chroma=1, depth=10, msb=0, parity=0, ty=0, ky=2, tc=512, kc=2, sstride=frame_in,
              ostride=frame_out, soff=0, ooff=0, out=None)
    src = torch.zeros(4 * frame_in + 16, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4 * frame_out,), FILL, dtype=torch.uint8, device=ctx.tdev)
    before = table.clone()

    def call(a):
        where = {"src": src.data_ptr(), "table": table.data_ptr()}
        d_out = out.data_ptr() + a["ooff"] if a["out"] is None else where[a["out"][0]] + a["out"][1]
        ptr = lambda v: None if v is None else C.c_void_p(table.data_ptr() + v)      # noqa: E731
        return lib.vse_yuv_resample(ctx.handle, C.c_void_p(src.data_ptr() + a["soff"]), a["n"], a["h"], a["w_in"], a["w_out"], a["sub_x"], a["sub_y"],
                                    a["chroma"], a["depth"], a["msb"], a["parity"], ptr(a["ty"]), a["ky"], ptr(a["tc"]), a["kc"], a["sstride"],
                                    C.c_void_p(d_out), a["ostride"], ctx.stream())
    bad = [dict(h=0), dict(w_in=0), dict(w_out=0), dict(n=0), dict(h=-1), dict(n=-1), dict(w_out=-4), dict(sub_x=0, sub_y=1), dict(sub_x=2),
           dict(sub_y=-1), dict(chroma=3), dict(chroma=-1), dict(chroma=0), dict(chroma=2, sub_y=0), dict(depth=7), dict(depth=17),
           dict(depth=8, msb=1), dict(msb=2), dict(msb=-1), dict(parity=2), dict(parity=-1), dict(sub_y=0, parity=1),
           dict(h=1 << 16, w_in=1 << 15), dict(h=1 << 16, w_out=1 << 15),                       # h * max(w) > 2^31 - 1
           dict(ky=3), dict(ky=0), dict(ky=18), dict(ky=-2), dict(kc=5), dict(kc=0), dict(kc=18),
           dict(ty=None), dict(ty=4), dict(ty=8), dict(tc=None), dict(tc=516), dict(tc=520),
           dict(sstride=frame_in - 2), dict(ostride=frame_out - 2), dict(sstride=frame_in + 1), dict(ostride=frame_out + 1), dict(soff=1), dict(ooff=1),
           dict(out=("src", 0)), dict(out=("src", frame_in)), dict(out=("src", 2 * frame_in - 2)), dict(out=("table", 0)), dict(out=("table", 190)),
           dict(out=("table", 512 + 94))]
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
        msg = lib.vse_last_error().decode()
        assert "vse_yuv_resample" in msg and f"depth {dict(ok, **change)['depth']} " in msg, change
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((src == 0).all()) and bool((table == before).all())
    # the accepted calls next to them do write: all-zero pictures stay all zero, and only the packed bytes are written; a grey picture
    # needs no chroma table, and the output may lie right behind the input pictures
    for more, written in ((dict(), n * frame_out), (dict(sstride=frame_in + 16), n * frame_out),
                          (dict(chroma=0, sub_x=0, sub_y=0, tc=None, kc=0, ostride=2 * h * w_out), n * 2 * h * w_out),
                          (dict(chroma=0, sub_x=0, sub_y=0, tc=4, kc=7, ostride=2 * h * w_out), n * 2 * h * w_out)):
        out.fill_(FILL)
        assert call(dict(ok, **more)) == 0, more
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert np.all(host[:written] == 0) and np.all(host[written:] == FILL), more
    src.fill_(0)
    assert call(dict(ok, n=1, out=("src", frame_in))) == 0
    torch.cuda.synchronize()
    assert bool((src == 0).all())


def test_binding_holds_the_coefficient_bound(ctx):
    import torch
    from vse_amd import engine
    fmt = product_format((0, 0, 0, 8, 0, 0, 0))
    src = torch.zeros(64, dtype=torch.uint8, device=ctx.tdev)
    left = np.zeros(4, np.int64)
    for coef, word in ((np.array([[16384, 16384]] * 3 + [[16384, -16385]]), "32767"), (np.zeros((4, 3), np.int64), "taps even"),
                       (np.zeros((3, 2), np.int64), "left")):
        with pytest.raises(engine.VseError, match=word):
            ctx.yuv_resample(src, 1, 2, 8, fmt, RR.Tables(8, 4, (left, coef), None))
    with pytest.raises(engine.VseError, match="32767"):
        ctx.yuv_resample(src, 1, 2, 8, fmt, RR.Tables(8, 4, (left + (1 << 31) - 1, np.zeros((4, 2), np.int64)), None))
    with pytest.raises(engine.VseError, match="8 stored columns"):
        ctx.yuv_resample(src, 1, 2, 16, fmt, RR.Tables(8, 4, RR.identity(4), None))
    ok = ctx.yuv_resample(src, 1, 2, 8, fmt, RR.Tables(8, 4, (left, np.array([[16384, 16383]] * 4)), None))          # exactly 32767
    assert tuple(ok.shape) == (1, 16)


# ---- staging ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(1, 1, 1, 8, 0, 0, 0), (1, 1, 2, 10, 1, 1, 0), (1, 0, 1, 8, 0, 0, 1)], ids=ident)
def test_uploader_stages_resampled_frames(ctx, fmt):
    from vse_amd import ingest, staging
    h, w, w_out = 46, 70, 82
    rng = np.random.default_rng(53)
    pf = product_format(fmt)
    r = ingest.Resample(w, w_out, "lanczos" if fmt[2] == 2 else "bicubic")
    tabs = RR.tables(w, w_out, fmt, r.filter)
    pics = [R.random_planes(rng, h, w, fmt)]
    for _ in range(5):
        pics.append(D.near_threshold_prev(rng, pics[-1], fmt))
    tone = ingest.ToneMap("pq", "bt709") if fmt[3] == 10 else None
    plain = [ingest.YuvFrame(p, h, w, pf, tone=tone, resample=r) for p in pics]
    whole = [f.to_bgr() for f in plain]
    if tone is None:
        for f, p in zip(whole[:2], pics):
            assert np.array_equal(f, R.convert(RR.picture(p, fmt, *tabs), fmt))                  # the reference, for the host route
    order = "bff" if fmt[2] == 2 else "tff"
    woven = {mode: [ingest.InterlacedYuvFrame(p, h, w, pf, pics[k - 1] if k else None, order, mode, tone=tone, resample=r) for k, p in enumerate(pics)]
             for mode in ("adaptive", "match")}
    if tone is None:
        f = woven["adaptive"][2]
        assert np.array_equal(f.to_bgr(), R.convert(RR.picture(D.picture(f.planes, f.prev, fmt, f.keep), fmt, *tabs), fmt))
    up = staging.Uploader(ctx.tdev, depth=2, ctx=ctx)
    try:
        for rows in (slice(None), slice(23, None), slice(11, 40), slice(12, 13)):
            batch = [f[rows] for f in plain[:4]]
            got = up.stage(batch).tensor()
            want = np.stack([x[rows] for x in whole[:4]])
            assert tuple(got.shape) == want.shape == (4, want.shape[1], w_out, 3) and got.is_contiguous()
            assert np.array_equal(got.cpu().numpy(), want), rows
            for mode in ("adaptive", "match"):
                frames = woven[mode]
                for batch in ([f[rows] for f in frames[1:4]], [f[rows] for f in frames[:3]], [frames[3][rows], frames[1][rows], frames[4][rows]]):
                    got = up.stage(batch).tensor()
                    want = np.stack([f.to_bgr() for f in batch])
                    assert tuple(got.shape) == want.shape and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), (rows, mode)
        # the batch key holds the resample
        for other in (ingest.YuvFrame(pics[1], h, w, pf, tone=tone)[10:20], ingest.YuvFrame(pics[1], h, w, pf, tone=tone, resample=ingest.Resample(w, w_out, "bilinear"))[10:20]):
            with pytest.raises(ValueError, match="resample"):
                up.stage([plain[0][10:20], other])
        with pytest.raises(ValueError, match="resample"):
            up.stage([woven["adaptive"][1][10:20], ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], order, tone=tone)[10:20]])
    finally:
        up.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_extractor_over_a_squeezed_clip_equals_the_host_route(ctx, tmp_path):
    """tests/test_resample.py's clip (640 x 360 squeezed to 540 columns, A32:27): from the file and as a stream in one pass through the
    Uploader (resampled and converted on the device), and through the file source without one (on the host); the change selector on the
    engine every time, the area in display pixels.  Equal intervals, recognised frames, raw lines and SRT."""
    import torch
    from oracle import net_ref, pipeline_ref as P
    from test_one_pass import AREA, piped
    from test_resample import squeezed_clip
    from vse_amd import extractor, frame_select, ingest, pipeline, shim, staging
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")
    path, ref, truth = squeezed_clip(tmp_path)
    nos = {hashlib.sha1(np.ascontiguousarray(f).tobytes()).digest(): no for no, f in enumerate(ref, 1)}

    class EngineOcr:
        def __init__(self):
            self.seen = []

        def predict_batch(self, frames):
            dev = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).to(ctx.tdev)
            self.seen += [nos[hashlib.sha1(f.tobytes()).digest()] for f in dev.cpu().numpy()]
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr(dev)]

        def predict(self, frame):
            return self.predict_batch(np.ascontiguousarray(frame)[None])[0]

    with open(path, "rb") as fp:
        data = fp.read()
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    runs = []
    try:
        for route in ("file", "stream", "host"):
            fp, th = piped(data, 1 << 16) if route == "stream" else (None, None)
            src = ingest.Y4mStream(fp, square_pixels=True) if route == "stream" else ingest.Y4mSource(path, square_pixels=True)
            assert src.resample == ingest.Resample(540, 640)
            ocr = EngineOcr()
            ex = extractor.SubtitleExtractor(src, ocr, sub_area=AREA, mode="auto", drop_score=0.0, batch=8, uploader=None if route == "host" else up,
                                             frame_selector="change", change_counter=frame_select.EngineCounter(ctx))
            assert ex.one_pass == (route == "stream")
            text = ex.run()
            runs.append(([(s, e) for s, e, _r in ex.intervals], ocr.seen, ex.raw_lines, text))
            if route == "stream":
                th.join()
                fp.close()
            else:
                src.close()
    finally:
        up.close()
    assert runs[0] == runs[2] and runs[1] == runs[2]
    assert runs[2][0] == [(s, e) for s, e, _t in truth] and runs[2][1] == [(s + e) // 2 for s, e, _t in truth]
