"""vse_yuv_vscale on the MI355X: every comparison is byte equality with the int64 restatement of the rule (tests/vscale_ref.py), inside
buffers filled with 0xA5 so that a byte written outside a picture shows, and the inputs must come back unchanged.  Random tables that no
filter would produce (top off both picture edges, coefficients of both signs within the bound, sums that clip at both ends, every even K
from 2 to 16) over random full-range words, the general kernel's shapes and the fast kernel's, for 1- and 2-byte samples and every plane
layout; padded and byte-offset calls; whole pictures and row bands of both parities on both sides, cut by the reference's band rule; one
band narrower than the support, which pins the clamp to the band; the identity table; the product's own tables; what the call and the
binding must refuse; staging.Uploader over YuvFrames with vscale=; and SubtitleExtractor over an enlarged Y4M against the host route."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import resample_ref as RR
import vscale_ref as VR
import yuv_format_ref as R
from test_gpu_deinterlace import FORMATS
from test_yuv_formats import ident, product_format

pytestmark = pytest.mark.gpu

FILL = 0xA5
GENERAL_SHAPES = [(1, 1, 1), (3, 2, 2), (4, 5, 3), (23, 17, 5), (41, 34, 7), (37, 50, 37)]           # (w, h_in, h_out)
# the 16-byte kernel's shapes for 1-byte samples: width 32 has 16-byte aligned luma rows (and 16-byte chroma rows of subsampled planar
# formats), width 64 whole 16-byte runs in every plane of every layout; heights 4 .. 12, growing and shrinking
FAST_SHAPES = [(32, 4, 12), (32, 12, 4), (32, 7, 9), (64, 5, 11), (64, 11, 6), (64, 8, 8)]
FAST_SHAPES_2 = [(16, 6, 10), (48, 12, 5)]               # ... and for 2-byte samples
# (name, n, stride padding in samples, base offset in samples)
VARIANTS = [("packed", 1, 0, 0), ("packed", 3, 0, 0), ("padded 16", 3, 16, 0), ("padded odd", 3, 3, 0), ("base + 1", 3, 0, 1), ("base + 2", 1, 5, 2)]
TAPS = VR.TAPS


def run_variant(ctx, rng, fmt, w, h_in, h_out, variant, luma, chroma, rows=None, band=None, stats=None, planes=None, direct=False):
    """One call on pictures laid out as `variant` says, through the tables given: output rows `rows` (default: all) from the band of
    stored rows `band` (default: the whole picture) -> the reference's output planes of every frame.  direct: through lib.vse_yuv_vscale
    itself, past the binding's coverage check."""
    import torch
    _name, n, pad, off = variant
    ss = 1 if fmt[3] == 8 else 2
    (y0, y1), (s0, s1) = rows or (0, h_out), band or (0, h_in)
    frame_in, frame_out = R.packed_bytes(s1 - s0, w, fmt, s0 & fmt[1]), R.packed_bytes(y1 - y0, w, fmt, y0 & fmt[1])
    stride, base = frame_in + pad * ss, off * ss
    pics = planes if planes is not None else [R.random_planes(rng, h_in, w, fmt, wild=True) for _ in range(n)]
    bands = [R.sub_frame(p, fmt, s0, s1)[0] for p in pics]
    host = np.full(base + (n + 1) * stride, FILL, np.uint8)
    for k, p in enumerate(bands):
        host[base + k * stride:base + k * stride + frame_in] = R.pack(p, fmt)
    src = torch.from_numpy(host).to(ctx.tdev)
    packed = src[base:].as_strided((n, stride), (stride, 1))
    ostride = frame_out + (pad + (16 if pad % 16 == 0 else 1)) * ss                  # its own padding: 16-byte aligned where the input's is
    obase = 16 + base
    big = torch.full((obase + (n + 1) * ostride,), FILL, dtype=torch.uint8, device=ctx.tdev)
    out = big[obase:].as_strided((n, ostride), (ostride, 1))
    tables = VR.Tables(h_in, h_out, luma, chroma)
    pf = product_format(fmt)
    if direct:
        dl, dc = ctx.vscale_tables(tables, pf)
        assert ctx.lib.vse_yuv_vscale(ctx.handle, C.c_void_p(packed.data_ptr()), n, w, h_in, h_out, s0, s1, y0, y1, *fmt[:5], C.c_void_p(dl[0].data_ptr()),
                                      dl[1], None if dc is None else C.c_void_p(dc[0].data_ptr()), 0 if dc is None else dc[1], stride,
                                      C.c_void_p(out.data_ptr()), ostride, ctx.stream()) == 0, ctx.lib.vse_last_error()
    else:
        assert ctx.yuv_vscale(packed, n, h_in, w, pf, tables, s0, s1, y0, y1, out=out) is out
    want = np.full(big.numel(), FILL, np.uint8)
    outs = [VR.picture(p, fmt, luma, chroma, h_in, y0, y1, s0, s1, stats) for p in bands]
    for f, o in enumerate(outs):
        assert [q.shape for q in o] == R.plane_shapes(y1 - y0, w, fmt, y0 & fmt[1])
        want[obase + f * ostride:obase + f * ostride + frame_out] = R.pack(o, fmt)
    assert np.array_equal(big.cpu().numpy(), want), (fmt, w, h_in, h_out, variant, rows, band, np.asarray(luma[1]).shape[1])
    assert np.array_equal(src.cpu().numpy(), host)                                   # the inputs are read only
    for dev, raw in zip(ctx.vscale_tables(tables, pf), tables.packed(pf)):           # ... and so are the tables (the context's copies)
        assert (dev is None and raw is None) or dev[0].cpu().numpy().tobytes() == raw
    return outs


def random_tables(rng, fmt, h_in, h_out, k_y, k_c):
    luma = VR.random_table(rng, h_in, h_out, k_y)
    chroma = VR.random_table(rng, VR.chroma_height(h_in, fmt), VR.chroma_height(h_out, fmt), k_c) if fmt[2] else None
    return luma, chroma


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_bit_for_bit_with_sentinels(ctx, fmt):
    rng = np.random.default_rng(sum(fmt) + 3)
    calls = itertools.count()
    stats, seen_y, seen_c, parities, banded = VR.Stats(), set(), set(), set(), 0
    for (w, h_in, h_out), variant in itertools.product(GENERAL_SHAPES + FAST_SHAPES + FAST_SHAPES_2, VARIANTS):
        i = next(calls)
        k_y, k_c = TAPS[i % 8], TAPS[(3 * i + 1) % 8]                                 # both run through every even K, in different orders
        seen_y, seen_c = seen_y | {k_y}, seen_c | {k_c}
        luma, chroma = random_tables(rng, fmt, h_in, h_out, k_y, k_c)
        rows = band = None
        if i % 2 and h_out > 1:                                                       # a band of 1 .. 3 output rows, cut by the reference's rule
            y0 = int(rng.integers(0, h_out))
            rows = (y0, min(h_out, y0 + int(rng.integers(1, 4))))
            band = VR.source_rows(luma, chroma, fmt, h_in, *rows)
            assert VR.covers(luma, chroma, fmt, h_in, *rows, *band)
            parities.add((band[0] & 1, rows[0] & 1))
            banded += band != (0, h_in)
        before = stats.band
        run_variant(ctx, rng, fmt, w, h_in, h_out, variant, luma, chroma, rows, band, stats)
        assert stats.band == before                                                   # a band that covers the support: the second clamp is idle
    # one band narrower than the support, straight through the library: the clamp to the band is what keeps the loads inside
    for (w, h_in, h_out), variant in (((23, 17, 5), VARIANTS[3]), ((64, 11, 6), VARIANTS[1]), ((48, 12, 5), VARIANTS[2])):
        luma, chroma = random_tables(rng, fmt, h_in, h_out, 8, 6)
        run_variant(ctx, rng, fmt, w, h_in, h_out, variant, luma, chroma, (1, 4), (h_in // 2 - 1, h_in // 2 + 2), stats, direct=True)
    # by the reference: both clips, both picture clamps and the band clamp were exercised, with every even K, bands of every parity
    assert seen_y == seen_c == set(TAPS) and stats.low > 100 and stats.high > 100 and stats.above > 20 and stats.below > 20, vars(stats)
    assert stats.band > 20 and banded > 10 and parities == {(0, 0), (0, 1), (1, 0), (1, 1)}, (vars(stats), banded, parities)


@pytest.mark.parametrize("fmt", [f for f in FORMATS if f[1] == 1], ids=ident)
def test_bands_of_odd_parity_on_both_sides(ctx, fmt):
    """4:2:0, 8 -> 6 rows, two frames: stored rows 1:7 in and output rows 1:5 out both begin on an odd row, so each band has one chroma
    row more than half its luma rows.  Straight through the library: the band need not cover the support, the clamp to it is the rule."""
    rng = np.random.default_rng(sum(fmt) + 86)
    luma, chroma = random_tables(rng, fmt, 8, 6, 4, 2)
    run_variant(ctx, rng, fmt, 10, 8, 6, ("packed", 2, 0, 0), luma, chroma, (1, 5), (1, 7), direct=True)


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_identity_and_filter_tables(ctx, fmt):
    """The identity table gives the input bytes (valid samples: the low bits of a high-bit word are zero); ingest.VScale's own tables,
    through the binding's cache, give the reference builder's picture, whole and in a band."""
    from vse_amd import ingest
    rng = np.random.default_rng(sum(fmt) + 11)
    for (w, h, _), variant in itertools.product(GENERAL_SHAPES[1:] + FAST_SHAPES[:2] + FAST_SHAPES_2, (VARIANTS[1], VARIANTS[3])):
        planes = [R.random_planes(rng, h, w, fmt) for _ in range(variant[1])]
        if fmt[4]:
            planes = [tuple(p & np.uint16((0xFFFF << (16 - fmt[3])) & 0xFFFF) for p in f) for f in planes]
        tables = (VR.identity(h), VR.identity(VR.chroma_height(h, fmt)) if fmt[2] else None)
        outs = run_variant(ctx, rng, fmt, w, h, h, variant, *tables, planes=planes)
        assert all(np.array_equal(a, b) for o, f in zip(outs, planes) for a, b in zip(o, f))
    import torch
    pf = product_format(fmt)
    for (w, h_in, h_out), name in zip([(23, 17, 5), (37, 50, 37), (64, 11, 6), (48, 12, 5), (32, 4, 12)], ("bilinear", "lanczos", "bicubic", "bilinear", "bicubic")):
        v = ingest.VScale(h_in, h_out, name)
        tabs = VR.tables(h_in, h_out, fmt, name)
        planes = [R.random_planes(rng, h_in, w, fmt, wild=True) for _ in range(2)]
        for rows in ((0, h_out), (h_out // 2, h_out // 2 + 2)):
            s0, s1 = v.source_rows(pf, *rows)
            assert (s0, s1) == VR.source_rows(*tabs, fmt, h_in, *rows)
            dev = torch.from_numpy(np.concatenate([R.pack(R.sub_frame(p, fmt, s0, s1)[0], fmt) for p in planes])).to(ctx.tdev)
            frame = R.packed_bytes(rows[1] - rows[0], w, fmt, rows[0] & fmt[1])
            for _ in range(2):                                                      # the second call takes the cached device tables
                got = ctx.yuv_vscale(dev, 2, h_in, w, pf, v, s0, s1, *rows).cpu().numpy()
                for f, p in enumerate(planes):
                    assert np.array_equal(got[f, :frame], R.pack(VR.picture(p, fmt, *tabs, h_in, *rows), fmt)), (fmt, name, rows)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import torch
    lib = ctx.lib
    w, h_in, h_out, n = 16, 8, 12, 2
    fmt = (1, 1, 1, 10, 0, 1, 0)
    frame_in, frame_out = R.packed_bytes(h_in, w, fmt), R.packed_bytes(h_out, w, fmt)
    tabs = VR.Tables(h_in, h_out, VR.identity(h_out), VR.identity(h_out // 2)).packed(None)
    table = torch.zeros(1024, dtype=torch.uint8, device=ctx.tdev)                  # luma at 0, chroma at 512
    table[:len(tabs[0])] = torch.from_numpy(np.frombuffer(tabs[0], np.uint8).copy()).to(ctx.tdev)
    table[512:512 + len(tabs[1])] = torch.from_numpy(np.frombuffer(tabs[1], np.uint8).copy()).to(ctx.tdev)
    assert len(tabs[0]) == lib.vse_yuv_resample_table_bytes(h_out, 2) == 96 and len(tabs[1]) == lib.vse_yuv_resample_table_bytes(6, 2) == 48
    ok = dict(n=n, w=w, h_in=h_in, h_out=h_out, s0=0, s1=h_in, y0=0, y1=h_out, sub_x=1, sub_y=1, chroma=1, depth=10, msb=0, ty=0, ky=2, tc=512, kc=2,
              sstride=frame_in, ostride=frame_out, soff=0, ooff=0, out=None)
    src = torch.zeros(4 * frame_in + 16, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4 * frame_out,), FILL, dtype=torch.uint8, device=ctx.tdev)
    before = table.clone()

    def call(a):
        where = {"src": src.data_ptr(), "table": table.data_ptr()}
        d_out = out.data_ptr() + a["ooff"] if a["out"] is None else where[a["out"][0]] + a["out"][1]
        ptr = lambda v: None if v is None else C.c_void_p(table.data_ptr() + v)      # noqa: E731
        return lib.vse_yuv_vscale(ctx.handle, C.c_void_p(src.data_ptr() + a["soff"]), a["n"], a["w"], a["h_in"], a["h_out"], a["s0"], a["s1"], a["y0"],
                                  a["y1"], a["sub_x"], a["sub_y"], a["chroma"], a["depth"], a["msb"], ptr(a["ty"]), a["ky"], ptr(a["tc"]), a["kc"],
                                  a["sstride"], C.c_void_p(d_out), a["ostride"], ctx.stream())
    bad = [dict(n=0), dict(n=-1), dict(w=0), dict(w=-4), dict(h_in=0), dict(h_in=-1), dict(h_out=0), dict(h_out=-3),
           dict(s0=-1), dict(s1=h_in + 1), dict(s0=h_in, s1=h_in), dict(s0=4, s1=4), dict(s0=5, s1=3), dict(s1=0),          # bands outside, or empty
           dict(y0=-1), dict(y1=h_out + 1), dict(y0=h_out, y1=h_out), dict(y0=6, y1=6), dict(y0=7, y1=2), dict(y1=0),
           dict(h_in=1 << 16, w=1 << 15), dict(h_out=1 << 16, w=1 << 15),                                                   # rows * columns > 2^31 - 1
           dict(sub_x=0, sub_y=1), dict(sub_x=2), dict(sub_y=-1), dict(chroma=3), dict(chroma=-1), dict(chroma=0), dict(chroma=2, sub_y=0),
           dict(depth=7), dict(depth=17), dict(depth=8, msb=1), dict(msb=2), dict(msb=-1),
           dict(ky=3), dict(ky=0), dict(ky=18), dict(ky=-2), dict(kc=5), dict(kc=0), dict(kc=18),
           dict(ty=None), dict(ty=4), dict(ty=8), dict(tc=None), dict(tc=516), dict(tc=520),
           dict(sstride=frame_in - 2), dict(ostride=frame_out - 2), dict(sstride=frame_in + 1), dict(ostride=frame_out + 1), dict(soff=1), dict(ooff=1),
           dict(out=("src", 0)), dict(out=("src", frame_in)), dict(out=("src", 2 * frame_in - 2)), dict(out=("table", 0)), dict(out=("table", 94)),
           dict(out=("table", 512 + 46))]
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
        msg = lib.vse_last_error().decode()
        assert msg.startswith("vse_yuv_vscale:") and f"depth {dict(ok, **change)['depth']} " in msg, change
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((src == 0).all()) and bool((table == before).all())
    # the accepted calls next to them do write: all-zero pictures stay all zero, and only the packed bytes are written; a band of either
    # side writes its own packed size; a grey picture needs no chroma table, and the output may lie right behind the input pictures
    band_out = R.packed_bytes(5, w, fmt, 1)
    for more, written in ((dict(), n * frame_out), (dict(sstride=frame_in + 16), n * frame_out),
                          (dict(y0=3, y1=8, ostride=band_out), n * band_out), (dict(s0=1, s1=6, y0=3, y1=8, ostride=band_out), n * band_out),
                          (dict(chroma=0, sub_x=0, sub_y=0, tc=None, kc=0, ostride=2 * h_out * w), n * 2 * h_out * w),
                          (dict(chroma=0, sub_x=0, sub_y=0, tc=4, kc=7, ostride=2 * h_out * w), n * 2 * h_out * w)):
        out.fill_(FILL)
        assert call(dict(ok, **more)) == 0, (more, lib.vse_last_error())
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert np.all(host[:written] == 0) and np.all(host[written:] == FILL), more
    src.fill_(0)
    assert call(dict(ok, n=1, out=("src", frame_in))) == 0
    torch.cuda.synchronize()
    assert bool((src == 0).all())


def test_binding_holds_the_bounds_and_the_coverage(ctx):
    import torch
    from vse_amd import engine
    fmt = product_format((0, 0, 0, 8, 0, 0, 0))
    src = torch.zeros(64, dtype=torch.uint8, device=ctx.tdev)
    top = np.zeros(4, np.int64)
    for coef, word in ((np.array([[16384, 16384]] * 3 + [[16384, -16385]]), "32767"), (np.zeros((4, 3), np.int64), "taps even"),
                       (np.zeros((3, 2), np.int64), "top")):
        with pytest.raises(engine.VseError, match=word):
            ctx.yuv_vscale(src, 1, 8, 2, fmt, VR.Tables(8, 4, (top, coef), None), 0, 8, 0, 4)
    with pytest.raises(engine.VseError, match="32767"):
        ctx.yuv_vscale(src, 1, 8, 2, fmt, VR.Tables(8, 4, (top + (1 << 31) - 1, np.zeros((4, 2), np.int64)), None), 0, 8, 0, 4)
    with pytest.raises(engine.VseError, match="8 stored rows"):
        ctx.yuv_vscale(src, 1, 16, 2, fmt, VR.Tables(8, 4, VR.identity(4), None), 0, 16, 0, 4)
    exact = VR.Tables(8, 4, (top, np.array([[16384, 16383]] * 4)), None)                     # exactly 32767; every row reads stored rows 0 and 1
    ok = ctx.yuv_vscale(src, 1, 8, 2, fmt, exact, 0, 8, 0, 4)
    assert tuple(ok.shape) == (1, 16)
    assert tuple(ctx.yuv_vscale(src, 1, 8, 2, fmt, exact, 0, 2, 1, 3).shape) == (1, 16)     # the smallest band that covers them
    for band, rows in (((1, 8), (0, 4)), ((0, 1), (2, 3)), ((2, 8), (3, 4))):
        with pytest.raises(engine.VseError, match="does not cover the support"):
            ctx.yuv_vscale(src, 1, 8, 2, fmt, exact, *band, *rows)
    for band, rows in (((0, 9), (0, 4)), ((-1, 8), (0, 4)), ((3, 3), (0, 4)), ((0, 8), (0, 5)), ((0, 8), (2, 2))):
        with pytest.raises(engine.VseError, match="inside their pictures"):
            ctx.yuv_vscale(src, 1, 8, 2, fmt, exact, *band, *rows)
    # chroma rows count too: 4:2:0, luma needs stored rows 0 and 1 only, chroma row 3 (stored luma rows 6 and 7)
    fmt420 = product_format((1, 1, 1, 8, 0, 0, 0))
    chroma = (np.full(2, 3, np.int64), np.array([[16384, 0]] * 2))
    both = VR.Tables(8, 4, (top, np.array([[16384, 16383]] * 4)), chroma)
    with pytest.raises(engine.VseError, match="chroma rows 0:1, .* read chroma rows 3:4"):
        ctx.yuv_vscale(src, 1, 8, 2, fmt420, both, 0, 2, 0, 4)
    assert tuple(ctx.yuv_vscale(src, 1, 8, 2, fmt420, both, 0, 7, 0, 4).shape) == (1, 16)


# ---- staging ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(1, 1, 1, 8, 0, 0, 0), (1, 1, 2, 10, 1, 1, 0), (1, 0, 1, 8, 0, 0, 1)], ids=ident)
def test_uploader_stages_scaled_frames(ctx, fmt):
    from vse_amd import ingest, staging
    h, h_out, w, w_out = 70, 46, 70, 52
    rng = np.random.default_rng(53)
    pf = product_format(fmt)
    name = "lanczos" if fmt[2] == 2 else "bicubic"
    v = ingest.VScale(h, h_out, name)
    pics = [R.random_planes(rng, h, w, fmt) for _ in range(4)]
    tone = ingest.ToneMap("pq", "bt709") if fmt[3] == 10 else None
    up = staging.Uploader(ctx.tdev, depth=2, ctx=ctx)
    try:
        for r in (None, ingest.Resample(w, w_out, name)):
            frames = [ingest.YuvFrame(p, h, w, pf, tone=tone, resample=r, vscale=v) for p in pics]
            whole = [f.to_bgr() for f in frames]
            if tone is None:                                                          # the reference, for the host route
                rows = VR.picture(pics[0], fmt, *VR.tables(h, h_out, fmt, name), h, 0, h_out)
                rows = rows if r is None else RR.picture(rows, fmt, *RR.tables(w, w_out, fmt, name))
                assert np.array_equal(whole[0], R.convert(rows, fmt))
            for cut in (slice(None), slice(23, None), slice(11, 40), slice(12, 13)):
                got = up.stage([f[cut] for f in frames]).tensor()
                want = np.stack([x[cut] for x in whole])
                assert tuple(got.shape) == want.shape == (4, want.shape[1], w if r is None else w_out, 3) and got.is_contiguous()
                assert np.array_equal(got.cpu().numpy(), want), (cut, r)
        # the batch key holds the vscale and the first output row
        for other in (ingest.YuvFrame(pics[1], h, w, pf, tone=tone, resample=r)[10:20],
                      ingest.YuvFrame(pics[1], h, w, pf, tone=tone, resample=r, vscale=ingest.VScale(h, h_out, "bilinear"))[10:20],
                      frames[1][11:21], frames[1][12:22]):
            with pytest.raises(ValueError, match="vscale"):
                up.stage([frames[0][10:20], other])
        got = up.stage([frames[0][10:20], frames[1][10:20]]).tensor()
        assert np.array_equal(got.cpu().numpy(), np.stack([whole[0][10:20], whole[1][10:20]]))
    finally:
        up.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_extractor_over_an_enlarged_clip_equals_the_host_route(ctx, tmp_path):
    """tests/test_vscale.py's clip (640 x 360 enlarged to 1280 x 720): from the file and as a stream in one pass through the Uploader
    (scaled both ways and converted on the device), and through the file source without one (on the host); the change selector on the
    engine every time, the area in output pixels.  Equal intervals, recognised frames, raw lines and SRT."""
    import torch
    from oracle import net_ref, pipeline_ref as P
    from test_one_pass import AREA, piped
    from test_vscale import enlarged_clip
    from vse_amd import extractor, frame_select, ingest, pipeline, shim, staging
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")
    path, ref, truth = enlarged_clip(tmp_path)
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
            src = ingest.Y4mStream(fp, scale=360) if route == "stream" else ingest.Y4mSource(path, scale=360)
            assert (src.vscale, src.resample) == (ingest.VScale(720, 360), ingest.Resample(1280, 640))
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
