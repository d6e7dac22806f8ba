"""The vertical scale for UHD and other oversized YUV on the host: ingest.VScale's tables against the reference builder over the heights,
its validation, the integers of vse_yuv_vscale in YuvFrame.to_bgr() against the int64 restatement of tests/vscale_ref.py (vertical, then
horizontal, then the conversion), row slices, the band rule and its minimality, the sources' scale= option, what they refuse, both command
lines with a scripted recogniser, and the change selector over a clip enlarged twofold and read back with scale=360.  CPU only."""
import logging

import numpy as np
import pytest

import area_cells_ref
import resample_ref as RR
import vscale_ref as VR
import yuv_format_ref as R
from frame_change_ref import NumpyCounter
from test_gpu_deinterlace import FORMATS
from test_one_pass import AREA, FPS, LookupOcr, clip, host_stack, piped, run, text_box  # noqa: F401  (host_stack is a fixture)
from test_yuv_formats import bgr_source, ident, product_format
from vse_amd import area_locator, extractor, frame_select, ingest

FMT420 = (1, 1, 1, 8, 0, 0, 0)
# (stored, output) plane heights: the issue's, the GPU test's shapes (tiny, odd, growing and shrinking) and the chroma heights of them
HEIGHTS = [(2160, 1080), (1080, 720), (720, 1080), (480, 1080), (1080, 540), (540, 360), (360, 540), (240, 540), (1, 1), (2, 2), (5, 3), (17, 5),
           (34, 7), (50, 37), (3, 2), (9, 3), (17, 4), (25, 19), (4, 12), (12, 4), (5, 11), (11, 6), (8, 7), (2, 6), (6, 2), (3, 6), (6, 3), (4, 4)]


# ---- the tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RR.FILTERS)
def test_tables_equal_the_reference_builder(name):
    fmt, built = product_format(FMT420), 0
    for h_in, h_out in HEIGHTS:
        ch_in, ch_out = VR.chroma_height(h_in, FMT420), VR.chroma_height(h_out, FMT420)
        if max(RR.taps_needed(h_in, h_out, name), RR.taps_needed(ch_in, ch_out, name)) > 16:
            with pytest.raises(ValueError, match="taps"):
                ingest.VScale(h_in, h_out, name).tables(fmt)
            continue
        built += 1
        got, want = ingest.VScale(h_in, h_out, name).tables(fmt), VR.tables(h_in, h_out, FMT420, name)
        for (top, coef), (want_top, want_coef) in zip(got, want):
            assert top.dtype == np.int32 and coef.dtype == np.int16 and not top.flags.writeable and not coef.flags.writeable
            assert np.array_equal(top, want_top) and np.array_equal(coef, want_coef), (name, h_in, h_out)
            assert np.all(coef.astype(np.int64).sum(axis=1) == 16384) and np.abs(coef.astype(np.int64)).sum(axis=1).max() <= 32767
        assert got[0][0].shape == (h_out,) and got[1][0].shape == (ch_out,)
    assert built >= 20


def test_vscale_is_a_hashable_validated_tuple():
    a, b = ingest.VScale(2160, 1080), ingest.VScale(2160, 1080, "bicubic")
    assert a == b and hash(a) == hash(b) and a != ingest.VScale(2160, 1080, "lanczos") and len({a, b}) == 1
    assert (a.in_height, a.out_height, a.filter) == (2160, 1080, "bicubic")
    fmt, grey = product_format(FMT420), product_format((0, 0, 0, 8, 0, 0, 0))
    assert a.tables(fmt) is b.tables(fmt) and a.tables(fmt)[0][1].shape == (1080, 8) and a.tables(fmt)[1][0].shape == (540,)
    assert a.tables(grey)[1] is None and a.packed(grey)[1] is None
    full = a.tables(product_format((0, 0, 1, 8, 0, 0, 0)))                               # 4:4:4: the chroma planes have the luma's rows
    assert np.array_equal(full[1][0], full[0][0]) and np.array_equal(full[1][1], full[0][1])
    luma, chroma = a.packed(fmt)
    assert len(luma) == 1080 * (4 + 2 * 8) and len(chroma) == 540 * (4 + 2 * 8)
    assert np.array_equal(np.frombuffer(luma, "<i4", 1080), a.tables(fmt)[0][0])
    assert np.array_equal(np.frombuffer(luma, "<i2", offset=4 * 1080).reshape(1080, 8), a.tables(fmt)[0][1])
    with pytest.raises(ValueError, match=r"'lanczos' from 2160 to 540 columns needs 24 taps"):     # the existing error of the builder
        ingest.VScale(2160, 540, "lanczos")
    with pytest.raises(ValueError, match=r"'bicubic' from 100 to 20 columns needs 20 taps"):
        ingest.VScale(100, 20)
    assert ingest.VScale(2160, 540, "bicubic").tables(fmt)[0][1].shape == (540, 16)
    for bad in (dict(filter="nearest"), dict(in_height=0), dict(out_height=-3), dict(in_height=7.5), dict(out_height=True)):
        with pytest.raises(ValueError, match="vscale"):
            ingest.VScale(**{**dict(in_height=720, out_height=480), **bad})
    rng = np.random.default_rng(2)
    planes = R.random_planes(rng, 6, 8, FMT420)
    with pytest.raises(ValueError, match="stored rows"):
        ingest.YuvFrame(planes, 6, 8, fmt, vscale=ingest.VScale(8, 4))
    with pytest.raises(ValueError, match="vscale must be"):
        ingest.YuvFrame(planes, 6, 8, fmt, vscale=(6, 4))
    with pytest.raises(ValueError, match="vscale"):
        ingest.InterlacedYuvFrame(planes, 6, 8, fmt, vscale=ingest.VScale(6, 4))
    with pytest.raises(ValueError):                                                   # y1 counts output rows
        ingest.YuvFrame(planes, 6, 8, fmt, y1=5, vscale=ingest.VScale(6, 4))


def test_identity_scale_is_the_identity():
    rng = np.random.default_rng(7)
    for fmt in FORMATS:
        pf = product_format(fmt)
        for name in RR.FILTERS:
            v = ingest.VScale(37, 37, name)
            for top, coef in (t for t in v.tables(pf) if t is not None):
                assert np.array_equal(RR.dense(top, coef, len(top)), 16384 * np.eye(len(top), dtype=np.int64))
        planes = R.random_planes(rng, 37, 6, fmt)
        if fmt[4]:
            planes = tuple(p & np.uint16((0xFFFF << (16 - fmt[3])) & 0xFFFF) for p in planes)
        assert all(np.array_equal(a, b) for a, b in zip(ingest.VScale(37, 37).planes(pf, planes), planes))
        ident_tables = (VR.identity(37), VR.identity(VR.chroma_height(37, fmt)) if fmt[2] else None)
        assert all(np.array_equal(a, b) for a, b in zip(VR.picture(planes, fmt, *ident_tables, 37, 0, 37), planes))
        frame = ingest.YuvFrame(planes, 37, 6, pf, vscale=ingest.VScale(37, 37))
        assert frame.band() == (0, 37) and frame[5:8].band() == (5, 8) and np.array_equal(frame.to_bgr(), ingest.YuvFrame(planes, 37, 6, pf).to_bgr())


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------
def reference_bgr(planes, fmt, h_in, h_out, name, w_out=None, tone=None):
    """Vertical, then horizontal, then the conversion, all by the references."""
    rows = VR.picture(planes, fmt, *VR.tables(h_in, h_out, fmt, name), h_in, 0, h_out)
    if w_out is not None:
        rows = RR.picture(rows, fmt, *RR.tables(planes[0].shape[1], w_out, fmt, name))
    if tone is not None:
        import tonemap_ref as TM
        return TM.convert(rows, fmt, *tone.tables())
    return R.convert(rows, fmt)


SLICES = ((0, 1), (0, 4), (3, 8), (5, 12), (2, 3), (7, 8), (6, 13), (12, 13), (11, 13), (0, 13))


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_frames_convert_as_the_reference_scales(fmt):
    rng = np.random.default_rng(sum(fmt) + 5)
    pf = product_format(fmt)
    for (h_in, h_out, w, w_out), name in (((25, 13, 10, None), "bicubic"), ((25, 13, 14, 9), "lanczos"), ((9, 13, 11, 16), "bilinear")):
        planes = R.random_planes(rng, h_in, w, fmt)
        v = ingest.VScale(h_in, h_out, name)
        r = None if w_out is None else ingest.Resample(w, w_out, name)
        frame = ingest.YuvFrame(planes, h_in, w, pf, resample=r, vscale=v)
        want = reference_bgr(planes, fmt, h_in, h_out, name, w_out)
        assert frame.shape == (h_out, w_out or w, 3) and (frame.height, frame.width, frame.y0, frame.y1) == (h_in, w, 0, h_out)
        assert np.array_equal(frame.to_bgr(), want), (name, h_in, h_out)
        assert frame.band() == v.source_rows(pf, 0, h_out) == (0, h_in) and frame.packed_bytes == R.packed_bytes(h_in, w, fmt)
        for a, b in SLICES:
            cut = frame[a:b]
            assert (cut.vscale, cut.resample, cut.y0, cut.y1) == (v, r, a, b) and cut.shape == (b - a, w_out or w, 3)
            assert np.array_equal(cut.to_bgr(), want[a:b]), (a, b)
            assert np.array_equal(cut[1:].to_bgr(), want[a + 1:b]) and cut[1:].y0 == a + 1                  # a slice of a slice
            s0, s1 = cut.band()
            assert (s0, s1) == VR.source_rows(*VR.tables(h_in, h_out, fmt, name), fmt, h_in, a, b) and cut.row_parity == s0 & fmt[1]
            buf = np.zeros(cut.packed_bytes + 3, np.uint8)
            assert cut.pack_into(buf) == cut.packed_bytes == R.packed_bytes(s1 - s0, w, fmt, s0 & fmt[1])    # the packing is the stored band's
            assert np.array_equal(buf[:-3], R.pack(R.sub_frame(planes, fmt, s0, s1)[0], fmt)) and not buf[-3:].any()
            # the reference on that band alone, through both clamps, gives the whole picture's rows
            band = VR.picture(R.sub_frame(planes, fmt, s0, s1)[0], fmt, *VR.tables(h_in, h_out, fmt, name), h_in, a, b, s0, s1)
            whole = VR.picture(planes, fmt, *VR.tables(h_in, h_out, fmt, name), h_in, a, b)
            assert all(np.array_equal(p, q) for p, q in zip(band, whole))
    # without a vscale every attribute is the stored picture's
    plain = ingest.YuvFrame(planes, h_in, w, pf)[3:8]
    assert plain.vscale is None and plain.band() == (3, 8) and plain.row_parity == 3 & fmt[1] and plain.shape == (5, w, 3)


def test_tone_map_follows_the_scale():
    fmt = (1, 1, 1, 10, 0, 2, 0)
    rng = np.random.default_rng(9)
    planes = R.random_planes(rng, 20, 34, fmt)
    tone = ingest.ToneMap("pq")
    for r, w_out in ((None, None), (ingest.Resample(34, 17), 17)):
        frame = ingest.YuvFrame(planes, 20, 34, product_format(fmt), tone=tone, resample=r, vscale=ingest.VScale(20, 10))
        want = reference_bgr(planes, fmt, 20, 10, "bicubic", w_out, tone)
        assert np.array_equal(frame.to_bgr(), want) and np.array_equal(frame[3:6].to_bgr(), want[3:6]) and frame[3:6].tone == tone


@pytest.mark.parametrize("fmt", [FMT420, (1, 0, 1, 8, 0, 0, 0), (0, 0, 0, 8, 0, 0, 0), (1, 1, 2, 10, 1, 2, 0)], ids=ident)
def test_band_is_minimal(fmt):
    """band() holds what the rows need in every plane, and neither its first nor its last row can go: by the reference's own account
    of which stored rows a row reads, and by the bytes for the whole picture."""
    pf = product_format(fmt)
    rng = np.random.default_rng(sum(fmt) + 1)
    parities = set()
    for (h_in, h_out), name in (((50, 37), "bicubic"), ((37, 50), "lanczos"), ((48, 24), "bilinear"), ((48, 24), "bicubic"), ((49, 20), "bilinear")):
        v = ingest.VScale(h_in, h_out, name)
        tabs = VR.tables(h_in, h_out, fmt, name)
        planes = R.random_planes(rng, h_in, 6, fmt)
        whole = VR.picture(planes, fmt, *tabs, h_in, 0, h_out)
        for y0, y1 in [(0, h_out), (0, 1), (h_out - 1, h_out), (0, 2), (h_out - 3, h_out)] + [(a, a + n) for a in range(1, h_out - 6, 3) for n in (1, 2, 5)]:
            s0, s1 = v.source_rows(pf, y0, y1)
            parities.add((s0 & 1, y0 & 1))
            assert 0 <= s0 < s1 <= h_in and VR.covers(*tabs, fmt, h_in, y0, y1, s0, s1), (y0, y1, s0, s1)
            assert s1 - s0 == 1 or (not VR.covers(*tabs, fmt, h_in, y0, y1, s0 + 1, s1) and not VR.covers(*tabs, fmt, h_in, y0, y1, s0, s1 - 1))
            assert (s0, s1) == VR.source_rows(*tabs, fmt, h_in, y0, y1)
            if y0 % 3 == 1 and y1 - y0 == 2:
                got = VR.picture(R.sub_frame(planes, fmt, s0, s1)[0], fmt, *tabs, h_in, y0, y1, s0, s1)
                c0, c1 = VR.chroma_rows(y0, y1, fmt)
                assert np.array_equal(got[0], whole[0][y0:y1]) and all(np.array_equal(g, p[c0:c1]) for g, p in zip(got[1:], whole[1:]))
    assert parities == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert ingest.VScale(48, 24).source_rows(pf, 5, 5) == (0, 0)                          # no rows asked, none packed


# ---- the sources ----------------------------------------------------------------------------------------------------------------------
def small_clip(tmp_path, aspect=(1, 1), fmt=FMT420, w=34, h=24, name="clip.y4m", count=3):
    rng = np.random.default_rng(4)
    frames = [R.random_planes(rng, h, w, fmt) for _ in range(count)]
    path = str(tmp_path / name)
    ingest.write_yuv(path, frames, product_format(fmt), fps=FPS, y4m=True, aspect=aspect)
    return path, frames


def test_sources_attach_vscale_and_resample(tmp_path, caplog):
    caplog.set_level(logging.INFO, logger="vse_amd.ingest")
    path, frames = small_clip(tmp_path)
    # scale=H keeps the display aspect: 34 * 12 / 24 = 17 -> the nearest even number, 18 (a tie goes up)
    want = [reference_bgr(p, FMT420, 24, 12, "bicubic", 18) for p in frames]
    for wide in (False, True):
        for src in (ingest.Y4mSource(path, wide=wide, scale=12), ingest.open_source(path, wide=wide, scale=12)):
            assert src.vscale == ingest.VScale(24, 12) and src.resample == ingest.Resample(34, 18) and (src.width, src.height) == (34, 24)
            assert src.fmt == product_format(FMT420)
            for no, raw in enumerate(src.raw_frames(), 1):
                assert type(raw) is ingest.YuvFrame and (raw.vscale, raw.resample) == (src.vscale, src.resample) and raw.shape == (12, 18, 3)
                assert np.array_equal(raw.to_bgr(), want[no - 1]) and np.array_equal(src.read(no), want[no - 1])
            src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    fp, th = piped(data, 7)
    st = ingest.Y4mStream(fp, scale=12)
    assert (st.vscale, st.resample) == (ingest.VScale(24, 12), ingest.Resample(34, 18))
    assert [np.array_equal(f, x) for f, x in zip(st.frames(), want)] == [True] * 3
    th.join()
    fp.close()
    # scale=(W, H) says both, and resample_filter picks the tables of both passes
    src = ingest.Y4mSource(path, scale=(20, 16), resample_filter="lanczos")
    assert (src.vscale, src.resample) == (ingest.VScale(24, 16, "lanczos"), ingest.Resample(34, 20, "lanczos"))
    assert np.array_equal(src.read(2), reference_bgr(frames[1], FMT420, 24, 16, "lanczos", 20))
    src.close()
    # only one of the two where the other size is the stored one
    src = ingest.Y4mSource(path, scale=(34, 12))
    assert (src.vscale, src.resample) == (ingest.VScale(24, 12), None) and src.read_raw(1).shape == (12, 34, 3)
    assert np.array_equal(src.read(3), reference_bgr(frames[2], FMT420, 24, 12, "bicubic"))
    src.close()
    src = ingest.Y4mSource(path, scale=(18, 24))
    assert (src.vscale, src.resample) == (None, ingest.Resample(34, 18)) and src.read_raw(1).shape == (24, 18, 3)
    src.close()
    assert not caplog.records
    # with square_pixels the display width is the ratio's: 34 * 32 / 27 -> 40 columns shown, 40 * 12 / 24 = 20; ONE table from 34 to 20
    squeezed, planes = small_clip(tmp_path, (32, 27), name="squeezed.y4m")
    for kw in (dict(square_pixels=True), dict(sar=(32, 27))):
        src = ingest.Y4mSource(squeezed, scale=12, **kw)
        assert (src.vscale, src.resample) == (ingest.VScale(24, 12), ingest.Resample(34, 20))
        assert np.array_equal(src.read(1), reference_bgr(planes[0], FMT420, 24, 12, "bicubic", 20))
        src.close()
    src = ingest.Y4mSource(squeezed, scale=12)                                          # ... and without it the stored one
    assert src.resample == ingest.Resample(34, 18)
    src.close()
    # headerless files
    p010 = (1, 1, 2, 10, 1, 1, 0)
    rng = np.random.default_rng(8)
    planes = [R.random_planes(rng, 24, 34, p010) for _ in range(2)]
    raw_path = str(tmp_path / "clip.p010")
    ingest.write_yuv(raw_path, planes, product_format(p010))
    src = ingest.open_source(raw_path, size=(34, 24), fps=FPS, matrix="bt709", scale=16)
    assert isinstance(src, ingest.YuvSource) and (src.vscale, src.resample) == (ingest.VScale(24, 16), ingest.Resample(34, 22))
    assert np.array_equal(src.read(2), reference_bgr(planes[1], p010, 24, 16, "bicubic", 22))
    src.close()
    nv12 = (1, 1, 2, 8, 0, 0, 0)
    planes = [R.random_planes(rng, 24, 34, nv12) for _ in range(2)]
    yuv_path = str(tmp_path / "clip.nv12")
    ingest.write_yuv(yuv_path, planes, product_format(nv12))
    src = ingest.open_source(yuv_path, size=(34, 24), fps=FPS, scale=(34, 12))
    assert isinstance(src, ingest.YuvSource) and (src.vscale, src.resample) == (ingest.VScale(24, 12), None) and src.fmt == product_format(nv12)
    assert np.array_equal(src.read(1), reference_bgr(planes[0], nv12, 24, 12, "bicubic"))
    src.close()


def test_no_op_scale_gives_todays_frames(tmp_path, caplog):
    path, _ = small_clip(tmp_path)
    caplog.set_level(logging.INFO, logger="vse_amd.ingest")
    for kw in (dict(scale=24), dict(scale=(34, 24)), dict(scale=24, resample_filter="lanczos")):
        caplog.clear()
        a, b = ingest.Y4mSource(path, **kw), ingest.Y4mSource(path)
        assert a.vscale is None and a.resample is None and a.fmt is None
        lines = [r.getMessage() for r in caplog.records]
        assert len(lines) == 1 and "34 x 24" in lines[0] and "left as stored" in lines[0], lines
        for x, y in zip(a.raw_frames(), b.raw_frames()):
            assert type(x) is ingest.Yuv420Frame and x.shape == y.shape and np.array_equal(x.to_bgr(), y.to_bgr())
            buf_a, buf_b = np.zeros(x.packed_bytes, np.uint8), np.zeros(y.packed_bytes, np.uint8)
            x.pack_into(buf_a), y.pack_into(buf_b)
            assert np.array_equal(buf_a, buf_b)
        a.close()
        b.close()
    caplog.clear()
    st = ingest.Y4mStream(open(path, "rb"), scale=24)
    assert st.vscale is None and st.resample is None and type(next(st.raw_frames())) is ingest.Yuv420Frame and len(caplog.records) == 1
    raw = str(tmp_path / "clip.yuv")
    rng = np.random.default_rng(3)
    ingest.write_yuv420(raw, [R.random_planes(rng, 24, 34, FMT420)])
    caplog.clear()
    src = ingest.open_source(raw, size=(34, 24), fps=FPS, scale=24)
    assert isinstance(src, ingest.Yuv420Source) and type(src.read_raw(1)) is ingest.Yuv420Frame and len(caplog.records) == 1
    src.close()
    caplog.clear()
    src = ingest.open_source(raw, size=(34, 24), fps=FPS, scale=12)                       # ... and none where it scales
    assert isinstance(src, ingest.YuvSource) and src.vscale == ingest.VScale(24, 12) and not caplog.records
    src.close()
    src = ingest.open_source(path)                                                      # off: nothing attached, nothing logged
    assert src.vscale is None and src.resample is None and type(src.read_raw(1)) is ingest.Yuv420Frame and not caplog.records
    src.close()


def test_refusals_name_the_option(tmp_path):
    path, _ = small_clip(tmp_path)
    npy = str(tmp_path / "clip.npy")
    np.save(npy, np.zeros((1, 4, 6, 3), np.uint8))
    for call, word in ((lambda: ingest.Y4mSource(path, scale=0), "scale must be"), (lambda: ingest.Y4mSource(path, scale=(12,  0)), "scale must be"),
                       (lambda: ingest.Y4mSource(path, scale="12"), "scale must be"), (lambda: ingest.Y4mSource(path, scale=(1, 2, 3)), "scale must be"),
                       (lambda: ingest.Y4mSource(path, scale=12.0), "scale must be"), (lambda: ingest.Y4mSource(path, scale=True), "scale must be"),
                       (lambda: ingest.Y4mStream(open(path, "rb"), scale=-4), "scale must be"),
                       (lambda: ingest.open_source(path, scale=(0, 12)), "scale must be"),
                       (lambda: ingest.Y4mSource(path, scale=12, resample_filter="nearest"), "resample_filter"),
                       (lambda: ingest.Y4mSource(path, resample_filter="lanczos"), "resample_filter belongs"),
                       (lambda: ingest.Y4mSource(path, wide=True, deinterlace="adaptive", field_order="tff", scale=12), "scale does not go with deinterlace"),
                       (lambda: ingest.Y4mStream(open(path, "rb"), wide=True, deinterlace="match", field_order="tff", scale=12),
                        "scale does not go with deinterlace"),
                       (lambda: ingest.open_source(path, wide=True, deinterlace="adaptive", field_order="tff", scale=(34, 12)),
                        "scale does not go with deinterlace"),
                       (lambda: ingest.YuvSource(path, 34, 24, FPS, product_format(FMT420), deinterlace="interpolate", field_order="bff", scale=12),
                        "scale does not go with deinterlace"),
                       (lambda: ingest.open_source(npy, fps=FPS, scale=2), "scale takes YUV4MPEG2"),
                       (lambda: ingest.open_source(str(tmp_path / "film.avi"), scale=(6, 2)), "scale takes YUV4MPEG2"),
                       (lambda: ingest.Y4mSource(path, scale=2, resample_filter="lanczos"), r"'lanczos' from 24 to 2 columns needs 72 taps"),
                       (lambda: ingest.Y4mSource(path, scale=(4, 24)), r"'bicubic' from 34 to 4 columns needs 34 taps")):
        with pytest.raises(ValueError, match=word):
            call()


# ---- the command lines and the end-to-end run -------------------------------------------------------------------------------------------
_enlarged = {}


def enlarged_clip(tmp_path, name="bicubic"):
    """The change clip (640 x 360) enlarged to 1280 x 720 by repeating every sample of every plane twice each way, in a Y4M -> (path, the
    frames Y4mSource(scale=360, resample_filter=name) gives on the host, truth)."""
    frames, truth = clip("change")
    if "planes" not in _enlarged:
        _enlarged["planes"] = [tuple(np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in ingest.bgr_to_yuv420(f)) for f in frames]
    path = str(tmp_path / "enlarged.y4m")
    ingest.write_yuv(path, _enlarged["planes"], product_format(FMT420), fps=FPS, y4m=True)
    if name not in _enlarged:
        src = ingest.Y4mSource(path, scale=360, resample_filter=name)
        assert (src.width, src.height, src.frame_count) == (1280, 720, len(frames))
        assert (src.vscale, src.resample) == (ingest.VScale(720, 360, name), ingest.Resample(1280, 640, name))
        _enlarged[name] = list(src.frames())
        src.close()
    return path, _enlarged[name], truth


@pytest.mark.parametrize("name", RR.FILTERS)
def test_enlarged_clip_keeps_its_intervals(tmp_path, name):
    """The host route end to end: the frames come out 640 x 360, and the change selector with the numpy counter over AREA finds the
    original clip's three intervals.  The round-trip difference is printed (EXPERIMENTS.md AG), not asserted."""
    frames, truth = clip("change")
    _path, decoded, _ = enlarged_clip(tmp_path, name)
    assert all(f.shape == (360, 640, 3) and f.dtype == np.uint8 for f in decoded) and len(decoded) == len(frames)
    diff = np.abs(np.stack(decoded).astype(np.int16) - frames)
    print(f"640x360 -> 1280x720 (sample repeat) -> 640x360 {name}, 8-bit 4:2:0: max |diff| {diff.max()}, mean {diff.mean():.4f} levels against "
          "the original clip")

    def intervals(fr):
        return [(s, e) for s, e, _rep in frame_select.ChangeFrameSelector(NumpyCounter(), batch=8).run(list(fr), AREA, FPS)]
    want = intervals(frames)
    assert want == [(s, e) for s, e, _t in truth] and len(want) == 3
    assert intervals(decoded) == want


def test_extractor_command_line_takes_scale(host_stack, tmp_path, monkeypatch, capsys):
    path, decoded, truth = enlarged_clip(tmp_path)
    _, want = run(bgr_source(decoded), decoded, truth, "change", 8, None)
    assert want[3].count(" --> ") == len(truth)
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"               # output pixels: the area of the 640 x 360 picture
    common = ["--area", area, "--selector", "change", "--batch", "8"]
    out = str(tmp_path / "out.srt")
    for flags in (["--scale", "360"], ["--scale", "640x360"], ["--scale", "360", "--resample-filter", "bicubic"], ["--wide-yuv", "--scale", "640X360"]):
        ocr = LookupOcr(decoded, truth, text_box(AREA))
        assert extractor.main([path, "-o", out] + flags + common, ocr=ocr, counter=NumpyCounter()) == 0, flags
        assert open(out).read() == want[3] and ocr.seen == want[1]
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 4099)
    monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main(["-", "--scale", "360"] + common, ocr=ocr, counter=NumpyCounter()) == 0
    pipe.close()
    th.join()
    assert capsys.readouterr().out == want[3]
    # the options reach the source
    args = type("Args", (), dict(square_pixels=False, sar=None, resample_filter="lanczos", scale="480"))()
    assert extractor.square_arguments(args) == dict(scale=480, resample_filter="lanczos")
    src = ingest.open_source(path, **extractor.square_arguments(args))
    assert (src.vscale, src.resample) == (ingest.VScale(720, 480, "lanczos"), ingest.Resample(1280, 854, "lanczos"))
    src.close()
    args = type("Args", (), dict(square_pixels=True, sar="4:3", resample_filter=None, scale="960x540"))()
    assert extractor.square_arguments(args) == dict(square_pixels=True, sar=(4, 3), resample_filter="bicubic", scale=(960, 540))
    assert extractor.square_arguments(type("Args", (), dict(square_pixels=False, sar=None, resample_filter=None, scale=None))()) == {}
    # refusals: exit status 2 and the message on standard error, nothing recognised
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    np.save(str(tmp_path / "clip.npy"), np.zeros((1, 4, 6, 3), np.uint8))
    for argv, word in (([path, "--scale", "0"], "--scale takes"), ([path, "--scale", "640x"], "--scale takes"), ([path, "--scale", "a"], "--scale takes"),
                       ([path, "--scale", "1x2x3"], "--scale takes"), ([path, "--resample-filter", "lanczos"], "--resample-filter belongs"),
                       ([path, "--scale", "90", "--resample-filter", "lanczos"], "taps"),
                       ([path, "--wide-yuv", "--deinterlace", "adaptive", "--field-order", "tff", "--scale", "360"], "scale does not go with deinterlace"),
                       ([str(tmp_path / "clip.npy"), "--fps", "12", "--scale", "2"], "scale takes YUV4MPEG2")):
        assert extractor.main(argv + common, ocr=ocr, counter=NumpyCounter()) == 2 and ocr.seen == [], argv
        err = capsys.readouterr().err
        assert err.startswith("extractor: ") and word in err, (argv, err)


def test_locator_command_line_takes_scale(tmp_path, capsys):
    path, decoded, _ = enlarged_clip(tmp_path)
    want = area_locator.AreaLocator(area_cells_ref.NumpyCells()).run(decoded, FPS)
    assert want is not None
    for flags in (["--scale", "360"], ["--scale", "640x360", "--resample-filter", "bicubic"]):
        assert area_locator.main([path] + flags, cells_fn=area_cells_ref.NumpyCells()) == 0
        assert capsys.readouterr().out.split() == [str(v) for v in (want.ymin, want.ymax, want.xmin, want.xmax)]
    assert area_locator.main([path, "--scale", "x360"], cells_fn=area_cells_ref.NumpyCells()) == 2
    assert "--scale takes" in capsys.readouterr().err
    assert area_locator.main([path, "--resample-filter", "bilinear"], cells_fn=area_cells_ref.NumpyCells()) == 2
    assert "--resample-filter belongs" in capsys.readouterr().err
