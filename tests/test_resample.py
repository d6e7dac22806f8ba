"""The horizontal resample to square pixels on the host: ingest.Resample's tables against the builder of tests/resample_ref.py and their
properties, the display-width rule, the integers of vse_yuv_resample in YuvFrame.to_bgr() / InterlacedYuvFrame.to_bgr() against the int64
restatement, row bands, the Y4M header's A token and the sources' three options, what they refuse, both command lines with a scripted
recogniser, and the change selector over a squeezed clip read back with square pixels.  CPU only."""
import logging

import numpy as np
import pytest

import area_cells_ref
import deinterlace_ref as D
import resample_ref as RR
import yuv_format_ref as R
from frame_change_ref import NumpyCounter
from test_gpu_deinterlace import FORMATS
from test_one_pass import AREA, FPS, LookupOcr, clip, host_stack, piped, run, text_box  # noqa: F401  (host_stack is a fixture)
from test_yuv_formats import bgr_source, ident, product_format
from vse_amd import area_locator, extractor, frame_select, ingest

FMT420 = (1, 1, 1, 8, 0, 0, 0)
# (stored, shown) plane widths: the ratios of the issue, the GPU test's shapes (odd, tiny, shrinking), and chroma widths of them
WIDTHS = [(720, 854), (720, 1048), (720, 640), (1440, 1920), (1280, 1920), (960, 1280), (360, 427), (540, 640), (270, 320), (1, 1), (2, 3),
          (5, 4), (17, 23), (34, 41), (50, 37), (3, 2), (64, 48)]


# ---- the tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RR.FILTERS)
def test_tables_equal_the_reference_builder(name):
    for pw_in, pw_out in WIDTHS:
        left, coef = ingest.resample_table(pw_in, pw_out, name)
        want_left, want_coef = RR.table(pw_in, pw_out, name)
        assert left.dtype == np.int32 and coef.dtype == np.int16 and not left.flags.writeable and not coef.flags.writeable
        assert np.array_equal(left, want_left) and np.array_equal(coef, want_coef), (name, pw_in, pw_out)


@pytest.mark.parametrize("name", RR.FILTERS)
def test_table_properties(name):
    worst = 0
    for pw_in, pw_out in WIDTHS:
        left, coef = (a.astype(np.int64) for a in ingest.resample_table(pw_in, pw_out, name))
        k = coef.shape[1]
        assert k % 2 == 0 and 2 <= k <= 16 and k == RR.taps_needed(pw_in, pw_out, name) and left.shape == (pw_out,)
        assert np.all(coef.sum(axis=1) == 16384), (name, pw_in, pw_out)                   # a flat row stays flat
        worst = max(worst, int(np.abs(coef).sum(axis=1).max()))
        assert np.abs(coef).sum(axis=1).max() <= 32767
        # every tap that carries weight lies within the stretched support of its centre
        c = (np.arange(pw_out) + 0.5) * pw_in / pw_out - 0.5
        reach = RR.SUPPORT[name] * max(1.0, pw_in / pw_out)
        pos = left[:, None] + np.arange(k)[None, :]
        assert np.all((np.abs(pos - c[:, None]) < reach + 1e-9) | (coef == 0))
        # mirror symmetry of the filter as applied (the clamped taps added up), except in a column whose centre lies midway between two
        # samples: its two largest taps are equal and the rounding remainder goes to the first of them
        dense = RR.dense(left, coef, pw_in)
        midway = np.abs(c - np.floor(c) - 0.5) < 1e-9
        sym = np.all(dense == dense[::-1, ::-1], axis=1)
        assert np.all(sym | midway | midway[::-1]), (name, pw_in, pw_out)
    print(f"{name}: largest sum of |coef| {worst}")
    assert worst == {"bicubic": 20600, "bilinear": 16384, "lanczos": 25288}[name]      # the issue's figures, on its widths


def test_identity_scale_is_the_identity_table():
    for name in RR.FILTERS:
        left, coef = ingest.resample_table(37, 37, name)
        assert np.array_equal(RR.dense(left, coef, 37), 16384 * np.eye(37, dtype=np.int64))


def test_display_width_rule():
    assert len(RR.DISPLAY) == 8
    for w, (num, den), shown in RR.DISPLAY:
        assert ingest.display_width(w, num, den) == shown == RR.display_width(w, num, den) and shown % 2 == 0
        assert abs(shown - w * num / den) <= 1.0
        r = ingest.Resample.from_sar(w, num, den)
        assert (r.in_width, r.out_width, r.filter) == (w, shown, "bicubic")
    assert ingest.display_width(720, 1, 1) == 720 and ingest.display_width(721, 1, 1) == 722


def test_resample_is_a_hashable_validated_tuple():
    a, b = ingest.Resample(720, 854), ingest.Resample(720, 854, "bicubic")
    assert a == b and hash(a) == hash(b) and a != ingest.Resample(720, 854, "lanczos") and len({a, b}) == 1
    fmt = product_format(FMT420)
    assert a.tables(fmt) is b.tables(fmt) and a.tables(fmt)[1][0].shape == (427,)
    assert a.tables(product_format((0, 0, 0, 8, 0, 0, 0)))[1] is None and a.packed(product_format((0, 0, 0, 8, 0, 0, 0)))[1] is None
    luma, chroma = a.packed(fmt)
    assert len(luma) == 854 * (4 + 2 * 4) and len(chroma) == 427 * (4 + 2 * 4)
    assert np.array_equal(np.frombuffer(luma, "<i4", 854), a.tables(fmt)[0][0])
    assert np.array_equal(np.frombuffer(luma, "<i2", offset=4 * 854).reshape(854, 4), a.tables(fmt)[0][1])
    with pytest.raises(ValueError, match=r"'lanczos' from 1920 to 480 columns needs 24 taps"):
        ingest.Resample(1920, 480, "lanczos")
    with pytest.raises(ValueError, match=r"'bicubic' from 100 to 20 columns needs 20 taps"):
        ingest.Resample(100, 20)
    assert ingest.resample_table(100, 25, "bicubic")[1].shape == (25, 16)
    for bad in (dict(filter="nearest"), dict(in_width=0), dict(out_width=-3), dict(in_width=7.5), dict(out_width=True)):
        with pytest.raises(ValueError, match="resample"):
            ingest.Resample(**{**dict(in_width=720, out_width=854), **bad})
    with pytest.raises(ValueError, match="32767"):
        ingest.check_resample_table(np.zeros(2, np.int32), np.array([[20000, 12768], [16384, 0]], np.int16))
    with pytest.raises(ValueError, match="K even"):
        ingest.check_resample_table(np.zeros(2, np.int32), np.zeros((2, 3), np.int16))
    rng = np.random.default_rng(1)
    left, coef = RR.random_table(rng, 9, 7, 6)
    ingest.check_resample_table(left, coef)


# ---- the arithmetic -------------------------------------------------------------------------------------------------------------------
def valid_planes(rng, h, w, fmt):
    """Random planes of valid samples: the low bits of a high-bit word are zero, as a decoder writes them."""
    planes = R.random_planes(rng, h, w, fmt)
    return tuple(p & np.uint16((0xFFFF << (16 - fmt[3])) & 0xFFFF) for p in planes) if fmt[4] else planes


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_identity_and_constant_planes(fmt):
    rng = np.random.default_rng(sum(fmt))
    pf = product_format(fmt)
    h, w = 5, 17
    planes = valid_planes(rng, h, w, fmt)
    ident_tables = (RR.identity(w), RR.identity(RR.chroma_width(w, fmt)) if fmt[2] else None)
    for got, want in zip(RR.picture(planes, fmt, *ident_tables), planes):
        assert np.array_equal(got, want)
    shift, maxv = (16 - fmt[3] if fmt[4] else 0), (1 << fmt[3]) - 1
    for got, want in zip((ingest.resample_rows(p, *(np.asarray(a) for a in ident_tables[1 if k else 0]), comps=2 if k and fmt[2] == 2 else 1,
                                               shift=shift, maxv=maxv) for k, p in enumerate(planes)), planes):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    for name in RR.FILTERS:
        r = ingest.Resample(w, 23, name)
        for value in (0, 1, maxv // 3, maxv):
            flat = tuple(np.full(p.shape, value << shift, p.dtype) for p in planes)
            if fmt[2] == 2:
                flat[1][:, 1::2] = (maxv - value) << shift                            # U and V keep their own constants
            out = r.planes(pf, flat)
            assert out[0].shape == (h, 23) and np.all(out[0] == value << shift)
            for p in out[1:]:
                assert np.all(p[:, 0::2] == value << shift) and np.all(p[:, 1::2] == ((maxv - value if fmt[2] == 2 else value) << shift))


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_frames_convert_as_the_reference_resamples(fmt):
    """YuvFrame.to_bgr() and InterlacedYuvFrame.to_bgr() with resample= equal the reference resample of the (deinterlaced) planes, then the
    existing conversion; a row slice equals the whole frame's rows."""
    rng = np.random.default_rng(sum(fmt) + 5)
    pf = product_format(fmt)
    h = 10
    for (w, w_out), name in (((17, 23), "bicubic"), ((34, 41), "lanczos"), ((50, 37), "bilinear")):
        r = ingest.Resample(w, w_out, name)
        tabs = RR.tables(w, w_out, fmt, name)
        planes = R.random_planes(rng, h, w, fmt)
        frame = ingest.YuvFrame(planes, h, w, pf, resample=r)
        want = R.convert(RR.picture(planes, fmt, *tabs), fmt)
        assert frame.shape == (h, w_out, 3) and frame.width == w and frame.packed_bytes == R.packed_bytes(h, w, fmt)
        assert np.array_equal(frame.to_bgr(), want)
        for a, b in ((0, 1), (3, 8), (5, 10), (1, 2)):
            cut = frame[a:b]
            assert cut.resample == r and cut.shape == (b - a, w_out, 3) and np.array_equal(cut.to_bgr(), want[a:b]), (a, b)
            buf = np.zeros(cut.packed_bytes, np.uint8)
            assert cut.pack_into(buf) == cut.packed_bytes                             # the packing is the stored picture's
            assert np.array_equal(buf, R.pack(R.sub_frame(planes, fmt, a, b)[0], fmt))
        prev = D.near_threshold_prev(rng, planes, fmt)
        for mode in ("adaptive", "match"):
            inter = ingest.InterlacedYuvFrame(planes, h, w, pf, prev, "tff", mode, resample=r)
            prog = inter.deinterlaced_planes()
            assert np.array_equal(inter.to_bgr(), R.convert(RR.picture(prog, fmt, *tabs), fmt)) and inter.shape == (h, w_out, 3)
            if mode == "adaptive":
                assert all(np.array_equal(p, q) for p, q in zip(prog, D.picture(planes, prev, fmt, 0)))
                assert np.array_equal(inter[3:8].to_bgr(), inter.to_bgr()[3:8]) and inter[3:8].resample == r
    with pytest.raises(ValueError, match="stored columns"):
        ingest.YuvFrame(planes, h, 50, pf, resample=ingest.Resample(17, 23))
    with pytest.raises(ValueError, match="resample must be"):
        ingest.YuvFrame(planes, h, 50, pf, resample=(50, 37))


def test_tone_map_follows_the_resample():
    import tonemap_ref as TM
    fmt = (1, 1, 1, 10, 0, 2, 0)
    rng = np.random.default_rng(9)
    planes = R.random_planes(rng, 6, 34, fmt)
    tone, r = ingest.ToneMap("pq"), ingest.Resample(34, 41)
    got = ingest.YuvFrame(planes, 6, 34, product_format(fmt), tone=tone, resample=r).to_bgr()
    assert np.array_equal(got, TM.convert(RR.picture(planes, fmt, *RR.tables(34, 41, fmt, "bicubic")), fmt, *tone.tables()))


# ---- the sources ----------------------------------------------------------------------------------------------------------------------
def header(token):
    return b"YUV4MPEG2 W6 H4 F12:1 Ip " + token + b" C420jpeg"


def test_a_token():
    for token, want in ((b"A32:27", (32, 27)), (b"A0:0", None), (b"A1:1", (1, 1)), (b"", None), (b"A16:11", (16, 11)), (b"A4:0", None),
                        (b"Awide", None), (b"A3", None)):
        assert ingest.parse_y4m_aspect(header(token)) == want, token
    # the parsers' own results do not change
    for token in (b"A32:27", b"A0:0", b""):
        assert ingest.parse_y4m_header(header(token), "x") == (6, 4, 12.0)
        assert ingest.parse_y4m_header_fields(header(token), "x")[:3] == (6, 4, 12.0)


def small_clip(tmp_path, aspect, fmt=FMT420, w=34, name="clip.y4m", count=3):
    rng = np.random.default_rng(4)
    frames = [R.random_planes(rng, 6, w, fmt) for _ in range(count)]
    path = str(tmp_path / name)
    ingest.write_yuv(path, frames, product_format(fmt), fps=FPS, y4m=True, aspect=aspect)
    return path, frames


def test_sources_attach_the_resample(tmp_path, caplog):
    path, frames = small_clip(tmp_path, (32, 27))
    shown = RR.display_width(34, 32, 27)
    assert shown == 40
    want = [R.convert(RR.picture(p, FMT420, *RR.tables(34, shown, FMT420, "bicubic")), FMT420) for p in frames]
    for wide in (False, True):
        for src in (ingest.Y4mSource(path, wide=wide, square_pixels=True), ingest.open_source(path, wide=wide, square_pixels=True)):
            assert src.resample == ingest.Resample(34, shown) and src.width == 34 and src.fmt == product_format(FMT420)
            for no, raw in enumerate(src.raw_frames(), 1):
                assert type(raw) is ingest.YuvFrame and raw.resample == src.resample and raw.shape == (6, shown, 3)
                assert np.array_equal(raw.to_bgr(), want[no - 1]) and np.array_equal(src.read(no), want[no - 1])
            src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    fp, th = piped(data, 7)
    st = ingest.Y4mStream(fp, square_pixels=True)
    assert st.resample == ingest.Resample(34, shown)
    assert [np.array_equal(f, x) for f, x in zip(st.frames(), want)] == [True] * 3
    th.join()
    fp.close()
    # sar= overrides the header, and picks the filter's tables
    src = ingest.Y4mSource(path, sar=(16, 11), resample_filter="lanczos")
    assert src.resample == ingest.Resample(34, RR.display_width(34, 16, 11), "lanczos")
    assert np.array_equal(src.read(2), R.convert(RR.picture(frames[1], FMT420, *RR.tables(34, src.resample.out_width, FMT420, "lanczos")), FMT420))
    src.close()
    # interlaced frames carry it: deinterlace, then resample, then convert
    src = ingest.Y4mSource(path, wide=True, deinterlace="adaptive", field_order="tff", square_pixels=True)
    raw = src.read_raw(2)
    assert isinstance(raw, ingest.InterlacedYuvFrame) and raw.resample == ingest.Resample(34, shown)
    assert np.array_equal(raw.to_bgr(), R.convert(RR.picture(D.picture(frames[1], frames[0], FMT420, 0), FMT420, *RR.tables(34, shown, FMT420, "bicubic")),
                                                 FMT420))
    src.close()
    # headerless files: sar is the only way; 8-bit 4:2:0 by extension goes through YuvSource
    p010 = (1, 1, 2, 10, 1, 1, 0)
    rng = np.random.default_rng(8)
    planes = [R.random_planes(rng, 6, 34, p010) for _ in range(2)]
    raw_path = str(tmp_path / "clip.p010")
    ingest.write_yuv(raw_path, planes, product_format(p010))
    src = ingest.open_source(raw_path, size=(34, 6), fps=FPS, matrix="bt709", sar=(4, 3))
    assert isinstance(src, ingest.YuvSource) and src.resample == ingest.Resample(34, 46)
    assert np.array_equal(src.read(2), R.convert(RR.picture(planes[1], p010, *RR.tables(34, 46, p010, "bicubic")), p010))
    src.close()
    yuv_path = str(tmp_path / "clip.nv12")
    nv12 = (1, 1, 2, 8, 0, 0, 0)
    planes = [R.random_planes(rng, 6, 34, nv12) for _ in range(2)]
    ingest.write_yuv(yuv_path, planes, product_format(nv12))
    src = ingest.open_source(yuv_path, size=(34, 6), fps=FPS, sar=(8, 9))
    assert isinstance(src, ingest.YuvSource) and src.resample == ingest.Resample(34, 30) and src.fmt == product_format(nv12)
    assert np.array_equal(src.read(1), R.convert(RR.picture(planes[0], nv12, *RR.tables(34, 30, nv12, "bicubic")), nv12))
    src.close()


def test_no_op_cases_give_todays_frames(tmp_path, caplog):
    rng = np.random.default_rng(3)
    yuv = [R.random_planes(rng, 6, 34, FMT420) for _ in range(2)]
    square, none, wide10 = str(tmp_path / "square.y4m"), str(tmp_path / "none.y4m"), str(tmp_path / "ten.y4m")
    ingest.write_y4m(square, yuv, FPS)                                               # A1:1
    with open(square, "rb") as fp:
        data = fp.read()
    with open(none, "wb") as fp:
        fp.write(data.replace(b" A1:1", b"", 1))
    ten, _ = small_clip(tmp_path, (0, 0), (1, 1, 1, 10, 0, 0, 0), name="ten.y4m")
    assert ten == wide10
    caplog.set_level(logging.INFO, logger="vse_amd.ingest")
    for path, kw, word in ((square, dict(square_pixels=True), "square pixels"), (none, dict(square_pixels=True), "no sample aspect ratio"),
                           (square, dict(sar=(1, 1)), "square pixels"), (square, dict(sar=(5, 5), resample_filter="lanczos"), "square pixels"),
                           (square, dict(sar=(100, 99)), "as stored")):
        caplog.clear()
        a, b = ingest.Y4mSource(path, **kw), ingest.Y4mSource(path)
        assert a.resample is None and a.fmt is None
        lines = [r.getMessage() for r in caplog.records]
        assert len(lines) == 1 and word in lines[0], lines
        for x, y in zip(a.raw_frames(), b.raw_frames()):
            assert type(x) is ingest.Yuv420Frame and x.shape == y.shape and np.array_equal(x.to_bgr(), y.to_bgr())
        buf_a, buf_b = np.zeros(x.packed_bytes, np.uint8), np.zeros(y.packed_bytes, np.uint8)
        x.pack_into(buf_a), y.pack_into(buf_b)
        assert np.array_equal(buf_a, buf_b)
        a.close()
        b.close()
    # wide readers: YuvFrames without a resample; the header that the 8-bit reader refuses is still refused without wide
    a = ingest.Y4mSource(wide10, wide=True, square_pixels=True)
    assert a.resample is None and type(a.read_raw(1)) is ingest.YuvFrame and a.read_raw(1).resample is None and a.read_raw(1).shape == (6, 34, 3)
    a.close()
    # ... in today's words, whichever way the option ends up attaching nothing (the no-op is decided before the parser is chosen)
    def refusal(make):
        with pytest.raises(ValueError) as e:
            make()
        return str(e.value)
    for kw in (dict(square_pixels=True), dict(sar=(1, 1)), dict(sar=(100, 99))):
        assert refusal(lambda: ingest.Y4mSource(wide10, **kw)) == refusal(lambda: ingest.Y4mSource(wide10)) and "C420p10" in refusal(
            lambda: ingest.Y4mSource(wide10, **kw))
        assert refusal(lambda: ingest.Y4mStream(open(wide10, "rb"), **kw)) == refusal(lambda: ingest.Y4mStream(open(wide10, "rb")))
    st = ingest.Y4mStream(open(none, "rb"), square_pixels=True)
    assert st.resample is None and st.fmt is None and type(next(st.raw_frames())) is ingest.Yuv420Frame
    # headerless: square_pixels alone has no ratio to go by
    raw = str(tmp_path / "clip.yuv")
    ingest.write_yuv420(raw, yuv)
    for kw in (dict(square_pixels=True), dict(sar=(1, 1)), dict(sar=(100, 99))):
        caplog.clear()
        src = ingest.open_source(raw, size=(34, 6), fps=FPS, **kw)
        assert isinstance(src, ingest.Yuv420Source) and type(src.read_raw(1)) is ingest.Yuv420Frame
        assert len(caplog.records) == 1 and "as stored" in caplog.records[0].getMessage()          # one line, whichever way
        src.close()
    caplog.clear()
    src = ingest.open_source(raw, size=(34, 6), fps=FPS, sar=(4, 3))                              # ... and none where it resamples
    assert isinstance(src, ingest.YuvSource) and src.resample == ingest.Resample(34, 46) and not caplog.records
    src.close()
    # with the option off nothing is parsed, logged or attached
    caplog.clear()
    src = ingest.open_source(small_clip(tmp_path, (32, 27), name="wide.y4m")[0])
    assert src.resample is None and type(src.read_raw(1)) is ingest.Yuv420Frame and src.read_raw(1).shape == (6, 34, 3) and not caplog.records
    src.close()


def test_refusals_name_the_option(tmp_path):
    path, _ = small_clip(tmp_path, (32, 27))
    npy = str(tmp_path / "clip.npy")
    np.save(npy, np.zeros((1, 4, 6, 3), np.uint8))
    for call, word in ((lambda: ingest.Y4mSource(path, square_pixels=True, resample_filter="nearest"), "resample_filter"),
                       (lambda: ingest.Y4mSource(path, resample_filter="lanczos"), "resample_filter belongs"),
                       (lambda: ingest.Y4mSource(path, sar=(32, 0)), "sar must be"), (lambda: ingest.Y4mSource(path, sar="32:27"), "sar must be"),
                       (lambda: ingest.Y4mSource(path, sar=(1.5, 1)), "sar must be"), (lambda: ingest.Y4mSource(path, sar=(32, 27, 1)), "sar must be"),
                       (lambda: ingest.Y4mStream(open(path, "rb"), sar=(0, 1)), "sar must be"),
                       (lambda: ingest.open_source(path, sar=(-1, 1)), "sar must be"),
                       (lambda: ingest.open_source(npy, fps=FPS, square_pixels=True), "square_pixels / sar"),
                       (lambda: ingest.open_source(str(tmp_path / "film.avi"), sar=(32, 27)), "square_pixels / sar"),
                       (lambda: ingest.Y4mSource(path, sar=(1, 100)), "shows 34 columns as 0"),
                       (lambda: ingest.Y4mSource(path, sar=(1, 8), resample_filter="lanczos"), r"'lanczos' from 34 to 4 columns needs 52 taps"),
                       (lambda: ingest.YuvSource(path, 34, 6, FPS, product_format(FMT420), sar=(1, 6)), r"'bicubic' from 34 to 6 columns needs 24 taps")):
        with pytest.raises(ValueError, match=word):
            call()


# ---- the command lines and the end-to-end run -------------------------------------------------------------------------------------------
_squeezed = {}


def squeezed_clip(tmp_path):
    """The change clip (640 x 360) squeezed to 540 columns with the reference's bicubic tables (540 * 32 / 27 = 640 exactly) in a Y4M
    with A32:27 -> (path, the frames Y4mSource(square_pixels=True) gives on the host, truth)."""
    frames, truth = clip("change")
    if "planes" not in _squeezed:
        tabs = RR.tables(640, 540, FMT420, "bicubic")
        _squeezed["planes"] = [RR.picture(ingest.bgr_to_yuv420(f), FMT420, *tabs) for f in frames]
    path = str(tmp_path / "squeezed.y4m")
    ingest.write_yuv(path, _squeezed["planes"], product_format(FMT420), fps=FPS, y4m=True, aspect=(32, 27))
    if "decoded" not in _squeezed:
        src = ingest.Y4mSource(path, square_pixels=True)
        assert (src.width, src.height, src.frame_count) == (540, 360, len(frames)) and src.resample == ingest.Resample(540, 640)
        _squeezed["decoded"] = list(src.frames())
        src.close()
    return path, _squeezed["decoded"], truth


def test_squeezed_clip_keeps_its_intervals_in_display_pixels(tmp_path):
    """The host route end to end: the frames come out 640 wide, and the change selector with the numpy counter over the area given in
    display pixels finds the original clip's intervals.  The round-trip error is printed (EXPERIMENTS.md AF)."""
    frames, truth = clip("change")
    _path, decoded, _ = squeezed_clip(tmp_path)
    assert all(f.shape == (360, 640, 3) and f.dtype == np.uint8 for f in decoded) and len(decoded) == len(frames)
    diff = np.abs(np.stack(decoded).astype(np.int16) - frames)
    print(f"640 -> 540 -> 640 bicubic, 8-bit 4:2:0: max |diff| {diff.max()}, mean {diff.mean():.4f} levels against the original clip")

    def intervals(fr):
        return [(s, e) for s, e, _rep in frame_select.ChangeFrameSelector(NumpyCounter(), batch=8).run(list(fr), AREA, FPS)]
    want = intervals(frames)
    assert want == [(s, e) for s, e, _t in truth] and len(want) == 3
    assert intervals(decoded) == want
    # the stored columns alone put the same area (in display pixels) off the frame
    stored = ingest.Y4mSource(_path)
    assert stored.read(1).shape == (360, 540, 3)
    stored.close()


def test_extractor_command_line_takes_square_pixels(host_stack, tmp_path, monkeypatch, capsys):
    path, decoded, truth = squeezed_clip(tmp_path)
    _, want = run(bgr_source(decoded), decoded, truth, "change", 8, None)
    assert want[3].count(" --> ") == len(truth)
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"               # display pixels: xmax 640 lies outside the 540 stored columns
    common = ["--area", area, "--selector", "change", "--batch", "8"]
    out = str(tmp_path / "out.srt")
    for flags in (["--square-pixels"], ["--sar", "32:27"], ["--square-pixels", "--resample-filter", "bicubic"], ["--wide-yuv", "--square-pixels"]):
        ocr = LookupOcr(decoded, truth, text_box(AREA))
        assert extractor.main([path, "-o", out] + flags + common, ocr=ocr, counter=NumpyCounter()) == 0, flags
        assert open(out).read() == want[3] and ocr.seen == want[1]
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 4099)
    monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main(["-", "--square-pixels"] + common, ocr=ocr, counter=NumpyCounter()) == 0
    pipe.close()
    th.join()
    assert capsys.readouterr().out == want[3]
    # the options reach the source
    args = type("Args", (), dict(square_pixels=False, sar="16:11", resample_filter="lanczos"))()
    assert extractor.square_arguments(args) == dict(square_pixels=True, sar=(16, 11), resample_filter="lanczos")
    src = ingest.open_source(path, **extractor.square_arguments(args))
    assert src.resample == ingest.Resample(540, 786, "lanczos")
    src.close()
    assert extractor.square_arguments(type("Args", (), dict(square_pixels=False, sar=None, resample_filter=None))()) == {}
    # refusals: exit status 2 and the message on standard error, nothing recognised
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    np.save(str(tmp_path / "clip.npy"), np.zeros((1, 4, 6, 3), np.uint8))
    for argv, word in (([path, "--sar", "32"], "--sar takes"), ([path, "--sar", "0:1"], "--sar takes"), ([path, "--sar", "a:b"], "--sar takes"),
                       ([path, "--resample-filter", "lanczos"], "--resample-filter belongs"),
                       ([path, "--sar", "1:9", "--resample-filter", "lanczos"], "taps"),
                       ([str(tmp_path / "clip.npy"), "--fps", "12", "--square-pixels"], "square_pixels / sar")):
        assert extractor.main(argv + common, ocr=ocr, counter=NumpyCounter()) == 2 and ocr.seen == [], argv
        err = capsys.readouterr().err
        assert err.startswith("extractor: ") and word in err, (argv, err)
    with pytest.raises(SystemExit) as e:
        extractor.main([path, "--resample-filter", "nearest"] + common, ocr=ocr, counter=NumpyCounter())
    assert e.value.code == 2


def test_locator_command_line_takes_square_pixels(tmp_path, capsys):
    path, decoded, _ = squeezed_clip(tmp_path)
    want = area_locator.AreaLocator(area_cells_ref.NumpyCells()).run(decoded, FPS)
    assert want is not None
    for flags in (["--square-pixels"], ["--sar", "32:27", "--resample-filter", "bicubic"]):
        assert area_locator.main([path] + flags, cells_fn=area_cells_ref.NumpyCells()) == 0
        assert capsys.readouterr().out.split() == [str(v) for v in (want.ymin, want.ymax, want.xmin, want.xmax)]
    stored = ingest.Y4mSource(path)
    other = area_locator.AreaLocator(area_cells_ref.NumpyCells()).run(list(stored.frames()), FPS)
    stored.close()
    assert other is None or (other.xmin, other.xmax) != (want.xmin, want.xmax)          # without the option the area is in stored columns
    assert area_locator.main([path, "--sar", "32"], cells_fn=area_cells_ref.NumpyCells()) == 2
    assert "--sar takes" in capsys.readouterr().err
    assert area_locator.main([path, "--resample-filter", "bilinear"], cells_fn=area_cells_ref.NumpyCells()) == 2
    assert "--resample-filter belongs" in capsys.readouterr().err
