"""Interlaced YUV on the host: ingest.InterlacedYuvFrame against the int64 restatement of the rule (tests/deinterlace_ref.py) for every
plane layout, the threshold by hand, static clips, row bands, what the headers and sources accept and refuse, the change selector's intervals
on a clip whose subtitles switch between the two fields of a frame, one pass against several, and the command line.  CPU only."""
import itertools

import numpy as np
import pytest

import deinterlace_ref as D
import yuv_format_ref as R
from frame_change_ref import NumpyCounter
from test_change_select import AREA as CHANGE_AREA, SCHEDULE
from test_one_pass import AREA, FPS, LookupOcr, host_stack, piped, run, text_box  # noqa: F401  (host_stack is a fixture)
from test_yuv_formats import ident, product_format
from vse_amd import extractor, frame_select, ingest, synth

# (sub_x, sub_y, chroma, depth, msb, matrix, full_range): every subsampling, planar and semi-planar, depths 8, 10 and 16, high-bit words
FORMATS = [(0, 0, 0, 8, 0, 0, 0), (0, 0, 1, 8, 0, 1, 0), (1, 0, 1, 8, 0, 0, 1), (1, 1, 1, 8, 0, 0, 0), (1, 1, 2, 8, 0, 1, 0),
           (0, 0, 0, 10, 0, 0, 0), (0, 0, 1, 10, 0, 2, 0), (1, 0, 1, 10, 0, 1, 0), (1, 1, 1, 10, 0, 1, 0), (1, 1, 2, 10, 1, 2, 0),
           (1, 1, 1, 16, 0, 0, 0), (1, 1, 2, 16, 1, 1, 0), (0, 0, 1, 16, 1, 0, 1), (1, 0, 1, 12, 1, 2, 0)]
HEIGHTS = (1, 2, 3, 5, 7, 46)
MODES = ("adaptive", "interpolate")
ORDERS = ("tff", "bff")


def pictures(rng, h, w, fmt, thresh=10):
    """(planes, previous planes) of random words with P = C + d around the threshold."""
    cur = R.random_planes(rng, h, w, fmt)
    return cur, D.near_threshold_prev(rng, cur, fmt, thresh)


def equal_planes(a, b):
    return len(a) == len(b) and all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(a, b))


# ---- the rule --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_deinterlaced_planes_equal_the_reference(fmt):
    rng = np.random.default_rng(sum(fmt))
    pf = product_format(fmt)
    for h, w in itertools.product(HEIGHTS, (1, 6, 23)):
        cur, prev = pictures(rng, h, w, fmt)
        for keep, mode, with_prev in itertools.product((0, 1), (0, 1), (True, False)):
            f = ingest.InterlacedYuvFrame(cur, h, w, pf, prev if with_prev else None, ORDERS[keep], MODES[mode])
            want = D.picture(cur, prev if with_prev else None, fmt, keep, mode)
            assert equal_planes(f.deinterlaced_planes(), want), (h, w, keep, mode, with_prev)
            assert np.array_equal(f.to_bgr(), R.convert(want, fmt)), (h, w, keep, mode, with_prev)
    # both branches were taken on the adaptive cases: neither all woven nor all interpolated
    cur, prev = pictures(rng, 46, 23, fmt)
    inter, woven = D.shares(cur, prev, fmt)
    assert 0.25 <= inter / (inter + woven) <= 0.75, (inter, woven)


@pytest.mark.parametrize("fmt,t", [((0, 0, 0, 8, 0, 0, 0), 10), ((0, 0, 0, 10, 0, 0, 0), 40), ((0, 0, 0, 10, 1, 0, 0), 2560)], ids=["8", "10", "10msb"])
def test_threshold_and_edges_by_hand(fmt, t):
    """One column of five rows, top field first: rows 1 and 3 are the second field's.  |d| = T weaves, T + 1 interpolates, and a
    difference in the row above or below counts as one in the row itself."""
    pf = product_format(fmt)
    dt = R.sample_dtype(fmt)
    unit = t // 10
    col = (np.array([10, 50, 30, 90, 20]) * unit).astype(dt)[:, None]

    def out(prev_col, order="tff", h=5):
        prev = None if prev_col is None else (np.asarray(prev_col).astype(dt)[:, None],)
        return ingest.InterlacedYuvFrame((col[:h],), h, 1, pf, prev, order, thresh=10).deinterlaced_planes()[0][:, 0].tolist()
    c = col[:, 0].astype(np.int64)
    mean = lambda a, b: int((c[a] + c[b] + 1) >> 1)       # noqa: E731
    assert pf.depth == fmt[3] and ingest.InterlacedYuvFrame((col,), 5, 1, pf, None, thresh=10).thresh_words == t == D.threshold(fmt, 10)
    assert out(c) == c.tolist()                                                        # nothing changed: woven
    assert out(c + [0, t, 0, -t, 0]) == c.tolist()                                     # |d| = T: woven
    assert out(c + [0, t + 1, 0, 0, 0]) == [c[0], mean(0, 2), c[2], c[3], c[4]]        # T + 1 in the row itself
    assert out(c + [0, 0, 0, -t - 1, 0]) == [c[0], c[1], c[2], mean(2, 4), c[4]]
    assert out(c + [0, 0, t + 1, 0, 0]) == [c[0], mean(0, 2), c[2], mean(2, 4), c[4]]  # in the row between: both neighbours
    assert out(c + [t + 1, 0, 0, 0, 0]) == [c[0], mean(0, 2), c[2], c[3], c[4]]        # in the row above
    assert out(c + [0, 0, 0, 0, t + 1]) == [c[0], c[1], c[2], mean(2, 4), c[4]]        # in the row below
    assert out(None) == [c[0], mean(0, 2), c[2], mean(2, 4), c[4]]                     # no previous picture
    # bottom field first: rows 0, 2, 4 are interpolated; the top and bottom rows have one neighbour, which counts twice
    assert out(None, "bff") == [c[1], c[1], mean(1, 3), c[3], c[3]]
    assert out(None, "tff", 4) == [c[0], mean(0, 2), c[2], c[2]]
    assert out(None, "bff", 2) == [c[1], c[1]] and out(None, "tff", 2) == [c[0], c[0]]
    assert out(None, "bff", 1) == [c[0]] and out(None, "tff", 1) == [c[0]]
    # the rounding: (a + b + 1) >> 1
    assert mean(0, 2) == (10 * unit + 30 * unit + 1) // 2


def test_static_clip_is_left_as_it_is():
    """A still picture with noise of at most thresh - 1 levels between frames: every frame but the first equals its input, the first
    (no previous picture) equals mode interpolate."""
    rng = np.random.default_rng(3)
    for fmt in ((1, 1, 1, 8, 0, 0, 0), (1, 1, 2, 10, 1, 1, 0)):
        pf = product_format(fmt)
        h, w, unit = 10, 14, D.threshold(fmt, 1)
        base = tuple(np.clip(p.astype(np.int64), 16 * unit, 200 * unit) for p in R.random_planes(rng, h, w, fmt))
        clip = [tuple((p + rng.integers(0, 10 * unit, size=p.shape)).astype(R.sample_dtype(fmt)) for p in base) for _ in range(4)]
        for k, cur in enumerate(clip):
            f = ingest.InterlacedYuvFrame(cur, h, w, pf, clip[k - 1] if k else None, thresh=10)
            if k:
                assert equal_planes(f.deinterlaced_planes(), cur)
                assert not equal_planes(ingest.InterlacedYuvFrame(cur, h, w, pf, clip[k - 1], thresh=4).deinterlaced_planes(), cur)
            else:
                assert equal_planes(f.deinterlaced_planes(), ingest.InterlacedYuvFrame(cur, h, w, pf, clip[1], mode="interpolate").deinterlaced_planes())
                assert not equal_planes(f.deinterlaced_planes(), cur)


@pytest.mark.parametrize("fmt", [(1, 1, 1, 8, 0, 0, 0), (1, 1, 2, 10, 1, 1, 0), (1, 0, 1, 10, 0, 2, 1), (0, 0, 0, 16, 0, 0, 0)], ids=ident)
def test_row_bands(fmt):
    """f[a:b].to_bgr() == f.to_bgr()[a:b] for every band at h = 9 and some at h = 46; slices keep class, prev and parameters, and the band
    packed for the device starts every plane on a top-field row and keeps its edge rows away from the rows asked for."""
    rng = np.random.default_rng(7)
    pf = product_format(fmt)
    for h, bands in ((9, [(a, b) for a in range(10) for b in range(a, 10)]), (46, [(0, 46), (23, 46), (0, 23), (11, 40), (12, 13), (45, 46), (1, 2)])):
        w = 10
        cur, prev = pictures(rng, h, w, fmt)
        for order in ORDERS:
            f = ingest.InterlacedYuvFrame(cur, h, w, pf, prev, order)
            whole = f.to_bgr()
            assert whole.shape == f.shape == (h, w, 3)
            for a, b in bands:
                g = f[a:b]
                assert type(g) is ingest.InterlacedYuvFrame and g.prev is f.prev and (g.field_order, g.mode, g.thresh) == (order, "adaptive", 10)
                assert g.shape == (b - a, w, 3) and g.row_parity == (a & fmt[1]) and np.array_equal(g.to_bgr(), whole[a:b]), (h, a, b)
                if b - a > 2:
                    assert np.array_equal(g[1:-1].to_bgr(), whole[a + 1:b - 1])
                lo, hi = g.band()
                assert lo % 4 == 0 and (hi % 2 == 0 or hi == h) and 0 <= lo <= a and b <= hi <= h
                assert (lo == 0 or lo <= a - 2) and (hi == h or hi >= b + 2)
                # what the device computes on the packed band equals the picture's rows: the reference on the band's planes
                if b > a:
                    sub_c, _ = R.sub_frame(cur, fmt, lo, hi)
                    sub_p, _ = R.sub_frame(prev, fmt, lo, hi)
                    got = R.convert(D.picture(sub_c, sub_p, fmt, ORDERS.index(order)), fmt)[a - lo:b - lo]
                    assert np.array_equal(got, whole[a:b]), (h, a, b)
                    buf = np.zeros(g.band_bytes, np.uint8)
                    assert g.pack_band_into(buf) == buf.size == R.packed_bytes(hi - lo, w, fmt)
                    assert np.array_equal(buf, R.pack(sub_c, fmt))
                    assert g.pack_band_into(buf, prev=True) == buf.size and np.array_equal(buf, R.pack(sub_p, fmt))
    with pytest.raises(TypeError):
        f[3]
    with pytest.raises(TypeError):
        f[::2]


def test_frame_checks_its_arguments():
    fmt = ingest.YuvFormat()
    cur = R.random_planes(np.random.default_rng(1), 4, 6, (1, 1, 1, 8, 0, 0, 0))
    for bad in (dict(field_order="auto"), dict(field_order="x"), dict(mode="weave"), dict(mode=None), dict(thresh=-1), dict(thresh=256), dict(thresh=1.5),
                dict(prev=cur[:2]), dict(prev=(cur[0], cur[1], cur[2][:1]))):
        with pytest.raises(ValueError):
            ingest.InterlacedYuvFrame(cur, 4, 6, fmt, **bad)
    f = ingest.InterlacedYuvFrame(cur, 4, 6, fmt, prev=cur)
    assert extractor._frame_nbytes(f) == 2 * extractor._frame_nbytes(ingest.YuvFrame(cur, 4, 6, fmt)) == 2 * 36
    assert extractor._frame_nbytes(ingest.InterlacedYuvFrame(cur, 4, 6, fmt)) == 36


# ---- headers and sources -------------------------------------------------------------------------------------------------------------
def y4m_file(tmp_path, token, frames, fmt=(1, 1, 1, 8, 0, 0, 0), name="clip.y4m"):
    h, w = frames[0][0].shape
    path = str(tmp_path / name)
    with open(path, "wb") as fp:
        fp.write(b"YUV4MPEG2 W%d H%d F25:1 %sA1:1 C420jpeg\n" % (w, h, (token + " ").encode() if token else b""))
        for f in frames:
            fp.write(b"FRAME\n" + R.pack(f, fmt).tobytes())
    return path


def open_both(path, **kw):
    """The file source and the stream over the same bytes -> [(source, its raw frames)]."""
    out = []
    src = ingest.Y4mSource(path, **kw)
    out.append((src, list(src.raw_frames())))
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 4099)
    st = ingest.Y4mStream(pipe, name=path, **kw)
    out.append((st, list(st.raw_frames())))
    th.join()
    pipe.close()
    return out


def test_without_deinterlace_every_refusal_is_unchanged(tmp_path):
    frames = [R.random_planes(np.random.default_rng(2), 4, 6, (1, 1, 1, 8, 0, 0, 0))]
    for token in ("It", "Ib", "Im"):
        path = y4m_file(tmp_path, token, frames)
        for kw in ({}, {"wide": True}, {"wide": True, "field_order": "tff"}):
            for make in (lambda: ingest.Y4mSource(path, **kw), lambda: ingest.open_source(path, **kw)):
                with pytest.raises(ValueError) as e:
                    make()
                assert str(e.value) == f"{path}: interlaced video ({token}) is not supported"
            with open(path, "rb") as fp, pytest.raises(ValueError) as e:
                ingest.Y4mStream(fp, name=path, **kw)
            assert str(e.value) == f"{path}: interlaced video ({token}) is not supported"
        for parse in (ingest.parse_y4m_header, ingest.parse_y4m_header_wide):
            with pytest.raises(ValueError, match=rf"interlaced video \({token}\) is not supported"):
                parse(b"YUV4MPEG2 W6 H4 F25:1 " + token.encode(), "x")
    assert len(ingest.parse_y4m_header_wide(b"YUV4MPEG2 W6 H4 F25:1 Ip", "x")) == 4


def test_header_and_source_behaviour_with_deinterlace(tmp_path):
    fmt = (1, 1, 1, 8, 0, 0, 0)
    rng = np.random.default_rng(5)
    frames = [R.random_planes(rng, 6, 8, fmt) for _ in range(4)]
    # (I token, field_order) -> the order the frames carry; None: plain YuvFrames
    cases = {("It", "auto"): "tff", ("Ib", "auto"): "bff", ("Ip", "auto"): None, ("I?", "auto"): None, ("", "auto"): None, ("It", "bff"): "bff",
             ("Ib", "tff"): "tff", ("Ip", "tff"): "tff", ("I?", "bff"): "bff", ("", "tff"): "tff", ("Im", "tff"): "tff", ("Im", "bff"): "bff"}
    for (token, order), want in cases.items():
        path = y4m_file(tmp_path, token, frames)
        for mode in MODES:
            for src, raws in open_both(path, wide=True, deinterlace=mode, field_order=order, deinterlace_thresh=7):
                assert src.field_order == want and src.deinterlace == mode and len(raws) == 4
                for k, raw in enumerate(raws):
                    assert equal_planes(raw.planes, frames[k])
                    if want is None:
                        assert type(raw) is ingest.YuvFrame
                        continue
                    assert type(raw) is ingest.InterlacedYuvFrame and (raw.field_order, raw.mode, raw.thresh) == (want, mode, 7)
                    assert (raw.prev is None) == (k == 0) and (k == 0 or raw.prev is raws[k - 1].planes or ingest._same_planes(raw.prev, raws[k - 1].planes))
                    ref = D.picture(frames[k], frames[k - 1] if k else None, fmt, ORDERS.index(want), MODES.index(mode), 7)
                    assert np.array_equal(raw.to_bgr(), R.convert(ref, fmt))
        src = ingest.Y4mSource(path, wide=True, deinterlace="adaptive", field_order=order)
        if want is not None:                                # read() and frames() go through to_bgr(); read_raw in any order
            for no in (3, 1, 4, 2, 3):
                ref = D.picture(frames[no - 1], frames[no - 2] if no > 1 else None, fmt, ORDERS.index(want))
                assert np.array_equal(src.read(no), R.convert(ref, fmt))
                raw = src.read_raw(no)
                assert (raw.prev is None) == (no == 1) and (no == 1 or equal_planes(raw.prev, frames[no - 2]))
            assert src.read_raw(3).prev is src.read_raw(2).planes or ingest._same_planes(src.read_raw(3).prev, src.read_raw(2).planes)
            assert all(np.array_equal(a, src.read(no)) for no, a in enumerate(src.frames(), 1))
        assert src.read_raw(0) is None and src.read_raw(5) is None
        src.close()
    # Im names no order: refused with auto; deinterlace needs wide; bad values
    path = y4m_file(tmp_path, "Im", frames)
    for make in (lambda: ingest.Y4mSource(path, wide=True, deinterlace="adaptive"),
                 lambda: ingest.open_source(path, wide=True, deinterlace="interpolate", field_order="auto")):
        with pytest.raises(ValueError, match="Im"):
            make()
    with open(path, "rb") as fp, pytest.raises(ValueError, match="Im"):
        ingest.Y4mStream(fp, wide=True, deinterlace="adaptive")
    path = y4m_file(tmp_path, "It", frames)
    for kw in (dict(deinterlace="adaptive"), dict(deinterlace="adaptive", wide=False, field_order="tff")):
        with pytest.raises(ValueError, match="wide"):
            ingest.Y4mSource(path, **kw)
        with pytest.raises(ValueError, match="wide"):
            ingest.open_source(path, **kw)
        with open(path, "rb") as fp, pytest.raises(ValueError, match="wide"):
            ingest.Y4mStream(fp, **kw)
    for kw in (dict(deinterlace="yadif"), dict(deinterlace="adaptive", field_order="top"), dict(deinterlace="adaptive", deinterlace_thresh=256),
               dict(deinterlace="adaptive", deinterlace_thresh=-1)):
        with pytest.raises(ValueError):
            ingest.Y4mSource(path, wide=True, **kw)
    with pytest.raises(ValueError, match="Ix"):
        ingest.Y4mSource(y4m_file(tmp_path, "Ix", frames), wide=True, deinterlace="adaptive", field_order="tff")


def test_headerless_source_needs_a_field_order(tmp_path):
    fmt = (1, 1, 2, 10, 1, 1, 0)
    pf = product_format(fmt)
    rng = np.random.default_rng(6)
    frames = [R.random_planes(rng, 6, 8, fmt) for _ in range(3)]
    path = str(tmp_path / "clip.p010")
    ingest.write_yuv(path, frames, pf)
    for make in (lambda **kw: ingest.YuvSource(path, 8, 6, 25.0, pf, **kw), lambda **kw: ingest.open_source(path, size=(8, 6), fps=25.0, matrix="bt709", **kw)):
        with pytest.raises(ValueError, match="field order"):
            make(deinterlace="adaptive")
        with pytest.raises(ValueError, match="field order"):
            make(deinterlace="interpolate", field_order="auto")
        assert type(make().read_raw(2)) is ingest.YuvFrame
        src = make(deinterlace="adaptive", field_order="bff", deinterlace_thresh=3)
        for no in (1, 2, 3):
            raw = src.read_raw(no)
            assert type(raw) is ingest.InterlacedYuvFrame and (raw.field_order, raw.thresh) == ("bff", 3) and (raw.prev is None) == (no == 1)
            ref = D.picture(frames[no - 1], frames[no - 2] if no > 1 else None, fmt, 1, 0, 3)
            assert np.array_equal(src.read(no), R.convert(ref, fmt))
        src.close()
    # the sources that have no planes of a YuvFormat do not take it
    for name in ("clip.yuv", "clip.npy", "clip.avi"):
        with pytest.raises(ValueError, match="deinterlace"):
            ingest.open_source(str(tmp_path / name), size=(8, 6), fps=25.0, deinterlace="adaptive", field_order="tff")


def test_write_yuv_names_the_interlacing(tmp_path):
    fmt = ingest.YuvFormat()
    frames = [R.random_planes(np.random.default_rng(8), 4, 6, (1, 1, 1, 8, 0, 0, 0)) for _ in range(2)]
    for flag, order in (("t", "tff"), ("b", "bff"), ("p", None)):
        path = str(tmp_path / f"{flag}.y4m")
        ingest.write_yuv(path, frames, fmt, fps=25, y4m=True, interlace=flag)
        with open(path, "rb") as fp:
            assert f" I{flag} ".encode() in fp.readline()
        src = ingest.Y4mSource(path, wide=True, deinterlace="adaptive")
        assert src.field_order == order and src.frame_count == 2
        src.close()
    ingest.write_yuv(str(tmp_path / "d.y4m"), frames, fmt, fps=25, y4m=True)
    with open(str(tmp_path / "d.y4m"), "rb") as a, open(str(tmp_path / "p.y4m"), "rb") as b:
        assert a.read() == b.read()
    with pytest.raises(ValueError):
        ingest.write_yuv(str(tmp_path / "x.y4m"), frames, fmt, fps=25, y4m=True, interlace="m")


# ---- the clip whose subtitles switch between the two fields of a frame -----------------------------------------------------------------
FMT420 = (1, 1, 1, 8, 0, 0, 0)
_clip = {}


def interlaced_clip():
    """tests/test_change_select.py's schedule rendered at field rate: entry i gets 2 frames + 1 fields for even i and 2 frames - 1 for odd
    i, so the subtitles switch between the two fields of a frame; the last field is dropped to make the count even.  -> dict of the
    field-rate BGR pictures, the woven (Y, U, V) triples (top field first), the progressive triples at the first field's times, and the
    truth in frame numbers of the progressive clip [(start, end, text)]."""
    if not _clip:
        sched = [(item[0], 2 * item[1] + (1 if i % 2 == 0 else -1)) + tuple(item[2:]) for i, item in enumerate(SCHEDULE)]
        bgr, truth = synth.make_clip(sched, 360, 640, seed=5)
        bgr = bgr[:len(bgr) & ~1]
        # field numbers (1-based) -> frames of the clip that shows the first field of each pair: frame k shows field 2 k - 1
        truth = [((s + 2) // 2, min((e + 1) // 2, len(bgr) // 2), t) for s, e, t in truth]
        _clip.update(bgr=bgr, woven=synth.interlace_yuv420(bgr, "tff"), first=[ingest.bgr_to_yuv420(f) for f in bgr[0::2]], truth=truth)
    return _clip


def deinterlaced_bgr(woven, order="tff", mode="adaptive", thresh=10):
    pf = product_format(FMT420)
    h, w = woven[0][0].shape
    return [ingest.InterlacedYuvFrame(f, h, w, pf, woven[k - 1] if k else None, order, mode, thresh).to_bgr() for k, f in enumerate(woven)]


def test_interlace_yuv420_weaves_the_fields():
    rng = np.random.default_rng(9)
    bgr = rng.integers(0, 256, size=(5, 6, 8, 3), dtype=np.uint8)
    for order, keep in (("tff", 0), ("bff", 1)):
        woven = synth.interlace_yuv420(bgr, order)
        assert len(woven) == 2
        for k, planes in enumerate(woven):
            first, second = ingest.bgr_to_yuv420(bgr[2 * k]), ingest.bgr_to_yuv420(bgr[2 * k + 1])
            for p, a, b in zip(planes, first, second):
                assert p.shape == a.shape and p.dtype == np.uint8
                assert np.array_equal(p[keep::2], a[keep::2]) and np.array_equal(p[1 - keep::2], b[1 - keep::2])


def test_deinterlaced_clip_keeps_the_intervals_the_woven_clip_loses():
    """The change selector (numpy counter, threshold 128) on the woven frames, on the progressive clip at the first field's times and on the
    deinterlaced frames: deinterlaced = progressive; the woven clip merges two subtitles into one and so finds fewer."""
    clip = interlaced_clip()
    pf = product_format(FMT420)
    h, w = clip["woven"][0][0].shape
    ref = [R.convert(D.picture(f, clip["woven"][k - 1] if k else None, FMT420), FMT420) for k, f in enumerate(clip["woven"])]
    got = deinterlaced_bgr(clip["woven"])
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))                 # the product's host route is the reference run

    def intervals(frames):
        return [(s, e) for s, e, _r in frame_select.ChangeFrameSelector(NumpyCounter(), batch=8).run(list(frames), CHANGE_AREA)]
    woven = intervals([ingest.YuvFrame(f, h, w, pf).to_bgr() for f in clip["woven"]])
    progressive = intervals([ingest.YuvFrame(f, h, w, pf).to_bgr() for f in clip["first"]])
    deinterlaced = intervals(ref)
    print("woven", woven, "\nprogressive", progressive, "\ndeinterlaced", deinterlaced)
    assert deinterlaced == progressive
    assert len(woven) < len(progressive) == len([s for s in SCHEDULE if s[0] is not None])


@pytest.mark.parametrize("batch", [7, 64])
def test_one_pass_equals_several_passes_on_the_interlaced_y4m(host_stack, tmp_path, batch):
    clip = interlaced_clip()
    path = str(tmp_path / "fields.y4m")
    ingest.write_yuv(path, clip["woven"], product_format(FMT420), fps=FPS, y4m=True, interlace="t")
    src = ingest.Y4mSource(path, wide=True, deinterlace="adaptive")
    assert src.field_order == "tff"
    decoded = list(src.frames())
    assert all(np.array_equal(a, b) for a, b in zip(decoded, deinterlaced_bgr(clip["woven"])))
    _, want = run(src, decoded, clip["truth"], "change", batch, None, sub_area=CHANGE_AREA)
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe, wide=True, deinterlace="adaptive")
    ex, got = run(stream, decoded, clip["truth"], "change", batch, None, sub_area=CHANGE_AREA)
    th.join()
    pipe.close()
    assert ex.one_pass and got == want and ex.clamped_intervals == 0 and stream.frame_count == len(decoded)
    assert len(got[0]) == len(clip["truth"]) and got[3].count(" --> ") >= 2
    src.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_extractor_command_line_deinterlaces(host_stack, tmp_path, capsys):
    clip = interlaced_clip()
    path = str(tmp_path / "fields.y4m")
    ingest.write_yuv(path, clip["woven"], product_format(FMT420), fps=FPS, y4m=True, interlace="t")
    decoded = deinterlaced_bgr(clip["woven"], thresh=12)
    src = ingest.Y4mSource(path, wide=True, deinterlace="adaptive", deinterlace_thresh=12)
    _, want = run(src, decoded, clip["truth"], "change", 8, None, sub_area=CHANGE_AREA)
    src.close()
    area = f"{CHANGE_AREA.ymin},{CHANGE_AREA.ymax},{CHANGE_AREA.xmin},{CHANGE_AREA.xmax}"
    common = ["--area", area, "--selector", "change", "--batch", "8"]
    ocr = LookupOcr(decoded, clip["truth"], text_box(CHANGE_AREA))
    assert extractor.main([path, "--deinterlace", "adaptive", "--deinterlace-thresh", "12"] + common, ocr=ocr, counter=NumpyCounter()) == 0
    assert capsys.readouterr().out == want[3] and ocr.seen == want[1] and want[3].count(" --> ") >= 2
    # without the flag the header is refused in the parser's words, with or without --wide-yuv
    for more in ([], ["--wide-yuv"]):
        assert extractor.main([path] + more + common, ocr=ocr, counter=NumpyCounter()) == 2
        assert "interlaced video (It) is not supported" in capsys.readouterr().err


def test_command_line_argument_errors_exit_with_status_2(tmp_path, capsys):
    frames = [R.random_planes(np.random.default_rng(2), 4, 6, FMT420)]
    it, im = y4m_file(tmp_path, "It", frames, name="it.y4m"), y4m_file(tmp_path, "Im", frames, name="im.y4m")
    raw = str(tmp_path / "clip.yuv")
    ingest.write_yuv(raw, frames, ingest.YuvFormat())
    ocr = LookupOcr([], [], None)
    for argv in ([it, "--deinterlace", "yadif"], [it, "--deinterlace"], [it, "--deinterlace", "adaptive", "--field-order", "top"],
                 [it, "--deinterlace", "adaptive", "--deinterlace-thresh", "ten"]):
        with pytest.raises(SystemExit) as e:
            extractor.main(argv, ocr=ocr, counter=NumpyCounter())
        assert e.value.code == 2
        capsys.readouterr()
    for argv, word in (([it, "--field-order", "tff"], "--deinterlace"), ([it, "--deinterlace-thresh", "5"], "--deinterlace"),
                       ([it, "--deinterlace", "adaptive", "--deinterlace-thresh", "256"], "0..255"),
                       ([it, "--deinterlace", "interpolate", "--deinterlace-thresh", "-1"], "0..255"),
                       ([im, "--deinterlace", "adaptive"], "Im"),
                       ([raw, "--deinterlace", "adaptive", "--field-order", "tff", "--size", "6x4", "--fps", "25"], "pix_fmt"),
                       ([raw, "--deinterlace", "adaptive", "--pix-fmt", "yuv420p", "--size", "6x4", "--fps", "25"], "field order")):
        assert extractor.main(argv, ocr=ocr, counter=NumpyCounter()) == 2, argv
        err = capsys.readouterr().err
        assert err.startswith("extractor: ") and word in err, (argv, err)
    assert ocr.seen == []
