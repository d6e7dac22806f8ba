"""HDR ingest on the host: ingest.ToneMap's tables against closed forms written out again here, YuvFrame(..., tone=...).to_bgr() against
the restated integers (tests/tonemap_ref.py), the round trip synth.hdr_grade -> tone map against the SDR clip that went in, what
happens to the change selector without the tone map, the sources and both command lines.  CPU only."""
import math

import numpy as np
import pytest

import area_cells_ref
import tonemap_ref as TM
import yuv_format_ref as R
from frame_change_ref import NumpyCounter
from test_one_pass import AREA, FPS, LookupOcr, clip, host_stack, piped, run, text_box  # noqa: F401  (host_stack is a fixture)
from test_yuv_formats import bgr_source, ident, product_format
from vse_amd import area_locator, extractor, frame_select, ingest, synth


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def pq_nits(e):
    m1, m2, c1, c2, c3 = 0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875
    p = e ** (1.0 / m2)
    return 10000.0 * (max(p - c1, 0.0) / (c2 - c3 * p)) ** (1.0 / m1)


def hlg_nits(e):
    a = 0.17883277
    b, c = 1.0 - 4.0 * a, 0.5 - a * math.log(4.0 * a)
    scene = e * e / 3.0 if e <= 0.5 else (math.exp((e - c) / a) + b) / 12.0
    return 1000.0 * scene ** 1.2


def knee_curve(x, p, knee):
    if x <= knee:
        return x
    s, t = (p - knee) / (1.0 - knee), min((x - knee) / (p - knee), 1.0)
    return knee + (1.0 - knee) * s * t / (1.0 + (s - 1.0) * t)


CODES = (0, 1, 64, 777, 1500, 2040, 2081, 2600, 3000, 3333, 4079, 4080, 4081, 4095)


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
@pytest.mark.parametrize("curve,white,peak,knee", [("knee", 203.0, 1000.0, 0.8), ("clip", 203.0, 1000.0, 0.8), ("knee", 100.0, 4000.0, 0.5)])
def test_tables(transfer, curve, white, peak, knee):
    tone = ingest.ToneMap(transfer, white_nits=white, peak_nits=peak, curve=curve, knee=knee)
    a, t, m = tone.tables()
    assert (a.shape, a.dtype, t.shape, t.dtype, m.shape, m.dtype) == ((4096,), np.uint16, (7936,), np.uint8, (3, 3), np.int32)
    assert np.all(np.diff(a.astype(np.int32)) >= 0) and np.all(np.diff(t.astype(np.int32)) >= 0)
    assert a[0] == 0 and t[0] == 0 and t[-1] == 255
    assert m.sum(axis=1).tolist() == [16384] * 3 and TM.gamut_ok(m)
    assert tone.tables()[0] is a and ingest.ToneMap(transfer, white_nits=white, peak_nits=peak, curve=curve, knee=knee).tables()[0] is a      # cached
    assert tone.packed() == TM.pack_table(a, t).tobytes() and len(tone.packed()) == TM.TABLE_BYTES == 16128
    nits = pq_nits if transfer == "pq" else hlg_nits
    for i in CODES:
        x = nits(min(i / 4080.0, 1.0)) / white
        want = 65535.0 * (min(x, 1.0) if curve == "clip" else knee_curve(x, peak / white, knee))
        assert abs(int(a[i]) - want) <= 1, (i, int(a[i]), want)
    for j in (0, 1, 2, 100, 4095, 4096, 5000, 7935):
        lin = j / 65535.0 if j < 4096 else ((j - 3840) * 16 + 8) / 65535.0
        assert abs(int(t[j]) - 255.0 * lin ** (1.0 / 2.4)) <= 0.5 + 1e-9, j
    if curve == "clip":
        # saturates at the code of white_nits: the first code whose light reaches it, and every code from there on
        first = next(i for i in range(4096) if nits(min(i / 4080.0, 1.0)) >= white)
        assert np.all(a[first:] == 65535) and a[first - 1] < 65535
    else:
        assert a[-1] == 65535 or nits(1.0) < peak               # the roll-off reaches SDR white at peak_nits (HLG ends at 1000 nits)


def test_gamut_matrix():
    m = ingest.ToneMap("pq").tables()[2]
    # BT.2087's BT.2020 -> BT.709 matrix to its six printed digits, times 2^14, within one unit
    want = 16384.0 * np.array([[1.660491, -0.587641, -0.072850], [-0.124550, 1.132900, -0.008349], [-0.018151, -0.100579, 1.118730]])
    assert np.abs(m - want).max() <= 1.0
    assert np.array_equal(ingest.ToneMap("hlg", primaries="bt709").tables()[2], 16384 * np.eye(3, dtype=np.int32))
    assert np.allclose(ingest.bt2020_to_bt709() @ np.ones(3), np.ones(3), atol=1e-12)


def test_tone_map_is_a_hashable_validated_tuple():
    a, b = ingest.ToneMap("pq"), ingest.ToneMap("pq", "bt2020", 203, 1000, "knee", 0.8, 2.4)
    assert a == b and hash(a) == hash(b) and len({a, b, ingest.ToneMap("hlg")}) == 2
    assert a._fields == ("transfer", "primaries", "white_nits", "peak_nits", "curve", "knee", "gamma")
    assert tuple(a) == ("pq", "bt2020", 203.0, 1000.0, "knee", 0.8, 2.4)
    bad = [dict(transfer="sdr"), dict(primaries="p3"), dict(curve="hable"), dict(white_nits=0), dict(white_nits="bright"), dict(peak_nits=100.0),
           dict(peak_nits=20000.0), dict(knee=0.0), dict(knee=1.0), dict(gamma=0.5), dict(gamma=float("nan")), dict(white_nits=float("nan"))]
    for change in bad:
        with pytest.raises(ValueError, match=next(iter(change)) if "transfer" not in change else "transfer"):
            ingest.ToneMap(**{"transfer": "pq", **change})
    for gamut in ([[32767, 1, 0], [0, 16384, 0], [0, 0, 16384]], [[16384, 0, 0], [-32768, -1, 32767], [0, 0, 16384]]):
        assert not TM.gamut_ok(gamut)
        with pytest.raises(ValueError, match="gamut row"):
            ingest.check_gamut(gamut)
    with pytest.raises(ValueError, match="tone"):
        ingest.YuvFrame(R.random_planes(np.random.default_rng(0), 2, 2, (0, 0, 1, 8, 0, 0, 0)), 2, 2, ingest.YuvFormat(0, 0), tone="pq")


# ---- the integers ----------------------------------------------------------------------------------------------------------------------
class Tables:
    """What YuvFrame asks of a tone: tables() and packed(); hashable by identity.  Lets the host route run on random tables."""

    def __init__(self, rng):
        self.a, self.t, self.m = TM.random_tables(rng)

    def tables(self):
        return self.a, self.t, self.m

    def packed(self):
        return TM.pack_table(self.a, self.t).tobytes()


def tone_formats(depths=(8, 10, 12, 16)):
    """(sub_x, sub_y, chroma, depth, msb, matrix, full_range): every load pattern at every depth, the matrices and ranges dealt round."""
    out = []
    for depth in depths:
        for msb in ((0,) if depth == 8 else (0, 1)):
            for k, lay in enumerate([(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (1, 1, 2)]):
                out.append(lay + (depth, msb, (k + depth) % 3, (k + msb) & 1))
    return out


@pytest.mark.parametrize("fmt", tone_formats(), ids=ident)
def test_host_to_bgr_equals_reference(fmt):
    rng = np.random.default_rng(sum(fmt))
    real = ingest.ToneMap("pq" if fmt[3] & 2 else "hlg", curve="clip" if fmt[0] else "knee")
    for tone in (Tables(rng), real):
        a, t, m = tone.tables()
        for h, w in ((1, 1), (5, 7), (6, 16), (11, 37)):
            planes = R.random_planes(rng, h, w, fmt, wild=bool(h & 1))
            frame = ingest.YuvFrame(planes, h, w, product_format(fmt), tone=tone)
            whole = frame.to_bgr()
            assert whole.dtype == np.uint8 and whole.shape == (h, w, 3) and np.array_equal(whole, TM.convert(planes, fmt, a, t, m))
            for y0, y1 in ((0, h), (1, h), (0, h - 1), (h // 2, h // 2 + 1), (2, 2)):
                if 0 <= y0 <= y1 <= h:
                    band = frame[y0:y1]
                    assert band.tone is tone and np.array_equal(band.to_bgr(), whole[y0:y1]), (h, w, y0, y1)
                    sub, parity = R.sub_frame(planes, fmt, y0, y1)
                    assert np.array_equal(band.to_bgr(), TM.convert(sub, fmt, a, t, m, rows=(0, y1 - y0), parity=parity))
    # without a tone the frame is what it was
    plain = ingest.YuvFrame(planes, h, w, product_format(fmt))
    assert plain.tone is None and np.array_equal(plain.to_bgr(), R.convert(planes, fmt))


def test_interlaced_frames_carry_the_tone():
    fmt = (1, 1, 1, 10, 0, 2, 0)
    rng = np.random.default_rng(5)
    tone = Tables(rng)
    h, w = 12, 10
    prev, cur = R.random_planes(rng, h, w, fmt), R.random_planes(rng, h, w, fmt)
    f = ingest.InterlacedYuvFrame(cur, h, w, product_format(fmt), prev, "tff", "adaptive", 10, tone=tone)
    want = TM.convert(f.deinterlaced_planes(), fmt, *tone.tables())
    assert np.array_equal(f.to_bgr(), want) and f[3:9].tone is tone and np.array_equal(f[3:9].to_bgr(), want[3:9])


@pytest.mark.parametrize("depth,matrix,full", [(8, 0, 0), (10, 2, 0), (10, 1, 1), (12, 2, 1), (16, 0, 0)])
def test_grey_in_grey_out(depth, matrix, full):
    """U = V = coff: B == G == R for every Y, in 4:4:4 and in a grey format, since every row of M sums to 2^14."""
    n = 1 << min(depth, 12)
    y = (np.arange(n, dtype=np.int64) << (depth - min(depth, 12))).reshape(1, n)
    dt = R.sample_dtype((0, 0, 1, depth, 0, 0, 0))
    c = np.full((1, n), 128 << (depth - 8), dt)
    for transfer in ("pq", "hlg"):
        tone = ingest.ToneMap(transfer, primaries="bt2020")
        out = ingest.YuvFrame((y.astype(dt), c, c), 1, n, ingest.YuvFormat(0, 0, 1, depth, 0, R.MATRICES[matrix], full), tone=tone).to_bgr()
        assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 1], out[..., 2])
        grey = ingest.YuvFrame((y.astype(dt),), 1, n, ingest.YuvFormat(0, 0, 0, depth, 0, R.MATRICES[matrix], full), tone=tone).to_bgr()
        assert np.array_equal(grey, out) and out.max() > 200 and out.min() == 0


# ---- the round trip and the problem ----------------------------------------------------------------------------------------------------
RT_H, RT_W = 120, 320
RT_AREA = extractor.SubtitleArea(ymin=int(0.75 * RT_H), ymax=RT_H, xmin=0, xmax=RT_W)
RT_SCHEDULE = [(None, 2), ("the quick brown fox", 5), ("near frozen lakes", 4), (None, 2), ("seven wizards", 4), (None, 1)]
_rt = {}


def rt_clip():
    if "clip" not in _rt:
        _rt["clip"] = synth.make_clip(RT_SCHEDULE, RT_H, RT_W, seed=6)
    return _rt["clip"]


def graded(white, sub, transfer="pq"):
    key = (white, sub, transfer)
    if key not in _rt:
        _rt[key] = synth.hdr_grade(rt_clip()[0], white_nits=white, transfer=transfer, depth=10, sub=sub)
    return _rt[key]


def converted(planes_list, fmt, tone):
    return np.stack([ingest.YuvFrame(p, RT_H, RT_W, fmt, tone=tone).to_bgr() for p in planes_list])


@pytest.mark.parametrize("white", [203.0, 100.0])
def test_round_trip_444(white):
    """hdr_grade, then the clip tone map at the same white: the SDR clip comes back within 3 levels (measured: 2; EXPERIMENTS.md AD)."""
    frames, _ = rt_clip()
    fmt = ingest.YuvFormat(0, 0, 1, 10, 0, "bt2020", 0)
    got = converted(graded(white, (0, 0)), fmt, ingest.ToneMap("pq", white_nits=white, peak_nits=1000.0, curve="clip"))
    diff = np.abs(got.astype(np.int16) - frames)
    print(f"round trip 4:4:4 at {white} nits: max |diff| {diff.max()}, mean {diff.mean():.4f}")
    assert diff.max() <= 3


def test_round_trip_420():
    """4:2:0: chroma is the mean of 2 x 2 and read back nearest, so chroma edges move; the share of bytes off by more than 8 stays
    below 1 % (measured: see EXPERIMENTS.md AD)."""
    frames, _ = rt_clip()
    fmt = ingest.YuvFormat(1, 1, 1, 10, 0, "bt2020", 0)
    got = converted(graded(203.0, (1, 1)), fmt, ingest.ToneMap("pq", curve="clip"))
    diff = np.abs(got.astype(np.int16) - frames)
    share = float((diff > 8).mean())
    print(f"round trip 4:2:0 at 203 nits: share of bytes off by more than 8 {100 * share:.3f} %, max |diff| {diff.max()}")
    assert share <= 0.01


def intervals_of(frames, edge_thresh):
    got = frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=edge_thresh).run(list(frames), RT_AREA, FPS)
    return [(s, e) for s, e, _rep in got]


def test_the_problem_and_its_end():
    """Without a tone map the graded clip's white comes out at 148 and the selector loses the subtitles from edge_thresh 160 on; with
    transfer="pq", under both curves, it finds them at 128, 160 and 192, as on the SDR clip."""
    frames, truth = rt_clip()
    want = [(s, e) for s, e, _t in truth]
    assert len(want) == 3 and frames.max() == 255
    fmt = ingest.YuvFormat(0, 0, 1, 10, 0, "bt2020", 0)
    planes = graded(203.0, (0, 0))
    flat = converted(planes, fmt, None)
    assert flat.max() <= 150
    assert intervals_of(flat, 160) == [] and intervals_of(flat, 192) == []
    for thresh in (128, 160, 192):
        assert intervals_of(frames, thresh) == want
    for curve in ("knee", "clip"):
        sdr = converted(planes, fmt, ingest.ToneMap("pq", curve=curve))
        for thresh in (128, 160, 192):
            assert intervals_of(sdr, thresh) == want, (curve, thresh)


def test_hlg_round_trip():
    """The HLG route is the inverse of its grade as well (per channel on both sides)."""
    frames, _ = rt_clip()
    fmt = ingest.YuvFormat(0, 0, 1, 10, 0, "bt2020", 0)
    got = converted(graded(203.0, (0, 0), "hlg")[:4], fmt, ingest.ToneMap("hlg", curve="clip"))
    assert np.abs(got.astype(np.int16) - frames[:4]).max() <= 3


# ---- sources ---------------------------------------------------------------------------------------------------------------------------
def test_sources_attach_the_tone_map(tmp_path):
    h, w = 6, 10
    rng = np.random.default_rng(2)
    fmt = (1, 1, 1, 10, 0, 2, 0)
    pf = product_format(fmt)
    frames = [R.random_planes(rng, h, w, fmt) for _ in range(3)]
    path = str(tmp_path / "clip.y4m")
    ingest.write_yuv(path, frames, pf, fps=FPS, y4m=True)
    tone = ingest.ToneMap("pq", "bt2020", white_nits=100.0, curve="clip")
    want = [TM.convert(p, fmt, *tone.tables()) for p in frames]
    kw = dict(wide=True, matrix="bt2020", transfer="pq", tone_params={"white_nits": 100, "curve": "clip"})
    for src in (ingest.Y4mSource(path, **kw), ingest.open_source(path, **kw)):
        assert src.tone == tone
        for no, raw in enumerate(src.raw_frames(), 1):
            assert raw.tone == tone and raw[1:4].tone == tone and np.array_equal(raw.to_bgr(), want[no - 1]) and np.array_equal(src.read(no), want[no - 1])
        src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    fp, th = piped(data, 7)
    st = ingest.Y4mStream(fp, **kw)
    assert [np.array_equal(f, x) for f, x in zip(st.frames(), want)] == [True] * 3
    th.join()
    fp.close()
    # primaries follow the matrix unless given; without transfer nothing changes
    src = ingest.Y4mSource(path, wide=True, matrix="bt709", transfer="hlg")
    assert src.tone == ingest.ToneMap("hlg", "bt709") and src.read_raw(1).tone == src.tone
    src.close()
    src = ingest.Y4mSource(path, wide=True, matrix="bt709", transfer="hlg", tone_params={"primaries": "bt2020"})
    assert src.tone.primaries == "bt2020"
    src.close()
    src = ingest.Y4mSource(path, wide=True, matrix="bt2020")
    assert src.tone is None and src.read_raw(1).tone is None and np.array_equal(src.read(1), R.convert(frames[0], fmt))
    src.close()
    # interlaced frames carry it too
    src = ingest.Y4mSource(path, wide=True, matrix="bt2020", deinterlace="adaptive", field_order="tff", transfer="pq")
    raw = src.read_raw(2)
    assert isinstance(raw, ingest.InterlacedYuvFrame) and raw.tone == ingest.ToneMap("pq")
    assert np.array_equal(raw.to_bgr(), TM.convert(raw.deinterlaced_planes(), fmt, *raw.tone.tables()))
    src.close()
    # a headerless P010 file
    p010 = (1, 1, 2, 10, 1, 2, 0)
    planes = [R.random_planes(rng, h, w, p010) for _ in range(2)]
    raw_path = str(tmp_path / "clip.p010")
    ingest.write_yuv(raw_path, planes, product_format(p010))
    src = ingest.open_source(raw_path, size=(w, h), fps=FPS, matrix="bt2020", transfer="hlg")
    assert isinstance(src, ingest.YuvSource) and src.tone == ingest.ToneMap("hlg")
    assert np.array_equal(src.read(2), TM.convert(planes[1], p010, *src.tone.tables()))
    src.close()


def test_sources_refuse_naming_the_option(tmp_path):
    h, w = 4, 6
    rng = np.random.default_rng(3)
    path10, path8 = str(tmp_path / "ten.y4m"), str(tmp_path / "eight.y4m")
    ingest.write_yuv(path10, [R.random_planes(rng, h, w, (1, 1, 1, 10, 0, 0, 0))], ingest.YuvFormat(depth=10), fps=FPS, y4m=True)
    ingest.write_y4m(path8, [R.random_planes(rng, h, w, (1, 1, 1, 8, 0, 0, 0))], FPS)
    raw, npy = str(tmp_path / "clip.yuv"), str(tmp_path / "clip.npy")
    ingest.write_yuv420(raw, [R.random_planes(rng, h, w, (1, 1, 1, 8, 0, 0, 0))])
    np.save(npy, np.zeros((1, h, w, 3), np.uint8))
    for call in (lambda: ingest.Y4mSource(path8, transfer="pq"), lambda: ingest.open_source(path8, transfer="pq"),
                 lambda: ingest.open_source(path10, transfer="hlg"), lambda: ingest.open_source(raw, size=(w, h), fps=FPS, transfer="pq"),
                 lambda: ingest.open_source(npy, fps=FPS, transfer="pq"), lambda: ingest.open_source(str(tmp_path / "film.avi"), transfer="pq"),
                 lambda: ingest.Y4mStream(open(path8, "rb"), transfer="pq")):
        with pytest.raises(ValueError, match="transfer="):
            call()
    with pytest.raises(ValueError, match="transfer"):
        ingest.Y4mSource(path10, wide=True, transfer="gamma")
    with pytest.raises(ValueError, match="tone_params"):
        ingest.Y4mSource(path10, wide=True, tone_params={"white_nits": 100})
    with pytest.raises(ValueError, match="tone_params"):
        ingest.Y4mSource(path10, wide=True, transfer="pq", tone_params={"nits": 100})
    with pytest.raises(ValueError, match="white_nits"):
        ingest.open_source(path10, wide=True, transfer="pq", tone_params={"white_nits": -1})
    # the 8-bit 4:2:0 reader without these keywords is what it was
    src = ingest.open_source(path8)
    assert isinstance(src.read_raw(1), ingest.Yuv420Frame)
    src.close()


# ---- the command lines -----------------------------------------------------------------------------------------------------------------
def pq_clip(tmp_path):
    """The change clip graded as 10-bit 4:2:0 PQ BT.2020 in a Y4M file -> (path, its frames tone-mapped on the host, truth)."""
    frames, truth = clip("change")
    path = str(tmp_path / "pq.y4m")
    ingest.write_yuv(path, synth.hdr_grade(frames, depth=10, sub=(1, 1)), ingest.YuvFormat(depth=10), fps=FPS, y4m=True)
    src = ingest.Y4mSource(path, wide=True, matrix="bt2020", transfer="pq")
    decoded = list(src.frames())
    src.close()
    return path, decoded, truth


def test_extractor_command_line_takes_a_transfer(host_stack, tmp_path, monkeypatch, capsys):
    path, decoded, truth = pq_clip(tmp_path)
    _, want = run(bgr_source(decoded), decoded, truth, "change", 8, None)
    assert want[3].count(" --> ") == len(truth)
    # the SDR original gives the same SRT
    frames, _ = clip("change")
    _, sdr = run(bgr_source(list(frames)), list(frames), truth, "change", 8, None)
    assert sdr[3] == want[3]
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"
    common = ["--area", area, "--selector", "change", "--batch", "8"]
    hdr = ["--wide-yuv", "--matrix", "bt2020", "--transfer", "pq"]
    out = str(tmp_path / "out.srt")
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main([path, "-o", out] + hdr + common, ocr=ocr, counter=NumpyCounter()) == 0
    assert open(out).read() == want[3] and ocr.seen == want[1]
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 4099)
    monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main(["-"] + hdr + common, ocr=ocr, counter=NumpyCounter()) == 0
    pipe.close()
    th.join()
    assert capsys.readouterr().out == want[3]
    # the tone options reach the source: another white point gives other frames, which the scripted recogniser does not know
    src = ingest.open_source(path, wide=True, matrix="bt2020", **extractor.tone_arguments(
        type("Args", (), dict(transfer="pq", white_nits=100.0, peak_nits=400.0, tone_curve="clip"))()))
    assert src.tone == ingest.ToneMap("pq", "bt2020", 100.0, 400.0, "clip")
    src.close()
    # refusals: exit status 2 and the message on standard error, nothing recognised
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    for argv, word in (([path, "--transfer", "pq"], "transfer="), ([path, "--wide-yuv", "--white-nits", "100"], "--transfer"),
                       ([path, "--wide-yuv", "--tone-curve", "clip"], "--transfer"), ([path, "--wide-yuv", "--transfer", "pq", "--white-nits", "0"], "white_nits"),
                       ([str(tmp_path / "clip.npy"), "--fps", "12", "--transfer", "hlg"], "transfer=")):
        assert extractor.main(argv + common, ocr=ocr, counter=NumpyCounter()) == 2 and ocr.seen == []
        err = capsys.readouterr().err
        assert err.startswith("extractor: ") and word in err, (argv, err)


def test_locator_command_line_takes_a_transfer(tmp_path, capsys):
    path, decoded, _ = pq_clip(tmp_path)
    want = area_locator.AreaLocator(area_cells_ref.NumpyCells()).run(decoded, FPS)
    assert want is not None
    hdr = ["--wide-yuv", "--matrix", "bt2020", "--transfer", "pq"]
    assert area_locator.main([path] + hdr, cells_fn=area_cells_ref.NumpyCells()) == 0
    assert capsys.readouterr().out.split() == [str(v) for v in (want.ymin, want.ymax, want.xmin, want.xmax)]
    assert area_locator.main([path, "--transfer", "pq"], cells_fn=area_cells_ref.NumpyCells()) == 2
    assert "transfer=" in capsys.readouterr().err
    assert area_locator.main([path, "--wide-yuv", "--peak-nits", "400"], cells_fn=area_cells_ref.NumpyCells()) == 2
    assert "--transfer" in capsys.readouterr().err
