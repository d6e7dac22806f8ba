"""One pass over a sequential source, on the host: frame_select.IntervalTracker against change_intervals, ingest.Y4mStream over an OS pipe
against Y4mSource on the same bytes, SubtitleExtractor(one_pass=True) against the multi-pass run (intervals, frames recognised, raw.txt
lines, SRT), what it keeps and what the cap does, what it refuses, the command line, and the BT.709 integers (tests/yuv709_ref.py).
CPU only: numpy counters (frame_change_ref, frame_hold_ref) and a scripted recogniser."""
import gc
import hashlib
import logging
import os
import threading
import weakref

import numpy as np
import pytest

import yuv709_ref
import yuv_ref
from frame_change_ref import NumpyCounter
from frame_hold_ref import NumpyHoldCounter
from test_frame_hold import BAND, MOVING
from vse_amd import extractor, frame_select, ingest, synth

H, W, FPS = 360, 640, 12.0
AREA = extractor.SubtitleArea(ymin=int(0.75 * H), ymax=H, xmin=0, xmax=W)
# the schedule of tests/test_gpu_frame_change.py::test_extractor_change_selector_on_engine (hard cuts: every interval exact)
SCHEDULE = [(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4), ("near frozen lakes", 8), (None, 2)]
HOLD = 5
_cache = {}


def clip(kind):
    if kind not in _cache:
        _cache[kind] = synth.make_clip(SCHEDULE, H, W, seed=6) if kind == "change" else synth.make_moving_clip(MOVING)
    return _cache[kind]


def selector_kwargs(kind):
    """SubtitleExtractor arguments of the selector `kind` on clip(kind)'s frames (the fps sampler runs on the change clip)."""
    if kind == "hold":
        return dict(sub_area=BAND, frame_selector="hold", change_counter=NumpyHoldCounter(), change_params={"hold_frames": HOLD})
    if kind == "change":
        return dict(sub_area=AREA, frame_selector="change", change_counter=NumpyCounter())
    return dict(sub_area=AREA, frame_selector="fps", extract_frequency=4)


# ---- the tracker ----------------------------------------------------------------------------------------------------------------
def brute_open_start(rows, min_edges, ratio):
    """First frame of the run that is open after `rows`, by the definition: walk back from the last row while no cut intervenes."""
    t = len(rows)
    if t == 0 or rows[-1][0] < min_edges:
        return None
    while t > 1:
        e, a, v = rows[t - 1]
        prev = rows[t - 2][0]
        if prev < min_edges or (prev + a and (a + v) / (prev + a) >= ratio):
            break
        t -= 1
    return t


@pytest.mark.parametrize("min_frames", [2, HOLD])
def test_tracker_fed_in_pieces_equals_change_intervals(min_frames):
    rng = np.random.default_rng(100 + min_frames)
    min_edges, ratio = 40, 0.5
    total = 0
    for _ in range(2000):
        n = int(rng.integers(0, 61))
        # edges straddle min_edges; (appeared + vanished) against the union prev + appeared lies around the ratio threshold and far
        # from it; absent frames and cuts are rare enough for runs of five frames and more to exist
        edges = rng.choice([0, 39, 40, 41, 80, 120], size=n, p=[0.06, 0.06, 0.22, 0.22, 0.22, 0.22])
        a = rng.choice([0, 1, 20, 40, 60], size=n, p=[0.5, 0.2, 0.1, 0.1, 0.1])
        v = rng.choice([0, 1, 19, 20, 21, 40, 80], size=n, p=[0.4, 0.2, 0.08, 0.08, 0.08, 0.08, 0.08])
        rows = [tuple(int(x) for x in r) for r in zip(edges, a, v)]
        want = frame_select.change_intervals(np.asarray(rows, np.int32).reshape(-1, 3), min_edges, ratio, min_frames)
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, size=int(rng.integers(0, 6))))
        tr = frame_select.IntervalTracker(min_edges, ratio, min_frames)
        got, pos = [], 0
        for c in cuts + [n]:
            got += tr.feed(rows[pos:c])
            pos = c
            assert tr.fed == pos and tr.open_start == brute_open_start(rows[:pos], min_edges, ratio)
        got += tr.flush()
        assert got == want and tr.open_start is None
        assert all(r == (s + e) // 2 and e - s + 1 >= min_frames for s, e, r in got)
        total += len(got)
    assert total > 2000, total                            # the sequences do hold intervals
    assert frame_select.hold_intervals(np.asarray(rows, np.int32).reshape(-1, 3), min_edges, HOLD, ratio) == \
        frame_select.change_intervals(np.asarray(rows, np.int32).reshape(-1, 3), min_edges, ratio, HOLD)


# ---- the reader -----------------------------------------------------------------------------------------------------------------
def piped(data, chunk):
    """A binary file object that reads `data` from an OS pipe, unbuffered (short reads reach the reader), written by a thread in
    pieces of `chunk` bytes -> (file object, thread)."""
    r, w = os.pipe()

    def write():
        try:
            for i in range(0, len(data), chunk):
                os.write(w, data[i:i + chunk])
        except BrokenPipeError:
            pass
        finally:
            os.close(w)
    th = threading.Thread(target=write, daemon=True)
    th.start()
    return os.fdopen(r, "rb", buffering=0), th


def y4m_bytes(header, triples, frame_header=b"FRAME\n"):
    return header + b"".join(frame_header + b"".join(np.ascontiguousarray(p).tobytes() for p in tr) for tr in triples)


@pytest.mark.parametrize("chunk", [1, 7, 4099])
@pytest.mark.parametrize("hw", [(6, 8), (5, 7)])
def test_stream_over_a_pipe_equals_the_file_source(tmp_path, hw, chunk):
    h, w = hw
    rng = np.random.default_rng(h * 100 + chunk)
    triples = [yuv_ref.random_planes(rng, h, w, "i420") for _ in range(5)]
    data = y4m_bytes(b"YUV4MPEG2 W%d H%d F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n" % (w, h), triples, b"FRAME Ip XFOO=1\n")
    path = str(tmp_path / "clip.y4m")
    with open(path, "wb") as fp:
        fp.write(data)
    src = ingest.Y4mSource(path)
    fp, th = piped(data, chunk)
    st = ingest.Y4mStream(fp)
    assert (st.width, st.height, st.layout, st.fps) == (src.width, src.height, "i420", src.fps)
    assert st.frame_count is None and not hasattr(st, "read") and not hasattr(st, "read_raw")
    got = list(st.raw_frames())
    th.join()
    assert st.frame_count == src.frame_count == len(got) == 5
    for no, raw in enumerate(got, 1):
        assert isinstance(raw, ingest.Yuv420Frame) and raw.shape == (h, w, 3)
        assert all(np.array_equal(a, b) for a, b in zip(raw.planes, src.read_raw(no).planes))
        assert np.array_equal(raw.to_bgr(), src.read(no)) and np.array_equal(raw.to_bgr(), yuv_ref.convert(triples[no - 1], "i420"))
        assert raw.planes[0].base is not got[no % 5].planes[0].base                    # every frame owns its bytes
    assert [st.pos_msec(k) for k in (-1, 0, 4, 5)] == [src.pos_msec(k) for k in (-1, 0, 4, 5)]
    fp.close()
    fp, th = piped(data, chunk)
    assert all(np.array_equal(a, b) for a, b in zip(ingest.Y4mStream(fp).frames(), src.frames()))
    th.join()
    fp.close()
    src.close()


def test_stream_drops_a_partial_last_frame(tmp_path):
    triples = [yuv_ref.random_planes(np.random.default_rng(8), 4, 6, "i420") for _ in range(3)]
    data = y4m_bytes(b"YUV4MPEG2 W6 H4 F25:1\n", triples)
    per = 6 + 4 * 6 * 3 // 2
    path = str(tmp_path / "cut.y4m")
    # cut inside the payload, right behind / inside / in front of the frame header, inside the frame before, nowhere
    for cut, frames in [(1, 2), (per - 7, 2), (per - 6, 2), (per - 5, 2), (per - 3, 2), (per, 2), (per + 2, 1), (0, 3)]:
        with open(path, "wb") as fp:
            fp.write(data[:len(data) - cut])
        assert ingest.Y4mSource(path).frame_count == frames
        fp, th = piped(data[:len(data) - cut], 5)
        st = ingest.Y4mStream(fp)
        got = list(st.frames())
        th.join()
        fp.close()
        assert st.frame_count == len(got) == frames, cut
        assert np.array_equal(got[-1], yuv_ref.convert(triples[frames - 1], "i420"))
    # inside the parameters of a FRAME header
    fp, th = piped(data + b"FRAME Ip XFO", 5)
    st = ingest.Y4mStream(fp)
    assert len(list(st.raw_frames())) == st.frame_count == 3
    th.join()
    fp.close()


def test_stream_garbage_between_frames_names_the_offset():
    triples = [yuv_ref.random_planes(np.random.default_rng(11), 4, 6, "i420") for _ in range(2)]
    head = b"YUV4MPEG2 W6 H4 F25:1\n"
    one = y4m_bytes(b"", triples[:1])
    for junk in (b"junkjunkjunk", b"FRAMEX\n" + b"\0" * 40, b"RIFF"):
        fp, th = piped(head + one + junk + y4m_bytes(b"", triples[1:]), 7)
        st = ingest.Y4mStream(fp)
        with pytest.raises(ValueError) as e:
            list(st.raw_frames())
        assert f"offset {len(head) + len(one)} " in str(e.value), (junk, str(e.value))
        fp.close()
        th.join()
    fp, th = piped(b"RIFF....AVI ", 7)
    with pytest.raises(ValueError):
        ingest.Y4mStream(fp)
    fp.close()
    th.join()


@pytest.mark.parametrize("token", ["C422", "C420p10", "It", "XCOLORRANGE=FULL", "C444", "Cmono", "C420p16", "Ib", "Im"])
def test_stream_refuses_what_the_file_source_refuses(tmp_path, token):
    data = y4m_bytes(b"YUV4MPEG2 W2 H2 F25:1 " + token.encode() + b"\n", [yuv_ref.random_planes(np.random.default_rng(10), 2, 2, "i420")])
    path = str(tmp_path / "bad.y4m")
    with open(path, "wb") as fp:
        fp.write(data)
    with pytest.raises(ValueError) as of_file:
        ingest.Y4mSource(path)
    fp, th = piped(data, 3)
    with pytest.raises(ValueError) as of_stream:
        ingest.Y4mStream(fp, name=path)
    fp.close()
    th.join()
    assert token in str(of_stream.value) and str(of_stream.value) == str(of_file.value)          # one parser, one message


def test_stream_frame_rate_and_stdin(monkeypatch):
    one = [yuv_ref.random_planes(np.random.default_rng(9), 2, 2, "i420")]
    for head in (b"YUV4MPEG2 W2 H2 F0:0\n", b"YUV4MPEG2 W2 H2\n"):
        fp, th = piped(y4m_bytes(head, one), 64)
        with pytest.raises(ValueError, match="fps"):
            ingest.Y4mStream(fp)
        fp.close()
        th.join()
        fp, th = piped(y4m_bytes(head, one), 64)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": fp})())
        st = ingest.open_source("-", fps=12.5)
        assert isinstance(st, ingest.Y4mStream) and st.fps == 12.5 and len(list(st.frames())) == 1 and st.frame_count == 1
        fp.close()
        th.join()


# ---- one pass against the multi-pass run ----------------------------------------------------------------------------------------
class LookupOcr:
    """Recognises a frame by its bytes: the truth text of the frame number that `frames` (BGR, 1-based) gives it."""

    def __init__(self, frames, truth, box):
        self.nos = {hashlib.sha1(np.ascontiguousarray(f).tobytes()).digest(): no for no, f in enumerate(frames, 1)}
        self.truth, self.box, self.seen = truth, box, []

    def predict(self, img):
        no = self.nos[hashlib.sha1(np.ascontiguousarray(img).tobytes()).digest()]
        self.seen.append(no)
        for s, e, text in self.truth:
            if s <= no <= e:
                return [self.box], [(text, 0.95)]
        return [], []

    def predict_batch(self, frames):
        return [self.predict(np.asarray(f)) for f in frames]


def text_box(area):
    y0, y1 = int(area.ymin) + 4, int(area.ymax) - 4
    return [[40, y0], [280, y0], [280, y1], [40, y1]]


def run(source, frames, truth, kind, batch, one_pass, **more):
    kw = {**selector_kwargs(kind), **more}
    ocr = LookupOcr(frames, truth, text_box(kw["sub_area"]))
    ex = extractor.SubtitleExtractor(source, ocr, mode="fast", drop_score=0.0, batch=batch, one_pass=one_pass, **kw)
    text = ex.run()
    return ex, (ex.intervals, ocr.seen, ex.raw_lines, text)


@pytest.fixture
def host_stack(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames


@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("kind", ["fps", "change", "hold"])
def test_one_pass_equals_multi_pass_on_an_array_source(host_stack, kind, batch):
    frames, truth = clip("hold" if kind == "hold" else "change")
    src = extractor.ArraySource(list(frames), FPS)
    _, want = run(src, frames, truth, kind, batch, None)
    ex, got = run(src, frames, truth, kind, batch, True)
    assert got == want and ex.clamped_intervals == 0
    assert len(got[1]) > 0 and got[3].count(" --> ") >= 2
    if kind == "fps":
        assert got[0] is None and got[1] == list(range(1, len(frames) + 1, 3))           # int(12 // 4) = 3
    else:
        assert [(s, e) for s, e, _r in got[0]] == [(s, e) for s, e, _t in truth]          # ... and they are the clip's truth
        assert got[1] == [(s + e) // 2 for s, e, _t in truth]


@pytest.mark.parametrize("batch", [7, 64])
@pytest.mark.parametrize("kind", ["fps", "change", "hold"])
def test_one_pass_over_a_piped_stream_equals_the_file(host_stack, tmp_path, kind, batch):
    frames, truth = clip("hold" if kind == "hold" else "change")
    path = str(tmp_path / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    _, want = run(src, decoded, truth, kind, batch, None)
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe)
    ex, got = run(stream, decoded, truth, kind, batch, None)
    th.join()
    pipe.close()
    assert ex.one_pass and got == want and ex.clamped_intervals == 0 and stream.frame_count == len(frames)
    assert got[3].count(" --> ") >= 2
    if kind != "fps":
        assert [(s, e) for s, e, _r in got[0]] == [(s, e) for s, e, _t in truth]
    src.close()


# ---- what is kept ---------------------------------------------------------------------------------------------------------------
class RecordingSource:
    """A sequential source that hands out a fresh copy of each frame and watches how many of them are alive whenever it decodes one."""

    def __init__(self, frames, fps):
        self._frames, self.fps, self.frame_count = frames, fps, None
        self.alive, self.peak = [], 0

    def frames(self):
        for f in self._frames:
            gc.collect()
            self.alive = [r for r in self.alive if r() is not None]
            self.peak = max(self.peak, len(self.alive))
            f = f.copy()
            self.alive.append(weakref.ref(f))
            yield f
            del f


@pytest.mark.parametrize("kind,batch", [("change", 1), ("change", 4), ("hold", 1), ("hold", 4)])
def test_retention_is_half_the_longest_run(host_stack, kind, batch):
    if kind == "change":
        frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", 41), ("near frozen lakes", 12), (None, 3)], 120, 320, seed=3)
    else:
        frames, truth = clip("hold")
    longest = max(e - s + 1 for s, e, _t in truth)
    src = RecordingSource(frames, FPS)
    ex, got = run(src, frames, truth, kind, batch, None, **({"sub_area": extractor.SubtitleArea(60, 120, 0, 320)} if kind == "change" else {}))
    assert [(s, e) for s, e, _r in got[0]] == [(s, e) for s, e, _t in truth] and ex.clamped_intervals == 0
    bound = longest // 2 + 2 * batch + (HOLD if kind == "hold" else 0)
    assert longest // 2 <= src.peak <= bound and ex.peak_retained <= bound, (src.peak, ex.peak_retained, bound)
    assert src.peak < len(frames) // 2                    # far from keeping the clip


def test_retain_bytes_clamps_the_rep_and_nothing_else(host_stack, caplog):
    frames, truth = synth.make_clip([(None, 3), ("the quick brown fox", 40), (None, 3)], 120, 320, seed=4)
    (s, e, _t), = truth
    src = extractor.ArraySource(list(frames), FPS)
    kw = dict(sub_area=extractor.SubtitleArea(60, 120, 0, 320), frame_selector="change", mode="fast", drop_score=0.0, batch=4)
    ocr = LookupOcr(frames, truth, text_box(kw["sub_area"]))
    want_text = extractor.SubtitleExtractor(src, ocr, change_counter=NumpyCounter(), **kw).run()
    ocr = LookupOcr(frames, truth, text_box(kw["sub_area"]))
    ex = extractor.SubtitleExtractor(src, ocr, change_counter=NumpyCounter(), one_pass=True, retain_bytes=1, **kw)
    with caplog.at_level(logging.WARNING, logger="vse_amd.extractor"):
        text = ex.run()
    # with room for nothing, a batch leaves the last frame it showed the tracker and nothing older: when frame e + 1 closes the run,
    # the frames still there are the last frame of the batch before, (e // 4) * 4, and that batch's own: the oldest at or after the middle
    rep = (e // 4) * 4
    assert (s + e) // 2 < rep <= e
    assert ex.intervals == [(s, e, rep)] and ocr.seen == [rep] and ex.clamped_intervals == 1
    assert text == want_text and text.count(" --> ") == 1                       # start and end, hence the times, and the text
    assert len([r for r in caplog.records if "retain_bytes" in r.getMessage()]) == 1
    assert ex.peak_retained <= 2 * 4


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,kw", [("sub_area", dict(sub_area="auto")), ("mode", dict(sub_area=AREA, mode="accurate")),
                                        ("interval_image", dict(sub_area=AREA, frame_selector="change", interval_image="min")),
                                        ("interval_text", dict(sub_area=AREA, frame_selector="change", interval_text="fused")),
                                        ("shard", dict(shard=(0, 2)))])
def test_one_pass_refuses_what_needs_a_second_look(option, kw):
    frames, truth = clip("change")
    fp, th = piped(y4m_bytes(b"YUV4MPEG2 W2 H2 F25:1\n", []), 64)
    for source, more in ((ingest.Y4mStream(fp), {}), (extractor.ArraySource(list(frames), FPS), {"one_pass": True})):
        with pytest.raises(ValueError) as e:
            extractor.SubtitleExtractor(source, LookupOcr([], truth, None), **kw, **more)
        assert option in str(e.value) and "second look" in str(e.value)
    with pytest.raises(ValueError, match="one_pass=False"):
        extractor.SubtitleExtractor(ingest.Y4mStream.__new__(ingest.Y4mStream), LookupOcr([], truth, None), one_pass=False)
    fp.close()
    th.join()
    # the same options on a seekable source, in several passes: accepted as before
    extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], truth, None), **kw)


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_command_line_reads_a_pipe(host_stack, tmp_path, monkeypatch, capsys):
    frames, truth = clip("change")
    path, out, txt = str(tmp_path / "clip.y4m"), str(tmp_path / "out.srt"), str(tmp_path / "out.txt")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    _, want = run(src, decoded, truth, "change", 8, None)
    with open(path, "rb") as fp:
        data = fp.read()
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"

    def main(args):
        pipe, th = piped(data, 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = LookupOcr(decoded, truth, text_box(AREA))
        rc = extractor.main(args, ocr=ocr, counter=NumpyCounter())
        pipe.close()
        th.join()
        return rc, ocr
    rc, ocr = main(["-", "--area", area, "--selector", "change", "--batch", "8", "-o", out, "--txt", txt])
    assert rc == 0 and ocr.seen == want[1]
    assert open(out).read() == want[3] and want[3].count(" --> ") == len(truth)
    assert open(txt).read() == extractor.SubtitleExtractor.srt2txt(want[3]) != ""
    assert capsys.readouterr().out == ""
    rc, _ = main(["-", "--area", area, "--selector", "change", "--batch", "8"])            # no -o: standard output
    assert rc == 0 and capsys.readouterr().out == want[3]
    rc, _ = main([path, "--area", area, "--selector", "change", "--batch", "8", "-o", out])     # a file goes through open_source
    assert rc == 0 and open(out).read() == want[3]
    for bad in (["-", "--area", "1,2,3"], ["-", "--area", "auto"], ["-", "--area", area, "--mode", "accurate"],
                [str(tmp_path / "missing.y4m")]):
        rc, ocr = main(bad)
        err = capsys.readouterr().err
        assert rc == 2 and err.startswith("extractor: ") and ocr.seen == [], bad
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    assert "BT.709" in capsys.readouterr().out


# ---- BT.709 ---------------------------------------------------------------------------------------------------------------------
def test_bt709_reference_anchors_and_factors():
    assert yuv709_ref.factors() == (yuv709_ref.BU, yuv709_ref.GU, yuv709_ref.GV, yuv709_ref.RV) == ingest.YUV_MATRICES["bt709"]
    for (y, u, v), bgr in yuv709_ref.ANCHORS:
        assert yuv709_ref.pixels(y, u, v).tolist() == bgr, (y, u, v)
        one = ingest.Yuv420Frame((np.array([[y]], np.uint8), np.array([[u, v]], np.uint8)), 1, 1, "nv12", matrix="bt709")
        assert one.to_bgr().tolist() == [[bgr]] and one.to_bgr("bt601").tolist() == [[yuv_ref.pixels(y, u, v).tolist()]]
    # the largest sum over the whole input domain fits int32, every factor 24 bits
    y, u, v = (np.array(a, np.int64) for a in np.meshgrid([0, 16, 255], [0, 255], [0, 255], indexing="ij"))
    c = np.maximum(y - 16, 0) * 1220542 + 2 ** 19
    sums = np.stack([c + yuv709_ref.BU * (u - 128), c + yuv709_ref.GU * (u - 128) + yuv709_ref.GV * (v - 128), c + yuv709_ref.RV * (v - 128)])
    assert np.abs(sums).max() == 573540604 < 5.8e8 < 2 ** 31 and max(abs(f) for f in yuv709_ref.factors()) < 2 ** 23


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (6, 10), (16, 32)])
def test_host_bt709_equals_reference(hw, layout):
    h, w = hw
    rng = np.random.default_rng(h * 31 + w)
    for mid in (False, True):
        planes = yuv_ref.random_planes(rng, h, w, layout, mid=mid)
        frame = ingest.Yuv420Frame(planes, h, w, layout, matrix="bt709")
        want = yuv709_ref.convert(planes, layout)
        assert np.array_equal(frame.to_bgr(), want)
        assert np.array_equal(frame[1:].to_bgr(), want[1:]) and frame[1:].matrix == "bt709"          # the matrix travels with a slice
        assert np.array_equal(ingest.Yuv420Frame(planes, h, w, layout).to_bgr(), yuv_ref.convert(planes, layout))      # default: BT.601
        if h * w >= 64 and not mid:
            assert not np.array_equal(want, yuv_ref.convert(planes, layout))
    with pytest.raises(ValueError, match="matrix"):
        ingest.Yuv420Frame(planes, h, w, layout, matrix="bt2020")


def test_luma_only_pictures_are_the_same_under_both_matrices(tmp_path):
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    grey = (y, np.full((8, 8), 128, np.uint8), np.full((8, 8), 128, np.uint8))
    assert np.array_equal(yuv709_ref.convert(grey, "i420"), yuv_ref.convert(grey, "i420"))
    path = str(tmp_path / "grey.y4m")
    ingest.write_y4m(path, [grey, yuv_ref.random_planes(np.random.default_rng(1), 16, 16, "i420")], 25)
    a, b = ingest.open_source(path), ingest.open_source(path, matrix="bt709")
    assert (a.matrix, b.matrix) == ("bt601", "bt709")
    assert np.array_equal(a.read(1), b.read(1)) and not np.array_equal(a.read(2), b.read(2))
    assert np.array_equal(b.read(2), yuv709_ref.convert(b.read_raw(2).planes, "i420")) and b.read_raw(2).matrix == "bt709"
    with open(path, "rb") as fp:
        st = ingest.Y4mStream(fp, matrix="bt709")
        assert np.array_equal(list(st.frames())[1], b.read(2))
    raw = str(tmp_path / "grey.nv12")
    ingest.write_yuv420(raw, [grey], "nv12")
    assert np.array_equal(ingest.open_source(raw, fps=25, size=(16, 16), matrix="bt709").read(1), a.read(1))
