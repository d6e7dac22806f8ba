"""The streaming composite on the host: frame_select.StreamingCompositor, driven by the numpy restatement of vse_interval_stream
(tests/interval_stream_ref.py, whose ring raises on a frame that is not there), gives the patches of IntervalCompositor.run on random
timelines under every selector lag; SubtitleExtractor with composite_params={"streaming": True} equals today's several-pass composite run
in several passes, in one pass and over a pipe; what it refuses; the command line.  CPU only: scripted counters and recogniser."""
import hashlib

import numpy as np
import pytest

import interval_rank_ref
import interval_ref
import interval_stream_ref
from frame_change_ref import NumpyCounter
from frame_hold_ref import NumpyHoldCounter
from test_one_pass import AREA, FPS, HOLD, clip, piped
from test_frame_hold import BAND
from vse_amd import engine, extractor, frame_select, ingest

MODES = interval_ref.MODES
SMALL = extractor.SubtitleArea(ymin=2, ymax=6, xmin=1, xmax=9)
MIN_EDGES, RATIO = 40, 0.5


# ---- the planner on random timelines ----------------------------------------------------------------------------------------------
class ScriptedRows:
    """count_fn of every selector: hands out the rows of a whole clip's timeline as the device would, trailing the frames by `lag`."""

    def __init__(self, rows, lag):
        self.rows, self.lag, self.fed = np.asarray(rows, np.int32).reshape(-1, 3), lag, 0

    def __call__(self, frames, area, edge_thresh, *more):
        if len(more) == 1:                                # the change selector: reset
            self.fed = 0 if more[0] else self.fed
            fed, flush = self.fed, False
            self.fed += len(frames)
        else:                                             # hold: (hold, fed, flush); bounded: (hold, max_hold, fed, flush)
            fed, flush = more[-2], more[-1]
        done = lambda f: f if flush else max(0, f - self.lag)          # noqa: E731
        return self.rows[max(0, fed - self.lag):done(fed + len(frames))]


def selector(kind, rows, min_frames, batch, comp):
    kw = dict(min_edges=MIN_EDGES, change_ratio=RATIO, min_frames=min_frames, batch=batch, compositor=comp)
    if kind == "change":
        return frame_select.ChangeFrameSelector(ScriptedRows(rows, 0), **kw), 0
    if kind == "hold":
        return frame_select.HoldFrameSelector(ScriptedRows(rows, 3), hold_frames=4, **kw), 3
    return frame_select.HoldFrameSelector(ScriptedRows(rows, 20), hold_frames=2, max_hold_frames=20, **kw), 20


def random_rows(rng, n):
    """The timelines of test_one_pass's tracker test, with longer runs: present frames, rare cuts and gaps."""
    edges = rng.choice([0, 39, 40, 80, 120], size=n, p=[0.04, 0.04, 0.3, 0.3, 0.32])
    a = rng.choice([0, 1, 20, 60], size=n, p=[0.6, 0.25, 0.1, 0.05])
    v = rng.choice([0, 1, 19, 21, 80], size=n, p=[0.5, 0.3, 0.08, 0.06, 0.06])
    return np.stack([edges, a, v], axis=1).astype(np.int32)


def check_timeline(frames, rows, kind, mode, trim, batch, min_frames):
    """-> (the intervals, the streamer) after holding the streamed patches against IntervalCompositor.run on the same intervals."""
    fn = interval_stream_ref.NumpyStreamer()
    comp = frame_select.StreamingCompositor(fn, mode=mode, trim_seconds=float(trim))
    sel, lag = selector(kind, rows, min_frames, batch, comp)
    intervals = sel.run(list(frames), SMALL, fps=1.0)
    mf = min_frames if kind == "change" else max(min_frames, sel.hold)
    assert intervals == frame_select.change_intervals(rows, MIN_EDGES, RATIO, mf)
    want = frame_select.IntervalCompositor(interval_ref.NumpyCompositor(), mode=mode, trim_seconds=float(trim), batch=batch).run(
        list(frames), SMALL, intervals, 1.0)
    what = (kind, mode, trim, batch, min_frames, len(frames))
    assert sorted(comp.patches) == sorted(want) == [r for _s, _e, r in intervals], what
    for r in want:
        assert comp.patches[r].dtype == np.uint8 and np.array_equal(comp.patches[r], want[r]), (what, r)
    assert comp.cap == lag + trim + 1 and comp.peak_ring <= comp.cap and fn.peak_ring <= comp.cap, what
    return intervals, fn


def test_streamed_patches_equal_the_second_pass_on_random_timelines():
    rng = np.random.default_rng(2024)
    clips = intervals = short = dropped = ends_inside = 0
    for k in range(360):
        kind, mode = ("change", "hold", "bounded")[k % 3], MODES[(k // 3) % 3]
        trim, batch = (0, 1, 2, 6)[(k // 9) % 4], (1, 7, 64)[(k // 36) % 3]
        min_frames = (1, 2, 8)[int(rng.integers(0, 3))]
        n = int(rng.integers(1, 140))
        rows = random_rows(rng, n)
        if n and k % 4 == 0:
            rows[-int(rng.integers(1, 12)):, 0] = 120          # the clip ends inside a run
            rows[-1, 1:] = 0
        frames = rng.integers(0, 256, size=(n, 7, 10, 3), dtype=np.uint8)
        got, _fn = check_timeline(frames, rows, kind, mode, trim, batch, min_frames)
        clips += 1
        intervals += len(got)
        short += sum(1 for s, e, _r in got if e - s + 1 < 2 * trim + 1)
        ends_inside += bool(got and got[-1][1] == n)
        dropped += len(frame_select.change_intervals(rows, MIN_EDGES, RATIO, 1)) - len(got)
    assert clips == 360 and intervals > 1000 and short > 50 and dropped > 100 and ends_inside > 30, (intervals, short, dropped, ends_inside)


@pytest.mark.parametrize("mode", MODES)
def test_more_closings_in_a_batch_than_one_call_takes(mode):
    """min_frames 1 and a cut before every frame: 64 intervals close in a batch of 64, in calls of at most 32 segments on the same batch."""
    rng = np.random.default_rng(5)
    n = 150
    rows = np.tile(np.array([[120, 100, 100]], np.int32), (n, 1))
    frames = rng.integers(0, 256, size=(n, 7, 10, 3), dtype=np.uint8)
    got, fn = check_timeline(frames, rows, "change", mode, 1, 64, 1)
    assert len(got) == n and fn.calls >= 2 * 2 + 1 and fn.calls > -(-n // 64) + 1
    got, fn = check_timeline(frames, rows, "hold", mode, 0, 64, 1)             # hold 4: nothing is as long, nothing is kept
    assert got == []


def test_planner_asserts_its_ring():
    """The cap is a condition: a selector that trails by more than it said is caught before a frame is lost."""
    comp = frame_select.StreamingCompositor(interval_stream_ref.NumpyStreamer(), trim_seconds=1.0)
    rows = np.tile(np.array([[120, 0, 0]], np.int32), (30, 1))
    sel = frame_select.HoldFrameSelector(ScriptedRows(rows, 9), hold_frames=4, min_edges=MIN_EDGES, batch=7, compositor=comp)
    with pytest.raises(AssertionError, match="StreamingCompositor"):
        sel.run(list(np.zeros((30, 7, 10, 3), np.uint8)), SMALL, fps=1.0)
    with pytest.raises(ValueError, match="mode"):
        frame_select.StreamingCompositor(mode="quantile")


def test_reference_ring_raises_on_a_frame_that_is_gone():
    st = interval_stream_ref.Stream(3)
    frames = np.arange(5 * 2 * 2 * 3, dtype=np.uint8).reshape(5, 2, 2, 3)
    area = (0, 2, 0, 2)
    st.stream(frames, area, 0, [], 3, "min")                                   # frames 3, 4, 5 are stored
    got = st.stream(frames[:0], area, 5, [(3, 5, interval_stream_ref.EMIT, 3)], 6, "max")
    assert np.array_equal(got[0], frames[2:5].max(0))
    st.stream(frames[:1], area, 5, [], 7, "min")                               # frame 6 passes by and is not stored
    with pytest.raises(LookupError):
        st.stream(frames[:0], area, 6, [(4, 6, interval_stream_ref.EMIT, 3)], 7, "min")      # inside the window, but never stored
    got = st.stream(frames[:2], area, 6, [(4, 5, interval_stream_ref.EMIT, 2)], 7, "min")    # frame 7 replaces frame 4 after the read
    assert np.array_equal(got[0], frames[3:5].min(0))
    with pytest.raises(LookupError):
        st.stream(frames[:0], area, 8, [(6, 6, 0, 0)], 9, "min")                             # its slot still holds frame 3
    with pytest.raises(ValueError):
        st.stream(frames[:0], area, 8, [(5, 5, interval_stream_ref.EMIT, 1)], 9, "min")      # outside (fed - cap, fed + n]
    assert (interval_stream_ref.CONTINUE, interval_stream_ref.EMIT, interval_stream_ref.MAX_SEGS) == \
        (engine.INTERVAL_SEG_CONTINUE, engine.INTERVAL_SEG_EMIT, engine.INTERVAL_STREAM_MAX_SEGS)


# ---- the extractor ----------------------------------------------------------------------------------------------------------------
class AreaOcr:
    """Recognises a frame by the bytes above the subtitle area (every frame of the clips differs there): the truth text of that frame
    number; keeps what it was shown inside the area."""

    def __init__(self, frames, truth, area):
        self.y0, self.y1 = int(area.ymin), int(area.ymax)
        self.nos = {hashlib.sha1(np.ascontiguousarray(f[:self.y0]).tobytes()).digest(): no for no, f in enumerate(frames, 1)}
        assert len(self.nos) == len(frames)
        self.truth, self.seen, self.shown = truth, [], {}
        self.box = [[40, self.y0 + 4], [280, self.y0 + 4], [280, self.y1 - 4], [40, self.y1 - 4]]

    def predict(self, img):
        no = self.nos[hashlib.sha1(np.ascontiguousarray(img[:self.y0]).tobytes()).digest()]
        self.seen.append(no)
        self.shown[no] = np.array(img[self.y0:self.y1])
        for s, e, text in self.truth:
            if s <= no <= e:
                return [self.box], [(text, 0.95)]
        return [], []

    def predict_batch(self, frames):
        return [self.predict(np.asarray(f)) for f in frames]


def kind_kwargs(kind):
    if kind == "hold":
        return dict(sub_area=BAND, frame_selector="hold", change_counter=NumpyHoldCounter(), change_params={"hold_frames": HOLD})
    return dict(sub_area=AREA, frame_selector="change", change_counter=NumpyCounter())


def extract(source, frames, truth, kind, batch, one_pass, image, params):
    kw = kind_kwargs(kind)
    ocr = AreaOcr(frames, truth, kw["sub_area"])
    ex = extractor.SubtitleExtractor(source, ocr, mode="fast", drop_score=0.0, batch=batch, one_pass=one_pass, interval_image=image,
                                     composite_params=params, **kw)
    text = ex.run()
    return ex, ocr, (ex.intervals, ocr.seen, ex.raw_lines, text)


def same_pictures(ex, ocr, want_ex, want_ocr):
    reps = [r for _s, _e, r in want_ex.intervals]
    assert sorted(ex.interval_patches) == sorted(want_ex.interval_patches) == reps
    for r in reps:
        assert np.array_equal(ex.interval_patches[r], want_ex.interval_patches[r]), r
        assert np.array_equal(ocr.shown[r], want_ocr.shown[r]), r


@pytest.fixture
def host_stack(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames


@pytest.mark.parametrize("image", ["min", "mean"])
@pytest.mark.parametrize("batch", [7, 64])
@pytest.mark.parametrize("kind", ["change", "hold"])
def test_extractor_streaming_equals_the_composite_pass(host_stack, kind, batch, image):
    frames, truth = clip(kind)
    src = extractor.ArraySource(list(frames), FPS)
    want_ex, want_ocr, want = extract(src, frames, truth, kind, batch, None, image,
                                      {"accumulate_fn": interval_ref.NumpyCompositor(), "trim_seconds": 0.2})
    assert [(s, e) for s, e, _r in want[0]] == [(s, e) for s, e, _t in truth] and want[3].count(" --> ") >= 2
    assert any(not np.array_equal(want_ocr.shown[r], frames[r - 1][want_ocr.y0:want_ocr.y1]) for _s, _e, r in want[0])
    for one_pass in (False, True):
        fn = interval_stream_ref.NumpyStreamer()
        ex, ocr, got = extract(src, frames, truth, kind, batch, one_pass, image,
                               {"streaming": True, "stream_fn": fn, "trim_seconds": 0.2, "keep_patches": True})
        assert ex.one_pass == one_pass and got == want and fn.calls > 0 and ex.clamped_intervals == 0
        same_pictures(ex, ocr, want_ex, want_ocr)
    # one pass drops a picture once its frame has been recognised, unless told to keep it; several passes keep them
    fn = interval_stream_ref.NumpyStreamer()
    ex, ocr, got = extract(src, frames, truth, kind, batch, True, image, {"streaming": True, "stream_fn": fn, "trim_seconds": 0.2})
    assert got == want and ex.interval_patches is None and all(np.array_equal(ocr.shown[r], want_ocr.shown[r]) for r in ocr.shown)
    ex, ocr, got = extract(src, frames, truth, kind, batch, False, image, {"streaming": True, "stream_fn": fn, "trim_seconds": 0.2})
    assert got == want
    same_pictures(ex, ocr, want_ex, want_ocr)


@pytest.mark.parametrize("kind", ["change", "hold"])
def test_extractor_streaming_over_a_piped_stream(host_stack, tmp_path, kind):
    frames, truth = clip(kind)
    path = str(tmp_path / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    want_ex, want_ocr, want = extract(src, decoded, truth, kind, 7, None, "min", {"accumulate_fn": interval_ref.NumpyCompositor()})
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe)
    ex, ocr, got = extract(stream, decoded, truth, kind, 7, None, "min",
                           {"streaming": True, "stream_fn": interval_stream_ref.NumpyStreamer(), "keep_patches": True})
    th.join()
    pipe.close()
    src.close()
    assert ex.one_pass and got == want and stream.frame_count == len(frames) and got[3].count(" --> ") >= 2
    same_pictures(ex, ocr, want_ex, want_ocr)


def test_streaming_refusals():
    frames, truth = clip("change")
    src = extractor.ArraySource(list(frames), FPS)
    base = dict(sub_area=AREA, frame_selector="change")
    on = {"streaming": True}
    for kw, word in ((dict(interval_image="quantile", composite_params=on), "quantile"),
                     (dict(interval_image="middle", composite_params=on), "middle"),
                     (dict(composite_params=on), "middle"),
                     (dict(interval_image="min", composite_params=on, shard=(0, 2)), "shard"),
                     (dict(interval_image="min", composite_params={**on, "accumulate_fn": None}), "accumulate_fn"),
                     (dict(interval_image="min", composite_params={**on, "samples": 3}), "samples")):
        for one_pass in (False, True):
            with pytest.raises(ValueError) as e:
                extractor.SubtitleExtractor(src, None, one_pass=one_pass, **base, **kw)
            assert "streaming" in str(e.value) and word in str(e.value), (kw, str(e.value))
    with pytest.raises(ValueError) as e:
        extractor.SubtitleExtractor(src, None, interval_image="min", interval_text="fused", composite_params=on, **base)
    assert "streaming" in str(e.value) and "fused" in str(e.value)
    # without the key, one pass refuses the composites as before, in the same words
    with pytest.raises(ValueError) as e:
        extractor.SubtitleExtractor(src, None, one_pass=True, interval_image="min", composite_params={"trim_seconds": 0.1}, **base)
    assert "interval_image" in str(e.value) and "second look" in str(e.value)
    for one_pass in (False, True):
        for image in MODES:
            ex = extractor.SubtitleExtractor(src, None, one_pass=one_pass, interval_image=image, composite_params={**on, "keep_patches": True},
                                             **base)
            assert ex.streaming and ex.one_pass == one_pass
    # the extractor's own keys mean nothing without the option, and say so before any work
    for params, word in (({"streaming": False, "keep_patches": True}, "keep_patches"), ({"keep_patches": False}, "keep_patches"),
                         ({"stream_fn": None}, "stream_fn")):
        with pytest.raises(ValueError) as e:
            extractor.SubtitleExtractor(src, None, interval_image="min", composite_params=params, **base)
        assert "streaming" in str(e.value) and word in str(e.value)


@pytest.mark.parametrize("image", ["min", "quantile"])
def test_a_falsy_streaming_key_is_the_run_without_it(host_stack, image):
    """The key is taken out before the remaining params reach IntervalCompositor / IntervalQuantile / StreamingCompositor."""
    frames, truth = clip("change")
    src = extractor.ArraySource(list(frames), FPS)
    fns = (lambda: {"rank_fn": interval_rank_ref.NumpyRanker(), "samples": 5}) if image == "quantile" else \
        (lambda: {"accumulate_fn": interval_ref.NumpyCompositor()})
    want_ex, want_ocr, want = extract(src, frames, truth, "change", 7, None, image, fns())
    given = {"streaming": False, **fns()}
    ex, ocr, got = extract(src, frames, truth, "change", 7, None, image, given)
    assert not ex.streaming and "streaming" not in ex.composite_params and given["streaming"] is False       # (the caller's dict is its own)
    assert got == want
    same_pictures(ex, ocr, want_ex, want_ocr)
    ex = extractor.SubtitleExtractor(src, None, interval_image="min", composite_params={"streaming": True, "keep_patches": True,
                                                                                       "trim_seconds": 0.1}, **kind_kwargs("change"))
    assert ex.streaming and ex.keep_patches and ex.composite_params == {"trim_seconds": 0.1}


def test_command_line_streaming_composite(host_stack, tmp_path, monkeypatch, capsys):
    frames, truth = clip("change")
    path, out = str(tmp_path / "clip.y4m"), str(tmp_path / "out.srt")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    _want_ex, want_ocr, want = extract(src, decoded, truth, "change", 8, None, "max", {"accumulate_fn": interval_ref.NumpyCompositor()})
    src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"

    def main(args, **fns):
        pipe, th = piped(data, 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = AreaOcr(decoded, truth, AREA)
        rc = extractor.main(args, ocr=ocr, counter=NumpyCounter(), **fns)
        pipe.close()
        th.join()
        return rc, ocr
    common = ["--area", area, "--selector", "change", "--batch", "8", "-o", out]
    fn = interval_stream_ref.NumpyStreamer()
    rc, ocr = main(["-", "--interval-image", "max", "--streaming-composite"] + common, stream_fn=fn)
    assert rc == 0 and ocr.seen == want[1] and open(out).read() == want[3] and fn.calls > 0
    assert all(np.array_equal(ocr.shown[r], want_ocr.shown[r]) for r in want[1])
    fn = interval_stream_ref.NumpyStreamer()
    rc, ocr = main([path, "--interval-image", "max", "--streaming-composite"] + common, stream_fn=fn)        # a file: several passes
    assert rc == 0 and ocr.seen == want[1] and open(out).read() == want[3] and fn.calls > 0
    capsys.readouterr()
    for bad, word in ((["-", "--streaming-composite"] + common, "--streaming-composite"),
                      (["-", "--interval-image", "quantile", "--streaming-composite"] + common, "--streaming-composite"),
                      (["-", "--interval-image", "max"] + common, "second look")):
        rc, ocr = main(bad, stream_fn=fn)
        err = capsys.readouterr().err
        assert rc == 2 and err.startswith("extractor: ") and word in err and ocr.seen == [], bad
    rc = extractor.main([path, "--interval-image", "max", "--streaming-composite"] + common, ocr=AreaOcr(decoded, truth, AREA),
                        counter=NumpyCounter(), composite_fn=interval_ref.NumpyCompositor())
    assert rc == 2 and "composite_fn" in capsys.readouterr().err             # an injected composite_fn would never be called
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    assert "--streaming-composite" in capsys.readouterr().out
