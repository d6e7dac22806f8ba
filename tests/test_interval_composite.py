"""Interval composite on the host: which frames of an interval are used (frame_select.trim_range), IntervalCompositor fed by the numpy
restatement (tests/interval_ref.py) on the area locator's clip, extractor.CompositedSource, and
SubtitleExtractor(interval_image=...) with a scripted recogniser.  CPU only."""
import numpy as np
import pytest

import area_clip
import interval_ref
from frame_change_ref import NumpyCounter
from vse_amd import extractor, frame_select, parallel, synth

H, W, FPS = area_clip.H, area_clip.W, area_clip.FPS
AREA = extractor.SubtitleArea(ymin=int(0.78 * H), ymax=int(0.99 * H), xmin=int(0.05 * W), xmax=int(0.95 * W))
BOX = (AREA.ymin, AREA.ymax, AREA.xmin, AREA.xmax)
FADED = area_clip.TEXT_C


@pytest.fixture(scope="module")
def clip():
    """(frames, truth, intervals): make_clip with the locator tests' schedule, and its true intervals with their middle frames."""
    frames, truth = synth.make_clip(area_clip.SCHEDULE, H, W, seed=3)
    frames.setflags(write=False)
    return frames, truth, [(s, e, (s + e) // 2) for s, e, _t in truth]


def fill_masks():
    """text -> (bool mask [lh, lw] of its fill pixels, (row, column) of the mask in the AREA's patch): re-rendered as area_clip.text_boxes does."""
    gh = max(12, int(60 * H / 1080.0))
    out = {}
    for text in sorted({s[0] for s in area_clip.SCHEDULE if s[0] is not None}):
        fill, _ = synth.render_line(text, gh, np.random.default_rng([3, *text.encode()]))
        lh, lw = fill.shape[0], min(fill.shape[1], int(0.88 * W))
        yy, xx = min(int(0.99 * H) - gh - 8, H - lh - 2), (W - lw) // 2
        assert AREA.ymin <= yy and yy + lh <= AREA.ymax and AREA.xmin <= xx and xx + lw <= AREA.xmax
        out[text] = (fill[:, :lw] > 0, (yy - AREA.ymin, xx - AREA.xmin))
    return out


def fill_pixels(patch, mask, at):
    return patch[at[0]:at[0] + mask.shape[0], at[1]:at[1] + mask.shape[1]][mask]


class CountingFrames:
    """Frames in decode order that count how many were handed out."""

    def __init__(self, frames):
        self.frames, self.reads = frames, 0

    def __iter__(self):
        for f in self.frames:
            self.reads += 1
            yield f


# ---- which frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start, end, fps, trim, want", [
    (7, 7, 10.0, 0.25, (7, 7)), (7, 8, 10.0, 0.25, (7, 8)), (7, 9, 10.0, 0.25, (8, 8)), (7, 16, 10.0, 0.25, (9, 14)),
    (7, 7, 23.976, 0.25, (7, 7)), (7, 8, 23.976, 0.25, (7, 8)), (7, 9, 23.976, 0.25, (8, 8)), (7, 16, 23.976, 0.25, (11, 12)),
    (7, 16, 10.0, 0.3, (10, 13)), (7, 16, 10.0, 0.0, (7, 16)), (7, 16, 10.0, 60.0, (11, 12)), (7, 15, 10.0, 60.0, (11, 11)),
    (7, 16, 23.976, 0.125, (10, 13))])
def test_trim_range(start, end, fps, trim, want):
    """Lengths 1, 2, 3 and 10 at 10 and 23.976 fps; round(0.25 * 10) = 2 and round(0.25 * 23.976) = 6, cut to (end - start) // 2; a trim
    far beyond half the interval leaves its one or two middle frames."""
    assert frame_select.trim_range(start, end, fps, trim) == want == interval_ref.trim_range(start, end, fps, trim)
    assert want[0] <= want[1]


# ---- the compositor on a clip ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [4, 64])
def test_min_composite_keeps_text(clip, batch):
    frames, truth, ivs = clip
    fn = interval_ref.NumpyCompositor()
    comp = frame_select.IntervalCompositor(fn, mode="min", trim_seconds=0.3, batch=batch)
    patches = comp.run(list(frames), AREA, ivs, FPS)
    assert comp.area == BOX and sorted(patches) == [r for _s, _e, r in ivs]
    masks = fill_masks()
    used = 0
    for (s, e, rep), (_s, _e, text) in zip(ivs, truth):
        patch = patches[rep]
        first, last = interval_ref.trim_range(s, e, FPS, 0.3)
        used += last - first + 1
        assert patch.dtype == np.uint8 and patch.shape == (BOX[1] - BOX[0], BOX[3] - BOX[2], 3)
        want = interval_ref.composite(interval_ref.accumulate(None, frames[first - 1:last], BOX), last - first + 1, "min")
        assert np.array_equal(patch, want)
        mask, at = masks[text]
        assert mask.sum() > 200 and (fill_pixels(patch, mask, at) == 255).all()         # the text survives whole
        assert (patch <= frames[rep - 1, BOX[0]:BOX[1], BOX[2]:BOX[3]]).all()            # nothing is lighter than in the middle frame
        assert patch[~np.pad(mask, ((at[0], patch.shape[0] - at[0] - mask.shape[0]), (at[1], patch.shape[1] - at[1] - mask.shape[1])))].max() < 255
    assert fn.frames_seen == used                                                       # only frames inside a used range reach the device


def test_trim_removes_the_fade(clip):
    frames, truth, ivs = clip
    k = next(i for i, item in enumerate(t for t in area_clip.SCHEDULE if t[0] is not None) if len(item) > 2)
    assert truth[k][2] == FADED and truth[k][1] - truth[k][0] + 1 == 16
    mask, at = fill_masks()[FADED]
    rep = ivs[k][2]
    for trim, whole in ((0.3, True), (0.0, False)):
        comp = frame_select.IntervalCompositor(interval_ref.NumpyCompositor(), mode="min", trim_seconds=trim)
        patches = comp.run(list(frames), AREA, ivs, FPS, only=range(k, k + 1))
        assert sorted(patches) == [rep]
        assert bool((fill_pixels(patches[rep], mask, at) == 255).all()) == whole
        if not whole:
            assert (fill_pixels(patches[rep], mask, at) < 255).all()                     # the first faded frame holds every fill pixel down


@pytest.mark.parametrize("mode", ["max", "mean"])
def test_other_modes_match_the_restatement(clip, mode):
    frames, _truth, ivs = clip
    patches = frame_select.IntervalCompositor(interval_ref.NumpyCompositor(), mode=mode, trim_seconds=0.1, batch=5).run(iter(frames), AREA, ivs, FPS)
    for s, e, rep in ivs:
        first, last = interval_ref.trim_range(s, e, FPS, 0.1)
        assert np.array_equal(patches[rep], interval_ref.composite(interval_ref.accumulate(None, frames[first - 1:last], BOX), last - first + 1, mode))


def test_only_and_reading_stops(clip):
    frames, _truth, ivs = clip
    src = CountingFrames(frames)
    fn = interval_ref.NumpyCompositor()
    comp = frame_select.IntervalCompositor(fn, trim_seconds=0.2)
    patches = comp.run(src, AREA, ivs, FPS, only=range(1, 3))
    assert sorted(patches) == [ivs[1][2], ivs[2][2]]
    last_needed = interval_ref.trim_range(*ivs[2][:2], FPS, 0.2)[1]
    assert src.reads == last_needed < len(frames)
    assert fn.frames_seen == sum(b - a + 1 for a, b in (interval_ref.trim_range(s, e, FPS, 0.2) for s, e, _r in ivs[1:3]))
    nothing = CountingFrames(frames)
    assert comp.run(nothing, AREA, ivs, FPS, only=range(0, 0)) == {} and nothing.reads == 0
    assert comp.run(nothing, AREA, [], FPS) == {} and nothing.reads == 0


def test_area_is_clipped_like_the_selector(clip):
    frames, _truth, ivs = clip
    wide = extractor.SubtitleArea(ymin=300, ymax=H + 50, xmin=-20, xmax=W + 7)
    comp = frame_select.IntervalCompositor(interval_ref.NumpyCompositor(), trim_seconds=0)
    patches = comp.run(list(frames), wide, ivs[:1], FPS)
    assert comp.area == (300, H, 0, W) == frame_select.clip_area(wide, H, W)
    s, e, rep = ivs[0]
    assert np.array_equal(patches[rep], frames[s - 1:e, 300:H].min(0))
    with pytest.raises(ValueError):
        comp.run(list(frames), extractor.SubtitleArea(ymin=H, ymax=H + 9, xmin=0, xmax=W), ivs[:1], FPS)
    with pytest.raises(ValueError):
        comp.run(list(frames[:ivs[0][1] - 1]), AREA, ivs[:1], FPS)                        # the clip ends inside the interval
    with pytest.raises(ValueError):
        frame_select.IntervalCompositor(mode="median")


# ---- the source the recogniser reads ----------------------------------------------------------------------------------------
def test_composited_source():
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, size=(4, 20, 30, 3), dtype=np.uint8)
    keep = frames.copy()

    class Timed(extractor.ArraySource):
        @staticmethod
        def pos_msec(no):
            return 40.0 * no + 7

    src = Timed(list(frames), 25.0)
    patch = rng.integers(0, 256, size=(6, 11, 3), dtype=np.uint8)
    cs = extractor.CompositedSource(src, extractor.SubtitleArea(ymin=9, ymax=15, xmin=4, xmax=15), {3: patch})
    assert (cs.fps, cs.frame_count) == (25.0, 4) and cs.pos_msec(2) == 87.0 and not hasattr(cs, "read_raw")
    got = cs.read(3)
    assert np.array_equal(got[9:15, 4:15], patch)
    outside = np.ones((20, 30), bool)
    outside[9:15, 4:15] = False
    assert np.array_equal(got[outside], keep[2][outside])
    assert np.array_equal(frames, keep) and got is not src.read(3)                        # a copy: the source's frame is as it was
    assert cs.read(2) is src.read(2) and cs.read(5) is None                               # no patch: the plain frame
    by_area = extractor.CompositedSource(src, extractor.SubtitleArea(ymin=9, ymax=99, xmin=-3, xmax=11), {1: patch})
    assert np.array_equal(by_area.read(1)[9:15, 0:11], patch)                             # placed where the clipped area starts
    assert extractor.CompositedSource(extractor.ArraySource(list(frames), 25.0), AREA, {}).pos_msec is None


# ---- the extractor ------------------------------------------------------------------------------------------------------------
class ScriptedOcr:
    """Recognises the frame number stamped into pixel (0, 0) (outside the area) as the truth text of that frame, and keeps what it was
    shown inside the area."""

    def __init__(self, truth, batched):
        self.truth, self.seen = truth, {}
        if batched:
            self.predict_batch = lambda frames: [self.predict(np.asarray(f)) for f in frames]

    def predict(self, img):
        no = int(img[0, 0, 0]) | (int(img[0, 0, 1]) << 8)
        self.seen[no] = img[BOX[0]:BOX[1], BOX[2]:BOX[3]].copy()
        for s, e, text in self.truth:
            if s <= no <= e:
                return [[[60, 300], [580, 300], [580, 340], [60, 340]]], [(text, 0.95)]
        return [], []


def stamped(frames):
    frames = frames.copy()
    for i in range(len(frames)):
        frames[i, 0, 0, 0], frames[i, 0, 0, 1] = (i + 1) & 255, (i + 1) >> 8
    return frames


def extract(frames, truth, batched, **kw):
    src = extractor.ArraySource(list(stamped(frames)), FPS)
    ocr = ScriptedOcr(truth, batched)
    ex = extractor.SubtitleExtractor(src, ocr, sub_area=AREA, mode="fast", frame_selector="change", change_counter=NumpyCounter(),
                                     drop_score=0.0, batch=8, **kw)
    return ex, ocr, ex.run()


@pytest.mark.parametrize("batched", [False, True])
def test_extractor_interval_image(batched, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = synth.make_clip([item[:2] for item in area_clip.SCHEDULE], H, W, seed=3)       # hard cuts only: every interval exact
    plain, plain_ocr, plain_text = extract(frames, truth, batched)
    middle, middle_ocr, middle_text = extract(frames, truth, batched, interval_image="middle")
    assert middle_text == plain_text and middle.raw_lines == plain.raw_lines and middle.intervals == plain.intervals
    assert middle.interval_patches is None and sorted(middle_ocr.seen) == sorted(plain_ocr.seen)
    assert all(np.array_equal(middle_ocr.seen[no], plain_ocr.seen[no]) for no in plain_ocr.seen)

    fn = interval_ref.NumpyCompositor()
    ex, ocr, text = extract(frames, truth, batched, interval_image="min", composite_params={"accumulate_fn": fn, "trim_seconds": 0.2})
    assert ex.intervals == plain.intervals == [(s, e, (s + e) // 2) for s, e, _t in truth]
    assert sorted(ocr.seen) == sorted(ex.interval_patches) == [r for _s, _e, r in ex.intervals]
    src_frames = stamped(frames)
    for s, e, rep in ex.intervals:
        first, last = interval_ref.trim_range(s, e, FPS, 0.2)
        want = interval_ref.composite(interval_ref.accumulate(None, src_frames[first - 1:last], BOX), last - first + 1, "min")
        assert np.array_equal(ocr.seen[rep], want) and np.array_equal(ex.interval_patches[rep], want)
        assert not np.array_equal(want, plain_ocr.seen[rep])
    times = [ln for ln in text.split("\n") if " --> " in ln]
    assert times and times == [ln for ln in plain_text.split("\n") if " --> " in ln]
    assert text == plain_text and ex.raw_lines == plain.raw_lines                      # the scripted recogniser reads the stamp, not the area


def test_extractor_composites_only_its_shard(monkeypatch):
    frames, truth = synth.make_clip([item[:2] for item in area_clip.SCHEDULE], H, W, seed=3)
    src = extractor.ArraySource(list(frames), FPS)
    ex = extractor.SubtitleExtractor(src, ScriptedOcr(truth, False), sub_area=AREA, mode="fast", frame_selector="change",
                                     change_counter=NumpyCounter(), interval_image="mean", shard=(1, 2),
                                     composite_params={"accumulate_fn": interval_ref.NumpyCompositor()})
    tasks = ex.select_tasks()
    lo, hi = parallel.shard_range(len(tasks), 1, 2)
    assert 0 < lo < hi == len(tasks) == len(ex.intervals)
    shown = ex.composite_intervals(len(tasks))
    assert sorted(ex.interval_patches) == [t[1] for t in tasks[lo:hi]]
    assert shown.read(tasks[0][1]) is src.read(tasks[0][1]) and shown.read(tasks[lo][1]) is not src.read(tasks[lo][1])


def test_extractor_refuses_bad_interval_image():
    src = extractor.ArraySource([np.zeros((8, 8, 3), np.uint8)], 25.0)
    for kw in (dict(frame_selector="change", interval_image="median"), dict(frame_selector="change", interval_image=None),
               dict(frame_selector="fps", interval_image="min"), dict(interval_image="mean")):
        with pytest.raises(ValueError):
            extractor.SubtitleExtractor(src, ScriptedOcr([], False), sub_area=AREA, **kw)
    extractor.SubtitleExtractor(src, ScriptedOcr([], False), sub_area=AREA, interval_image="middle")       # the default, with any selector
