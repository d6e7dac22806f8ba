"""Interval quantile on the host: the rank a quantile stands for (frame_select.quantile_rank), IntervalQuantile fed by the numpy
restatement (tests/interval_rank_ref.py) on the area locator's clip, what the median does that min / max cannot (polarity, an outlier
frame), SubtitleExtractor(interval_image="quantile") with a scripted recogniser, and the command line's flags.  CPU only."""
import numpy as np
import pytest

import area_clip
import interval_rank_ref
import interval_ref
from frame_change_ref import NumpyCounter
from vse_amd import extractor, frame_select, parallel, synth

H, W, FPS = area_clip.H, area_clip.W, area_clip.FPS
AREA = extractor.SubtitleArea(ymin=int(0.78 * H), ymax=int(0.99 * H), xmin=int(0.05 * W), xmax=int(0.95 * W))
BOX = (AREA.ymin, AREA.ymax, AREA.xmin, AREA.xmax)


@pytest.fixture(scope="module")
def clip():
    """(frames, truth, intervals): make_clip with the locator tests' schedule, and its true intervals with their middle frames."""
    frames, truth = synth.make_clip(area_clip.SCHEDULE, H, W, seed=3)
    frames.setflags(write=False)
    return frames, truth, [(s, e, (s + e) // 2) for s, e, _t in truth]


class CountingFrames:
    """Frames in decode order that count how many were handed out."""

    def __init__(self, frames):
        self.frames, self.reads = frames, 0

    def __iter__(self):
        for f in self.frames:
            self.reads += 1
            yield f


class RowCounter:
    """A frame that counts the row slices taken of it (what IntervalQuantile stages) and is otherwise the array."""

    def __init__(self, arr, no, log):
        self.arr, self.no, self.log, self.shape = arr, no, log, arr.shape

    def __getitem__(self, key):
        self.log.append((self.no, key))
        return self.arr[key]


# ---- the rank of a quantile -------------------------------------------------------------------------------------------------
def test_quantile_rank_table():
    for k in range(1, 64):
        assert frame_select.quantile_rank(0, k) == 0 and frame_select.quantile_rank(0.0, k) == 0
        assert frame_select.quantile_rank(1, k) == k - 1 and frame_select.quantile_rank(1.0, k) == k - 1
        assert frame_select.quantile_rank(0.5, k) == k // 2                            # odd k: the median; even k: the upper middle
        if k % 2:
            assert frame_select.quantile_rank(0.5, k) == (k - 1) // 2
        assert all(0 <= frame_select.quantile_rank(q / 20, k) < k for q in range(21))
    assert frame_select.quantile_rank(0.5, 4) == 2
    assert frame_select.quantile_rank(0.1, 15) == 1
    assert frame_select.quantile_rank(0.9, 15) == 13
    assert frame_select.quantile_rank(0.25, 9) == 2 and frame_select.quantile_rank(0.75, 9) == 6


# ---- sampling ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples, batch", [(5, 8), (15, 64), (1, 4), (3, 3)])
def test_patches_are_the_rank_of_the_sampled_frames(clip, samples, batch):
    frames, _truth, ivs = clip
    fn = interval_rank_ref.NumpyRanker()
    comp = frame_select.IntervalQuantile(fn, quantile=0.5, samples=samples, trim_seconds=0.2, batch=batch)
    patches = comp.run(list(frames), AREA, ivs, FPS)
    assert comp.area == BOX and comp.patches is patches and sorted(patches) == [r for _s, _e, r in ivs]
    want_calls = []
    for s, e, rep in ivs:
        nos, _pos = frame_select.fuse_samples(s, e, rep, FPS, samples, 0.2)
        k = len(nos)
        first, last = interval_ref.trim_range(s, e, FPS, 0.2)
        assert k == min(samples, last - first + 1)
        want = interval_rank_ref.rank(frames[[n - 1 for n in nos]], BOX, frame_select.quantile_rank(0.5, k))
        assert patches[rep].dtype == np.uint8 and patches[rep].shape == (BOX[1] - BOX[0], BOX[3] - BOX[2], 3)
        assert np.array_equal(patches[rep], want)
        want_calls.append((k, frame_select.quantile_rank(0.5, k)))
    assert fn.calls == want_calls                                                    # one call per interval, on its own samples


def test_only_the_sampled_rows_are_staged_and_reading_stops(clip):
    frames, _truth, ivs = clip
    log = []
    src = CountingFrames([RowCounter(f, i + 1, log) for i, f in enumerate(frames)])
    fn = interval_rank_ref.NumpyRanker()
    comp = frame_select.IntervalQuantile(fn, samples=4, trim_seconds=0.2, batch=8)
    patches = comp.run(src, AREA, ivs, FPS, only=range(1, 3))
    assert sorted(patches) == [ivs[1][2], ivs[2][2]]
    nos = [n for s, e, rep in ivs[1:3] for n in frame_select.fuse_samples(s, e, rep, FPS, 4, 0.2)[0]]
    assert [no for no, _key in log] == nos                                           # only the sampled frames are touched at all ...
    assert all(key == slice(BOX[0], BOX[1]) for _no, key in log)                     # ... and only the area's rows of them
    assert src.reads == nos[-1] < len(frames)                                        # nothing is read beyond the last sample
    assert fn.frames_seen == len(nos)
    nothing = CountingFrames(frames)
    assert comp.run(nothing, AREA, ivs, FPS, only=range(0, 0)) == {} and nothing.reads == 0
    assert comp.run(nothing, AREA, [], FPS) == {} and nothing.reads == 0


def test_whole_intervals_share_a_staged_batch(clip, monkeypatch):
    """batch 8, 3 samples per interval: two intervals per staged batch, never a split one."""
    frames, _truth, ivs = clip
    sizes = []
    real = frame_select.staging.staged_batches

    def spy(batches, uploader):
        for items, data in real(batches, uploader):
            sizes.append(len(items))
            yield items, data
    monkeypatch.setattr(frame_select.staging, "staged_batches", spy)
    frame_select.IntervalQuantile(interval_rank_ref.NumpyRanker(), samples=3, trim_seconds=0.0, batch=8).run(list(frames), AREA, ivs, FPS)
    assert len(ivs) >= 3 and sum(sizes) == 3 * len(ivs) and all(n == 6 for n in sizes[:-1]) and sizes[-1] in (3, 6)


def test_value_errors(clip):
    frames, _truth, ivs = clip
    fn = interval_rank_ref.NumpyRanker()
    for kw in (dict(quantile=-0.01), dict(quantile=1.01), dict(samples=0), dict(samples=64), dict(samples=9, batch=8),
               dict(samples=64, batch=128)):
        with pytest.raises(ValueError):
            frame_select.IntervalQuantile(fn, **kw)
    frame_select.IntervalQuantile(fn, quantile=0, samples=63, batch=64)               # the limits themselves
    frame_select.IntervalQuantile(fn, quantile=1, samples=8, batch=8)
    comp = frame_select.IntervalQuantile(fn, samples=5, trim_seconds=0.0)
    with pytest.raises(ValueError):
        comp.run(list(frames), AREA, [ivs[1], ivs[0]], FPS)                            # descending
    with pytest.raises(ValueError):
        comp.run(list(frames), AREA, [ivs[0], (ivs[0][1], ivs[1][1], ivs[1][2])], FPS)  # overlapping
    with pytest.raises(ValueError):
        comp.run(list(frames[:ivs[0][1] - 1]), AREA, ivs[:1], FPS)                    # the clip ends before the last sample
    with pytest.raises(ValueError):
        comp.run(list(frames), extractor.SubtitleArea(ymin=H, ymax=H + 9, xmin=0, xmax=W), ivs[:1], FPS)
    with pytest.raises(ValueError):
        frame_select.IntervalCompositor(mode="median")                               # the compositor's modes are as they were
    assert frame_select.COMPOSITE_MODES == ("min", "max", "mean")


# ---- polarity and outliers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text, lo, hi, outlier", [(235, 0, 200, 0), (16, 60, 256, 255)])
def test_median_needs_no_polarity_and_survives_an_outlier(text, lo, hi, outlier):
    """A static mask over per-frame noise in a 9-frame interval, one frame replaced by an outlier: with light text the min composite is
    0 at every mask byte (with dark text the max is 255) and the median is the text's value, with the same settings for both."""
    rng = np.random.default_rng(text)
    h, w = 24, 40
    mask = np.zeros((h, w), bool)
    mask[6:18:2, 5:35] = True
    mask[8:16, 10:14] = True
    frames = rng.integers(lo, hi, size=(9, h, w, 3)).astype(np.uint8)
    frames[:, mask] = text
    frames[4] = outlier
    area = extractor.SubtitleArea(ymin=0, ymax=h, xmin=0, xmax=w)
    ivs = [(1, 9, 5)]
    ruined = frame_select.IntervalCompositor(interval_ref.NumpyCompositor(), mode="min" if text > 128 else "max", trim_seconds=0)
    assert (ruined.run(list(frames), area, ivs, FPS)[5][mask] == outlier).all()
    comp = frame_select.IntervalQuantile(interval_rank_ref.NumpyRanker(), quantile=0.5, samples=15, trim_seconds=0)
    patch = comp.run(list(frames), area, ivs, FPS)[5]
    assert (patch[mask] == text).all()
    assert (patch[~mask] != text).any() and (patch[~mask] != outlier).all()          # the background is neither the text nor the outlier


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


@pytest.fixture(scope="module")
def hard_cuts():
    return synth.make_clip([item[:2] for item in area_clip.SCHEDULE], H, W, seed=3)       # hard cuts only: every interval exact


@pytest.mark.parametrize("batched", [False, True])
def test_extractor_interval_image_quantile(hard_cuts, batched, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = hard_cuts
    plain, plain_ocr, plain_text = extract(frames, truth, batched)
    fn = interval_rank_ref.NumpyRanker()
    params = {"rank_fn": fn, "quantile": 0.5, "samples": 7, "trim_seconds": 0.2}
    ex, ocr, text = extract(frames, truth, batched, interval_image="quantile", composite_params=params)
    assert ex.intervals == plain.intervals == [(s, e, (s + e) // 2) for s, e, _t in truth]
    assert sorted(ocr.seen) == sorted(ex.interval_patches) == [r for _s, _e, r in ex.intervals]
    src_frames = stamped(frames)
    for s, e, rep in ex.intervals:
        nos, _pos = frame_select.fuse_samples(s, e, rep, FPS, 7, 0.2)
        want = interval_rank_ref.rank(src_frames[[n - 1 for n in nos]], BOX, frame_select.quantile_rank(0.5, len(nos)))
        assert np.array_equal(ocr.seen[rep], want) and np.array_equal(ex.interval_patches[rep], want)      # the patch, in the rep frame
        assert not np.array_equal(want, plain_ocr.seen[rep])
    times = [ln for ln in text.split("\n") if " --> " in ln]
    assert times and times == [ln for ln in plain_text.split("\n") if " --> " in ln]
    assert text == plain_text and ex.raw_lines == plain.raw_lines                      # the scripted recogniser reads the stamp, not the area


def test_extractor_quantile_composites_only_its_shard(hard_cuts):
    frames, truth = hard_cuts
    src = extractor.ArraySource(list(frames), FPS)
    ex = extractor.SubtitleExtractor(src, ScriptedOcr(truth, False), sub_area=AREA, mode="fast", frame_selector="change",
                                     change_counter=NumpyCounter(), interval_image="quantile", shard=(1, 2),
                                     composite_params={"rank_fn": interval_rank_ref.NumpyRanker(), "samples": 3})
    tasks = ex.select_tasks()
    lo, hi = parallel.shard_range(len(tasks), 1, 2)
    assert 0 < lo < hi == len(tasks) == len(ex.intervals)
    shown = ex.composite_intervals(len(tasks))
    assert sorted(ex.interval_patches) == [t[1] for t in tasks[lo:hi]]
    assert shown.read(tasks[0][1]) is src.read(tasks[0][1]) and shown.read(tasks[lo][1]) is not src.read(tasks[lo][1])


def test_extractor_refusals():
    src = extractor.ArraySource([np.zeros((8, 8, 3), np.uint8)], 25.0)
    ocr = ScriptedOcr([], False)
    for kw in (dict(frame_selector="fps", interval_image="quantile"), dict(interval_image="quantile"),
               dict(frame_selector="change", interval_image="quantile", interval_text="fused"),
               dict(frame_selector="hold", interval_image="quantile", interval_text="fused"),
               dict(frame_selector="change", interval_image="median"), dict(frame_selector="change", interval_image="quantiles"),
               dict(frame_selector="change", interval_image=None)):
        with pytest.raises(ValueError):
            extractor.SubtitleExtractor(src, ocr, sub_area=AREA, **kw)
    for selector in ("change", "hold"):
        extractor.SubtitleExtractor(src, ocr, sub_area=AREA, frame_selector=selector, interval_image="quantile")
        with pytest.raises(ValueError, match="second look") as err:
            extractor.SubtitleExtractor(src, ocr, sub_area=AREA, frame_selector=selector, interval_image="quantile", one_pass=True)
        assert str(err.value) == ("interval_image='quantile' is not available in one pass (a sequential source, or one_pass=True): it needs a "
                                  "second look at frames already gone")


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_command_line(hard_cuts, tmp_path, capsys):
    frames, truth = hard_cuts
    path, out = str(tmp_path / "clip.npy"), str(tmp_path / "out.srt")
    np.save(path, stamped(frames))
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"
    base = [path, "--fps", str(FPS), "--area", area, "--selector", "change", "--batch", "16", "-o", out]

    def api(**kw):
        src = extractor.ArraySource(list(stamped(frames)), FPS)
        ocr = ScriptedOcr(truth, False)
        ex = extractor.SubtitleExtractor(src, ocr, sub_area=AREA, mode="fast", frame_selector="change", change_counter=NumpyCounter(), batch=16, **kw)
        return ex.run(), ocr

    want, want_ocr = api(interval_image="quantile", composite_params={"rank_fn": interval_rank_ref.NumpyRanker(), "quantile": 0.5, "samples": 9})
    ocr, fn = ScriptedOcr(truth, False), interval_rank_ref.NumpyRanker()
    rc = extractor.main(base + ["--interval-image", "quantile", "--quantile", "0.5", "--interval-samples", "9"], ocr=ocr, counter=NumpyCounter(),
                        composite_fn=fn)
    assert rc == 0 and open(out).read() == want and want.count(" --> ") == len(truth)
    assert fn.calls and max(k for k, _r in fn.calls) <= 9
    assert sorted(ocr.seen) == sorted(want_ocr.seen) and all(np.array_equal(ocr.seen[no], want_ocr.seen[no]) for no in ocr.seen)

    want, want_ocr = api(interval_image="min", composite_params={"accumulate_fn": interval_ref.NumpyCompositor()})
    ocr, fn = ScriptedOcr(truth, False), interval_ref.NumpyCompositor()
    rc = extractor.main(base + ["--interval-image", "min"], ocr=ocr, counter=NumpyCounter(), composite_fn=fn)
    assert rc == 0 and open(out).read() == want and fn.calls
    assert sorted(ocr.seen) == sorted(want_ocr.seen) and all(np.array_equal(ocr.seen[no], want_ocr.seen[no]) for no in ocr.seen)

    capsys.readouterr()
    for bad in (["--interval-image", "quantile", "--quantile", "1.5"], ["--interval-image", "quantile", "--interval-samples", "9", "--batch", "4"],
                ["--interval-image", "quantile", "--interval-samples", "0"]):
        ocr = ScriptedOcr(truth, False)
        rc = extractor.main(base + bad, ocr=ocr, counter=NumpyCounter(), composite_fn=interval_rank_ref.NumpyRanker())
        err = capsys.readouterr().err
        assert rc == 2 and err.startswith("extractor: ") and ocr.seen == {}, bad
    with pytest.raises(SystemExit) as exc:
        extractor.main(base + ["--interval-image", "median"])
    assert exc.value.code == 2
