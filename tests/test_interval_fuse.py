"""Interval fusion on the host: the numpy restatement of vse_ctc_fuse (tests/ctc_fuse_ref.py) on hand-made posteriors, which frames of
an interval frame_select.IntervalFuser samples and how it batches them, fed to a scripted fuse_fn, and
SubtitleExtractor(interval_text="fused") with a scripted recogniser.  CPU only."""
import numpy as np
import pytest

import area_clip
import ctc_fuse_ref
from frame_change_ref import NumpyCounter
from vse_amd import extractor, frame_select, parallel, synth

H, W, FPS = area_clip.H, area_clip.W, area_clip.FPS
AREA = extractor.SubtitleArea(ymin=int(0.78 * H), ymax=int(0.99 * H), xmin=int(0.05 * W), xmax=int(0.95 * W))


# ---- the reference --------------------------------------------------------------------------------------------------------------
def test_fusion_beats_a_vote_over_strings():
    """T = 6, 8 classes, truth [3,0,5,0,2,0] at 0.9; row k has, at step [0,2,4][k], 0.45 on the truth and 0.55 on class 7.  Every row
    alone decodes to another wrong string, no two agree; the mean has 0.75 on the truth at the contested steps."""
    truth, ncls = [3, 0, 5, 0, 2, 0], 8
    probs = np.full((3, 6, ncls), np.float32(0.1 / 7), np.float32)
    for k in range(3):
        for s, c in enumerate(truth):
            probs[k, s, c] = 0.9
        s = [0, 2, 4][k]
        probs[k, s] = 0.0
        probs[k, s, truth[s]], probs[k, s, 7] = 0.45, 0.55
    alone = [ctc_fuse_ref.ctc_greedy(*(a[0] for a in ctc_fuse_ref.fuse(probs[k:k + 1], [0, 1])))[0] for k in range(3)]
    assert alone == [[7, 5, 2], [3, 7, 2], [3, 5, 7]]
    idx, maxp = ctc_fuse_ref.fuse(probs, [0, 3])
    assert idx.dtype == np.int32 and maxp.dtype == np.float32 and idx.shape == maxp.shape == (1, 6)
    assert idx[0].tolist() == truth
    ids, conf = ctc_fuse_ref.ctc_greedy(idx[0], maxp[0])
    assert ids == [3, 5, 2]
    want = (np.float32(0.9) + np.float32(0.9) + np.float32(0.45)) / np.float32(3)
    assert [maxp[0, s] for s in (0, 2, 4)] == [want] * 3 and abs(float(want) - 0.75) < 1e-6 and abs(conf - 0.75) < 1e-6
    # the order of the adds is the members' order: (0.45 + 0.9) + 0.9 at step 0, (0.9 + 0.45) + 0.9 at step 2 ... all the same float here
    assert maxp[0, 1] == (np.float32(0.9) + np.float32(0.9) + np.float32(0.9)) / np.float32(3)


def test_identical_rows_fuse_to_themselves():
    rng = np.random.default_rng(5)
    p = rng.random((1, 9, 97), dtype=np.float32)
    p /= p.sum(-1, keepdims=True)
    one = ctc_fuse_ref.fuse(p, [0, 1])
    two = ctc_fuse_ref.fuse(np.concatenate([p, p]), [0, 2])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1].view(np.uint32), two[1].view(np.uint32))
    assert np.array_equal(one[0][0], p[0].argmax(-1)) and np.array_equal(one[1][0], p[0].max(-1))
    short = ctc_fuse_ref.fuse(np.concatenate([p, p]), [0, 2], tlen=[4])
    assert np.array_equal(short[0][0, :4], one[0][0, :4]) and not short[0][0, 4:].any() and not short[1][0, 4:].any()
    assert ctc_fuse_ref.ctc_greedy([2, 2, 0, 2, 5, 0], np.float32([.5, .7, .9, .25, 1, 1])) == ([2, 2, 5], float(np.float32(1.75) / np.float32(3)))
    assert ctc_fuse_ref.ctc_greedy([0, 0], np.float32([1, 1])) == ([], 0.0)


# ---- which frames ---------------------------------------------------------------------------------------------------------------
def test_sample_positions():
    """n = 1..12 frames after the trim, samples 1..6: both ends and an even spread in between, in integers; K == 1 is rep."""
    for n in range(1, 13):
        for samples in range(1, 7):
            start, end = 20, 20 + n - 1
            rep = (start + end) // 2
            nos, pos = frame_select.fuse_samples(start, end, rep, FPS, samples, 0.0)
            k = min(samples, n)
            assert len(nos) == k and all(b > a for a, b in zip(nos, nos[1:])), (n, samples, nos)
            if k == 1:
                assert nos == [rep] and pos == 0
                continue
            assert nos == [start + (i * (n - 1)) // (k - 1) for i in range(k)] and nos[0] == start and nos[-1] == end
            dist = [abs(v - rep) for v in nos]
            assert dist[pos] == min(dist) and pos == dist.index(min(dist))                # the nearest to rep, the earlier one on a tie
    assert frame_select.fuse_samples(20, 31, 25, FPS, 5, 0.0) == ([20, 22, 25, 28, 31], 2)
    assert frame_select.fuse_samples(20, 31, 25, FPS, 2, 0.0) == ([20, 31], 0)            # 5 and 6 away: the nearer
    assert frame_select.fuse_samples(20, 30, 25, FPS, 2, 0.0) == ([20, 30], 0)            # a tie: the earlier
    # the trim of the compositor: round(0.25 * 10) = 2 frames off both ends of 20..31, five samples of the eight left
    assert frame_select.fuse_samples(20, 31, 25, FPS, 5, 0.25) == ([22, 23, 25, 27, 29], 2)
    assert frame_select.fuse_samples(20, 31, 25, FPS, 5, 0.25)[0][0::4] == list(frame_select.trim_range(20, 31, FPS, 0.25))
    assert frame_select.fuse_samples(7, 7, 7, FPS, 5, 0.25) == ([7], 0)


# ---- the fuser with a scripted fuse_fn -------------------------------------------------------------------------------------------
def numbered(n, h=8, w=6):
    """n frames whose every pixel holds the frame's 1-based number."""
    return [np.full((h, w, 3), i + 1, np.uint8) for i in range(n)]


class Recorder:
    """fuse_fn that keeps what it was given and answers each group with the frame numbers of its members and of its detect member."""

    def __init__(self):
        self.calls = []

    def __call__(self, frames, groups):
        frames = np.asarray(frames)
        self.calls.append((frames.shape, [([int(frames[m, 0, 0, 0]) for m in mem], pos) for mem, pos in groups]))
        return [([[int(frames[mem[pos], 0, 0, 0])]], [("+".join(str(int(frames[m, 0, 0, 0])) for m in mem), 1.0)]) for mem, pos in groups]


class CountingFrames:
    def __init__(self, frames):
        self.frames, self.reads = frames, 0

    def __iter__(self):
        for f in self.frames:
            self.reads += 1
            yield f


INTERVALS = [(3, 14, 8), (15, 15, 15), (20, 29, 24), (31, 33, 32), (40, 52, 46)]


def test_fuser_samples_detects_and_batches():
    rec = Recorder()
    src = CountingFrames(numbered(60))
    fuser = frame_select.IntervalFuser(rec, samples=4, trim_seconds=0.0, batch=9)
    out = fuser.run(src, INTERVALS, FPS)
    want = [frame_select.fuse_samples(s, e, r, FPS, 4, 0.0) for s, e, r in INTERVALS]
    assert [w[0] for w in want] == [[3, 6, 10, 14], [15], [20, 23, 26, 29], [31, 32, 33], [40, 44, 48, 52]]
    assert sorted(out) == [r for _s, _e, r in INTERVALS] and out is fuser.results
    for (s, e, rep), (nos, pos) in zip(INTERVALS, want):
        assert out[rep] == ([[nos[pos]]], [("+".join(map(str, nos)), 1.0)])               # every sample reached it, detect = nearest to rep
    # whole intervals per call, at most 9 frames: 4 + 1 + 4 | 3 + 4
    assert [[m for m, _p in c[1]] for c in rec.calls] == [[w[0] for w in want[:3]], [w[0] for w in want[3:]]]
    assert [c[0] for c in rec.calls] == [(9, 8, 6, 3), (7, 8, 6, 3)]
    assert [[p for _m, p in c[1]] for c in rec.calls] == [[w[1] for w in want[:3]], [w[1] for w in want[3:]]]
    assert src.reads == 52 < 60                                                           # not beyond the last sample

    rec1 = Recorder()
    frame_select.IntervalFuser(rec1, samples=4, trim_seconds=0.0, batch=4).run(numbered(60), INTERVALS, FPS)
    assert [len(c[1]) for c in rec1.calls] == [1, 1, 1, 1, 1] and max(c[0][0] for c in rec1.calls) == 4       # never split, never above batch
    one = Recorder()
    got = frame_select.IntervalFuser(one, samples=1).run(numbered(60), INTERVALS, FPS)
    assert [c[1] for c in one.calls] == [[([r], 0) for _s, _e, r in INTERVALS]] and sorted(got) == sorted(out)  # K == 1: the middle frame
    with pytest.raises(ValueError):
        frame_select.IntervalFuser(rec, samples=5, batch=4)
    with pytest.raises(ValueError):
        frame_select.IntervalFuser(rec, samples=0)


def test_fuser_only_reading_stops_and_short_clips():
    rec = Recorder()
    src = CountingFrames(numbered(60))
    fuser = frame_select.IntervalFuser(rec, samples=3, trim_seconds=0.1)
    out = fuser.run(src, INTERVALS, FPS, only=range(1, 3))
    assert sorted(out) == [15, 24]
    assert rec.calls == [((4, 8, 6, 3), [([15], 0), ([21, 24, 28], 1)])]                  # 20..29 trimmed by round(0.1 * 10) = 1 frame per end
    assert src.reads == 28
    nothing = CountingFrames(numbered(60))
    assert fuser.run(nothing, INTERVALS, FPS, only=range(0, 0)) == {} and fuser.run(nothing, [], FPS) == {} and nothing.reads == 0
    assert len(rec.calls) == 1
    with pytest.raises(ValueError):
        fuser.run(numbered(27), INTERVALS, FPS, only=range(1, 3))                        # the clip ends before the sample at frame 28
    with pytest.raises(ValueError):
        fuser.run(numbered(60), [(3, 14, 8), (10, 20, 15)], FPS)                         # overlapping intervals


def test_fuser_applies_the_default_area():
    frames = numbered(20, h=9)
    for k, f in enumerate(frames):
        f[:4] = 200                                                                       # the upper half says nothing about the frame
    for area, rows, first in ((extractor.LOWER_PART, 5, None), (extractor.UPPER_PART, 4, 200), (None, 9, 200)):
        rec = Recorder()
        out = frame_select.IntervalFuser(rec, samples=3, trim_seconds=0).run(list(frames), [(2, 10, 6)], FPS, default_area=area)
        assert rec.calls[0][0] == (3, rows, 6, 3)
        if first is None:
            assert out[6] == ([[6]], [("2+6+10", 1.0)])                                  # every sample was cropped: the stamps are visible
        else:
            assert out[6] == ([[200]], [("200+200+200", 1.0)])


# ---- the extractor ------------------------------------------------------------------------------------------------------------------
class ScriptedOcr:
    """Recognises the frame number stamped into pixel (0, 0) as the truth text of that frame; predict_fused answers for the detect
    member and keeps the stamps of every group."""

    def __init__(self, truth):
        self.truth, self.single, self.groups = truth, [], []

    def _of(self, img):
        no = int(img[0, 0, 0]) | (int(img[0, 0, 1]) << 8)
        for s, e, text in self.truth:
            if s <= no <= e:
                return no, ([[[60, 300], [580, 300], [580, 340], [60, 340]]], [(text, 0.95)])
        return no, ([], [])

    def predict(self, img):
        no, res = self._of(np.asarray(img))
        self.single.append(no)
        return res

    def predict_batch(self, frames):
        return [self.predict(f) for f in frames]

    def predict_fused(self, frames, groups):
        out = []
        for mem, pos in groups:
            self.groups.append(([self._of(np.asarray(frames[m]))[0] for m in mem], pos))
            out.append(self._of(np.asarray(frames[mem[pos]]))[1])
        return out


def stamped(frames):
    frames = frames.copy()
    for i in range(len(frames)):
        frames[i, 0, 0, 0], frames[i, 0, 0, 1] = (i + 1) & 255, (i + 1) >> 8
    return frames


@pytest.fixture(scope="module")
def clip():
    frames, truth = synth.make_clip([item[:2] for item in area_clip.SCHEDULE], H, W, seed=3)      # hard cuts only: every interval exact
    frames = stamped(frames)
    frames.setflags(write=False)
    return frames, truth


def extract(clip, **kw):
    frames, truth = clip
    ocr = ScriptedOcr(truth)
    ex = extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), ocr, sub_area=AREA, mode="fast", frame_selector="change",
                                     change_counter=NumpyCounter(), drop_score=0.0, batch=8, **kw)
    return ex, ocr


def test_extractor_fused(clip, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    _frames, truth = clip
    plain, plain_ocr = extract(clip)
    plain_text = plain.run()
    assert plain.interval_results is None and plain_ocr.groups == [] and len(plain_ocr.single) == len(truth)
    single, single_ocr = extract(clip, interval_text="single", fuse_params={"samples": 3})
    assert single.run() == plain_text and single_ocr.groups == [] and single.interval_results is None

    ex, ocr = extract(clip, interval_text="fused", fuse_params={"samples": 3, "trim_seconds": 0.2})
    text = ex.run()
    assert ocr.single == []                                                               # predict / predict_batch never ran
    assert ex.intervals == plain.intervals == [(s, e, (s + e) // 2) for s, e, _t in truth]
    want = [frame_select.fuse_samples(s, e, r, FPS, 3, 0.2) for s, e, r in ex.intervals]
    assert ocr.groups == want and all(len(nos) == 3 for nos, _p in want)
    assert sorted(ex.interval_results) == [r for _s, _e, r in ex.intervals]
    for (s, e, rep), (_s, _e, t) in zip(ex.intervals, truth):
        assert ex.interval_results[rep][1] == [(t, 0.95)]
    assert text == plain_text and ex.raw_lines == plain.raw_lines and text.count(" --> ") == len(truth)

    tasks = ex.fuse_intervals(ex.select_tasks())                                           # every task carries its interval's result
    assert [t[1] for t in tasks] == [r for _s, _e, r in ex.intervals]
    assert all((t[2], t[3]) == tuple(ex.interval_results[t[1]]) and t[2] is not None for t in tasks)
    assert all(len(t) == 6 and t[0] == len(_frames) and t[4] is None and t[5] is None for t in tasks)


def test_extractor_fused_uses_fuse_fn_and_shards(clip):
    _frames, truth = clip
    seen = []

    def fuse_fn(frames, groups):
        seen.append(len(groups))
        return [([], []) for _ in groups]

    ex, ocr = extract(clip, interval_text="fused", fuse_params={"fuse_fn": fuse_fn, "samples": 2})
    assert ex.run().strip() == "" and ocr.groups == [] and ocr.single == [] and sum(seen) == len(truth)
    covered = []
    for rank in range(2):
        ex, ocr = extract(clip, interval_text="fused", shard=(rank, 2), fuse_params={"samples": 2, "trim_seconds": 0})
        tasks = ex.select_tasks()
        lo, hi = parallel.shard_range(len(tasks), rank, 2)
        fused = ex.fuse_intervals(tasks)
        assert sorted(ex.interval_results) == [t[1] for t in tasks[lo:hi]] and len(ocr.groups) == hi - lo > 0
        assert [t[2] is not None for t in fused] == [lo <= k < hi for k in range(len(tasks))]
        covered += sorted(ex.interval_results)
    assert covered == [r for _s, _e, r in ex.intervals]                                   # disjoint slices that cover the intervals


def test_extractor_refuses_bad_interval_text():
    src = extractor.ArraySource([np.zeros((8, 8, 3), np.uint8)], 25.0)
    for kw in (dict(frame_selector="change", interval_text="mean"), dict(frame_selector="change", interval_text=None),
               dict(frame_selector="fps", interval_text="fused"), dict(interval_text="fused"),
               dict(frame_selector="change", interval_text="fused", interval_image="min"),
               dict(frame_selector="hold", interval_text="fused", interval_image="mean")):
        with pytest.raises(ValueError) as err:
            extractor.SubtitleExtractor(src, ScriptedOcr([]), sub_area=AREA, **kw)
        if kw.get("interval_text") == "fused":
            assert "frame_selector" in str(err.value) and "interval_image" in str(err.value)
    for sel in ("change", "hold"):
        extractor.SubtitleExtractor(src, ScriptedOcr([]), sub_area=AREA, frame_selector=sel, interval_text="fused")
    extractor.SubtitleExtractor(src, ScriptedOcr([]), sub_area=AREA, interval_text="single", interval_image="middle")
