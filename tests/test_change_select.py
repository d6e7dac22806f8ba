"""Subtitle-change frame selection on the host: the interval state machine (frame_select.change_intervals), the numpy counts
of tests/frame_change_ref.py on synth.make_clip clips, the interval SRT writer (srt.generate_subtitle_file_intervals) and
SubtitleExtractor(frame_selector="change") with a scripted recogniser.  CPU only."""
import numpy as np
import pytest

from frame_change_ref import NumpyCounter, counts as ref_counts
from vse_amd import extractor, frame_select, srt, synth

H, W = 360, 640
AREA = extractor.SubtitleArea(ymin=int(0.78 * H), ymax=int(0.99 * H), xmin=int(0.05 * W), xmax=int(0.95 * W))
SCHEDULE = [(None, 3), ("the quick brown fox", 7), ("the quick brown box", 6), (None, 4), ("seven wizards", 5),
            ("near frozen lakes", 6), (None, 2), ("the quick brown fox", 5), (None, 3), ("bright morning light", 9, 4), (None, 2)]


def intervals(rows, min_edges=10, change_ratio=0.5, min_frames=2):
    return frame_select.change_intervals(np.asarray(rows, np.int32).reshape(-1, 3), min_edges, change_ratio, min_frames)


# ---- state machine ------------------------------------------------------------------------------------------------------
def test_presence_threshold():
    rows = [(9, 9, 0), (10, 1, 0), (10, 0, 0), (10, 0, 0), (9, 0, 1), (30, 30, 0), (30, 0, 0)]
    assert intervals(rows) == [(2, 4, 3), (6, 7, 6)]


def test_cut_ratio_exactly_at_threshold():
    # (appeared + vanished) / (edges[t-1] + appeared)
    assert intervals([(100, 100, 0), (100, 0, 0), (100, 0, 50), (100, 0, 0)]) == [(1, 2, 1), (3, 4, 3)]     # 50 / 100 = 0.5: cut
    assert intervals([(100, 100, 0), (100, 0, 0), (100, 0, 49), (100, 0, 0)]) == [(1, 4, 2)]                # 0.49: none
    rows = [(100, 100, 0), (100, 0, 0), (100, 25, 25), (100, 0, 0)]                                            # 50 / 125 = 0.4
    assert intervals(rows, change_ratio=0.4) == [(1, 2, 1), (3, 4, 3)]
    assert intervals(rows, change_ratio=0.40001) == [(1, 4, 2)]


def test_min_frames_and_open_interval():
    rows = [(50, 50, 0), (0, 0, 50), (50, 50, 0), (50, 0, 0), (0, 0, 50), (50, 50, 0), (50, 0, 0), (50, 0, 0)]
    assert intervals(rows) == [(3, 4, 3), (6, 8, 7)]                       # the one-frame run is dropped, the last is open
    assert intervals(rows, min_frames=1) == [(1, 1, 1), (3, 4, 3), (6, 8, 7)]
    assert intervals(rows, min_frames=3) == [(6, 8, 7)]


def test_empty_and_one_frame_clips():
    assert intervals([]) == []
    assert intervals([(50, 50, 0)]) == []
    assert intervals([(50, 50, 0)], min_frames=1) == [(1, 1, 1)]
    assert intervals([(5, 5, 0)], min_frames=1) == []


def test_selector_on_no_frames():
    sel = frame_select.ChangeFrameSelector(NumpyCounter())
    assert sel.run([], AREA) == []


# ---- numpy counts on a scripted clip ------------------------------------------------------------------------------------
def clip():
    return synth.make_clip(SCHEDULE, H, W, seed=5)


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_counts_batches_chain(batch):
    frames, _ = clip()
    area = (AREA.ymin, AREA.ymax, AREA.xmin, AREA.xmax)
    whole, _ = ref_counts(frames, area, 128)
    counter = NumpyCounter()
    got = np.concatenate([counter(frames[i:i + batch], area, 128, i == 0) for i in range(0, len(frames), batch)])
    assert np.array_equal(got, whole)


def test_intervals_match_truth():
    frames, truth = clip()
    counter = NumpyCounter()
    sel = frame_select.ChangeFrameSelector(counter, batch=8)
    got = sel.run(list(frames), AREA)
    assert counter.calls == (len(frames) + 7) // 8                # every frame looked at once
    fade_start, fade_end = truth[-1][0], truth[-1][0] + 3
    hard = [(s, e) for s, e, _t in truth[:-1]]
    assert [(s, e) for s, e, _r in got[:-1]] == hard              # every hard cut exact to the frame
    s, e, r = got[-1]
    assert fade_start <= s <= fade_end and e == truth[-1][1]       # the fade-in: one interval, inside the fade, exact end
    assert all(r == (s + e) // 2 for s, e, r in got)


# ---- interval SRT writer ------------------------------------------------------------------------------------------------
def line(no, text, box="(10, 200, 300, 340)"):
    return f"{no:08d}\t{box}\t{text}\n"


IV = [(3, 9, 6), (10, 15, 12), (16, 20, 18), (25, 30, 27), (33, 40, 36)]


def test_intervals_srt_merges_neighbours():
    lines = [line(6, "hello world"), line(12, "hello world!"), line(18, "other text"), line(36, "last")]
    text, norm = srt.generate_subtitle_file_intervals(lines, IV, 10.0)
    assert text == ("1\n00:00:00,003 --> 00:00:01,005\nhello world!\n\n"
                    "2\n00:00:01,006 --> 00:00:02,000\nother text\n\n"
                    "3\n00:00:03,003 --> 00:00:04,000\nlast\n\n")
    assert [ln.split("\t")[0] for ln in norm] == ["00000006", "00000012", "00000018", "00000036"]


def test_intervals_srt_keeps_empty_when_asked():
    lines = [line(6, "hello world"), line(12, "hello world!"), line(18, "other text"), line(36, "last")]
    text, _ = srt.generate_subtitle_file_intervals(lines, IV, 10.0, delete_empty=False)
    assert text == ("1\n00:00:00,003 --> 00:00:01,005\nhello world!\n\n"
                    "2\n00:00:01,006 --> 00:00:02,000\nother text\n\n"
                    "3\n00:00:02,005 --> 00:00:03,000\n\n\n"
                    "4\n00:00:03,003 --> 00:00:04,000\nlast\n\n")


def test_intervals_srt_pos_msec():
    lines = [line(6, "a subtitle"), line(18, "another one")]
    text, _ = srt.generate_subtitle_file_intervals(lines, IV[:3], 25.0, pos_msec=lambda no: 1000.0 * no + 250)
    assert text == ("1\n00:00:03,250 --> 00:00:09,250\na subtitle\n\n"
                    "2\n00:00:16,250 --> 00:00:20,250\nanother one\n\n")


# ---- the extractor ------------------------------------------------------------------------------------------------------
class ScriptedOcr:
    """Recognises the frame number stamped into pixel (0, 0) (outside the area) as the truth text of that frame."""

    def __init__(self, truth, batched):
        self.truth, self.seen = truth, []
        if batched:
            self.predict_batch = lambda frames: [self.predict(np.asarray(f)) for f in frames]

    def predict(self, img):
        no = int(img[0, 0, 0]) | (int(img[0, 0, 1]) << 8)
        self.seen.append(no)
        for s, e, text in self.truth:
            if s <= no <= e:
                return [[[60, 300], [580, 300], [580, 340], [60, 340]]], [(text, 0.95)]
        return [], []


def stamped(frames):
    frames = frames.copy()
    for i in range(len(frames)):
        frames[i, 0, 0, 0], frames[i, 0, 0, 1] = (i + 1) & 255, (i + 1) >> 8
    return frames


@pytest.mark.parametrize("batched", [False, True])
def test_extractor_change_selector(batched, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = synth.make_clip([item[:2] for item in SCHEDULE], H, W, seed=5)        # hard cuts only: every interval exact
    src = extractor.ArraySource(list(stamped(frames)), 25.0)
    ocr = ScriptedOcr(truth, batched)
    ex = extractor.SubtitleExtractor(src, ocr, sub_area=AREA, mode="fast", frame_selector="change", change_counter=NumpyCounter(),
                                     drop_score=0.0, batch=8)
    text = ex.run()
    want = [(s, e, (s + e) // 2) for s, e, _t in truth]
    assert ex.intervals == want
    assert sorted(ocr.seen) == [r for _s, _e, r in want]                 # exactly one OCR call per interval, on its middle frame
    lines = sum((extractor.frame_lines(r, *ScriptedOcr(truth, False).predict(src.read(r)), AREA, "ch", 0.0, 0.0) for _s, _e, r in want), [])
    assert len(lines) == len(truth)
    assert text == srt.generate_subtitle_file_intervals(lines, want, 25.0)[0]
    assert text.count(" --> ") == 5                      # fox -> box merged as similar text; fox after a gap is a block of its own
    assert ex.short_lines == []


def test_fps_selector_unchanged_by_default(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = clip()
    src = extractor.ArraySource(list(stamped(frames)), 25.0)
    ex = extractor.SubtitleExtractor(src, ScriptedOcr(truth, True), sub_area=AREA, mode="fast", change_counter=NumpyCounter())
    ex.run()
    assert ex.intervals is None
    with pytest.raises(ValueError):
        extractor.SubtitleExtractor(src, ScriptedOcr(truth, True), frame_selector="vsf")
