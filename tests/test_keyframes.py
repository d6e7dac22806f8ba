"""vse_amd.keyframes on the CPU: the numpy restatement of the scene-cut counts (tests/scene_cut_ref.py) behaves on generator clips as
the detector needs (pans are followed, cuts are not, a subtitle is no cut), the detector's rule, find_keyframes over .npy and AVI
sources with the numpy counter, and Sushi's keyframes file written and read."""
import json
import os

import numpy as np
import pytest

from scene_cut_ref import NumpySceneCounter, counts as ref_counts, planes
from vse_amd import ingest, keyframes, synth, timeline_sync as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = json.load(open(os.path.join(ROOT, "tests", "golden", "timeline_sync_keyframes.json")))

# frame: 0 first, 1..5 panned (at most 24 source pixels per frame and axis-parallel or small: a 24-pixel pan along both axes at once
# uncovers a row AND a column of new blocks, 61 of 880 = 6.9 %, which no search can predict), 6 held, 7 a hard cut, 8 static, 9 a
# subtitle line appears, 10 it stays
PANS = [(0, 24), (24, 0), (10, -7), (0, -24), (5, 5), (0, 0)]


@pytest.fixture(scope="module")
def clip_1080p():
    frames, cuts = synth.make_scenes([dict(frames=7, pan=PANS, hold=[6]), dict(frames=4, text=("the quick brown fox jumps", 2, 3))],
                                     1080, 1920, seed=1)
    c, _, zero = ref_counts(frames, 3, 8, 1024, with_zero=True)
    c.setflags(write=False)
    return cuts, c, zero


def test_reference_on_a_1080p_clip(clip_1080p):
    cuts, c, zero = clip_1080p
    blocks = (1080 // 3 // 16) * (1920 // 3 // 16)
    assert cuts == [0, 7] and blocks == 880
    print("changed blocks per frame:", c[:, 0].tolist(), "sum inter:", c[:, 1].tolist(), "zero-vector sum:", zero.tolist())
    assert tuple(c[0][:2]) == (blocks, 0)
    for t in range(1, 6):                                  # pans: at most 5 % of the blocks changed
        assert c[t, 0] * 100 <= 5 * blocks, (t, c[t])
    assert any(c[t, 1] < zero[t] for t in range(1, 6))     # the search really picks nonzero vectors
    assert all(c[t, 1] <= zero[t] for t in range(1, len(c)))
    assert c[6, 0] == 0 and c[6, 1] == 0                   # a held frame
    assert c[7, 0] * 100 >= 90 * blocks                    # the frame after a hard cut
    assert c[9, 0] * 100 <= 5 * blocks and c[9, 0] > 0     # a subtitle line appears over a held scene (static camera, fresh noise)
    assert c[8, 0] == 0 and c[10, 0] == 0


def test_planes_box_filter_and_remainders():
    rng = np.random.default_rng(0)
    f = rng.integers(0, 256, size=(2, 37, 50, 3), dtype=np.uint8)
    a = planes(f, 3)
    assert a.shape == (2, 12, 16)
    i = f.astype(int)
    y = (29 * i[..., 0] + 150 * i[..., 1] + 77 * i[..., 2] + 128) >> 8
    assert a[1, 11, 15] == (y[1, 33:36, 45:48].sum() + 4) // 9
    g = f.copy()
    g[:, 36:] ^= 255                                        # rows / columns beyond ah * s, aw * s are not read
    g[:, :, 48:] ^= 255
    assert np.array_equal(planes(g, 3), a)
    assert np.array_equal(planes(f, 1)[0], y[0])


def test_clipped_vectors_and_remainder_pixels():
    """A block at the plane's edge only counts vectors whose displaced block is inside; plane pixels beyond the last block are
    reference pixels."""
    rng = np.random.default_rng(1)
    world = rng.integers(0, 256, size=(40, 60, 3), dtype=np.uint8)
    a = world[4:4 + 20, 8:8 + 35]                           # 20 x 35 plane: one block row, two block columns, remainders 4 and 3
    b = world[4:4 + 20, 5:5 + 35]                           # the camera moved 3 to the left: content moved 3 to the right (dx = -3)
    c, _ = ref_counts(np.stack([a, b]), 1, 3, 0)
    # block 1 (x 16..31) finds its content at dx = -3 exactly; block 0 would need columns -3..12: clipped, so it cannot match
    assert c[1, 0] == 1 and c[1, 1] > 0
    c2, _ = ref_counts(np.stack([b, a]), 1, 3, 0)           # the other way round both blocks match at dx = +3 (block 1 uses columns 19..34)
    assert tuple(c2[1][:2]) == (0, 0)
    c3, _ = ref_counts(np.stack([b, a]), 1, 2, 0)           # out of range
    assert c3[1, 0] == 2


class FakeCounter:
    def __init__(self, changed, blocks):
        self.changed, self.blocks, self.at, self.resets = changed, blocks, 0, []

    def __call__(self, frames, scale, search, bias, reset):
        self.resets.append(reset)
        n = len(frames)
        out = np.zeros((n, 3), np.int32)
        out[:, 0] = self.changed[self.at:self.at + n]
        self.at += n
        return out


def test_detector_rule():
    # 64 x 64 frames, scale 1: 16 blocks
    changed = [16, 0, 7, 8, 9, 16, 0, 16, 16, 3]
    det = keyframes.SceneCutDetector(FakeCounter(changed, 16), 64, 64, scale=1)
    assert det.blocks == 16 and det.scale == 1
    assert det.feed(np.zeros((4, 64, 64, 3), np.uint8)) == [0, 3] and det.feed(np.zeros((6, 64, 64, 3), np.uint8)) == [4, 5, 7, 8]
    assert det.counter.resets == [True, False] and det.frames_seen == 10
    det = keyframes.SceneCutDetector(FakeCounter(changed, 16), 64, 64, scale=1, cut_percent=100, min_gap=1)
    assert det.feed(np.zeros((10, 64, 64, 3), np.uint8)) == [0, 5, 7, 8]
    det = keyframes.SceneCutDetector(FakeCounter(changed, 16), 64, 64, scale=1, cut_percent=50, min_gap=3)
    assert det.feed(np.zeros((10, 64, 64, 3), np.uint8)) == [0, 3, 7]
    det = keyframes.SceneCutDetector(FakeCounter([0, 0, 16], 16), 64, 64, scale=1)
    assert det.feed(np.zeros((3, 64, 64, 3), np.uint8)) == [0, 2]          # frame 0 always is a keyframe
    assert [keyframes.default_scale(w) for w in (320, 640, 1280, 1920, 3840, 7680)] == [1, 1, 2, 3, 6, 8]
    assert keyframes.SceneCutDetector(FakeCounter([], 1), 1080, 1920).blocks == 880
    with pytest.raises(ValueError):
        keyframes.SceneCutDetector(FakeCounter([], 1), 15, 64, scale=1)
    with pytest.raises(ValueError):
        keyframes.SceneCutDetector(FakeCounter([], 1), 64, 64, scale=1, search=9)


def cut_clip():
    return synth.make_scenes([dict(frames=9, pan=(0, 3)), dict(frames=8, pan=(2, -2), hold=[3, 4]),
                              dict(frames=10, text=("seven wizards quietly box", 3, 8)), dict(frames=6, pan=(-4, 0))], 180, 320, seed=9)


@pytest.mark.parametrize("kind", ["npy", "avi"])
def test_find_keyframes_finds_the_generators_cuts(tmp_path, kind):
    frames, cuts = cut_clip()
    assert cuts == [0, 9, 17, 27] and len(frames) == 33
    if kind == "npy":
        np.save(tmp_path / "clip.npy", frames)
        src = ingest.open_source(str(tmp_path / "clip.npy"), fps=24.0)
    else:
        ingest.write_avi_bgr24(str(tmp_path / "clip.avi"), frames, 24.0)
        src = ingest.open_source(str(tmp_path / "clip.avi"))
    counter = NumpySceneCounter()
    assert keyframes.find_keyframes(src, ctx=counter, batch=7) == cuts
    assert counter.calls == 5
    if kind == "avi":
        return
    # (the camera keeps moving through the two held frames: frame 14 is displaced by (6, -6) against frame 13)
    kf, count = keyframes.scan(src, NumpySceneCounter(), 64, search=6, cut_percent=60)
    assert kf == cuts and count == 33
    assert keyframes.find_keyframes(src, ctx=NumpySceneCounter(), search=4) == [0, 9, 14, 17, 27]          # the known limit: a jump beyond the range reads as a cut


def test_make_scenes():
    frames, cuts = synth.make_scenes([dict(frames=4, pan=[(0, 2), (3, 0)], hold=[3]), dict(frames=2)], 48, 64, seed=4)
    again, _ = synth.make_scenes([dict(frames=4, pan=[(0, 2), (3, 0)], hold=[3]), dict(frames=2)], 48, 64, seed=4)
    assert frames.shape == (6, 48, 64, 3) and frames.dtype == np.uint8 and cuts == [0, 4] and np.array_equal(frames, again)
    assert np.array_equal(frames[3], frames[2])                                   # held
    d = np.abs(frames[1][:, :-2].astype(int) - frames[0][:, 2:].astype(int))      # the camera moved 2 to the right: fresh noise of +-3 twice
    assert d.max() <= 6 and d.max() > 0
    d = np.abs(frames[2][:-3, :-2].astype(int) - frames[0][3:, 2:].astype(int))   # then 3 down (the short pan list repeats its last step)
    assert d.max() <= 6
    assert abs(frames[4].mean() - frames[0].mean()) > 1 or np.abs(frames[4].astype(int) - frames[3]).mean() > 10


# ---- Sushi's keyframes file -------------------------------------------------------------------------------------------------------

def test_write_parse_round_trip(tmp_path):
    p = str(tmp_path / "kf.txt")
    for kf, count in (([0, 5, 6, 99], 100), ([0], 1), ([0, 1, 2], 3)):
        assert keyframes.parse_keyframes(keyframes.write_keyframes(p, kf, count)) == kf
    lines = open(keyframes.write_keyframes(p, [0, 2], 4)).read().splitlines()
    assert lines[0].startswith("# XviD 2pass stat file") and len(lines) == 3 + 4 and [x[0] for x in lines[3:]] == ["i", "p", "i", "p"]
    assert keyframes.parse_keyframes(keyframes.write_keyframes(p, [3], 6)) == [0, 3]          # frame 0 is inserted if absent
    with pytest.raises(ValueError):
        keyframes.write_keyframes(p, [4], 4)


@pytest.mark.parametrize("case", DOC["keyframes_files"], ids=lambda c: str(c["keyframes"]))
def test_parse_gives_what_the_reference_parser_gave(tmp_path, case):
    p = str(tmp_path / "kf.txt")
    assert open(keyframes.write_keyframes(p, case["keyframes"], case["frame_count"])).read() == case["text"]
    assert keyframes.parse_keyframes(p) == case["parsed"]


def test_parse_refuses_other_files(tmp_path):
    p = tmp_path / "other.txt"
    p.write_text("# keyframe format v1\nfps 0\n0\n10\n")
    with pytest.raises(ts.TimelineSyncError, match="Unsupported keyframes type"):
        keyframes.parse_keyframes(str(p))
    with pytest.raises(ts.TimelineSyncError, match="not found"):
        keyframes.parse_keyframes(str(tmp_path / "none.txt"))
    # a real XviD first-pass log: the numbers behind the frame type are ignored
    p.write_text("# XviD 2pass stat file (core version 1.3.7)\n# Please do not modify this file\n\ni 2 1234 56 7 8 9\np 3 10 2 0 0 0\nb 4 1 1 0 0 0\n"
                 "i 2 999 56 7 8 9\n")
    assert keyframes.parse_keyframes(str(p)) == [0, 3]


def test_cli_reports_an_unreadable_video(tmp_path):
    bad = tmp_path / "x.avi"
    bad.write_bytes(b"not an avi file at all")
    assert keyframes.main([str(bad), "-o", str(tmp_path / "k.txt")]) == 2
