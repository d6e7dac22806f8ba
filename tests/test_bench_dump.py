"""bench.py --dump-outputs: the records of the last timed step -> DIR/<name>.npy, float32 / float64 only."""
import numpy as np

import bench


def _box(v):
    return np.full((4, 2), v, np.float32)


def test_dump_outputs_writes_the_last_step_in_frame_order(tmp_path):
    # (frame number, boxes, [(text, score)]) as run_steps returns them; frames 2 and 3 are the last step
    out = [(0, [_box(1)], [("ab", 0.9)]), (3, [_box(4)], [("héllo", 0.75)]), (1, [], []),
           (2, [_box(2), _box(3)], [("x", 0.5), ("", 0.25)])]
    bench.dump_outputs(str(tmp_path), out, 2)
    got = {p.stem: np.load(p) for p in tmp_path.iterdir()}
    assert sorted(got) == ["box_counts", "boxes", "frame_numbers", "scores", "text_codepoints"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["frame_numbers"].tolist() == [2, 3] and got["box_counts"].tolist() == [2, 1]
    assert got["boxes"].shape == (3, 4, 2) and got["boxes"][:, 0, 0].tolist() == [2, 3, 4]
    assert got["scores"].tolist() == [0.5, 0.25, 0.75]
    codes = got["text_codepoints"]
    assert codes.shape == (3, 5)
    assert "".join(chr(int(c)) for c in codes[2]) == "héllo" and codes[0].tolist() == [ord("x")] + [-1] * 4
    assert (codes[1] == -1).all()


def test_dump_outputs_without_boxes(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), [(0, [], []), (1, [], [])], 0)
    assert np.load(tmp_path / "d" / "boxes.npy").shape == (0, 4, 2)
    assert np.load(tmp_path / "d" / "text_codepoints.npy").shape == (0, 1)
    assert np.load(tmp_path / "d" / "box_counts.npy").tolist() == [0, 0]
