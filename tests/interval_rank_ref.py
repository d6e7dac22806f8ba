"""numpy restatement of the interval rank (include/vse_hip.h vse_interval_rank): the device kernel must agree with it byte for byte, and
the CPU tests drive frame_select.IntervalQuantile with it."""
import numpy as np


def rank(frames, area, rank):
    """uint8 BGR [n,H,W,3] -> uint8 [y1-y0, x1-x0, 3]: per byte, element `rank` (0-based) of the n frames' values sorted ascending."""
    y0, y1, x0, x1 = area
    a = np.asarray(frames)[:, y0:y1, x0:x1]
    assert a.dtype == np.uint8 and 0 <= rank < a.shape[0] and a.shape[1] == y1 - y0 and a.shape[2] == x1 - x0
    return np.sort(a, axis=0)[rank]


class NumpyRanker:
    """rank_fn of frame_select.IntervalQuantile on the host; keeps what it was called with."""

    def __init__(self):
        self.calls = []               # (frames in the call, rank)
        self.frames_seen = 0

    def __call__(self, frames, area, rank_):
        self.calls.append((len(frames), rank_))
        self.frames_seen += len(frames)
        return rank(np.asarray(frames), area, rank_)
