"""numpy restatement of the interval composite (include/vse_hip.h vse_interval_accumulate / vse_interval_composite): the device kernels
must agree with it byte for byte, and the CPU tests drive the host compositor with it."""
import numpy as np

MODES = ("min", "max", "mean")


def accumulate(state, frames, area):
    """uint8 BGR [n,H,W,3] folded into state = (mn uint8, mx uint8, sm uint32), each [y1-y0, x1-x0, 3]; state None starts from these
    frames alone (what `reset` does on the device)."""
    y0, y1, x0, x1 = area
    a = np.asarray(frames)[:, y0:y1, x0:x1]
    assert a.dtype == np.uint8 and a.shape[0] >= 1 and a.shape[1] == y1 - y0 and a.shape[2] == x1 - x0
    mn, mx, sm = a.min(0), a.max(0), a.sum(0, dtype=np.uint64).astype(np.uint32)
    if state is not None:
        mn, mx, sm = np.minimum(state[0], mn), np.maximum(state[1], mx), state[2] + sm          # (uint32 addition wraps, as on the device)
    return mn, mx, sm


def composite(state, frames, mode):
    """state of `frames` accumulated frames -> uint8 [ah, aw, 3]: min, max, or the mean with halves rounded up."""
    mn, mx, sm = state
    if mode == "min":
        return mn.copy()
    if mode == "max":
        return mx.copy()
    assert mode == "mean" and 1 <= frames <= 4194304
    return ((2 * sm.astype(np.uint64) + frames) // (2 * frames)).astype(np.uint8)


def trim_range(start, end, fps, trim_seconds):
    """The frames of the interval start..end (1-based, inclusive) that are composited: (first, last)."""
    tr = min(int(round(trim_seconds * fps)), (end - start) // 2)
    return start + tr, end - tr


class NumpyCompositor:
    """accumulate_fn of frame_select.IntervalCompositor on the host: keeps the state and the frame count of the open interval."""

    def __init__(self):
        self.state = None
        self.count = 0
        self.calls = 0
        self.frames_seen = 0

    def __call__(self, frames, area, reset, mode=None):
        self.calls += 1
        self.frames_seen += len(frames)
        self.state = accumulate(None if reset else self.state, np.asarray(frames), area)
        self.count = len(frames) if reset else self.count + len(frames)
        return composite(self.state, self.count, mode) if mode is not None else None
