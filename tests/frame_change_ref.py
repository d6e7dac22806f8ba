"""numpy restatement of the subtitle-change counts (include/vse_hip.h vse_frame_change): the device kernel must agree with it
bit for bit, and the CPU tests drive the host selector with it."""
import numpy as np


def edge_mask(frames, area, edge_thresh):
    """uint8 BGR [n,H,W,3], area (y0, y1, x0, x1) -> bool [n, y1-y0-2, x1-x0-2]: the edge pixels of the area's interior."""
    y0, y1, x0, x1 = area
    a = np.asarray(frames)[:, y0:y1, x0:x1].astype(np.int32)
    y = (29 * a[..., 0] + 150 * a[..., 1] + 77 * a[..., 2] + 128) >> 8
    gx = np.abs(y[:, 1:-1, 2:] - y[:, 1:-1, :-2])
    gy = np.abs(y[:, 2:, 1:-1] - y[:, :-2, 1:-1])
    return np.maximum(gx, gy) >= edge_thresh


def counts(frames, area, edge_thresh, prev=None):
    """-> (int32 [n,3] edges / appeared / vanished, the last frame's mask).  prev: the mask of the frame before the first
    (None = empty)."""
    e = edge_mask(frames, area, edge_thresh)
    p = np.concatenate([np.zeros_like(e[:1]) if prev is None else prev[None], e[:-1]])
    out = np.stack([e.sum((1, 2)), (e & ~p).sum((1, 2)), (p & ~e).sum((1, 2))], 1).astype(np.int32)
    return out, e[-1]


class NumpyCounter:
    """count_fn of frame_select.ChangeFrameSelector on the host: carries the last mask from one batch to the next."""

    def __init__(self):
        self.prev = None
        self.calls = 0

    def __call__(self, frames, area, edge_thresh, reset):
        self.calls += 1
        out, self.prev = counts(frames, area, edge_thresh, None if reset else self.prev)
        return out
