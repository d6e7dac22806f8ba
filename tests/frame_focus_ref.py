"""numpy restatement of the per-frame focus rows (include/vse_hip.h vse_frame_focus): the device kernel must agree with it bit for bit,
and the CPU tests drive the selectors and the extractor with it.  The mask is frame_change_ref's."""
import numpy as np

from frame_change_ref import edge_mask


def gradient(frames, area):
    """uint8 BGR [n,H,W,3], area (y0, y1, x0, x1) -> int32 [n, y1-y0-2, x1-x0-2]: g of the area's interior pixels, 0..255."""
    y0, y1, x0, x1 = area
    a = np.asarray(frames)[:, y0:y1, x0:x1].astype(np.int32)
    y = (29 * a[..., 0] + 150 * a[..., 1] + 77 * a[..., 2] + 128) >> 8
    gx = np.abs(y[:, 1:-1, 2:] - y[:, 1:-1, :-2])
    gy = np.abs(y[:, 2:, 1:-1] - y[:, :-2, 1:-1])
    return np.maximum(gx, gy)


def focus(frames, area, edge_thresh, prev=None):
    """-> (int64 [n,2] kept / focus, the last frame's mask).  prev: the mask of the frame before the first (None = empty)."""
    e = edge_mask(frames, area, edge_thresh)
    if not len(e):
        return np.zeros((0, 2), np.int64), prev
    p = np.concatenate([np.zeros_like(e[:1]) if prev is None else prev[None], e[:-1]])
    k = e & p
    g = gradient(frames, area).astype(np.int64)
    return np.stack([k.sum((1, 2)), (g * k).sum((1, 2))], 1).astype(np.int64), e[-1]


class NumpyFocus:
    """focus_fn of the frame selectors on the host: carries the last mask from one batch to the next."""

    def __init__(self):
        self.prev = None
        self.calls = []               # (frames, reset) per call

    def __call__(self, frames, area, edge_thresh, reset):
        self.calls.append((len(frames), bool(reset)))
        out, self.prev = focus(frames, area, edge_thresh, None if reset else self.prev)
        return out
