"""numpy restatement of the held-edge counts (include/vse_hip.h vse_frame_hold): the device kernel must agree with it bit for bit,
and the CPU tests drive the host selector with it."""
import numpy as np

from frame_change_ref import edge_mask


def held_masks(e, hold):
    """bool [T,h,w] edge masks of consecutive frames -> bool [T,h,w]: the edge pixels whose maximal run of consecutive edge frames
    (cut off at both ends of the stack) is at least `hold` frames long."""
    e = np.asarray(e, bool)
    before = np.zeros(e.shape, np.int32)        # edge frames in a row up to and including t
    after = np.zeros(e.shape, np.int32)         # ... from t on
    for t in range(len(e)):
        before[t] = np.where(e[t], (before[t - 1] if t else 0) + 1, 0)
    for t in range(len(e) - 1, -1, -1):
        after[t] = np.where(e[t], (after[t + 1] if t + 1 < len(e) else 0) + 1, 0)
    return e & (before + after - 1 >= hold)


def rows_of(held, prev=None):
    """held masks bool [T,h,w] of consecutive frames -> int32 [T,3]: |H_u|, |H_u minus H_{u-1}|, |H_{u-1} minus H_u|;
    prev: the mask before the first (None = empty)."""
    p = np.concatenate([np.zeros_like(held[:1]) if prev is None else prev[None], held[:-1]])
    return np.stack([held.sum((1, 2)), (held & ~p).sum((1, 2)), (p & ~held).sum((1, 2))], 1).astype(np.int32)


def counts(frames, area, edge_thresh, hold):
    """A whole clip, uint8 BGR [T,H,W,3], area (y0, y1, x0, x1) -> int32 [T,3]: the rows of all its frames (what a call with fed = 0
    and flush writes)."""
    return rows_of(held_masks(edge_mask(frames, area, edge_thresh), hold))


def emitted(fed, n, hold, flush):
    """-> (lo, hi): a call with n frames after `fed` earlier ones writes the rows of frames lo + 1 .. hi."""
    return max(0, fed - hold + 1), fed + n if flush else max(0, fed + n - hold + 1)


class NumpyHoldCounter:
    """count_fn of frame_select.HoldFrameSelector on the host, with the device's latency: a call returns the rows of the frames whose
    held mask it completes.  It keeps the edge masks a later frame's run can still reach back to, and the last mask it counted."""

    def __init__(self):
        self.calls = 0
        self.first = 1            # frame number of self.masks[0]
        self.masks = None         # bool [k,h,w]
        self.prev = None          # held mask of the last frame counted

    def __call__(self, frames, area, edge_thresh, hold, fed, flush):
        self.calls += 1
        frames = np.asarray(frames)
        y0, y1, x0, x1 = area
        new = edge_mask(frames, area, edge_thresh) if len(frames) else np.zeros((0, y1 - y0 - 2, x1 - x0 - 2), bool)
        if fed == 0:
            self.first, self.masks, self.prev = 1, new, None
        else:
            assert self.first + len(self.masks) == fed + 1, "frames of a clip arrive in order"
            self.masks = np.concatenate([self.masks, new])
        lo, hi = emitted(fed, len(frames), hold, flush)
        # the window starts at least hold - 1 frames before frame lo + 1 (or at frame 1): a run cut off there is long enough anyway;
        # it ends at frame fed + n, which is at least hold - 1 frames after frame hi unless this is the flush
        held = held_masks(self.masks, hold)[lo + 1 - self.first:hi + 1 - self.first]
        out = rows_of(held, self.prev) if len(held) else np.zeros((0, 3), np.int32)
        if len(held):
            self.prev = held[-1]
        keep = max(self.first, hi + 1 - (hold - 1))
        self.masks, self.first = self.masks[keep - self.first:], keep
        return out
