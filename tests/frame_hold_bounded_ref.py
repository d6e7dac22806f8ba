"""numpy restatement of the bounded held-edge counts (include/vse_hip.h vse_frame_hold_bounded): the device kernel must agree with it
bit for bit, and the CPU tests drive the host selector with it."""
import numpy as np

from frame_change_ref import edge_mask
from frame_hold_ref import rows_of


def bounded_masks(e, hold, max_hold):
    """bool [T,h,w] edge masks of consecutive frames -> bool [T,h,w]: the edge pixels whose maximal run of consecutive edge frames
    (cut off at both ends of the stack, as frame_hold_ref.held_masks cuts it) is hold .. max_hold frames long."""
    e = np.asarray(e, bool)
    before = np.zeros(e.shape, np.int32)        # edge frames in a row up to and including t
    after = np.zeros(e.shape, np.int32)         # ... from t on
    for t in range(len(e)):
        before[t] = np.where(e[t], (before[t - 1] if t else 0) + 1, 0)
    for t in range(len(e) - 1, -1, -1):
        after[t] = np.where(e[t], (after[t + 1] if t + 1 < len(e) else 0) + 1, 0)
    length = before + after - 1
    return e & (length >= hold) & (length <= max_hold)


def counts(frames, area, edge_thresh, hold, max_hold):
    """A whole clip, uint8 BGR [T,H,W,3], area (y0, y1, x0, x1) -> int32 [T,3]: the rows of all its frames (what a call with fed = 0
    and flush writes)."""
    return rows_of(bounded_masks(edge_mask(frames, area, edge_thresh), hold, max_hold))


def difference_rows(e, hold, max_hold):
    """The same rows in the form the device computes them: every run s..t in range adds 1 to appeared[s] and to vanished[t + 1], and
    the edges are the running sum of appeared - vanished.  bool [T,h,w] -> int32 [T,3]."""
    e = np.asarray(e, bool)
    n = len(e)
    a, v = np.zeros(n + 2, np.int64), np.zeros(n + 2, np.int64)
    run = np.zeros(e.shape[1:], np.int64)
    for u in range(1, n + 2):                   # step n + 1 is the flush: no edge anywhere
        cur = e[u - 1] if u <= n else np.zeros_like(e[0])
        ended = run[~cur & (run >= hold) & (run <= max_hold)]
        v[u] += len(ended)
        np.add.at(a, u - ended, 1)
        run = np.where(cur, run + 1, 0)
    return np.stack([np.cumsum(a - v)[1:n + 1], a[1:n + 1], v[1:n + 1]], 1).astype(np.int32)


def emitted(fed, n, max_hold, flush):
    """-> (lo, hi): a call with n frames after `fed` earlier ones writes the rows of frames lo + 1 .. hi."""
    return max(0, fed - max_hold), fed + n if flush else max(0, fed + n - max_hold)


class NumpyBoundedHoldCounter:
    """count_fn of frame_select.HoldFrameSelector with max_hold_* on the host, with the device's latency: a call returns the rows of
    the frames that max_hold further frames (or the flush) have made final.  It keeps the edge masks a pending row's run can still
    reach, and the last mask it counted."""

    def __init__(self):
        self.calls = 0
        self.first = 1            # frame number of self.masks[0]
        self.masks = None         # bool [k,h,w]
        self.prev = None          # bounded mask of the last frame counted

    def __call__(self, frames, area, edge_thresh, hold, max_hold, fed, flush):
        self.calls += 1
        frames = np.asarray(frames)
        y0, y1, x0, x1 = area
        new = edge_mask(frames, area, edge_thresh) if len(frames) else np.zeros((0, y1 - y0 - 2, x1 - x0 - 2), bool)
        if fed == 0:
            self.first, self.masks, self.prev = 1, new, None
        else:
            assert self.first + len(self.masks) == fed + 1, "frames of a clip arrive in order"
            self.masks = np.concatenate([self.masks, new])
        lo, hi = emitted(fed, len(frames), max_hold, flush)
        # the window starts at least max_hold frames before frame lo + 1 (or at frame 1) and, unless this is the flush, ends at least
        # max_hold frames after frame hi: a run that the window cuts off is longer than max_hold inside it, and out either way
        out = np.zeros((0, 3), np.int32)
        if hi > lo:
            held = bounded_masks(self.masks, hold, max_hold)[lo + 1 - self.first:hi + 1 - self.first]
            out, self.prev = rows_of(held, self.prev), held[-1]
        keep = max(self.first, hi + 1 - max_hold)
        self.masks, self.first = self.masks[keep - self.first:], keep
        return out
