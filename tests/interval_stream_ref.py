"""numpy restatement of vse_interval_stream (include/vse_hip.h), built on interval_ref.accumulate / composite: the device kernel must
agree with it byte for byte, and the CPU tests drive frame_select.StreamingCompositor with it.  The ring is a dict keyed by slot that
remembers which frame each slot holds, and a read of a frame that is not there raises: a planner's mistake surfaces on the CPU."""
import numpy as np

import interval_ref

CONTINUE, EMIT = 1, 2
MAX_SEGS = 32


class Stream:
    """The state of one clip: `acc` = (mn, mx, sm) as the last call's last segment left them (None: unspecified), `ring` = {slot:
    (frame number, area pixels)}.  `peak`: the most frames the ring held that a later call could still name, by the caller's floors."""

    def __init__(self, cap):
        self.cap, self.acc, self.ring = cap, None, {}
        self.calls = 0

    def _frame(self, f, frames, fed, area):
        y0, y1, x0, x1 = area
        if f > fed:
            return np.asarray(frames[f - fed - 1])[y0:y1, x0:x1]
        held = self.ring.get(f % self.cap)
        if held is None or held[0] != f:
            raise LookupError(f"frame {f} is not in the ring (slot {f % self.cap} holds {None if held is None else held[0]})")
        return held[1]

    def stream(self, frames, area, fed, segs, store_from, mode):
        """frames: uint8 [n,H,W,3], the frames fed + 1 .. fed + n; segs: (first, last, flags, frames[, out]) -> [patches, ah, aw, 3]
        (without `out`, the EMITs are numbered in order).  ValueError for what the library refuses about the segments."""
        n = len(frames)
        self.calls += 1
        if self.cap < 1 or fed < 0 or len(segs) > MAX_SEGS or mode not in interval_ref.MODES:
            raise ValueError("bad cap, fed, number of segments or mode")
        prev, outs = fed - self.cap, {}
        for k, g in enumerate(segs):
            first, last, flags, count = (int(v) for v in g[:4])
            emit = bool(flags & EMIT)
            if (first > last or first < 1 or first <= prev or last > fed + n or flags & ~3 or (flags & CONTINUE and k) or (not emit and k != len(segs) - 1)
                    or (emit and mode == "mean" and not 1 <= count <= 4194304)):
                raise ValueError(f"segment {k} {tuple(g)} with fed {fed}, n {n}, cap {self.cap}")
            prev = last
        for k, g in enumerate(segs):                      # every read comes before every store
            first, last, flags, count = (int(v) for v in g[:4])
            if flags & CONTINUE and self.acc is None:
                raise LookupError("CONTINUE, but the accumulators hold nothing")
            stack = np.stack([self._frame(f, frames, fed, area) for f in range(first, last + 1)])
            acc = interval_ref.accumulate(self.acc if flags & CONTINUE else None, stack, (0, stack.shape[1], 0, stack.shape[2]))
            if flags & EMIT:
                outs[int(g[4]) if len(g) > 4 else len(outs)] = interval_ref.composite(acc, count, mode)
                self.acc = None
            else:
                self.acc = acc
        y0, y1, x0, x1 = area
        for f in range(max(store_from, fed + 1), fed + n + 1):
            self.ring[f % self.cap] = (f, np.array(np.asarray(frames[f - fed - 1])[y0:y1, x0:x1]))
        if not outs:
            return np.zeros((0, y1 - y0, x1 - x0, 3), np.uint8)
        res = np.zeros((max(outs) + 1, y1 - y0, x1 - x0, 3), np.uint8)
        for k, patch in outs.items():
            res[k] = patch
        return res


class NumpyStreamer:
    """stream_fn of frame_select.StreamingCompositor on the host: keeps one Stream per clip (a call with fed == 0 starts a new one)."""

    def __init__(self):
        self.state = None
        self.calls = 0
        self.peak_ring = 0

    def __call__(self, frames, area, cap, fed, segs, store_from, mode):
        # a new clip starts at fed == 0; a Stream that holds nothing yet is as good as a new one (a split first batch calls twice)
        if self.state is None or (fed == 0 and (self.state.ring or self.state.acc is not None or self.state.cap != cap)):
            self.state = Stream(cap)
        assert self.state.cap == cap
        self.calls += 1
        out = self.state.stream(np.asarray(frames), area, fed, segs, store_from, mode)
        # what a later call may still name: the frames from store_from on that are in the ring
        floor = min(store_from, fed + len(frames) + 1)
        self.peak_ring = max(self.peak_ring, sum(1 for f, _p in self.state.ring.values() if f >= floor))
        return out
