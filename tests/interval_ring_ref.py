"""numpy restatement of the ring of vse_interval_stream (stores only) and of vse_interval_ring_rank (include/vse_hip.h): the device
kernel must agree with it byte for byte, and the CPU tests drive frame_select.StreamingQuantile with it.  The ring is a dict keyed by
slot that remembers which frame each slot holds, and a rank that names a frame which is not there raises: a planner's mistake
surfaces on the CPU."""
import numpy as np

MAX_GROUPS = 8
RANK_MAX = 63


class Ring:
    """`cap` area bands, frame f in slot f % cap: {slot: (frame number, area pixels)}."""

    def __init__(self, cap):
        if cap < 1:
            raise ValueError(f"cap {cap} is below 1")
        self.cap, self.slots = cap, {}

    def store(self, frames, fed):
        """frames: uint8 [n, ah, aw, 3], the area's pixels of the frames fed + 1 .. fed + n."""
        for k, f in enumerate(frames):
            self.slots[(fed + 1 + k) % self.cap] = (fed + 1 + k, np.array(f))

    def rank(self, groups, fed):
        """groups: [(frame numbers, rank[, out])] -> uint8 [patches, ah, aw, 3]: per byte, element `rank` of the named frames' values
        sorted ascending (without `out`, group k is patch k).  ValueError for what the library refuses about the groups, LookupError
        for a frame the ring does not hold."""
        if fed < 0 or len(groups) > MAX_GROUPS:
            raise ValueError("bad fed or number of groups")
        outs = {}
        for k, g in enumerate(groups):
            nos, r = [int(v) for v in g[0]], int(g[1])
            out = int(g[2]) if len(g) > 2 else k
            if not 1 <= len(nos) <= RANK_MAX or not 0 <= r < len(nos) or out < 0:
                raise ValueError(f"group {k}: {len(nos)} frames, rank {r}, out {out}")
            if any(b <= a for a, b in zip(nos, nos[1:])) or nos[0] < 1 or nos[0] <= fed - self.cap or nos[-1] > fed:
                raise ValueError(f"group {k}: frames {nos} must ascend strictly inside ({fed - self.cap}, {fed}]")
            bands = []
            for f in nos:
                held = self.slots.get(f % self.cap)
                if held is None or held[0] != f:
                    raise LookupError(f"frame {f} is not in the ring (slot {f % self.cap} holds {None if held is None else held[0]})")
                bands.append(held[1])
            outs[out] = np.sort(np.stack(bands), axis=0)[r]
        if not outs:
            return None
        first = next(iter(outs.values()))
        res = np.zeros((max(outs) + 1,) + first.shape, np.uint8)
        for k, patch in outs.items():
            res[k] = patch
        return res


class NumpyRingRanker:
    """ring_fn of frame_select.StreamingQuantile on the host: keeps one Ring per clip (a call with fed == 0 that stores starts a new
    one) and what it was called with."""

    def __init__(self):
        self.ring = None
        self.calls = []               # (frames stored, groups ranked)
        self.max_groups = 0

    def __call__(self, frames, area, cap, fed, n, groups):
        y0, y1, x0, x1 = area
        if self.ring is None or (fed == 0 and n):
            self.ring = Ring(cap)
        assert self.ring.cap == cap and len(frames) == n
        self.calls.append((n, len(groups)))
        self.max_groups = max(self.max_groups, len(groups))
        self.ring.store(np.asarray(frames)[:, y0:y1, x0:x1], fed)
        out = self.ring.rank(groups, fed + n)
        return np.zeros((0, y1 - y0, x1 - x0, 3), np.uint8) if out is None else out
