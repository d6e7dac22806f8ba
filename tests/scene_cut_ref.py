"""numpy restatement of the scene-cut counts (include/vse_hip.h vse_scene_change): the device kernel must agree with it bit for
bit, and the CPU tests drive the host keyframe detector with it."""
import numpy as np

MB = 16


def planes(frames, scale):
    """uint8 BGR [n,H,W,3] -> int32 [n, H // scale, W // scale]: the box-filtered luma planes."""
    f = np.asarray(frames)
    s = int(scale)
    ah, aw = f.shape[1] // s, f.shape[2] // s
    a = f[:, :ah * s, :aw * s].astype(np.int32)
    y = (29 * a[..., 0] + 150 * a[..., 1] + 77 * a[..., 2] + 128) >> 8
    box = y.reshape(len(f), ah, s, aw, s).sum((2, 4))
    return (box + (s * s) // 2) // (s * s)


def _blocks(x, bh, bw):
    """[.., bh * 16, bw * 16] -> per-block sums [.., bh, bw]"""
    return x.reshape(*x.shape[:-2], bh, MB, bw, MB).sum((-3, -1))


def inter_intra(cur, prev, search):
    """One plane and its predecessor (int32 [ah, aw]) -> (inter [bh, bw], intra [bh, bw]); zero_sad rides along as a third array."""
    ah, aw = cur.shape
    bh, bw = ah // MB, aw // MB
    c = cur[:bh * MB, :bw * MB]
    m = (_blocks(c, bh, bw) + 128) >> 8
    intra = _blocks(np.abs(c - np.repeat(np.repeat(m, MB, 0), MB, 1)), bh, bw)
    best = np.full((bh, bw), np.iinfo(np.int32).max, np.int64)
    zero = None
    for dy in range(-search, search + 1):
        # block rows whose displaced block lies inside the plane: 0 <= 16 by + dy and 16 by + dy + 16 <= ah
        y_lo = max(0, -(dy // MB)) if dy < 0 else 0
        y_hi = min(bh, (ah - MB - dy) // MB + 1)
        if y_hi <= y_lo:
            continue
        for dx in range(-search, search + 1):
            x_lo = max(0, -(dx // MB)) if dx < 0 else 0
            x_hi = min(bw, (aw - MB - dx) // MB + 1)
            if x_hi <= x_lo:
                continue
            a = c[y_lo * MB:y_hi * MB, x_lo * MB:x_hi * MB]
            p = prev[y_lo * MB + dy:y_hi * MB + dy, x_lo * MB + dx:x_hi * MB + dx]
            sad = _blocks(np.abs(a - p), y_hi - y_lo, x_hi - x_lo)
            view = best[y_lo:y_hi, x_lo:x_hi]
            np.minimum(view, sad, out=view)
            if dy == 0 and dx == 0:
                zero = sad
    return best, intra, zero


def counts(frames, scale, search, bias, prev=None, with_zero=False):
    """-> (int32 [n,3] changed blocks / sum inter / sum intra, the last frame's plane).  prev: the plane of the frame before the
    first (None = no predecessor).  with_zero: a third result, int64 [n]: the sum of the blocks' zero-vector SADs (0 for a frame
    without a predecessor)."""
    a = planes(frames, scale)
    bh, bw = a.shape[1] // MB, a.shape[2] // MB
    assert bh >= 1 and bw >= 1
    out = np.zeros((len(a), 3), np.int32)
    zeros = np.zeros(len(a), np.int64)
    for t in range(len(a)):
        p = prev if t == 0 else a[t - 1]
        if p is None:
            c = a[t][:bh * MB, :bw * MB]
            m = (_blocks(c, bh, bw) + 128) >> 8
            out[t] = (bh * bw, 0, np.abs(c - np.repeat(np.repeat(m, MB, 0), MB, 1)).sum())
            continue
        inter, intra, zero = inter_intra(a[t], p, search)
        out[t] = ((2 * inter > intra + bias).sum(), inter.sum(), intra.sum())
        zeros[t] = zero.sum()
    return (out, a[-1], zeros) if with_zero else (out, a[-1])


class NumpySceneCounter:
    """The counter of keyframes.SceneCutDetector on the host: carries the last plane from one batch to the next."""

    def __init__(self):
        self.prev = None
        self.calls = 0

    def __call__(self, frames, scale, search, bias, reset):
        self.calls += 1
        out, self.prev = counts(frames, scale, search, bias, None if reset else self.prev)
        return out
