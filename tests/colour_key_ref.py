"""numpy restatement of the colour key (include/vse_hip.h vse_colour_key): the device kernel and frame_select.ColourKey.apply must agree
with it integer for integer, and the CPU tests drive the selectors with it as their key_fn."""
import numpy as np


def slope_of(tol):
    """ceil(255 * 256 / tol): K = 255 at d = 0 and K = 0 from d = tol on."""
    return -(-255 * 256 // int(tol))


def key_of_distance(d, slope):
    """K = max(0, 255 - ((d * slope) >> 8)) for d int (array) in 0..255."""
    return np.maximum(0, 255 - ((np.asarray(d, np.int64) * int(slope)) >> 8)).astype(np.int32)


def key_plane(frames, bgr, slope):
    """uint8 BGR [..., 3] -> int32 [...]: K of every pixel."""
    d = np.abs(np.asarray(frames).astype(np.int32) - np.asarray(bgr, np.int32)).max(-1)
    return key_of_distance(d, slope)


def colour_key(frames, area, bgr, slope):
    """uint8 BGR [n,H,W,3], area (y0, y1, x0, x1) -> uint8 of the same shape: (K, K, K) inside the area, 0 elsewhere."""
    frames = np.asarray(frames)
    y0, y1, x0, x1 = area
    out = np.zeros(frames.shape, np.uint8)
    out[:, y0:y1, x0:x1] = key_plane(frames[:, y0:y1, x0:x1], bgr, slope)[..., None]
    return out


class NumpyKey:
    """key_fn of the selectors and the locator on the host: (frames, area) -> colour_key of them; `calls` keeps (shape, area) per call."""

    def __init__(self, bgr, tol):
        self.bgr, self.slope = tuple(bgr), slope_of(tol)
        self.calls = []

    def __call__(self, frames, area):
        self.calls.append((tuple(np.asarray(frames).shape), tuple(area)))
        return colour_key(frames, area, self.bgr, self.slope)
