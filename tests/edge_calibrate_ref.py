"""What the edge-threshold calibration's tests share: the host counterpart of vse_frame_cells_multi over the numpy cells of
tests/area_cells_ref.py, one threshold at a time, and the clips of little contrast."""
import numpy as np

import area_cells_ref as R


class NumpyCellsMulti:
    """cells_fn of area_locator.AreaLocator(edge_thresh="auto") on the host: one R.NumpyCells per threshold.  `rows` lists the
    height of every batch of frames it was handed."""

    def __init__(self):
        self.cells = None
        self.calls = 0
        self.rows = []

    def __call__(self, frames, area, params, reset, flush, thresholds=None):
        self.calls += 1
        if frames is not None:
            self.rows.append(np.asarray(frames).shape[1])
        ths = [R.Params(*params).edge_thresh] if thresholds is None else list(thresholds)
        if self.cells is None or len(self.cells) != len(ths):
            self.cells, reset = [R.NumpyCells() for _ in ths], True
        out = np.stack([c(frames, area, R.Params(*params)._replace(edge_thresh=th), reset, flush) for c, th in zip(self.cells, ths)])
        return out[0] if thresholds is None else out


def low_contrast(frames):
    """The clip compressed in contrast: text against its outline at about 89 grey levels, below the constant 128."""
    return (100 + 0.35 * frames).astype(np.uint8)


def noisy_low_contrast(frames, seed=23):
    """low_contrast plus +-20 levels of fresh noise per pixel and frame."""
    rng = np.random.default_rng(seed)
    return np.clip(low_contrast(frames).astype(np.int16) + rng.integers(-20, 21, size=frames.shape, dtype=np.int16), 0, 255).astype(np.uint8)
