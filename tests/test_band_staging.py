"""The plumbing the interval side shares: staging.staged_batches (an uploader's producer thread, or np.stack on the host),
frame_select.band_batches (first frame, clipped area, batches of (full frame, band) that keep no frame behind), and the staged route of
every consumer against its host route with a stand-in uploader.  CPU only."""
import gc
import threading
import weakref

import numpy as np
import pytest

from area_cells_ref import NumpyCells
from frame_change_ref import NumpyCounter
from frame_hold_ref import NumpyHoldCounter
from interval_ref import NumpyCompositor
from test_frame_hold import BAND, moving_clip
from vse_amd import area_locator, extractor, frame_select, staging


class Staged:
    def __init__(self, frames):
        self.frames = frames

    def tensor(self):
        return np.stack(self.frames)


class FakeUploader:
    def __init__(self):
        self.threads = set()

    def bind_thread(self):
        self.threads.add(threading.get_ident())

    def stage(self, frames):
        return Staged([np.array(f) for f in frames])


def batches(n, fail_at=None):
    for b in range(n):
        if b == fail_at:
            raise IOError("decoder died")
        yield [(10 * b + i, np.full((2, 2, 3), b + i, np.uint8)) for i in range(3)]


# ---- staging.staged_batches -----------------------------------------------------------------------------------------------------
def test_staged_batches_host_and_uploader_routes_agree():
    want = list(batches(5))
    host = list(staging.staged_batches(batches(5), None))
    up = FakeUploader()
    staged = list(staging.staged_batches(batches(5), up))
    assert up.threads and threading.get_ident() not in up.threads                  # staged by the producer thread
    for got in (host, staged):
        assert len(got) == 5
        for (items, data), src in zip(got, want):
            assert [k for k, _ in items] == [k for k, _ in src]
            assert all(np.array_equal(f, g) for (_, f), (_, g) in zip(items, src))  # the items unchanged
            assert isinstance(data, np.ndarray) and np.array_equal(data, np.stack([f for _, f in src]))


def test_staged_batches_close_ends_the_producer():
    before = set(threading.enumerate())
    it = staging.staged_batches(batches(50), FakeUploader())
    next(it)
    producers = set(threading.enumerate()) - before
    assert len(producers) == 1
    it.close()                                  # consumer gives up: prefetch is closed, its producer terminates
    assert not any(th.is_alive() for th in producers)


@pytest.mark.parametrize("uploader", [None, FakeUploader()], ids=["host", "staged"])
def test_staged_batches_source_error_reaches_the_consumer(uploader):
    it = staging.staged_batches(batches(5, fail_at=2), uploader)
    assert [items[0][0] for items, _ in (next(it), next(it))] == [0, 10]
    with pytest.raises(IOError, match="decoder died"):
        next(it)


# ---- frame_select.band_batches --------------------------------------------------------------------------------------------------
class Frame(np.ndarray):
    """An ndarray that takes weak references."""


BAND_12 = extractor.SubtitleArea(ymin=2, ymax=9, xmin=0, xmax=20)


def small_frames(n, h=12, w=20):
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8).view(Frame) for _ in range(n)]


def test_band_batches_sizes_geometry_and_bands():
    frames = small_frames(9)
    bands = frame_select.band_batches(iter(frames), extractor.SubtitleArea(ymin=3, ymax=10, xmin=2, xmax=17), 4, "Someone")
    assert (bands.geometry, bands.frame_hw, bands.area) == ((3, 10, 2, 17), (12, 20), (0, 7, 2, 17))   # before the first batch
    got = list(bands)
    assert [len(b) for b in got] == [4, 4, 1]                                       # no empty trailing list
    flat = [pair for b in got for pair in b]
    assert all(full is f and np.array_equal(band, f[3:10]) and band.shape == (7, 20, 3) for (full, band), f in zip(flat, frames))
    assert [len(b) for b in frame_select.band_batches(iter(small_frames(8)), None, 4, "Someone")] == [4, 4]
    whole = frame_select.band_batches(iter(frames), None, 16, "Someone")
    assert (whole.geometry, whole.area) == ((0, 12, 0, 20), (0, 12, 0, 20)) and [len(b) for b in whole] == [9]


def test_band_batches_clips_refuses_and_takes_an_empty_clip():
    frames = small_frames(2)
    outside = frame_select.band_batches(iter(frames), extractor.SubtitleArea(ymin=-5, ymax=40, xmin=4, xmax=99), 4, "Someone")
    assert (outside.geometry, outside.area) == ((0, 12, 4, 20), (0, 12, 4, 20))
    with pytest.raises(ValueError, match="Someone.*3 x 3"):
        frame_select.band_batches(iter(frames), extractor.SubtitleArea(ymin=10, ymax=14, xmin=0, xmax=20), 4, "Someone")   # 2 rows
    assert len(list(frame_select.band_batches(iter(frames), extractor.SubtitleArea(ymin=10, ymax=14, xmin=0, xmax=20), 4, "S", min_size=1))) == 1
    empty = frame_select.band_batches(iter([]), BAND, 4, "Someone")
    assert empty.geometry is None and empty.frame_hw is None and empty.area is None and list(empty) == []


def test_band_batches_keeps_no_frame_behind():
    frames = small_frames(9)
    refs = [weakref.ref(f) for f in frames]
    it = iter(frame_select.band_batches((frames.pop(0) for _ in range(9)), BAND_12, 4, "Someone"))      # the source gives its frames away
    batch = next(it)
    assert [r() is not None for r in refs] == [True] * 9
    del batch                                   # the first batch, the first frame (read ahead for the geometry) included
    gc.collect()
    assert [r() is not None for r in refs] == [False] * 4 + [True] * 5
    batch = next(it)
    del batch
    gc.collect()
    assert [r() is not None for r in refs] == [False] * 8 + [True]


# ---- the staged route of every consumer equals its host route -----------------------------------------------------------------
def run_change(frames, up):
    sel = frame_select.ChangeFrameSelector(NumpyCounter(), batch=16)
    sel.run(list(frames), BAND, uploader=up)
    return sel.counts, sel.intervals


def run_hold(frames, up):
    sel = frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=3, batch=16)
    sel.run(list(frames), BAND, 25.0, uploader=up)
    return sel.counts, sel.intervals


def run_locator(frames, up):
    loc = area_locator.AreaLocator(NumpyCells(), batch=16)
    loc.run(list(frames), 25.0, uploader=up)
    return loc.totals, loc.area


def run_compositor(frames, up):
    intervals = frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=3, batch=16).run(list(frames), BAND, 25.0)
    assert len(intervals) == 4
    comp = frame_select.IntervalCompositor(NumpyCompositor(), batch=16)
    patches = comp.run(list(frames), BAND, intervals, 25.0, uploader=up)
    return sorted(patches), [patches[k] for k in sorted(patches)]


@pytest.mark.parametrize("consumer", [run_change, run_hold, run_locator, run_compositor], ids=lambda f: f.__name__[4:])
def test_staged_route_equals_host_route(consumer):
    frames, _truth = moving_clip()                                                 # 120 x 320, 95 frames: six batches of 16
    up = FakeUploader()
    host, staged = consumer(frames, None), consumer(frames, up)
    assert up.threads and threading.get_ident() not in up.threads
    for a, b in zip(host, staged):
        if isinstance(a, list) and a and isinstance(a[0], np.ndarray):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        elif isinstance(a, np.ndarray):
            assert a.size and np.array_equal(a, b)
        else:
            assert a == b
