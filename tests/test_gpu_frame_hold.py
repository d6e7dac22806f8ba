"""vse_frame_hold on the MI355X, through the C ABI: the rows equal the numpy restatement (tests/frame_hold_ref.py) bit for bit, fed
whole or in batches, on every tile shape the kernel distinguishes; hold = 1 is vse_frame_change; bad arguments are refused before
anything reaches the device; and HoldFrameSelector on the engine finds the subtitles of a clip whose background moves."""
import ctypes as C

import numpy as np
import pytest

from frame_change_ref import edge_mask
from frame_hold_ref import counts as ref_counts, emitted

pytestmark = pytest.mark.gpu

THRESH = 96
GUARD = 3                 # rows behind the n + hold - 1 the call may write; they must stay as they were

# name -> (frame h, frame w, area (y0, y1, x0, x1) in the frame, how it is passed)
SHAPES = {
    "3x3": (3, 3, (0, 3, 0, 3), "whole"),                        # one interior pixel
    "5x66": (5, 66, (0, 5, 0, 66), "whole"),                     # exactly one word
    "10x67": (10, 67, (0, 10, 0, 67), "whole"),                  # a full 8-row tile plus a one-bit second word
    "11x131": (11, 131, (0, 11, 0, 131), "whole"),               # a tile plus one row, three words
    "11x131-offset": (40, 200, (17, 28, 45, 176), "padded"),     # an offset area in a larger frame with a padded pitch
    "11x131-rows": (40, 200, (17, 28, 45, 176), "rows"),         # the same area passed as its rows alone
}
CASES = [(s, h) for s in SHAPES for h in (1, 2, 3, 8)] + [(s, 32) for s in SHAPES if s.startswith("11x131")]
_cache = {}


def persistent_frames(n, h, w, hold, seed):
    """Frame 0 is uniform random bytes; in each later frame every 4 x 4 block is redrawn with probability 1 / hold and every other
    block is copied from the frame before: edges live about `hold` frames, so runs shorter and longer than `hold` are both common."""
    rng = np.random.default_rng(seed)
    f = np.empty((n, h, w, 3), np.uint8)
    f[0] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for t in range(1, n):
        fresh = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        redraw = rng.random(((h + 3) // 4, (w + 3) // 4)) < 1.0 / hold
        redraw = np.repeat(np.repeat(redraw, 4, 0), 4, 1)[:h, :w, None]
        f[t] = np.where(redraw, fresh, f[t - 1])
    return f


def case_data(shape, hold):
    """-> (frames, area, reference rows); computed once per frame size and hold, never modified."""
    h, w, area, _how = SHAPES[shape]
    key = (h, w, area, hold)
    if key not in _cache:
        frames = persistent_frames(2 * hold + 70, h, w, hold, seed=1000 * h + 10 * w + hold)
        frames.setflags(write=False)
        want = ref_counts(frames, area, THRESH, hold)
        want.setflags(write=False)
        _cache[key] = (frames, area, want)
    return _cache[key]


def device_view(ctx, frames, area, how):
    """-> (cuda uint8 [n,H,W,3] view, the area in its pixels)"""
    import torch
    n, h, w, _ = frames.shape
    y0, y1, x0, x1 = area
    if how == "rows":
        return torch.from_numpy(np.ascontiguousarray(frames[:, y0:y1])).to(ctx.tdev), (0, y1 - y0, x0, x1)
    if how == "padded":
        padded = torch.zeros((n, h + 3, w * 3 + 17), dtype=torch.uint8, device=ctx.tdev)
        view = padded[:, 2:2 + h, 6:6 + 3 * w].view(n, h, w, 3)
        view.copy_(torch.from_numpy(frames.copy()))
        assert view.stride(1) == w * 3 + 17 and view.stride(0) == (h + 3) * (w * 3 + 17)
        return view, area
    return torch.from_numpy(frames.copy()).to(ctx.tdev), area


def call(ctx, view, area, hold, state, fed, flush, first=0, n=None, thresh=THRESH):
    """One vse_frame_hold call on frames first .. first + n of the view -> host int32 rows; checks the rows it must not write."""
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    n = view.shape[0] - first if n is None else n
    part = view[first:first + n]
    out = torch.full((n + hold - 1 + GUARD, 3), -7, dtype=torch.int32, device=ctx.tdev)
    rc = lib.vse_frame_hold(ctx.handle, C.c_void_p(part.data_ptr()) if n else None, n, view.shape[1], view.shape[2], view.stride(1),
                            view.stride(0), *area, thresh, hold, C.c_void_p(state.data_ptr()), fed, int(flush),
                            C.c_void_p(out.data_ptr()), ctx.stream())
    assert rc == 0, lib.vse_last_error().decode()
    lo, hi = emitted(fed, n, hold, flush)
    out = out.cpu().numpy()
    assert (out[hi - lo:] == -7).all(), "rows behind the emitted ones were written"
    return out[:hi - lo]


def fed_in(ctx, view, area, hold, sizes, state=None):
    """The clip in batches of `sizes` frames, then a flush without frames -> all rows."""
    state = ctx.frame_hold_state(area[1] - area[0], area[3] - area[2], hold) if state is None else state
    out, fed = [], 0
    for n in sizes:
        out.append(call(ctx, view, area, hold, state, fed, False, first=fed, n=n))
        fed += n
    assert fed == view.shape[0]
    out.append(call(ctx, view, area, hold, state, fed, True, first=fed, n=0))
    return np.concatenate(out)


@pytest.mark.parametrize("shape,hold", CASES)
def test_reference_rows_are_busy(shape, hold):
    """The precondition of the comparison below, on the reference alone: all three columns are nonzero in at least a third of the
    rows from row `hold` on (one interior pixel cannot be that busy)."""
    _frames, _area, want = case_data(shape, hold)
    assert want.shape == (2 * hold + 70, 3)
    if shape != "3x3":
        busy = int((want[hold:] > 0).all(1).sum())
        assert 3 * busy >= len(want) - hold, (busy, len(want) - hold)


@pytest.mark.parametrize("shape,hold", CASES)
def test_rows_match_numpy(ctx, shape, hold):
    frames, area, want = case_data(shape, hold)
    view, dev_area = device_view(ctx, frames, area, SHAPES[shape][3])
    n = len(frames)
    state = ctx.frame_hold_state(area[1] - area[0], area[3] - area[2], hold)
    whole = call(ctx, view, dev_area, hold, state, 0, True)                          # one call: two LDS chunks, then the flush steps
    assert np.array_equal(whole, want), (shape, hold)
    split = fed_in(ctx, view, dev_area, hold, (1, hold - 1, hold, 64, n - 2 * hold - 64))
    assert np.array_equal(split, want), (shape, hold)


def test_flush_without_frames_drains_the_pending_rows(ctx):
    frames, area, want = case_data("11x131", 8)
    view, area = device_view(ctx, frames, area, "whole")
    state = ctx.frame_hold_state(11, 131, 8)
    head = call(ctx, view, area, 8, state, 0, False)
    assert len(head) == len(frames) - 7 and np.array_equal(head, want[:-7])
    tail = call(ctx, view, area, 8, state, len(frames), True, first=len(frames), n=0)
    assert len(tail) == 7 and np.array_equal(np.concatenate([head, tail]), want)
    # a clip shorter than hold: nothing until the flush, and no run is long enough
    state = ctx.frame_hold_state(11, 131, 8)
    assert len(call(ctx, view, area, 8, state, 0, False, n=5)) == 0
    assert np.array_equal(call(ctx, view, area, 8, state, 5, True, first=5, n=0), np.zeros((5, 3), np.int32))


@pytest.mark.parametrize("hold", [3, 32])
def test_second_clip_on_a_dirty_state(ctx, hold):
    frames, area, want = case_data("11x131", hold)
    view, area = device_view(ctx, frames, area, "whole")
    state = ctx.frame_hold_state(11, 131, hold)
    call(ctx, view, area, hold, state, 0, False, first=7, n=40)                     # a clip left open: runs and a counted mask pending
    assert int(state.count_nonzero()) > 0
    assert np.array_equal(fed_in(ctx, view, area, hold, (len(frames),), state=state), want)


def test_hold_one_is_frame_change(ctx):
    for shape in ("10x67", "11x131-offset"):
        frames, area, want = case_data(shape, 1)
        view, dev_area = device_view(ctx, frames, area, SHAPES[shape][3])
        st = ctx.frame_change_state(area[1] - area[0], area[3] - area[2])
        change = ctx.frame_change(view, dev_area, THRESH, st, reset=True).cpu().numpy()
        assert np.array_equal(change, want)
        assert np.array_equal(fed_in(ctx, view, dev_area, 1, (len(frames),)), change)


def test_rejects_bad_arguments(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the areas below
    st = torch.zeros(1 << 14, dtype=torch.uint8, device=ctx.tdev)
    cnt = torch.full((40, 3), -7, dtype=torch.int32, device=ctx.tdev)

    def rc(n=1, area=(0, 10, 0, 20), hold=2, fed=0, flush=1, state=st):
        return lib.vse_frame_hold(ctx.handle, C.c_void_p(buf.data_ptr()), n, 10, 20, 60, 600, *area, 128, hold,
                                  C.c_void_p(state.data_ptr()) if state is not None else None, fed, flush,
                                  C.c_void_p(cnt.data_ptr()), ctx.stream())
    for area in [(0, 2, 0, 10), (0, 10, 5, 7), (-1, 5, 0, 10), (0, 11, 0, 10), (0, 10, 0, 21), (4, 4, 0, 10)]:
        assert rc(area=area) == -1, area
        assert "area" in lib.vse_last_error().decode()
    for hold in (0, -1, 33):
        assert rc(hold=hold) == -1, hold
        assert "hold" in lib.vse_last_error().decode()
    assert rc(n=-1) == -1 and rc(fed=-1) == -1 and rc(state=None) == -1
    assert (cnt.cpu().numpy() == -7).all() and int(st.count_nonzero()) == 0      # nothing was enqueued
    assert rc(n=0, flush=0) == 0 and (cnt.cpu().numpy() == -7).all()             # nothing to do is not an error
    assert rc() == 0 and cnt.cpu().numpy()[:1].tolist() == [[0, 0, 0]]           # the same call with good arguments runs
    sb = lib.vse_frame_hold_state_bytes
    assert sb(2, 100, 2) == 0 and sb(100, 2, 2) == 0 and sb(10, 100, 0) == 0 and sb(10, 100, 33) == 0
    assert sb(3, 3, 1) > 0 and sb(11, 131, 32) >= sb(3, 3, 32) > 0


@pytest.mark.parametrize("staged", [False, True])
def test_hold_selector_on_engine_finds_the_moving_clip_truth(ctx, staged):
    from test_frame_hold import BAND, MOVING
    from vse_amd import frame_select, staging, synth
    if "moving" not in _cache:
        _cache["moving"] = synth.make_moving_clip(MOVING)
    frames, truth = _cache["moving"]
    sel = frame_select.HoldFrameSelector(frame_select.EngineHoldCounter(ctx), hold_frames=5, batch=40)
    got = sel.run(list(frames), BAND, 25.0, uploader=staging.Uploader(ctx.tdev) if staged else None)
    assert [(s, e) for s, e, _r in got] == [(s, e) for s, e, _t in truth]
    assert np.array_equal(sel.counts, ref_counts(frames, (60, 120, 0, 320), 128, 5))
    assert edge_mask(frames[:1], (60, 120, 0, 320), 128).sum() > 500                # the background alone is full of edges
