"""vse_frame_hold_bounded on the MI355X, through the C ABI: the rows equal the numpy restatement (tests/frame_hold_bounded_ref.py) bit
for bit, fed whole or in batches of any size, on every tile shape the kernel distinguishes and on clips that straddle its 64-step
launches and wrap its ring of pending rows; max_hold >= the clip's length is vse_frame_hold; bad arguments are refused before anything
reaches the device; and HoldFrameSelector(max_hold_frames=...) on the engine finds the subtitles over a busy background that stands
still."""
import ctypes as C

import numpy as np
import pytest

from frame_change_ref import edge_mask
from frame_hold_bounded_ref import counts as ref_counts, emitted
from test_gpu_frame_hold import device_view

pytestmark = pytest.mark.gpu

THRESH = 96
GUARD = 3                 # rows behind the n + max_hold the call may write; they must stay as they were
BLOCK = 4                 # the squares of the content

# name -> (frame h, frame w, area (y0, y1, x0, x1) in the frame, how it is passed)
SHAPES = {
    "3x3": (3, 3, (0, 3, 0, 3), "whole"),                        # one interior pixel
    "10x67": (10, 67, (0, 10, 0, 67), "whole"),                  # a full 8-row tile, two words, the second of one bit
    "17x130": (17, 130, (0, 17, 0, 130), "whole"),               # two tile rows, the second of 7 rows; two full words
    "17x130-offset": (40, 200, (17, 34, 45, 175), "padded"),     # the same area off zero in a larger frame with a padded pitch
    "12x180-offset": (30, 260, (9, 21, 33, 213), "padded"),      # three words, the last ragged; a tile row of 2 rows
}
HOLDS = (1, 3)


def max_holds(hold, n):
    return (hold, 5, 40, n + 7)             # the last: no run of the clip is too long, vse_frame_hold's rows


CASES = [(s, 130, h, m) for s in SHAPES for h in HOLDS for m in max_holds(h, 130)] + \
        [(s, n, h, m) for s in ("10x67", "17x130-offset") for n in (63, 64, 65) for h in HOLDS for m in max_holds(h, n)]
_cache = {}


def square_frames(n, h, w, hold, max_hold, seed):
    """A flat grey picture (no edge) on which every 4 x 4 square is switched on, showing a random texture of its own, and off again
    for random numbers of frames.  The lengths are drawn from those around which the kernel decides: hold - 1, hold, max_hold and
    max_hold + 1 among them.  The inner 2 x 2 pixels of a square see only the square itself, so their runs are exactly as long as the
    square is shown; a square may be on at the first frame and at the last, where the clip cuts its run off."""
    rng = np.random.default_rng(seed)
    decisive = [k for k in (hold - 1, hold, max_hold, max_hold + 1) if 1 <= k < n]       # every other square is shown that long
    lengths = sorted({1, 2, 3, 4, 6, 9, 41, 70, hold + 1, max(1, max_hold - 1)})
    f = np.full((n, h, w, 3), 128, np.uint8)
    for by in range(0, h, BLOCK):
        for bx in range(0, w, BLOCK):
            t, on = 0, bool(rng.integers(0, 2))
            while t < n:
                k = int(rng.choice(decisive if rng.integers(0, 2) else lengths)) if on else int(rng.integers(1, 4))
                if on:
                    f[t:t + k, by:by + BLOCK, bx:bx + BLOCK] = rng.integers(0, 256, (BLOCK, BLOCK, 3), dtype=np.uint8)[:h - by, :w - bx]
                t, on = t + k, not on
    return f


def run_lengths(e):
    """bool [T,h,w] -> int [T,h,w]: at every edge pixel the length of its run (cut off at both ends of the clip), elsewhere 0."""
    before, after = np.zeros(e.shape, np.int32), np.zeros(e.shape, np.int32)
    for t in range(len(e)):
        before[t] = np.where(e[t], (before[t - 1] if t else 0) + 1, 0)
    for t in range(len(e) - 1, -1, -1):
        after[t] = np.where(e[t], (after[t + 1] if t + 1 < len(e) else 0) + 1, 0)
    return np.where(e, before + after - 1, 0)


def case_data(shape, n, hold, max_hold):
    """-> (frames, area, reference rows); computed once per case, never modified."""
    h, w, area, _how = SHAPES[shape]
    key = (h, w, area, n, hold, max_hold)
    if key not in _cache:
        frames = square_frames(n, h, w, hold, max_hold, seed=100000 * h + 1000 * w + 100 * hold + max_hold + n)
        frames.setflags(write=False)
        want = ref_counts(frames, area, THRESH, hold, max_hold)
        want.setflags(write=False)
        _cache[key] = (frames, area, want)
    return _cache[key]


def call(ctx, view, area, hold, max_hold, state, fed, flush, first=0, n=None, thresh=THRESH):
    """One vse_frame_hold_bounded call on frames first .. first + n of the view -> host int32 rows; checks the rows it must not write."""
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    n = view.shape[0] - first if n is None else n
    part = view[first:first + n]
    out = torch.full((n + max_hold + GUARD, 3), -7, dtype=torch.int32, device=ctx.tdev)
    rc = lib.vse_frame_hold_bounded(ctx.handle, C.c_void_p(part.data_ptr()) if n else None, n, view.shape[1], view.shape[2], view.stride(1),
                                    view.stride(0), *area, thresh, hold, max_hold, C.c_void_p(state.data_ptr()), fed, int(flush),
                                    C.c_void_p(out.data_ptr()), ctx.stream())
    assert rc == 0, lib.vse_last_error().decode()
    lo, hi = emitted(fed, n, max_hold, flush)
    out = out.cpu().numpy()
    assert (out[hi - lo:] == -7).all(), "rows behind the emitted ones were written"
    return out[:hi - lo]


def fed_in(ctx, view, area, hold, max_hold, sizes, state=None):
    """The clip in batches of `sizes` frames, then a flush without frames -> all rows."""
    state = ctx.frame_hold_bounded_state(area[1] - area[0], area[3] - area[2], max_hold) if state is None else state
    out, fed = [], 0
    for n in sizes:
        out.append(call(ctx, view, area, hold, max_hold, state, fed, False, first=fed, n=n))
        fed += n
    assert fed == view.shape[0]
    out.append(call(ctx, view, area, hold, max_hold, state, fed, True, first=fed, n=0))
    return np.concatenate(out)


def batches(n, b):
    return (b,) * (n // b) + ((n % b,) if n % b else ())


@pytest.mark.parametrize("shape,n,hold,max_hold", CASES)
def test_reference_rows_cover_the_decisions(shape, n, hold, max_hold):
    """The precondition of the comparison below, on the reference alone: the clip holds runs of exactly hold - 1, hold, max_hold and
    max_hold + 1 frames and runs that the clip's start and end cut off, and all three columns of the rows are busy."""
    frames, area, want = case_data(shape, n, hold, max_hold)
    assert want.shape == (n, 3)
    if shape == "3x3":
        return                                 # one interior pixel cannot hold all of that
    e = edge_mask(frames, area, THRESH)
    seen = set(np.unique(run_lengths(e)).tolist())
    for length in (hold - 1, hold, max_hold, max_hold + 1):
        if 1 <= length < n:
            assert length in seen, (length, sorted(seen))
    assert e[0].any() and e[-1].any() and (e[0] & e[1]).any() and (e[-1] & e[-2]).any()
    assert (want > 0).all(1).sum() >= n // 3, int((want > 0).all(1).sum())


@pytest.mark.parametrize("shape,n,hold,max_hold", CASES)
def test_rows_match_numpy(ctx, shape, n, hold, max_hold):
    frames, area, want = case_data(shape, n, hold, max_hold)
    view, dev_area = device_view(ctx, frames, area, SHAPES[shape][3])
    state = ctx.frame_hold_bounded_state(area[1] - area[0], area[3] - area[2], max_hold)
    whole = call(ctx, view, dev_area, hold, max_hold, state, 0, True)               # one call, worked through in launches of 64 steps
    assert np.array_equal(whole, want), (shape, n, hold, max_hold)
    for b in (1, 7, 64, 100):                  # with max_hold <= 40 the 130-frame clip is longer than the ring: its slots are reused
        split = fed_in(ctx, view, dev_area, hold, max_hold, batches(n, b))
        assert np.array_equal(split, want), (shape, n, hold, max_hold, b)
    if max_hold >= n:                          # nothing is too long: vse_frame_hold's rows, from the same device
        st = ctx.frame_hold_state(area[1] - area[0], area[3] - area[2], hold)
        assert np.array_equal(ctx.frame_hold(view, dev_area, THRESH, hold, st, 0, flush=True).cpu().numpy(), want)


def test_largest_max_hold_and_the_context_method(ctx):
    frames, area, want = case_data("10x67", 65, 3, 72)
    view, area = device_view(ctx, frames, area, "whole")
    state = ctx.frame_hold_bounded_state(10, 67, 4000)
    assert np.array_equal(call(ctx, view, area, 3, 4000, state, 0, True), want)
    state = ctx.frame_hold_bounded_state(10, 67, 72)
    head = ctx.frame_hold_bounded(view[:50], area, THRESH, 3, 72, state, 0)
    assert tuple(head.shape) == (0, 3)
    tail = ctx.frame_hold_bounded(view[50:], area, THRESH, 3, 72, state, 50, flush=True)
    assert np.array_equal(tail.cpu().numpy(), want)


def test_flush_without_frames_drains_the_pending_rows(ctx):
    frames, area, want = case_data("17x130", 130, 3, 40)
    view, area = device_view(ctx, frames, area, "whole")
    state = ctx.frame_hold_bounded_state(17, 130, 40)
    head = call(ctx, view, area, 3, 40, state, 0, False)
    assert len(head) == 90 and np.array_equal(head, want[:90])
    tail = call(ctx, view, area, 3, 40, state, 130, True, first=130, n=0)
    assert len(tail) == 40 and np.array_equal(np.concatenate([head, tail]), want)
    # a clip shorter than max_hold: nothing until the flush
    short = ref_counts(frames[:30], (0, 17, 0, 130), THRESH, 3, 40)
    state = ctx.frame_hold_bounded_state(17, 130, 40)
    assert len(call(ctx, view, area, 3, 40, state, 0, False, n=30)) == 0
    assert np.array_equal(call(ctx, view, area, 3, 40, state, 30, True, first=30, n=0), short)


@pytest.mark.parametrize("max_hold", [5, 40])
def test_second_clip_on_a_stale_state(ctx, max_hold):
    frames, area, want = case_data("17x130", 130, 3, max_hold)
    view, area = device_view(ctx, frames, area, "whole")
    state = ctx.frame_hold_bounded_state(17, 130, max_hold)
    call(ctx, view, area, 3, max_hold, state, 0, False, first=7, n=90)              # a clip left open: runs, pending rows and a carry
    assert int(state.count_nonzero()) > 0
    assert np.array_equal(fed_in(ctx, view, area, 3, max_hold, (130,), state=state), want)
    state.fill_(0xff)                                                             # ... or anything at all
    assert np.array_equal(fed_in(ctx, view, area, 3, max_hold, (100, 30), state=state), want)


def test_rejects_bad_arguments(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the areas below
    st = torch.zeros(1 << 14, dtype=torch.uint8, device=ctx.tdev)
    cnt = torch.full((40, 3), -7, dtype=torch.int32, device=ctx.tdev)

    def rc(n=1, area=(0, 10, 0, 20), hold=2, max_hold=6, fed=0, flush=1, state=st, counts=cnt, bgr=buf):
        return lib.vse_frame_hold_bounded(ctx.handle, C.c_void_p(bgr.data_ptr()) if bgr is not None else None, n, 10, 20, 60, 600, *area, 128,
                                          hold, max_hold, C.c_void_p(state.data_ptr()) if state is not None else None, fed, flush,
                                          C.c_void_p(counts.data_ptr()) if counts is not None else None, ctx.stream())
    for area in [(0, 2, 0, 10), (0, 10, 5, 7), (-1, 5, 0, 10), (0, 11, 0, 10), (0, 10, 0, 21), (4, 4, 0, 10)]:
        assert rc(area=area) == -1, area
        assert "area" in lib.vse_last_error().decode()
    for hold, max_hold in ((0, 6), (-1, 6), (33, 40), (3, 2), (2, 1), (2, 4001), (1, 0)):
        assert rc(hold=hold, max_hold=max_hold) == -1, (hold, max_hold)
        assert "hold" in lib.vse_last_error().decode()
    assert rc(n=-1) == -1 and rc(fed=-1) == -1 and rc(state=None) == -1 and rc(bgr=None) == -1 and rc(counts=None) == -1
    assert (cnt.cpu().numpy() == -7).all() and int(st.count_nonzero()) == 0      # nothing was enqueued
    assert rc(n=0, flush=0) == 0 and (cnt.cpu().numpy() == -7).all()             # nothing to do is not an error
    assert rc(flush=0, counts=None) == 0                                         # no row comes out of one frame without a flush
    assert rc() == 0 and cnt.cpu().numpy()[:1].tolist() == [[0, 0, 0]]           # the same call with good arguments runs
    assert (cnt.cpu().numpy()[1:] == -7).all()
    sb = lib.vse_frame_hold_bounded_state_bytes
    assert sb(2, 100, 2) == 0 and sb(100, 2, 2) == 0 and sb(10, 100, 0) == 0 and sb(10, 100, 4001) == 0
    assert sb(3, 3, 1) > 0 and sb(17, 130, 4000) > sb(17, 130, 40) > sb(3, 3, 40) > 0 and sb(3, 3, 40) % 8 == 0
    with pytest.raises(engine.VseError):
        ctx.frame_hold_bounded_state(10, 100, 4001)


@pytest.mark.parametrize("staged", [False, True])
def test_bounded_selector_on_engine_finds_the_static_clip_truth(ctx, staged):
    from test_frame_hold_bounded import AREA, BAND, MAX_HOLD, TRUE, static_clip
    from vse_amd import frame_select, staging
    frames, _truth = static_clip("busy")
    sel = frame_select.HoldFrameSelector(frame_select.EngineBoundedHoldCounter(ctx), hold_frames=3, max_hold_frames=MAX_HOLD, batch=40)
    got = sel.run(list(frames), BAND, 25.0, uploader=staging.Uploader(ctx.tdev) if staged else None)
    assert [(s, e) for s, e, _r in got] == TRUE
    assert np.array_equal(sel.counts, ref_counts(frames, AREA, 128, 3, MAX_HOLD))
    lost = frame_select.HoldFrameSelector(frame_select.EngineHoldCounter(ctx), hold_frames=3, batch=40).run(list(frames), BAND, 25.0)
    assert (41, 80) in [(s, e) for s, e, _r in lost]                               # without the bound two subtitles are one
