"""vse_frame_cells_hold_bounded_masks and vse_frame_masks_replay_hold_bounded on the MI355X.  The masks entry: totals, cell counts and
state are, bit for bit, vse_frame_cells_hold_bounded's; the buffer read back is vse_frame_cells_masks' buffer and the numpy layout
(tests/frame_masks_ref.py): the EDGE words, whatever the bounds; no slot beside the call's is touched, the flush step takes none, and a
state passes between the two entries.  The replay: the rows of a rectangle are, integer for integer, vse_frame_hold_bounded's on the same
device frames and the numpy reference's (tests/frame_masks_hold_bounded_ref.py), whole or in pieces of 1, 63, 64 and 65 slots, without and
with a flush; the state it leaves is vse_frame_hold_bounded's, byte for byte, and vse_frame_hold_bounded continues the clip from it; the
buffer is only read; refused arguments touch nothing.  The regions and rectangles are tests/test_gpu_frame_masks_hold.py's; the clips are
tests/test_gpu_frame_hold_bounded.py's squares, 150 frames, so that a call spans more than two chunks of 64 and the ring of max_hold + 64
pending rows wraps at max_hold 5 and 30."""
import ctypes as C

import numpy as np
import pytest

import frame_masks_hold_bounded_ref as FMB
import frame_masks_ref as FM
from frame_change_ref import edge_mask
from frame_hold_bounded_ref import counts as bounded_counts, emitted
from test_gpu_frame_cells_counts import AREAS, FRAME_H, FRAME_W, P, T8, words
from test_gpu_frame_cells_multi import device_view
from test_gpu_frame_hold_bounded import GUARD, run_lengths, square_frames
from test_gpu_frame_masks import A5, RECTS, THS, dirty_buffer, host_words, run_masks

pytestmark = pytest.mark.gpu

N = 150                   # frames of a clip: more than two chunks of 64
BOUNDS = [(1, 1), (3, 30), (8, 70)]                               # (hold, max_hold) of the masks entry
RBOUNDS = [(1, 1), (2, 5), (3, 30), (8, 70), (3, 4000)]           # ... and of the replay; the first and the last are the degenerate ones
REGION = (0, 40, 0, 200)
RTHS = (32, 96, 160)
FURTHER = 40              # the frames vse_frame_hold_bounded continues with from the replayed state
_CLIPS, _WORDS, _ROWS, _KEPT, _DEV = {}, {}, {}, {}, {}


def clip_of(bounds):
    if bounds not in _CLIPS:
        hold, max_hold = bounds
        f = square_frames(N, FRAME_H, FRAME_W, hold, max_hold, seed=9000 + 100 * hold + max_hold)
        f.setflags(write=False)
        _CLIPS[bounds] = f
    return _CLIPS[bounds]


def dev_of(ctx, bounds):
    if bounds not in _DEV:
        _DEV[bounds] = device_view(ctx, clip_of(bounds), padded=True)
    return _DEV[bounds]


def want_words(bounds, area, ths, a, b):
    """numpy: the mask words of frames a .. b - 1 of the clip (a frame's words depend on that frame alone: computed once per clip)."""
    key = (bounds, area, tuple(ths))
    if key not in _WORDS:
        _WORDS[key] = FM.mask_words(clip_of(bounds), area, ths)
        _WORDS[key].setflags(write=False)
    return _WORDS[key][a:b]


def run_bounded(ctx, dev, area, ths, bounds, calls, masks=None, slot0=0, state=None):
    """calls: [(first, last, fed, flush)] through one state; with `masks` through vse_frame_cells_hold_bounded_masks, the frames landing
    in consecutive slots from slot0 on, without through vse_frame_cells_hold_bounded -> host totals, the calls' host cell counts, state."""
    y0, y1, x0, x1 = area
    hold, max_hold = bounds
    state = state or ctx.frame_cells_hold_bounded_state(y1 - y0, x1 - x0, len(ths), max_hold)
    counts = []
    for a, b, fed, flush in calls:
        if masks is None:
            _t, c = ctx.frame_cells_hold_bounded(dev[a:b], area, ths, hold, max_hold, P, state, fed, flush=flush, want_counts=True)
        else:
            _t, c = ctx.frame_cells_hold_bounded_masks(dev[a:b], area, ths, hold, max_hold, P, state, masks, slot0, fed, flush=flush,
                                                       want_counts=True)
            slot0 += b - a
        counts.append(c.cpu().numpy())
    return state.totals.cpu().numpy(), np.concatenate(counts, 1), state


# ---- the reference alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", RBOUNDS)
def test_reference_rows_cover_the_decisions(bounds):
    """The precondition of the comparisons below, on the reference alone: a row with e, a and v each nonzero, a run that ends in range
    and one that ends too long.  Not for the two degenerate bounds: with (1, 1) only single-frame runs count, and max_hold >= the clip
    leaves no run too long."""
    hold, max_hold = bounds
    for rect in RECTS["whole"]:
        if rect[3] - rect[2] - 2 < 8 or bounds in ((1, 1), (3, 4000)):
            continue
        for th in RTHS:
            want = want_rows(bounds, rect, th)
            assert want.shape == (N, 3) and (want > 0).all(1).any(), (rect, th)
            e = edge_mask(clip_of(bounds), rect, th)
            length = run_lengths(e)
            ends = e[:-1] & ~e[1:]                                 # a run that ends inside the clip
            assert (ends & (length[:-1] >= hold) & (length[:-1] <= max_hold)).any(), (rect, th)
            assert (ends & (length[:-1] > max_hold)).any(), (rect, th)


# ---- the masks entry: geometry, frame counts, numbers of thresholds, bounds --------------------------------------------------------------
@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("nt", [1, 3, 8])
@pytest.mark.parametrize("name", list(AREAS))
def test_totals_counts_state_and_masks_match_the_existing_entries_and_numpy(ctx, name, nt, bounds):
    area, ths, dev = AREAS[name], THS[nt], dev_of(ctx, bounds)
    for n in (1, 64, 65, N):
        calls = [(0, n, 0, True)]
        masks = dirty_buffer(ctx, area, nt, n + 3)
        totals, counts, state = run_bounded(ctx, dev, area, ths, bounds, calls, masks, slot0=1)
        bt, bc, bs = run_bounded(ctx, dev, area, ths, bounds, calls)
        assert totals.dtype == np.int32 and np.array_equal(totals, bt) and np.array_equal(counts, bc) and counts.shape[1] == n, n
        assert words(state) == words(bs), n
        got = host_words(masks)
        assert np.array_equal(got[1:1 + n], want_words(bounds, area, ths, 0, n)), n               # the edge words, whatever the bounds
        assert (got[0] == A5).all() and (got[1 + n:] == A5).all(), n                              # no slot beside the call's
        change = dirty_buffer(ctx, area, nt, n + 3)
        run_masks(ctx, dev, area, ths, [(0, n, True, True)], change, slot0=1)
        assert np.array_equal(got, host_words(change)), n                                         # vse_frame_cells_masks' buffer


def test_the_bounded_counts_are_busy_and_differ_with_the_bounds(ctx):
    """What the equality above compares is not empty: the cell counts of the 17 x 129 region have all three columns nonzero, and other
    bounds give other totals."""
    area = AREAS["17x129"]
    seen = []
    for bounds in BOUNDS[1:]:
        totals, counts, _s = run_bounded(ctx, dev_of(ctx, BOUNDS[1]), area, T8, bounds, [(0, N, 0, True)])
        assert (counts.sum((2, 3)) > 0).all(2).any() and totals.any()
        seen.append(totals)
    assert not np.array_equal(seen[0], seen[1])


# ---- call sequences ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", BOUNDS)
@pytest.mark.parametrize("name", ["9x65", "17x129"])
def test_batch_splits_and_a_later_slot_give_the_buffer_of_one_call(ctx, name, bounds):
    area, dev = AREAS[name], dev_of(ctx, bounds)
    whole = dirty_buffer(ctx, area, 8, N + 5)
    wt, wc, ws = run_bounded(ctx, dev, area, T8, bounds, [(0, N, 0, True)], whole)
    want = host_words(whole)
    assert np.array_equal(want[:N], want_words(bounds, area, T8, 0, N)) and (want[N:] == A5).all()
    for calls in ([(0, 1, 0, False), (1, N, 1, True)], [(0, 64, 0, False), (64, 129, 64, False), (129, N, 129, True)],
                  [(0, 65, 0, False), (65, N, 65, False), (N, N, N, True)]):
        masks = dirty_buffer(ctx, area, 8, N + 5)
        totals, counts, state = run_bounded(ctx, dev, area, T8, bounds, calls, masks)
        assert np.array_equal(host_words(masks), want) and np.array_equal(totals, wt) and np.array_equal(counts, wc)
        assert words(state) == words(ws)
    masks = dirty_buffer(ctx, area, 8, N + 5)
    totals, counts, state = run_bounded(ctx, dev, area, T8, bounds, [(0, 30, 0, False), (30, N, 30, True)], masks, slot0=5)
    got = host_words(masks)
    assert np.array_equal(got[5:N + 5], want[:N]) and (got[:5] == A5).all() and np.array_equal(totals, wt) and words(state) == words(ws)


def test_no_frames_with_flush_writes_no_slot(ctx):
    area, bounds = AREAS["17x129"], (3, 30)
    dev = dev_of(ctx, bounds)
    masks = dirty_buffer(ctx, area, 8, 80)
    open_totals, _c, state = run_bounded(ctx, dev, area, T8, bounds, [(0, 77, 0, False)], masks)
    before = host_words(masks).copy()
    totals, _c, state = run_bounded(ctx, dev, area, T8, bounds, [(77, 77, 77, True)], masks, slot0=77, state=state)
    assert np.array_equal(host_words(masks), before) and (before[77:] == A5).all()                # the flush step took no slot
    bt, _c, bs = run_bounded(ctx, dev, area, T8, bounds, [(0, 77, 0, False), (77, 77, 77, True)])
    assert np.array_equal(totals, bt) and words(state) == words(bs) and not np.array_equal(totals, open_totals)
    # n == 0 with a flush may pass no buffer at all
    from vse_amd import engine
    lib = engine.load_library()
    _t, _c, state = run_bounded(ctx, dev, area, T8, bounds, [(0, 77, 0, False)])
    y0, y1, x0, x1 = area
    rc = lib.vse_frame_cells_hold_bounded_masks(ctx.handle, None, 0, FRAME_H, FRAME_W, 3 * FRAME_W, 3 * FRAME_W * FRAME_H, y0, y1, x0, x1,
                                                (C.c_int * 8)(*T8), 8, 3, 30, P.min_edges, P.ratio_num, P.ratio_den, P.min_frames, P.max_frames,
                                                C.c_void_p(state.words.data_ptr()), 77, 1, C.c_void_p(state.totals.data_ptr()), None, None, 1, 0,
                                                ctx.stream())
    assert rc == 0, lib.vse_last_error().decode()
    assert np.array_equal(state.totals.cpu().numpy(), bt) and words(state) == words(bs)


def test_a_state_passes_between_the_two_entries(ctx):
    area, bounds = AREAS["17x129"], (3, 30)
    dev = dev_of(ctx, bounds)
    alone, alone_counts, alone_state = run_bounded(ctx, dev, area, T8, bounds, [(0, N, 0, True)])
    # begun by vse_frame_cells_hold_bounded, continued here
    _t, head, state = run_bounded(ctx, dev, area, T8, bounds, [(0, 70, 0, False)])
    masks = dirty_buffer(ctx, area, 8, N)
    totals, tail, state = run_bounded(ctx, dev, area, T8, bounds, [(70, N, 70, True)], masks, slot0=70, state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state) and np.array_equal(np.concatenate([head, tail], 1), alone_counts)
    assert np.array_equal(host_words(masks)[70:], want_words(bounds, area, T8, 70, N)) and (host_words(masks)[:70] == A5).all()
    # and the other way round
    _t, head, state = run_bounded(ctx, dev, area, T8, bounds, [(0, 70, 0, False)], dirty_buffer(ctx, area, 8, 70))
    totals, tail, state = run_bounded(ctx, dev, area, T8, bounds, [(70, N, 70, True)], state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state) and np.array_equal(np.concatenate([head, tail], 1), alone_counts)


# ---- replay ------------------------------------------------------------------------------------------------------------------------------
def want_rows(bounds, rect, th, n=None):
    """numpy: vse_frame_hold_bounded's rows of the first n frames (None: all) of the clip on the rectangle, as a whole clip."""
    key = (bounds, rect, th, n)
    if key not in _ROWS:
        _ROWS[key] = bounded_counts(clip_of(bounds)[:n], rect, th, *bounds)          # (the region is the whole frame: rect = area)
        _ROWS[key].setflags(write=False)
    return _ROWS[key]


def kept(ctx, bounds):
    """(device frames, masks of all of them over the region at RTHS, the buffer's host words), made once per clip by the masks entry."""
    import torch
    if bounds not in _KEPT:
        frames = torch.from_numpy(clip_of(bounds).copy()).to(ctx.tdev)
        masks = dirty_buffer(ctx, REGION, len(RTHS), N + 2)
        state = ctx.frame_cells_hold_bounded_state(40, 200, len(RTHS), 30)
        ctx.frame_cells_hold_bounded_masks(frames[:64], REGION, RTHS, 3, 30, P, state, masks, 0, 0)
        ctx.frame_cells_hold_bounded_masks(frames[64:], REGION, RTHS, 3, 30, P, state, masks, 64, 64, flush=True)
        _KEPT[bounds] = (frames, masks, host_words(masks).copy())
    return _KEPT[bounds]


def replay_call(ctx, masks, q, f0, f1, rect, bounds, state, fed, flush):
    """One vse_frame_masks_replay_hold_bounded call -> host int32 rows; checks the rows it must not write."""
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    hold, max_hold = bounds
    n = f1 - f0
    out = torch.full((n + max_hold + GUARD, 3), -7, dtype=torch.int32, device=ctx.tdev)
    rc = lib.vse_frame_masks_replay_hold_bounded(ctx.handle, C.c_void_p(masks.words.data_ptr()), masks.area_h, masks.area_w, masks.nt,
                                                 masks.cap, q, f0, f1, *rect, hold, max_hold, C.c_void_p(state.data_ptr()), fed, int(flush),
                                                 C.c_void_p(out.data_ptr()), ctx.stream())
    assert rc == 0, lib.vse_last_error().decode()
    lo, hi = emitted(fed, n, max_hold, flush)
    out = out.cpu().numpy()
    assert (out[hi - lo:] == -7).all(), "rows behind the emitted ones were written"
    return out[:hi - lo]


def bounded_rows(ctx, frames, rect, th, bounds, state, a, b, fed, flush):
    return ctx.frame_hold_bounded(frames[a:b], rect, th, *bounds, state, fed, flush=flush).cpu().numpy()


def in_pieces(ctx, masks, q, n, rect, bounds, state, piece):
    """Slots 0 .. n - 1 in pieces of `piece` slots, fed advancing, no flush -> the rows of all calls."""
    out = [replay_call(ctx, masks, q, a, min(n, a + piece), rect, bounds, state, a, False) for a in range(0, n, piece)]
    return np.concatenate(out)


@pytest.mark.parametrize("rect", RECTS["whole"])
@pytest.mark.parametrize("bounds", RBOUNDS)
def test_replay_is_frame_hold_bounded_on_the_rectangle_and_hands_its_state_over(ctx, bounds, rect):
    import torch
    hold, max_hold = bounds
    frames, masks, host = kept(ctx, bounds)
    cut = N - FURTHER
    before = masks.words.cpu().numpy().tobytes()
    assert np.array_equal(host[:N], want_words(bounds, REGION, RTHS, 0, N)) and (host[N:] == A5).all()
    h, w = rect[1] - rect[0], rect[3] - rect[2]

    def fresh_state():
        return ctx.frame_hold_bounded_state(h, w, max_hold)

    def dirty_state():                            # fed == 0 ignores the state's content
        return torch.full_like(fresh_state(), 0xA5)

    def same(a, b):
        return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()

    for q, th in enumerate(RTHS):
        want = want_rows(bounds, rect, th)
        # with a flush: every row of the clip, and the state that entry leaves
        rs, hs = fresh_state(), fresh_state()
        flushed = replay_call(ctx, masks, q, 0, N, rect, bounds, rs, 0, True)
        assert np.array_equal(flushed, bounded_rows(ctx, frames, rect, th, bounds, hs, 0, N, 0, True)) and same(rs, hs), (q, th)
        assert np.array_equal(flushed, want) and np.array_equal(flushed, FMB.replay_hold_bounded(host, 40, 200, q, 0, N, rect, *bounds)[0])
        # without: the rows trail by max_hold, and both states, zero-filled first, are equal byte for byte
        rs, hs = fresh_state(), fresh_state()
        rows = replay_call(ctx, masks, q, 0, N, rect, bounds, rs, 0, False)
        assert np.array_equal(rows, bounded_rows(ctx, frames, rect, th, bounds, hs, 0, N, 0, False)) and len(rows) == max(0, N - max_hold)
        assert np.array_equal(rows, want[:len(rows)]) and same(rs, hs)
        # in pieces, fed advancing: the rows and the state of one call; then the pending rows alone
        for piece in ((1, 63, 64, 65) if q == 0 else (63, 65)):
            ps = dirty_state()
            assert np.array_equal(in_pieces(ctx, masks, q, N, rect, bounds, ps, piece), rows), piece
            assert same(ps, rs), piece
            drained = replay_call(ctx, masks, q, N, N, rect, bounds, ps, N, True)
            assert np.array_equal(np.concatenate([rows, drained]), flushed), piece
        # vse_frame_hold_bounded carries on from the replayed state: the uninterrupted run of the first `cut` frames, FURTHER more and
        # a flush; and the state after those frames is that of the uninterrupted run
        cs, us = dirty_state(), fresh_state()
        head = replay_call(ctx, masks, q, 0, cut, rect, bounds, cs, 0, False)
        tail = bounded_rows(ctx, frames, rect, th, bounds, cs, cut, N, cut, True)
        assert np.array_equal(np.concatenate([head, tail]), want), (q, th)
        bounded_rows(ctx, frames, rect, th, bounds, us, 0, N, 0, True)
        assert same(cs, us)
    assert masks.words.cpu().numpy().tobytes() == before                                          # the buffer is only read


@pytest.mark.parametrize("rect", RECTS["whole"][:3])
def test_max_hold_beyond_the_clip_gives_the_unbounded_replays_rows(ctx, rect):
    bounds = (3, 4000)
    _frames, masks, _host = kept(ctx, bounds)
    h, w = rect[1] - rect[0], rect[3] - rect[2]
    for q in range(len(RTHS)):
        got = replay_call(ctx, masks, q, 0, N, rect, bounds, ctx.frame_hold_bounded_state(h, w, 4000), 0, True)
        held = ctx.frame_masks_replay_hold(masks, q, 0, N, rect, 3, ctx.frame_hold_state(h, w, 3), 0, flush=True).cpu().numpy()
        assert np.array_equal(got, held) and len(got) == N and got[:, 0].max() > 0


def test_the_context_method_and_the_selectors_callable(ctx):
    """Context.frame_masks_replay_hold_bounded sizes d_counts itself (n + max_hold rows), and EngineCellsHoldBoundedMasks.replay sets an
    EngineBoundedHoldCounter up to continue the clip."""
    from vse_amd import frame_select
    bounds, rect, th = (3, 30), RECTS["whole"][2], RTHS[1]
    frames, masks, _host = kept(ctx, bounds)
    want = want_rows(bounds, rect, th)
    h, w = rect[1] - rect[0], rect[3] - rect[2]
    got = ctx.frame_masks_replay_hold_bounded(masks, 1, 0, N, rect, 3, 30, ctx.frame_hold_bounded_state(h, w, 30), 0, flush=True)
    assert np.array_equal(got.cpu().numpy(), want)
    cells, counter = frame_select.EngineCellsHoldBoundedMasks(ctx), frame_select.EngineBoundedHoldCounter(ctx)
    cut = N - FURTHER
    cells(frames[:cut], REGION, P, True, False, RTHS, cut, 3, 30)
    head = cells.replay(REGION, 1, rect, counter, 3, 30, False).cpu().numpy()
    area = (0, h, rect[2], rect[3])
    tail = counter(frames[cut:, rect[0]:rect[1]].contiguous(), area, th, 3, 30, cut, True).cpu().numpy()
    assert np.array_equal(np.concatenate([head, tail]), want) and counter.fed == N
    with pytest.raises(ValueError, match="no masks"):
        frame_select.EngineCellsHoldBoundedMasks(ctx).replay(REGION, 0, rect, counter, 3, 30, False)


def test_rectangle_widths_cover_the_word_boundaries():
    widths = {r[3] - r[2] - 2 for r in RECTS["whole"]}
    assert {1, 63, 64, 65, 129} <= widths and {r[2] % 64 for r in RECTS["whole"]} == {0, 1, 63}
    assert any(r[0] % 8 for r in RECTS["whole"]) and any((r[1] - r[0] - 2) % 8 for r in RECTS["whole"])
    assert N > 2 * 64 and N > 5 + 64 and N > 30 + 64               # more than two chunks; the rings of max_hold 5 and 30 wrap


# ---- refused arguments -------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.zeros(1 << 15, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    msk = torch.full((4096,), 0xA5, dtype=torch.uint8, device=ctx.tdev)   # a 9 x 19 region: one cell, 64 bytes per slot and threshold
    good = dict(n=1, y0=1, y1=10, x0=1, x1=20, ths=(32, 128), nt=None, hold=3, max_hold=5, fed=0, state=st.data_ptr(), totals=tot.data_ptr(),
                masks=msk.data_ptr(), frames=buf.data_ptr(), cap=4, slot0=0)

    def call(**kw):
        a = {**good, **kw}
        ths = a["ths"]
        nt = len(ths) if a["nt"] is None else a["nt"]
        arr = (C.c_int * max(1, len(ths)))(*ths) if ths is not None else None
        return lib.vse_frame_cells_hold_bounded_masks(ctx.handle, C.c_void_p(a["frames"]), a["n"], 10, 20, 60, 600, a["y0"], a["y1"], a["x0"],
                                                      a["x1"], arr, nt, a["hold"], a["max_hold"], 16, 1, 2, 2, 5, C.c_void_p(a["state"]),
                                                      a["fed"], 1, C.c_void_p(a["totals"]), None, C.c_void_p(a["masks"]), a["cap"], a["slot0"],
                                                      ctx.stream())
    bad = [dict(ths=(), nt=0), dict(ths=(1, 2, 3, 4, 5, 6, 7, 8, 9)), dict(ths=None, nt=2), dict(ths=(128, 32)), dict(ths=(0, 32)),
           dict(ths=(32, 256)),                                                                    # the thresholds
           dict(y1=3), dict(x0=5, x1=7), dict(y0=4, y1=4),                                         # below 3 x 3
           dict(y0=-1, y1=5), dict(y1=11), dict(x1=21),                                            # outside the 10 x 20 frame
           dict(n=-1), dict(frames=None), dict(state=None), dict(totals=None), dict(masks=None), dict(state=st.data_ptr() + 4),
           dict(masks=msk.data_ptr() + 4),
           dict(hold=0), dict(hold=33, max_hold=40), dict(fed=-1), dict(max_hold=2), dict(max_hold=4001),     # vse_frame_cells_hold_bounded's
           dict(slot0=-1), dict(slot0=4), dict(n=2, slot0=3), dict(cap=0), dict(n=0, slot0=5)]     # the slots: no wrap
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells_hold_bounded_masks" in lib.vse_last_error().decode()
    hst = torch.full((8192,), 0x5A, dtype=torch.uint8, device=ctx.tdev)
    cnt = torch.full((64,), -9, dtype=torch.int32, device=ctx.tdev)

    def replay(area_h=9, area_w=19, nt=2, cap=4, q=0, f0=0, f1=1, rect=(0, 9, 0, 19), hold=3, max_hold=5, fed=0, flush=1, src=msk.data_ptr(),
               counts=cnt.data_ptr(), dst=hst.data_ptr()):
        return lib.vse_frame_masks_replay_hold_bounded(ctx.handle, C.c_void_p(src), area_h, area_w, nt, cap, q, f0, f1, *rect, hold, max_hold,
                                                       C.c_void_p(dst), fed, flush, C.c_void_p(counts), ctx.stream())
    for kw in [dict(q=-1), dict(q=2), dict(nt=8, q=8), dict(nt=0), dict(nt=9, q=1), dict(area_h=2), dict(area_w=2), dict(src=None),
               dict(dst=None), dict(counts=None), dict(dst=hst.data_ptr() + 4), dict(src=msk.data_ptr() + 4), dict(counts=cnt.data_ptr() + 2),
               dict(f0=-1), dict(f0=1, f1=1, flush=0), dict(f0=2, f1=1), dict(f1=5), dict(f0=4, f1=5), dict(f0=5, f1=5),
               dict(hold=0), dict(hold=33, max_hold=40), dict(fed=-1),
               dict(max_hold=2), dict(max_hold=4001), dict(hold=1, max_hold=0),
               dict(rect=(0, 2, 0, 19)), dict(rect=(0, 9, 3, 5)), dict(rect=(-1, 9, 0, 19)), dict(rect=(0, 10, 0, 19)),
               dict(rect=(0, 9, 0, 20)), dict(rect=(0, 9, -1, 19)), dict(rect=(5, 5, 0, 19))]:
        assert replay(**kw) == -1, kw
        assert "vse_frame_masks_replay_hold_bounded" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert set(tot.cpu().tolist()) == {-7} and set(cnt.cpu().tolist()) == {-9} and int(st.sum()) == 0      # nothing was enqueued
    assert set(hst.cpu().tolist()) == {0x5A} and set(msk.cpu().tolist()) == {0xA5}
    # accepted: two frames into slots 1 and 2 (zero frames: no edge anywhere), their replay, and an empty slot range with a flush
    assert call(n=2, slot0=1) == 0 and replay(f0=1, f1=3) == 0 and replay(f0=3, f1=3, fed=2) == 0
    torch.cuda.synchronize()
    got = msk.cpu().numpy()
    assert set(got[:128].tolist()) == {0xA5} and not got[128:384].any() and set(got[384:].tolist()) == {0xA5}      # slots 1 and 2, zeros
    assert tot.cpu().tolist()[:8] == [0] * 8 and tot.cpu().tolist()[8] == -7                      # one cell, two thresholds, fresh
    assert cnt.cpu().tolist()[:6] == [0] * 6 and cnt.cpu().tolist()[12] == -9                     # two rows; the drain found nothing pending
    n = lib.vse_frame_hold_bounded_state_bytes(9, 19, 5)
    assert not hst.cpu().numpy()[:n].any() and set(hst.cpu().numpy()[n:].tolist()) == {0x5A}      # the state of the rectangle, no more
