"""vse_frame_cells_hold_masks and vse_frame_masks_replay_hold on the MI355X.  The masks entry: totals and state are, bit for bit,
vse_frame_cells_hold's and the numpy cells' (tests/area_cells_hold_ref.py); the buffer read back is vse_frame_cells_masks' buffer and
the numpy layout (tests/frame_masks_ref.py): the EDGE words, whatever the hold; no slot beside the call's is touched, a flush's steps
take none, and a state passes between the two entries.  The replay: the rows of a rectangle are, integer for integer, vse_frame_hold's
on the same device frames and the numpy reference's (tests/frame_masks_hold_ref.py), whole or in pieces, without and with a flush; the
state it leaves is vse_frame_hold's, byte for byte, and vse_frame_hold continues the clip from it; the buffer is only read; refused
arguments touch nothing.  The regions and frame counts are those of tests/test_gpu_frame_cells_counts.py, the rectangles those of
tests/test_gpu_frame_masks.py (rx0 % 64 in 0, 1, 63; widths 1, 63, 64, 65, 129; row offsets off the 8-row grid)."""
import ctypes as C

import numpy as np
import pytest

import frame_masks_hold_ref as FMH
from area_cells_hold_ref import clip_totals_hold
from frame_hold_ref import counts as hold_counts, emitted
from test_gpu_frame_cells_counts import AREAS, FRAME_H, FRAME_W, FRAMES, P, T8, words
from test_gpu_frame_cells_multi import calib_frames, device_view
from test_gpu_frame_hold import GUARD, persistent_frames
from test_gpu_frame_masks import A5, RECTS, THS, dirty_buffer, host_words, run_masks, want_words

pytestmark = pytest.mark.gpu

HOLDS = (1, 3, 8)


@pytest.fixture(scope="module")
def clip():
    f = calib_frames(FRAMES, FRAME_H, FRAME_W, seed=71)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def dev(ctx, clip):
    return device_view(ctx, clip, padded=True)


_WANT = {}


def want_totals(clip, area, ths, hold, a, b, flush=True):
    key = (area, tuple(ths), hold, a, b, flush)
    if key not in _WANT:
        _WANT[key] = np.stack([clip_totals_hold(clip[a:b], area, P._replace(edge_thresh=th), hold, flush) for th in ths])
    return _WANT[key]


def run_hold(ctx, dev, area, ths, hold, calls, masks=None, slot0=0, state=None):
    """calls: [(first, last, fed, flush)] through one state; with `masks` through vse_frame_cells_hold_masks, the frames landing in
    consecutive slots from slot0 on, without through vse_frame_cells_hold -> host totals, the state."""
    y0, y1, x0, x1 = area
    state = state or ctx.frame_cells_hold_state(y1 - y0, x1 - x0, len(ths), hold)
    for a, b, fed, flush in calls:
        if masks is None:
            ctx.frame_cells_hold(dev[a:b], area, ths, hold, P, state, fed, flush=flush)
        else:
            ctx.frame_cells_hold_masks(dev[a:b], area, ths, hold, P, state, masks, slot0, fed, flush=flush)
            slot0 += b - a
    return state.totals.cpu().numpy(), state


# ---- the masks entry: geometry, frame counts, numbers of thresholds, holds -------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("nt", [1, 3, 8])
@pytest.mark.parametrize("name", list(AREAS))
def test_totals_state_and_masks_match_the_existing_entries_and_numpy(ctx, clip, dev, name, nt, hold):
    area, ths = AREAS[name], THS[nt]
    for n in (1, 63, 64, 65, 130):
        calls = [(0, n, 0, True)]
        masks = dirty_buffer(ctx, area, nt, n + 3)
        totals, state = run_hold(ctx, dev, area, ths, hold, calls, masks, slot0=1)
        ht, hs = run_hold(ctx, dev, area, ths, hold, calls)
        assert totals.dtype == np.int32 and np.array_equal(totals, ht) and words(state) == words(hs), n
        if n in (1, 65) or nt == 3:               # (the plain-Python automaton of every cell and threshold: the costly reference)
            assert np.array_equal(totals, want_totals(clip, area, ths, hold, 0, n)), n
        got = host_words(masks)
        assert np.array_equal(got[1:1 + n], want_words(clip, area, ths, 0, n)), n                 # the edge words, not the held ones
        assert (got[0] == A5).all() and (got[1 + n:] == A5).all(), n                              # no slot beside the call's
        change = dirty_buffer(ctx, area, nt, n + 3)
        run_masks(ctx, dev, area, ths, [(0, n, True, True)], change, slot0=1)
        assert np.array_equal(got, host_words(change)), n                                         # vse_frame_cells_masks' buffer


def test_the_held_totals_differ_from_the_change_totals(clip):
    """The precondition of the comparison above, on the reference alone: a hold changes the totals and the masks, so neither equal
    totals nor a buffer of edge words are an accident."""
    from frame_change_ref import edge_mask
    from frame_hold_ref import held_masks
    area = AREAS["17x129"]
    for hold in HOLDS[1:]:
        assert not np.array_equal(want_totals(clip, area, THS[3], hold, 0, 130), want_totals(clip, area, THS[3], 1, 0, 130))
        for th in (1, 60, 96):
            e = edge_mask(clip[:65], area, th)
            assert 0 < held_masks(e, hold).sum() < e.sum(), (hold, th)


# ---- call sequences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [3, 8])
@pytest.mark.parametrize("name", ["9x65", "17x129"])
def test_batch_splits_and_a_later_slot_give_the_buffer_of_one_call(ctx, clip, dev, name, hold):
    area = AREAS[name]
    whole = dirty_buffer(ctx, area, 8, 70)
    wt, ws = run_hold(ctx, dev, area, T8, hold, [(0, 65, 0, True)], whole)
    want = host_words(whole)
    assert np.array_equal(want[:65], want_words(clip, area, T8, 0, 65)) and (want[65:] == A5).all()
    for calls in ([(0, 1, 0, False), (1, 65, 1, True)], [(0, 64, 0, False), (64, 65, 64, True)]):
        masks = dirty_buffer(ctx, area, 8, 70)
        totals, state = run_hold(ctx, dev, area, T8, hold, calls, masks)
        assert np.array_equal(host_words(masks), want) and np.array_equal(totals, wt) and words(state) == words(ws)
    masks = dirty_buffer(ctx, area, 8, 70)
    totals, state = run_hold(ctx, dev, area, T8, hold, [(0, 30, 0, False), (30, 65, 30, True)], masks, slot0=5)
    got = host_words(masks)
    assert np.array_equal(got[5:70], want[:65]) and (got[:5] == A5).all() and np.array_equal(totals, wt) and words(state) == words(ws)


def test_no_frames_with_flush_writes_no_slot(ctx, clip, dev):
    area, hold = AREAS["17x129"], 8
    masks = dirty_buffer(ctx, area, 8, 40)
    open_totals, state = run_hold(ctx, dev, area, T8, hold, [(0, 37, 0, False)], masks)
    before = host_words(masks).copy()
    totals, state = run_hold(ctx, dev, area, T8, hold, [(37, 37, 37, True)], masks, slot0=37, state=state)
    assert np.array_equal(host_words(masks), before) and (before[37:] == A5).all()                # the flush's seven steps took no slot
    ht, hs = run_hold(ctx, dev, area, T8, hold, [(0, 37, 0, False), (37, 37, 37, True)])
    assert np.array_equal(totals, ht) and words(state) == words(hs) and not np.array_equal(totals, open_totals)


def test_a_state_passes_between_the_two_entries(ctx, clip, dev):
    area, hold = AREAS["17x129"], 3
    alone, alone_state = run_hold(ctx, dev, area, T8, hold, [(0, 130, 0, True)])
    # begun by vse_frame_cells_hold, continued here
    _t, state = run_hold(ctx, dev, area, T8, hold, [(0, 70, 0, False)])
    masks = dirty_buffer(ctx, area, 8, 130)
    totals, state = run_hold(ctx, dev, area, T8, hold, [(70, 130, 70, True)], masks, slot0=70, state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state)
    assert np.array_equal(host_words(masks)[70:], want_words(clip, area, T8, 70, 130)) and (host_words(masks)[:70] == A5).all()
    # and the other way round
    _t, state = run_hold(ctx, dev, area, T8, hold, [(0, 70, 0, False)], dirty_buffer(ctx, area, 8, 70))
    totals, state = run_hold(ctx, dev, area, T8, hold, [(70, 130, 70, True)], state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state)


# ---- replay ---------------------------------------------------------------------------------------------------------------------------
REGION = (0, 40, 0, 200)
RTHS = (32, 48, 64)
RHOLDS = (1, 2, 3, 8, 32)
FURTHER = 40              # the frames vse_frame_hold continues with from the replayed state
_CLIPS, _ROWS, _KEPT = {}, {}, {}


def hold_clip(hold):
    if hold not in _CLIPS:
        f = persistent_frames(2 * hold + 70, 40, 200, hold, seed=4000 + hold)
        f.setflags(write=False)
        _CLIPS[hold] = f
    return _CLIPS[hold]


def want_rows(hold, rect, th, n=None):
    """numpy: vse_frame_hold's rows of the first n frames (None: all) of hold_clip(hold) on the rectangle, as a whole clip."""
    key = (hold, rect, th, n)
    if key not in _ROWS:
        _ROWS[key] = hold_counts(hold_clip(hold)[:n], rect, th, hold)                 # (the region is the whole frame: rect = area)
        _ROWS[key].setflags(write=False)
    return _ROWS[key]


def kept(ctx, hold):
    """(device frames, masks of all of them over the region at RTHS, the buffer's host words), made once per hold by the masks entry."""
    import torch
    if hold not in _KEPT:
        frames = torch.from_numpy(hold_clip(hold).copy()).to(ctx.tdev)
        n = len(frames)
        masks = dirty_buffer(ctx, REGION, len(RTHS), n + 2)
        state = ctx.frame_cells_hold_state(40, 200, len(RTHS), hold)
        ctx.frame_cells_hold_masks(frames[:64], REGION, RTHS, hold, P, state, masks, 0, 0)
        ctx.frame_cells_hold_masks(frames[64:], REGION, RTHS, hold, P, state, masks, 64, 64, flush=True)
        _KEPT[hold] = (frames, masks, host_words(masks).copy())
    return _KEPT[hold]


@pytest.mark.parametrize("rect", RECTS["whole"])
@pytest.mark.parametrize("hold", RHOLDS)
def test_reference_rows_are_busy(hold, rect):
    """The precondition of the comparison below, on the reference alone: all three columns are nonzero in at least a third of the rows
    from row `hold` on (one interior column cannot be that busy)."""
    for th in RTHS:
        want = want_rows(hold, rect, th)
        assert want.shape == (2 * hold + 70, 3)
        if rect[3] - rect[2] - 2 > 1:
            busy = int((want[hold:] > 0).all(1).sum())
            assert 3 * busy >= len(want) - hold, (th, busy)


def replay_call(ctx, masks, q, f0, f1, rect, hold, state, fed, flush):
    """One vse_frame_masks_replay_hold call -> host int32 rows; checks the rows it must not write."""
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    n = f1 - f0
    out = torch.full((n + hold - 1 + GUARD, 3), -7, dtype=torch.int32, device=ctx.tdev)
    rc = lib.vse_frame_masks_replay_hold(ctx.handle, C.c_void_p(masks.words.data_ptr()), masks.area_h, masks.area_w, masks.nt, masks.cap, q,
                                         f0, f1, *rect, hold, C.c_void_p(state.data_ptr()), fed, int(flush), C.c_void_p(out.data_ptr()),
                                         ctx.stream())
    assert rc == 0, lib.vse_last_error().decode()
    lo, hi = emitted(fed, n, hold, flush)
    out = out.cpu().numpy()
    assert (out[hi - lo:] == -7).all(), "rows behind the emitted ones were written"
    return out[:hi - lo]


def hold_rows(ctx, frames, rect, th, hold, state, a, b, fed, flush):
    return ctx.frame_hold(frames[a:b], rect, th, hold, state, fed, flush=flush).cpu().numpy()


@pytest.mark.parametrize("rect", RECTS["whole"])
@pytest.mark.parametrize("hold", RHOLDS)
def test_replay_is_frame_hold_on_the_rectangle_and_hands_its_state_over(ctx, hold, rect):
    import torch
    frames, masks, host = kept(ctx, hold)
    n = len(frames)
    cut = n - FURTHER
    before = masks.words.cpu().numpy().tobytes()
    assert np.array_equal(host[:n], want_words(hold_clip(hold), REGION, RTHS, 0, n)) and (host[n:] == A5).all()
    h, w = rect[1] - rect[0], rect[3] - rect[2]

    def dirty_state():                            # fed == 0 ignores the state's content
        return torch.full_like(ctx.frame_hold_state(h, w, hold), 0xA5)

    for q, th in enumerate(RTHS):
        want = want_rows(hold, rect, th)
        # with a flush: every row of the clip
        flushed = replay_call(ctx, masks, q, 0, n, rect, hold, dirty_state(), 0, True)
        assert np.array_equal(flushed, hold_rows(ctx, frames, rect, th, hold, ctx.frame_hold_state(h, w, hold), 0, n, 0, True)), (q, th)
        assert np.array_equal(flushed, want) and np.array_equal(flushed, FMH.replay_hold(host, 40, 200, q, 0, n, rect, hold))
        # without: the rows trail by hold - 1, and both states, zero-filled first, are equal byte for byte
        rs, hs = ctx.frame_hold_state(h, w, hold), ctx.frame_hold_state(h, w, hold)
        rows = replay_call(ctx, masks, q, 0, n, rect, hold, rs, 0, False)
        assert np.array_equal(rows, hold_rows(ctx, frames, rect, th, hold, hs, 0, n, 0, False)) and len(rows) == n - hold + 1
        assert np.array_equal(rows, want[:n - hold + 1]) and np.array_equal(rows, FMH.replay_hold(host, 40, 200, q, 0, n, rect, hold, False))
        assert rs.cpu().numpy().tobytes() == hs.cpu().numpy().tobytes()
        # in two pieces, fed advancing: inside the first chunk, and one behind it; then the pending rows alone
        for split in (33, 64 + 1):
            ps = dirty_state()
            head = replay_call(ctx, masks, q, 0, split, rect, hold, ps, 0, False)
            tail = replay_call(ctx, masks, q, split, n, rect, hold, ps, split, False)
            assert np.array_equal(np.concatenate([head, tail]), rows), split
            assert ps.cpu().numpy().tobytes() == rs.cpu().numpy().tobytes(), split
            drained = replay_call(ctx, masks, q, n, n, rect, hold, ps, n, True)
            assert np.array_equal(np.concatenate([rows, drained]), flushed), split
        # vse_frame_hold carries on from the replayed state: the uninterrupted run of the first `cut` frames, FURTHER more and a flush
        cs = dirty_state()
        head = replay_call(ctx, masks, q, 0, cut, rect, hold, cs, 0, False)
        tail = hold_rows(ctx, frames, rect, th, hold, cs, cut, n, cut, True)
        assert np.array_equal(np.concatenate([head, tail]), want), (q, th)
    assert masks.words.cpu().numpy().tobytes() == before                                          # the buffer is only read


def test_rectangle_widths_cover_the_word_boundaries():
    widths = {r[3] - r[2] - 2 for r in RECTS["whole"]}
    assert {1, 63, 64, 65, 129} <= widths and {r[2] % 64 for r in RECTS["whole"]} == {0, 1, 63}
    assert any(r[0] % 8 for r in RECTS["whole"]) and any((r[1] - r[0] - 2) % 8 for r in RECTS["whole"])


# ---- refused arguments ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.zeros(8192, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    msk = torch.full((4096,), 0xA5, dtype=torch.uint8, device=ctx.tdev)   # a 9 x 19 region: one cell, 64 bytes per slot and threshold
    good = dict(n=1, y0=1, y1=10, x0=1, x1=20, ths=(32, 128), nt=None, hold=3, fed=0, state=st.data_ptr(), totals=tot.data_ptr(),
                masks=msk.data_ptr(), frames=buf.data_ptr(), cap=4, slot0=0)

    def call(**kw):
        a = {**good, **kw}
        ths = a["ths"]
        nt = len(ths) if a["nt"] is None else a["nt"]
        arr = (C.c_int * max(1, len(ths)))(*ths) if ths is not None else None
        return lib.vse_frame_cells_hold_masks(ctx.handle, C.c_void_p(a["frames"]), a["n"], 10, 20, 60, 600, a["y0"], a["y1"], a["x0"], a["x1"],
                                              arr, nt, a["hold"], 16, 1, 2, 2, 5, C.c_void_p(a["state"]), a["fed"], 1, C.c_void_p(a["totals"]),
                                              None, C.c_void_p(a["masks"]), a["cap"], a["slot0"], ctx.stream())
    bad = [dict(ths=(), nt=0), dict(ths=(1, 2, 3, 4, 5, 6, 7, 8, 9)), dict(ths=None, nt=2), dict(ths=(128, 32)), dict(ths=(0, 32)),
           dict(ths=(32, 256)),                                                                    # the thresholds
           dict(y1=3), dict(x0=5, x1=7), dict(y0=4, y1=4),                                         # below 3 x 3
           dict(y0=-1, y1=5), dict(y1=11), dict(x1=21),                                            # outside the 10 x 20 frame
           dict(n=-1), dict(frames=None), dict(state=None), dict(totals=None), dict(masks=None), dict(state=st.data_ptr() + 4),
           dict(masks=msk.data_ptr() + 4),
           dict(hold=0), dict(hold=33), dict(fed=-1),                                              # vse_frame_cells_hold's own
           dict(slot0=-1), dict(slot0=4), dict(n=2, slot0=3), dict(cap=0), dict(n=0, slot0=5)]     # the slots: no wrap
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells_hold_masks" in lib.vse_last_error().decode()
    hst = torch.full((4096,), 0x5A, dtype=torch.uint8, device=ctx.tdev)
    cnt = torch.full((64,), -9, dtype=torch.int32, device=ctx.tdev)

    def replay(area_h=9, area_w=19, nt=2, cap=4, q=0, f0=0, f1=1, rect=(0, 9, 0, 19), hold=3, fed=0, flush=1, src=msk.data_ptr(),
               counts=cnt.data_ptr(), dst=hst.data_ptr()):
        return lib.vse_frame_masks_replay_hold(ctx.handle, C.c_void_p(src), area_h, area_w, nt, cap, q, f0, f1, *rect, hold, C.c_void_p(dst),
                                               fed, flush, C.c_void_p(counts), ctx.stream())
    for kw in [dict(q=-1), dict(q=2), dict(nt=8, q=8), dict(nt=0), dict(nt=9, q=1), dict(area_h=2), dict(area_w=2), dict(src=None),
               dict(dst=None), dict(counts=None), dict(dst=hst.data_ptr() + 4), dict(src=msk.data_ptr() + 4), dict(counts=cnt.data_ptr() + 2),
               dict(f0=-1), dict(f0=1, f1=1, flush=0), dict(f0=2, f1=1), dict(f1=5), dict(f0=4, f1=5), dict(f0=5, f1=5),
               dict(hold=0), dict(hold=33), dict(fed=-1),
               dict(rect=(0, 2, 0, 19)), dict(rect=(0, 9, 3, 5)), dict(rect=(-1, 9, 0, 19)), dict(rect=(0, 10, 0, 19)),
               dict(rect=(0, 9, 0, 20)), dict(rect=(0, 9, -1, 19)), dict(rect=(5, 5, 0, 19))]:
        assert replay(**kw) == -1, kw
        assert "vse_frame_masks_replay_hold" in lib.vse_last_error().decode()
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
    n = lib.vse_frame_hold_state_bytes(9, 19, 3)
    assert not hst.cpu().numpy()[:n].any() and set(hst.cpu().numpy()[n:].tolist()) == {0x5A}      # the state of the rectangle, no more
