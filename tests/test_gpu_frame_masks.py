"""vse_frame_cells_masks and vse_frame_masks_replay on the MI355X: totals and state are, bit for bit, vse_frame_cells_multi's and the
numpy cells' (tests/area_cells_ref.py); the mask buffer read back is the numpy layout (tests/frame_masks_ref.py) and no slot beside the
call's is touched; a state passes between the two entries; the replay of a rectangle gives, integer for integer, vse_frame_change's
counts on the same device frames and the numpy reference's, leaves vse_frame_change's state behind so that vse_frame_change and
vse_frame_focus continue the clip, and only reads the buffer; refused arguments touch nothing.  The shapes are those of
tests/test_gpu_frame_cells_counts.py: one interior pixel, interiors that end at, before and after a word (64 columns) and a tile
(8 rows), frame counts around the 64 frames of a chunk, 1, 3 and 8 thresholds; the rectangles start at, one behind and one before a
word boundary of the region and end inside its partial last word and cell."""
import ctypes as C

import numpy as np
import pytest

import area_cells_ref as R
import frame_change_ref as FC
import frame_focus_ref as FF
import frame_masks_ref as FM
from test_gpu_frame_cells_counts import AREAS, FRAME_H, FRAME_W, FRAMES, P, T3, T8, run_change, run_multi, words
from test_gpu_frame_cells_multi import calib_frames, device_view

pytestmark = pytest.mark.gpu

THS = {1: (96,), 3: T3, 8: T8}
REGIONS = {"whole": (0, FRAME_H, 0, FRAME_W), "17x129": AREAS["17x129"], "9x65": AREAS["9x65"]}
# (ry0, ry1, rx0, rx1) in region coordinates; the interior is two pixels smaller each way.  rx0 % 64 is 0, 1 or 63.
RECTS = {
    "whole": [(0, 40, 0, 200),             # the region itself: its partial last word and cell
              (0, 12, 0, 3),               # the top-left corner, one interior column
              (5, 30, 1, 66),              # one behind a word boundary, 63 columns
              (2, 13, 63, 129),            # one before it, 64 columns
              (10, 40, 64, 131),           # at it, 65 columns, down to the bottom border
              (22, 40, 65, 196),           # 129 columns, bottom border
              (30, 40, 127, 200),          # the right and bottom border from one before a word boundary
              (1, 4, 191, 194)],           # one pixel inside the last word
    "17x129": [(0, 19, 0, 131), (0, 3, 0, 3), (3, 19, 1, 131), (1, 12, 63, 130), (8, 19, 64, 131), (2, 9, 1, 66)],
    "9x65": [(0, 11, 0, 67), (0, 3, 0, 3), (2, 11, 1, 67), (0, 11, 63, 67), (1, 10, 1, 66)],
}


@pytest.fixture(scope="module")
def clip():
    f = calib_frames(FRAMES, FRAME_H, FRAME_W, seed=71)
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def dev(ctx, clip):
    d = device_view(ctx, clip, padded=True)
    assert d.stride(1) > 3 * FRAME_W and d.stride(0) > FRAME_H * d.stride(1)
    return d


_WANT = {}


def want_words(clip, area, ths, a, b):
    key = ("words", area, tuple(ths), a, b)
    if key not in _WANT:
        _WANT[key] = FM.mask_words(clip[a:b], area, ths)
    return _WANT[key]


def want_totals(clip, area, ths, a, b, flush=True):
    key = ("totals", area, tuple(ths), a, b, flush)
    if key not in _WANT:
        _WANT[key] = np.stack([R.clip_totals(clip[a:b], area, P._replace(edge_thresh=th), flush=flush) for th in ths])
    return _WANT[key]


def dirty_buffer(ctx, area, nt, cap):
    y0, y1, x0, x1 = area
    masks = ctx.frame_masks_buffer(y1 - y0, x1 - x0, nt, cap)
    masks.words.fill_(0xA5)
    return masks


def host_words(masks):
    gy, gx = FM.dims(masks.area_h, masks.area_w)
    return masks.words.cpu().numpy().view(np.uint64).reshape(masks.cap, masks.nt, gy, gx, 8)


def run_masks(ctx, dev, area, ths, calls, masks, slot0=0, state=None):
    """calls: [(first, last, reset, flush)] through one state, the frames landing in consecutive slots from slot0 on -> host totals,
    the state."""
    y0, y1, x0, x1 = area
    state = state or ctx.frame_cells_multi_state(y1 - y0, x1 - x0, len(ths))
    for a, b, reset, flush in calls:
        ctx.frame_cells_masks(dev[a:b], area, ths, P, state, masks, slot0, reset=reset, flush=flush)
        slot0 += b - a
    return state.totals.cpu().numpy(), state


A5 = np.uint64(0xA5A5A5A5A5A5A5A5)


# ---- geometry, frame counts, numbers of thresholds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", list(AREAS))
def test_totals_state_and_masks_match_the_existing_entry_and_numpy(ctx, clip, dev, name, n, nt):
    area, ths = AREAS[name], THS[nt]
    calls = [(0, n, True, True)]
    masks = dirty_buffer(ctx, area, nt, n + 3)
    totals, state = run_masks(ctx, dev, area, ths, calls, masks, slot0=1)
    mt, ms = run_multi(ctx, dev, area, ths, calls)
    assert totals.dtype == np.int32 and np.array_equal(totals, mt) and words(state) == words(ms)
    assert np.array_equal(totals, want_totals(clip, area, ths, 0, n))
    got = host_words(masks)
    assert np.array_equal(got[1:1 + n], want_words(clip, area, ths, 0, n))
    assert (got[0] == A5).all() and (got[1 + n:] == A5).all()                                     # no slot beside the call's
    if name != "1x1" and n >= 63 and nt == 8:
        assert len({got[1:1 + n, q].tobytes() for q in range(8)}) >= 5                            # the thresholds differ


# ---- call sequences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x65", "17x129"])
def test_batch_splits_and_a_later_slot_give_the_buffer_of_one_call(ctx, clip, dev, name):
    area = AREAS[name]
    whole = dirty_buffer(ctx, area, 8, 70)
    wt, ws = run_masks(ctx, dev, area, T8, [(0, 65, True, True)], whole)
    want = host_words(whole)
    assert np.array_equal(want[:65], want_words(clip, area, T8, 0, 65)) and (want[65:] == A5).all()
    for calls in ([(0, 1, True, False), (1, 65, False, True)], [(0, 64, True, False), (64, 65, False, True)]):
        masks = dirty_buffer(ctx, area, 8, 70)
        totals, state = run_masks(ctx, dev, area, T8, calls, masks)
        assert np.array_equal(host_words(masks), want) and np.array_equal(totals, wt) and words(state) == words(ws)
    masks = dirty_buffer(ctx, area, 8, 70)
    totals, state = run_masks(ctx, dev, area, T8, [(0, 30, True, False), (30, 65, False, True)], masks, slot0=5)
    got = host_words(masks)
    assert np.array_equal(got[5:70], want[:65]) and (got[:5] == A5).all() and np.array_equal(totals, wt) and words(state) == words(ws)


def test_no_frames_with_flush_writes_no_slot(ctx, clip, dev):
    area = AREAS["17x129"]
    masks = dirty_buffer(ctx, area, 8, 40)
    open_totals, state = run_masks(ctx, dev, area, T8, [(0, 37, True, False)], masks)
    before = host_words(masks).copy()
    totals, state = run_masks(ctx, dev, area, T8, [(37, 37, False, True)], masks, slot0=37, state=state)
    assert np.array_equal(host_words(masks), before) and (before[37:] == A5).all()
    want = want_totals(clip, area, T8, 0, 37)
    assert np.array_equal(totals, want) and not np.array_equal(want, open_totals)                 # the flush had runs to close
    mt, ms = run_multi(ctx, dev, area, T8, [(0, 37, True, False), (37, 37, False, True)])
    assert np.array_equal(totals, mt) and words(state) == words(ms)


def test_a_state_passes_between_the_two_entries(ctx, clip, dev):
    area = AREAS["17x129"]
    alone, alone_state = run_multi(ctx, dev, area, T8, [(0, 130, True, True)])
    # begun by vse_frame_cells_multi, continued here
    _t, state = run_multi(ctx, dev, area, T8, [(0, 70, True, False)])
    masks = dirty_buffer(ctx, area, 8, 130)
    totals, state = run_masks(ctx, dev, area, T8, [(70, 130, False, True)], masks, slot0=70, state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state)
    assert np.array_equal(host_words(masks)[70:], want_words(clip, area, T8, 70, 130)) and (host_words(masks)[:70] == A5).all()
    # and the other way round
    _t, state = run_masks(ctx, dev, area, T8, [(0, 70, True, False)], dirty_buffer(ctx, area, 8, 70))
    totals, state = run_multi(ctx, dev, area, T8, [(70, 130, False, True)], state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state)
    assert np.array_equal(alone, want_totals(clip, area, T8, 0, 130))


# ---- replay ---------------------------------------------------------------------------------------------------------------------------
_KEPT = {}


def kept(ctx, dev, region_name, n):
    """The masks of the clip's first n frames over a region, made once per region."""
    key = (region_name, n)
    if key not in _KEPT:
        region = REGIONS[region_name]
        ths = T8 if region_name == "17x129" else T3
        masks = dirty_buffer(ctx, region, len(ths), n + 2)
        run_masks(ctx, dev, region, ths, [(0, 64, True, False), (64, n, False, True)], masks)
        _KEPT[key] = (masks, ths)
    return _KEPT[key]


@pytest.mark.parametrize("region_name,rect", [(name, rect) for name in RECTS for rect in RECTS[name]])
def test_replay_is_frame_change_on_the_rectangle_and_hands_its_state_over(ctx, clip, dev, region_name, rect):
    import torch
    cut, end = 70, 110
    region = REGIONS[region_name]
    masks, ths = kept(ctx, dev, region_name, cut)
    ry0, ry1, rx0, rx1 = rect
    assert rx0 % 64 in (0, 1, 63)
    area = (region[0] + ry0, region[0] + ry1, region[2] + rx0, region[2] + rx1)               # the rectangle in the frames' pixels
    before = masks.words.cpu().numpy().tobytes()
    want_host = host_words(masks)
    for q, th in enumerate(ths):
        rows, ref_state = run_change(ctx, dev, area, th, [(0, cut, True, False)])
        dirty = torch.full((ref_state.numel(),), 0xA5, dtype=torch.uint8, device=ctx.tdev)      # every word is written, the flag set
        counts, out = ctx.frame_masks_replay(masks, q, 0, cut, rect, reset=True, out=dirty)
        assert out is dirty and counts.dtype == torch.int32 and tuple(counts.shape) == (cut, 3)
        counts = counts.cpu().numpy()
        assert np.array_equal(counts, rows), (q, th)
        assert np.array_equal(counts, FC.counts(clip[:cut], area, th)[0])
        assert np.array_equal(counts, FM.replay(want_host, masks.area_h, masks.area_w, q, 0, cut, rect)[0])
        got, ref = out.cpu().numpy(), ref_state.cpu().numpy()
        assert np.array_equal(got[16:], ref[16:]) and got[:4].view(np.uint32)[0] != 0
        # in two pieces: reset on the first, the slot before on the second
        head, _s = ctx.frame_masks_replay(masks, q, 0, 33, rect, reset=True)
        tail, fresh = ctx.frame_masks_replay(masks, q, 33, cut, rect, reset=False)
        assert np.array_equal(np.concatenate([head.cpu().numpy(), tail.cpu().numpy()]), counts)
        assert np.array_equal(fresh.cpu().numpy()[16:], ref[16:])
        # the selectors carry on from the replayed state
        whole = run_change(ctx, dev, area, th, [(0, end, True, False)])[0]
        assert np.array_equal(run_change(ctx, dev, area, th, [(cut, end, False, False)], state=out)[0], whole[cut:])
        focus = run_change(ctx, dev, area, th, [(0, end, True, False)], fn="frame_focus")[0]
        assert np.array_equal(run_change(ctx, dev, area, th, [(cut, end, False, False)], fn="frame_focus", state=fresh)[0], focus[cut:])
        assert np.array_equal(focus, FF.focus(clip[:end], area, th)[0])
    assert masks.words.cpu().numpy().tobytes() == before                                          # the buffer is only read


def test_rectangle_widths_cover_the_word_boundaries():
    widths = {r[3] - r[2] - 2 for rects in RECTS.values() for r in rects}
    assert {1, 63, 64, 65, 129} <= widths
    assert {r[2] % 64 for rects in RECTS.values() for r in rects} == {0, 1, 63}


# ---- refused arguments ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.zeros(8192, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    msk = torch.full((4096,), 0xA5, dtype=torch.uint8, device=ctx.tdev)   # a 9 x 19 region: one cell, 64 bytes per slot and threshold
    good = dict(n=1, y0=1, y1=10, x0=1, x1=20, ths=(32, 128), nt=None, state=st.data_ptr(), totals=tot.data_ptr(), masks=msk.data_ptr(),
                frames=buf.data_ptr(), cap=4, slot0=0)

    def call(**kw):
        a = {**good, **kw}
        ths = a["ths"]
        nt = len(ths) if a["nt"] is None else a["nt"]
        arr = (C.c_int * max(1, len(ths)))(*ths) if ths is not None else None
        return lib.vse_frame_cells_masks(ctx.handle, C.c_void_p(a["frames"]), a["n"], 10, 20, 60, 600, a["y0"], a["y1"], a["x0"], a["x1"],
                                         arr, nt, 16, 1, 2, 2, 5, C.c_void_p(a["state"]), 1, 1, C.c_void_p(a["totals"]),
                                         C.c_void_p(a["masks"]), a["cap"], a["slot0"], ctx.stream())
    bad = [dict(ths=(), nt=0), dict(ths=(1, 2, 3, 4, 5, 6, 7, 8, 9)), dict(ths=None, nt=2), dict(ths=(128, 32)), dict(ths=(0, 32)),
           dict(ths=(32, 256)),                                                                    # the thresholds
           dict(y1=3), dict(x0=5, x1=7), dict(y0=4, y1=4),                                         # below 3 x 3
           dict(y0=-1, y1=5), dict(y1=11), dict(x1=21),                                            # outside the 10 x 20 frame
           dict(n=-1), dict(frames=None), dict(state=None), dict(totals=None), dict(masks=None), dict(state=st.data_ptr() + 4),
           dict(masks=msk.data_ptr() + 4),
           dict(slot0=-1), dict(slot0=4), dict(n=2, slot0=3), dict(cap=0), dict(n=0, slot0=5)]     # the slots: no wrap
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells_masks" in lib.vse_last_error().decode()
    chg = torch.full((4096,), 0x5A, dtype=torch.uint8, device=ctx.tdev)
    cnt = torch.full((64,), -9, dtype=torch.int32, device=ctx.tdev)

    def replay(area_h=9, area_w=19, nt=2, cap=4, q=0, f0=0, f1=1, rect=(0, 9, 0, 19), reset=1, src=msk.data_ptr(), counts=cnt.data_ptr(),
               dst=chg.data_ptr()):
        return lib.vse_frame_masks_replay(ctx.handle, C.c_void_p(src), area_h, area_w, nt, cap, q, f0, f1, *rect, reset, C.c_void_p(counts),
                                          C.c_void_p(dst), ctx.stream())
    for kw in [dict(q=-1), dict(q=2), dict(nt=8, q=8), dict(nt=0), dict(nt=9, q=1), dict(area_h=2), dict(area_w=2), dict(src=None),
               dict(dst=None), dict(counts=None), dict(dst=chg.data_ptr() + 4), dict(src=msk.data_ptr() + 4),
               dict(f0=-1), dict(f0=1, f1=1), dict(f0=2, f1=1), dict(f1=5), dict(reset=0), dict(f0=4, f1=5),
               dict(rect=(0, 2, 0, 19)), dict(rect=(0, 9, 3, 5)), dict(rect=(-1, 9, 0, 19)), dict(rect=(0, 10, 0, 19)),
               dict(rect=(0, 9, 0, 20)), dict(rect=(0, 9, -1, 19)), dict(rect=(5, 5, 0, 19))]:
        assert replay(**kw) == -1, kw
        assert "vse_frame_masks_replay" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert set(tot.cpu().tolist()) == {-7} and set(cnt.cpu().tolist()) == {-9} and int(st.sum()) == 0      # nothing was enqueued
    assert set(chg.cpu().tolist()) == {0x5A} and set(msk.cpu().tolist()) == {0xA5}
    assert call(n=2, slot0=1) == 0 and replay(f0=1, f1=3) == 0 and replay(q=1, f0=2, f1=3, reset=0, rect=(1, 8, 2, 12)) == 0
    torch.cuda.synchronize()
    got = msk.cpu().numpy()
    assert set(got[:128].tolist()) == {0xA5} and not got[128:384].any() and set(got[384:].tolist()) == {0xA5}      # slots 1 and 2, zeros
    assert tot.cpu().tolist()[:8] == [0] * 8 and tot.cpu().tolist()[8] == -7                      # one cell, two thresholds, reset
    assert cnt.cpu().tolist()[:3] == [0] * 3 and cnt.cpu().tolist()[6] == -9
    n = lib.vse_frame_change_state_bytes(7, 10)
    got = chg.cpu().numpy()
    assert int(got[:4].view(np.uint32)[0]) != 0 and not got[16:n].any()
