"""vse_frame_cells_counts and vse_frame_cells_export_state on the MI355X: the counts are, integer for integer, vse_frame_change's rows
at every threshold on the same device tensors and the numpy restatement's (tests/frame_change_ref.py); totals and state are, bit for
bit, vse_frame_cells_multi's and the numpy cells' (tests/area_cells_ref.py); a state passes between the two entries; every exported
slice continues under vse_frame_change and vse_frame_focus as an uninterrupted run of theirs; refused arguments touch nothing.  The
shapes are the smallest at which the kernel can go wrong: one interior pixel, interiors that end at, before and after a word (64
columns) and a tile (8 rows), frame counts around the 64 frames of a chunk, 1, 3 and 8 thresholds."""
import ctypes as C

import numpy as np
import pytest

import area_cells_ref as R
import frame_change_ref as FC
import frame_focus_ref as FF
from test_gpu_frame_cells_multi import calib_frames, device_view

pytestmark = pytest.mark.gpu

P = R.Params(edge_thresh=0, min_edges=8, ratio_num=1, ratio_den=2, min_frames=3, max_frames=10)      # edge_thresh: ignored
T8 = (1, 24, 32, 48, 96, 128, 200, 255)
T3 = (1, 60, 255)
FRAME_H, FRAME_W, FRAMES = 40, 200, 130
# (y0, y1, x0, x1), y0 and x0 > 0; the interior is two pixels smaller each way
AREAS = {"1x1": (5, 8, 7, 10), "7x63": (3, 12, 9, 74), "8x64": (11, 21, 2, 68), "9x65": (20, 31, 100, 167), "17x129": (6, 25, 33, 164),
         "17x63": (21, 40, 135, 200), "7x129": (1, 10, 1, 132)}


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


def want_counts(clip, area, ths, a, b):
    """numpy: int32 [b - a, nt, 3], frames a..b-1 of the clip with an empty mask before frame a."""
    key = (area, tuple(ths), a, b)
    if key not in _WANT:
        _WANT[key] = np.stack([FC.counts(clip[a:b], area, th)[0] for th in ths], 1)
    return _WANT[key]


def want_totals(clip, area, ths, a, b, flush=True):
    return np.stack([R.clip_totals(clip[a:b], area, P._replace(edge_thresh=th), flush=flush) for th in ths])


def run_counts(ctx, dev, area, ths, calls, state=None):
    """calls: [(first, last, reset, flush)] through one state -> (host counts of all calls in order, host totals, the state)."""
    y0, y1, x0, x1 = area
    state = state or ctx.frame_cells_multi_state(y1 - y0, x1 - x0, len(ths))
    rows = []
    for a, b, reset, flush in calls:
        _tot, c = ctx.frame_cells_counts(dev[a:b], area, ths, P, state, reset=reset, flush=flush)
        assert tuple(c.shape) == (b - a, len(ths), 3)
        rows.append(c.cpu().numpy())
    return np.concatenate(rows), state.totals.cpu().numpy(), state


def run_multi(ctx, dev, area, ths, calls, state=None):
    y0, y1, x0, x1 = area
    state = state or ctx.frame_cells_multi_state(y1 - y0, x1 - x0, len(ths))
    for a, b, reset, flush in calls:
        ctx.frame_cells_multi(dev[a:b], area, ths, P, state, reset=reset, flush=flush)
    return state.totals.cpu().numpy(), state


def run_change(ctx, dev, area, th, calls, fn="frame_change", state=None):
    """The same call sequence through vse_frame_change (or vse_frame_focus) at one threshold -> host rows, the state."""
    y0, y1, x0, x1 = area
    state = ctx.frame_change_state(y1 - y0, x1 - x0) if state is None else state
    rows = [getattr(ctx, fn)(dev[a:b], area, th, state, reset=reset).cpu().numpy() for a, b, reset, _f in calls if b > a]
    return np.concatenate(rows), state


def words(state):
    return state.words.cpu().numpy().tobytes()


# ---- geometry, frame counts, numbers of thresholds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("name", list(AREAS))
def test_counts_totals_and_state_match_the_existing_entries_and_numpy(ctx, clip, dev, name, n):
    area = AREAS[name]
    calls = [(0, n, True, True)]
    counts, totals, state = run_counts(ctx, dev, area, T8, calls)
    assert counts.dtype == np.int32 and totals.dtype == np.int32
    for q, th in enumerate(T8):
        assert np.array_equal(counts[:, q], run_change(ctx, dev, area, th, calls)[0]), (q, th)
    assert np.array_equal(counts, want_counts(clip, area, T8, 0, n))
    mt, ms = run_multi(ctx, dev, area, T8, calls)
    assert np.array_equal(totals, mt) and words(state) == words(ms)
    assert np.array_equal(totals, want_totals(clip, area, T8, 0, n))
    if name != "1x1" and n >= 63:
        assert len({counts[:, q].tobytes() for q in range(8)}) >= 5 and counts[:, :, 1:].max() > 0      # the thresholds differ; masks change


@pytest.mark.parametrize("ths", [(1,), (255,), (128,), T3])
def test_one_and_three_thresholds(ctx, clip, dev, ths):
    area = AREAS["9x65"]
    calls = [(0, 65, True, True)]
    counts, totals, state = run_counts(ctx, dev, area, ths, calls)
    for q, th in enumerate(ths):
        assert np.array_equal(counts[:, q], run_change(ctx, dev, area, th, calls)[0])
    assert np.array_equal(counts, want_counts(clip, area, ths, 0, 65))
    mt, ms = run_multi(ctx, dev, area, ths, calls)
    assert np.array_equal(totals, mt) and words(state) == words(ms)
    assert np.array_equal(totals, want_totals(clip, area, ths, 0, 65))


# ---- call sequences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x65", "17x129"])
def test_batch_splits_give_one_call(ctx, clip, dev, name):
    area = AREAS[name]
    whole = run_counts(ctx, dev, area, T8, [(0, 65, True, True)])
    for calls in ([(0, 1, True, False), (1, 65, False, True)], [(0, 64, True, False), (64, 65, False, True)]):
        got = run_counts(ctx, dev, area, T8, calls)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]) and words(got[2]) == words(whole[2])
    assert np.array_equal(whole[0], want_counts(clip, area, T8, 0, 65))


def test_reset_in_mid_clip(ctx, clip, dev):
    area = AREAS["17x129"]
    calls = [(0, 50, True, False), (50, 100, True, False), (100, 130, False, True)]              # the second call starts a clip
    counts, totals, state = run_counts(ctx, dev, area, T8, calls)
    assert np.array_equal(counts[50:], want_counts(clip, area, T8, 50, 130))
    assert np.array_equal(counts[:50], want_counts(clip, area, T8, 0, 50))
    assert not np.array_equal(counts[50:], want_counts(clip, area, T8, 0, 130)[50:])               # the reset shows in frame 50's row
    assert np.array_equal(totals, want_totals(clip, area, T8, 50, 130))
    for q, th in enumerate(T8):
        assert np.array_equal(counts[:, q], run_change(ctx, dev, area, th, calls)[0])
    mt, ms = run_multi(ctx, dev, area, T8, calls)
    assert np.array_equal(totals, mt) and words(state) == words(ms)


def test_no_frames_with_flush_only_closes_the_runs(ctx, clip, dev):
    area = AREAS["17x129"]
    counts, open_totals, state = run_counts(ctx, dev, area, T8, [(0, 37, True, False)])
    assert np.array_equal(open_totals, want_totals(clip, area, T8, 0, 37, flush=False))
    more, totals, _ = run_counts(ctx, dev, area, T8, [(37, 37, False, True)], state=state)
    assert more.shape == (0, 8, 3)
    want = want_totals(clip, area, T8, 0, 37)
    assert np.array_equal(totals, want) and not np.array_equal(want, open_totals)                 # the flush had runs to close
    assert np.array_equal(counts, want_counts(clip, area, T8, 0, 37))
    mt, ms = run_multi(ctx, dev, area, T8, [(0, 37, True, False), (37, 37, False, True)])
    assert np.array_equal(totals, mt) and words(state) == words(ms)


def test_a_state_passes_between_the_two_entries(ctx, clip, dev):
    area = AREAS["17x129"]
    alone, alone_state = run_multi(ctx, dev, area, T8, [(0, 130, True, True)])
    # begun by vse_frame_cells_multi, continued here
    _t, state = run_multi(ctx, dev, area, T8, [(0, 70, True, False)])
    counts, totals, state = run_counts(ctx, dev, area, T8, [(70, 130, False, True)], state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state)
    assert np.array_equal(counts, want_counts(clip, area, T8, 0, 130)[70:])                        # compared with the mask the other entry left
    # and the other way round
    _c, _t, state = run_counts(ctx, dev, area, T8, [(0, 70, True, False)])
    totals, state = run_multi(ctx, dev, area, T8, [(70, 130, False, True)], state=state)
    assert np.array_equal(totals, alone) and words(state) == words(alone_state)
    assert np.array_equal(alone, want_totals(clip, area, T8, 0, 130))


# ---- export ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ths", [("1x1", T3), ("7x63", T3), ("9x65", T8), ("17x129", T8)])
def test_every_exported_slice_continues_as_an_uninterrupted_run(ctx, clip, dev, name, ths):
    import torch
    area = AREAS[name]
    y0, y1, x0, x1 = area
    cut, end = 41, 110
    _c, _t, state = run_counts(ctx, dev, area, ths, [(0, cut, True, False)])
    before = words(state)
    for q, th in enumerate(ths):
        rows, ref_state = run_change(ctx, dev, area, th, [(0, cut, True, False)])
        nbytes = ref_state.numel()
        dirty = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=ctx.tdev)                   # every word is written, the flag set
        out = ctx.frame_cells_export_state(state, y1 - y0, x1 - x0, q, out=dirty)
        assert out is dirty
        got, ref = out.cpu().numpy(), ref_state.cpu().numpy()
        assert np.array_equal(got[16:], ref[16:]) and got[:4].view(np.uint32)[0] != 0
        fresh = ctx.frame_cells_export_state(state, y1 - y0, x1 - x0, q)
        assert np.array_equal(fresh.cpu().numpy(), ref)
        whole = run_change(ctx, dev, area, th, [(0, end, True, False)])[0]
        assert np.array_equal(run_change(ctx, dev, area, th, [(cut, end, False, False)], state=fresh)[0], whole[cut:])
        assert np.array_equal(whole, want_counts(clip, area, (th,), 0, end)[:, 0])
        focus = run_change(ctx, dev, area, th, [(0, end, True, False)], fn="frame_focus")[0]
        again = ctx.frame_cells_export_state(state, y1 - y0, x1 - x0, q)
        assert np.array_equal(run_change(ctx, dev, area, th, [(cut, end, False, False)], fn="frame_focus", state=again)[0], focus[cut:])
        assert np.array_equal(focus, FF.focus(clip[:end], area, th)[0])
    assert words(state) == before                                                                  # the cells' state is only read


# ---- refused arguments ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.zeros(8192, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    cnt = torch.full((64,), -9, dtype=torch.int32, device=ctx.tdev)
    good = dict(n=1, y0=1, y1=10, x0=1, x1=20, ths=(32, 128), nt=None, state=st.data_ptr(), totals=tot.data_ptr(), counts=cnt.data_ptr(),
                frames=buf.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        ths = a["ths"]
        nt = len(ths) if a["nt"] is None else a["nt"]
        arr = (C.c_int * max(1, len(ths)))(*ths) if ths is not None else None
        return lib.vse_frame_cells_counts(ctx.handle, C.c_void_p(a["frames"]), a["n"], 10, 20, 60, 600, a["y0"], a["y1"], a["x0"], a["x1"],
                                          arr, nt, 16, 1, 2, 2, 5, C.c_void_p(a["state"]), 1, 1, C.c_void_p(a["totals"]),
                                          C.c_void_p(a["counts"]), ctx.stream())
    bad = [dict(ths=(), nt=0), dict(ths=(1, 2, 3, 4, 5, 6, 7, 8, 9)), dict(ths=None, nt=2), dict(ths=(128, 32)), dict(ths=(0, 32)),
           dict(ths=(32, 256)),                                                                    # the thresholds
           dict(y1=3), dict(x0=5, x1=7), dict(y0=4, y1=4),                                         # below 3 x 3
           dict(y0=-1, y1=5), dict(y1=11), dict(x1=21),                                            # outside the 10 x 20 frame
           dict(n=-1), dict(frames=None), dict(state=None), dict(totals=None), dict(counts=None), dict(state=st.data_ptr() + 4)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells_counts" in lib.vse_last_error().decode()
    chg = torch.full((4096,), 0x5A, dtype=torch.uint8, device=ctx.tdev)

    def export(area_h=9, area_w=19, nt=2, q=0, src=st.data_ptr(), dst=chg.data_ptr()):
        return lib.vse_frame_cells_export_state(ctx.handle, C.c_void_p(src), area_h, area_w, nt, q, C.c_void_p(dst), ctx.stream())
    for kw in [dict(q=-1), dict(q=2), dict(nt=8, q=8), dict(nt=0), dict(nt=9, q=1), dict(area_h=2), dict(area_w=2), dict(src=None),
               dict(dst=None), dict(dst=chg.data_ptr() + 4)]:
        assert export(**kw) == -1, kw
        assert "vse_frame_cells_export_state" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert set(tot.cpu().tolist()) == {-7} and set(cnt.cpu().tolist()) == {-9} and int(st.sum()) == 0      # nothing was enqueued
    assert set(chg.cpu().tolist()) == {0x5A}
    assert call() == 0 and export() == 0 and export(q=1) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist()[:6] == [0] * 6 and cnt.cpu().tolist()[6] == -9                      # one frame of zeros, two thresholds
    assert tot.cpu().tolist()[:8] == [0] * 8 and tot.cpu().tolist()[8] == -7                      # one cell, two thresholds, reset
    n = lib.vse_frame_change_state_bytes(9, 19)
    got = chg.cpu().numpy()
    assert int(got[:4].view(np.uint32)[0]) != 0 and not got[16:n].any() and set(got[n:].tolist()) == {0x5A}
