"""vse_frame_cells_hold_bounded on the MI355X, through the C ABI: for every threshold, hold and max_hold its totals and per-cell counts
are the integers of the numpy restatement (tests/area_cells_hold_bounded_ref.py), over the regions, bounds and call sequences at which
the kernel can go wrong (the ring of pending rows wrapping, nothing final before the flush, batches across the 64-step chunks); the
counts summed over the cells are vse_frame_hold_bounded's rows and max_hold 4000 is vse_frame_cells_hold, both on the device; refused
arguments touch nothing; and AreaLocator with max_hold_frames on the engine equals the numpy path.  Integers throughout; no timing."""
import ctypes as C

import numpy as np
import pytest

import area_cells_ref as R
from area_cells_hold_bounded_ref import NumpyCellsHoldBounded, bounded_cell_counts, totals_of
from test_area_locator_hold_bounded import noisy_clip, static_clip
from test_gpu_frame_cells_multi import device_view

pytestmark = pytest.mark.gpu

P = R.Params(edge_thresh=0, min_edges=16, ratio_num=1, ratio_den=2, min_frames=3, max_frames=25)     # edge_thresh: the thresholds are passed apart
T1 = (128,)
T3 = (24, 96, 200)
T8 = (24, 32, 48, 64, 96, 128, 160, 192)
# (3, 5): the 69-slot ring wraps inside the 90 frames; (2, 200): nothing is final before the flush
BOUNDS = [(1, 1), (3, 3), (3, 5), (3, 30), (2, 200)]
# the whole frame's interior is 118 x 318: the last cell row and the last cell column are cut off
REGIONS = {"whole": (0, 120, 0, 320), "3x3": (95, 98, 100, 103), "11x67": (88, 99, 30, 97)}
N = 90
BATCHES = {"90": (90,), "64+26": (64, 26), "65+25": (65, 25), "1s": (1,) * 90, "7s": (7,) * 12 + (6,)}
_ref, _dev = {}, {}


def clip(name):
    return noisy_clip() if name == "noisy" else static_clip(name)[0]


def dev_of(ctx, name):
    """The clip on the device behind an odd base address, with a row pitch and a frame stride wider than any region."""
    if name not in _dev:
        _dev[name] = device_view(ctx, clip(name), padded=True)
    return _dev[name]


def ref_counts(name, region, ths, hold, max_hold):
    """[nt,N,gy,gx,3] of the clip in the region, computed once per case."""
    key = (name, region, tuple(ths), hold, max_hold)
    if key not in _ref:
        _ref[key] = np.stack([bounded_cell_counts(clip(name), REGIONS[region], th, hold, max_hold) for th in ths])
        _ref[key].setflags(write=False)
    return _ref[key]


def ref_totals(name, region, ths, hold, max_hold, upto=N, flush=True):
    """[nt,gy,gx,4] over the clip's rows 1 .. upto (rows that are final are the whole clip's rows)."""
    key = ("totals", name, region, tuple(ths), hold, max_hold, upto, flush)
    if key not in _ref:
        c = ref_counts(name, region, ths, hold, max_hold)
        _ref[key] = np.stack([totals_of(c[k, :upto], P, flush) for k in range(len(ths))])
    return _ref[key]


def calls_of(batches, tail_flush):
    """[(first, last, fed, flush)]: the batches in order; the clip ends with the last batch, or with a call of its own without frames."""
    edges = np.concatenate([[0], np.cumsum(batches)]).tolist()
    calls = [(a, b, a, False) for a, b in zip(edges[:-1], edges[1:])]
    if tail_flush:
        return calls + [(edges[-1], edges[-1], edges[-1], True)]
    return calls[:-1] + [calls[-1][:3] + (True,)]


def run_bounded(ctx, dev, area, ths, hold, max_hold, calls, state=None):
    """calls through one state -> (host totals [nt,gy,gx,4], the calls' cell counts joined, [nt,rows,gy,gx,3])."""
    y0, y1, x0, x1 = area
    state = state or ctx.frame_cells_hold_bounded_state(y1 - y0, x1 - x0, len(ths), max_hold)
    rows = []
    for a, b, fed, flush in calls:
        _t, c = ctx.frame_cells_hold_bounded(dev[a:b], area, ths, hold, max_hold, P, state, fed, flush=flush, want_counts=True)
        rows.append(c.cpu().numpy())
    return state.totals.cpu().numpy(), np.concatenate(rows, 1)


# ---- the cases are not vacuous -------------------------------------------------------------------------------------------------
def test_reference_is_busy():
    for hold, max_hold in BOUNDS:
        c = ref_counts("noisy", "whole", T8, hold, max_hold)
        assert c[..., 0].max() > 0 and c[..., 1].max() > 0 and c[..., 2].max() > 0, (hold, max_hold)
        assert len({c[k].tobytes() for k in range(8)}) == 8
    for name in ("busier", "loud"):
        t = ref_totals(name, "whole", T8, 3, 30)
        assert t[..., 0].max() > 0 and t[..., 3].max() > 0 and t.shape == (8, 15, 5, 4), name
    assert ref_totals("noisy", "11x67", T3, 3, 30)[..., 2].max() > 0
    assert ref_counts("noisy", "3x3", T3, 1, 1)[..., 0].max() == 1


# ---- bounds and call sequences, the whole frame at eight thresholds ----------------------------------------------------------------
@pytest.mark.parametrize("batches", list(BATCHES))
@pytest.mark.parametrize("hold,max_hold", BOUNDS)
def test_batches_give_the_totals_of_one_call(ctx, hold, max_hold, batches):
    dev, area = dev_of(ctx, "noisy"), REGIONS["whole"]
    want, want_counts = ref_totals("noisy", "whole", T8, hold, max_hold), ref_counts("noisy", "whole", T8, hold, max_hold)
    for tail_flush in (False, True):
        got, counts = run_bounded(ctx, dev, area, T8, hold, max_hold, calls_of(BATCHES[batches], tail_flush))
        assert got.shape == (8, 15, 5, 4) and got.dtype == np.int32
        assert np.array_equal(counts, want_counts), tail_flush
        assert np.array_equal(got, want), tail_flush
    # without the flush: the rows 1 .. N - max_hold, the last run left open
    got, counts = run_bounded(ctx, dev, area, T8, hold, max_hold, calls_of(BATCHES[batches], True)[:-1])
    final = max(0, N - max_hold)
    assert counts.shape[1] == final and np.array_equal(counts, want_counts[:, :final])
    assert np.array_equal(got, ref_totals("noisy", "whole", T8, hold, max_hold, upto=final, flush=False))


# ---- regions, numbers of thresholds, clips -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ths", [T1, T3, T8], ids=("nt1", "nt3", "nt8"))
@pytest.mark.parametrize("region", list(REGIONS))
def test_regions_and_threshold_counts(ctx, region, ths):
    area = REGIONS[region]
    dims = R.dims(area[1] - area[0], area[3] - area[2])
    for name, (hold, max_hold), batches in [("noisy", b, "7s") for b in BOUNDS] + [("busier", (3, 30), "65+25"), ("loud", (3, 5), "64+26"),
                                                                                 ("loud", (2, 200), "90")]:
        got, counts = run_bounded(ctx, dev_of(ctx, name), area, ths, hold, max_hold, calls_of(BATCHES[batches], name == "noisy"))
        assert got.shape == (len(ths),) + dims + (4,) and counts.shape == (len(ths), N) + dims + (3,)
        assert np.array_equal(counts, ref_counts(name, region, ths, hold, max_hold)), (name, hold, max_hold)
        assert np.array_equal(got, ref_totals(name, region, ths, hold, max_hold)), (name, hold, max_hold)


# ---- against the other entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold,max_hold", BOUNDS)
def test_counts_summed_over_the_cells_are_frame_hold_bounded_rows(ctx, hold, max_hold):
    dev, area = dev_of(ctx, "noisy"), REGIONS["whole"]
    y0, y1, x0, x1 = area
    state = ctx.frame_hold_bounded_state(y1 - y0, x1 - x0, max_hold)
    rows = [ctx.frame_hold_bounded(dev[a:b], area, 96, hold, max_hold, state, a, flush=flush).cpu().numpy()
            for a, b, flush in ((0, 70, False), (70, N, True))]
    _t, counts = run_bounded(ctx, dev, area, (96,), hold, max_hold, [(0, 70, 0, False), (70, N, 70, True)])
    assert counts.shape[:2] == (1, N) and np.array_equal(counts[0].sum((1, 2)), np.concatenate(rows))
    assert counts[0, ..., 0].max() > 0


@pytest.mark.parametrize("hold", (1, 3, 8))
def test_max_hold_4000_is_frame_cells_hold(ctx, hold):
    dev, area = dev_of(ctx, "noisy"), REGIONS["whole"]
    calls = [(0, 50, 0, False), (50, N, 50, True)]
    got, counts = run_bounded(ctx, dev, area, T8, hold, 4000, calls)
    state = ctx.frame_cells_hold_state(120, 320, 8, hold)
    held = []
    for a, b, fed, flush in calls:
        _t, c = ctx.frame_cells_hold(dev[a:b], area, T8, hold, P, state, fed, flush=flush, want_counts=True)
        held.append(c.cpu().numpy())
    assert np.array_equal(got, state.totals.cpu().numpy()) and got[..., 0].max() > 0
    assert np.array_equal(counts, np.concatenate(held, 1))


# ---- states ------------------------------------------------------------------------------------------------------------------------
def test_fed_zero_restarts_in_mid_clip_and_a_dirty_state_is_reused(ctx):
    from vse_amd import engine
    dev, area = dev_of(ctx, "noisy"), REGIONS["whole"]
    big = ctx.frame_cells_hold_bounded_state(120, 320, 8, 30)
    big.words.fill_(0xA5)                                                              # a clip's first call ignores what it finds
    calls = [(0, 40, 0, False), (40, 70, 0, False), (70, N, 30, True)]                 # the second call starts a clip
    got, counts = run_bounded(ctx, dev, area, T8, 3, 30, calls, state=big)
    tail = np.stack([bounded_cell_counts(clip("noisy")[40:], area, th, 3, 30) for th in T8])
    assert np.array_equal(got, np.stack([totals_of(tail[k], P) for k in range(8)]))
    assert np.array_equal(counts[:, 10:], tail)                                        # (the first call completed the rows of frames 1-10)
    # the same words, now dirty, under a smaller region, fewer thresholds and another max_hold
    state = engine.CellsState(big.words, ctx.torch.full((3, 2, 2, 4), -5, dtype=ctx.torch.int32, device=ctx.tdev))
    got, counts = run_bounded(ctx, dev, REGIONS["11x67"], T3, 3, 5, [(0, 40, 0, False), (40, N, 40, True)], state=state)
    assert np.array_equal(got, ref_totals("noisy", "11x67", T3, 3, 5))
    assert np.array_equal(counts, ref_counts("noisy", "11x67", T3, 3, 5))


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
def test_rejects_bad_arguments_without_touching_the_buffers(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    cnt = torch.full((8 * 33 * 3,), -9, dtype=torch.int32, device=ctx.tdev)
    good = dict(n=1, y0=0, y1=10, x0=0, x1=20, num=1, den=2, minf=2, maxf=5, pitch=60, ths=(32, 128), nt=None, hold=3, max_hold=5, fed=0,
                state=st.data_ptr(), totals=tot.data_ptr(), frames=buf.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        ths = a["ths"]
        nt = len(ths) if a["nt"] is None else a["nt"]
        arr = (C.c_int * max(1, len(ths)))(*ths) if ths is not None else None
        return lib.vse_frame_cells_hold_bounded(ctx.handle, C.c_void_p(a["frames"]), a["n"], 10, 20, a["pitch"], 600, a["y0"], a["y1"],
                                                a["x0"], a["x1"], arr, nt, a["hold"], a["max_hold"], 16, a["num"], a["den"], a["minf"],
                                                a["maxf"], C.c_void_p(a["state"]), a["fed"], 1, C.c_void_p(a["totals"]),
                                                C.c_void_p(cnt.data_ptr()), ctx.stream())
    bad = [dict(y1=2), dict(x0=5, x1=7), dict(y0=-1, y1=5), dict(y1=11), dict(x1=21), dict(y0=4, y1=4), dict(n=-1), dict(num=0),
           dict(den=0), dict(den=1025), dict(minf=0), dict(minf=6, maxf=5), dict(pitch=59),
           dict(frames=None), dict(state=None), dict(totals=None), dict(state=st.data_ptr() + 4),
           dict(ths=(), nt=0), dict(ths=(1, 2, 3, 4, 5, 6, 7, 8, 9)), dict(ths=(32, 128), nt=-1), dict(ths=None, nt=2),
           dict(ths=(128, 32)), dict(ths=(32, 32)), dict(ths=(32, 128, 64)), dict(ths=(0, 32)), dict(ths=(32, 256)), dict(ths=(-1,)),
           dict(hold=0), dict(hold=33, max_hold=40), dict(hold=-1), dict(fed=-1),
           dict(max_hold=2), dict(max_hold=0), dict(max_hold=-1), dict(max_hold=4001), dict(hold=1, max_hold=0),
           dict(n=2 ** 31 - 1), dict(n=2 ** 31 - 5), dict(n=2 ** 31 - 4000, max_hold=4000)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells_hold_bounded" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert set(tot.cpu().tolist()) == {-7} and set(cnt.cpu().tolist()) == {-9} and set(st.cpu().tolist()) == {0x5A}    # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert tot.cpu().tolist()[:8] == [0] * 8 and tot.cpu().tolist()[8] == -7        # one cell, two thresholds, a fresh clip
    got = cnt.cpu().tolist()                                                        # per threshold n + max_hold = 6 rows of room, one written
    assert got[:3] == [0] * 3 and got[3:18] == [-9] * 15 and got[18:21] == [0] * 3 and set(got[21:]) == {-9}
    assert call(ths=(1, 2, 3, 4, 5, 6, 7, 255), hold=32, max_hold=32) == 0
    torch.cuda.synchronize()
    assert tot.cpu().tolist()[:32] == [0] * 32 and tot.cpu().tolist()[32] == -7
    # state: per threshold 128 bytes per word of every interior row, then per threshold and cell max_hold + 64 slots of 4 bytes, then 8
    # bytes per threshold and cell, padded to 8 bytes
    size = lib.vse_frame_cells_hold_bounded_state_bytes
    assert size(11, 67, 1, 1) == 9 * 2 * 128 + 4 * 65 * 4 + 4 * 8
    assert size(11, 67, 8, 360) == 8 * (9 * 2 * 128 + 4 * 424 * 4 + 4 * 8)
    assert size(3, 3, 1, 1) == 128 + 65 * 4 + 8 + 4
    assert size(1080, 1920, 8, 360) == 8 * (1078 * 30 * 128 + 135 * 30 * (424 * 4 + 8))
    for h, w, nt, max_hold in ((2, 67, 4, 30), (11, 2, 4, 30), (11, 67, 0, 30), (11, 67, 9, 30), (11, 67, 4, 0), (11, 67, 4, 4001)):
        assert size(h, w, nt, max_hold) == 0
    with pytest.raises(engine.VseError):
        ctx.frame_cells_hold_bounded_state(11, 67, 9, 30)
    with pytest.raises(engine.VseError):
        ctx.frame_cells_hold_bounded_state(11, 67, 2, 4001)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_bounded_locator_on_the_engine_equals_the_numpy_path(ctx):
    from test_area_locator_hold_bounded import FPS, as_tuple
    from vse_amd import area_locator
    frames, _truth = static_clip("loud")
    kw = dict(automaton="hold", edge_thresh="auto", hold_frames=3, max_hold_frames=30)
    host = area_locator.AreaLocator(NumpyCellsHoldBounded(), **kw)
    want = host.run(list(frames), FPS)
    dev = area_locator.AreaLocator(area_locator.EngineCells(ctx), batch=16, **kw)
    got = dev.run(iter(frames), FPS)
    assert np.array_equal(dev.totals, host.totals) and dev.totals.shape[0] == 8 and (dev.hold, dev.max_hold) == (3, 30)
    assert list(dev.scores) == list(host.scores) and dev.edge_thresh == host.edge_thresh == 64
    assert as_tuple(got) == as_tuple(want) == (81, 120, 1, 320)
    # one threshold, the integer path; and without the option the held automaton, which finds nothing here
    one = area_locator.AreaLocator(area_locator.EngineCells(ctx), automaton="hold", edge_thresh=64, hold_frames=3, max_hold_frames=30, batch=40)
    assert as_tuple(one.run(iter(frames), FPS)) == (81, 120, 1, 320) and np.array_equal(one.totals, host.totals[3])
    held = area_locator.AreaLocator(area_locator.EngineCells(ctx), automaton="hold", edge_thresh="auto", hold_frames=3)
    assert held.run(iter(frames), FPS) is None and held.max_hold is None
