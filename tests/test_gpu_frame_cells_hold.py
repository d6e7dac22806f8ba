"""vse_frame_cells_hold on the MI355X, through the C ABI: for every threshold and hold its totals and per-cell counts are the integers
of the numpy restatement (tests/area_cells_hold_ref.py), over the geometries, frame counts, holds and call sequences at which the
kernel can go wrong; hold 1 is vse_frame_cells_multi and the counts summed over the cells are vse_frame_hold's rows; refused arguments
touch nothing; and AreaLocator / SubtitleExtractor with automaton="hold" on the engine equal the numpy path.  Integers throughout."""
import ctypes as C

import numpy as np
import pytest

import area_cells_ref as R
from area_cells_hold_ref import NumpyCellsHold, clip_totals_hold, held_cell_counts
from test_gpu_frame_cells_multi import REGIONS, calib_frames, device_view, run_multi

pytestmark = pytest.mark.gpu

P = R.Params(edge_thresh=0, min_edges=8, ratio_num=1, ratio_den=2, min_frames=3, max_frames=10)      # edge_thresh: the thresholds are passed apart
T3 = (24, 96, 200)
T8 = (1, 24, 32, 48, 96, 128, 200, 255)
HOLDS = (1, 2, 3, 8, 31, 32)
N = 130
_ref = {}


@pytest.fixture(scope="module")
def clips():
    out = {name: calib_frames(N, h, w, seed=h * 1000 + w) for name, (h, w, _a) in REGIONS.items()}
    for f in out.values():
        f.setflags(write=False)
    return out


def ref_totals(clips, region, n, ths, hold, flush=True):
    """[nt,gy,gx,4] of the first n frames of the region's clip, computed once per case."""
    key = ("totals", region, n, tuple(ths), hold, flush)
    if key not in _ref:
        area = REGIONS[region][2]
        _ref[key] = np.stack([clip_totals_hold(clips[region][:n], area, P._replace(edge_thresh=th), hold, flush) for th in ths])
        _ref[key].setflags(write=False)
    return _ref[key]


def ref_counts(clips, region, n, ths, hold):
    """[nt,n,gy,gx,3] of the first n frames of the region's clip."""
    key = ("counts", region, n, tuple(ths), hold)
    if key not in _ref:
        _ref[key] = np.stack([held_cell_counts(clips[region][:n], REGIONS[region][2], th, hold) for th in ths])
        _ref[key].setflags(write=False)
    return _ref[key]


def run_hold(ctx, dev, area, ths, hold, calls, p=P, state=None):
    """calls: [(first, last, fed, flush)] over the frames of dev, through one state -> (host totals [nt,gy,gx,4], the calls' cell
    counts joined, [nt,rows,gy,gx,3])."""
    y0, y1, x0, x1 = area
    state = state or ctx.frame_cells_hold_state(y1 - y0, x1 - x0, len(ths), hold)
    rows = []
    for a, b, fed, flush in calls:
        _t, c = ctx.frame_cells_hold(dev[a:b], area, ths, hold, p, state, fed, flush=flush, want_counts=True)
        rows.append(c.cpu().numpy())
    return state.totals.cpu().numpy(), np.concatenate(rows, 1)


def one_call(n):
    return [(0, n, 0, True)]


def dev_of(ctx, clips, region):
    return device_view(ctx, clips[region], padded=region == "27x200-inset")


# ---- the cases are not vacuous -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", list(REGIONS))
def test_reference_is_busy(clips, region):
    base = ref_totals(clips, region, N, T3, 1)
    for hold in (2, 3, 8, 32):
        want = ref_totals(clips, region, N, T3, hold)
        # (the one pixel of 3x3 never reaches min_edges, so its totals are zero at every hold: there the counts must differ)
        assert region == "3x3" or not np.array_equal(want, base), hold
        assert not np.array_equal(ref_counts(clips, region, N, T3, hold), ref_counts(clips, region, N, T3, 1)), hold
        if region != "3x3" and hold <= 8:
            assert want[..., 0].max() > 0 and want[..., 3].max() > 0, hold
    if region != "3x3":
        for hold in HOLDS[:4]:
            assert len({ref_totals(clips, region, N, T3, hold)[k].tobytes() for k in range(3)}) == 3, hold


# ---- geometry, holds and frame counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", HOLDS)
@pytest.mark.parametrize("region", list(REGIONS))
def test_totals_and_counts_match_numpy(ctx, clips, region, hold):
    area = REGIONS[region][2]
    dev = dev_of(ctx, clips, region)
    ths = T8 if region == "27x200-inset" else T3
    dims = R.dims(area[1] - area[0], area[3] - area[2])
    for n in sorted({1, hold - 1, hold, 63, 64, 65, N} - {0}):
        got, counts = run_hold(ctx, dev, area, ths, hold, one_call(n))
        assert got.shape == (len(ths),) + dims + (4,) and got.dtype == np.int32
        assert np.array_equal(got, ref_totals(clips, region, n, ths, hold)), n
        assert counts.shape == (len(ths), n) + dims + (3,) and np.array_equal(counts, ref_counts(clips, region, n, ths, hold)), n
    # n == 0: 37 frames without a flush, then a call without frames that drains the pending rows and closes the open runs
    calls = [(0, 37, 0, False), (37, 37, 37, True)]
    got, counts = run_hold(ctx, dev, area, ths, hold, calls)
    assert np.array_equal(got, ref_totals(clips, region, 37, ths, hold))
    assert np.array_equal(counts, ref_counts(clips, region, 37, ths, hold))
    open_runs, first = run_hold(ctx, dev, area, ths, hold, calls[:1])
    assert np.array_equal(open_runs, ref_totals(clips, region, 37, ths, hold, flush=False))
    assert first.shape[1] == max(0, 37 - hold + 1)


@pytest.mark.parametrize("ths", [(1,), (255,), (128,), (1, 255), (60, 61), T8])
def test_one_two_and_eight_thresholds(ctx, clips, ths):
    area = REGIONS["11x67"][2]
    dev = dev_of(ctx, clips, "11x67")
    for hold in (1, 3):
        got, counts = run_hold(ctx, dev, area, ths, hold, one_call(65))
        assert got.shape[0] == len(ths)
        assert np.array_equal(got, ref_totals(clips, "11x67", 65, ths, hold))
        assert np.array_equal(counts, ref_counts(clips, "11x67", 65, ths, hold))


# ---- against the other entry points --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("region", list(REGIONS))
def test_hold_one_is_frame_cells_multi(ctx, clips, region):
    area = REGIONS[region][2]
    dev = dev_of(ctx, clips, region)
    got, _c = run_hold(ctx, dev, area, T8, 1, [(0, 50, 0, False), (50, N, 50, True)])
    assert np.array_equal(got, run_multi(ctx, dev, area, T8, [(0, 50, True, False), (50, N, False, True)]))
    assert np.array_equal(got, ref_totals(clips, region, N, T8, 1))


@pytest.mark.parametrize("hold", HOLDS)
def test_counts_summed_over_the_cells_are_frame_hold_rows(ctx, clips, hold):
    area = REGIONS["27x200-inset"][2]
    dev = dev_of(ctx, clips, "27x200-inset")
    y0, y1, x0, x1 = area
    state = ctx.frame_hold_state(y1 - y0, x1 - x0, hold)
    rows = [ctx.frame_hold(dev[a:b], area, 96, hold, state, a, flush=flush).cpu().numpy() for a, b, flush in ((0, 70, False), (70, N, True))]
    _t, counts = run_hold(ctx, dev, area, (96,), hold, [(0, 70, 0, False), (70, N, 70, True)])
    assert counts.shape[:2] == (1, N) and np.array_equal(counts[0].sum((1, 2)), np.concatenate(rows))
    assert counts[0, :, :, :, 0].max() > 0


# ---- call sequences ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,hold", [(0, 3), (1, 8), (2, 32)])
def test_random_batch_splits_equal_one_call(ctx, clips, seed, hold):
    area = REGIONS["27x200-inset"][2]
    dev = dev_of(ctx, clips, "27x200-inset")
    rng = np.random.default_rng(seed)
    cuts = sorted(int(c) for c in rng.integers(0, N + 1, size=int(rng.integers(2, 9))))          # equal cuts: a call without frames
    edges = [0] + cuts + [N]
    calls = [(a, b, a, False) for a, b in zip(edges[:-1], edges[1:])] + [(N, N, N, True)]       # the last call only flushes
    got, counts = run_hold(ctx, dev, area, T8, hold, calls)
    assert np.array_equal(got, ref_totals(clips, "27x200-inset", N, T8, hold))
    assert np.array_equal(counts, ref_counts(clips, "27x200-inset", N, T8, hold))
    one, _c = run_hold(ctx, dev, area, T8, hold, one_call(N))
    assert np.array_equal(got, one)
    unflushed, _c = run_hold(ctx, dev, area, T8, hold, calls[:-1])
    assert np.array_equal(unflushed, ref_totals(clips, "27x200-inset", N, T8, hold, flush=False))


def test_fed_zero_restarts_in_mid_clip_and_a_dirty_state_is_reused(ctx, clips):
    area = REGIONS["27x200-inset"][2]
    frames = clips["27x200-inset"]
    dev = dev_of(ctx, clips, "27x200-inset")
    big = ctx.frame_cells_hold_state(27, 200, 8, 8)
    calls = [(0, 50, 0, False), (50, 100, 0, False), (100, N, 50, True)]              # the second call starts a clip
    got, _c = run_hold(ctx, dev, area, T8, 8, calls, state=big)
    want = np.stack([clip_totals_hold(frames[50:], area, P._replace(edge_thresh=th), 8) for th in T8])
    assert np.array_equal(got, want)
    assert not np.array_equal(got, ref_totals(clips, "27x200-inset", N, T8, 8))
    # the same words, now dirty, under a smaller region, fewer thresholds and a smaller hold
    from vse_amd import engine
    state = engine.CellsState(big.words, ctx.torch.full((3, 2, 2, 4), -5, dtype=ctx.torch.int32, device=ctx.tdev))
    got, counts = run_hold(ctx, dev_of(ctx, clips, "11x67"), REGIONS["11x67"][2], T3, 3, [(0, 40, 0, False), (40, 70, 40, True)], state=state)
    assert np.array_equal(got, ref_totals(clips, "11x67", 70, T3, 3))
    assert np.array_equal(counts, ref_counts(clips, "11x67", 70, T3, 3))


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
def test_rejects_bad_arguments_without_touching_the_buffers(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.zeros(16384, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    cnt = torch.full((8 * 32 * 3,), -9, dtype=torch.int32, device=ctx.tdev)
    good = dict(n=1, y0=0, y1=10, x0=0, x1=20, num=1, den=2, minf=2, maxf=5, pitch=60, ths=(32, 128), nt=None, hold=3, fed=0,
                state=st.data_ptr(), totals=tot.data_ptr(), frames=buf.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        ths = a["ths"]
        nt = len(ths) if a["nt"] is None else a["nt"]
        arr = (C.c_int * max(1, len(ths)))(*ths) if ths is not None else None
        return lib.vse_frame_cells_hold(ctx.handle, C.c_void_p(a["frames"]), a["n"], 10, 20, a["pitch"], 600, a["y0"], a["y1"], a["x0"],
                                        a["x1"], arr, nt, a["hold"], 16, a["num"], a["den"], a["minf"], a["maxf"], C.c_void_p(a["state"]),
                                        a["fed"], 1, C.c_void_p(a["totals"]), C.c_void_p(cnt.data_ptr()), ctx.stream())
    bad = [dict(y1=2), dict(x0=5, x1=7), dict(y0=-1, y1=5), dict(y1=11), dict(x1=21), dict(y0=4, y1=4), dict(n=-1), dict(num=0),
           dict(den=0), dict(den=1025), dict(minf=0), dict(minf=6, maxf=5), dict(pitch=59),
           dict(frames=None), dict(state=None), dict(totals=None), dict(state=st.data_ptr() + 4),
           dict(ths=(), nt=0), dict(ths=(1, 2, 3, 4, 5, 6, 7, 8, 9)), dict(ths=(32, 128), nt=-1), dict(ths=None, nt=2),
           dict(ths=(128, 32)), dict(ths=(32, 32)), dict(ths=(32, 128, 64)), dict(ths=(0, 32)), dict(ths=(32, 256)), dict(ths=(-1,)),
           dict(hold=0), dict(hold=33), dict(hold=-1), dict(fed=-1), dict(n=2 ** 31 - 1, hold=2), dict(n=2 ** 31 - 31, hold=32)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells_hold" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert set(tot.cpu().tolist()) == {-7} and set(cnt.cpu().tolist()) == {-9} and int(st.sum()) == 0       # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert tot.cpu().tolist()[:8] == [0] * 8 and tot.cpu().tolist()[8] == -7        # one cell, two thresholds, a fresh clip
    assert cnt.cpu().tolist()[:3] == [0] * 3 and cnt.cpu().tolist()[3:9] == [-9] * 6 and cnt.cpu().tolist()[9:12] == [0] * 3
    assert call(ths=(1, 2, 3, 4, 5, 6, 7, 255), hold=32) == 0
    torch.cuda.synchronize()
    assert tot.cpu().tolist()[:32] == [0] * 32 and tot.cpu().tolist()[32] == -7
    # state: per threshold 128 bytes per word of every interior row, then one int32 per threshold and cell, padded to 8 bytes
    assert lib.vse_frame_cells_hold_state_bytes(11, 67, 1, 1) == lib.vse_frame_cells_hold_state_bytes(11, 67, 1, 32) == 9 * 2 * 128 + 16
    assert lib.vse_frame_cells_hold_state_bytes(11, 67, 8, 3) == 8 * 9 * 2 * 128 + 128
    assert lib.vse_frame_cells_hold_state_bytes(10, 66, 3, 2) == 3 * 8 * 128 + 16
    assert lib.vse_frame_cells_hold_state_bytes(3, 3, 1, 1) == 128 + 8
    for h, w, nt, hold in ((2, 67, 4, 3), (11, 2, 4, 3), (11, 67, 0, 3), (11, 67, 9, 3), (11, 67, 4, 0), (11, 67, 4, 33)):
        assert lib.vse_frame_cells_hold_state_bytes(h, w, nt, hold) == 0
    with pytest.raises(engine.VseError):
        ctx.frame_cells_hold_state(11, 67, 9, 3)
    with pytest.raises(engine.VseError):
        ctx.frame_cells_hold_state(11, 67, 2, 33)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_held_locator_on_the_engine_equals_the_numpy_path(ctx):
    from test_area_locator_hold import FPS, HELD_AREA, as_tuple, busy_clip
    from vse_amd import area_locator
    frames, _truth = busy_clip()
    host = area_locator.AreaLocator(NumpyCellsHold(), automaton="hold", edge_thresh="auto")
    want = host.run(list(frames), FPS)
    dev = area_locator.AreaLocator(area_locator.EngineCells(ctx), automaton="hold", edge_thresh="auto", batch=16)
    got = dev.run(iter(frames), FPS)
    assert np.array_equal(dev.totals, host.totals) and dev.totals.shape[0] == 8 and dev.hold == host.hold == 8
    assert list(dev.scores) == list(host.scores) and dev.edge_thresh == host.edge_thresh == 64
    assert as_tuple(got) == as_tuple(want) == HELD_AREA
    # one threshold, the integer path
    one = area_locator.AreaLocator(area_locator.EngineCells(ctx), automaton="hold", batch=40)
    assert as_tuple(one.run(iter(frames), FPS)) == HELD_AREA and np.array_equal(one.totals, host.totals[5])


def test_extractor_on_the_engine_locates_on_held_edges(ctx, monkeypatch):
    from test_area_locator_hold import HELD_AREA, as_tuple, busy_clip, run_extractor
    from vse_amd import area_locator, extractor, frame_select
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = busy_clip()
    auto, got = run_extractor(frames, truth, "auto", change_counter=frame_select.EngineHoldCounter(ctx),
                              area_params={"automaton": "hold", "cells_fn": area_locator.EngineCells(ctx)})
    assert as_tuple(auto.located_area) == HELD_AREA
    _given, want = run_extractor(frames, truth, extractor.SubtitleArea(*HELD_AREA), change_counter=frame_select.EngineHoldCounter(ctx))
    assert got == want and got[1] == [(s, e, (s + e) // 2) for s, e, _t in truth]
