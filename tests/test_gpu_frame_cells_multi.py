"""vse_frame_cells_multi on the MI355X, through the C ABI: for every threshold its totals are the integers of the numpy restatement
(tests/area_cells_ref.py) at that threshold AND the integers vse_frame_cells leaves for the same frames and call sequence, over the
geometries, frame counts and call sequences at which the kernel can go wrong; refused arguments touch nothing; and AreaLocator with
edge_thresh="auto" on the engine picks the area and the threshold that the numpy path picks."""
import ctypes as C

import numpy as np
import pytest

import area_cells_ref as R

pytestmark = pytest.mark.gpu

P = R.Params(edge_thresh=0, min_edges=8, ratio_num=1, ratio_den=2, min_frames=3, max_frames=10)      # edge_thresh: ignored by the multi call
T8 = (1, 24, 32, 48, 96, 128, 200, 255)
FRAME_H, FRAME_W = 40, 256
INSET = (6, 33, 31, 231)                  # 27 x 200 inside the 40 x 256 frame
REGIONS = {"3x3": (3, 3, (0, 3, 0, 3)), "10x66": (10, 66, (0, 10, 0, 66)), "11x67": (11, 67, (0, 11, 0, 67)),
           "27x200-inset": (FRAME_H, FRAME_W, INSET)}


def calib_frames(n, h, w, seed):
    """Per patch of 8 x 64 pixels: fresh noise in every frame at one of several amplitudes (from flat to full contrast), and over it a
    schedule of segments of 1..15 frames that show either the noise or grey bars of one of several contrasts, which hold still for the
    segment: runs (some longer than max_frames), ratio cuts where the bars change, and contrasts that fall between the thresholds."""
    rng = np.random.default_rng(seed)
    f = np.empty((n, h, w, 3), np.uint8)
    for y in range(0, h, 8):
        for x in range(0, w, 64):
            ph, pw = min(8, h - y), min(64, w - x)
            amp = int(rng.choice([0, 6, 30, 90, 255]))
            f[:, y:y + ph, x:x + pw] = rng.integers(0, 256 - amp, dtype=np.int64) + rng.integers(0, amp + 1, size=(n, ph, pw, 3))
            t = 0
            while t < n:
                length = int(rng.integers(1, 16))
                if rng.integers(0, 4):
                    c, period, phase = int(rng.choice([20, 28, 40, 70, 110, 160, 250])), int(rng.integers(3, 9)), int(rng.integers(0, 8))
                    bars = ((np.arange(pw) + phase) // period) & 1
                    f[t:t + length, y:y + ph, x:x + pw] = np.where(bars, 2 + c, 2).astype(np.uint8)[None, None, :, None]
                t += length
    return f


@pytest.fixture(scope="module")
def clips():
    out = {name: calib_frames(130, h, w, seed=h * 1000 + w) for name, (h, w, _a) in REGIONS.items()}
    for f in out.values():
        f.setflags(write=False)
    return out


def device_view(ctx, frames, padded):
    """The frames on the device; `padded`: behind an odd base address, with a padded row pitch and frame stride."""
    import torch
    n, h, w, _ = frames.shape
    if not padded:
        return torch.from_numpy(np.array(frames)).to(ctx.tdev)
    pitch, rows = (w + 13) * 3 + 5, h + 4
    buf = torch.zeros(max(n, 1) * rows * pitch + 1, dtype=torch.uint8, device=ctx.tdev)
    view = buf[1:].view(max(n, 1), rows, pitch)[:n, 3:3 + h, 6:6 + 3 * w].view(n, h, w, 3)
    view.copy_(torch.from_numpy(np.array(frames)))
    assert view.stride(1) == pitch and (n == 0 or view.stride(0) == rows * pitch)
    return view


def run_multi(ctx, dev, area, ths, calls, p=P, state=None):
    """calls: [(first, last, reset, flush)] over the frames of dev, through one state -> host totals [nt,gy,gx,4]."""
    y0, y1, x0, x1 = area
    state = state or ctx.frame_cells_multi_state(y1 - y0, x1 - x0, len(ths))
    for a, b, reset, flush in calls:
        ctx.frame_cells_multi(dev[a:b], area, ths, p, state, reset=reset, flush=flush)
    return state.totals.cpu().numpy()


def run_single(ctx, dev, area, ths, calls, p=P):
    """The same call sequence through vse_frame_cells, one threshold and one state at a time."""
    y0, y1, x0, x1 = area
    out = []
    for th in ths:
        state = ctx.frame_cells_state(y1 - y0, x1 - x0)
        for a, b, reset, flush in calls:
            ctx.frame_cells(dev[a:b], area, p._replace(edge_thresh=th), state, reset=reset, flush=flush)
        out.append(state.totals.cpu().numpy())
    return np.stack(out)


def reference(frames, area, ths, p=P, flush=True):
    return np.stack([R.clip_totals(frames, area, p._replace(edge_thresh=th), flush=flush) for th in ths])


def one_call(n):
    return [(0, n, True, True)]


# ---- geometry and frame counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
@pytest.mark.parametrize("region", list(REGIONS))
def test_totals_match_numpy_and_the_single_kernel(ctx, clips, region, n):
    _h, _w, area = REGIONS[region]
    frames = clips[region]
    dev = device_view(ctx, frames, padded=region == "27x200-inset")
    # n == 0: 37 frames without a flush, then a call without frames that only closes the open runs
    calls = [(0, 37, True, False), (37, 37, False, True)] if n == 0 else one_call(n)
    used = frames[:37] if n == 0 else frames[:n]
    got = run_multi(ctx, dev, area, T8, calls)
    want = reference(used, area, T8)
    assert got.shape == (8,) + R.dims(area[1] - area[0], area[3] - area[2]) + (4,) and got.dtype == np.int32
    assert np.array_equal(got, want)
    assert np.array_equal(got, run_single(ctx, dev, area, T8, calls))
    if n == 0:
        open_runs = reference(used, area, T8, flush=False)
        assert np.array_equal(run_multi(ctx, dev, area, T8, calls[:1]), open_runs)
        assert region in ("3x3", "10x66") or not np.array_equal(open_runs, want)       # in the larger regions the flush has runs to close
    if region != "3x3" and n >= 63:
        # qualifying runs, ratio cuts and runs beyond max_frames (present frames that no run covers) all occur, and the thresholds differ
        assert want[..., 0].max() > 0 and want[..., 3].max() > 0 and (want[..., 2] - want[..., 0]).max() > P.max_frames
        assert len({want[k].tobytes() for k in range(8)}) >= 5


@pytest.mark.parametrize("ths", [(1,), (255,), (128,), (1, 255), (60, 61)])
def test_one_and_two_thresholds(ctx, clips, ths):
    _h, _w, area = REGIONS["11x67"]
    frames = clips["11x67"][:65]
    dev = device_view(ctx, frames, padded=False)
    got = run_multi(ctx, dev, area, ths, one_call(65))
    assert got.shape[0] == len(ths)
    assert np.array_equal(got, reference(frames, area, ths))
    assert np.array_equal(got, run_single(ctx, dev, area, ths, one_call(65)))


# ---- call sequences ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_batch_splits_equal_one_call(ctx, clips, seed):
    _h, _w, area = REGIONS["27x200-inset"]
    frames = clips["27x200-inset"]
    dev = device_view(ctx, frames, padded=True)
    rng = np.random.default_rng(seed)
    cuts = sorted(int(c) for c in rng.integers(0, 131, size=int(rng.integers(2, 9))))          # equal cuts: a call without frames
    edges = [0] + cuts + [130]
    calls = [(a, b, k == 0, k == len(edges) - 2) for k, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
    got = run_multi(ctx, dev, area, T8, calls)
    assert np.array_equal(got, reference(frames, area, T8))
    assert np.array_equal(got, run_multi(ctx, dev, area, T8, one_call(130)))


def test_reset_in_mid_clip_and_state_reused_after_another_region_size(ctx, clips):
    _h, _w, area = REGIONS["27x200-inset"]
    frames = clips["27x200-inset"]
    dev = device_view(ctx, frames, padded=True)
    big = ctx.frame_cells_multi_state(27, 200, 8)
    calls = [(0, 50, True, False), (50, 100, True, False), (100, 130, False, True)]              # the second call starts a clip
    got = run_multi(ctx, dev, area, T8, calls, state=big)
    assert np.array_equal(got, reference(frames[50:], area, T8))
    assert np.array_equal(got, run_single(ctx, dev, area, T8, calls))
    assert not np.array_equal(got, reference(frames, area, T8))
    # the same words, now dirty, under a smaller region and fewer thresholds
    from vse_amd import engine
    _h, _w, small_area = REGIONS["11x67"]
    small = clips["11x67"][:70]
    ths = (32, 96, 200)
    state = engine.CellsState(big.words, ctx.torch.full((3, 2, 2, 4), -5, dtype=ctx.torch.int32, device=ctx.tdev))
    got = run_multi(ctx, device_view(ctx, small, padded=False), small_area, ths, one_call(70), state=state)
    assert np.array_equal(got, reference(small, small_area, ths))


# ---- refused arguments -------------------------------------------------------------------------------------------------------------
def test_rejects_bad_arguments_without_touching_the_buffers(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.zeros(8192, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    good = dict(n=1, y0=0, y1=10, x0=0, x1=20, num=1, den=2, minf=2, maxf=5, pitch=60, ths=(32, 128), nt=None, state=st.data_ptr(),
                totals=tot.data_ptr(), frames=buf.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        ths = a["ths"]
        nt = len(ths) if a["nt"] is None else a["nt"]
        arr = (C.c_int * max(1, len(ths)))(*ths) if ths is not None else None
        return lib.vse_frame_cells_multi(ctx.handle, C.c_void_p(a["frames"]), a["n"], 10, 20, a["pitch"], 600, a["y0"], a["y1"], a["x0"],
                                         a["x1"], arr, nt, 16, a["num"], a["den"], a["minf"], a["maxf"], C.c_void_p(a["state"]), 1, 1,
                                         C.c_void_p(a["totals"]), ctx.stream())
    bad = [dict(y1=2), dict(x0=5, x1=7), dict(y0=-1, y1=5), dict(y1=11), dict(x1=21), dict(y0=4, y1=4), dict(n=-1), dict(num=0),
           dict(den=0), dict(den=1025), dict(minf=0), dict(minf=6, maxf=5), dict(pitch=59),            # what vse_frame_cells refuses
           dict(frames=None), dict(state=None), dict(totals=None), dict(state=st.data_ptr() + 4),
           dict(ths=(), nt=0), dict(ths=(1, 2, 3, 4, 5, 6, 7, 8, 9)), dict(ths=(32, 128), nt=-1), dict(ths=None, nt=2),
           dict(ths=(128, 32)), dict(ths=(32, 32)), dict(ths=(32, 128, 64)), dict(ths=(0, 32)), dict(ths=(32, 256)), dict(ths=(-1,))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells_multi" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert set(tot.cpu().tolist()) == {-7} and int(st.sum()) == 0                # nothing was enqueued
    assert call() == 0 and call(ths=(1, 2, 3, 4, 5, 6, 7, 255)) == 0
    torch.cuda.synchronize()
    assert tot.cpu().tolist()[:32] == [0] * 32 and tot.cpu().tolist()[32] == -7      # one cell, eight thresholds, reset
    assert lib.vse_frame_cells_multi_state_bytes(11, 67, 1) == lib.vse_frame_cells_state_bytes(11, 67) == 2 * 2 * 72
    assert lib.vse_frame_cells_multi_state_bytes(11, 67, 8) == 8 * 2 * 2 * 72
    assert lib.vse_frame_cells_multi_state_bytes(11, 67, 0) == 0 and lib.vse_frame_cells_multi_state_bytes(11, 67, 9) == 0
    assert lib.vse_frame_cells_multi_state_bytes(2, 67, 4) == 0
    with pytest.raises(engine.VseError):
        ctx.frame_cells_multi_state(11, 67, 9)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_auto_locator_on_the_engine_equals_the_numpy_path(ctx):
    from area_clip import FPS, LOCATOR, as_tuple, decorated_clip, text_boxes
    from edge_calibrate_ref import NumpyCellsMulti, low_contrast
    from vse_amd import area_locator
    from vse_amd.extractor import SubtitleArea
    frames = low_contrast(decorated_clip()[0])
    lower = SubtitleArea(ymin=240, ymax=360, xmin=0, xmax=640)          # the lower third: the numpy cells take seconds on the whole frame
    host = area_locator.AreaLocator(NumpyCellsMulti(), edge_thresh="auto", search_area=lower, **LOCATOR)
    want = host.run(list(frames), FPS)
    dev = area_locator.AreaLocator(area_locator.EngineCells(ctx), edge_thresh="auto", search_area=lower, batch=16, **LOCATOR)
    got = dev.run(iter(frames), FPS)
    assert np.array_equal(dev.totals, host.totals) and dev.totals.shape[0] == 8
    assert list(dev.scores) == list(host.scores) and dev.edge_thresh == host.edge_thresh and dev.edge_thresh < 96
    assert want is not None and as_tuple(got) == as_tuple(want)
    for y0, y1, x0, x1 in text_boxes():
        assert got.ymin <= y0 and y1 <= got.ymax and got.xmin <= x0 and x1 <= got.xmax
