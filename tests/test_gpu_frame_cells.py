"""vse_frame_cells on the MI355X, through the C ABI: per-cell totals and counts equal the restatement of tests/area_cells_ref.py
integer for integer over the geometries at which the kernel can go wrong, calls chained through the state equal one call, and
AreaLocator on the engine locates what the restatement locates on the frames the device saw."""
import ctypes as C

import numpy as np
import pytest

import area_cells_ref as R
from frame_change_ref import counts as change_counts

pytestmark = pytest.mark.gpu

P = R.Params(edge_thresh=60, min_edges=8, ratio_num=1, ratio_den=2, min_frames=3, max_frames=10)


def mixed_frames(n, h, w, seed):
    """Noise of little contrast; over it, per cell-sized patch and frame, bars that mostly hold and sometimes switch off, move or
    change phase; one patch in four shows fresh full-contrast noise in every frame."""
    rng = np.random.default_rng(seed)
    f = rng.integers(60, 100, size=(n, h, w, 3), dtype=np.uint8)
    for y in range(0, h, 8):
        for x in range(0, w, 64):
            ph, pw = min(8, h - y), min(64, w - x)
            if rng.integers(0, 4) == 0:
                f[:, y:y + ph, x:x + pw] = rng.integers(0, 256, size=(n, ph, pw, 3), dtype=np.uint8)
                continue
            kind, period = 1, 4
            for t in range(n):
                r = rng.integers(0, 12)
                if r == 0:
                    kind = 0
                elif r == 1:
                    kind, period = 1, int(rng.integers(3, 9))
                elif r == 2:
                    kind = 2
                if kind:
                    bars = ((np.arange(pw) + (t if kind == 2 else 0)) // period) & 1
                    f[t, y:y + ph, x:x + pw] = np.where(bars, 250, 5).astype(np.uint8)[None, :, None]
    return f


def run_cells(ctx, dev, area, p=P, splits=None, flush=True, want_counts=False):
    """dev: cuda uint8 [n,H,W,3] view, fed in calls of `splits` frames through one state -> host totals (and counts)."""
    y0, y1, x0, x1 = area
    state = ctx.frame_cells_state(y1 - y0, x1 - x0)
    n = dev.shape[0]
    splits = splits or [n]
    assert sum(splits) == n
    counts, at = [], 0
    for k, m in enumerate(splits):
        out = ctx.frame_cells(dev[at:at + m], area, p, state, reset=(k == 0), flush=flush and k == len(splits) - 1, want_counts=want_counts)
        if want_counts:
            counts.append(out[1].cpu().numpy())
        at += m
    totals = state.totals.cpu().numpy()
    return (totals, np.concatenate(counts)) if want_counts else totals


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry_frames():
    return {(h, w): mixed_frames(130, h, w, seed=h * 1000 + w) for h, w in [(3, 3), (9, 65), (10, 66), (11, 67), (10, 130), (37, 150)]}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("hw", [(3, 3), (9, 65), (10, 66), (11, 67), (10, 130)])      # interiors 1x1, 7x63, 8x64, 9x65, 8x128
def test_totals_and_counts_match_reference(ctx, geometry_frames, hw, n):
    import torch
    frames = geometry_frames[hw][:n]
    area = (0, hw[0], 0, hw[1])
    want_counts, _ = R.cell_counts(frames, area, P.edge_thresh)
    want = R.clip_totals(frames, area, P)
    got, counts = run_cells(ctx, torch.from_numpy(frames).cuda(), area, want_counts=True)
    assert counts.shape == (n,) + R.dims(*hw) + (3,) == want_counts.shape
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(got, want)
    if hw != (3, 3) and n >= 63:
        assert want[..., 0].max() > 0 and want[..., 3].max() > 0          # the content has qualifying runs and ratio cuts


def test_inset_region_padded_pitch_stride_and_odd_base(ctx, geometry_frames):
    import torch
    frames = geometry_frames[(37, 150)][:70]
    area = (2, 35, 3, 147)
    padded = torch.zeros(70 * 41 * (163 * 3 + 5) + 1, dtype=torch.uint8, device=ctx.tdev)
    view = padded[1:].view(70, 41, 163 * 3 + 5)[:, 3:40, 6:6 + 450].view(70, 37, 150, 3)
    view.copy_(torch.from_numpy(frames))
    assert view.data_ptr() % 2 == 1 and view.stride(1) == 163 * 3 + 5 and view.stride(0) == 41 * (163 * 3 + 5)
    got, counts = run_cells(ctx, view, area, want_counts=True)
    assert np.array_equal(counts, R.cell_counts(frames, area, P.edge_thresh)[0])
    assert np.array_equal(got, R.clip_totals(frames, area, P))
    assert got.shape == (4, 3, 4) and got[..., 0].max() > 0


# ---- d_cell_counts ----------------------------------------------------------------------------------------------------------------
def test_cell_counts_sum_to_frame_change_and_are_optional(ctx, geometry_frames):
    import torch
    frames = geometry_frames[(37, 150)][:66]
    area = (1, 36, 2, 149)
    dev = torch.from_numpy(frames).cuda()
    totals, counts = run_cells(ctx, dev, area, want_counts=True)
    change = ctx.frame_change(dev, area, P.edge_thresh, ctx.frame_change_state(35, 147), reset=True).cpu().numpy()
    assert np.array_equal(counts.sum((1, 2)), change)
    assert np.array_equal(change, change_counts(frames, area, P.edge_thresh)[0])
    assert np.array_equal(run_cells(ctx, dev, area, want_counts=False), totals)          # d_cell_counts == NULL: the same totals


# ---- state ------------------------------------------------------------------------------------------------------------------------
def boundary_clip():
    """130 frames of one 10 x 200 region (4 cells) whose second cell holds a run open across the call boundaries at frames 1 and 72
    and changes all its bars exactly at the boundary at frame 65 (calls of 1, 64, 7, 58 frames)."""
    f = mixed_frames(130, 10, 200, seed=5)
    a = np.where((np.arange(64) // 4) & 1, 250, 5).astype(np.uint8)
    b = np.where(((np.arange(64) + 2) // 4) & 1, 250, 5).astype(np.uint8)
    f[:, :, 60:135] = 80                                    # nothing but the bars below makes an edge in the middle cell
    f[0:2, :, 65:129] = a[None, None, :, None]              # open across the boundary at 1
    f[60:65, :, 65:129] = a[None, None, :, None]
    f[65:80, :, 65:129] = b[None, None, :, None]            # every edge moves at 65; the run 65..79 is open across 72 (15 frames)
    return f


def test_calls_chain_through_the_state(ctx):
    import torch
    frames = boundary_clip()
    area = (0, 10, 0, 200)
    p = P._replace(min_frames=2, max_frames=20)
    counts, _ = R.cell_counts(frames, area, p.edge_thresh)
    mid = counts[:, 0, 1]
    assert mid[0, 0] >= p.min_edges and mid[1, 0] >= p.min_edges and mid[1, 1] == mid[1, 2] == 0          # a run open across frame 1
    assert min(mid[64, 0], mid[65, 0]) >= p.min_edges and 2 * (mid[65, 1] + mid[65, 2]) >= mid[64, 0] + mid[65, 1]      # a ratio cut at 65
    assert all(mid[t, 1] == mid[t, 2] == 0 and mid[t, 0] >= p.min_edges for t in range(66, 80))         # a run open across frame 72
    want = R.clip_totals(frames, area, p)
    assert list(want[0, 1]) == [2 + 5 + 15, 3, 22, 1]
    dev = torch.from_numpy(frames).cuda()
    one = run_cells(ctx, dev, area, p)
    assert np.array_equal(one, want)
    assert np.array_equal(run_cells(ctx, dev, area, p, splits=[1, 64, 7, 58]), want)
    assert np.array_equal(run_cells(ctx, dev, area, p, splits=[64, 66]), want)


def test_open_runs_count_after_flush_and_reset_clears(ctx):
    import torch
    frames = boundary_clip()[:75]                           # ends inside the run 65..79
    area = (0, 10, 0, 200)
    p = P._replace(min_frames=2, max_frames=20)
    closed, still_open = R.clip_totals(frames, area, p), R.clip_totals(frames, area, p, flush=False)
    assert list(closed[0, 1]) == [2 + 5 + 10, 3, 17, 1] and list(still_open[0, 1]) == [2 + 5, 2, 17, 1]
    dev = torch.from_numpy(frames).cuda()
    state = ctx.frame_cells_state(10, 200)
    assert np.array_equal(ctx.frame_cells(dev[:40], area, p, state, reset=True).cpu().numpy(), R.clip_totals(frames[:40], area, p, flush=False))
    assert np.array_equal(ctx.frame_cells(dev[40:], area, p, state).cpu().numpy(), still_open)
    assert np.array_equal(ctx.frame_cells(dev[:0], area, p, state).cpu().numpy(), still_open)              # n = 0 without flags: nothing
    assert np.array_equal(ctx.frame_cells(dev[:0], area, p, state, flush=True).cpu().numpy(), closed)      # n = 0, flush: closes them
    assert np.array_equal(ctx.frame_cells(dev[:0], area, p, state, flush=True).cpu().numpy(), closed)      # nothing open any more
    # reset: the totals start from zero and the first frame is compared with an empty mask
    other = frames[60:75]
    got, counts = ctx.frame_cells(dev[60:75], area, p, state, reset=True, flush=True, want_counts=True)
    assert np.array_equal(got.cpu().numpy(), R.clip_totals(other, area, p))
    c = counts.cpu().numpy()
    assert np.array_equal(c, R.cell_counts(other, area, p.edge_thresh)[0])
    assert np.array_equal(c[0, ..., 1], c[0, ..., 0]) and not c[0, ..., 2].any()
    assert int(ctx.frame_cells(dev[:0], area, p, state, reset=True).sum()) == 0 and int(state.words.sum()) == 0      # n = 0, reset


# ---- the automaton on the device -----------------------------------------------------------------------------------------------
def column_frames(sets, h=10, w=66):
    """One cell (8 x 64 interior pixels): frame t shows one-pixel bright columns at the interior columns of sets[t]; a column gives
    two edge columns of 8 rows = 16 edge pixels, and columns 4 apart share none."""
    f = np.full((len(sets), h, w, 3), 20, np.uint8)
    for t, cols in enumerate(sets):
        for c in cols:
            f[t, :, 1 + c] = 240
    return f


def test_run_lengths_at_the_bounds_on_the_device(ctx):
    import torch
    p = R.Params(60, 16, 1, 2, 4, 7)
    on, off = [8], []
    sets = []
    for length in (3, 4, 7, 8):
        sets += [on] * length + [off] * 2
    frames = column_frames(sets)
    area = (0, 10, 0, 66)
    assert list(R.clip_totals(frames, area, p)[0, 0]) == [4 + 7, 2, 22, 0]
    assert list(run_cells(ctx, torch.from_numpy(frames).cuda(), area, p)[0, 0]) == [11, 2, 22, 0]
    for n in (3, 4, 7, 8):                                     # and as the open run that a flush closes
        dev = torch.from_numpy(column_frames([on] * n)).cuda()
        assert list(run_cells(ctx, dev, area, p)[0, 0]) == [n if 4 <= n <= 7 else 0, int(4 <= n <= 7), n, 0]
        assert list(run_cells(ctx, dev, area, p, flush=False)[0, 0]) == [0, 0, n, 0]


@pytest.mark.parametrize("num,den,cut", [(2, 5, True), (409, 1024, True), (410, 1024, False), (1, 2, False), (2, 4, False),
                                         (512, 1024, False), (1, 3, True)])
def test_ratio_test_equality_two_fifths(ctx, num, den, cut):
    """Columns {8,16,24,32} -> {8,16,24,40}: appeared 16, vanished 16, union 80: exactly 2 / 5."""
    import torch
    sets = [[8, 16, 24, 32]] * 3 + [[8, 16, 24, 40]] * 3
    frames = column_frames(sets)
    area = (0, 10, 0, 66)
    c = R.cell_counts(frames, area, 60)[0][:, 0, 0]
    assert list(c[3]) == [64, 16, 16] and c[2, 0] == 64
    p = R.Params(60, 16, num, den, 2, 100)
    want = [6, 2, 6, 1] if cut else [6, 1, 6, 0]
    assert list(R.clip_totals(frames, area, p)[0, 0]) == want
    assert list(run_cells(ctx, torch.from_numpy(frames).cuda(), area, p)[0, 0]) == want


@pytest.mark.parametrize("num,den,cut", [(512, 1024, True), (513, 1024, False), (1, 2, True), (1024, 1024, False), (2147483647, 1, False)])
def test_ratio_test_equality_one_half(ctx, num, den, cut):
    """Columns {8,16,24} -> {8,16,40}: appeared 16, vanished 16, union 64: exactly 512 / 1024."""
    import torch
    frames = column_frames([[8, 16, 24]] * 2 + [[8, 16, 40]] * 2)
    area = (0, 10, 0, 66)
    p = R.Params(60, 16, num, den, 2, 100)
    want = [4, 2, 4, 1] if cut else [4, 1, 4, 0]
    assert list(R.clip_totals(frames, area, p)[0, 0]) == want
    assert list(run_cells(ctx, torch.from_numpy(frames).cuda(), area, p)[0, 0]) == want


# ---- refused arguments -----------------------------------------------------------------------------------------------------------
def test_rejects_bad_arguments_without_touching_the_buffers(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the regions below
    st = torch.zeros(4096, dtype=torch.uint8, device=ctx.tdev)
    tot = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    cnt = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)
    good = dict(n=1, y0=0, y1=10, x0=0, x1=20, num=1, den=2, minf=2, maxf=5, pitch=60)

    def call(**kw):
        a = {**good, **kw}
        return lib.vse_frame_cells(ctx.handle, C.c_void_p(buf.data_ptr()), a["n"], 10, 20, a["pitch"], 600, a["y0"], a["y1"], a["x0"], a["x1"],
                                   128, 16, a["num"], a["den"], a["minf"], a["maxf"], C.c_void_p(st.data_ptr()), 1, 1,
                                   C.c_void_p(tot.data_ptr()), C.c_void_p(cnt.data_ptr()), ctx.stream())
    bad = [dict(y1=2), dict(x0=5, x1=7), dict(y0=-1, y1=5), dict(y1=11), dict(x1=21), dict(y0=4, y1=4), dict(n=-1), dict(num=0),
           dict(den=0), dict(den=1025), dict(minf=0), dict(minf=6, maxf=5), dict(pitch=59)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_frame_cells" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert set(tot.cpu().tolist()) == {-7} and set(cnt.cpu().tolist()) == {-7} and int(st.sum()) == 0      # nothing was enqueued
    assert call() == 0 and call(den=1024, num=1 << 30, minf=1, maxf=1) == 0
    assert tot.cpu().tolist()[:4] == [0, 0, 0, 0] and tot.cpu().tolist()[4] == -7                         # one cell, reset
    gy, gx = C.c_int(-1), C.c_int(-1)
    assert lib.vse_frame_cells_dims(2, 100, C.byref(gy), C.byref(gx)) == -1 and lib.vse_frame_cells_dims(100, 2, C.byref(gy), C.byref(gx)) == -1
    assert (gy.value, gx.value) == (-1, -1)
    assert lib.vse_frame_cells_dims(3, 3, C.byref(gy), C.byref(gx)) == 0 and (gy.value, gx.value) == (1, 1)
    assert lib.vse_frame_cells_dims(1080, 1920, C.byref(gy), C.byref(gx)) == 0 and (gy.value, gx.value) == (135, 30)
    assert lib.vse_frame_cells_state_bytes(2, 100) == 0 and lib.vse_frame_cells_state_bytes(3, 3) == 72
    assert lib.vse_frame_cells_state_bytes(11, 67) == 2 * 2 * 72


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def located_reference():
    from area_clip import FPS, LOCATOR, decorated_clip
    from vse_amd import area_locator
    frames, _truth = decorated_clip()
    p = area_locator.AreaLocator(**LOCATOR).params(FPS)
    totals = R.clip_totals(frames, (0, 360, 0, 640), p)
    return frames, p, totals, R.locate(totals, len(frames), (0, 360, 0, 640), (360, 640))


@pytest.mark.parametrize("staged", [False, True])
def test_locator_on_the_engine(ctx, located_reference, staged):
    from area_clip import FPS, LOCATOR, as_tuple
    from vse_amd import area_locator, staging
    frames, _p, totals, want = located_reference
    up = staging.Uploader(ctx.tdev, ctx=ctx) if staged else None
    loc = area_locator.AreaLocator(area_locator.EngineCells(ctx), batch=16, **LOCATOR)
    try:
        area = loc.run(iter(frames), FPS, uploader=up)
    finally:
        if up is not None:
            up.close()
    assert np.array_equal(loc.totals, totals) and loc.frames_scanned == len(frames)
    assert as_tuple(area) == want and want[0] <= 328 and want[1] >= 348


def test_locator_on_the_engine_from_y4m(ctx, located_reference, tmp_path):
    from area_clip import FPS, LOCATOR, as_tuple
    from vse_amd import area_locator, ingest, staging
    frames, p, _totals, _want = located_reference
    path = tmp_path / "clip.y4m"
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(str(path))
    seen = np.stack([f.to_bgr() for f in src.raw_frames()])                  # what the device converts the planes to
    totals = R.clip_totals(seen, (0, 360, 0, 640), p)
    want = R.locate(totals, len(seen), (0, 360, 0, 640), (360, 640))
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    loc = area_locator.AreaLocator(area_locator.EngineCells(ctx), batch=16, **LOCATOR)
    try:
        area = loc.run(src.raw_frames(), src.fps, uploader=up)
    finally:
        up.close()
        src.close()
    assert np.array_equal(loc.totals, totals)
    assert want is not None and as_tuple(area) == want and want[0] <= 328 and want[1] >= 348
