"""vse_interval_accumulate / vse_interval_composite on the MI355X: every byte of the device composites equals the numpy restatement
(tests/interval_ref.py) in all three modes, for every width and byte alignment, through the 16-byte and the general loads alike;
batches chained through the state equal one call; nothing outside the output is written; refusals touch nothing; and
IntervalCompositor on the engine gives the patches of the run fed by the numpy restatement."""
import ctypes as C

import numpy as np
import pytest

import interval_ref

pytestmark = pytest.mark.gpu


def dev_composites(ctx, batches, area, state=None, resets=None):
    """batches: cuda uint8 [n,H,W,3] views fed one after the other through one state (the first with reset, or as `resets` says)
    -> {mode: host uint8 [ah, aw, 3]} of the frames since the last reset."""
    y0, y1, x0, x1 = area
    state = ctx.interval_state(y1 - y0, x1 - x0) if state is None else state
    count = 0
    for k, b in enumerate(batches):
        reset = (k == 0) if resets is None else resets[k]
        ctx.interval_accumulate(b, area, state, reset=reset)
        count = b.shape[0] if reset else count + b.shape[0]
    return {m: ctx.interval_composite(state, y1 - y0, x1 - x0, count, m).cpu().numpy() for m in interval_ref.MODES}


def ref_composites(frames, area):
    st = interval_ref.accumulate(None, frames, area)
    return {m: interval_ref.composite(st, len(frames), m) for m in interval_ref.MODES}


def same(got, want, what):
    for m in interval_ref.MODES:
        assert got[m].dtype == np.uint8 and np.array_equal(got[m], want[m]), (what, m)


def padded_view(ctx, frames, row_pad, lead, frame_rows_extra):
    """The same pixels in a strided view: rows `row_pad` bytes longer, starting `lead` bytes into their row, frames further apart."""
    import torch
    n, h, w, _ = frames.shape
    pitch = 3 * w + row_pad
    buf = torch.full((n, h + frame_rows_extra, pitch), 0x5A, dtype=torch.uint8, device=ctx.tdev)
    view = buf[:, 1:1 + h, lead:lead + 3 * w].view(n, h, w, 3)
    view.copy_(torch.from_numpy(frames))
    assert view.stride(1) == pitch and view.stride(0) == (h + frame_rows_extra) * pitch > h * pitch
    return view


@pytest.mark.parametrize("area_h", [1, 2, 9])
def test_every_width_and_alignment(ctx, area_h):
    """area_w 1..17 at x0 0..5: 3 x0 and 3 area_w take every residue mod 4 and mod 16; 11 x 37 frames (pitch 111, so every row starts
    on another residue), packed and in a view with a padded pitch (116 + an odd lead) and a frame stride above h * pitch."""
    import torch
    frames = np.random.default_rng(area_h).integers(0, 256, size=(5, 11, 37, 3), dtype=np.uint8)
    packed = torch.from_numpy(frames).to(ctx.tdev)
    padded = padded_view(ctx, frames, 5, 3, 2)
    assert {3 * x % 16 for x in range(6)} | {3 * w % 16 for w in range(1, 18)} == set(range(16))
    for area_w in range(1, 18):
        for x0 in range(6):
            area = (1, 1 + area_h, x0, x0 + area_w)
            want = ref_composites(frames, area)
            same(dev_composites(ctx, [packed], area), want, ("packed", area))
            same(dev_composites(ctx, [padded], area), want, ("padded", area))


@pytest.mark.parametrize("x0, area_w", [(0, 64), (16, 37), (0, 63), (32, 32)])
def test_wide_loads_equal_general_loads(ctx, x0, area_w):
    """src_w 64 with 16-byte aligned base, pitch and frame stride, 3 x0 a multiple of 16: the 16-byte loads (with the general load on
    the short run that ends a row, where 3 area_w is no multiple of 16).  The same pixels one pixel further into a buffer are misaligned
    and take the general loads: identical bytes."""
    import torch
    n, h, w = 11, 6, 64
    frames = np.random.default_rng(x0 + area_w).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    area = (0, h, x0, x0 + area_w)
    aligned = torch.from_numpy(frames).to(ctx.tdev)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(1) % 16 == 0 and aligned.stride(0) % 16 == 0 and 3 * x0 % 16 == 0
    flat = torch.zeros(frames.size + 16, dtype=torch.uint8, device=ctx.tdev)
    shifted = flat[3:3 + frames.size].view(n, h, w, 3)
    shifted.copy_(aligned)
    assert shifted.data_ptr() % 16 == 3
    want = ref_composites(frames, area)
    wide, general = dev_composites(ctx, [aligned], area), dev_composites(ctx, [shifted], area)
    same(wide, want, "wide")
    same(general, want, "general")
    one = dev_composites(ctx, [aligned[:1]], area)                                    # n = 1: no frame stride to be aligned
    same(one, ref_composites(frames[:1], area), "one frame")


@pytest.mark.parametrize("aligned", [True, False])
def test_batches_chain_through_state(ctx, aligned):
    """75 frames as 1 + 7 + 64 + 3 calls and as one call; a reset in the middle starts over."""
    import torch
    n, h, w = 75, 5, 48 if aligned else 45
    frames = np.random.default_rng(75).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    area = (1, 4, 0, w) if aligned else (1, 4, 2, 43)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    want = ref_composites(frames, area)
    whole = dev_composites(ctx, [dev], area)
    parts = dev_composites(ctx, [dev[0:1], dev[1:8], dev[8:72], dev[72:75]], area)
    same(whole, want, "one call")
    same(parts, want, "1 + 7 + 64 + 3")
    again = dev_composites(ctx, [dev[0:1], dev[1:8], dev[8:72], dev[72:75]], area, resets=[True, False, True, False])
    same(again, ref_composites(frames[8:], area), "reset at frame 8")


def test_state_needs_no_content_before_a_reset(ctx):
    import torch
    frames = np.random.default_rng(9).integers(0, 256, size=(3, 4, 21, 3), dtype=np.uint8)
    area = (0, 4, 1, 20)
    state = ctx.interval_state(4, 19)
    state.fill_(0xC3)
    same(dev_composites(ctx, [torch.from_numpy(frames).to(ctx.tdev)], area, state=state), ref_composites(frames, area), "dirty state")


def test_range_of_values(ctx):
    import torch
    area = (0, 2, 0, 16)
    # all 255 over 300 frames: the sums pass 16 bits; all 0
    for value, n in ((255, 300), (0, 9)):
        frames = np.full((n, 2, 16, 3), value, np.uint8)
        got = dev_composites(ctx, [torch.from_numpy(frames).to(ctx.tdev)], area)
        assert all((got[m] == value).all() for m in interval_ref.MODES), value
    assert 255 * 300 > 65535
    # a ramp: the 48 bytes of a 16-pixel run all differ (b -> b (5 + 2 f) + f mod 256, an odd factor) and move differently per frame
    b = np.arange(48, dtype=np.int64).reshape(16, 3)
    ramp = np.stack([np.stack([(b * (5 + 2 * f) + f + 11 * r) % 256 for r in range(2)]) for f in range(13)]).astype(np.uint8)
    assert all(len(set(ramp[f, r].ravel().tolist())) == 48 for f in range(13) for r in range(2))
    want = ref_composites(ramp, area)
    assert len({tuple(want["min"][0].ravel()[k::16]) for k in range(16)}) == 16
    dev = torch.from_numpy(ramp).to(ctx.tdev)
    same(dev_composites(ctx, [dev], area), want, "ramp, 16-byte loads")
    off = torch.zeros(ramp.size + 8, dtype=torch.uint8, device=ctx.tdev)
    shifted = off[1:1 + ramp.size].view(ramp.shape)
    shifted.copy_(dev)
    same(dev_composites(ctx, [shifted], area), want, "ramp, general loads")


def test_mean_rounds_halves_up(ctx):
    import torch
    a = np.arange(255, dtype=np.uint8).reshape(1, 85, 3)                             # every value 0..254
    two = np.stack([a, a + 1])                                                       # sm = 2 a + 1: the mean is a + 1/2
    four = np.stack([a, a + 1, a + 1, a])                                            # sm = 4 a + 2
    assert (four.astype(np.int64).sum(0) % 4 == 2).all()
    for frames in (two, four):
        area = (0, 1, 0, 85)
        got = dev_composites(ctx, [torch.from_numpy(frames).to(ctx.tdev)], area)
        assert np.array_equal(got["mean"], a + 1), len(frames)
        same(got, ref_composites(frames, area), len(frames))


def test_writes_only_the_output(ctx):
    import torch
    frames = np.random.default_rng(2).integers(0, 256, size=(4, 7, 29, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (2, 7, 3, 26)
    ah, aw = 5, 23
    want = ref_composites(frames, area)
    state = ctx.interval_state(ah, aw)
    ctx.interval_accumulate(dev, area, state, reset=True)
    for lead, pitch in ((5, 3 * aw + 7), (16, 3 * aw + 11), (0, 3 * aw)):
        for m in interval_ref.MODES:
            buf = torch.full((ah + 2, pitch + lead), 0xA5, dtype=torch.uint8, device=ctx.tdev)
            out = buf[1:1 + ah, lead:lead + 3 * aw].view(ah, aw, 3)
            assert ctx.interval_composite(state, ah, aw, 4, m, out=out) is out
            host = buf.cpu().numpy()
            assert np.array_equal(host[1:1 + ah, lead:lead + 3 * aw].reshape(ah, aw, 3), want[m]), (lead, pitch, m)
            host[1:1 + ah, lead:lead + 3 * aw] = 0xA5
            assert (host == 0xA5).all(), (lead, pitch, m)                             # row gaps and the rows around: the canary
    assert np.array_equal(dev.cpu().numpy(), frames)                                  # the input is read only


def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)                    # far larger than any of the frames below
    st = torch.full((4096,), 0xA5, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=ctx.tdev)

    def acc(n=1, h=10, w=20, pitch=60, fstride=600, y0=0, y1=10, x0=0, x1=20):
        return lib.vse_interval_accumulate(ctx.handle, C.c_void_p(buf.data_ptr()), n, h, w, pitch, fstride, y0, y1, x0, x1,
                                           C.c_void_p(st.data_ptr()), 1, ctx.stream())

    def comp(ah=4, aw=5, frames=1, mode=0, pitch=15):
        return lib.vse_interval_composite(ctx.handle, C.c_void_p(st.data_ptr()), ah, aw, frames, mode, C.c_void_p(out.data_ptr()), pitch,
                                          ctx.stream())

    for kw in (dict(y0=4, y1=4), dict(x0=7, x1=7), dict(y0=5, y1=3), dict(y0=-1), dict(x0=-1), dict(y1=11), dict(x1=21),      # empty / outside
               dict(n=0), dict(n=-1), dict(n=65536), dict(pitch=59)):
        assert acc(**kw) == -1, kw
        assert "vse_interval_accumulate" in lib.vse_last_error().decode()
    for kw in (dict(mode=3), dict(mode=-1), dict(frames=0), dict(frames=4194305), dict(pitch=14), dict(ah=0), dict(aw=0)):
        assert comp(**kw) == -1, kw
        assert "vse_interval_composite" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert int((st != 0xA5).sum()) == 0 and int((out != 0xA5).sum()) == 0 and int(buf.sum()) == 0      # nothing was enqueued
    assert lib.vse_interval_state_bytes(0, 5) == 0 and lib.vse_interval_state_bytes(5, 0) == 0 and lib.vse_interval_state_bytes(-1, -1) == 0
    assert lib.vse_interval_state_bytes(2, 5) == 2 * 16 * 6 and lib.vse_interval_state_bytes(3, 16) == 3 * 48 * 6
    assert acc(n=65535, fstride=0, h=1, w=1, pitch=3, y1=1, x1=1) == -1                # (frames may not overlap: the stride is checked too)
    assert acc() == 0 and comp(frames=4194304, mode=2) == 0                            # the limits themselves are accepted
    torch.cuda.synchronize()


@pytest.mark.parametrize("staged", [False, True])
def test_compositor_on_engine(ctx, staged):
    """IntervalCompositor with the default-style EngineCompositor (area rows only, batches of 4, with and without the uploader) gives the
    patches of the run fed by the numpy restatement."""
    from vse_amd import extractor, frame_select, staging, synth
    h, w = 120, 200
    frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", 9), ("seven wizards", 7, 2), (None, 3), ("near frozen lakes", 6)], h, w, seed=6)
    ivs = [(s, e, (s + e) // 2) for s, e, _t in truth]
    area = extractor.SubtitleArea(ymin=int(0.7 * h), ymax=h, xmin=7, xmax=w - 4)
    up = staging.Uploader(ctx.tdev) if staged else None
    for mode in interval_ref.MODES:
        want = frame_select.IntervalCompositor(interval_ref.NumpyCompositor(), mode=mode, trim_seconds=0.1, batch=4).run(list(frames), area, ivs, 10.0)
        comp = frame_select.IntervalCompositor(frame_select.EngineCompositor(ctx), mode=mode, trim_seconds=0.1, batch=4)
        got = comp.run(list(frames), area, ivs, 10.0, uploader=up)
        assert sorted(got) == sorted(want) == [r for _s, _e, r in ivs]
        assert all(got[r].dtype == np.uint8 and np.array_equal(got[r], want[r]) for r in want), mode
    if up is not None:
        up.close()
