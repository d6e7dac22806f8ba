"""vse_colour_key on the MI355X: the bytes of both forms equal the numpy restatement (tests/colour_key_ref.py) and nothing else is
touched, every refusal leaves the output alone, the selectors' kernels over Context.colour_key's output equal their numpy references over
the reference key, and ChangeFrameSelector(key_fn=EngineKey) through a real uploader finds the subtitles of the coloured clip."""
import ctypes as C

import numpy as np
import pytest

import colour_key_ref as ref

pytestmark = pytest.mark.gpu
FILL = 0xA5
E_INVAL = -1


def call(ctx, src, dst, base, obase, n, h, w, pitch, fstride, area, key, slope, opitch=None, ofstride=None):
    """vse_colour_key on flat cuda uint8 buffers: frames at src + base, output at dst + obase."""
    y0, y1, x0, x1 = area
    opitch, ofstride = pitch if opitch is None else opitch, fstride if ofstride is None else ofstride
    return ctx.lib.vse_colour_key(ctx.handle, C.c_void_p(src.data_ptr() + base), n, h, w, pitch, fstride, y0, y1, x0, x1, *key, slope,
                                  C.c_void_p(dst.data_ptr() + obase), opitch, ofstride, ctx.stream())


def check(ctx, n, h, w, pitch, base, area, key, slope, seed, frames=None):
    """Random frames in a buffer of 0xA5 with one frame of room behind the last; the output buffer is all 0xA5 before the call."""
    import torch
    rng = np.random.default_rng(seed)
    fstride = h * pitch + (16 if pitch % 16 == 0 else 5)
    if pitch % 16 == 0:
        fstride = (fstride + 15) // 16 * 16
    size = base + (n + 1) * fstride + 64
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) if frames is None else frames
    idx = (base + np.arange(n)[:, None, None, None] * fstride + np.arange(h)[None, :, None, None] * pitch
           + np.arange(w)[None, None, :, None] * 3 + np.arange(3)[None, None, None, :])
    host = np.full(size, FILL, np.uint8)
    host[idx] = frames
    src, dst = torch.from_numpy(host).to(ctx.tdev), torch.full((size,), FILL, dtype=torch.uint8, device=ctx.tdev)
    assert call(ctx, src, dst, base, base, n, h, w, pitch, fstride, area, key, slope) == 0
    out = dst.cpu().numpy()
    assert np.array_equal(src.cpu().numpy(), host)                                    # the input comes back unchanged
    y0, y1, x0, x1 = area
    want = np.repeat(ref.key_plane(frames, key, slope).astype(np.uint8)[..., None], 3, -1)
    assert np.array_equal(out[idx[:, y0:y1, x0:x1]], want[:, y0:y1, x0:x1])           # the area is written in full
    rows = out[idx[:, y0:y1]]
    assert np.all((rows == FILL) | (rows == want[:, y0:y1]))                          # its rows: untouched, or the key of the pixel there
    other = np.ones(size, bool)
    other[idx[:, y0:y1].ravel()] = False
    assert np.all(out[other] == FILL)                                                 # other rows, row padding, the frame behind the last
    return out[idx]


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("base", (1, 2))
@pytest.mark.parametrize("h, w, area", ((3, 3, (1, 2, 1, 2)), (5, 7, (1, 4, 2, 5)), (7, 41, (1, 6, 1, 24))))
def test_general_form(ctx, n, base, h, w, area):
    check(ctx, n, h, w, 3 * w + 4 + (w % 2 == 0), base, area, (0, 255, 255), ref.slope_of(48), seed=n + base + h)


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("h, w", ((4, 32), (10, 80)))
@pytest.mark.parametrize("x0", (0, 5, 16))
def test_fast_form(ctx, n, h, w, x0):
    pitch = 3 * w + 16
    assert pitch % 16 == 0
    for x1 in sorted({w, w - 16, w - 3, x0 + 1} - set(range(x0 + 1))):     # ending on and off a 16-pixel boundary
        for y0, y1 in ((0, h), (1, h - 1)):
            check(ctx, n, h, w, pitch, 0, (y0, y1, x0, x1), (200, 30, 90), ref.slope_of(127), seed=x0 + x1 + y0)


def test_fast_form_frame_edge_cuts_a_group(ctx):
    """A width that is no multiple of 16 with aligned pitches: the last group of a row goes pixel by pixel and stops at the frame's edge."""
    for w in (33, 47):
        check(ctx, 2, 5, w, (3 * w + 15) // 16 * 16 + 16, 0, (1, 4, 3, w), (255, 255, 255), ref.slope_of(24), seed=w)
        check(ctx, 2, 5, w, (3 * w + 15) // 16 * 16 + 16, 0, (0, 5, w - 1, w), (255, 255, 255), ref.slope_of(24), seed=w + 1)


@pytest.mark.parametrize("pitch_pad, base", ((16, 0), (7, 1)))
def test_every_distance(ctx, pitch_pad, base):
    """One frame whose B channel runs 0..255 against key 0: d takes every value, in both forms."""
    frames = np.zeros((1, 2, 256, 3), np.uint8)
    frames[0, :, :, 0] = np.arange(256)
    frames[0, 1, :, 2] = np.arange(256)[::-1] // 2                         # (second row: R is the larger distance on its left half)
    for tol in (1, 2, 24, 48, 127, 255):
        got = check(ctx, 1, 2, 256, 768 + pitch_pad, base, (0, 2, 0, 256), (0, 0, 0), ref.slope_of(tol), seed=0, frames=frames)
        assert np.array_equal(got[0, 0, :, 0], ref.key_of_distance(np.arange(256), ref.slope_of(tol)))


@pytest.mark.parametrize("seed", range(4))
def test_random_keys_and_slopes(ctx, seed):
    rng = np.random.default_rng(100 + seed)
    for slope in (256, 65280, int(rng.integers(256, 65281))):
        key = tuple(int(v) for v in rng.integers(0, 256, 3))
        check(ctx, 2, 6, 48, 160, 0, (1, 5, 7, 40), key, slope, seed=seed)
        check(ctx, 2, 6, 45, 141, 2, (1, 5, 7, 40), key, slope, seed=seed)
    check(ctx, 2, 40, 101, 305, 1, (3, 37, 5, 99), (9, 99, 199), 1360, seed=seed)          # the general form over several blocks
    for key in ((0, 0, 0), (255, 255, 255), (0, 255, 0)):
        check(ctx, 1, 4, 32, 112, 0, (0, 4, 0, 32), key, 65280, seed=seed)


def test_refusals(ctx):
    import torch
    n, h, w, pitch = 2, 6, 20, 64
    fstride = h * pitch
    src = torch.full((4 * fstride,), 7, dtype=torch.uint8, device=ctx.tdev)
    dst = torch.full((4 * fstride,), FILL, dtype=torch.uint8, device=ctx.tdev)
    good = dict(n=n, h=h, w=w, pitch=pitch, fstride=fstride, area=(1, 5, 2, 18), key=(0, 255, 255), slope=1360)
    assert call(ctx, src, dst, 0, 0, **good) == 0
    dst.fill_(FILL)
    bad = [dict(area=a) for a in ((3, 3, 2, 18), (1, 5, 9, 9), (4, 2, 2, 18), (-1, 5, 2, 18), (1, 7, 2, 18), (1, 5, -1, 18), (1, 5, 2, 21))]
    bad += [dict(key=k) for k in ((-1, 0, 0), (0, 256, 0), (0, 0, 300))]
    bad += [dict(slope=s) for s in (255, 65281, 0, -5)]
    bad += [dict(pitch=59), dict(opitch=59), dict(n=-1)]
    for change in bad:
        assert call(ctx, src, dst, 0, 0, **{**good, **change}) == E_INVAL, change
        assert ctx.lib.vse_last_error()
    # overlapping byte ranges: in place, the output starting inside the input's last frame, and the input inside the output
    assert call(ctx, src, src, 0, 0, **good) == E_INVAL
    assert call(ctx, src, src, 0, fstride + 3 * pitch, **good) == E_INVAL              # (its first row begins in the input's last row)
    assert call(ctx, src, src, 2 * fstride, fstride, **good) == E_INVAL
    assert call(ctx, src, src, 0, 2 * fstride, **good) == 0                # side by side in one buffer is no overlap
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())
    assert call(ctx, src, dst, 0, 0, **{**good, "n": 0}) == 0 and bool((dst == FILL).all())      # n == 0: success without a launch
    assert call(ctx, src, dst, 0, 0, **{**good, "area": (2, 3, 4, 5)}) == 0                      # 1 x 1 is allowed


# ---- on a cut of the coloured clip ------------------------------------------------------------------------------------------
AREA = (60, 120, 0, 320)
TRUE = [(8, 27), (28, 45), (52, 76), (77, 90)]


@pytest.fixture(scope="module")
def coloured():
    """test_colour_key's clip: 120 x 320, its first 90 frames, and their reference key over the band."""
    from test_frame_hold import MOVING
    from vse_amd import frame_select, synth
    frames, _ = synth.make_moving_clip(MOVING, amp=(120, 120), text_bgr=(0, 255, 255), outline=False, chroma=True)
    frames = frames[:90]
    key = frame_select.ColourKey("yellow", 48)
    keyed = ref.colour_key(frames, AREA, key.bgr, key.slope)
    frames.setflags(write=False)
    keyed.setflags(write=False)
    return frames, keyed, key


def test_context_colour_key(ctx, coloured):
    import torch
    frames, keyed, key = coloured
    dev = torch.from_numpy(np.array(frames)).to(ctx.tdev)
    out = ctx.colour_key(dev, AREA, key)
    assert out.shape == dev.shape and out.dtype == torch.uint8 and out.is_cuda
    assert np.array_equal(out[:, 60:120].cpu().numpy(), keyed[:, 60:120])
    assert np.array_equal(dev.cpu().numpy(), frames)
    again = torch.full_like(dev, FILL)
    assert ctx.colour_key(dev, (70, 100, 33, 200), key, out=again) is again
    got = again.cpu().numpy()
    assert np.array_equal(got[:, 70:100, 33:200], keyed[:, 70:100, 33:200]) and np.all(got[:, :70] == FILL) and np.all(got[:, 100:] == FILL)


def test_the_selectors_kernels_on_the_keyed_band(ctx, coloured):
    import torch
    from frame_change_ref import counts as change_counts
    from frame_focus_ref import focus as focus_rows
    from frame_hold_ref import counts as hold_counts
    from vse_amd import frame_select
    frames, keyed, key = coloured
    out = ctx.colour_key(torch.from_numpy(np.array(frames)).to(ctx.tdev), AREA, key)
    for thresh in (64, 128):
        got = frame_select.EngineCounter(ctx)(out, AREA, thresh, True).cpu().numpy()
        assert np.array_equal(got, change_counts(keyed, AREA, thresh)[0])
        got = frame_select.EngineFocus(ctx)(out, AREA, thresh, True).cpu().numpy()
        assert np.array_equal(got, focus_rows(keyed, AREA, thresh)[0])
        got = frame_select.EngineHoldCounter(ctx)(out, AREA, thresh, 5, 0, True).cpu().numpy()
        assert np.array_equal(got, hold_counts(keyed, AREA, thresh, 5))
    assert change_counts(keyed, AREA, 128)[0][:, 0].max() > 200


def test_change_selector_with_engine_key_through_an_uploader(ctx, coloured):
    from frame_change_ref import counts as change_counts
    from test_frame_hold import BAND
    from vse_amd import frame_select, staging
    frames, keyed, key = coloured
    sel = frame_select.ChangeFrameSelector(frame_select.EngineCounter(ctx), key_fn=frame_select.EngineKey(ctx, key), batch=40)
    got = sel.run(list(frames), BAND, 25.0, uploader=staging.Uploader(ctx.tdev))
    assert [(s, e) for s, e, _r in got] == TRUE
    assert np.array_equal(sel.counts, change_counts(keyed, AREA, 128)[0])
    plain = frame_select.ChangeFrameSelector(frame_select.EngineCounter(ctx), batch=40).run(list(frames), BAND, 25.0)
    assert [(s, e) for s, e, _r in plain] != TRUE
