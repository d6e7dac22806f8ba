"""vse_frame_focus on the MI355X, through the C ABI: the rows equal the numpy restatement (tests/frame_focus_ref.py) bit for bit on the
smallest areas and frame counts at which the kernel takes another path (one pixel, either side of a 64-column word and an 8-row tile,
either side of the eight waves' shares of the frames), batches chained through the state equal one call, the state passes between
vse_frame_change and vse_frame_focus, what is refused launches nothing; then frame_select.EngineFocus under the change selector, and
SubtitleExtractor(interval_frame="sharpest") on the engine in one pass against several passes."""
import ctypes as C

import numpy as np
import pytest

from frame_change_ref import counts as ref_counts
from frame_focus_ref import NumpyFocus, focus as ref_focus

pytestmark = pytest.mark.gpu

GARBAGE = -1234567
THRESHOLDS = (1, 128, 255)


def raw_focus(ctx, frames, area, thresh, state, reset=False, n=None, src_hw=None, out=None):
    """The C entry itself on a cuda uint8 [n,H,W,3] view -> (return code, the int32 [n,2] tensor it was given, pre-filled with garbage)."""
    import torch
    y0, y1, x0, x1 = area
    n = frames.shape[0] if n is None else n
    h, w = frames.shape[1:3] if src_hw is None else src_hw
    if out is None:
        out = torch.full((max(n, 1), 2), GARBAGE, dtype=torch.int32, device=ctx.tdev)
    rc = ctx.lib.vse_frame_focus(ctx.handle, C.c_void_p(frames.data_ptr()), n, h, w, frames.stride(1), frames.stride(0), y0, y1, x0, x1, thresh,
                                 C.c_void_p(state.data_ptr()), int(reset), C.c_void_p(out.data_ptr()), ctx.stream())
    return rc, out


def dev_focus(ctx, frames, area, thresh, splits=None, resets=()):
    """host int64 [n,2] of the frames fed through ONE fresh state in calls of `splits` frames; resets: the calls (by index) given `reset`."""
    y0, y1, x0, x1 = area
    state = ctx.frame_change_state(y1 - y0, x1 - x0)
    rows, at = [], 0
    for k, n in enumerate(splits or [frames.shape[0]]):
        rc, out = raw_focus(ctx, frames[at:at + n], area, thresh, state, reset=k in resets)
        assert rc == 0, ctx.lib.vse_last_error().decode()
        rows.append(out.cpu().numpy().astype(np.int64))
        at += n
    assert at == frames.shape[0]
    return np.concatenate(rows)


def draws(n, h, w, seed):
    """Random uint8 frames; every third is stretched to full contrast (each pixel black or white, so that the threshold of 255 finds edges
    too), and every odd frame repeats the left half of the one before it (so that edges stand from one frame to the next)."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f[2::3] = (rng.integers(0, 2, size=(n, h, w, 1), dtype=np.uint8) * 255)[2::3]
    for i in range(1, n, 2):
        f[i, :, :(w + 1) // 2] = f[i - 1, :, :(w + 1) // 2]
    return f


# interior height x width: one pixel; either side of a word of 64 columns and of a tile of 8 rows; more than two words, more than two tiles
@pytest.mark.parametrize("ih,iw", [(1, 1), (7, 63), (8, 64), (9, 65), (17, 130), (8, 130), (17, 63), (7, 65)])
def test_rows_match_numpy_on_every_tile_edge(ctx, ih, iw):
    import torch
    frames = draws(6, ih + 2, iw + 2, seed=ih * 1000 + iw)
    dev = torch.from_numpy(frames).cuda()
    area = (0, ih + 2, 0, iw + 2)
    for thresh in THRESHOLDS:
        want, _ = ref_focus(frames, area, thresh)
        assert np.array_equal(dev_focus(ctx, dev, area, thresh), want), thresh
        assert want[0].tolist() == [0, 0]                                       # a fresh state: nothing stood before the first frame
        assert ih * iw == 1 or want[:, 1].max() > 0, thresh                      # every threshold does find standing edges


def test_area_off_origin_in_a_padded_frame_and_rows_alone(ctx):
    import torch
    frames = draws(7, 37, 150, seed=7)
    area = (3, 33, 5, 148)                                                       # odd x0; interior 28 x 141
    padded = torch.zeros((7, 41, 163 * 3 + 5), dtype=torch.uint8, device=ctx.tdev)      # padded rows inside padded frames
    view = padded[:, 3:40, 6:6 + 450].view(7, 37, 150, 3)
    view.copy_(torch.from_numpy(frames))
    assert view.stride(1) == 163 * 3 + 5 != 3 * (area[3] - area[2]) and view.stride(0) == 41 * (163 * 3 + 5)
    band = torch.from_numpy(np.ascontiguousarray(frames[:, 3:33])).cuda()              # the area's rows alone
    for thresh in THRESHOLDS:
        want, _ = ref_focus(frames, area, thresh)
        assert want[:, 1].max() > 0
        assert np.array_equal(dev_focus(ctx, view, area, thresh), want), thresh
        assert np.array_equal(dev_focus(ctx, band, (0, 30, 5, 148), thresh), want), thresh


@pytest.fixture(scope="module")
def long_clip():
    """130 frames of 12 x 70 pixels (two tiles by two words) and their rows at 128, computed once and left alone."""
    frames = draws(130, 12, 70, seed=130)
    want, _ = ref_focus(frames, (0, 12, 0, 70), 128)
    want.setflags(write=False)
    return frames, want


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 63, 64, 65, 130])
def test_frame_counts_around_the_waves_shares(ctx, long_clip, n):
    import torch
    frames, want = long_clip
    got = dev_focus(ctx, torch.from_numpy(frames[:n]).cuda(), (0, 12, 0, 70), 128)
    assert np.array_equal(got, want[:n]) and (n < 2 or want[:n, 1].max() > 0)


def test_batches_chain_through_the_state_and_reset_cuts(ctx, long_clip):
    import torch
    frames, want = long_clip
    dev = torch.from_numpy(frames).cuda()
    area = (0, 12, 0, 70)
    assert np.array_equal(dev_focus(ctx, dev, area, 128, splits=[1, 64, 65]), want)
    assert np.array_equal(dev_focus(ctx, dev, area, 128, splits=[3] * 43 + [1]), want)
    cut = dev_focus(ctx, dev, area, 128, splits=[1, 64, 65], resets=(1,))
    again, _ = ref_focus(frames[1:], area, 128)                                  # the second call starts over: its first frame meets no mask
    assert np.array_equal(cut[1:], again) and cut[1].tolist() == [0, 0] and want[1, 0] > 0
    assert np.array_equal(cut[:1], want[:1])


@pytest.mark.parametrize("ih,iw", [(8, 64), (9, 130)])
def test_period_four_columns_keep_every_pixel_at_full_gradient(ctx, ih, iw):
    import torch
    row = np.tile(np.array([0, 0, 255, 255], np.uint8), (iw + 2 + 3) // 4)[:iw + 2]
    frames = np.broadcast_to(row[None, None, :, None], (4, ih + 2, iw + 2, 3)).copy()
    dev = torch.from_numpy(frames).cuda()
    for thresh in THRESHOLDS:
        got = dev_focus(ctx, dev, (0, ih + 2, 0, iw + 2), thresh)
        assert got.tolist() == [[0, 0]] + [[ih * iw, 255 * ih * iw]] * 3, thresh
        assert np.array_equal(got, ref_focus(frames, (0, ih + 2, 0, iw + 2), thresh)[0])


def test_state_passes_between_frame_change_and_frame_focus(ctx):
    import torch
    frames = draws(15, 21, 140, seed=15)
    area = (1, 20, 2, 139)
    dev = torch.from_numpy(frames).cuda()
    want_counts, _ = ref_counts(frames, area, 100)
    want_focus, _ = ref_focus(frames, area, 100)
    parts = [slice(0, 5), slice(5, 10), slice(10, 15)]
    for focus_first in (False, True):
        state = ctx.frame_change_state(area[1] - area[0], area[3] - area[2])
        for k, part in enumerate(parts):
            if (k % 2 == 0) == focus_first:
                rc, out = raw_focus(ctx, dev[part], area, 100, state)
                assert rc == 0 and np.array_equal(out.cpu().numpy(), want_focus[part]), (focus_first, k)
            else:
                got = ctx.frame_change(dev[part], area, 100, state).cpu().numpy()
                assert np.array_equal(got, want_counts[part]), (focus_first, k)
    assert want_focus[5, 0] > 0 and want_focus[10, 0] > 0                        # the rows at the hand-overs do depend on the mask handed over


def test_refused_arguments_launch_nothing(ctx):
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev).view(1, -1, 1, 1)        # far larger than any area that could be launched
    st = torch.zeros(4096, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4, 2), GARBAGE, dtype=torch.int32, device=ctx.tdev)

    def call(n, h, w, pitch, fstride, y0, y1, x0, x1):
        return ctx.lib.vse_frame_focus(ctx.handle, C.c_void_p(buf.data_ptr()), n, h, w, pitch, fstride, y0, y1, x0, x1, 128,
                                       C.c_void_p(st.data_ptr()), 0, C.c_void_p(out.data_ptr()), ctx.stream())
    assert call(0, 10, 20, 60, 600, 0, 10, 0, 20) == -1                          # n = 0
    assert call(-1, 10, 20, 60, 600, 0, 10, 0, 20) == -1
    assert call(1, 10, 20, 60, 600, 0, 2, 0, 5) == -1 and "area" in ctx.lib.vse_last_error().decode()       # a 2 x 5 area
    assert call(1, 10, 20, 60, 600, 0, 11, 0, 10) == -1 and "area" in ctx.lib.vse_last_error().decode()     # out of the frame
    assert call(1, 10, 20, 60, 600, 0, 10, 15, 21) == -1
    # an interior of 2^23 + 1 pixels, by the arguments alone: one row of them in a frame that is never read
    wide = (1 << 23) + 1 + 2
    assert call(1, 3, wide, 3 * wide, 9 * wide, 0, 3, 0, wide) == -1 and "2^23" in ctx.lib.vse_last_error().decode()
    assert call(1, 2050, 4100, 3 * 4100, 3 * 4100 * 2050, 0, 2050, 0, 4099) == -1            # 2048 x 4097 = 2^23 + 2048
    torch.cuda.synchronize()
    assert bool((out == GARBAGE).all()) and int(st.sum()) == 0                  # nothing was enqueued
    assert call(1, 10, 20, 60, 600, 0, 10, 0, 20) == 0                           # the same buffers, accepted
    assert out.cpu().numpy().tolist() == [[0, 0]] + [[GARBAGE, GARBAGE]] * 3


def test_engine_focus_under_the_change_selector(ctx):
    from vse_amd import frame_select, synth
    frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", 11), ("seven wizards", 9), (None, 3)], 120, 320, seed=2)

    class Area:
        ymin, ymax, xmin, xmax = 60, 120, 3, 317
    runs = []
    for focus_fn, batch in ((NumpyFocus(), 25), (frame_select.EngineFocus(ctx), 25), (frame_select.EngineFocus(ctx), 4)):
        sel = frame_select.ChangeFrameSelector(frame_select.EngineCounter(ctx), batch=batch, focus_fn=focus_fn)
        intervals = sel.run(list(frames), Area, 12.0)
        assert sel.focus.dtype == np.int64 and sel.focus.shape == (len(frames), 2)
        runs.append((intervals, sel.focus))
    assert [(s, e) for s, e, _r in runs[0][0]] == [(s, e) for s, e, _t in truth]
    assert runs[0][1][:, 1].max() > 255 * 100
    for intervals, focus in runs[1:]:
        assert intervals == runs[0][0] and np.array_equal(focus, runs[0][1])


def test_extractor_sharpest_one_pass_equals_several_passes_on_engine(ctx, tmp_path):
    """Engine counter, engine focus, staged device batches and the engine's recogniser (real detector, stand-in recogniser weights,
    drop_score 0), over a pipe and over the same bytes as a file; the middle frame of the first interval is at 70 % contrast."""
    from oracle import net_ref, pipeline_ref as P
    from test_gpu_one_pass import EngineOcr
    from test_one_pass import piped
    from vse_amd import extractor, frame_select, ingest, pipeline, staging, synth
    h, w = 360, 640
    frames, truth = synth.make_clip([(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4),
                                     ("near frozen lakes", 8), (None, 2)], h, w, seed=6)
    bad = (truth[0][0] + truth[0][1]) // 2
    frames[bad - 1, int(0.75 * h):] = (frames[bad - 1, int(0.75 * h):].astype(np.float32) * 0.7).astype(np.uint8)
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")
    path = str(tmp_path / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], 12)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    with open(path, "rb") as fp:
        data = fp.read()
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    area = extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w)
    runs = []
    try:
        for one_pass in (False, True):
            fp, th = piped(data, 1 << 16) if one_pass else (None, None)
            source = ingest.Y4mStream(fp) if one_pass else src
            ocr = EngineOcr(pipe, decoded)
            ex = extractor.SubtitleExtractor(source, ocr, mode="auto", drop_score=0.0, batch=8, uploader=up, sub_area=area,
                                             frame_selector="change", change_counter=frame_select.EngineCounter(ctx),
                                             interval_frame="sharpest", frame_params={"focus_fn": frame_select.EngineFocus(ctx)})
            assert ex.one_pass == one_pass
            text = ex.run()
            runs.append((ex.intervals, ocr.seen, ex.raw_lines, text))
            if one_pass:
                th.join()
                fp.close()
                assert ex.clamped_intervals == 0 and 0 < ex.peak_retained < len(frames)
            want, _ = ref_focus(np.stack(decoded), (int(0.75 * h), h, 0, w), 128)
            assert np.array_equal(ex.focus, want)
    finally:
        up.close()
        src.close()
    for k, what in enumerate(("intervals", "frames seen", "raw_lines", "SRT")):
        assert runs[0][k] == runs[1][k], what
    intervals, seen, _lines, text = runs[1]
    assert [(s, e) for s, e, _r in intervals] == [(s, e) for s, e, _t in truth]
    assert seen == [frame_select.sharpest_rep(s, e, want, 12.0) for s, e, _r in intervals] and seen[0] != bad
    assert text.count(" --> ") >= 1
