"""vse_frame_change on the MI355X: the device counts equal the numpy restatement (tests/frame_change_ref.py) bit for bit, batches
chained through the state equal one batch, and SubtitleExtractor(frame_selector="change") on the engine gives the intervals,
OCR'd frames and time codes of the run fed by the numpy counts."""
import ctypes as C

import numpy as np
import pytest

from frame_change_ref import NumpyCounter, counts as ref_counts

pytestmark = pytest.mark.gpu


def dev_counts(ctx, frames, area, thresh=128, batches=None):
    """frames: cuda uint8 [n,H,W,3] view -> host int32 [n,3], fed in batches of `batches` frames through one state."""
    y0, y1, x0, x1 = area
    state = ctx.frame_change_state(y1 - y0, x1 - x0)
    n = frames.shape[0]
    step = batches or n
    out = [ctx.frame_change(frames[i:i + step], area, thresh, state, reset=(i == 0)).cpu().numpy() for i in range(0, n, step)]
    return np.concatenate(out)


def random_frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    f[n // 2:] = f[n // 2 - 1]                                     # held frames: nothing appears or vanishes
    f[n // 2 + 1:, h // 3:] = rng.integers(0, 256, size=(n - n // 2 - 1, h - h // 3, w, 3), dtype=np.uint8)
    return f


@pytest.mark.parametrize("area", [(0, 40, 0, 100), (5, 8, 3, 6), (1, 39, 61, 100), (10, 30, 7, 71), (0, 40, 37, 100), (12, 15, 0, 200),
                                  (0, 3, 130, 200)])
@pytest.mark.parametrize("thresh", [1, 60, 128])
def test_counts_match_numpy_random(ctx, area, thresh):
    import torch
    frames = random_frames(9, 40, 200, seed=sum(area) + thresh)
    want, _ = ref_counts(frames, area, thresh)
    got = dev_counts(ctx, torch.from_numpy(frames).cuda(), area, thresh)
    assert np.array_equal(got, want), (area, thresh)


def test_counts_padded_pitch_and_stride(ctx):
    import torch
    frames = random_frames(6, 37, 150, seed=7)
    area = (2, 37, 5, 149)
    want, _ = ref_counts(frames, area, 40)
    padded = torch.zeros((6, 41, 163 * 3 + 5), dtype=torch.uint8, device=ctx.tdev)     # padded rows inside padded frames
    view = padded[:, 3:40, 6:6 + 450].view(6, 37, 150, 3)
    view.copy_(torch.from_numpy(frames))
    assert view.stride(1) == 163 * 3 + 5 and view.stride(0) == 41 * (163 * 3 + 5)
    assert np.array_equal(dev_counts(ctx, view, area, 40), want)


def test_area_rows_only_upload(ctx):
    import torch
    from vse_amd import synth
    frames, _ = synth.make_clip([(None, 2), ("the quick brown fox", 5), ("seven wizards", 4), (None, 1)], 360, 640, seed=2)
    y0, y1, x0, x1 = int(0.78 * 360), int(0.99 * 360), int(0.05 * 640), int(0.95 * 640)
    want, _ = ref_counts(frames, (y0, y1, x0, x1), 128)
    full = dev_counts(ctx, torch.from_numpy(frames).cuda(), (y0, y1, x0, x1))
    rows = dev_counts(ctx, torch.from_numpy(np.ascontiguousarray(frames[:, y0:y1])).cuda(), (0, y1 - y0, x0, x1))
    assert np.array_equal(full, want) and np.array_equal(rows, want)
    assert want[:, 0].max() > 500


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_batches_chain_through_state(ctx, batch):
    import torch
    from vse_amd import synth
    frames, _ = synth.make_clip([(None, 3), ("the quick brown fox", 20), ("the quick brown box", 30), (None, 10),
                                 ("near frozen lakes", 40, 4), (None, 30)], 240, 1000, seed=3)
    area = (int(0.78 * 240), int(0.99 * 240), 3, 997)
    want, _ = ref_counts(frames, area, 128)
    dev = torch.from_numpy(frames).cuda()
    assert np.array_equal(dev_counts(ctx, dev, area), want)                  # one batch of 133 frames (two LDS chunks)
    assert np.array_equal(dev_counts(ctx, dev, area, batches=batch), want)


def test_reset(ctx):
    import torch
    frames = random_frames(8, 30, 90, seed=11)
    area = (0, 30, 0, 90)
    dev = torch.from_numpy(frames).cuda()
    state = ctx.frame_change_state(30, 90)
    ctx.frame_change(dev[:5], area, 50, state)
    again = ctx.frame_change(dev[5:], area, 50, state, reset=True).cpu().numpy()
    want, _ = ref_counts(frames[5:], area, 50)
    assert np.array_equal(again, want)
    assert again[0, 1] == again[0, 0] and again[0, 2] == 0


def test_rejects_degenerate_area(ctx):
    from vse_amd import engine
    lib = engine.load_library()
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the areas below
    st = torch.zeros(4096, dtype=torch.uint8, device=ctx.tdev)
    cnt = torch.full((3,), -7, dtype=torch.int32, device=ctx.tdev)
    for y0, y1, x0, x1 in [(0, 2, 0, 10), (0, 10, 5, 7), (-1, 5, 0, 10), (0, 11, 0, 10), (0, 10, 0, 21), (4, 4, 0, 10)]:
        rc = lib.vse_frame_change(ctx.handle, C.c_void_p(buf.data_ptr()), 1, 10, 20, 60, 600, y0, y1, x0, x1, 128,
                                  C.c_void_p(st.data_ptr()), 0, C.c_void_p(cnt.data_ptr()), ctx.stream())
        assert rc == -1, (y0, y1, x0, x1)
        assert "area" in lib.vse_last_error().decode()
    assert cnt.cpu().tolist() == [-7, -7, -7] and int(st.sum()) == 0      # nothing was enqueued
    assert lib.vse_frame_change_state_bytes(2, 100) == 0 and lib.vse_frame_change_state_bytes(3, 66) == 16 + 8
    assert lib.vse_frame_change_state_bytes(10, 131) == 16 + 8 * 3 * 8


@pytest.mark.parametrize("staged", [False, True])
def test_extractor_change_selector_on_engine(ctx, staged):
    """Stand-in models as in test_gpu_pipeline.test_extractor_on_a_clip_engine_vs_oracle: the engine-fed selector gives the
    numpy-fed selector's intervals, OCR'd frames and SRT, and the intervals are the clip's truth."""
    import torch
    from oracle import net_ref, pipeline_ref as P
    from vse_amd import extractor, frame_select, pipeline, shim, srt, staging, synth
    det = net_ref.get_weights("V3_ch_det_fast")
    rec = net_ref.get_weights("V4_en_rec_fast")
    pipe = pipeline.OcrPipeline(ctx, det, rec, P.en_charset(), rec_mode="reference")

    class EngineOcr:
        def __init__(self):
            self.seen = 0

        def predict(self, frame):
            self.seen += 1
            b, r = pipe.ocr(torch.from_numpy(np.ascontiguousarray(frame)).cuda()[None])[0]
            return shim.OcrRecogniser.arrange(b, r)

    h, w = 360, 640
    frames, truth = synth.make_clip([(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4),
                                     ("near frozen lakes", 8), (None, 2)], h, w, seed=6)
    src = extractor.ArraySource(list(frames), 12.0)
    area = extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w)
    up = staging.Uploader(ctx.tdev) if staged else None
    runs = []
    for counter in (NumpyCounter(), frame_select.EngineCounter(ctx)):
        ocr = EngineOcr()
        ex = extractor.SubtitleExtractor(src, ocr, sub_area=area, mode="auto", frame_selector="change", change_counter=counter,
                                         drop_score=0.0, batch=8, uploader=up if isinstance(counter, frame_select.EngineCounter) else None)
        text = ex.run()
        runs.append((ex.intervals, ocr.seen, text, ex.raw_lines))
    assert runs[0] == runs[1]
    intervals, seen, text, _ = runs[1]
    assert [(s, e) for s, e, _r in intervals] == [(s, e) for s, e, _t in truth]
    assert seen == len(truth)
    codes = [ln for ln in text.split("\n") if " --> " in ln]
    assert codes
    starts = {srt.frame_to_timecode(s, 12.0) for s, _e, _t in truth}
    ends = {srt.frame_to_timecode(e, 12.0) for _s, e, _t in truth}
    assert all(c.split(" --> ")[0] in starts and c.split(" --> ")[1] in ends for c in codes)
