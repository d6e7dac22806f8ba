"""One pass on the MI355X: vse_yuv_to_bgr_matrix (BT.709) byte for byte against tests/yuv709_ref.py on both kernels and both layouts,
SubtitleExtractor in one pass over an ingest.Y4mStream on an OS pipe against the multi-pass run over the same bytes as a file (engine
counters, staging.Uploader, the engine's recogniser), and `python -m vse_amd.extractor -` as a fresh child process."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import yuv709_ref
import yuv_ref
from test_frame_hold import BAND, MOVING
from test_one_pass import piped

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("i420", "nv12")
FILL = 0xA5


# ---- the conversion -------------------------------------------------------------------------------------------------------------
def raw_call(ctx, name, packed, n, h, w, layout, parity, out, *matrix):
    """The C entry `name` itself (vse_yuv420_to_bgr, or vse_yuv_to_bgr_matrix with its one more argument) on packed frames back to back."""
    frame = ctx.lib.vse_yuv420_frame_bytes(h, w, parity)
    return getattr(ctx.lib, name)(ctx.handle, C.c_void_p(packed.data_ptr()), n, h, w, layout, parity, frame, C.c_void_p(out.data_ptr()),
                                  out.stride(1), out.stride(0), *matrix, ctx.stream())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bt709_fast_kernel(ctx, layout):
    """16 x 32, everything aligned: the 16-byte kernel.  Uniform bytes (about 40 % of the channels clip) and mid-range ones."""
    import torch
    h, w = 16, 32
    rng = np.random.default_rng(7)
    planes = [yuv_ref.random_planes(rng, h, w, layout, mid=k == 2) for k in range(3)]
    want = np.stack([yuv709_ref.convert(p, layout) for p in planes])
    packed = torch.from_numpy(np.concatenate([yuv_ref.pack(p, layout) for p in planes])).to(ctx.tdev)
    assert packed.data_ptr() % 16 == 0 and yuv_ref.packed_bytes(h, w) % 16 == 0
    got = ctx.yuv420_to_bgr(packed, 3, h, w, layout, matrix=1)
    assert got.data_ptr() % 16 == 0 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ctx.yuv420_to_bgr(packed, 3, h, w, layout, matrix="bt709").cpu().numpy(), want)
    assert not np.array_equal(want, np.stack([yuv_ref.convert(p, layout) for p in planes]))
    # matrix 0, the default and the old entry: BT.601, byte for byte the same
    old = torch.full((3, h, w, 3), FILL, dtype=torch.uint8, device=ctx.tdev)
    new = torch.full((3, h, w, 3), FILL, dtype=torch.uint8, device=ctx.tdev)
    code = {"i420": 0, "nv12": 1}[layout]
    assert raw_call(ctx, "vse_yuv420_to_bgr", packed, 3, h, w, code, 0, old) == 0
    assert raw_call(ctx, "vse_yuv_to_bgr_matrix", packed, 3, h, w, code, 0, new, 0) == 0
    want601 = np.stack([yuv_ref.convert(p, layout) for p in planes])
    assert np.array_equal(old.cpu().numpy(), want601) and np.array_equal(new.cpu().numpy(), want601)
    assert np.array_equal(ctx.yuv420_to_bgr(packed, 3, h, w, layout).cpu().numpy(), want601)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(5, 7), (6, 10)])
def test_bt709_general_kernel(ctx, hw, layout):
    """Odd sizes, row parity 1 and a padded pitch: the general kernel; the padding keeps its fill."""
    import torch
    h, w = hw
    n, parity = 2, 1
    rng = np.random.default_rng(h * 10 + w)
    planes = [yuv_ref.random_planes(rng, h, w, layout, parity) for _ in range(n)]
    want = np.stack([yuv709_ref.convert(p, layout, parity=parity) for p in planes])
    want601 = np.stack([yuv_ref.convert(p, layout, parity=parity) for p in planes])
    packed = torch.from_numpy(np.concatenate([yuv_ref.pack(p, layout) for p in planes])).to(ctx.tdev)
    pitch = 3 * w + 5
    fstride = h * pitch + 32
    for matrix, ref in ((1, want), (0, want601)):
        big = torch.full((n * fstride + 64,), FILL, dtype=torch.uint8, device=ctx.tdev)
        view = big.as_strided((n, h, w, 3), (fstride, pitch, 3, 1), 0)
        assert ctx.yuv420_to_bgr(packed, n, h, w, layout, parity, out=view, matrix=matrix) is view
        host = big.cpu().numpy()
        mask = np.zeros(host.size, bool)
        for f in range(n):
            for r in range(h):
                a = f * fstride + r * pitch
                mask[a:a + 3 * w] = True
                assert np.array_equal(host[a:a + 3 * w], ref[f, r].reshape(-1)), (matrix, f, r)
        assert np.all(host[~mask] == FILL), matrix
    old = torch.full((n, h, w, 3), FILL, dtype=torch.uint8, device=ctx.tdev)
    assert raw_call(ctx, "vse_yuv420_to_bgr", packed, n, h, w, {"i420": 0, "nv12": 1}[layout], parity, old) == 0
    assert np.array_equal(old.cpu().numpy(), want601)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bt709_every_value_of_each_sample(ctx, layout):
    """One input of 8 x 16 frames in which Y, U and V each take all 256 values (chroma has 32 samples per frame: 8 frames), on both
    kernels (the second call writes to a pitch that is no multiple of 16)."""
    import torch
    h, w, n = 8, 16, 8
    rng = np.random.default_rng(3)
    y = rng.permutation(np.arange(n * h * w) % 256).astype(np.uint8).reshape(n, h, w)
    u = rng.permutation(256).astype(np.uint8).reshape(n, 4, 8)
    v = rng.permutation(256).astype(np.uint8).reshape(n, 4, 8)
    assert all(len(np.unique(p)) == 256 for p in (y, u, v))
    planes = [(y[f], u[f], v[f]) if layout == "i420" else (y[f], np.stack([u[f], v[f]], axis=2).reshape(4, 16)) for f in range(n)]
    want = np.stack([yuv709_ref.convert(p, layout) for p in planes])
    packed = torch.from_numpy(np.concatenate([yuv_ref.pack(p, layout) for p in planes])).to(ctx.tdev)
    assert np.array_equal(ctx.yuv420_to_bgr(packed, n, h, w, layout, matrix=1).cpu().numpy(), want)
    big = torch.zeros((n, h, 3 * w + 4), dtype=torch.uint8, device=ctx.tdev)
    view = big.as_strided((n, h, w, 3), (h * (3 * w + 4), 3 * w + 4, 3, 1), 0)
    assert np.array_equal(ctx.yuv420_to_bgr(packed, n, h, w, layout, out=view, matrix=1).cpu().numpy(), want)


def test_bad_matrix_is_refused_and_launches_nothing(ctx):
    import torch
    from vse_amd import engine
    h, w = 8, 16
    packed = torch.zeros(yuv_ref.packed_bytes(h, w), dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((1, h, w, 3), FILL, dtype=torch.uint8, device=ctx.tdev)
    for matrix in (2, -1):
        assert raw_call(ctx, "vse_yuv_to_bgr_matrix", packed, 1, h, w, 0, 0, out, matrix) == -1          # VSE_E_INVAL
        assert "matrix" in ctx.lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    with pytest.raises(engine.VseError, match="matrix"):
        ctx.yuv420_to_bgr(packed, 1, h, w, matrix="bt2020")
    assert raw_call(ctx, "vse_yuv_to_bgr_matrix", packed, 1, h, w, 0, 0, out, 1) == 0
    assert np.all(out.cpu().numpy() == yuv709_ref.pixels(0, 0, 0))


def test_uploader_converts_with_the_frames_matrix(ctx):
    from vse_amd import ingest, staging
    h, w = 46, 70
    rng = np.random.default_rng(41)
    planes = [yuv_ref.random_planes(rng, h, w, "i420") for _ in range(4)]
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    try:
        for matrix, ref in (("bt709", yuv709_ref), ("bt601", yuv_ref)):
            frames = [ingest.Yuv420Frame(p, h, w, "i420", matrix=matrix)[11:40] for p in planes]
            want = np.stack([ref.convert(p, "i420", rows=(11, 40)) for p in planes])
            assert np.array_equal(up.stage(frames).tensor().cpu().numpy(), want)
            assert np.array_equal(np.stack([f.to_bgr() for f in frames]), want)
        with pytest.raises(ValueError, match="matrix"):
            up.stage([ingest.Yuv420Frame(planes[0], h, w, "i420"), ingest.Yuv420Frame(planes[1], h, w, "i420", matrix="bt709")])
    finally:
        up.close()


# ---- the extractor --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe_ocr(ctx):
    from oracle import net_ref, pipeline_ref as P
    from vse_amd import pipeline
    return pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")


class EngineOcr:
    """The engine's recogniser on staged device batches; `seen`: the frame numbers it was shown, found by the frames' bytes."""

    def __init__(self, pipe, frames):
        self.pipe, self.seen = pipe, []
        self.nos = {hashlib.sha1(np.ascontiguousarray(f).tobytes()).digest(): no for no, f in enumerate(frames, 1)}

    def predict_batch(self, frames):
        import torch
        from vse_amd import shim
        assert torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.is_cuda
        self.seen += [self.nos[hashlib.sha1(f.tobytes()).digest()] for f in frames.cpu().numpy()]
        return [shim.OcrRecogniser.arrange(b, r) for b, r in self.pipe.ocr(frames)]

    def predict(self, frame):
        import torch
        return self.predict_batch(torch.from_numpy(np.ascontiguousarray(frame)).cuda()[None])[0]


@pytest.mark.parametrize("kind", ["change", "hold"])
def test_one_pass_over_a_pipe_equals_multi_pass_over_the_file(ctx, pipe_ocr, tmp_path, kind):
    """Built as test_gpu_frame_change.test_extractor_change_selector_on_engine: real detector, stand-in recogniser, drop_score 0, batch 8.
    Equal intervals, frames shown to the recogniser, raw.txt lines and SRT; the intervals are the clip's truth."""
    from vse_amd import extractor, frame_select, ingest, staging, synth
    if kind == "change":
        h, w = 360, 640
        frames, truth = synth.make_clip([(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4),
                                         ("near frozen lakes", 8), (None, 2)], h, w, seed=6)
        kw = dict(sub_area=extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w), frame_selector="change")
        counter = lambda: frame_select.EngineCounter(ctx)                                   # noqa: E731
    else:
        frames, truth = synth.make_moving_clip(MOVING)
        kw = dict(sub_area=BAND, frame_selector="hold", change_params={"hold_frames": 5})
        counter = lambda: frame_select.EngineHoldCounter(ctx)                               # noqa: E731
    path = str(tmp_path / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], 12)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    with open(path, "rb") as fp:
        data = fp.read()
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    runs = []
    try:
        for one_pass in (False, True):
            fp, th = piped(data, 1 << 16) if one_pass else (None, None)
            source = ingest.Y4mStream(fp) if one_pass else src
            ocr = EngineOcr(pipe_ocr, decoded)
            ex = extractor.SubtitleExtractor(source, ocr, mode="auto", drop_score=0.0, batch=8, uploader=up, change_counter=counter(), **kw)
            assert ex.one_pass == one_pass
            text = ex.run()
            runs.append((ex.intervals, ocr.seen, ex.raw_lines, text))
            if one_pass:
                th.join()
                fp.close()
                assert ex.clamped_intervals == 0 and source.frame_count == len(frames) and 0 < ex.peak_retained < len(frames)
    finally:
        up.close()
        src.close()
    for k, what in enumerate(("intervals", "frames seen", "raw_lines", "SRT")):
        assert runs[0][k] == runs[1][k], what
    intervals, seen, _lines, text = runs[1]
    assert [(s, e) for s, e, _r in intervals] == [(s, e) for s, e, _t in truth]
    assert seen == [(s + e) // 2 for s, e, _t in truth]
    assert text.count(" --> ") >= 1


def test_command_line_in_a_fresh_process(ctx, tmp_path, monkeypatch):
    """`python -m vse_amd.extractor -` as a child of its own (this process has the GPU open), the Y4M bytes on its standard input:
    exit status 0 and as many SRT blocks as the same run in this process."""
    from vse_amd import extractor, ingest, shim, staging, synth
    h, w = 360, 640
    frames, truth = synth.make_clip([(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4),
                                     ("near frozen lakes", 8), (None, 2)], h, w, seed=6)
    path, out = str(tmp_path / "clip.y4m"), str(tmp_path / "out.srt")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], 12)
    area = f"{int(0.75 * h)},{h},0,{w}"
    with open(path, "rb") as fp:
        r = subprocess.run([sys.executable, "-m", "vse_amd.extractor", "-", "--allow-standin-weights", "--area", area, "--selector", "change",
                            "--batch", "8", "-o", out], cwd=ROOT, stdin=fp, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = open(out).read()
    for name, value in (("language", "ch"), ("mode", "fast"), ("allow_standin_weights", True), ("weights_dir", None)):
        monkeypatch.setattr(shim.config, name, value)
    src = ingest.Y4mSource(path)
    up = staging.default_uploader()
    try:
        ex = extractor.SubtitleExtractor(src, shim.OcrRecogniser(), sub_area=extractor.SubtitleArea(int(0.75 * h), h, 0, w), mode="fast",
                                         batch=8, uploader=up, frame_selector="change")
        here = ex.run()
    finally:
        up.close()
        src.close()
    assert [(s, e) for s, e, _r in ex.intervals] == [(s, e) for s, e, _t in truth]
    assert child.count(" --> ") == here.count(" --> ") and child == here
