"""Keyframes (scene cuts) for timeline sync's snapping step: find them on the GPU, write and read Sushi's keyframes file.

Sushi makes keyframes by piping the video through ffmpeg (scale=640:360) into SCXvid, an XviD first pass whose I-frame decisions
mark the cuts (backend/sushi/demux.py:113-135).  Neither tool exists here, and XviD's rate control is not restated: this module
plays the same role with its own, fully specified rule.  Per frame the device counts the 16x16 macroblocks of a box-filtered luma
plane that the frame before cannot predict within a search range (vse_scene_change, csrc/scene_cut.hip); the host calls a frame a
keyframe when at least `cut_percent` of its blocks changed.

The defaults are a judgement, not a measurement on real video (there is none to measure on):
  scale        max(1, width // 640), at most 8: SCXvid's 640x360 plane for 720p, 1080p and 2160p;
  search       8 plane pixels, the device's largest radius;
  bias         1024 = 4 grey levels per pixel of a block: a flat block (intra 0) counts as changed only when the best prediction is
               off by more than 2 levels per pixel, so sensor noise on a flat wall is no cut;
  cut_percent  50: half of the blocks unpredictable;
  min_gap      1: consecutive keyframes are allowed, as in an XviD stat file.
Known limit: a pan faster than search * scale source pixels per frame leaves every block without a match and reads as a cut,
as it does beyond SCXvid's own search range; so does a fade through black or a flash.

    python -m vse_amd.keyframes VIDEO -o keyframes.txt [--search N --bias N --cut-percent N --scale N --batch N]
                                [--size WxH --layout i420|nv12]

VIDEO is what ingest.open_source reads: uncompressed BGR24 or Motion-JPEG AVI, a .npy frame stack, YUV4MPEG2 (.y4m), or headerless
YUV 4:2:0 (.yuv / .i420 / .nv12, with --size).
"""
import argparse
import sys

import numpy as np

from . import staging
from .engine import DeviceState
from .timeline_sync import TimelineSyncError

MB = 16
STAT_HEADER = "# XviD 2pass stat file"


def default_scale(width):
    return min(max(1, int(width) // 640), 8)


class EngineSceneCounter(DeviceState):
    """The counter of SceneCutDetector on the GPU (engine.Context.scene_change): keeps the device state and a workspace between
    calls."""
    _ws = None

    def __call__(self, frames, scale, search, bias, reset):
        t = self.ctx.torch
        frames = self._device(frames)
        n, h, w, _ = frames.shape
        reset = self._fresh((h, w, scale), self.ctx.scene_change_state) or reset
        need = self.ctx.lib.vse_scene_change_workspace_bytes(n, h, w, scale)
        if self._ws is None or self._ws.numel() < need:
            self._ws = t.empty(max(need, 256), dtype=t.uint8, device=self.ctx.tdev)
        return self.ctx.scene_change(frames, scale, search, bias, self._state, reset, workspace=self._ws)


class SceneCutDetector:
    """Frames in, keyframe numbers out.  counter: an engine.Context, or any callable
    counter(frames uint8 [n,H,W,3], scale, search, bias, reset) -> int [n,3] (changed blocks, sum inter, sum intra) that carries the
    last frame's plane to the next call, as tests/scene_cut_ref.NumpySceneCounter does on the host.

    Frame t is a keyframe iff changed * 100 >= cut_percent * (number of blocks) and it lies at least min_gap frames after the
    keyframe before it; frame 0 always is one."""

    def __init__(self, counter, height, width, scale=None, search=8, bias=1024, cut_percent=50, min_gap=1):
        self.counter = EngineSceneCounter(counter) if hasattr(counter, "scene_change") else counter
        self.scale = default_scale(width) if scale is None else int(scale)
        if not 1 <= self.scale <= 8 or not 0 <= int(search) <= 8 or not 0 <= int(bias) <= 65535:
            raise ValueError(f"scale {self.scale} (1..8), search {search} (0..8) or bias {bias} (0..65535) out of range")
        self.search, self.bias, self.cut_percent, self.min_gap = int(search), int(bias), cut_percent, int(min_gap)
        self.height, self.width = int(height), int(width)
        self.blocks = (self.height // self.scale // MB) * (self.width // self.scale // MB)
        if self.blocks < 1:
            raise ValueError(f"{width}x{height} frames at scale {self.scale} hold no 16x16 macroblock")
        self.frames_seen = 0
        self.last_keyframe = None
        self.counts = []          # the [n,3] counts of every batch fed so far

    def feed(self, frames):
        """uint8 BGR [n,H,W,3] (numpy, or a device tensor for the engine), the next frames of the clip -> the 0-based numbers of
        those among them that are keyframes."""
        c = self.counter(frames, self.scale, self.search, self.bias, self.frames_seen == 0)
        c = c.cpu().numpy() if hasattr(c, "cpu") else np.asarray(c)
        self.counts.append(c)
        out = []
        for changed in c[:, 0]:
            no = self.frames_seen
            self.frames_seen += 1
            if no == 0 or (int(changed) * 100 >= self.cut_percent * self.blocks and no - self.last_keyframe >= self.min_gap):
                self.last_keyframe = no
                out.append(no)
        return out


def scan(source, ctx=None, batch=64, **detector_options):
    """-> (keyframes, frame count) of every frame source.frames() yields."""
    if ctx is None:
        from . import engine
        ctx = engine.Context(0)
    on_engine = hasattr(ctx, "scene_change")
    det = None
    keyframes = []

    def batches():
        group = []
        for f in source.frames():
            if f is None:
                raise TimelineSyncError(f"frame {len(group)} of a batch could not be read")
            group.append((None, f))
            if len(group) == batch:
                yield group
                group = []
        if group:
            yield group

    up = staging.Uploader(ctx.tdev) if on_engine else None
    try:
        for items, data in staging.staged_batches(batches(), up):
            if det is None:
                det = SceneCutDetector(ctx, items[0][1].shape[0], items[0][1].shape[1], **detector_options)
            keyframes.extend(det.feed(data))
    finally:
        if up is not None:
            up.close()
    return keyframes, (det.frames_seen if det else 0)


def find_keyframes(source, ctx=None, batch=64, **detector_options):
    """The 0-based keyframe numbers of a frame source (ingest.open_source, or anything with frames()).  ctx: an engine.Context
    (None: one on device 0) or a counter callable (see SceneCutDetector); detector_options: its keyword arguments."""
    return scan(source, ctx, batch, **detector_options)[0]


def write_keyframes(path, keyframes, frame_count):
    """The text form Sushi's parse_keyframes reads (backend/sushi/keyframes.py): an XviD first-pass stat file reduced to what the
    parser looks at: three header lines, then one line per frame that begins with `i` for a keyframe and `p` otherwise."""
    kf = set(int(k) for k in keyframes)
    if kf and (min(kf) < 0 or max(kf) >= frame_count):
        raise ValueError(f"keyframes outside 0..{frame_count - 1}")
    with open(path, "w") as f:
        f.write(STAT_HEADER + " (scene cuts of vse_amd.keyframes)\n# Please do not modify this file\n\n")
        f.write("".join("i\n" if no in kf else "p\n" for no in range(frame_count)))
    return path


def parse_keyframes(path):
    """backend/sushi/keyframes.py: frame = line index - 3 for the lines that begin with `i`; frame 0 is inserted if absent."""
    try:
        with open(path) as f:
            text = f.read()
    except OSError:
        raise TimelineSyncError(f"Keyframes file {path} not found")
    if STAT_HEADER not in text:
        raise TimelineSyncError("Unsupported keyframes type")
    frames = [i - 3 for i, line in enumerate(text.splitlines()) if line and line[0] == "i"]
    if 0 not in frames:
        frames.insert(0, 0)
    return frames


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m vse_amd.keyframes", description="Find a video's scene cuts on the GPU and write them as a "
                                "keyframes file for python -m vse_amd.timeline_sync --src-keyframes / --dst-keyframes.")
    p.add_argument("video", help="uncompressed BGR24 or Motion-JPEG AVI, a .npy frame stack, .y4m, or headerless .yuv / .i420 / .nv12")
    p.add_argument("-o", "--output", required=True, help="keyframes file to write")
    p.add_argument("--search", type=int, default=8, help="search radius in plane pixels, 0..8 [8]")
    p.add_argument("--bias", type=int, default=1024, help="a block changed iff 2 * inter > intra + bias [1024]")
    p.add_argument("--cut-percent", type=float, default=50, help="changed blocks that make a keyframe, in percent [50]")
    p.add_argument("--scale", type=int, default=None, help="box filter edge, 1..8 [width // 640]")
    p.add_argument("--batch", type=int, default=64, help="frames per device call [64]")
    p.add_argument("--size", default=None, metavar="WxH", help="frame size of a headerless YUV 4:2:0 file")
    p.add_argument("--layout", default=None, choices=("i420", "nv12"), help="plane layout of a headerless YUV 4:2:0 file [by extension]")
    args = p.parse_args(argv)
    from . import ingest
    try:
        size = None
        if args.size is not None:
            w, sep, h = args.size.lower().partition("x")
            if not (sep and w.isdigit() and h.isdigit()):
                raise ValueError(f"--size takes WIDTHxHEIGHT, not {args.size!r}")
            size = (int(w), int(h))
        if args.video.lower().endswith((".npy", ".yuv", ".i420", ".nv12")):       # no frame rate in the file, and none is needed here
            source = ingest.open_source(args.video, fps=1.0, size=size, layout=args.layout)
        else:
            source = ingest.open_source(args.video)
        if args.batch < 1:
            raise ValueError("--batch must be at least 1")
        kf, count = scan(source, None, args.batch, scale=args.scale, search=args.search, bias=args.bias, cut_percent=args.cut_percent)
        write_keyframes(args.output, kf, count)
    except (OSError, ValueError, TimelineSyncError) as e:
        print(f"keyframes: {e}", file=sys.stderr)
        return 2
    print(f"{args.output}: {len(kf)} keyframes in {count} frames")
    return 0


if __name__ == "__main__":
    sys.exit(main())
