"""Frames -> raw.txt -> SRT: the reference's SubtitleExtractor.run (backend/main.py:103-191) around the batched OCR engine.

What the reference does with one process, two threads and bounded queues — pick the frames to look at (fps sampler
`extract_frame_by_fps`, main.py:228-253, or the accurate-mode detector loop, main.py:255-376), seek + read + crop each of
them (`ocr_task_producer` / `frame_preprocess`, backend/tools/subtitle_ocr.py:163-208,270-289), OCR it and filter its lines
(`ocr_task_consumer` -> `extract_subtitles`, subtitle_ocr.py:20-85,126-161), clean raw.txt (main.py:506-612,671-729) and write
the SRT (main.py:614-637) — is done here as: task list -> BATCHES of frames through `predict_batch` -> the same per-frame line
logic on the host.  Frames are independent, so the tasks of one video can also be sharded over ranks (`shard=(rank, world)`)
and the per-frame records gathered on rank 0 (parallel.gather_records) before the sequential text logic runs.

Pinned by tests/golden/extract.json (the reference's own producer / consumer / fps sampler executed on scripted inputs),
frame_loop.json, srt.json, raw_filters.json and text_cleanup.json.  Not rebuilt: VideoSubFinder itself (closed binary; its role,
finding where each subtitle starts and stops, is frame_selector="change"), GUI progress plumbing; reformat.execute is
text_cleanup.py with the word segmenter as a parameter (its corpus is not installed here).

Frame sources: anything with `frame_count`, `fps`, `read(frame_no) -> uint8 BGR [H,W,3] | None` (1-based, like
cap.set(CAP_PROP_POS_FRAMES, frame_no - 1); cap.read()) and `frames()` (decode order).  `ArraySource` wraps decoded frames;
ingest.py reads the lossless containers that need no codec (neither box has cv2 / ffmpeg).  A source without `read` (ingest.Y4mStream:
a pipe from any decoder) is sequential: SubtitleExtractor then works in one pass (`one_pass`).

Command line: python -m vse_amd.extractor VIDEO|- [-o OUT.srt]   (main below).
"""
import argparse
import itertools
import logging
import re
import sys
from collections import deque
from types import SimpleNamespace

import numpy as np

from . import frame_select, parallel, raw_filters, shim, srt, staging, text_cleanup

# backend/tools/constant.py:5-13 — default subtitle position used by the fps sampler's half-frame crop
LOWER_PART, UPPER_PART, UNKNOWN = "LOWER_PART", "UPPER_PART", "UNKNOWN"


class SubtitleArea(SimpleNamespace):
    """backend/bean/subtitle_area.py: (ymin, ymax, xmin, xmax) in frame pixels."""

    def __init__(self, ymin, ymax, xmin, xmax):
        super().__init__(ymin=ymin, ymax=ymax, xmin=xmin, xmax=xmax)


class ArraySource:
    def __init__(self, frames, fps):
        self._frames = frames
        self.frame_count = len(frames)
        self.fps = float(fps)

    def read(self, frame_no):
        return self._frames[frame_no - 1] if 1 <= frame_no <= self.frame_count else None

    def frames(self):
        return iter(self._frames)

    pos_msec = None        # no container timestamps: SRT time codes fall back to frame_no / fps (main.py:745-748)


class CompositedSource:
    """A frame source whose rep frames show the interval composite inside the subtitle area: read(no) is a copy of source.read(no)
    with the area replaced by patches[no] (frame_select.IntervalCompositor) where there is one, and the plain frame otherwise.
    area: the SubtitleArea the patches were made for; a patch goes where the area, clipped to the frame, starts.  Forwards fps,
    frame_count and, where present, pos_msec.  No read_raw on purpose: a 4:2:0 source is then converted on the host, by the same integers."""

    def __init__(self, source, area, patches):
        self._source, self._patches = source, patches
        self._y0, self._x0 = max(0, int(area.ymin)), max(0, int(area.xmin))
        self.fps, self.frame_count = source.fps, source.frame_count
        if hasattr(source, "pos_msec"):
            self.pos_msec = source.pos_msec

    def read(self, frame_no):
        frame = self._source.read(frame_no)
        patch = self._patches.get(frame_no)
        if frame is None or patch is None:
            return frame
        out = np.array(frame, copy=True)
        out[self._y0:self._y0 + patch.shape[0], self._x0:self._x0 + patch.shape[1]] = patch
        return out


class RetainedSource:
    """The frames a one-pass run still holds, as the source run_ocr_tasks reads: read(no) is the BGR frame, read_raw(no), only where
    the frames are unconverted ingest.Yuv420Frames, the planes (uploaded as they are and converted on the device)."""

    def __init__(self, frames, fps, raw):
        self._frames, self.fps, self.frame_count = frames, fps, None
        if raw:
            self.read_raw = frames.get

    def read(self, frame_no):
        f = self._frames.get(frame_no)
        return f.to_bgr() if hasattr(f, "to_bgr") else f


def _drain(frames):
    """The frames of a list, front to back, each let go of as it is handed out."""
    frames.reverse()
    while frames:
        yield frames.pop()


def _frame_nbytes(frame):
    """Bytes a retained frame keeps alive: its planes, and for an ingest.InterlacedYuvFrame its previous picture's too (it pins them)."""
    if not hasattr(frame, "planes"):
        return frame.nbytes
    return sum(p.nbytes for p in frame.planes) + sum(p.nbytes for p in getattr(frame, "prev", None) or ())


def frame_preprocess(subtitle_area, frame):
    """Half-frame crop of subtitle_ocr.py:270-289 (a view, like the reference's slice)."""
    if subtitle_area == LOWER_PART:
        return frame[int(frame.shape[0] // 2):]
    if subtitle_area == UPPER_PART:
        return frame[:int(frame.shape[0] // 2)]
    return frame


def fps_tasks(frame_count, fps, extract_frequency, default_area=None):
    """extract_frame_by_fps (main.py:228-253): one task per read that is followed by int(fps // frequency) - 1 skipped reads.
    Task = (total_frame_count, frame_no, dt_box, rec_res, total_ms, default_subtitle_area)."""
    tasks = []
    reads = no = 0
    skip = int(fps // extract_frequency) - 1
    while reads < frame_count:
        reads += 1
        no += 1
        tasks.append((frame_count, no, None, None, None, default_area))
        for _ in range(skip):
            if reads < frame_count:
                reads += 1
                no += 1
    return tasks


def frame_lines(frame_no, dt_box, rec_res, sub_area, rec_char_type, drop_score, deviation_rate):
    """extract_subtitles (subtitle_ocr.py:20-85) for one frame: raw.txt lines of the recognised text that passes the filters."""
    return shim.extract_subtitles(frame_no, (dt_box, rec_res), sub_area, rec_char_type, deviation_rate, drop_score)


def run_ocr_tasks(source, tasks, ocr, sub_area=None, rec_char_type="ch", drop_score=0.75, deviation_rate=0.0, batch=64,
                  shard=None, gather_device=None, uploader=None):
    """Producer + consumer of subtitle_ocr.py over a task list.  `ocr` has predict(frame) and optionally
    predict_batch(batch of equal-shaped frames).  Tasks whose frame cannot be read are skipped like the reference's failed
    cap.read(); tasks that carry a cached (dt_box, rec_res) — accurate mode — are not recognised again.
    uploader (staging.Uploader): batches are assembled in pinned memory and uploaded by a producer thread while the previous
    batch is recognised — the reference's producer / consumer pair at batch granularity; predict_batch then receives a
    device uint8 tensor [n,H,W,3] (a source with read_raw is read through it: its 4:2:0 planes are uploaded and converted on the
    device).  Without one the frames are stacked on the host.
    shard=(rank, world): this rank recognises a contiguous slice of the tasks; every rank gets the records of all tasks back
    (one variable-length gather) and therefore returns the same lines.  -> list of raw.txt lines in task order."""
    tasks = [t for t in tasks if t[1] != -1]
    lo, hi = (0, len(tasks)) if shard is None else parallel.shard_range(len(tasks), *shard)
    if shard is not None and shard[1] > 1:
        parallel.cap_host_threads(shard[1])       # one process per GPU: this rank's numpy / torch pools get cores / world threads
    results = {}                        # task index -> (dt_box, rec_res)
    batched = hasattr(ocr, "predict_batch")
    # a YUV 4:2:0 source (ingest.Y4mSource / Yuv420Source) on the staged route hands out its planes: the uploader sends them as they
    # are and converts on the device; every other route reads BGR ndarrays, converted on the host by the same integers
    read = source.read_raw if batched and uploader is not None and hasattr(source, "read_raw") else source.read

    def batches():
        """lists of (task index, frame): consecutive readable tasks of one frame shape, at most `batch` of them"""
        pend = []
        for k in range(lo, hi):
            _total, no, dt_box, rec_res, _ms, default_area = tasks[k]
            frame = read(no)
            if frame is None:
                continue
            if dt_box is not None and rec_res is not None:
                results[k] = (dt_box, rec_res)
                continue
            if default_area is not None:
                frame = frame_preprocess(default_area, frame)
            if pend and (pend[0][1].shape != frame.shape or len(pend) >= batch):
                yield pend
                pend = []
            pend.append((k, frame))
        if pend:
            yield pend

    if batched and uploader is not None:
        staged = staging.prefetch(batches(), uploader)
        if hasattr(ocr, "predict_stream"):
            # the recogniser overlaps the detector of the next batches with the recognition of the current one; results come
            # back in batch order, so the item lists are matched through a queue
            pending = deque()

            def tensors():
                for items, sb in staged:
                    pending.append(items)
                    yield sb.tensor()
            for out in ocr.predict_stream(tensors()):
                for (k, _), r in zip(pending.popleft(), out):
                    results[k] = r
        else:
            for items, sb in staged:
                for (k, _), r in zip(items, ocr.predict_batch(sb.tensor())):
                    results[k] = r
    else:
        for items in batches():
            frames = [f for _, f in items]
            out = ocr.predict_batch(_stack(frames)) if batched and len(frames) > 1 else [ocr.predict(f) for f in frames]
            for (k, _), r in zip(items, out):
                results[k] = r
    if shard is not None and shard[1] > 1:
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() != shard[1]:
            raise RuntimeError(f"run_ocr_tasks(shard={shard}): torch.distributed is not initialised with world size {shard[1]} — "
                               "this rank recognised only its slice of the tasks and the other slices cannot be gathered")
        recs = [(k, _boxes_array(results[k][0]), list(results[k][1])) for k in sorted(results)]
        results = {k: (_boxes_list(b), r) for k, b, r in parallel.gather_records(recs, device=gather_device, to_all=True)}
    lines = []
    for k in sorted(results):
        dt_box, rec_res = results[k]
        lines += frame_lines(tasks[k][1], dt_box, rec_res, sub_area, rec_char_type, drop_score, deviation_rate)
    return lines


def _stack(frames):
    try:
        import torch
        if isinstance(frames[0], torch.Tensor):
            return torch.stack(frames)
        return torch.from_numpy(np.stack(frames)).to(shim._context().tdev)
    except ImportError:                 # host-only use with a scripted recogniser (tests)
        return np.stack(frames)


def _key_names(params):
    """The colour-key names among change_params / area_params."""
    return sorted(set(params or {}) & {"text_colour", "colour_tol", "key_fn"})


def _key_params(params, where):
    """change_params / area_params with `text_colour` (frame_select.parse_colour's forms) and `colour_tol` (1..255, default 48) ->
    (the params with a `key_fn` in their place, the frame_select.ColourKey or None): an EngineKey on the shim's device, made when it is
    first called.  A `key_fn` given instead, a callable (frames, area) -> frames, is kept as it is."""
    names = _key_names(params)
    if not names:
        return params, None
    if "key_fn" in names:
        if len(names) > 1:
            raise ValueError(f"{where}: key_fn is a colour key of the caller's own; it does not combine with {names}")
        return params, None
    if "text_colour" not in names:
        raise ValueError(f"{where}: colour_tol needs a text_colour")
    params = dict(params)
    try:
        key = frame_select.ColourKey(params.pop("text_colour"), params.pop("colour_tol", 48))
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    params["key_fn"] = frame_select.EngineKey(None, key)
    return params, key


def _boxes_array(dt_box):
    return np.asarray(dt_box, np.float32).reshape(-1, 4, 2)


def _boxes_list(arr):
    # OcrRecogniser.predict returns lists of four (x, y) int tuples (ocr.py:80-82); get_coordinates needs a list
    return [[(int(x), int(y)) for x, y in q] for q in np.asarray(arr).reshape(-1, 4, 2)]


# what the recogniser may be shown for an interval: its middle frame, a composite of all its frames (frame_select.COMPOSITE_MODES),
# or the per-pixel quantile of a few of them (frame_select.IntervalQuantile)
INTERVAL_IMAGES = ("middle",) + frame_select.COMPOSITE_MODES + ("quantile",)
# which single frame of an interval is recognised: its middle frame, or the one whose standing edges are sharpest (frame_select.sharpest_rep)
INTERVAL_FRAMES = ("middle", "sharpest")


class SubtitleExtractor:
    """run() = backend/main.py:103-191 without the GUI/process plumbing.

    mode 'accurate' (+ a subtitle area): frames are chosen by the detector loop (frame_select.AccurateFrameSelector);
    otherwise by the fps sampler (the reference would use the closed VideoSubFinder binary in fast/auto mode when an area is
    given; the sampler is what it runs without an area and on platforms without that binary).
    frame_selector="change" takes VideoSubFinder's role in fast / auto mode with an area: every frame of the area is compared
    with the one before it on the device (frame_select.ChangeFrameSelector, `change_params` its keyword arguments,
    `change_counter` its count_fn), one OCR task goes to the middle frame of each interval, and the SRT takes its times from
    the intervals (srt.generate_subtitle_file_intervals); the intervals are kept on the object (`intervals`).
    frame_selector="hold" is the change selector for footage whose background moves behind the subtitle: only edges that hold still
    for a while are counted (frame_select.HoldFrameSelector, `change_params` its keyword arguments, `change_counter` its count_fn);
    everything that follows "change" below follows "hold" the same way.  Its default hold of 0.3 s and its behaviour on real footage
    are not measured here; background edges that stand still that long still count: while the background moves they can add intervals,
    never lose one, but over a static busy shot, a logo or a watermark they dilute the cut ratio and subtitles are merged and lost.
    change_params={"max_hold_seconds": 12} (or "max_hold_frames"; frame_selector="hold" only) is for that footage: only edges that
    hold for hold .. max_hold frames are counted, so what stands still for longer than a subtitle does drops out
    (frame_select.HoldFrameSelector has the limits: a subtitle shown for longer than that disappears too, and 12-15 s is a guess).  The
    selector's rows then trail its frames by max_hold, so one pass keeps about max_hold more frames (360 frames of 1080p 4:2:0 at 15 s
    and 24 fps are 1.1 GB; `retain_bytes` stays the fallback).  The locator and the calibration do not inherit it: they bound their
    runs only when `area_params` carries a max_hold_seconds / max_hold_frames of its own (below).
    interval_image="min" | "max" | "mean" (change selector only; default "middle", the above): one recognition error on that single
    frame is final, so the recogniser is instead shown, inside the area of the same middle frame, the per-pixel minimum (light
    text) / maximum (dark text) / mean of ALL frames of the interval, one more pass over the area's rows on the device
    (frame_select.IntervalCompositor, `composite_params` its keyword arguments); the pictures are kept as `interval_patches`.
    Intervals and SRT times are untouched.  What it gains on real footage is not measured here.
    composite_params={"streaming": True, ...} with interval_image="min" | "max" | "mean": the same pictures, byte for byte, made in the
    selector's own pass (frame_select.StreamingCompositor folds each staged batch while it is on the device; the frames whose fate is
    open wait in a small ring there), so the compositor's pass over the clip is saved and the option also works in one pass.  The other
    keys it takes: `trim_seconds`, `stream_fn`, and `keep_patches` (one pass drops a picture once its frame is recognised, a film has
    thousands of about 1 MB each; True keeps them as `interval_patches`, as several passes always do).  `streaming` and `keep_patches`
    are this class's own and are taken out before the rest reaches a compositor; a falsy `streaming` is the run without the key.  Not with
    interval_image="middle", interval_text="fused", interval_frame="sharpest" or shard.
    interval_image="quantile" (change / hold selector): the picture is instead the per-pixel quantile over time (default 0.5, the median)
    of up to `samples` (default 15) evenly spaced frames of the interval (frame_select.IntervalQuantile, `composite_params` its keyword
    arguments: quantile, samples, trim_seconds, rank_fn).  The median needs no knowledge of the text's polarity, and a minority of
    outlier frames (a flash, a black frame, a cut found one frame late) cannot move it, where a single one ruins `min` / `max`; only
    the samples are uploaded.  Exact over the trimmed interval when it has at most `samples` frames, an estimate from `samples` frames
    otherwise.  Not available with frame_selector="fps" or interval_text="fused", nor as it stands in one pass.  What it gains on real
    footage is not measured here either.
    composite_params={"streaming": True, "ring_seconds": S, ...} with interval_image="quantile": the same pictures, byte for byte, made
    in the selector's own pass, which also works in one pass (a pipe): the area band of every frame is parked in a ring on the device
    and a subtitle's samples are ranked there once its end is known (frame_select.StreamingQuantile, vse_interval_ring_rank), which
    also saves the quantile's own decode and upload in several passes.  `ring_seconds` must be given: the ring is device memory that
    the caller grants (about 1.2 MB per frame of a 1080p default band), and {"streaming": True} alone stays the ValueError it was.  It
    is a policy, and the command line takes 60: every subtitle whose trimmed range is at most that long is ranked on exactly the
    several-pass samples; a longer one whose first sample has left the ring is ranked on samples of its last ring_seconds or so and
    counted in `clamped_quantiles`, with one warning per clip.  The other keys it takes: `quantile`, `samples`, `trim_seconds`,
    `ring_fn` and `keep_patches`.  Not with interval_text="fused", interval_frame="sharpest" or shard: fusion in one pass needs whole
    frames, not bands.
    interval_text="fused" (change / hold selector with interval_image="middle" only; default "single", the above): the other answer to
    that single frame, in probability space: up to `samples` frames of each interval go through the recogniser, the boxes detected
    once on the sample nearest to the middle frame, and the recogniser's per-step class probabilities are averaged on the device before
    the CTC decode (frame_select.IntervalFuser, `fuse_params` its keyword arguments; fuse_fn defaults to ocr.predict_fused).  Each
    task then carries its interval's (dt_box, rec_res), kept as `interval_results`, and is not recognised again.  It needs no knowledge
    of the text's polarity; the recogniser runs once per sample.  What it gains on real footage is not measured here either.
    sub_area="auto": nobody drew a box, so run() first looks for the subtitle band itself, one more pass over the clip's frames
    on the device (area_locator.AreaLocator, `area_params` its keyword arguments), keeps what it found as `located_area` and goes
    on exactly as if that area had been passed; when it finds none it warns and goes on exactly as with sub_area=None.  With
    `shard`, every rank scans the same frames and gets the same integers, hence the same area.
    change_params={"edge_thresh": "auto"} (frame_selector "change" or "hold"): the selectors' constant 128 describes white text with a
    black outline; on yellow, shadowed, unoutlined or washed-out subtitles no pixel reaches it and the SRT comes out empty.  "auto"
    chooses the threshold for this clip before the selector is built (area_locator.AreaLocator(edge_thresh="auto"), `area_params` its
    keyword arguments; the selectors keep taking integers) and keeps it as `edge_thresh`: with sub_area="auto" the one locator pass
    yields the area and the threshold, with a given area one calibration pass runs over the area's rows.  When no threshold scores
    (no subtitles, or a textured background that moves behind them: the calibration uses the change automaton unless
    `automaton="hold"`) it warns and uses 128.  How the choice behaves on real footage is not measured here.
    change_params={"text_colour": "#RRGGBB" | a name | (B, G, R), "colour_tol": 48} (frame_selector "change" or "hold", in several passes
    and in one): coloured subtitles over a background with many luma edges.  The selector, whichever of the classes above it is, builds
    its masks on the colour key of the band (frame_select.ColourKey, vse_colour_key: 255 on the colour, 0 from colour_tol levels away in
    any channel) instead of on its luma; the locator and the calibration do the same, with area_params' own text_colour / colour_tol
    where it names them (not with a locator or calibration in the selector's own pass, whose key is the selector's).  The compositors,
    the quantile, the fuser and the recogniser keep the frames as they are.  `colour_key` is the ColourKey, `key_fn` what takes it (an
    EngineKey on the shim's device; change_params={"key_fn": callable} gives another).  colour_tol=48 is a guess checked on a synthetic
    clip only; the colour is not chosen automatically, BGR is the only colour space, and accurate mode and the fps sampler build no mask.
    area_params={"automaton": "hold"}: the locator and the calibration count held edges (area_locator's module text), which is what a
    textured background that moves behind the subtitles needs; with frame_selector="hold" they take the selector's hold_seconds /
    hold_frames from change_params unless area_params sets its own.  Opt-in: without it nothing changes.
    area_params={"automaton": "hold", "max_hold_seconds": 12} (or "max_hold_frames"): the locator pass, and the calibration pass with a
    given area, count only edges whose run is hold .. max_hold frames long (area_locator's module text has the limits), which is what
    a busy background that stands still behind the subtitles needs: on held edges alone its cells fall to the logo rule and neither
    an area nor a threshold is found.  It is NOT inherited from change_params as hold_seconds is: runs that set the selector's
    max_hold_* together with automaton="hold" keep their results, and the locator bounds its runs only when area_params says so.
    area_params={"streaming": True} with change_params={"edge_thresh": "auto"}, frame_selector="change" and a given area: the threshold is
    chosen in the selector's own pass instead of a calibration pass of its own (frame_select.CalibratingChangeSelector: the calibration's
    cells tile the selector's area and share its mask, so one kernel, vse_frame_cells_counts, gives the calibration's totals and the
    selector's counts at every candidate threshold), which saves a decode and an upload of the band in several passes and is what makes
    "auto" work in one pass (a pipe).  `calibrate_seconds`: S decides after round(S * fps) frames, None (several passes only) after the
    whole clip; the threshold, intervals, recognised frames, raw_lines and SRT are those of the run without the key whose area_params
    say probe=(1, that many frames).  In one pass S must be given: until the decision a frame is kept while ANY of the eight candidates'
    trackers may still want it (by the rule below, per candidate, plus the middle frames of the intervals a candidate has closed), and the
    window bounds that; `retain_bytes` stays the fallback behind it, `peak_retained` reports what was held, and after the decision the
    frames only other thresholds wanted go.  The command line takes 300 s for a pipe: a policy, not a measurement.  `streaming`,
    `calibrate_seconds`, `cells_counts_fn` and `export_fn` (the selector's callables; default the GPU's) are this class's own and are taken
    out before the rest reaches the locator; `edge_scores` and `frames_calibrated` say what the choice rests on.  Refused with the key,
    by name: frame_selector other than "change", automaton="hold" / max_hold_* in area_params, sub_area="auto" or None, mode="accurate",
    interval_frame="sharpest", composite_params' streaming, shard, probe; the key without edge_thresh="auto", and the other three keys
    without the key, mean nothing and are refused too.
    area_params={"streaming_locate": True} with sub_area="auto", frame_selector="change" and mode "fast" or "auto": the area is found in the
    selector's own pass instead of the locator's (frame_select.LocatingChangeSelector: the located rectangle lies a pixel off the locator's
    cell grid, so the cells' counts cannot be summed for it; instead the locator's kernel keeps its edge masks, one bit per pixel and
    threshold, vse_frame_cells_masks, and once the area is decided vse_frame_masks_replay counts it out of them, integer for integer
    vse_frame_change's rows), which saves a decode and an upload in several passes and is what makes sub_area="auto" work in one pass (a
    pipe).  change_params' edge_thresh may be an integer or "auto", which is then decided in the same pass and needs no "streaming" key;
    the two keys together are refused.  `locate_seconds`: S decides after round(S * fps) frames, None (several passes only) after the
    whole clip; located area, threshold, intervals, recognised frames, raw_lines and SRT are those of the run without the key whose
    area_params say probe=(1, that many frames).  In one pass S must be given: any frame of the window may become a middle frame, so all of
    them are kept until the decision, and a window whose frames exceed `retain_bytes` is a ValueError as soon as the frame size is
    known (nothing is clamped silently inside the window; after the decision the rule below applies).  `mask_gib` (default 8: a policy,
    not a measurement; 33140 frames of 1080p at one threshold, 4142 at eight) bounds the masks on the device the same way.  No area found:
    the warning above, and the run continues without one, in one pass over the frames kept, in order, and the rest of the source.  The
    command line takes for a pipe the largest whole number of seconds up to 300 that fits both bounds: a policy, not a measurement.
    `streaming_locate`, `locate_seconds`, `mask_gib`, `cells_masks_fn` and `replay_fn` (the selector's callables; default the GPU's) are
    this class's own; `frames_located` says how many frames the area rests on.  Refused with the key, by name: frame_selector other than
    "change", automaton="hold" / max_hold_* / search_area / probe in area_params, area_params' streaming, interval_frame="sharpest",
    composite_params' streaming, shard, mode="accurate", a sub_area that is not "auto"; the other keys without the key mean nothing and are
    refused too.
    area_params={"streaming_locate_hold": True} with sub_area="auto", frame_selector="hold" and mode "fast" or "auto": the same for the hold
    selector, the only one that works when a textured background moves behind the subtitle, where the change automaton finds neither an
    area nor a threshold (frame_select.LocatingHoldSelector: the held locator's kernel keeps the EDGE words it builds anyway,
    vse_frame_cells_hold_masks, and once the area is decided vse_frame_masks_replay_hold walks the located rectangle's pixels through
    them with the selector's hold, integer for integer vse_frame_hold's rows and state).  A sibling key, because "streaming_locate" keeps
    refusing frame_selector="hold" and automaton="hold" by name; the two together are refused.  The key implies automaton="hold" for the
    locator (giving it is accepted), whose hold follows the selector's hold_seconds / hold_frames unless area_params sets its own.
    `locate_seconds` and `mask_gib` are the other key's, with its meaning, bounds and error texts; `cells_hold_masks_fn` and
    `replay_hold_fn` are the selector's callables (default the GPU's); `located_area`, `edge_thresh`, `edge_scores` and `frames_located`
    are filled as there, and the results are those of the run without the key whose area_params say automaton="hold" and probe=(1, that
    many frames).  In one pass sub_area="auto" and edge_thresh="auto" are accepted with it; the window's frames are kept on the host until
    the decision, after which the hold selector's rows trail its frames by hold - 1 as always.  The held locator's limits carry over, and
    nothing is measured on real footage.  Refused with the key, by name: streaming_locate together with it, frame_selector other than
    "hold", an automaton other than "hold", max_hold_* in area_params or change_params, search_area, probe, area_params' streaming,
    interval_frame="sharpest", composite_params' streaming, shard, mode="accurate", a sub_area that is not "auto".
    area_params={"streaming_locate_bounded": True} with sub_area="auto", frame_selector="hold", max_hold_seconds / max_hold_frames in
    change_params AND in area_params, and mode "fast" or "auto": the same for the hold selector with bounded runs, the one for a busy
    background that stands still behind the subtitle (an interview, a news desk, an animation still, a logo in the band), where the
    unbounded selector merges the subtitles and the held locator scores nothing (frame_select.LocatingBoundedHoldSelector: the bounded
    locator's kernel keeps the EDGE words it builds anyway, vse_frame_cells_hold_bounded_masks, and once the area is decided
    vse_frame_masks_replay_hold_bounded walks the located rectangle's pixels through them with the selector's hold and max_hold, integer
    for integer vse_frame_hold_bounded's rows and state).  A third sibling key, because the two others keep refusing max_hold_* by name;
    any two together are refused.  The key implies automaton="hold"; the locator's bound is area_params' own and is NOT inherited from
    change_params' (nor the other way round): both are required.  `locate_seconds` and `mask_gib` are the other keys', with their
    meaning, bounds and error texts; `cells_bounded_masks_fn` and `replay_bounded_fn` are the selector's callables (default the GPU's);
    the results are those of the run without the key whose area_params say automaton="hold", max_hold_* and probe=(1, that many frames).
    In one pass sub_area="auto" and edge_thresh="auto" are accepted with it; the window's frames are kept on the host until the decision,
    after which the selector's rows trail its frames by max_hold as always with a bound.  The bounded locator's limits carry over (a gap
    between two subtitles shorter than max_hold comes back as an interval, a subtitle shown for longer than max_hold vanishes); max_hold
    12-15 s and the window are guesses, nothing is measured on real footage.  Refused with the key, by name: either other locate key
    together with it, frame_selector other than "hold", an automaton other than "hold", search_area, probe, area_params' streaming,
    interval_frame="sharpest", composite_params' streaming, shard, mode="accurate", a sub_area that is not "auto".
    one_pass (None: exactly when the source has no `read`, e.g. ingest.Y4mStream over a pipe; True forces it on a seekable source and
    halves its decode work; False on a sequential source is a ValueError): the clip is read once, in decode order.  frame_selector="fps":
    frame `no` is a task iff (no - 1) % max(1, int(fps // extract_frequency)) == 0 (fps_tasks' rule without the frame count); tasks go
    to OCR `batch` at a time and nothing is kept.  "change" / "hold" with an area in fast / auto mode: the selector yields batch by batch
    (iter_run), the middle frames of the intervals that closed are recognised `batch` at a time, and frames are kept only while they can
    still become a middle frame: with t the last frame whose row the tracker has seen and s the start of the open run, frames
    >= (s + t) // 2 (the middle can only move forward from there), frames > t without an open run, and the middle frames not yet
    recognised; a run of L frames holds about L / 2 frames plus the batches in flight.  `retain_bytes` (default 4 GiB, a policy, not a
    measurement: about 1380 frames of 1080p 4:2:0, so runs up to about 2700 frames stay exact) bounds them: when an open run exceeds
    it, its oldest kept frame goes and that interval is recognised on max(middle, oldest frame still kept); start and end, hence the
    SRT times, are untouched; `clamped_intervals` counts them and one warning is logged per run.  Where no interval was clamped, the
    intervals, the frames recognised, raw_lines and the SRT equal those of the multi-pass run() on the same frames with the same
    arguments (recognition does not depend on how frames are grouped into batches: tests/test_gpu_ragged.py).  Refused in one pass,
    because they need a second look at frames already gone: sub_area="auto" (unless area_params says "streaming_locate", "streaming_locate_hold" or "streaming_locate_bounded"), mode="accurate" with an area, interval_image other than
    "middle" (unless composite_params says "streaming": min / max / mean and the quantile), interval_text="fused", shard, change_params' edge_thresh="auto" (unless area_params says "streaming" or one of the three locate keys).
    interval_frame="sharpest" (change / hold selector with interval_image="middle" and interval_text="single" only; default "middle", all
    of the above): the one frame an interval is recognised on is chosen instead of being the middle one, which in compressed video is as
    likely as any other to be a coarse B-frame, a half-faded frame or a flash.  In the selector's own pass over the staged area rows the
    device scores every frame by the gradients of the edge pixels that already stood one frame earlier (vse_frame_focus through the
    selector's focus_fn; the rows are kept as `focus`), and each interval's rep becomes frame_select.sharpest_rep: the largest focus
    among the frames that `trim_seconds` leaves at either end, the earliest of equals.  `frame_params`: trim_seconds (default 0.25) and
    focus_fn (default frame_select.EngineFocus on the shim's device).  It needs no second look, so it is the one protection against a bad
    middle frame that works in one pass, with the same intervals, recognised frames, raw_lines and SRT as in several passes; one pass then
    keeps a frame only while it can still become its interval's rep: with T = round(trim_seconds * fps), of an open run s..t the frames
    >= (s + t) // 2 while t - s < 2 T, afterwards the frames > t - T and the best frame so far among s + T .. t - T: about 2 T + 1 frames
    plus the batches in flight however long the run, instead of half the run; `retain_bytes` remains the fallback behind it.  What it gains
    in recognition on real footage is not measured here (no real clips, stand-in recogniser weights).  Known limit: edges of a static
    background count alike in every frame, and on a busy static shot the score also rewards the background's sharpness."""

    def __init__(self, source, ocr, detect_batch=None, sub_area=None, mode="fast", language="ch", extract_frequency=3,
                 default_subtitle_area=None, drop_score=0.75, deviation_rate=0.0, threshold=80, batch=64,
                 watermark_decide=None, scene_text_decide=lambda band: True, shard=None, gather_device=None,
                 word_segmentation=False, segment=None, uploader=None, detect_stream=None, frame_selector="fps", change_params=None,
                 change_counter=None, delete_empty=True, area_params=None, interval_image="middle", composite_params=None,
                 interval_text="single", fuse_params=None, one_pass=None, retain_bytes=4 << 30, interval_frame="middle",
                 frame_params=None):
        if frame_selector not in ("fps", "change", "hold"):
            raise ValueError(f"frame_selector must be 'fps', 'change' or 'hold', not {frame_selector!r}")
        if interval_image not in INTERVAL_IMAGES:
            raise ValueError(f"interval_image must be one of {INTERVAL_IMAGES}, not {interval_image!r}")
        if interval_image != "middle" and frame_selector not in ("change", "hold"):
            raise ValueError(f"interval_image={interval_image!r} composites the intervals of frame_selector='change' or 'hold', not {frame_selector!r}")
        if interval_text not in ("single", "fused"):
            raise ValueError(f"interval_text must be 'single' or 'fused', not {interval_text!r}")
        # composite_params={"streaming": True}: the pictures are made in the selector's own pass (frame_select.StreamingCompositor, or
        # StreamingQuantile for interval_image="quantile").
        # The keys that are this class's own, `streaming` and `keep_patches`, are taken out here; what remains goes to the compositor.
        composite_params = None if composite_params is None else dict(composite_params)
        self.streaming = bool(composite_params.pop("streaming", False)) if composite_params else False
        self.keep_patches = bool(composite_params.pop("keep_patches", False)) if composite_params and self.streaming else False
        if not self.streaming:
            own = sorted(set(composite_params or {}) & {"keep_patches", "stream_fn", "ring_fn", "ring_seconds"})
            if own:
                raise ValueError(f"composite_params: {own} belong to composite_params={{'streaming': True}} and mean nothing without it")
        if self.streaming:
            option = "composite_params={'streaming': True}"
            if interval_image not in frame_select.COMPOSITE_MODES + ("quantile",):
                raise ValueError(f"{option} makes the min / max / mean picture of each interval in the selector's own pass; "
                                 f"interval_image={interval_image!r} is not one of them")
            if interval_text != "single":
                raise ValueError(f"{option} does not combine with interval_text={interval_text!r}")
            if shard is not None:
                raise ValueError(f"{option} composites every interval where the selector runs; it does not combine with shard={shard!r}")
            if interval_image == "quantile":
                if "ring_seconds" not in composite_params:
                    raise ValueError(f"{option} with interval_image='quantile' keeps the area's rows of every frame in a ring on the device "
                                     "until a subtitle's end is known: say how many seconds of them with ring_seconds (the command line "
                                     "takes 60; about 1.2 MB per frame of a 1080p band)")
                unknown = set(composite_params) - {"quantile", "samples", "trim_seconds", "ring_seconds", "ring_fn"}
                if unknown:
                    raise ValueError(f"{option} with interval_image='quantile' takes quantile, samples, trim_seconds, ring_seconds, ring_fn "
                                     f"and keep_patches beside it, not {sorted(unknown)}")
            else:
                unknown = set(composite_params) - {"trim_seconds", "stream_fn"}
                if unknown:
                    raise ValueError(f"{option} takes trim_seconds, stream_fn and keep_patches beside it, not {sorted(unknown)}")
        if interval_text == "fused" and (frame_selector not in ("change", "hold") or interval_image != "middle"):
            raise ValueError(f"interval_text='fused' reads the intervals of frame_selector='change' or 'hold' (not {frame_selector!r}) from their "
                             f"own frames, interval_image='middle' (not {interval_image!r}): composites and fused posteriors do not combine")
        if interval_frame not in INTERVAL_FRAMES:
            raise ValueError(f"interval_frame must be one of {INTERVAL_FRAMES}, not {interval_frame!r}")
        if interval_frame == "sharpest":
            for name, value, wanted in (("frame_selector", frame_selector, ("change", "hold")), ("interval_image", interval_image, ("middle",)),
                                        ("interval_text", interval_text, ("single",))):
                if value not in wanted:
                    raise ValueError(f"interval_frame='sharpest' chooses the one frame an interval of frame_selector='change' or 'hold' is "
                                     f"recognised on (interval_image='middle', interval_text='single'); it does not combine with {name}={value!r}")
            unknown = set(frame_params or {}) - {"trim_seconds", "focus_fn"}
            if unknown:
                raise ValueError(f"frame_params takes trim_seconds and focus_fn, not {sorted(unknown)}")
        self.interval_frame, self.frame_params, self.focus = interval_frame, frame_params, None
        self.source, self.ocr, self.detect_batch = source, ocr, detect_batch
        # area_params={"streaming": True}: the threshold of edge_thresh="auto" is chosen in the selector's own pass
        # (frame_select.CalibratingChangeSelector).  The keys that are this class's own, `streaming`, `calibrate_seconds`, `cells_counts_fn`
        # and `export_fn`, are taken out here; what remains goes to the locator.
        area_params = None if area_params is None else dict(area_params)
        self.calibrating = bool(area_params.pop("streaming", False)) if area_params else False
        if not self.calibrating:
            own = sorted(set(area_params or {}) & {"calibrate_seconds", "cells_counts_fn", "export_fn"})
            if own:
                raise ValueError(f"area_params: {own} belong to area_params={{'streaming': True}} and mean nothing without it")
        self.calibrate_seconds = area_params.pop("calibrate_seconds", None) if self.calibrating else None
        self._calibrate_fns = (area_params.pop("cells_counts_fn", None), area_params.pop("export_fn", None)) if self.calibrating else None
        # area_params={"streaming_locate": True}: sub_area="auto" is found in the selector's own pass (frame_select.LocatingChangeSelector).
        # Its keys, `streaming_locate`, `locate_seconds`, `mask_gib`, `cells_masks_fn` and `replay_fn`, are taken out here as well.
        # area_params={"streaming_locate_hold": True}: the same for frame_selector="hold" on held edges (frame_select.LocatingHoldSelector),
        # a sibling key with callables of its own, `cells_hold_masks_fn` and `replay_hold_fn`; `locate_seconds` and `mask_gib` go with either.
        # area_params={"streaming_locate_bounded": True}: the same for frame_selector="hold" with max_hold_* on bounded runs
        # (frame_select.LocatingBoundedHoldSelector), a third sibling with `cells_bounded_masks_fn` and `replay_bounded_fn`.
        # `locating` is set by all three keys, `locating_hold` and `locating_bounded` say which.
        self.locating_bounded = bool(area_params.pop("streaming_locate_bounded", False)) if area_params else False
        self.locating_hold = bool(area_params.pop("streaming_locate_hold", False)) if area_params else False
        self.locating = bool(area_params.pop("streaming_locate", False)) if area_params else False
        if self.locating_bounded and (self.locating or self.locating_hold):
            other = "streaming_locate" if self.locating else "streaming_locate_hold"
            raise ValueError("area_params={'streaming_locate_bounded': True} finds the area for frame_selector='hold' with max_hold_* and "
                             f"area_params={{'{other}': True}} for frame_selector={'change' if self.locating else 'hold'!r}"
                             f"{'' if self.locating else ' with unbounded runs'}; it does not combine with {other}, give one of them")
        if self.locating and self.locating_hold:
            raise ValueError("area_params={'streaming_locate_hold': True} finds the area for frame_selector='hold' and area_params="
                             "{'streaming_locate': True} for frame_selector='change'; it does not combine with streaming_locate, give one of them")
        locating_change = self.locating
        self.locating = self.locating or self.locating_hold or self.locating_bounded
        self._locate_key = ("streaming_locate_bounded" if self.locating_bounded else
                            "streaming_locate_hold" if self.locating_hold else "streaming_locate")
        change_fns, hold_fns = {"cells_masks_fn", "replay_fn"}, {"cells_hold_masks_fn", "replay_hold_fn"}
        bounded_fns = {"cells_bounded_masks_fn", "replay_bounded_fn"}
        if not self.locating:
            own = sorted(set(area_params or {}) & ({"locate_seconds", "mask_gib"} | change_fns))
            if own:
                raise ValueError(f"area_params: {own} belong to area_params={{'streaming_locate': True}} and mean nothing without it")
        for other, fns, given in (("streaming_locate", change_fns, locating_change), ("streaming_locate_hold", hold_fns, self.locating_hold),
                                  ("streaming_locate_bounded", bounded_fns, self.locating_bounded)):
            own = sorted(set(area_params or {}) & fns)
            if own and not given:                 # the callables of a key that is not set
                raise ValueError(f"area_params: {own} belong to area_params={{'{other}': True}} and mean nothing without it")
        self.locate_seconds = area_params.pop("locate_seconds", None) if self.locating else None
        self.mask_gib = area_params.pop("mask_gib", 8) if self.locating else None
        names = (("cells_bounded_masks_fn", "replay_bounded_fn") if self.locating_bounded else
                 ("cells_hold_masks_fn", "replay_hold_fn") if self.locating_hold else ("cells_masks_fn", "replay_fn"))
        self._locate_fns = tuple(area_params.pop(k, None) for k in names) if self.locating else None
        self.auto_area, self.area_params, self.located_area = isinstance(sub_area, str) and sub_area == "auto", area_params, None
        self.sub_area, self.mode, self.language = None if self.auto_area else sub_area, mode, language
        self.extract_frequency, self.default_subtitle_area = extract_frequency, default_subtitle_area
        self.drop_score, self.deviation_rate, self.threshold, self.batch = drop_score, deviation_rate, threshold, batch
        self.watermark_decide, self.scene_text_decide = watermark_decide, scene_text_decide
        self.shard, self.gather_device = shard, gather_device
        # staging.Uploader (or "auto": one on the shim's device when there is a GPU): detect_batch / predict_batch then receive
        # device uint8 tensors [n,H,W,3] staged through pinned memory by a producer thread instead of lists of host frames
        self.uploader = uploader
        # accurate mode with an uploader: detect_stream(iterable of device batches) -> generator of detect_batch results (the
        # detector of the next chunks stays in flight); ocr.predict_with_dets, when it exists, recognises from those boxes
        self.detect_stream = detect_stream
        self.word_segmentation, self.segment = word_segmentation, segment      # config.wordSegmentation (main.py:181-182)
        # change_params={"text_colour": ..., "colour_tol": ...}: the selector, and the locator and calibration unless area_params names a
        # colour of its own, build their masks on the colour key of the band (frame_select.ColourKey).  Both pairs become a `key_fn` here.
        if _key_names(change_params) and frame_selector not in ("change", "hold"):
            raise ValueError(f"change_params: {_key_names(change_params)} key the band of frame_selector='change' or 'hold', which build a "
                             f"mask; frame_selector={frame_selector!r} builds none")
        if _key_names(self.area_params) and (self.locating or self.calibrating):
            raise ValueError(f"area_params: {_key_names(self.area_params)} do not combine with a locator or calibration that runs in the "
                             "selector's own pass (streaming, streaming_locate*): there the key is the selector's, change_params' text_colour")
        change_params, self.colour_key = _key_params(change_params, "change_params")
        self.area_params, _own = _key_params(self.area_params, "area_params")
        self.key_fn = (change_params or {}).get("key_fn")
        self.frame_selector, self.change_params, self.change_counter = frame_selector, change_params, change_counter
        et = (change_params or {}).get("edge_thresh", 128)
        self.auto_thresh = isinstance(et, str) and et == "auto"
        if isinstance(et, str) and not self.auto_thresh:
            raise ValueError(f"change_params: edge_thresh must be an integer or 'auto', not {et!r}")
        self.edge_thresh = None if self.auto_thresh else et          # "auto": the integer run() resolves it to
        self.delete_empty = delete_empty          # config.deleteEmptyTimeStamp (intervals of the change selector only)
        self.interval_image, self.composite_params, self.interval_patches = interval_image, composite_params, None
        self.interval_text, self.fuse_params, self.interval_results = interval_text, fuse_params, None
        self.raw_lines = None
        self.short_lines = None
        self.intervals = None
        self.one_pass = (not hasattr(source, "read")) if one_pass is None else bool(one_pass)
        self.retain_bytes, self.clamped_intervals, self.peak_retained = retain_bytes, 0, 0
        self.edge_scores, self.frames_calibrated = None, 0       # area_params' streaming: the scores and the frames the choice rests on
        self.clamped_quantiles = 0        # streaming quantile: intervals that reached back beyond the ring (StreamingQuantile.clamped)
        if not self.one_pass and not hasattr(source, "read"):
            raise ValueError("one_pass=False needs a source with read(frame_no): this one is sequential and its frames cannot be looked at a second time")
        self.frames_located = 0           # area_params' streaming_locate: the frames the located area rests on
        if self.locating_bounded:
            option = "area_params={'streaming_locate_bounded': True}"
            bounds = {"max_hold_seconds", "max_hold_frames"}
            refused = [(f"frame_selector={frame_selector!r}", frame_selector != "hold"),
                       (f"automaton={self.area_params.get('automaton')!r}", self.area_params.get("automaton", "hold") != "hold"),
                       ("search_area in area_params", "search_area" in self.area_params),
                       ("probe in area_params (locate_seconds says how many frames decide)", "probe" in self.area_params),
                       ("area_params={'streaming': True}", self.calibrating),
                       (f"interval_frame={interval_frame!r}", interval_frame != "middle"),
                       ("composite_params={'streaming': True}", self.streaming), (f"shard={shard!r}", shard is not None),
                       (f"mode={mode!r}", mode not in ("fast", "auto")),
                       (f"sub_area={sub_area!r} (the key finds the area of sub_area='auto' and means nothing with another)", not self.auto_area)]
            for what, hit in refused:
                if hit:
                    raise ValueError(f"{option} finds the area of sub_area='auto' for frame_selector='hold' with max_hold_* while that "
                                     f"selector runs, with the held automaton on whole frames and bounded runs; it does not combine with "
                                     f"{what}, which needs the area from the first frame, counts other runs or has a pass of its own")
            for where, given in (("change_params", change_params or {}), ("area_params", self.area_params)):
                if all(given.get(k) is None for k in bounds):
                    raise ValueError(f"{option} needs max_hold_seconds or max_hold_frames in {where}: the selector's bound and the locator's "
                                     "are given each in its own place, neither is inherited from the other (without a bound the key is "
                                     "streaming_locate_hold)")
            self.area_params["automaton"] = "hold"            # (implied by the key)
        elif self.locating_hold:
            option = "area_params={'streaming_locate_hold': True}"
            held = sorted(set(self.area_params) & {"max_hold_seconds", "max_hold_frames"})
            held_sel = sorted(set(change_params or {}) & {"max_hold_seconds", "max_hold_frames"})
            refused = [(f"frame_selector={frame_selector!r}", frame_selector != "hold"),
                       (f"automaton={self.area_params.get('automaton')!r}", self.area_params.get("automaton", "hold") != "hold"),
                       (f"{held[0] if held else 'max_hold_seconds'} in area_params", bool(held)),
                       (f"{held_sel[0] if held_sel else 'max_hold_seconds'} in change_params", bool(held_sel)),
                       ("search_area in area_params", "search_area" in self.area_params),
                       ("probe in area_params (locate_seconds says how many frames decide)", "probe" in self.area_params),
                       ("area_params={'streaming': True}", self.calibrating),
                       (f"interval_frame={interval_frame!r}", interval_frame != "middle"),
                       ("composite_params={'streaming': True}", self.streaming), (f"shard={shard!r}", shard is not None),
                       (f"mode={mode!r}", mode not in ("fast", "auto")),
                       (f"sub_area={sub_area!r} (the key finds the area of sub_area='auto' and means nothing with another)", not self.auto_area)]
            for what, hit in refused:
                if hit:
                    raise ValueError(f"{option} finds the area of sub_area='auto' for frame_selector='hold' while that selector runs, with "
                                     f"the held automaton on whole frames and unbounded runs; it does not combine with {what}, which needs "
                                     "the area from the first frame, bounds the runs or has a pass of its own")
            self.area_params["automaton"] = "hold"            # (implied by the key)
        elif self.locating:
            option = "area_params={'streaming_locate': True}"
            held = sorted(set(self.area_params) & {"max_hold_seconds", "max_hold_frames"})
            refused = [(f"frame_selector={frame_selector!r}", frame_selector != "change"),
                       (f"automaton={self.area_params.get('automaton')!r}", self.area_params.get("automaton", "change") != "change"),
                       (f"{held[0] if held else 'max_hold_seconds'} in area_params", bool(held)),
                       ("search_area in area_params", "search_area" in self.area_params),
                       ("probe in area_params (locate_seconds says how many frames decide)", "probe" in self.area_params),
                       ("area_params={'streaming': True}", self.calibrating),
                       (f"interval_frame={interval_frame!r}", interval_frame != "middle"),
                       ("composite_params={'streaming': True}", self.streaming), (f"shard={shard!r}", shard is not None),
                       (f"mode={mode!r}", mode not in ("fast", "auto")),
                       (f"sub_area={sub_area!r} (the key finds the area of sub_area='auto' and means nothing with another)", not self.auto_area)]
            for what, hit in refused:
                if hit:
                    raise ValueError(f"{option} finds the area of sub_area='auto' for frame_selector='change' while that selector runs, with "
                                     f"the change automaton on whole frames; it does not combine with {what}, which needs the area from the "
                                     "first frame or has a pass of its own")
        if self.locating:
            if self.locate_seconds is not None and not self.locate_seconds > 0:
                raise ValueError(f"{option}: locate_seconds must be positive, not {self.locate_seconds!r}")
            if not self.mask_gib > 0:
                raise ValueError(f"{option}: mask_gib must be positive, not {self.mask_gib!r}")
            if self.one_pass and self.locate_seconds is None:
                raise ValueError(f"{option} in one pass needs locate_seconds: every frame of the window is kept until the area is decided, "
                                 "and the window bounds that (the command line takes what fits retain_bytes and mask_gib, at most 300, for a pipe)")
        if self.calibrating:
            option = "area_params={'streaming': True}"
            if not self.auto_thresh:
                raise ValueError(f"{option} chooses the threshold of change_params={{'edge_thresh': 'auto'}} in the selector's own pass and means "
                                 "nothing without it")
            held = sorted(set(self.area_params) & {"max_hold_seconds", "max_hold_frames"})
            refused = [(f"frame_selector={frame_selector!r}", frame_selector != "change"),
                       (f"automaton={self.area_params.get('automaton')!r}", self.area_params.get("automaton", "change") != "change"),
                       (f"{held[0] if held else 'max_hold_seconds'} in area_params", bool(held)),
                       ("sub_area='auto'", self.auto_area), ("sub_area=None", sub_area is None),
                       (f"mode={mode!r}", mode not in ("fast", "auto")),
                       (f"interval_frame={interval_frame!r}", interval_frame != "middle"),
                       ("composite_params={'streaming': True}", self.streaming), (f"shard={shard!r}", shard is not None),
                       ("probe in area_params (calibrate_seconds says how many frames decide)", "probe" in self.area_params)]
            for what, hit in refused:
                if hit:
                    raise ValueError(f"{option} decides the threshold of frame_selector='change' over a given sub_area while that selector "
                                     f"runs, with the change automaton on every frame; it does not combine with {what}, which needs the "
                                     "threshold from the first frame or has a calibration of its own")
            if self.calibrate_seconds is not None and not self.calibrate_seconds > 0:
                raise ValueError(f"{option}: calibrate_seconds must be positive, not {self.calibrate_seconds!r}")
            if self.one_pass and self.calibrate_seconds is None:
                raise ValueError(f"{option} in one pass needs calibrate_seconds: the window bounds the frames kept while eight thresholds "
                                 "are undecided (the command line takes 300 for a pipe)")
        if self.one_pass:
            refused = [("sub_area='auto'", self.auto_area and not self.locating),
                       ("mode='accurate' with a subtitle area", mode == "accurate" and sub_area is not None),
                       (f"interval_image={interval_image!r}", interval_image != "middle" and not self.streaming),
                       (f"interval_text={interval_text!r}", interval_text != "single"), (f"shard={shard!r}", shard is not None),
                       ("edge_thresh='auto'", self.auto_thresh and not self.calibrating and not self.locating)]
            for what, hit in refused:
                if hit:
                    raise ValueError(f"{what} is not available in one pass (a sequential source, or one_pass=True): it needs a second look "
                                     "at frames already gone")

    def _uploader(self):
        if self.uploader == "auto":
            self.uploader = staging.default_uploader() if hasattr(self.ocr, "predict_batch") else None
        return self.uploader

    def _decode_order(self, uploader):
        """The clip's frames for a selector: unconverted 4:2:0 planes where the source has them and an uploader converts them."""
        if uploader is not None and hasattr(self.source, "raw_frames"):
            return self.source.raw_frames()
        return self.source.frames()

    def _selects_intervals(self):
        return self.sub_area is not None and self.mode in ("fast", "auto") and self.frame_selector in ("change", "hold")

    def _locator(self, **kw):
        from . import area_locator
        params = {"batch": self.batch, **(self.area_params or {}), **kw}
        own = self.area_params or {}
        if params.get("automaton") == "hold" and self.frame_selector == "hold" and "hold_seconds" not in own and "hold_frames" not in own:
            # the locator and the calibration hold as long as the selector does, unless area_params says otherwise
            params.update({k: v for k, v in (self.change_params or {}).items() if k in ("hold_seconds", "hold_frames")})
        if self.auto_thresh and self.frame_selector in ("change", "hold"):
            params["edge_thresh"] = "auto"
        if self.key_fn is not None and "key_fn" not in own:
            params["key_fn"] = self.key_fn            # the locator and the calibration key as the selector does, unless area_params says otherwise
        return area_locator.AreaLocator(**params)

    def _keep_edge_thresh(self, loc):
        """change_params' edge_thresh="auto": what the locator chose, or 128 when no threshold scored (the locator has warned)."""
        from . import area_locator
        if loc.auto:
            self.edge_thresh = area_locator.DEFAULT_EDGE_THRESH if loc.edge_thresh is None else loc.edge_thresh

    def locate_area(self):
        """sub_area="auto": find the area (area_locator.AreaLocator over the clip in decode order) and make it this run's sub_area;
        with change_params' edge_thresh="auto" the same pass chooses the selector's threshold."""
        up = self._uploader()
        loc = self._locator()
        self.sub_area = self.located_area = loc.run(self._decode_order(up), self.source.fps, uploader=up)
        self._keep_edge_thresh(loc)
        if self.located_area is None:
            logging.getLogger(__name__).warning("sub_area='auto': no subtitle area found in %d frames; continuing without one "
                                                "(fps sampler, scene-text filtering)", loc.frames_scanned)
        return self.located_area

    def calibrate_edge_thresh(self):
        """change_params' edge_thresh="auto" with a given area: one pass over the area's rows (AreaLocator with search_area = the
        area) -> the threshold, kept as `edge_thresh`."""
        up = self._uploader()
        loc = self._locator(search_area=self.sub_area)
        loc.run(self._decode_order(up), self.source.fps, uploader=up)
        self._keep_edge_thresh(loc)
        return self.edge_thresh

    def _keep_calibration(self, sel):
        """area_params' streaming: what the selector decided in its own pass (128 for a clip without a frame)."""
        from . import area_locator
        self.edge_thresh = area_locator.DEFAULT_EDGE_THRESH if sel.edge_thresh is None else sel.edge_thresh
        self.edge_scores, self.frames_calibrated = sel.scores, sel.frames_scanned

    def _locate_window(self, first):
        """area_params' streaming_locate: the frames that decide, checked against what keeps them, as soon as the first frame says how
        large a frame is: the device mask buffer (mask_gib) and, in one pass, the frames themselves (retain_bytes)."""
        from . import area_locator
        fps = self.source.fps
        if self.locate_seconds is None:
            window = max(1, int(self.source.frame_count))
        else:
            window = int(round(self.locate_seconds * fps))
            if window < 1:
                raise ValueError(f"area_params: locate_seconds={self.locate_seconds!r} is less than one frame at {fps} fps")
        if first is None:
            return window
        h, w = first.shape[:2]
        if h >= 3 and w >= 3:
            gy, gx = area_locator.cells_dims(h, w)
            nt = len(self.area_params.get("thresholds", area_locator.AUTO_THRESHOLDS)) if self.auto_thresh else 1
            need, bound = window * nt * gy * gx * 64, int(self.mask_gib * (1 << 30))
            if need > bound:
                raise ValueError(f"area_params={{'{self._locate_key}': True}}: the masks of a window of {window} frames of {h} x {w} pixels at "
                                 f"{nt} threshold{'s' if nt > 1 else ''} take {need} bytes on the device, more than mask_gib={self.mask_gib} "
                                 f"({bound} bytes): give a shorter locate_seconds or a larger mask_gib / --mask-gib")
        if self.one_pass:
            need = window * _frame_nbytes(first)
            if need > self.retain_bytes:
                raise ValueError(f"area_params={{'{self._locate_key}': True}}: one pass keeps every frame of the window until the area is decided, "
                                 f"and {window} frames of {_frame_nbytes(first)} bytes are {need} bytes, more than retain_bytes={self.retain_bytes}: "
                                 "give a shorter locate_seconds or a larger retain_bytes / --retain-gib")
        return window

    def _keep_location(self, sel):
        """area_params' streaming_locate: what the selector decided in its own pass (AreaLocator's results by another road)."""
        from . import area_locator
        self.sub_area = self.located_area = sel.area
        if self.auto_thresh:
            self.edge_thresh = area_locator.DEFAULT_EDGE_THRESH if sel.edge_thresh is None else sel.edge_thresh
            self.edge_scores = sel.scores
        self.frames_located = sel.frames_scanned
        if sel.area is None:
            logging.getLogger(__name__).warning("sub_area='auto': no subtitle area found in %d frames; continuing without one "
                                                "(fps sampler, scene-text filtering)", sel.frames_scanned)

    def _locating_selector(self, window):
        if self.locating_hold or self.locating_bounded:
            params = {k: v for k, v in self.area_params.items() if k not in ("cells_fn", "batch")}
            if "hold_seconds" not in params and "hold_frames" not in params:
                # _locator's rule: the locator holds as long as the selector does, unless area_params says otherwise
                params.update({k: v for k, v in (self.change_params or {}).items() if k in ("hold_seconds", "hold_frames")})
            cls = frame_select.LocatingBoundedHoldSelector if self.locating_bounded else frame_select.LocatingHoldSelector
            return cls(self.change_counter, *self._locate_fns, window=window, batch=self.batch, locator_params=params,
                       **(self.change_params or {}))
        return frame_select.LocatingChangeSelector(self.change_counter, *self._locate_fns, window=window, batch=self.batch,
                                                   locator_params={k: v for k, v in self.area_params.items() if k not in ("cells_fn", "batch")},
                                                   **(self.change_params or {}))

    def _change_params(self):
        """The selector's keyword arguments, edge_thresh="auto" resolved to the integer."""
        if not self.auto_thresh:
            return self.change_params or {}
        return {**self.change_params, "edge_thresh": 128 if self.edge_thresh is None else self.edge_thresh}

    def _interval_selector(self):
        """The change or hold selector of this run (`_selects_intervals`); both take run / iter_run(frames, sub_area, fps, uploader)."""
        if self.calibrating:
            window = None if self.calibrate_seconds is None else int(round(self.calibrate_seconds * self.source.fps))
            if window is not None and window < 1:
                raise ValueError(f"area_params: calibrate_seconds={self.calibrate_seconds!r} is less than one frame at {self.source.fps} fps")
            params = {k: v for k, v in (self.change_params or {}).items() if k != "edge_thresh"}
            return frame_select.CalibratingChangeSelector(self.change_counter, *self._calibrate_fns, window=window, batch=self.batch,
                                                          locator_params={k: v for k, v in self.area_params.items() if k != "cells_fn"},
                                                          **params)
        cls = frame_select.ChangeFrameSelector if self.frame_selector == "change" else frame_select.HoldFrameSelector
        more = {}
        if self.interval_frame == "sharpest":
            more["focus_fn"] = (self.frame_params or {}).get("focus_fn") or frame_select.EngineFocus(shim._context())
        if self.streaming and self.interval_image == "quantile":
            more["compositor"] = self._compositor = frame_select.StreamingQuantile(**{"batch": self.batch, **self.composite_params})
        elif self.streaming:
            more["compositor"] = self._compositor = frame_select.StreamingCompositor(
                **{"mode": self.interval_image, **self.composite_params})
        return cls(self.change_counter, batch=self.batch, **self._change_params(), **more)

    def _trim_seconds(self):
        return (self.frame_params or {}).get("trim_seconds", 0.25)

    def select_tasks(self):
        s = self.source
        if self.sub_area is not None and self.mode == "accurate" and self.detect_batch is not None:
            up = self._uploader()
            sel = frame_select.AccurateFrameSelector(self.detect_batch, self.ocr.predict, self.sub_area, s.frame_count,
                                                     self.threshold, chunk=self.batch,
                                                     predict_batch=getattr(self.ocr, "predict_batch", None) and self._predict_list,
                                                     detect_stream=self.detect_stream,
                                                     predict_with_dets=getattr(self.ocr, "predict_with_dets", None))
            return [(t[0], t[1], t[2], t[3], None, None) for t in sel.run(self._decode_order(up), uploader=up)]
        if self.locating and self.sub_area is None and self.located_area is None:
            # the locator's pass folded into the selector's: one decode, and the area is known after the window
            up = self._uploader()
            frames = iter(self._decode_order(up))
            first = next(frames, None)
            sel = self._locating_selector(self._locate_window(first))
            intervals = sel.run(frames if first is None else itertools.chain([first], frames), None, s.fps, uploader=up)
            self._keep_location(sel)
            if sel.area is None:
                return fps_tasks(s.frame_count, s.fps, self.extract_frequency, self.default_subtitle_area)
            self.intervals = intervals
            return [(s.frame_count, rep, None, None, None, self.default_subtitle_area) for _start, _end, rep in self.intervals]
        if self._selects_intervals():
            up = self._uploader()
            sel = self._interval_selector()
            self.intervals = sel.run(self._decode_order(up), self.sub_area, s.fps, uploader=up)
            if self.calibrating:
                self._keep_calibration(sel)
            if self.streaming:
                self.interval_patches = self._compositor.patches
                self.clamped_quantiles = getattr(self._compositor, "clamped", 0)
            if self.interval_frame == "sharpest":
                self.focus = getattr(sel, "focus", None)            # (a clip without a frame leaves none, and no interval)
                self.intervals = [(start, end, frame_select.sharpest_rep(start, end, self.focus, s.fps, self._trim_seconds()))
                                  for start, end, _rep in self.intervals]
            return [(s.frame_count, rep, None, None, None, self.default_subtitle_area) for _start, _end, rep in self.intervals]
        return fps_tasks(s.frame_count, s.fps, self.extract_frequency, self.default_subtitle_area)

    def composite_intervals(self, n_tasks):
        """interval_image other than "middle": the picture of each interval this rank will recognise (with `shard`, the slice
        run_ocr_tasks gives it) -> the source run_ocr_tasks reads, which shows them in the rep frames."""
        up = self._uploader()
        if self.interval_image == "quantile":
            comp = frame_select.IntervalQuantile(**{"batch": self.batch, **(self.composite_params or {})})
        else:
            comp = frame_select.IntervalCompositor(**{"mode": self.interval_image, "batch": self.batch, **(self.composite_params or {})})
        only = None if self.shard is None else range(*parallel.shard_range(n_tasks, *self.shard))
        self.interval_patches = comp.run(self._decode_order(up), self.sub_area, self.intervals, self.source.fps, uploader=up, only=only)
        return CompositedSource(self.source, self.sub_area, self.interval_patches)

    def fuse_intervals(self, tasks):
        """interval_text="fused": the (dt_box, rec_res) of each interval this rank will report (with `shard`, the slice run_ocr_tasks
        gives it), read from several of its frames -> the tasks, those intervals' carrying their result."""
        up = self._uploader()
        params = {"batch": self.batch, **(self.fuse_params or {})}
        if params.get("fuse_fn") is None and hasattr(self.ocr, "predict_fused"):
            params["fuse_fn"] = self.ocr.predict_fused
        only = None if self.shard is None else range(*parallel.shard_range(len(tasks), *self.shard))
        self.interval_results = frame_select.IntervalFuser(**params).run(self._decode_order(up), self.intervals, self.source.fps, uploader=up,
                                                                          only=only, default_area=self.default_subtitle_area)
        return [t[:2] + tuple(self.interval_results[t[1]]) + t[4:] if t[1] in self.interval_results else t for t in tasks]

    def _predict_list(self, frames):
        return self.ocr.predict_batch(frames if not isinstance(frames, list) else _stack(frames))

    # ---- one pass ---------------------------------------------------------------------------------------------------------------
    def _recognise(self, frames, nos, uploader, patches=None):
        """raw.txt lines of the retained frames `nos`, through run_ocr_tasks like any other task list.  patches ({frame number: the
        area's picture}, a streaming composite): those frames are shown with it in the area (CompositedSource)."""
        tasks = [(getattr(self.source, "frame_count", None), no, None, None, None, self.default_subtitle_area) for no in nos]
        raw = patches is None and any(hasattr(frames[no], "pack_into") for no in nos)
        source = RetainedSource(frames, self.source.fps, raw)
        if patches is not None:
            source = CompositedSource(source, self.sub_area, patches)
        return run_ocr_tasks(source, tasks, self.ocr, self.sub_area, self.language, self.drop_score,
                             self.deviation_rate, self.batch, None, None, uploader)

    def _one_pass_fps(self, frames, uploader):
        step = max(1, int(self.source.fps // self.extract_frequency))
        lines, held = [], {}
        for no, frame in enumerate(frames, 1):
            if (no - 1) % step:
                continue
            held[no] = frame
            self.peak_retained = max(self.peak_retained, len(held))
            if len(held) == self.batch:
                lines += self._recognise(held, list(held), uploader)
                held = {}
        if held:
            lines += self._recognise(held, list(held), uploader)
        return lines

    def _one_pass_intervals(self, frames, uploader):
        if self.locating:
            # the area is found in this pass: until it is decided every frame of the window is kept, any of them may become a middle frame
            self.sub_area = self.located_area = None
            self.frames_located = 0
            frames = iter(frames)
            first = next(frames, None)
            sel = self._locating_selector(self._locate_window(first))
            if first is not None:
                frames = itertools.chain([first], frames)
            del first
        else:
            sel = self._interval_selector()
        batches = sel.iter_run(frames, self.sub_area, self.source.fps, uploader=uploader)
        # the recogniser's batches are staged while the selector's producer thread stages the next bands: a slab ring of their own
        ocr_up = uploader.sibling() if uploader is not None else None
        self.intervals = []
        kept, nbytes = {}, 0              # frame number -> full frame, and their bytes
        queue = []                        # rep frames of closed intervals, not yet recognised
        lines, no = [], 0
        # composite_params' streaming: the selector's compositor has the picture of every closed interval, under its middle frame
        comp = sel.compositor if self.streaming else None
        keep_patches = self.keep_patches

        def recognise(nos):
            got = self._recognise(kept, nos, ocr_up, None if comp is None else comp.patches)
            if comp is not None and not keep_patches:
                for no in nos:
                    comp.patches.pop(no, None)
            return got

        def still_kept(start, end, rep):
            """retain_bytes took frame `rep`: the oldest frame still kept at or behind it, inside the interval when there is one (of an
            interval that a candidate threshold closed long before the decision every frame may be gone: None)."""
            inside = [k for k in kept if rep <= k <= end] or [k for k in kept if start <= k < rep][-1:]
            return min(inside or [k for k in kept if k >= rep], default=None)

        sharpest = self.interval_frame == "sharpest"
        trim = int(round(self._trim_seconds() * self.source.fps)) if sharpest else 0
        # interval_frame="sharpest": the best frame so far of the open run starting at best_of, among its frames best_of + trim .. best_to
        best_of = best = None
        best_to = 0
        try:
            for items, closed in batches:
                for full, _band in items:
                    no += 1
                    kept[no] = full
                    nbytes += _frame_nbytes(full)
                self.peak_retained = max(self.peak_retained, len(kept))
                if self.locating:
                    if sel.decided and self.frames_located == 0:
                        self._keep_location(sel)
                    if sel.area is None:                 # undecided, or decided that there is none: nothing closes, everything stays
                        continue
                for start, end, rep in closed:
                    if sharpest:
                        rep = frame_select.sharpest_rep(start, end, sel.focus, self.source.fps, self._trim_seconds())
                    if rep not in kept:                   # the cap took it: the oldest frame of the interval that is still there
                        gone, rep = rep, still_kept(start, end, rep)
                        self.clamped_intervals += 1
                        if self.clamped_intervals == 1:
                            logging.getLogger(__name__).warning(
                                "one pass: the interval %d..%d outgrew retain_bytes=%d; it is recognised on frame %s instead of its %s "
                                "frame (its times are untouched; further such intervals are counted in clamped_intervals)",
                                start, end, self.retain_bytes, rep, self.interval_frame)
                        if rep is None:                   # nothing of it is left to recognise: it keeps its times and has no text
                            self.intervals.append((start, end, gone))
                            continue
                    if comp is not None and rep != (start + end) // 2:
                        comp.patches[rep] = comp.patches.pop((start + end) // 2)      # (a clamped interval: its picture goes with the frame shown)
                    self.intervals.append((start, end, rep))
                    queue.append(rep)
                while len(queue) >= self.batch:
                    lines += recognise(queue[:self.batch])
                    del queue[:self.batch]
                if self.calibrating and not sel.decided:
                    # the threshold is open: a frame stays while ANY candidate may still want it, by the rule below per candidate
                    # (at or behind the middle of its open run) or as the middle frame of an interval it has closed
                    t = sel.trackers[0].fed
                    floor = min(t + 1 if tr.open_start is None else (tr.open_start + t) // 2 for tr in sel.trackers)
                    reps = {rep for closed_by in sel.pending for _s, _e, rep in closed_by}
                    for k in [k for k in kept if k < floor and k not in reps]:
                        nbytes -= _frame_nbytes(kept.pop(k))
                    if nbytes > self.retain_bytes:
                        for k in sorted(k for k in kept if k < t):                          # frame t itself always stays
                            nbytes -= _frame_nbytes(kept.pop(k))
                            if nbytes <= self.retain_bytes:
                                break
                    continue
                t, open_start = sel.tracker.fed, sel.tracker.open_start
                floor = t + 1 if open_start is None else (open_start + t) // 2
                if sharpest and open_start is not None:
                    # a frame stays only while it can still become the rep (sharpest_rep): while the run is shorter than two trims its
                    # candidates lie at or behind its middle, as above; from then on they are open_start + trim .. end - trim, of which
                    # the frames up to t - trim are decided among themselves (the best so far, the earliest of equals) and the later ones not yet
                    if best_of != open_start:
                        best_of, best, best_to = open_start, None, open_start + trim - 1
                    if t - open_start >= 2 * trim:
                        for k in range(best_to + 1, t - trim + 1):
                            if best is None or sel.focus[k - 1, 1] > sel.focus[best - 1, 1]:
                                best = k
                        best_to, floor = t - trim, t - trim + 1
                for k in [k for k in kept if k < floor and k not in queue and not (sharpest and open_start is not None and k == best)]:
                    nbytes -= _frame_nbytes(kept.pop(k))
                if nbytes > self.retain_bytes and open_start is not None:
                    for k in sorted(k for k in kept if k < t and k not in queue):       # frame t itself always stays
                        nbytes -= _frame_nbytes(kept.pop(k))
                        if nbytes <= self.retain_bytes:
                            break
            if self.locating and self.frames_located == 0:
                self._keep_location(sel)               # (a clip that ended inside the window decides behind its last batch)
            if self.locating and sel.area is None:
                # no area: the run continues as it does without one, over the frames kept, in order, and the rest of the source
                self.intervals = None
                batches.close()
                held = [kept.pop(k) for k in sorted(kept)]
                return self._one_pass_fps(itertools.chain(_drain(held), frames), uploader)
            if queue:
                lines += recognise(queue)
            if keep_patches:
                self.interval_patches = comp.patches
            self.clamped_quantiles = getattr(comp, "clamped", 0)
            if sharpest:
                self.focus = getattr(sel, "focus", None)
            if self.calibrating:
                self._keep_calibration(sel)
        finally:
            batches.close()
            if ocr_up is not None:
                ocr_up.close()
        return lines

    def _run_one_pass(self):
        self.clamped_intervals = self.peak_retained = 0
        up = self._uploader()
        frames = self._decode_order(up)
        if self._selects_intervals() or self.locating:
            return self._one_pass_intervals(frames, up)
        return self._one_pass_fps(frames, up)

    def run(self):
        """-> SRT text.  raw_lines (normalised, as the reference rewrites raw.txt) and short_lines are kept on the object."""
        self.intervals = self.focus = None
        if self.one_pass:
            self.interval_patches = self.interval_results = None
            lines = self._run_one_pass()
        else:
            lines = self._run_multi_pass()
        if self.sub_area is None:
            if self.watermark_decide is not None:               # the reference asks on stdin (main.py:164-170)
                lines = raw_filters.filter_watermark(lines, self.watermark_decide)
            lines = raw_filters.filter_scene_text(lines, self.scene_text_decide) if lines else lines
        if self.intervals is not None:
            text, self.raw_lines = srt.generate_subtitle_file_intervals(lines, self.intervals, self.source.fps, self.threshold,
                                                                        getattr(self.source, "pos_msec", None), self.delete_empty)
            self.short_lines = []
        else:
            text, self.short_lines, self.raw_lines = srt.generate_subtitle_file(lines, self.source.fps, self.threshold,
                                                                                  getattr(self.source, "pos_msec", None))
        if self.word_segmentation:
            text, _ = text_cleanup.cleanup_srt(text, self.language, self.segment or text_cleanup.default_segmenter())
        return text

    def _run_multi_pass(self):
        if self.auto_thresh:
            self.edge_thresh = None
        if self.auto_area and self.locating:
            self.sub_area = self.located_area = None          # select_tasks finds it
            self.frames_located = 0
        elif self.auto_area:
            self.locate_area()
        elif self.auto_thresh and self._selects_intervals() and not self.calibrating:
            self.calibrate_edge_thresh()
        self.interval_patches = None
        tasks = self.select_tasks()
        source = self.source
        if self.streaming and self.intervals is not None:
            source = CompositedSource(self.source, self.sub_area, self.interval_patches)
        elif self.interval_image != "middle" and self.intervals is not None:
            source = self.composite_intervals(len(tasks))
        self.interval_results = None
        if self.interval_text == "fused" and self.intervals is not None:
            tasks = self.fuse_intervals(tasks)
        return run_ocr_tasks(source, tasks, self.ocr, self.sub_area, self.language, self.drop_score,
                             self.deviation_rate, self.batch, self.shard, self.gather_device, self._uploader())

    @staticmethod
    def srt2txt(srt_text):
        """main.py:1037-1043 (pysrt: every block's text, one block after the other)."""
        blocks = [b for b in re.split(r"\n(?=\d+\n\d\d:\d\d:\d\d,\d{3} --> )", srt_text) if b.strip()]
        return "".join(b.split("\n", 2)[2].rstrip("\n") + "\n" for b in blocks)


def _parse_area(text):
    if text == "auto":
        return "auto"
    parts = text.split(",")
    if len(parts) != 4 or not all(p.strip().lstrip("-").isdigit() for p in parts):
        raise ValueError(f"--area takes ymin,ymax,xmin,xmax or auto, not {text!r}")
    return SubtitleArea(*(int(p) for p in parts))


def tone_arguments(args):
    """--transfer, --white-nits, --peak-nits and --tone-curve of a parsed command line -> the keywords ingest.open_source takes for them."""
    params = {k: v for k, v in (("white_nits", args.white_nits), ("peak_nits", args.peak_nits), ("curve", args.tone_curve)) if v is not None}
    if args.transfer is None:
        if params:
            raise ValueError("--white-nits, --peak-nits and --tone-curve belong to --transfer pq | hlg")
        return {}
    return {"transfer": args.transfer, "tone_params": params or None}


def add_match_arguments(p):
    """--comb-thresh and --comb-limit of `--deinterlace match`, for the command lines that take it."""
    p.add_argument("--comb-thresh", type=int, default=None, metavar="N", help="--deinterlace match: a luma sample that stands out of the "
                   "rows above and below it by more than N 8-bit levels, the same way, is combed, 0..255 [10]")
    p.add_argument("--comb-limit", default=None, metavar="N|off", help="--deinterlace match: a frame whose best weave still has more than "
                   "N per mille of its luma samples combed is video and gets the adaptive rule, 0..1000; off: never [20]")


def match_arguments(args):
    """--comb-thresh and --comb-limit of a parsed command line -> the keywords ingest.open_source takes for them."""
    if args.comb_thresh is None and args.comb_limit is None:
        return {}
    if args.deinterlace != "match":
        raise ValueError("--comb-thresh and --comb-limit belong to --deinterlace match")
    out = {}
    if args.comb_thresh is not None:
        if not 0 <= args.comb_thresh <= 255:
            raise ValueError(f"--comb-thresh takes 0..255 (8-bit levels), not {args.comb_thresh}")
        out["comb_thresh"] = args.comb_thresh
    if args.comb_limit is not None:
        if args.comb_limit != "off" and not (args.comb_limit.isdigit() and int(args.comb_limit) <= 1000):
            raise ValueError(f"--comb-limit takes 0..1000 (per mille) or off, not {args.comb_limit!r}")
        out["comb_limit"] = None if args.comb_limit == "off" else int(args.comb_limit)
    return out


def add_colour_arguments(p):
    """--text-colour / --colour-tol of both command lines (colour_arguments reads them)."""
    p.add_argument("--text-colour", default=None, metavar="RRGGBB|name", help="coloured subtitles: build the edge masks on how near each "
                   "pixel is to this fill colour instead of on its luma, which tells the text from a background with many luma edges; "
                   "RRGGBB, #RRGGBB, or one of " + ", ".join(sorted(frame_select.COLOUR_NAMES)) + " [none: luma]")
    p.add_argument("--colour-tol", default=None, metavar="N", help="--text-colour: the largest channel difference, 1..255, at which a "
                   "pixel no longer counts as that colour [48, a guess checked on a synthetic clip only]")


def colour_arguments(args):
    """-> the frame_select.ColourKey the two options ask for, or None; ValueError, naming the option, for a bad value."""
    if args.text_colour is None:
        if args.colour_tol is not None:
            raise ValueError("--colour-tol is the tolerance of --text-colour and means nothing without it")
        return None
    tol = 48 if args.colour_tol is None else args.colour_tol
    if isinstance(tol, str):
        if not (tol.isdigit() and 1 <= int(tol) <= 255):
            raise ValueError(f"--colour-tol takes an integer 1..255, not {tol!r}")
        tol = int(tol)
    try:
        return frame_select.ColourKey(args.text_colour, tol)
    except ValueError as e:
        raise ValueError(f"--text-colour: {e}") from None


def add_square_arguments(p):
    """--square-pixels, --sar, --scale and --resample-filter, for the command lines that take them."""
    p.add_argument("--square-pixels", action="store_true", help="anamorphic YUV (DVD, HDV, DVCPRO HD, 1440-column broadcast): resample "
                   "every frame to square pixels on the GPU by the Y4M header's sample aspect ratio (its A token), so that the detector "
                   "and the recogniser see glyphs of their true width and --area is in display pixels; --size stays the stored size; "
                   "a ratio of 1:1 or none changes nothing [off]")
    p.add_argument("--sar", default=None, metavar="N:D", help="the sample aspect ratio, in the header's place (32:27 and 8:9 NTSC DVD, 16:11 "
                   "PAL DVD 16:9, 4:3 HDV); the only way for a headerless YUV file; turns --square-pixels on")
    p.add_argument("--scale", default=None, metavar="H|WxH", help="oversized YUV (UHD): scale every frame to H rows on the GPU before "
                   "anything else sees it, keeping the display aspect, or to W x H exactly; the detector, the recogniser and --area then "
                   "work in output pixels, --size stays the stored size; not with --deinterlace; the size the picture already has changes "
                   "nothing [off]")
    p.add_argument("--resample-filter", default=None, choices=("bicubic", "bilinear", "lanczos"), help="--square-pixels / --sar / --scale: "
                   "the filter [bicubic]")


def square_arguments(args):
    """--square-pixels, --sar, --scale and --resample-filter of a parsed command line -> the keywords ingest.open_source takes for them."""
    sar = None
    if args.sar is not None:
        num, sep, den = args.sar.partition(":")
        if not (sep and num.isdigit() and den.isdigit() and int(num) > 0 and int(den) > 0):
            raise ValueError(f"--sar takes NUM:DEN of positive integers, not {args.sar!r}")
        sar = (int(num), int(den))
    scale = None
    if getattr(args, "scale", None) is not None:
        parts = args.scale.lower().split("x")
        if not (1 <= len(parts) <= 2 and all(v.isdigit() and int(v) > 0 for v in parts)):
            raise ValueError(f"--scale takes H or WxH of positive integers, not {args.scale!r}")
        scale = int(parts[0]) if len(parts) == 1 else (int(parts[0]), int(parts[1]))
    if not args.square_pixels and sar is None:
        if scale is not None:
            return {"scale": scale, "resample_filter": args.resample_filter or "bicubic"}
        if args.resample_filter is not None:
            raise ValueError("--resample-filter belongs to --square-pixels, --sar N:D or --scale H|WxH")
        return {}
    out = {"square_pixels": True, "sar": sar, "resample_filter": args.resample_filter or "bicubic"}
    if scale is not None:
        out["scale"] = scale
    return out


def default_locate_seconds(source, raw, auto_thresh, retain_bytes, mask_gib, limit=300):
    """--streaming-locate on a pipe without --locate-seconds: the largest whole number of seconds, at most `limit`, whose frames fit
    retain_bytes on the host (`raw`: kept as the stream's own YUV bytes, else as BGR) and whose masks fit mask_gib on the device.  A
    policy, not a measurement: nobody has tried whether that much of a real film finds its band."""
    from . import area_locator
    h, w = int(source.height), int(source.width)
    if getattr(source, "resample", None) is not None and not raw:
        w = source.resample.out_width
    fmt = getattr(source, "fmt", None)
    per = 3 * h * w if not raw else (h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2) if fmt is None else fmt.frame_bytes(h, w))
    if raw and getattr(source, "deinterlace", None) is not None:
        per *= 2                          # (an interlaced frame pins its previous picture)
    gy, gx = area_locator.cells_dims(max(3, h), max(3, w))
    frames = min(retain_bytes // per, int(mask_gib * (1 << 30)) // ((len(area_locator.AUTO_THRESHOLDS) if auto_thresh else 1) * gy * gx * 64))
    seconds = min(int(limit), int(frames / source.fps))
    if seconds < 1:
        raise ValueError(f"--streaming-locate: not one second of {h} x {w} frames at {source.fps} fps fits --retain-gib and --mask-gib")
    return float(seconds)


def main(argv=None, ocr=None, counter=None, cells_fn=None, composite_fn=None, focus_fn=None, stream_fn=None, ring_fn=None,
         cells_counts_fn=None, export_fn=None, cells_masks_fn=None, replay_fn=None, cells_hold_masks_fn=None, replay_hold_fn=None,
         cells_bounded_masks_fn=None, replay_bounded_fn=None, key_fn=None):
    """ocr: the recogniser (None: shim.OcrRecogniser on the GPU, frames staged through staging.default_uploader, YUV 4:2:0 converted
    on the device); counter: the change / hold selector's count_fn (None: the GPU's); cells_fn: the locator's (None: the GPU's);
    composite_fn: what makes the picture of `--interval-image`, the compositor's accumulate_fn for min / max / mean and the quantile's
    rank_fn for quantile (None: the GPU's); focus_fn: what scores the frames of `--interval-frame sharpest` (None: the GPU's);
    stream_fn: what makes the min / max / mean pictures of `--streaming-composite`, StreamingCompositor's stream_fn (None: the GPU's);
    ring_fn: what makes its quantile pictures, StreamingQuantile's ring_fn (None: the GPU's); cells_counts_fn, export_fn: what counts
    and hands over for `--streaming-calibration`, CalibratingChangeSelector's cells_fn and export_fn (None: the GPU's); cells_masks_fn,
    replay_fn: what keeps and replays the masks for `--streaming-locate`, LocatingChangeSelector's cells_fn and replay_fn (None: the GPU's);
    cells_hold_masks_fn, replay_hold_fn: the same for `--streaming-locate-hold`, LocatingHoldSelector's cells_fn and replay_fn (None: the
    GPU's); cells_bounded_masks_fn, replay_bounded_fn: the same for `--streaming-locate-bounded`, LocatingBoundedHoldSelector's (None: the
    GPU's); key_fn: given the frame_select.ColourKey of `--text-colour`, what takes the key (None: frame_select.EngineKey on the GPU)."""
    p = argparse.ArgumentParser(prog="python -m vse_amd.extractor", description="Extract a video's hard subtitles to SRT on the GPU.  "
                                "`-` reads YUV4MPEG2 from standard input in one pass, e.g. "
                                "`ffmpeg -i film.mkv -pix_fmt yuv420p -f yuv4mpegpipe - | python -m vse_amd.extractor - -o film.srt`.")
    p.add_argument("video", help="`-` (YUV4MPEG2 on standard input), or a file: uncompressed BGR24 or Motion-JPEG AVI, a .npy frame stack, "
                   ".y4m, or headerless .yuv / .i420 / .nv12 / .p010")
    p.add_argument("-o", "--output", default=None, metavar="OUT.srt", help="write the SRT here [standard output]")
    p.add_argument("--fps", type=float, default=None, help="frame rate, for input that carries none (.npy, headerless YUV, Y4M with F0:0)")
    p.add_argument("--size", default=None, metavar="WxH", help="frame size of a headerless YUV 4:2:0 file")
    p.add_argument("--layout", default=None, choices=("i420", "nv12"), help="plane layout of a headerless YUV 4:2:0 file [by extension]")
    p.add_argument("--matrix", default="bt601", choices=("bt601", "bt709", "bt2020"), help="YUV -> BGR matrix [bt601]; Y4M carries no tag "
                   "for it, and HD encodes are normally BT.709; bt2020 needs --wide-yuv or --pix-fmt")
    p.add_argument("--wide-yuv", action="store_true", help="Y4M: also accept 9 to 16 bits, 4:2:2, 4:4:4, grey and full range (what "
                   "`ffmpeg -strict -1 -f yuv4mpegpipe` writes without `-pix_fmt yuv420p`), converted on the GPU")
    p.add_argument("--range", default="auto", choices=("auto", "limited", "full"), help="--wide-yuv / --pix-fmt: the colour range [auto: "
                   "the Y4M header's XCOLORRANGE or the pixel format's own, else limited]")
    p.add_argument("--pix-fmt", default=None, metavar="NAME", help="pixel format of a headerless YUV file by FFmpeg's name (yuv420p10le, "
                   "yuv422p, yuv444p, gray, p010le, yuvj420p ...) [by extension; .p010 is p010le]")
    p.add_argument("--deinterlace", default=None, choices=("adaptive", "interpolate", "match"), help="interlaced YUV (576i / 480i / 1080i: "
                   "Y4M with It / Ib, or a headerless file with --pix-fmt and --field-order): deinterlace on the GPU, weaving what stood still "
                   "(adaptive), interpolating the second field throughout, or, for film carried in interlaced video (3:2 pulldown, shifted "
                   "fields), weaving each frame with the partner field that combs least (match: the film's own pictures; a frame that "
                   "combs with every partner gets adaptive); turns --wide-yuv on")
    p.add_argument("--field-order", default="auto", choices=("auto", "tff", "bff"), help="--deinterlace: which field comes first [auto: the "
                   "Y4M header's It / Ib; Ip is then left as it is]; tff / bff override the header")
    p.add_argument("--deinterlace-thresh", type=int, default=10, metavar="N", help="--deinterlace adaptive: a sample that changed by more "
                   "than N 8-bit levels since the previous frame has moved, 0..255 [10]")
    add_match_arguments(p)
    add_square_arguments(p)
    p.add_argument("--transfer", default=None, choices=("pq", "hlg"), help="HDR video (needs --wide-yuv or --pix-fmt, normally with --matrix "
                   "bt2020): undo PQ (UHD Blu-ray, streaming masters) or HLG (UHD broadcast) and tone-map to SDR on the GPU; Y4M carries no tag "
                   "for it [none: the samples are taken as SDR and HDR material comes out flat]")
    p.add_argument("--white-nits", type=float, default=None, metavar="N", help="--transfer: the luminance that becomes SDR white [203]")
    p.add_argument("--peak-nits", type=float, default=None, metavar="N", help="--transfer, --tone-curve knee: the luminance that the "
                   "roll-off brings down to SDR white [1000]")
    p.add_argument("--tone-curve", default=None, choices=("knee", "clip"), help="--transfer: roll highlights off above 0.8 of SDR white, "
                   "or clip at SDR white [knee]")
    p.add_argument("--area", default=None, metavar="ymin,ymax,xmin,xmax|auto", help="the subtitle area in frame pixels, or `auto` to "
                   "look for it first (not in one pass) [none: the whole frame, fps sampler]")
    p.add_argument("--selector", default="fps", choices=("fps", "change", "hold"), help="which frames go to OCR [fps]")
    p.add_argument("--edge-thresh", default="128", metavar="auto|N", help="change / hold selector: the luma gradient that makes an edge "
                   "pixel, or `auto` to choose it for this clip first (not in one pass) [128]")
    add_colour_arguments(p)
    p.add_argument("--streaming-calibration", action="store_true", help="--selector change --edge-thresh auto with a given --area: choose "
                   "the threshold in the selector's own pass instead of a pass of its own, which also works in one pass (a pipe)")
    p.add_argument("--calibrate-seconds", type=float, default=None, metavar="S", help="--streaming-calibration: the threshold is chosen "
                   "on the first S seconds; until then one pass keeps the frames any of the eight candidate thresholds may want [a file: "
                   "the whole clip; `-`: 300, a policy, not a measurement: nobody has tried it on real films]")
    p.add_argument("--streaming-locate", action="store_true", help="--area auto --selector change: find the area in the selector's own pass "
                   "instead of a pass of its own, which also works in one pass (a pipe); --edge-thresh auto is chosen in that pass too")
    p.add_argument("--streaming-locate-hold", action="store_true", help="--area auto --selector hold: the same on held edges, for a "
                   "textured background that moves behind the subtitles (the locator counts with the hold automaton); takes --locate-seconds "
                   "and --mask-gib as --streaming-locate does")
    p.add_argument("--streaming-locate-bounded", action="store_true", help="--area auto --selector hold --max-hold-seconds S: the same on "
                   "bounded runs, for a busy background that stands still behind the subtitles (an interview, a news desk, a logo in the "
                   "band); the locator's bound is --locator-max-hold-seconds, and --max-hold-seconds when that is not given; takes "
                   "--locate-seconds and --mask-gib as --streaming-locate does")
    p.add_argument("--locate-seconds", type=float, default=None, metavar="S", help="--streaming-locate / --streaming-locate-hold / --streaming-locate-bounded: the area is found on the first S "
                   "seconds; until then one pass keeps every frame and the device one bit per pixel and threshold [a file: the whole "
                   "clip; `-`: the largest whole number of seconds up to 300 whose frames fit --retain-gib and --mask-gib, about 57 for "
                   "1080p 4:2:0 at 24 fps, a policy, not a measurement: nobody has tried whether a minute of a real film finds its band]")
    p.add_argument("--mask-gib", type=float, default=None, metavar="G", help="--streaming-locate / --streaming-locate-hold / --streaming-locate-bounded: bound on the masks kept on the device "
                   "until the area is found, GiB [8, a policy, not a measurement]")
    p.add_argument("--max-hold-seconds", type=float, default=None, metavar="S", help="--selector hold: count only edges that hold still for "
                   "at most S seconds, so a static busy background, a logo or a watermark drops out; a subtitle shown for longer drops out "
                   "too, and one pass keeps S seconds more of frames [none: no bound]")
    p.add_argument("--locator-automaton", default="change", choices=("change", "hold"), help="what `--area auto` and `--edge-thresh auto` "
                   "count: every edge pixel, or with `hold` only edges that hold still (a textured background that moves) [change]")
    p.add_argument("--locator-max-hold-seconds", type=float, default=None, metavar="S", help="--locator-automaton hold: `--area auto` and "
                   "`--edge-thresh auto` count only edges that hold still for at most S seconds (a busy background that stands still); "
                   "independent of --max-hold-seconds [none: no bound]")
    p.add_argument("--interval-image", default="middle", choices=INTERVAL_IMAGES, help="change / hold selector: what the recogniser is "
                   "shown for each subtitle: its middle frame, the per-pixel min (light text) / max (dark text) / mean of all its frames, "
                   "or the per-pixel quantile of a few evenly spaced ones, which needs no polarity and shrugs off a flash or a late cut "
                   "[middle].  Other than middle, they work in one pass only with --streaming-composite.")
    p.add_argument("--streaming-composite", action="store_true", help="--interval-image min / max / mean / quantile: make the pictures "
                   "in the selector's own pass instead of a pass of their own, which also works in one pass (a pipe)")
    p.add_argument("--quantile", type=float, default=0.5, metavar="Q", help="--interval-image quantile: 0..1, 0.5 the median [0.5]")
    p.add_argument("--interval-samples", type=int, default=15, metavar="K", help="--interval-image quantile: frames sampled per subtitle, "
                   "1..min(batch, 63), with --streaming-composite 1..63; exact when the subtitle has no more frames, an estimate "
                   "otherwise [15]")
    p.add_argument("--ring-seconds", type=float, default=None, metavar="S", help="--interval-image quantile --streaming-composite: the "
                   "area's rows of about this many seconds wait on the GPU (1.2 MB per frame of a 1080p band); a subtitle shown for "
                   "longer gets the quantile of its last S seconds or so [60]")
    p.add_argument("--interval-frame", default="middle", choices=INTERVAL_FRAMES, help="change / hold selector: which single frame of each "
                   "subtitle is recognised: its middle frame, or the one whose standing edges are sharpest, scored in the selector's own pass "
                   "(works in one pass; not with --interval-image other than middle) [middle]")
    p.add_argument("--mode", default="fast", choices=("fast", "auto", "accurate"))
    p.add_argument("--language", default="ch")
    p.add_argument("--frequency", type=int, default=3, help="frames per second the fps sampler looks at [3]")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--retain-gib", type=float, default=4.0, help="one pass: bound on the frames kept for the open subtitle, GiB [4]")
    p.add_argument("--txt", default=None, metavar="OUT.txt", help="also write the subtitles' text alone (srt2txt)")
    p.add_argument("--weights-dir", default=None, help="directory of <model id>.npz weight files")
    p.add_argument("--allow-standin-weights", action="store_true", help="run with seeded stand-in weights where a model's are missing")
    args = p.parse_args(argv)
    from . import ingest
    try:
        size = None
        if args.size is not None:
            w, sep, h = args.size.lower().partition("x")
            if not (sep and w.isdigit() and h.isdigit()):
                raise ValueError(f"--size takes WIDTHxHEIGHT, not {args.size!r}")
            size = (int(w), int(h))
        area = None if args.area is None else _parse_area(args.area)
        from .area_locator import parse_edge_thresh
        edge_thresh = parse_edge_thresh(args.edge_thresh)
        change_params = {} if edge_thresh == 128 else {"edge_thresh": edge_thresh}
        colour = colour_arguments(args)
        if colour is not None:
            if args.selector == "fps":
                raise ValueError("--text-colour keys the band of `--selector change` or `--selector hold`, which build a mask; `--selector "
                                 "fps` builds none")
            change_params.update({"text_colour": colour.bgr, "colour_tol": colour.tol} if key_fn is None else {"key_fn": key_fn(colour)})
        if args.max_hold_seconds is not None:
            if args.selector != "hold":
                raise ValueError(f"--max-hold-seconds bounds the runs of `--selector hold`, not of `--selector {args.selector}`")
            change_params["max_hold_seconds"] = args.max_hold_seconds
        if args.locator_max_hold_seconds is not None and args.locator_automaton != "hold" and not args.streaming_locate_bounded:
            raise ValueError(f"--locator-max-hold-seconds bounds the runs of `--locator-automaton hold`, not of `--locator-automaton "
                             f"{args.locator_automaton}`")
        calibration = {}
        if args.streaming_calibration:
            calibrate_seconds = 300.0 if args.calibrate_seconds is None and args.video == "-" else args.calibrate_seconds
            calibration = {"streaming": True, **({} if calibrate_seconds is None else {"calibrate_seconds": calibrate_seconds}),
                           **({} if cells_counts_fn is None else {"cells_counts_fn": cells_counts_fn}),
                           **({} if export_fn is None else {"export_fn": export_fn})}
        elif args.calibrate_seconds is not None:
            raise ValueError("--calibrate-seconds sets the window of --streaming-calibration and means nothing without it")
        if args.streaming_locate and args.streaming_locate_hold:
            raise ValueError("--streaming-locate finds the area for `--selector change` and --streaming-locate-hold for `--selector hold`: "
                             "give one of them")
        if args.streaming_locate_bounded and (args.streaming_locate or args.streaming_locate_hold):
            other = "--streaming-locate" if args.streaming_locate else "--streaming-locate-hold"
            raise ValueError(f"--streaming-locate-bounded finds the area for `--selector hold --max-hold-seconds S` and {other} for `--selector "
                             f"{'change' if args.streaming_locate else 'hold'}`{'' if args.streaming_locate else ' without a bound'}: give one "
                             "of them")
        locator_max_hold_seconds = args.locator_max_hold_seconds
        if args.streaming_locate_bounded and locator_max_hold_seconds is None and args.max_hold_seconds is not None:
            locator_max_hold_seconds = args.max_hold_seconds
            logging.getLogger(__name__).info("--streaming-locate-bounded: the locator bounds its runs as the selector does, --max-hold-seconds "
                                             "%g (a policy; --locator-max-hold-seconds sets it apart)", locator_max_hold_seconds)
        if (not args.streaming_locate and not args.streaming_locate_hold and not args.streaming_locate_bounded
                and (args.locate_seconds is not None or args.mask_gib is not None)):
            raise ValueError("--locate-seconds and --mask-gib set the window and the device bound of --streaming-locate and mean nothing "
                             "without it")
        ring = args.streaming_composite and args.interval_image == "quantile"
        if args.streaming_composite and not ring and args.interval_image not in frame_select.COMPOSITE_MODES:
            raise ValueError(f"--streaming-composite makes the picture of `--interval-image min`, `max` or `mean`, not of "
                             f"`--interval-image {args.interval_image}`")
        if args.ring_seconds is not None and not ring:
            raise ValueError("--ring-seconds sizes the ring of `--interval-image quantile --streaming-composite` and means nothing without them")
        composite_params = None
        if ring:
            if composite_fn is not None or stream_fn is not None:
                raise ValueError("--streaming-composite makes the pictures of `--interval-image quantile` with ring_fn; the "
                                 f"{'composite_fn' if composite_fn is not None else 'stream_fn'} given makes other pictures and would not be called")
            composite_params = {"streaming": True, "quantile": args.quantile, "samples": args.interval_samples,
                                "ring_seconds": 60.0 if args.ring_seconds is None else args.ring_seconds,
                                **({} if ring_fn is None else {"ring_fn": ring_fn})}
            frame_select.StreamingQuantile(**{k: v for k, v in composite_params.items() if k != "streaming"})       # a bad value is refused before any work
        elif args.interval_image == "quantile":
            composite_params = {"quantile": args.quantile, "samples": args.interval_samples, "rank_fn": composite_fn}
            frame_select.IntervalQuantile(**{"batch": args.batch, **composite_params})          # a bad value is refused before any work
        elif args.interval_image != "middle":
            composite_params = {"accumulate_fn": composite_fn}
        if args.streaming_composite and not ring:
            if composite_fn is not None:
                raise ValueError("--streaming-composite makes its pictures with stream_fn; the composite_fn given makes those of the "
                                 "compositor's own pass and would not be called")
            composite_params = {"streaming": True, **({} if stream_fn is None else {"stream_fn": stream_fn})}
        if args.deinterlace is None and (args.field_order != "auto" or args.deinterlace_thresh != 10):
            raise ValueError("--field-order and --deinterlace-thresh belong to --deinterlace adaptive | interpolate | match")
        source = ingest.open_source(args.video, fps=args.fps, size=size, layout=args.layout, matrix=args.matrix,
                                    wide=args.wide_yuv or args.deinterlace is not None, range=args.range, pix_fmt=args.pix_fmt,
                                    deinterlace=args.deinterlace, field_order=args.field_order, deinterlace_thresh=args.deinterlace_thresh,
                                    **match_arguments(args), **tone_arguments(args), **square_arguments(args))
        uploader = None
        if ocr is None:
            if args.weights_dir is not None:
                shim.config.weights_dir = args.weights_dir
            if args.allow_standin_weights:
                shim.config.allow_standin_weights = True
            shim.config.language, shim.config.mode = args.language, args.mode
            ocr, uploader = shim.OcrRecogniser(), staging.default_uploader()
        location = {}
        if args.streaming_locate or args.streaming_locate_hold or args.streaming_locate_bounded:
            flag, key = ("--streaming-locate-hold", "streaming_locate_hold") if args.streaming_locate_hold else ("--streaming-locate", "streaming_locate")
            fns = ({"cells_hold_masks_fn": cells_hold_masks_fn, "replay_hold_fn": replay_hold_fn} if args.streaming_locate_hold else
                   {"cells_masks_fn": cells_masks_fn, "replay_fn": replay_fn})
            if args.streaming_locate_bounded:
                flag, key = "--streaming-locate-bounded", "streaming_locate_bounded"
                fns = {"cells_bounded_masks_fn": cells_bounded_masks_fn, "replay_bounded_fn": replay_bounded_fn}
            locate_seconds, mask_gib = args.locate_seconds, 8.0 if args.mask_gib is None else args.mask_gib
            if locate_seconds is None and args.video == "-" and area == "auto" and mask_gib > 0:
                locate_seconds = default_locate_seconds(source, uploader is not None and hasattr(source, "raw_frames"), edge_thresh == "auto",
                                                        int(args.retain_gib * (1 << 30)), mask_gib)
                logging.getLogger(__name__).info("%s: the area is found on the first %d seconds (what fits --retain-gib "
                                                 "%g and --mask-gib %g, at most 300)", flag, int(locate_seconds), args.retain_gib, mask_gib)
            location = {key: True, "mask_gib": mask_gib, **({} if locate_seconds is None else {"locate_seconds": locate_seconds}),
                        **{k: v for k, v in fns.items() if v is not None}}
        ex = SubtitleExtractor(source, ocr, sub_area=area, mode=args.mode, language=args.language, extract_frequency=args.frequency,
                               batch=args.batch, uploader=uploader, frame_selector=args.selector, change_counter=counter,
                               retain_bytes=int(args.retain_gib * (1 << 30)), interval_image=args.interval_image,
                               composite_params=composite_params, interval_frame=args.interval_frame,
                               frame_params=None if focus_fn is None else {"focus_fn": focus_fn},
                               change_params=change_params or None,
                               area_params={**calibration, **location, **({} if cells_fn is None else {"cells_fn": cells_fn}),
                                            **({} if args.locator_automaton == "change" else {"automaton": args.locator_automaton}),
                                            **({} if locator_max_hold_seconds is None
                                               else {"max_hold_seconds": locator_max_hold_seconds})} or None)
        text = ex.run()
        if args.output is None:
            sys.stdout.write(text)
        else:
            with open(args.output, "w", encoding="utf-8") as fp:
                fp.write(text)
        if args.txt is not None:
            with open(args.txt, "w", encoding="utf-8") as fp:
                fp.write(SubtitleExtractor.srt2txt(text))
    except (OSError, ValueError) as e:
        print(f"extractor: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
