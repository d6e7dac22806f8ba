"""Accurate-mode ("precise") frame selection on top of the batched OCR engine — row a13 of SURVEY §8(a).

The reference decodes a frame, runs the detector on it, maybe runs the full OCR on it, and only then decodes the
next frame (backend/main.py:255-376): three dependent device round trips per frame at batch 1.  Frames are
independent, so here a CHUNK of frames goes through `detect_batch` in one launch sequence (and, optionally, the
frames that show an in-area box through `predict_batch`), after which the start/end-of-subtitle automaton is resolved
on the tiny results on the host.  The emitted OCR tasks are identical to the reference's queue, including its quirks
(tests/golden/frame_loop.json): a start is armed by the first in-area detection and re-armed after each end; the end
of a subtitle is the first frame whose in-area text has Levenshtein ratio <= threshold against the START frame, or the
first frame without an in-area box; cached OCR results older than 10 frames are evicted; when tasks are flushed the
cached result is looked up by the CURRENT frame number (not the queued one), so a task carries boxes/text only when
those coincide.

The interval side (subtitle-change selection and what follows it) shares its plumbing: `band_batches` reads the first frame, clips
the area and hands out batches of (full frame, the area's rows), keeping no frame behind; `staging.staged_batches` turns such batches
into stacked data, through an uploader's pinned memory and producer thread or with np.stack on the host; `_IntervalSelector` is the
one run / iter_run body of ChangeFrameSelector and HoldFrameSelector; and the Engine* callables keep their device state through
`engine.DeviceState`.  area_locator.AreaLocator and keyframes.scan stand on the same pieces.  A selector given a `focus_fn` (EngineFocus,
vse_frame_focus) also scores every frame in the same pass, and `sharpest_rep` picks an interval's frame by that score.  A selector given
a `compositor` (StreamingCompositor, vse_interval_stream) also makes each interval's min / max / mean picture in that pass, or
(StreamingQuantile, vse_interval_ring_rank) its quantile picture.  CalibratingChangeSelector (vse_frame_cells_counts) is the change
selector that chooses its edge threshold per clip in that same pass, and LocatingChangeSelector (vse_frame_cells_masks,
vse_frame_masks_replay) the one that finds its area there.  Any of them given a `key_fn` (ColourKey.apply, EngineKey: vse_colour_key)
builds its masks on the colour key of the band, for coloured subtitles, and leaves pictures and text to the frames as they are.
"""
from collections import deque
from contextlib import closing
from itertools import islice

from . import staging
from .engine import FRAME_HOLD_BOUNDED_MAX, INTERVAL_RANK_MAX, INTERVAL_RING_MAX_GROUPS, DeviceState
from .shim import get_coordinates


def similarity(a, b):
    """Levenshtein.ratio as used at backend/main.py:949: normalised InDel similarity, 1.0 for two empty strings."""
    if not a and not b:
        return 1.0
    la, lb = len(a), len(b)
    row = [0] * (lb + 1)
    for i in range(la):
        diag = 0
        ca = a[i]
        for j in range(lb):
            up = row[j + 1]
            row[j + 1] = diag + 1 if ca == b[j] else (up if up >= row[j] else row[j])
            diag = up
    return 2.0 * row[lb] / (la + lb)


def _inside(c, area):
    return area.xmin <= c[0] and c[1] <= area.xmax and area.ymin <= c[2] and c[3] <= area.ymax


class AccurateFrameSelector:
    # before the first subtitle / waiting for a start / waiting for the end / last frame consumed while tracking
    IDLE, ARMED, TRACKING, DONE = 0, 1, 2, 3

    def __init__(self, detect_batch, predict, sub_area, frame_count, threshold=80, chunk=64, predict_batch=None,
                 detect_stream=None, predict_with_dets=None):
        """detect_batch(list of frames) -> list of ndarray[N,4,2];  predict(frame) -> (boxes, [(text, score)]);
        predict_batch(list of frames) -> list of those (optional: prefetches every frame of a chunk that has an in-area
        box; the automaton asks for a subset of them).
        With an uploader (run): detect_stream(iterable of device batches) -> generator of detect_batch results keeps the
        detector of the next chunks in flight while a chunk is resolved, and predict_with_dets(device frames, their detections)
        -> list of predict results recognises the wanted frames from the boxes the detector already produced (the reference
        runs the same detector a second time inside predict: same frame, same boxes)."""
        self.detect_batch = detect_batch
        self.predict = predict
        self.predict_batch = predict_batch
        self.detect_stream = detect_stream
        self.predict_with_dets = predict_with_dets
        self.area = sub_area
        self.frame_count = frame_count
        self.threshold = threshold / 100.0
        self.chunk = chunk
        self.tasks = []
        self._state = self.IDLE
        self._no = 0
        self._start_no = 0
        self._pending = deque()
        self._ocr = {}                        # frame_no -> {"text","dt_box","rec_res"} (reference's result cache)
        self._prefetched = {}

    # ---- OCR results ------------------------------------------------------------------------------------------
    def _area_text(self, boxes, res):
        if self.area is None:
            return ""                         # the reference appends nothing when no area is set (main.py:914-921)
        return "".join(r[0] for r, c in zip(res, get_coordinates(boxes)) if _inside(c, self.area))

    def _ocr_of(self, no, frame):
        if no in self._prefetched:
            return self._prefetched.pop(no)
        return self.predict(frame.to_bgr() if hasattr(frame, "to_bgr") else frame)      # (an unconverted ingest.Yuv420Frame)

    def _remember(self, no, frame):
        boxes, res = self._ocr_of(no, frame)
        self._ocr[no] = {"text": self._area_text(boxes, res), "dt_box": boxes, "rec_res": res}

    def _same_as_start(self, frame):
        if self._start_no not in self._ocr:
            self._remember(self._start_no, None)      # cannot happen in the reference either unless evicted mid-run
        if self._no not in self._ocr:
            self._remember(self._no, frame)
        a, b = self._ocr[self._start_no]["text"], self._ocr[self._no]["text"]
        horizon = min(self._start_no, self._no) - 10
        for k in [k for k in self._ocr if k < horizon]:
            del self._ocr[k]
        return similarity(a, b) > self.threshold

    # ---- task queue ---------------------------------------------------------------------------------------------
    def _flush(self, keep):
        while len(self._pending) > keep:
            no = self._pending.popleft()
            hit = self._ocr.get(self._no)
            self.tasks.append((self.frame_count, no, hit["dt_box"], hit["rec_res"]) if hit else
                              (self.frame_count, no, None, None))

    # ---- automaton ------------------------------------------------------------------------------------------------
    def _has_subtitle(self, boxes):
        if self.area is None:
            return len(boxes) > 0
        return any(_inside(c, self.area) for c in get_coordinates(boxes.tolist()))

    def _step(self, frame, boxes):
        self._no += 1
        has = self._has_subtitle(boxes)
        if has and self._state == self.IDLE and self.area is not None:
            self._state = self.ARMED
        if has:
            if self._state == self.ARMED:
                self._start_no = self._no
                had = self._no in self._ocr
                b, r = self._ocr_of(self._no, frame)
                if not had:
                    self._ocr[self._no] = {"text": self._area_text(b, r), "dt_box": b, "rec_res": r}
                    self._pending.append(self._no)
                self._state = self.TRACKING
            if self._state == self.TRACKING and self._no == self.frame_count:
                self._state = self.DONE
                self._pending.append(self._no)
            if self._state == self.TRACKING and not self._same_as_start(frame):
                self._state = self.ARMED
                self._pending.append(self._no - 1)
        elif self._state == self.TRACKING:
            self._state = self.ARMED
            self._pending.append(self._no - 1)
        self._flush(1)

    def run(self, frames, uploader=None):
        """frames: iterable of frames in decode order.  Returns the task list
        [(frame_count, frame_no, dt_box | None, rec_res | None)] in the reference's queue order.
        uploader (staging.Uploader): chunks are staged through pinned memory by a producer thread; detect_batch and
        predict_batch then receive device uint8 tensors [n,H,W,3] (one upload per chunk serves both)."""
        def chunks():
            buf = []
            for f in frames:
                if buf and (len(buf) == self.chunk or getattr(buf[0][1], "shape", None) != getattr(f, "shape", None)):
                    yield buf
                    buf = []
                buf.append((None, f))
            if buf:
                yield buf
        if uploader is not None:
            from . import staging
            staged_chunks = staging.prefetch(chunks(), uploader)
            if self.detect_stream is not None:
                pending = deque()

                def tensors():
                    for items, staged in staged_chunks:
                        dev = staged.tensor()
                        pending.append((items, dev))
                        yield dev
                for dets in self.detect_stream(tensors()):
                    items, dev = pending.popleft()
                    self._consume([f for _, f in items], dev, dets)
            else:
                for items, staged in staged_chunks:
                    self._consume([f for _, f in items], staged.tensor())
        else:
            for items in chunks():
                self._consume([f for _, f in items])
        self._flush(0)
        return self.tasks

    def _consume(self, frames, dev=None, dets=None):
        if dets is None:
            dets = self.detect_batch(frames if dev is None else dev)
        if self.predict_batch is not None or (dev is not None and self.predict_with_dets is not None):
            want = [i for i, b in enumerate(dets) if self._has_subtitle(b)]
            if want:
                sub = [frames[i] for i in want] if dev is None else dev[want]
                if dev is not None and self.predict_with_dets is not None:
                    got = self.predict_with_dets(sub, [dets[i] for i in want])
                else:
                    got = self.predict_batch(sub)
                for i, r in zip(want, got):
                    self._prefetched[self._no + 1 + i] = r
        for f, b in zip(frames, dets):
            self._step(f, b)
        self._prefetched.clear()


# ---- subtitle-change selection (fast / auto mode with an area) ---------------------------------------------------------
def default_min_edges(area_h, area_w):
    """Edge pixels a frame needs to count as showing a subtitle: 0.05 % of the area's interior, at least 64."""
    return max(64, int(0.0005 * max(area_h - 2, 0) * max(area_w - 2, 0)))


class IntervalTracker:
    """The subtitle-change automaton, fed in pieces.  A frame is present when edges >= min_edges; a cut falls between t-1 and t when
    presence changes, or when both are present and (appeared + vanished) / (edges[t-1] + appeared) >= change_ratio (the union of the two
    masks); an interval is a maximal run of present frames without a cut inside, kept when it is at least min_frames long; rep is its
    middle frame.  feed(rows of (edges, appeared, vanished)) -> the intervals (start, end, rep), 1-based frame numbers, that those rows
    closed; flush() closes the open run at the last fed frame.  `fed`: rows seen; `open_start`: first frame of the open run, or None
    (a run still shorter than min_frames is open too)."""

    def __init__(self, min_edges, change_ratio=0.5, min_frames=2):
        self.min_edges, self.change_ratio, self.min_frames = min_edges, change_ratio, min_frames
        self.fed = 0
        self.open_start = None
        self._prev_edges = 0

    def _close(self, end, out):
        if self.open_start is not None and end - self.open_start + 1 >= self.min_frames:
            out.append((self.open_start, end, (self.open_start + end) // 2))

    def feed(self, rows):
        out = []
        for e, a, v in rows:
            e, a, v = int(e), int(a), int(v)
            self.fed += 1
            t = self.fed
            if e < self.min_edges:
                self._close(t - 1, out)
                self.open_start = None
            elif self.open_start is None:
                self.open_start = t
            else:
                union = self._prev_edges + a
                if union and (a + v) / union >= self.change_ratio:
                    self._close(t - 1, out)
                    self.open_start = t
            self._prev_edges = e
        return out

    def flush(self):
        out = []
        self._close(self.fed, out)
        self.open_start = None
        return out


def change_intervals(counts, min_edges, change_ratio=0.5, min_frames=2):
    """Per-frame (edges, appeared, vanished) of a whole clip -> [(start, end, rep)] with 1-based frame numbers: IntervalTracker fed
    the whole clip at once, then flushed."""
    tracker = IntervalTracker(min_edges, change_ratio, min_frames)
    return tracker.feed(counts) + tracker.flush()


def clip_area(sub_area, h, w):
    """sub_area (.ymin .ymax .xmin .xmax in frame pixels) clipped to an h x w frame -> (y0, y1, x0, x1); empty when y1 <= y0 or x1 <= x0."""
    return max(0, int(sub_area.ymin)), min(h, int(sub_area.ymax)), max(0, int(sub_area.xmin)), min(w, int(sub_area.xmax))


class band_batches:
    """The frames of a clip as batches of their band: iterating yields lists of (full frame, frame[y0:y1]) of at most `batch` frames,
    in decode order, and keeps no reference to a frame once the list holding it has been handed out (a caller that drops a frame it
    was handed frees it).  `region` (.ymin .ymax .xmin .xmax, or None for the whole frame) is clipped to the first frame, which is read
    at once: `geometry` = (y0, y1, x0, x1) in frame pixels, `frame_hw`, and `area`, the same rectangle in the band's own pixels
    (0, y1 - y0, x0, x1), are known before the first batch; all three are None when there is no frame.  ValueError in the name of
    `who` when less than min_size x min_size pixels remain."""

    def __init__(self, frames, region, batch, who, min_size=3):
        self._it, self._batch = iter(frames), batch
        self._head = list(islice(self._it, 1))
        self.geometry = self.frame_hw = self.area = None
        if self._head:
            h, w = self._head[0].shape[:2]
            y0, y1, x0, x1 = (0, h, 0, w) if region is None else clip_area(region, h, w)
            if y1 - y0 < min_size or x1 - x0 < min_size:
                raise ValueError(f"{who}: subtitle area {region} leaves less than {min_size} x {min_size} pixels of a {h} x {w} frame")
            self.geometry, self.frame_hw, self.area = (y0, y1, x0, x1), (h, w), (0, y1 - y0, x0, x1)

    def _take(self):
        frames, self._head = self._head, []
        frames.extend(islice(self._it, self._batch - len(frames)))
        return [(f, f[self.geometry[0]:self.geometry[1]]) for f in frames]

    def __iter__(self):
        return iter(self._take, [])           # (no generator frame that would hold on to the list it yielded last)


# ---- colour key (coloured subtitles over a background with many luma edges) ----------------------------------------------------------
COLOUR_NAMES = {"white": (255, 255, 255), "yellow": (0, 255, 255), "cyan": (255, 255, 0), "green": (0, 255, 0), "black": (0, 0, 0)}      # B, G, R


def parse_colour(colour):
    """The one place a text colour is read: (B, G, R) of three integers 0..255, "#RRGGBB" / "RRGGBB", or a name of COLOUR_NAMES ->
    (B, G, R).  ValueError for anything else."""
    if isinstance(colour, str):
        text = colour.strip().lower()
        if text in COLOUR_NAMES:
            return COLOUR_NAMES[text]
        digits = text[1:] if text.startswith("#") else text
        if len(digits) == 6 and all(c in "0123456789abcdef" for c in digits):
            return int(digits[4:6], 16), int(digits[2:4], 16), int(digits[0:2], 16)
        raise ValueError(f"text colour {colour!r} is not RRGGBB, #RRGGBB or one of {', '.join(sorted(COLOUR_NAMES))}")
    try:
        bgr = tuple(int(v) for v in colour)
        exact = all(int(v) == v for v in colour)
    except (TypeError, ValueError):
        bgr, exact = (), False
    if len(bgr) != 3 or not exact or not all(0 <= v <= 255 for v in bgr):
        raise ValueError(f"text colour {colour!r} is not (B, G, R) of three integers 0..255")
    return bgr


class ColourKey:
    """The selectors' second cue beside the luma gradient: how near a pixel is to the subtitle's fill colour.  With
    d = max(|B - b|, |G - g|, |R - r|) against colour = (b, g, r), a pixel becomes (K, K, K), K = max(0, 255 - ((d * slope) >> 8)) and
    slope = ceil(255 * 256 / tol): K is 255 on the colour itself, falls with d and is 0 from d = tol on.  The selectors' luma of (K, K,
    K) is K (29 + 150 + 77 = 256), so a selector, locator or calibration given a key_fn runs unchanged on K's gradient: a background of
    other colours is flat there however many luma edges it has.  colour: see parse_colour; tol: 1..255.  tol=48 is a guess, checked on
    the synthetic clip only (no real clips).  Known limit: a background whose colours saturate to the corners of the colour cube passes
    the key where it meets the text's corner (3 to 10 % of random cells at amplitude 250), and the keyed selector then fails as well.
    `bgr`, `slope`: what vse_colour_key takes.  apply(frames, area) is the key_fn in numpy, the same integers as the device's."""

    def __init__(self, colour, tol=48):
        self.bgr = parse_colour(colour)
        if isinstance(tol, bool) or int(tol) != tol or not 1 <= int(tol) <= 255:
            raise ValueError(f"colour tolerance {tol!r} is not an integer 1..255")
        self.tol = int(tol)
        self.slope = -(-255 * 256 // self.tol)

    def apply(self, frames, area):
        """frames uint8 [n,h,w,3], area (y0, y1, x0, x1) in their pixels -> uint8 of the same shape: the key inside the area, 0 elsewhere."""
        import numpy as np
        frames = np.asarray(frames)
        y0, y1, x0, x1 = area
        out = np.zeros(frames.shape, np.uint8)
        d = np.abs(frames[:, y0:y1, x0:x1].astype(np.int32) - np.asarray(self.bgr, np.int32)).max(-1)
        out[:, y0:y1, x0:x1] = np.maximum(0, 255 - ((d * self.slope) >> 8))[..., None]
        return out


class EngineKey(DeviceState):
    """key_fn of the selectors and the locator on the GPU (Context.colour_key): (frames [n,h,w,3] uint8, area) -> the keyed frames, a
    device tensor of the same shape, launched on the current stream, so in front of the count that reads it.  One output tensor is kept
    per shape and written again by the next call with that shape: the result is for the kernels launched before that call.
    ctx None: the shim's device, asked for at the first call.  key: a ColourKey (default: white at its default tolerance)."""

    def __init__(self, ctx, key=None):
        super().__init__(ctx)
        self.key = ColourKey("white") if key is None else key
        self._outs = {}

    def __call__(self, frames, area):
        if self.ctx is None:
            from . import shim
            self.ctx = shim._context()
        frames = self._device(frames)
        out = self._outs.get(tuple(frames.shape))
        if out is None:
            out = self._outs[tuple(frames.shape)] = self.ctx.torch.empty(tuple(frames.shape), dtype=self.ctx.torch.uint8, device=self.ctx.tdev)
        return self.ctx.colour_key(frames, area, self.key, out=out)


class EngineCounter(DeviceState):
    """count_fn of ChangeFrameSelector on the GPU (Context.frame_change): keeps the device state of the last area between calls."""

    def __call__(self, frames, area, edge_thresh, reset):
        y0, y1, x0, x1 = area
        reset = self._fresh((y1 - y0, x1 - x0), self.ctx.frame_change_state) or reset
        return self.ctx.frame_change(self._device(frames), area, edge_thresh, self._state, reset)


class EngineFocus(DeviceState):
    """focus_fn of the selectors on the GPU (Context.frame_focus): keeps the device state of the last area between calls."""

    def __call__(self, frames, area, edge_thresh, reset):
        y0, y1, x0, x1 = area
        reset = self._fresh((y1 - y0, x1 - x0), self.ctx.frame_change_state) or reset
        return self.ctx.frame_focus(self._device(frames), area, edge_thresh, self._state, reset)


class _IntervalSelector:
    """The body ChangeFrameSelector and HoldFrameSelector share: frames -> band_batches -> staging.staged_batches -> count_fn ->
    IntervalTracker.  A selector says which engine callable is its default count_fn, what the tracker's min_frames is (`_min_frames`),
    how count_fn is called per batch (`_count`) and what follows the last batch (`_flush`).
    focus_fn(frames [n,h,w,3] uint8, area, edge_thresh, reset) -> [n,2] kept, focus per frame (vse_frame_focus; it carries the last
    frame's mask to the next call): when given, it is called once per batch on the same staged data as count_fn, with reset on the
    first batch, and its rows are appended to `focus`, int64 [frames fed, 2], readable while iterating.  Focus rows belong to the
    frames fed: they do not trail like the hold selector's counts.  None: no call, and `focus` is not touched.
    compositor (StreamingCompositor or StreamingQuantile): when given, begin(fps, lag) is called before the first batch, with `lag` the number of frames by
    which the rows trail (`_lag`), then compositor(data, area, n, tracker, closed) once per staged batch, after the tracker has been
    fed and while the batch is still resident, and once more after the flush with n = 0 and the last closings.  None: nothing changes.
    key_fn(frames [n,h,w,3] uint8, area) -> frames of the same shape (ColourKey.apply, EngineKey): when given, it is called once per
    staged batch (or once per slice a body cuts from a batch), with the area the mask is about to be built on, and its result goes to
    whatever builds a mask (count_fn, focus_fn, cells_fn); the compositor and the yielded items keep the staged band and the frames.
    None: count_fn, focus_fn and cells_fn receive the staged data itself."""

    def __init__(self, count_fn=None, edge_thresh=128, change_ratio=0.5, min_edges=None, min_frames=2, batch=64, focus_fn=None,
                 compositor=None, key_fn=None):
        self.count_fn, self.focus_fn, self.compositor, self.key_fn = count_fn, focus_fn, compositor, key_fn
        self.edge_thresh, self.change_ratio, self.min_edges, self.min_frames = edge_thresh, change_ratio, min_edges, min_frames
        self.batch = batch
        self.counts = None
        self.intervals = None

    def run(self, frames, sub_area, fps=None, uploader=None):
        """frames: iterable of uint8 BGR frames in decode order; sub_area: .ymin .ymax .xmin .xmax in frame pixels (clipped to the
        frame); fps: the clip's frame rate (the hold selector's hold_seconds; the change selector ignores it) -> [(start, end, rep)].
        Only the area's rows are staged (band_batches), through `uploader` when there is one (staging.staged_batches)."""
        for _ in self.iter_run(frames, sub_area, fps, uploader):
            pass
        return self.intervals

    def iter_run(self, frames, sub_area, fps=None, uploader=None):
        """run() as a generator: per staged batch (items, the intervals its rows closed), items = [(full frame, its area rows)] in
        decode order, so a caller that may need a frame again receives it with the batch itself; after the last batch one more
        ([], what the flushed rows and the end of the clip closed).  `tracker` (IntervalTracker) is in step with what has been
        yielded: `tracker.fed` is the last frame whose row has been seen (the hold selector's rows trail its frames by hold - 1, or with max_hold_*
        by max_hold, until the flush, and the frames behind it are still the caller's to keep); `intervals` grows as they close, `counts` is set when
        the generator is exhausted."""
        import numpy as np
        if self.count_fn is None:
            from . import shim
            self.count_fn = self.engine_count_fn(shim._context())
        min_frames = self._min_frames(fps)
        self.counts, self.intervals, self.tracker = np.zeros((0, 3), np.int32), [], None
        if self.focus_fn is not None:
            self.focus = np.zeros((0, 2), np.int64)
        bands = band_batches(frames, sub_area, self.batch, type(self).__name__)
        if bands.area is None:
            return
        min_edges = default_min_edges(bands.area[1], bands.area[3] - bands.area[2]) if self.min_edges is None else self.min_edges
        self.tracker = IntervalTracker(min_edges, self.change_ratio, min_frames)
        if self.compositor is not None:
            self.compositor.begin(fps, self._lag())

        def feed(c):
            out.append(np.asarray(c.cpu() if hasattr(c, "cpu") else c, np.int32).reshape(-1, 3))
            closed = self.tracker.feed(out[-1])
            self.intervals += closed
            return closed

        out, fed, data = [], 0, None
        room = np.zeros((0, 2), np.int64)
        with closing(staging.staged_batches(bands, uploader)) as staged:
            for items, data in staged:
                keyed = data if self.key_fn is None else self.key_fn(data, bands.area)
                counts = self._count(keyed, bands.area, fed)
                if self.focus_fn is not None:             # (launched before the counts are read back: one wait for both)
                    rows = self.focus_fn(keyed, bands.area, self.edge_thresh, fed == 0)
                closed = feed(counts)
                if self.focus_fn is not None:
                    rows = np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows, np.int64).reshape(-1, 2)
                    if fed + len(rows) > len(room):           # `focus` is a view of `room`, which doubles when it is full
                        room = np.concatenate([room[:fed], np.zeros((max(len(room), len(rows), 1024), 2), np.int64)])
                    room[fed:fed + len(rows)] = rows
                    self.focus = room[:fed + len(rows)]
                if self.compositor is not None:
                    self.compositor(data, bands.area, len(items), self.tracker, closed)
                fed += len(items)
                yield items, closed
        closed = feed(self._flush(data, bands.area, fed))         # (no frames: nothing to key)
        self.counts = np.concatenate(out)
        last = self.tracker.flush()
        self.intervals += last
        if self.compositor is not None:
            self.compositor(data[:0], bands.area, 0, self.tracker, closed + last)
        yield [], closed + last


class ChangeFrameSelector(_IntervalSelector):
    """The role of VideoSubFinder in fast / auto mode with a subtitle area (backend/main.py:137-147, 378-505): look at EVERY frame
    of the area and report where each subtitle starts and stops, so that one frame per subtitle goes to OCR and the SRT takes
    its times from the intervals (srt.generate_subtitle_file_intervals).  VideoSubFinder is a closed binary; this is not its
    algorithm but the same role: per frame the device counts the area's luma edge pixels and how many of them appeared or
    vanished against the frame before (vse_frame_change), and change_intervals turns those integers into intervals.
    The defaults lean towards cutting: an extra cut costs one OCR call and the duplicate removal merges it again, a missed
    change loses a subtitle.  run / iter_run: _IntervalSelector's.

    count_fn(frames [n,h,w,3] uint8, area (y0, y1, x0, x1) in their pixels, edge_thresh, reset) -> [n,3] counts; it carries the
    last frame's mask to the next call (reset on the first batch of a clip).  Default: EngineCounter on the shim's device."""
    engine_count_fn = EngineCounter

    def _min_frames(self, fps):
        return self.min_frames

    def _lag(self):
        return 0

    def _count(self, data, area, fed):
        return self.count_fn(data, area, self.edge_thresh, fed == 0)

    def _flush(self, data, area, fed):
        return ()                         # every row came with its frame


# ---- the change selector that chooses its own edge threshold while the frames go by ------------------------------------------------
class EngineCellsCounts(DeviceState):
    """cells_fn of CalibratingChangeSelector on the GPU (Context.frame_cells_counts), beside area_locator.EngineCells: keeps the device
    state of the last region and threshold count between calls; (frames | None, area, engine.CellParams, reset, flush, thresholds) ->
    (totals [nt,gy,gx,4], counts [n,nt,3]), frames None with flush closing the open runs.  `export(area, q, counter)` makes slice q of
    that state the state of an EngineCounter (Context.frame_cells_export_state), whose next call then continues the clip."""

    def __call__(self, frames, area, params, reset, flush, thresholds):
        t = self.ctx.torch
        y0, y1, x0, x1 = area
        frames = t.empty((0, y1, x1, 3), dtype=t.uint8, device=self.ctx.tdev) if frames is None else self._device(frames)
        reset = self._fresh((y1 - y0, x1 - x0, len(thresholds)), self.ctx.frame_cells_multi_state) or reset
        return self.ctx.frame_cells_counts(frames, area, thresholds, params, self._state, reset, flush)

    def export(self, area, q, counter):
        y0, y1, x0, x1 = area
        if self._key is None or self._key[:2] != (y1 - y0, x1 - x0):
            raise ValueError(f"EngineCellsCounts: no state of a {y1 - y0} x {x1 - x0} region to export")
        counter._fresh((y1 - y0, x1 - x0), self.ctx.frame_change_state)
        self.ctx.frame_cells_export_state(self._state, y1 - y0, x1 - x0, q, out=counter._state)


class CalibratingChangeSelector(_IntervalSelector):
    """ChangeFrameSelector with change_params' edge_thresh="auto" and a given area, in ONE pass over the frames: what
    area_locator.AreaLocator(edge_thresh="auto", search_area=the area) decides in a pass of its own is decided here while the selector
    runs, so a pipe, which cannot be read twice, gets a calibrated threshold, and a file is decoded once less.  The calibration's cells
    tile the interior of the selector's area and their mask is the selector's, so one kernel (vse_frame_cells_counts) hands back both
    the calibration's totals and, per frame and candidate threshold, exactly the counts vse_frame_change would write at that threshold.
    Up to the decision the batches go through cells_fn, one IntervalTracker per threshold is fed its row of the counts (each built as
    ChangeFrameSelector builds its one: default_min_edges, change_ratio, min_frames), and no interval is yielded.  The decision falls
    after the row of frame `window` (None: after the clip's last frame; a clip that ends sooner decides at its end; a batch that
    straddles it is split there): the cells are flushed, the totals read once, area_locator.pick_edge_thresh chooses with frames_scanned
    = the frames of the window, so the choice is AreaLocator(search_area=the area, probe=(1, window))'s; when no threshold scores, the
    locator's warning is given and 128 is used (which must therefore be among the thresholds).  export_fn then hands the chosen
    threshold's last mask to count_fn, `tracker` becomes that threshold's tracker, the intervals it has closed so far are yielded in
    order with that batch, and from there on this is a plain ChangeFrameSelector at the chosen threshold.  The intervals and counts are
    those of ChangeFrameSelector(edge_thresh=the choice) over the whole clip.  How the choice or a window behaves on real footage is not
    measured here (no real clips).

    cells_fn(frames [n,h,w,3] uint8 | None, area, engine.CellParams, reset, flush, thresholds) -> (totals [nt,gy,gx,4], counts [n,nt,3]);
    default EngineCellsCounts on the shim's device.  export_fn(area, q, count_fn): count_fn's next call continues from threshold q's
    last mask; default cells_fn.export.  count_fn: ChangeFrameSelector's; it is never called with reset.  locator_params: AreaLocator's
    keyword arguments (thresholds, min_edges, change_ratio, min_seconds, max_seconds, plateau_frac, static_frac), the cells' rule.
    Before the decision `tracker` is None, `trackers` are the candidates' and `pending[q]` the intervals candidate q has closed; after
    it `edge_thresh`, `scores`, `totals`, `frames_scanned` and `chosen` (the index) say what was decided and on what."""

    def __init__(self, count_fn=None, cells_fn=None, export_fn=None, window=None, locator_params=None, change_ratio=0.5, min_edges=None,
                 min_frames=2, batch=64, key_fn=None):
        super().__init__(count_fn, None, change_ratio, min_edges, min_frames, batch, key_fn=key_fn)
        from . import area_locator
        if window is not None and int(window) < 1:
            raise ValueError(f"CalibratingChangeSelector: window must be at least 1 frame or None, not {window}")
        self.window = None if window is None else int(window)
        self.cells_fn, self.export_fn = cells_fn, export_fn
        self.locator = area_locator.AreaLocator(**{**(locator_params or {}), "edge_thresh": "auto"})
        if self.locator.automaton != "change":
            raise ValueError("CalibratingChangeSelector: the calibration in the selector's pass counts with the change automaton, not "
                             f"automaton={self.locator.automaton!r}")
        if area_locator.DEFAULT_EDGE_THRESH not in self.locator.thresholds:
            raise ValueError(f"CalibratingChangeSelector: thresholds {self.locator.thresholds} must contain {area_locator.DEFAULT_EDGE_THRESH}, "
                             "the threshold used when none scores")
        self.trackers, self.pending, self.tracker, self.decided = [], [], None, False
        self.scores = self.totals = self.chosen = None
        self.frames_scanned = 0

    def iter_run(self, frames, sub_area, fps=None, uploader=None):
        """ChangeFrameSelector.iter_run; up to the decision every batch is yielded with no closed interval and `tracker` is None."""
        import logging

        import numpy as np
        from . import area_locator
        if self.count_fn is None or self.cells_fn is None:
            from . import shim
            self.count_fn = EngineCounter(shim._context()) if self.count_fn is None else self.count_fn
            self.cells_fn = EngineCellsCounts(shim._context()) if self.cells_fn is None else self.cells_fn
        export = self.cells_fn.export if self.export_fn is None else self.export_fn
        loc, ths = self.locator, self.locator.thresholds
        self.counts, self.intervals, self.tracker, self.decided = np.zeros((0, 3), np.int32), [], None, False
        self.trackers, self.pending = [], []
        self.edge_thresh = self.scores = self.totals = self.chosen = None
        self.frames_scanned = 0
        bands = band_batches(frames, sub_area, self.batch, type(self).__name__)
        if bands.area is None:
            return
        area, params = bands.area, loc.params(fps)
        min_edges = default_min_edges(area[1], area[3] - area[2]) if self.min_edges is None else self.min_edges
        self.trackers = [IntervalTracker(min_edges, self.change_ratio, self.min_frames) for _ in ths]
        self.pending = [[] for _ in ths]
        seen, rows = [], []                   # the counts of the window [n,nt,3] and of the frames behind it [n,3], batch by batch

        def host(c, shape):
            return np.asarray(c.cpu() if hasattr(c, "cpu") else c, np.int32).reshape(shape)

        def decide(scanned):
            totals, _none = self.cells_fn(None, area, params, False, True, ths)
            self.totals, self.frames_scanned = host(totals, tuple(totals.shape)), scanned
            static_frac = loc.locate_kwargs.get("static_frac", 0.95)
            self.scores = area_locator.edge_thresh_scores(self.totals, scanned, static_frac)
            k = area_locator.pick_edge_thresh(self.totals, ths, scanned, static_frac, loc.plateau_frac)
            if k is None:
                logging.getLogger(area_locator.__name__).warning(
                    "edge_thresh='auto': none of the thresholds %s scores with the %s automaton in %d frames; falling back to %d", ths,
                    loc.describe_automaton(), scanned, area_locator.DEFAULT_EDGE_THRESH)
                k = ths.index(area_locator.DEFAULT_EDGE_THRESH)
            self.chosen, self.edge_thresh = k, ths[k]
            export(area, k, self.count_fn)
            self.tracker, self.intervals, self.decided = self.trackers[k], list(self.pending[k]), True
            return list(self.pending[k])

        fed = 0
        with closing(staging.staged_batches(bands, uploader)) as staged:
            for items, data in staged:
                n, head, closed = len(items), 0, []
                if not self.decided:
                    head = n if self.window is None else min(n, self.window - fed)
                    part = data if head == n else data[:head]
                    _totals, c = self.cells_fn(part if self.key_fn is None else self.key_fn(part, area), area, params, fed == 0, False, ths)
                    seen.append(host(c, (-1, len(ths), 3)))
                    for q, tracker in enumerate(self.trackers):
                        self.pending[q] += tracker.feed(seen[-1][:, q])
                    if self.window is not None and fed + head >= self.window:
                        closed = decide(fed + head)
                if self.decided and head < n:
                    part = data[head:] if head else data
                    rows.append(host(self.count_fn(part if self.key_fn is None else self.key_fn(part, area), area, self.edge_thresh, False),
                                     (-1, 3)))
                    got = self.tracker.feed(rows[-1])
                    self.intervals += got
                    closed = closed + got
                fed += n
                yield items, closed
        closed = [] if self.decided else decide(fed)
        last = self.tracker.flush()
        self.intervals += last
        self.counts = np.concatenate([c[:, self.chosen] for c in seen] + rows)
        yield [], closed + last


# ---- the change selector that finds its own area while the frames go by -------------------------------------------------------------
class EngineCellsMasks(DeviceState):
    """cells_fn of LocatingChangeSelector on the GPU (Context.frame_cells_masks), beside area_locator.EngineCells: keeps the device state
    and the mask buffer of the last region, threshold count and `cap`, and `fed`, the frames fed since the last reset, which is the slot
    the next frame takes; (frames | None, area, engine.CellParams, reset, flush, thresholds, cap) -> totals [nt,gy,gx,4], frames None with
    flush closing the open runs.  `replay(area, q, rect, counter)` counts the slots 0 .. fed - 1 at threshold index q on `rect` (y0, y1,
    x0, x1 in the region's pixels) at once (Context.frame_masks_replay) -> counts [fed,3], and makes the result state the state of an
    EngineCounter, whose next call then continues the clip on that rectangle."""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.fed, self._masks = 0, None

    def __call__(self, frames, area, params, reset, flush, thresholds, cap):
        t = self.ctx.torch
        y0, y1, x0, x1 = area
        frames = t.empty((0, y1, x1, 3), dtype=t.uint8, device=self.ctx.tdev) if frames is None else self._device(frames)
        if self._fresh((y1 - y0, x1 - x0, len(thresholds), int(cap)), lambda h, w, nt, _cap: self.ctx.frame_cells_multi_state(h, w, nt)):
            self._masks, reset = self.ctx.frame_masks_buffer(y1 - y0, x1 - x0, len(thresholds), cap), True
        if reset:
            self.fed = 0
        totals = self.ctx.frame_cells_masks(frames, area, thresholds, params, self._state, self._masks, self.fed, reset, flush)
        self.fed += len(frames)
        return totals

    def replay(self, area, q, rect, counter):
        y0, y1, x0, x1 = area
        if self._key is None or self._key[:2] != (y1 - y0, x1 - x0) or not self.fed:
            raise ValueError(f"EngineCellsMasks: no masks of a {y1 - y0} x {x1 - x0} region to replay")
        ry0, ry1, rx0, rx1 = rect
        counter._fresh((ry1 - ry0, rx1 - rx0), self.ctx.frame_change_state)
        counts, _state = self.ctx.frame_masks_replay(self._masks, q, 0, self.fed, rect, True, out=counter._state)
        return counts


class LocatingChangeSelector(_IntervalSelector):
    """ChangeFrameSelector with sub_area="auto", in ONE pass over the frames: what area_locator.AreaLocator(probe=(1, window)) decides in
    a pass of its own is decided here while the selector runs, so a pipe, which cannot be read twice, gets its area, and a file is
    decoded once less.  The located rectangle's interior lies a row and a column off the locator's cell grid, so no sum of the cells'
    counts gives the selector's counts on it; but a pixel's edge mask does not depend on the area, so up to the decision the batches
    (whole frames) go through cells_fn, which keeps every frame's mask words beside the locator's totals (vse_frame_cells_masks), and
    nothing is yielded as closed.  The decision falls after frame `window` (a clip that ends sooner decides at its end): the cells are
    flushed, the totals read once, with edge_thresh="auto" area_locator.pick_edge_thresh chooses with frames_scanned = the frames of the
    window, and area_locator.locate_area decides on that threshold's totals, so area, threshold, `scores`, `totals` and `frames_scanned`
    are AreaLocator(probe=(1, window)).run(...)'s, its warning and no area when no threshold scores included.  With an area, replay_fn
    counts the kept masks of frames 1 .. window on it (vse_frame_masks_replay: integer for integer vse_frame_change's counts) and hands
    the last mask to count_fn; one IntervalTracker, built as ChangeFrameSelector builds its own, is fed them, the intervals it has
    closed are yielded with the deciding batch, and the rest of the frames run over the area's rows through count_fn like a plain
    ChangeFrameSelector: the intervals and counts are ChangeFrameSelector(edge_thresh=the choice)'s over the whole clip on the located
    area.  Without an area, `area` stays None, `decided` is True and the generator ends, having consumed min(window, clip) frames
    exactly: the first `window` frames are a staged run of their own, so neither this nor an uploader's producer thread reads beyond
    them before the area is known.  Whether a window of some length finds the band of a real film is not measured here (no real clips).

    cells_fn(frames [n,h,w,3] uint8 | None, area, engine.CellParams, reset, flush, thresholds, cap) -> totals [nt,gy,gx,4]; default
    EngineCellsMasks on the shim's device.  replay_fn(area, q, rect, count_fn) -> counts [frames fed,3] at threshold index q on rect (y0,
    y1, x0, x1 in the region's pixels), after which count_fn's next call continues from the last mask; default cells_fn.replay.
    count_fn: ChangeFrameSelector's; it is never called with reset.  window: frames, required.  edge_thresh: an integer or "auto".
    locator_params: AreaLocator's keyword arguments (thresholds, min_edges, change_ratio, min_seconds, max_seconds, plateau_frac and
    locate_area's); automaton="hold", max_hold_*, search_area and probe are refused.  Before the decision `tracker` is None."""

    def __init__(self, count_fn=None, cells_fn=None, replay_fn=None, window=None, locator_params=None, edge_thresh=128, change_ratio=0.5,
                 min_edges=None, min_frames=2, batch=64, key_fn=None):
        super().__init__(count_fn, edge_thresh, change_ratio, min_edges, min_frames, batch, key_fn=key_fn)
        from . import area_locator
        if window is None or int(window) < 1:
            raise ValueError(f"LocatingChangeSelector: window must be at least 1 frame, not {window}")
        self.window, self.cells_fn, self.replay_fn = int(window), cells_fn, replay_fn
        params = dict(locator_params or {})
        refused = [f"automaton={params['automaton']!r}"] if params.get("automaton", "change") != "change" else []
        refused += sorted(set(params) & {"max_hold_seconds", "max_hold_frames", "search_area", "probe"})
        if refused:
            raise ValueError("LocatingChangeSelector: the locator in the selector's pass counts whole frames with the change automaton and "
                             f"`window` says how many decide; it does not take {', '.join(refused)}")
        self.locator = area_locator.AreaLocator(**{**params, "edge_thresh": edge_thresh})
        self.area, self.tracker, self.decided = None, None, False
        self.scores = self.totals = None
        self.frames_scanned = 0

    def iter_run(self, frames, sub_area=None, fps=None, uploader=None):
        """ChangeFrameSelector.iter_run over whole frames (sub_area must be None: this finds it); up to the decision every batch is
        yielded with no closed interval and `tracker` is None."""
        import logging

        import numpy as np
        from . import area_locator
        if sub_area is not None:
            raise ValueError(f"LocatingChangeSelector: it finds the area itself and takes none, not {sub_area}")
        if self.count_fn is None or self.cells_fn is None:
            from . import shim
            self.count_fn = EngineCounter(shim._context()) if self.count_fn is None else self.count_fn
            self.cells_fn = EngineCellsMasks(shim._context()) if self.cells_fn is None else self.cells_fn
        replay = self.cells_fn.replay if self.replay_fn is None else self.replay_fn
        loc = self.locator
        ths = loc.thresholds if loc.auto else (loc.edge_thresh,)
        self.counts, self.intervals, self.tracker, self.decided, self.area = np.zeros((0, 3), np.int32), [], None, False, None
        self.edge_thresh = None if loc.auto else loc.edge_thresh
        self.scores = self.totals = None
        self.frames_scanned = 0
        it = iter(frames)
        bands = band_batches(islice(it, self.window), None, self.batch, type(self).__name__)
        if bands.area is None:
            return
        region, params = bands.area, loc.params(fps)
        rows = []                             # the counts of the window [n,3], then of the frames behind it, batch by batch

        def host(c, shape):
            return np.asarray(c.cpu() if hasattr(c, "cpu") else c, np.int32).reshape(shape)

        def decide(scanned):
            totals = self.cells_fn(None, region, params, False, True, ths, self.window)
            self.totals, self.frames_scanned, self.decided = host(totals, tuple(totals.shape)), scanned, True
            q, chosen = 0, self.totals[0]
            if loc.auto:
                static_frac = loc.locate_kwargs.get("static_frac", 0.95)
                self.scores = area_locator.edge_thresh_scores(self.totals, scanned, static_frac)
                q = area_locator.pick_edge_thresh(self.totals, ths, scanned, static_frac, loc.plateau_frac)
                if q is None:
                    logging.getLogger(area_locator.__name__).warning(
                        "edge_thresh='auto': none of the thresholds %s scores with the %s automaton in %d frames; falling back to %d", ths,
                        loc.describe_automaton(), scanned, area_locator.DEFAULT_EDGE_THRESH)
                    return []
                self.edge_thresh, chosen = ths[q], self.totals[q]
            else:
                self.totals = chosen          # (AreaLocator's totals at one threshold are [gy,gx,4])
            self.area = area_locator.locate_area(chosen, scanned, bands.geometry, bands.frame_hw, **loc.locate_kwargs)
            if self.area is None:
                return []
            y0, y1, x0, x1 = clip_area(self.area, *bands.frame_hw)
            rows.append(host(replay(region, q, (y0 - bands.geometry[0], y1 - bands.geometry[0], x0 - region[2], x1 - region[2]),
                                    self.count_fn), (-1, 3)))
            min_edges = default_min_edges(y1 - y0, x1 - x0) if self.min_edges is None else self.min_edges
            self.tracker = IntervalTracker(min_edges, self.change_ratio, self.min_frames)
            self.intervals = self.tracker.feed(rows[-1])
            return list(self.intervals)

        fed, closed = 0, []
        with closing(staging.staged_batches(bands, uploader)) as staged:
            for items, data in staged:
                self.cells_fn(data if self.key_fn is None else self.key_fn(data, region), region, params, fed == 0, False, ths, self.window)
                fed += len(items)
                if fed >= self.window:
                    closed = decide(fed)
                yield items, closed
        if not self.decided:                  # the clip ended inside the window
            closed = decide(fed)
        elif self.area is not None:
            closed = []                       # (they went out with the deciding batch)
            rest = band_batches(it, self.area, self.batch, type(self).__name__)
            if rest.area is not None:
                with closing(staging.staged_batches(rest, uploader)) as staged:
                    for items, data in staged:
                        keyed = data if self.key_fn is None else self.key_fn(data, rest.area)        # (over the located rectangle)
                        rows.append(host(self.count_fn(keyed, rest.area, self.edge_thresh, False), (-1, 3)))
                        got = self.tracker.feed(rows[-1])
                        self.intervals += got
                        yield items, got
        if self.area is None:
            return
        last = self.tracker.flush()
        self.intervals += last
        self.counts = np.concatenate(rows)
        yield [], closed + last


# ---- held-edge selection (the change selector for footage whose background moves) ------------------------------------------
def hold_intervals(counts, min_edges, hold, change_ratio=0.5, min_frames=2):
    """change_intervals on the held-edge counts of a whole clip (vse_frame_hold): the same automaton; an interval shorter than `hold`
    frames cannot hold an edge for `hold` frames, so it is not kept either."""
    return change_intervals(counts, min_edges, change_ratio, max(min_frames, hold))


class EngineHoldCounter(DeviceState):
    """count_fn of HoldFrameSelector on the GPU (Context.frame_hold): keeps the device state of the last area and `hold`, and the
    number of frames of the clip fed so far, between calls."""
    fed = 0

    def __call__(self, frames, area, edge_thresh, hold, fed, flush):
        y0, y1, x0, x1 = area
        key = (y1 - y0, x1 - x0, hold)
        if fed and self._key != key:
            raise ValueError(f"EngineHoldCounter: the area or hold changed to {key} after {fed} frames of a clip")
        self._fresh(key, self.ctx.frame_hold_state)
        if fed and fed != self.fed:
            raise ValueError(f"EngineHoldCounter: fed {fed}, but {self.fed} frames of this clip went to earlier calls")
        self.fed = fed + len(frames)
        return self.ctx.frame_hold(self._device(frames), area, edge_thresh, hold, self._state, fed, flush)


class EngineBoundedHoldCounter(DeviceState):
    """count_fn of HoldFrameSelector with max_hold_* on the GPU (Context.frame_hold_bounded): keeps the device state of the last area and
    `max_hold`, and the number of frames of the clip fed so far, between calls."""
    fed = 0
    _hold = None

    def __call__(self, frames, area, edge_thresh, hold, max_hold, fed, flush):
        y0, y1, x0, x1 = area
        key = (y1 - y0, x1 - x0, max_hold)
        if fed and (self._key, self._hold) != (key, hold):
            raise ValueError(f"EngineBoundedHoldCounter: the area, hold or max_hold changed to {key + (hold,)} after {fed} frames of a clip")
        self._fresh(key, self.ctx.frame_hold_bounded_state)
        self._hold = hold
        if fed and fed != self.fed:
            raise ValueError(f"EngineBoundedHoldCounter: fed {fed}, but {self.fed} frames of this clip went to earlier calls")
        self.fed = fed + len(frames)
        return self.ctx.frame_hold_bounded(self._device(frames), area, edge_thresh, hold, max_hold, self._state, fed, flush)


class HoldFrameSelector(_IntervalSelector):
    """ChangeFrameSelector for footage whose background moves behind the subtitle.  The change selector compares every edge pixel of the
    area with the frame before; a textured background that pans puts hundreds of edge pixels into the band that all move every
    frame, so every frame is a cut and no subtitle is found.  A subtitle's edges hold still for many frames and a moving background's
    do not: here the device counts only HELD edges, edge pixels inside a run of at least `hold` consecutive edge frames at that pixel
    (vse_frame_hold), and hold_intervals runs the unchanged automaton on those counts.  hold = 1 is ChangeFrameSelector.
    `hold_frames`, or max(1, min(32, round(hold_seconds * fps))) when it is None; hold_seconds=0.3 and the behaviour on real footage
    are not measured here (no real clips).  Known limit: background edges that stay on one pixel for `hold` frames still count (a
    static busy shot, a pan along an edge's own direction: in a numpy prototype a horizontal pan at hold 2-5 added intervals in the
    gaps).  While the background moves such intervals cost OCR calls and lose no subtitle; over a background that STANDS STILL they do
    lose subtitles: its edges sit in the denominator of the automaton's cut ratio and in neither numerator, so once they outnumber the
    text's own edges a subtitle that vanishes or is replaced makes no cut and is merged with its neighbour (a logo or watermark in the
    band does the same in a milder form, and keeps every gap frame present).  `max_hold_seconds` / `max_hold_frames` are for that
    footage: only runs of hold .. max_hold frames are counted (vse_frame_hold_bounded), a subtitle's edges holding for some seconds at
    most and a logo's or a static shot's far longer.  Both None (the default): the path above, call for call.  Otherwise max_hold =
    max_hold_frames, or round(max_hold_seconds * fps) when that is None; below hold or above 4000 is a ValueError.  Its limits: a
    subtitle shown for longer than max_hold disappears with the background; a static shot shorter than max_hold dilutes the ratio as
    before; pixels that flicker around the threshold make short runs and can add intervals in the gaps (OCR calls, no subtitle lost);
    the rows then trail the frames by max_hold instead of hold - 1, which is what one pass keeps (360 frames of 1080p 4:2:0 at 15 s
    and 24 fps are 1.1 GB).  12-15 s is a guess: nothing here is measured on real footage.
    run / iter_run: _IntervalSelector's, with fps; after the last batch a call without frames flushes the rows still pending.

    count_fn(frames [n,h,w,3] uint8, area (y0, y1, x0, x1) in their pixels, edge_thresh, hold, fed, flush) -> [rows,3] counts of the
    frames whose held mask the call completes: they trail the frames fed by hold - 1 until the flush (fed: frames of the clip given
    to earlier calls, 0 on the first batch; flush: the clip ends with this call).  Default: EngineHoldCounter on the shim's device.
    With max_hold_*: count_fn(frames, area, edge_thresh, hold, max_hold, fed, flush), whose rows trail by max_hold.  Default:
    EngineBoundedHoldCounter."""
    engine_count_fn = EngineHoldCounter

    def __init__(self, count_fn=None, hold_seconds=0.3, hold_frames=None, edge_thresh=128, change_ratio=0.5, min_edges=None,
                 min_frames=2, batch=64, focus_fn=None, max_hold_seconds=None, max_hold_frames=None, compositor=None, key_fn=None):
        super().__init__(count_fn, edge_thresh, change_ratio, min_edges, min_frames, batch, focus_fn, compositor, key_fn)
        self.hold_seconds, self.hold_frames = hold_seconds, hold_frames
        self.max_hold_seconds, self.max_hold_frames = max_hold_seconds, max_hold_frames
        if max_hold_seconds is not None or max_hold_frames is not None:
            self.engine_count_fn = EngineBoundedHoldCounter
        self.hold = None              # the hold of the last run, in frames
        self.max_hold = None          # ... and its max_hold; None: runs are not bounded

    def _min_frames(self, fps):
        hold = self.hold_frames if self.hold_frames is not None else max(1, min(32, int(round(self.hold_seconds * fps))))
        if not 1 <= hold <= 32:
            raise ValueError(f"HoldFrameSelector: hold_frames must be 1..32, not {hold}")
        self.hold = hold
        self.max_hold = None
        if self.max_hold_frames is not None or self.max_hold_seconds is not None:
            max_hold = int(self.max_hold_frames if self.max_hold_frames is not None else round(self.max_hold_seconds * fps))
            if not hold <= max_hold <= FRAME_HOLD_BOUNDED_MAX:
                raise ValueError(f"HoldFrameSelector: max_hold must be hold ({hold}) .. {FRAME_HOLD_BOUNDED_MAX} frames, not {max_hold}")
            self.max_hold = max_hold
        return max(self.min_frames, hold)                  # (hold_intervals' min_frames)

    def _args(self):
        return (self.hold,) if self.max_hold is None else (self.hold, self.max_hold)

    def _lag(self):
        return self.hold - 1 if self.max_hold is None else self.max_hold

    def _count(self, data, area, fed):
        return self.count_fn(data, area, self.edge_thresh, *self._args(), fed, False)

    def _flush(self, data, area, fed):
        return self.count_fn(data[:0], area, self.edge_thresh, *self._args(), fed, True)


# ---- the hold selector that finds its own area while the frames go by ---------------------------------------------------------------
class EngineCellsHoldMasks(DeviceState):
    """cells_fn of LocatingHoldSelector on the GPU (Context.frame_cells_hold_masks), the counterpart of EngineCellsMasks: keeps the device
    state and the mask buffer of the last region, threshold count, hold and `cap`, and `fed`, the frames fed since the last reset, which
    is the slot the next frame takes; (frames | None, area, engine.CellParams, reset, flush, thresholds, cap, hold) -> totals
    [nt,gy,gx,4], frames None with flush draining and closing the open runs.  `replay(area, q, rect, counter, hold, flush)` walks the
    slots 0 .. fed - 1 at threshold index q on `rect` (y0, y1, x0, x1 in the region's pixels) with the SELECTOR's hold at once
    (Context.frame_masks_replay_hold) -> frame_hold's rows of those frames, and sets up an EngineHoldCounter, its state, key and `fed`, so
    that its next call continues the clip on that rectangle."""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.fed, self._masks = 0, None

    def __call__(self, frames, area, params, reset, flush, thresholds, cap, hold):
        t = self.ctx.torch
        y0, y1, x0, x1 = area
        frames = t.empty((0, y1, x1, 3), dtype=t.uint8, device=self.ctx.tdev) if frames is None else self._device(frames)
        if self._fresh((y1 - y0, x1 - x0, len(thresholds), int(hold), int(cap)),
                       lambda h, w, nt, hold, _cap: self.ctx.frame_cells_hold_state(h, w, nt, hold)):
            self._masks, reset = self.ctx.frame_masks_buffer(y1 - y0, x1 - x0, len(thresholds), cap), True
        if reset:
            self.fed = 0
        totals = self.ctx.frame_cells_hold_masks(frames, area, thresholds, hold, params, self._state, self._masks, self.fed, self.fed, flush)
        self.fed += len(frames)
        return totals

    def replay(self, area, q, rect, counter, hold, flush):
        y0, y1, x0, x1 = area
        if self._key is None or self._key[:2] != (y1 - y0, x1 - x0) or not self.fed:
            raise ValueError(f"EngineCellsHoldMasks: no masks of a {y1 - y0} x {x1 - x0} region to replay")
        ry0, ry1, rx0, rx1 = rect
        counter._fresh((ry1 - ry0, rx1 - rx0, hold), self.ctx.frame_hold_state)
        counter.fed = self.fed
        return self.ctx.frame_masks_replay_hold(self._masks, q, 0, self.fed, rect, hold, counter._state, 0, flush)


class LocatingHoldSelector(_IntervalSelector):
    """HoldFrameSelector with sub_area="auto", in ONE pass over the frames: LocatingChangeSelector's shape for footage whose textured
    background moves behind the subtitle, where only the held automaton finds an area or a threshold.  The held mask of a rectangle is a
    walk along the frames over its pixels' EDGE bits, and an edge bit does not depend on the area, so up to the decision the batches
    (whole frames) go through cells_fn with the held automaton, which keeps every frame's edge words beside the locator's totals
    (vse_frame_cells_hold_masks), and nothing is yielded as closed.  The decision falls after frame `window` (a clip that ends sooner
    decides at its end): the cells are flushed, the totals read once, with edge_thresh="auto" area_locator.pick_edge_thresh chooses, and
    area_locator.locate_area decides on that threshold's totals, so area, threshold, `scores`, `totals` and `frames_scanned` are
    AreaLocator(automaton="hold", probe=(1, window)).run(...)'s, its warning and no area when no threshold scores included.  With an
    area, replay_fn walks the kept words of frames 1 .. window on it with the SELECTOR's hold (vse_frame_masks_replay_hold: integer for
    integer vse_frame_hold's rows) and leaves count_fn where it would stand after those frames: without a flush while the clip goes on,
    so the tracker has seen the rows 1 .. window - hold + 1 (iter_run's `tracker.fed`), with one when the clip ended inside the window.
    One IntervalTracker, built as HoldFrameSelector builds its own (min_frames at least hold), is fed them, the intervals it has closed
    are yielded with the deciding batch, and the rest of the frames run over the area's rows through count_fn like a plain
    HoldFrameSelector, the usual flush behind them: the intervals and counts are HoldFrameSelector(edge_thresh=the choice)'s over the
    whole clip on the located area.  Without an area, `area` stays None, `decided` is True and the generator ends, having consumed
    min(window, clip) frames exactly (the first `window` frames are a staged run of their own).  The held locator's limits carry over
    (area_locator's module text); whether a window of some length finds the band of a real film is not measured here (no real clips).

    cells_fn(frames [n,h,w,3] uint8 | None, area, engine.CellParams, reset, flush, thresholds, cap, hold) -> totals [nt,gy,gx,4]; default
    EngineCellsHoldMasks on the shim's device.  replay_fn(area, q, rect, count_fn, hold, flush) -> rows [.,3] at threshold index q on rect
    (y0, y1, x0, x1 in the region's pixels), after which count_fn's next call (fed = the frames replayed) continues the clip; default
    cells_fn.replay.  count_fn, hold_seconds, hold_frames: HoldFrameSelector's; count_fn is never called with fed = 0.  window: frames,
    required.  edge_thresh: an integer or "auto".  locator_params: AreaLocator's keyword arguments (thresholds, min_edges, change_ratio,
    min_seconds, max_seconds, plateau_frac, hold_seconds, hold_frames and locate_area's; automaton="hold" is implied and may be given);
    another automaton, max_hold_*, search_area and probe are refused, max_hold_* for the selector too.  Before the decision `tracker` is
    None."""

    def __init__(self, count_fn=None, cells_fn=None, replay_fn=None, window=None, locator_params=None, hold_seconds=0.3, hold_frames=None,
                 edge_thresh=128, change_ratio=0.5, min_edges=None, min_frames=2, batch=64, max_hold_seconds=None, max_hold_frames=None,
                 key_fn=None):
        super().__init__(count_fn, edge_thresh, change_ratio, min_edges, min_frames, batch, key_fn=key_fn)
        from . import area_locator
        if window is None or int(window) < 1:
            raise ValueError(f"{type(self).__name__}: window must be at least 1 frame, not {window}")
        self.window, self.cells_fn, self.replay_fn = int(window), cells_fn, replay_fn
        self.hold_seconds, self.hold_frames, self.hold = hold_seconds, hold_frames, None
        params = dict(locator_params or {})
        self._check_params(params, max_hold_seconds, max_hold_frames)
        self.locator = area_locator.AreaLocator(**{**params, "automaton": "hold", "edge_thresh": edge_thresh})
        self.area, self.tracker, self.decided = None, None, False
        self.scores = self.totals = None
        self.frames_scanned = 0

    # What LocatingBoundedHoldSelector changes: the default callables, what the constructor refuses, the bounds, the lag, and the
    # arguments that follow `cap` for cells_fn and stand in place of `hold` for replay_fn and count_fn.
    engine_count_fn, engine_cells_fn = EngineHoldCounter, EngineCellsHoldMasks

    def _check_params(self, params, max_hold_seconds, max_hold_frames):
        refused = [f"automaton={params['automaton']!r}"] if params.get("automaton", "hold") != "hold" else []
        refused += sorted(set(params) & {"max_hold_seconds", "max_hold_frames", "search_area", "probe"})
        refused += [f"the selector's {k}" for k, v in (("max_hold_seconds", max_hold_seconds), ("max_hold_frames", max_hold_frames))
                    if v is not None]
        if refused:
            raise ValueError("LocatingHoldSelector: the locator in the selector's pass counts whole frames with the held automaton, the "
                             f"kept words are replayed with unbounded runs and `window` says how many frames decide; it does not take "
                             f"{', '.join(refused)}")

    # `hold` from hold_frames / hold_seconds and the frame rate, and the tracker's min_frames, by HoldFrameSelector's own rule (which
    # reads the two bounds: runs are never bounded here)
    _min_frames = HoldFrameSelector._min_frames
    max_hold_seconds = max_hold_frames = None

    def _lag(self):
        return self.hold - 1

    def _args(self):
        return (self.hold,)

    def _locator_args(self, fps):
        loc = self.locator
        loc.hold = loc.hold_for(fps)          # the locator's, which area_params may set apart
        return (loc.hold,)

    def iter_run(self, frames, sub_area=None, fps=None, uploader=None):
        """HoldFrameSelector.iter_run over whole frames (sub_area must be None: this finds it); up to the decision every batch is yielded
        with no closed interval and `tracker` is None."""
        import logging

        import numpy as np
        from . import area_locator
        if sub_area is not None:
            raise ValueError(f"{type(self).__name__}: it finds the area itself and takes none, not {sub_area}")
        if self.count_fn is None or self.cells_fn is None:
            from . import shim
            self.count_fn = self.engine_count_fn(shim._context()) if self.count_fn is None else self.count_fn
            self.cells_fn = self.engine_cells_fn(shim._context()) if self.cells_fn is None else self.cells_fn
        replay = self.cells_fn.replay if self.replay_fn is None else self.replay_fn
        loc = self.locator
        ths = loc.thresholds if loc.auto else (loc.edge_thresh,)
        self.counts, self.intervals, self.tracker, self.decided, self.area = np.zeros((0, 3), np.int32), [], None, False, None
        self.edge_thresh = None if loc.auto else loc.edge_thresh
        self.scores = self.totals = None
        self.frames_scanned = 0
        it = iter(frames)
        bands = band_batches(islice(it, self.window), None, self.batch, type(self).__name__)
        if bands.area is None:
            return
        min_frames = self._min_frames(fps)    # (sets `hold`, the selector's)
        region, params = bands.area, loc.params(fps)
        cells_args, args = self._locator_args(fps), self._args()
        rows = []                             # the rows of the window [.,3], then of the frames behind it, batch by batch
        target = None                         # the located area in the pixels of its own rows, as count_fn takes it

        def host(c, shape):
            return np.asarray(c.cpu() if hasattr(c, "cpu") else c, np.int32).reshape(shape)

        def decide(scanned, ended):
            nonlocal target
            totals = self.cells_fn(None, region, params, False, True, ths, self.window, *cells_args)
            self.totals, self.frames_scanned, self.decided = host(totals, tuple(totals.shape)), scanned, True
            q, chosen = 0, self.totals[0]
            if loc.auto:
                static_frac = loc.locate_kwargs.get("static_frac", 0.95)
                self.scores = area_locator.edge_thresh_scores(self.totals, scanned, static_frac)
                q = area_locator.pick_edge_thresh(self.totals, ths, scanned, static_frac, loc.plateau_frac)
                if q is None:
                    logging.getLogger(area_locator.__name__).warning(
                        "edge_thresh='auto': none of the thresholds %s scores with the %s automaton in %d frames; falling back to %d", ths,
                        loc.describe_automaton(), scanned, area_locator.DEFAULT_EDGE_THRESH)
                    return []
                self.edge_thresh, chosen = ths[q], self.totals[q]
            else:
                self.totals = chosen          # (AreaLocator's totals at one threshold are [gy,gx,4])
            self.area = area_locator.locate_area(chosen, scanned, bands.geometry, bands.frame_hw, **loc.locate_kwargs)
            if self.area is None:
                return []
            y0, y1, x0, x1 = clip_area(self.area, *bands.frame_hw)
            target = (0, y1 - y0, x0, x1)
            rows.append(host(replay(region, q, (y0 - bands.geometry[0], y1 - bands.geometry[0], x0 - region[2], x1 - region[2]),
                                    self.count_fn, *args, ended), (-1, 3)))
            min_edges = default_min_edges(y1 - y0, x1 - x0) if self.min_edges is None else self.min_edges
            self.tracker = IntervalTracker(min_edges, self.change_ratio, min_frames)
            self.intervals = self.tracker.feed(rows[-1])
            return list(self.intervals)

        fed, closed = 0, []
        with closing(staging.staged_batches(bands, uploader)) as staged:
            for items, data in staged:
                self.cells_fn(data if self.key_fn is None else self.key_fn(data, region), region, params, fed == 0, False, ths, self.window,
                              *cells_args)
                fed += len(items)
                if fed >= self.window:
                    closed = decide(fed, False)
                yield items, closed
        if not self.decided:                  # the clip ended inside the window: the replay has flushed
            closed = decide(fed, True)
        elif self.area is not None:
            closed = []                       # (they went out with the deciding batch)
            empty = np.zeros((0, target[1], bands.frame_hw[1], 3), np.uint8)
            rest = band_batches(it, self.area, self.batch, type(self).__name__)
            if rest.area is not None:
                with closing(staging.staged_batches(rest, uploader)) as staged:
                    for items, data in staged:
                        keyed = data if self.key_fn is None else self.key_fn(data, target)       # (over the located rectangle)
                        rows.append(host(self.count_fn(keyed, target, self.edge_thresh, *args, fed, False), (-1, 3)))
                        got = self.tracker.feed(rows[-1])
                        self.intervals += got
                        fed += len(items)
                        empty = data[:0]
                        yield items, got
            rows.append(host(self.count_fn(empty, target, self.edge_thresh, *args, fed, True), (-1, 3)))
            closed = self.tracker.feed(rows[-1])
            self.intervals += closed
        if self.area is None:
            return
        last = self.tracker.flush()
        self.intervals += last
        self.counts = np.concatenate(rows)
        yield [], closed + last


# ---- the same with bounded runs, for a busy background that stands still ------------------------------------------------------------
class EngineCellsHoldBoundedMasks(DeviceState):
    """cells_fn of LocatingBoundedHoldSelector on the GPU (Context.frame_cells_hold_bounded_masks), EngineCellsHoldMasks with the locator's
    max_hold: keeps the device state and the mask buffer of the last region, threshold count, max_hold and `cap`, and `fed`; (frames |
    None, area, engine.CellParams, reset, flush, thresholds, cap, hold, max_hold) -> totals [nt,gy,gx,4], frames None with flush draining
    and closing the open runs.  `replay(area, q, rect, counter, hold, max_hold, flush)` walks the slots 0 .. fed - 1 at threshold index q
    on `rect` (y0, y1, x0, x1 in the region's pixels) with the SELECTOR's hold and max_hold at once
    (Context.frame_masks_replay_hold_bounded) -> frame_hold_bounded's rows of those frames, and sets up an EngineBoundedHoldCounter, its
    state, key, hold and `fed`, so that its next call continues the clip on that rectangle."""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.fed, self._masks = 0, None

    def __call__(self, frames, area, params, reset, flush, thresholds, cap, hold, max_hold):
        t = self.ctx.torch
        y0, y1, x0, x1 = area
        frames = t.empty((0, y1, x1, 3), dtype=t.uint8, device=self.ctx.tdev) if frames is None else self._device(frames)
        if self._fresh((y1 - y0, x1 - x0, len(thresholds), int(max_hold), int(cap)),
                       lambda h, w, nt, max_hold, _cap: self.ctx.frame_cells_hold_bounded_state(h, w, nt, max_hold)):
            self._masks, reset = self.ctx.frame_masks_buffer(y1 - y0, x1 - x0, len(thresholds), cap), True
        if reset:
            self.fed = 0
        totals = self.ctx.frame_cells_hold_bounded_masks(frames, area, thresholds, hold, max_hold, params, self._state, self._masks,
                                                         self.fed, self.fed, flush)
        self.fed += len(frames)
        return totals

    def replay(self, area, q, rect, counter, hold, max_hold, flush):
        y0, y1, x0, x1 = area
        if self._key is None or self._key[:2] != (y1 - y0, x1 - x0) or not self.fed:
            raise ValueError(f"EngineCellsHoldBoundedMasks: no masks of a {y1 - y0} x {x1 - x0} region to replay")
        ry0, ry1, rx0, rx1 = rect
        counter._fresh((ry1 - ry0, rx1 - rx0, max_hold), self.ctx.frame_hold_bounded_state)
        counter._hold, counter.fed = hold, self.fed
        return self.ctx.frame_masks_replay_hold_bounded(self._masks, q, 0, self.fed, rect, hold, max_hold, counter._state, 0, flush)


class LocatingBoundedHoldSelector(LocatingHoldSelector):
    """HoldFrameSelector(max_hold_*) with sub_area="auto", in ONE pass over the frames: LocatingHoldSelector for the footage of bounded
    runs, a busy background that stands still behind the subtitle (an interview, a news desk, a logo in the band), where the unbounded
    held automaton finds no area and the unbounded selector merges the subtitles.  iter_run is LocatingHoldSelector's, text for text;
    what differs are the hooks: the locator counts bounded masks and keeps the edge words (vse_frame_cells_hold_bounded_masks), the
    replay walks them with the SELECTOR's hold and max_hold (vse_frame_masks_replay_hold_bounded: integer for integer
    vse_frame_hold_bounded's rows and state), count_fn has the bounded counter's signature, and the rows trail the frames by the
    selector's max_hold: after a window of W frames without a flush the tracker has seen the rows 1 .. max(0, W - max_hold).  So area,
    threshold, `scores`, `totals` and `frames_scanned` are AreaLocator(automaton="hold", max_hold_*=the locator's, probe=(1,
    window)).run(...)'s, and the intervals and counts HoldFrameSelector(max_hold_*=the selector's, edge_thresh=the choice)'s over the
    whole clip on the located area.  The bounded locator's limits carry over (area_locator's module text: a gap shorter than max_hold
    stays present, a subtitle shown for longer than max_hold vanishes); max_hold and the window are guesses, nothing is measured on
    real footage.

    cells_fn(frames | None, area, engine.CellParams, reset, flush, thresholds, cap, hold, max_hold) -> totals; default
    EngineCellsHoldBoundedMasks.  replay_fn(area, q, rect, count_fn, hold, max_hold, flush) -> rows; default cells_fn.replay.  count_fn:
    HoldFrameSelector's with max_hold_* (frames, area, edge_thresh, hold, max_hold, fed, flush); default EngineBoundedHoldCounter.
    max_hold_seconds / max_hold_frames: the selector's, one of them required.  locator_params: as LocatingHoldSelector's, and
    max_hold_seconds / max_hold_frames for the LOCATOR, one of them required too (they are not inherited from the selector's: the two
    may differ); another automaton, search_area and probe are refused."""
    engine_count_fn, engine_cells_fn = EngineBoundedHoldCounter, EngineCellsHoldBoundedMasks

    def __init__(self, count_fn=None, cells_fn=None, replay_fn=None, window=None, locator_params=None, hold_seconds=0.3, hold_frames=None,
                 edge_thresh=128, change_ratio=0.5, min_edges=None, min_frames=2, batch=64, max_hold_seconds=None, max_hold_frames=None,
                 key_fn=None):
        super().__init__(count_fn, cells_fn, replay_fn, window, locator_params, hold_seconds, hold_frames, edge_thresh, change_ratio,
                         min_edges, min_frames, batch, max_hold_seconds, max_hold_frames, key_fn)
        self.max_hold_seconds, self.max_hold_frames, self.max_hold = max_hold_seconds, max_hold_frames, None

    def _check_params(self, params, max_hold_seconds, max_hold_frames):
        refused = [f"automaton={params['automaton']!r}"] if params.get("automaton", "hold") != "hold" else []
        refused += sorted(set(params) & {"search_area", "probe"})
        if refused:
            raise ValueError("LocatingBoundedHoldSelector: the locator in the selector's pass counts whole frames with the held automaton "
                             f"on bounded runs and `window` says how many frames decide; it does not take {', '.join(refused)}")
        if max_hold_seconds is None and max_hold_frames is None:
            raise ValueError("LocatingBoundedHoldSelector: the selector's max_hold_seconds or max_hold_frames is required (without a "
                             "bound it is LocatingHoldSelector)")
        if params.get("max_hold_seconds") is None and params.get("max_hold_frames") is None:
            raise ValueError("LocatingBoundedHoldSelector: locator_params' max_hold_seconds or max_hold_frames is required: the locator's "
                             "bound is not inherited from the selector's")

    def _lag(self):
        return self.max_hold

    def _args(self):
        return (self.hold, self.max_hold)

    def _locator_args(self, fps):
        loc = self.locator
        loc.hold, loc.max_hold = loc.hold_for(fps), loc.max_hold_for(fps)
        return (loc.hold, loc.max_hold)


# ---- interval composite (one picture per interval of the change selector) ------------------------------------------------
COMPOSITE_MODES = ("min", "max", "mean")


def trim_range(start, end, fps, trim_seconds):
    """The frames of the interval start..end (1-based, inclusive) that are composited: start + tr .. end - tr with
    tr = min(round(trim_seconds * fps), (end - start) // 2), so at least one frame always remains."""
    tr = min(int(round(trim_seconds * fps)), (end - start) // 2)
    return start + tr, end - tr


def sharpest_rep(start, end, focus, fps, trim_seconds=0.25):
    """The frame on which the interval start..end (1-based, inclusive) is recognised with interval_frame="sharpest": among the frames
    trim_range(start, end, fps, trim_seconds) leaves (fades at either end are left out as the compositor leaves them out; an interval
    shorter than twice the trim keeps its middle) the one with the largest focus, the earliest of equals, hence the first candidate
    when every focus is 0.  focus: per frame of the clip, row no - 1 for frame no: [frames, 2] kept, focus (a selector's `focus`), or
    the focus column alone."""
    first, last = trim_range(start, end, fps, trim_seconds)
    col = [int(r[1]) if hasattr(r, "__len__") else int(r) for r in focus[first - 1:last]]
    return first + max(range(len(col)), key=lambda i: (col[i], -i))


class EngineCompositor(DeviceState):
    """accumulate_fn of IntervalCompositor on the GPU (Context.interval_accumulate / interval_composite): keeps the device state
    of the last area and the frame count of the open interval between calls."""
    _count = 0

    def __call__(self, frames, area, reset, mode=None):
        y0, y1, x0, x1 = area
        reset = self._fresh((y1 - y0, x1 - x0), self.ctx.interval_state) or reset
        self.ctx.interval_accumulate(self._device(frames), area, self._state, reset)
        self._count = len(frames) if reset else self._count + len(frames)
        return None if mode is None else self.ctx.interval_composite(self._state, y1 - y0, x1 - x0, self._count, mode)


class IntervalCompositor:
    """One picture of the subtitle area per interval of ChangeFrameSelector, made of ALL its frames instead of the middle one: a
    subtitle stands still while the picture behind it moves, so the per-pixel minimum (light text; `max` for dark text, `mean` to
    average noise) over the interval keeps the text and flattens the background.  VideoSubFinder builds the pictures it hands to
    OCR on the same idea; this is not its algorithm.  How much it helps recognition on real footage is not measured here (no
    real clips, stand-in recogniser weights); the integers, the plumbing and the cost are pinned.

    accumulate_fn(frames [n,h,w,3] uint8, area (y0, y1, x0, x1) in their pixels, reset, mode=None): folds the frames into the open
    interval's per-byte min / max / sum (reset: the interval starts with these frames) and, with a mode, returns its composite
    uint8 [y1-y0, x1-x0, 3].  Default: EngineCompositor on the shim's device.
    Fades at either end of a subtitle would drag a `min` of light text down, so trim_seconds of frames are left out at both ends
    (trim_range).  Host memory: one area patch per interval, kept in RAM; a 1080p default band (226 x 1728 pixels) is about 1 MB."""

    def __init__(self, accumulate_fn=None, mode="min", trim_seconds=0.25, batch=64):
        if mode not in COMPOSITE_MODES:
            raise ValueError(f"IntervalCompositor: mode must be one of {COMPOSITE_MODES}, not {mode!r}")
        self.accumulate_fn, self.mode, self.trim_seconds, self.batch = accumulate_fn, mode, trim_seconds, batch
        self.area = None              # (y0, y1, x0, x1): the area clipped to the frame, where the patches belong
        self.patches = None

    def run(self, frames, sub_area, intervals, fps, uploader=None, only=None):
        """frames: iterable of uint8 BGR frames in decode order (read once, and not beyond the last frame that is needed);
        sub_area: clipped to the frame exactly as ChangeFrameSelector.run clips it; intervals: its [(start, end, rep)], ascending;
        only: a range of interval indices (a rank's shard), the others are not composited -> {rep: uint8 ndarray [ah, aw, 3]}.
        Only the area's rows of the frames inside a used range are staged (staging.staged_batches)."""
        import numpy as np
        if self.accumulate_fn is None:
            from . import shim
            self.accumulate_fn = EngineCompositor(shim._context())
        todo = []                     # (first, last, rep) of the intervals to composite, ascending and disjoint
        for k, (start, end, rep) in enumerate(intervals):
            if only is None or k in only:
                first, last = trim_range(start, end, fps, self.trim_seconds)
                if todo and first <= todo[-1][1]:
                    raise ValueError(f"IntervalCompositor: intervals must ascend without overlap, got {intervals[k - 1]} then {intervals[k]}")
                todo.append((first, last, rep))
        self.patches = {}
        if not todo:
            return self.patches
        it = iter(frames)
        geometry = []                 # [y0, y1, x0, x1] once the first frame has been seen

        def rows(f):
            if not geometry:
                h, w = f.shape[:2]
                y0, y1, x0, x1 = clip_area(sub_area, h, w)
                if y1 <= y0 or x1 <= x0:
                    raise ValueError(f"IntervalCompositor: subtitle area {sub_area} leaves nothing of a {h} x {w} frame")
                geometry.extend((y0, y1, x0, x1))
            return f[geometry[0]:geometry[1]]

        def batches():
            """lists of ((rep, opens the interval, closes it), area rows): consecutive frames of ONE interval, at most `batch`"""
            no = 0
            for first, last, rep in todo:
                buf = []
                while no < last:
                    f = next(it, None)
                    if f is None:
                        raise ValueError(f"IntervalCompositor: the clip ends at frame {no}, inside or before the interval ending at {last}")
                    no += 1
                    if no < first:
                        continue
                    if len(buf) == self.batch:
                        yield buf
                        buf = []
                    buf.append(((rep, no == first, no == last), rows(f)))
                yield buf

        def fold(items, data):
            (rep, opens, _), (_, _, closes) = items[0][0], items[-1][0]
            y0, y1, x0, x1 = geometry
            out = self.accumulate_fn(data, (0, y1 - y0, x0, x1), opens, self.mode if closes else None)
            if closes:
                self.patches[rep] = out.cpu().numpy() if hasattr(out, "cpu") else np.array(out)

        for items, data in staging.staged_batches(batches(), uploader):
            fold(items, data)
        self.area = tuple(geometry)
        return self.patches


# ---- streaming composite (the compositor's pictures, made in the selector's own pass) ------------------------------------------
class EngineStreamer(DeviceState):
    """stream_fn of StreamingCompositor on the GPU (Context.interval_stream): keeps the device state (accumulators and ring) of the
    last area and `cap` between calls.  Nothing in the state is read that an earlier call of the same clip did not write, so a new
    clip needs no reset; the area or cap may change only where a clip starts."""

    def __call__(self, frames, area, cap, fed, segs, store_from, mode):
        y0, y1, x0, x1 = area
        key = (y1 - y0, x1 - x0, cap)
        if fed and self._key != key:
            raise ValueError(f"EngineStreamer: the area or cap changed to {key} after {fed} frames of a clip")
        self._fresh(key, self.ctx.interval_stream_state)
        return self.ctx.interval_stream(self._device(frames), area, self._state, cap, fed, segs, store_from, mode)


class StreamingCompositor:
    """IntervalCompositor's pictures without its pass over the clip: a selector given this as `compositor` hands it every staged batch
    while that is still on the device, and the per-byte min / max / mean over trim_range of each interval is folded there and then
    (vse_interval_stream).  What keeps IntervalCompositor waiting is only that an interval's end, hence its trimmed range, is unknown
    when a frame arrives.  With T = round(trim_seconds * fps), frame k of an open run s..t belongs to the picture for certain once
    t >= k + T and k >= s + T; the undecided frames, at most T + 1 of them plus the selector's lag L (frames whose rows have not come
    yet), wait in a ring of cap = L + T + 1 area bands on the device.  Per batch, with t = tracker.fed and s = tracker.open_start:
      every closed (start, end, rep): one segment max(first, folded_to + 1) .. last of trim_range(start, end), which CONTINUEs the
        open-run fold when that belongs to `start`, and EMITs with frames = last - first + 1;
      an open run with t - s > 2 T: the fold advances to t - T - 1 without EMIT, from s + T;  floor = t - T
        (the last certain frame t - T is held back: the run may end at t, and the segment that EMITs it must have a frame);
      an open run with t - s <= 2 T: nothing is folded;  floor = (s + t) // 2, the earliest frame the picture can start at;
      no open run: floor = t + 1.
    The batch frames from `floor` on are stored, the ring frames below it forgotten; that the ring never has to hold more than cap
    frames is asserted on every call, as is that every frame a segment names is in the batch or the ring.  More than
    INTERVAL_STREAM_MAX_SEGS segments go in several calls on the same batch, of which only the last stores.  A run dropped for
    min_frames leaves a stale fold behind, which the next run's first segment does not CONTINUE.  The bytes are IntervalCompositor.run's.

    stream_fn(frames [n,h,w,3] uint8, area (y0, y1, x0, x1) in their pixels, cap, fed, segs [(first, last, flags, frames)], store_from,
    mode) -> [EMITs, y1-y0, x1-x0, 3] uint8, the composites of the EMIT segments in order (Context.interval_stream).  Default:
    EngineStreamer on the shim's device.  `patches`: {rep: uint8 ndarray [ah, aw, 3]}, a plain dict as IntervalCompositor's: the
    composites of a call are read back when it returns, one read-back per batch in which a subtitle ends (the selector has just read
    that batch's counts back, so the device is waited for either way)."""

    def __init__(self, stream_fn=None, mode="min", trim_seconds=0.25):
        if mode not in COMPOSITE_MODES:
            raise ValueError(f"StreamingCompositor: mode must be one of {COMPOSITE_MODES}, not {mode!r}")
        self.stream_fn, self.mode, self.trim_seconds = stream_fn, mode, trim_seconds
        self.area = None              # the area in the band's own pixels (0, y1 - y0, x0, x1), once a batch has been seen
        self.patches = {}
        self.cap = self.peak_ring = None

    def begin(self, fps, lag):
        """A clip starts: its frame rate and the frames by which the selector's rows trail its frames."""
        if self.stream_fn is None:
            from . import shim
            self.stream_fn = EngineStreamer(shim._context())
        self.fps, self.lag = fps, int(lag)
        self.trim = int(round(self.trim_seconds * fps))
        self.cap, self.peak_ring = self.lag + self.trim + 1, 0
        self.patches = {}
        self._fed = 0                 # frames handed over so far
        self._floor = 1               # the ring holds the frames _floor .. _fed
        self._fold_of, self._folded_to = None, 0          # the run whose fold the accumulators hold, and its last folded frame

    def __call__(self, data, area, n, tracker, closed):
        import numpy as np
        from .engine import INTERVAL_SEG_CONTINUE, INTERVAL_SEG_EMIT, INTERVAL_STREAM_MAX_SEGS
        T, fed = self.trim, self._fed
        t, s = tracker.fed, tracker.open_start
        assert fed + n - t <= self.lag or n == 0, f"StreamingCompositor: the rows trail by {fed + n - t} frames, more than the lag {self.lag}"
        segs, reps = [], []
        for start, end, rep in closed:
            first, last = trim_range(start, end, self.fps, self.trim_seconds)
            cont = self._fold_of == start
            segs.append((max(first, self._folded_to + 1) if cont else first, last, (INTERVAL_SEG_CONTINUE if cont else 0) | INTERVAL_SEG_EMIT,
                         last - first + 1))
            reps.append(rep)
            self._fold_of = None
        if s is None:
            floor = t + 1
        elif t - s > 2 * T:
            cont = self._fold_of == s
            lo = self._folded_to + 1 if cont else s + T
            if lo <= t - T - 1:
                segs.append((lo, t - T - 1, INTERVAL_SEG_CONTINUE if cont else 0, 0))
                self._fold_of, self._folded_to = s, t - T - 1
            floor = t - T
        else:
            floor = (s + t) // 2
        for k, (lo, hi, flags, _frames) in enumerate(segs):
            assert lo <= hi and lo >= self._floor and hi <= fed + n and (k == 0 or lo > segs[k - 1][1]), \
                f"StreamingCompositor: segment {lo}..{hi} is not in the ring from {self._floor} or the batch {fed + 1}..{fed + n}"
            assert not (flags & INTERVAL_SEG_CONTINUE) or k == 0
        held = fed + n - floor + 1
        assert held <= self.cap and floor >= self._floor, f"StreamingCompositor: {held} frames to keep from {floor}, the ring holds {self.cap}"
        self.peak_ring = max(self.peak_ring, held)
        out = []
        calls = [segs[k:k + INTERVAL_STREAM_MAX_SEGS] for k in range(0, len(segs), INTERVAL_STREAM_MAX_SEGS)] or [[]]
        for k, part in enumerate(calls):
            final = k == len(calls) - 1
            if not part and (not n or floor > fed + n):
                break                                     # nothing to read and nothing to store
            res = self.stream_fn(data, area, self.cap, fed, part, floor if final else fed + n + 1, self.mode)
            emits = sum(1 for g in part if g[2] & INTERVAL_SEG_EMIT)
            if emits:
                res = res.cpu().numpy() if hasattr(res, "cpu") else np.asarray(res)
                out += [np.array(res[j]) for j in range(emits)]           # (copies: a patch does not keep its call's others alive)
        assert len(out) == len(reps)
        self.patches.update(zip(reps, out))
        self.area, self._fed, self._floor = tuple(area), fed + n, floor


# ---- interval fusion (several frames per interval of the change selector, fused in probability space) ----------------------
def fuse_samples(start, end, rep, fps, samples, trim_seconds):
    """The frames of the interval (start, end, rep) that are recognised together -> (frame numbers ascending, position of the one the
    detector runs on).  first, last = trim_range(...), n = last - first + 1, K = min(samples, n): K == 1 is [rep]; otherwise
    first + (i * (n - 1)) // (K - 1) for i in 0 .. K - 1, both ends included.  The detect member is the sample nearest to rep, the
    earlier one on a tie."""
    first, last = trim_range(start, end, fps, trim_seconds)
    n = last - first + 1
    k = min(int(samples), n)
    nos = [rep] if k <= 1 else [first + (i * (n - 1)) // (k - 1) for i in range(k)]
    return nos, min(range(len(nos)), key=lambda i: (abs(nos[i] - rep), i))


class IntervalFuser:
    """IntervalCompositor's sibling: instead of one picture made of all frames of an interval, up to `samples` frames of it go through
    the recogniser and their per-step class probabilities are averaged before the CTC decode (shim.OcrRecogniser.predict_fused): the
    boxes are detected once, on the sample nearest to the interval's middle frame, and read in every sample.  That needs no knowledge
    of the text's polarity and also averages what is not background: compression noise, a glyph between two near-tied classes, a fade.
    How much it helps recognition on real footage is not measured here (no real clips, stand-in recogniser weights); the integers,
    the plumbing and the cost (the recogniser runs once per sample) are pinned.

    fuse_fn(frames [n,h,w,3] uint8, groups) -> [(dt_box, rec_res)] per group; groups = [(indices of the members among these frames,
    position in that list of the member to detect on)].  Default: predict_fused of one shim.OcrRecogniser on the shim's device.
    Fades at either end are left out as the compositor leaves them out (trim_range, trim_seconds).  Whole intervals are gathered into
    one call until one more would exceed `batch` frames."""

    def __init__(self, fuse_fn=None, samples=5, trim_seconds=0.25, batch=64):
        if samples < 1 or samples > batch:
            raise ValueError(f"IntervalFuser: samples must be 1..batch ({batch}), not {samples}: an interval is never split over two calls")
        self.fuse_fn, self.samples, self.trim_seconds, self.batch = fuse_fn, int(samples), trim_seconds, int(batch)
        self.results = None

    def run(self, frames, intervals, fps, uploader=None, only=None, default_area=None):
        """frames: iterable of uint8 BGR frames in decode order (read once, and not beyond the last frame that is needed); intervals:
        the selector's [(start, end, rep)], ascending; only: a range of interval indices (a rank's shard), the others are not read;
        default_area: the half-frame crop a task's frame gets (extractor.frame_preprocess), applied to every sample
        -> {rep: (dt_box, rec_res)}.  The sampled frames are staged by staging.staged_batches."""
        if self.fuse_fn is None:
            from . import shim
            self.fuse_fn = shim.OcrRecogniser().predict_fused
        plan = [[]]                   # per call: [(rep, frame numbers, detect position)], whole intervals, at most `batch` frames
        last_no = 0
        for k, (start, end, rep) in enumerate(intervals):
            if only is None or k in only:
                nos, pos = fuse_samples(start, end, rep, fps, self.samples, self.trim_seconds)
                if nos[0] <= last_no:
                    raise ValueError(f"IntervalFuser: intervals must ascend without overlap, got {intervals[k - 1]} then {intervals[k]}")
                last_no = nos[-1]
                if plan[-1] and sum(len(n) for _r, n, _p in plan[-1]) + len(nos) > self.batch:
                    plan.append([])
                plan[-1].append((rep, nos, pos))
        self.results = {}
        if not plan[0]:
            return self.results
        it = iter(frames)

        def batches():
            """lists of (frame number, frame): the samples of one call's intervals, in decode order"""
            from .extractor import frame_preprocess
            no = 0
            for call in plan:
                buf = []
                for _rep, nos, _pos in call:
                    for want in nos:
                        while no < want:
                            f = next(it, None)
                            if f is None:
                                raise ValueError(f"IntervalFuser: the clip ends at frame {no}, before the sample at frame {want}")
                            no += 1
                        buf.append((no, frame_preprocess(default_area, f) if default_area is not None else f))
                yield buf

        def fuse(call, data):
            groups, at = [], 0
            for _rep, nos, pos in call:
                groups.append((list(range(at, at + len(nos))), pos))
                at += len(nos)
            out = self.fuse_fn(data, groups)
            if len(out) != len(call):
                raise ValueError(f"IntervalFuser: fuse_fn returned {len(out)} results for {len(call)} intervals")
            for (rep, _nos, _pos), r in zip(call, out):
                self.results[rep] = r

        for call, (_items, data) in zip(plan, staging.staged_batches(batches(), uploader)):
            fuse(call, data)
        return self.results


# ---- interval quantile (a per-pixel order statistic over a few samples of each interval of the change selector) ---------------
def quantile_rank(quantile, k):
    """The 0-based rank among k sorted samples that stands for `quantile` in [0, 1], in integers: the quantile in thousandths times
    k - 1, rounded to nearest with halves up.  0 -> 0 (the minimum), 1 -> k - 1 (the maximum), 0.5 with odd k -> the median."""
    return (int(round(quantile * 1000)) * (k - 1) + 500) // 1000


class EngineRanker(DeviceState):
    """rank_fn of IntervalQuantile on the GPU (Context.interval_rank).  The kernel is stateless: nothing is kept between calls."""

    def __call__(self, frames, area, rank):
        return self.ctx.interval_rank(self._device(frames), area, rank)


class IntervalQuantile:
    """IntervalCompositor's robust sibling: one picture of the subtitle area per interval, each byte the `quantile` of that byte over up
    to `samples` evenly spaced frames of the interval (fuse_samples, the frames IntervalFuser reads).  The temporal median of a subtitle
    that stands still over a picture that moves is the subtitle's own value at text pixels whatever its colour, so nobody has to know
    whether the text is light (`min`) or dark (`max`); a minority of outlier frames (a flash, a black frame, a cut found one frame
    late, a half-faded frame) cannot move it, where one of them destroys a `min` or `max`; a low or high quantile is the robust form
    of those two.  Only the samples are staged: min(samples, trimmed length) frames per interval instead of all of them.
    The quantile is exact over the trimmed interval whenever that has at most `samples` frames and an estimate from `samples` frames
    otherwise; an exact quantile over every frame is not attempted.  How much the picture helps recognition on real footage is not
    measured here (no real clips, stand-in recogniser weights); the integers, the plumbing and the cost are pinned.

    rank_fn(frames [k,h,w,3] uint8, area (y0, y1, x0, x1) in their pixels, rank) -> uint8 [y1-y0, x1-x0, 3]: per byte, element `rank`
    (0-based) of the k frames' values sorted ascending.  Default: EngineRanker on the shim's device.  Each interval's rank is
    quantile_rank(quantile, its number of samples).  Whole intervals are gathered into one staged batch until one more would exceed
    `batch` frames; rank_fn is then called once per interval, on its slice of the batch."""

    def __init__(self, rank_fn=None, quantile=0.5, samples=15, trim_seconds=0.25, batch=64):
        if not 0 <= quantile <= 1:
            raise ValueError(f"IntervalQuantile: quantile must be in [0, 1], not {quantile!r}")
        if samples < 1 or samples > min(batch, INTERVAL_RANK_MAX):
            raise ValueError(f"IntervalQuantile: samples must be 1..min(batch, {INTERVAL_RANK_MAX}) = {min(batch, INTERVAL_RANK_MAX)}, not "
                             f"{samples}: an interval is ranked in one call of at most {INTERVAL_RANK_MAX} frames")
        self.rank_fn, self.quantile, self.samples, self.trim_seconds, self.batch = rank_fn, quantile, int(samples), trim_seconds, int(batch)
        self.area = None              # (y0, y1, x0, x1): the area clipped to the frame, where the patches belong
        self.patches = None

    def run(self, frames, sub_area, intervals, fps, uploader=None, only=None):
        """frames: iterable of uint8 BGR frames in decode order (read once, and not beyond the last sample that is needed); sub_area:
        clipped to the frame exactly as ChangeFrameSelector.run clips it; intervals: its [(start, end, rep)], ascending; only: a range
        of interval indices (a rank's shard), the others are not read -> {rep: uint8 ndarray [ah, aw, 3]}.  Only the area's rows of
        the sampled frames are staged (staging.staged_batches)."""
        import numpy as np
        if self.rank_fn is None:
            from . import shim
            self.rank_fn = EngineRanker(shim._context())
        plan = [[]]                   # per staged batch: [(rep, frame numbers)], whole intervals, at most `batch` frames
        last_no = 0
        for k, (start, end, rep) in enumerate(intervals):
            if only is None or k in only:
                nos, _pos = fuse_samples(start, end, rep, fps, self.samples, self.trim_seconds)
                if nos[0] <= last_no:
                    raise ValueError(f"IntervalQuantile: intervals must ascend without overlap, got {intervals[k - 1]} then {intervals[k]}")
                last_no = nos[-1]
                if plan[-1] and sum(len(n) for _r, n in plan[-1]) + len(nos) > self.batch:
                    plan.append([])
                plan[-1].append((rep, nos))
        self.patches = {}
        if not plan[0]:
            return self.patches
        it = iter(frames)
        geometry = []                 # [y0, y1, x0, x1] once the first frame has been seen

        def rows(f):
            if not geometry:
                h, w = f.shape[:2]
                y0, y1, x0, x1 = clip_area(sub_area, h, w)
                if y1 <= y0 or x1 <= x0:
                    raise ValueError(f"IntervalQuantile: subtitle area {sub_area} leaves nothing of a {h} x {w} frame")
                geometry.extend((y0, y1, x0, x1))
            return f[geometry[0]:geometry[1]]

        def batches():
            """lists of (frame number, area rows): the samples of one staged batch's intervals, in decode order"""
            no = 0
            for call in plan:
                buf = []
                for _rep, nos in call:
                    for want in nos:
                        while no < want:
                            f = next(it, None)
                            if f is None:
                                raise ValueError(f"IntervalQuantile: the clip ends at frame {no}, before the sample at frame {want}")
                            no += 1
                        buf.append((no, rows(f)))
                yield buf

        for call, (_items, data) in zip(plan, staging.staged_batches(batches(), uploader)):
            y0, y1, x0, x1 = geometry
            at = 0
            for rep, nos in call:
                out = self.rank_fn(data[at:at + len(nos)], (0, y1 - y0, x0, x1), quantile_rank(self.quantile, len(nos)))
                self.patches[rep] = out.cpu().numpy() if hasattr(out, "cpu") else np.array(out)
                at += len(nos)
        self.area = tuple(geometry)
        return self.patches


# ---- streaming quantile (the quantile's pictures, made in the selector's own pass) ---------------------------------------------
class EngineRingRanker(DeviceState):
    """ring_fn of StreamingQuantile on the GPU: Context.interval_stream with no segments parks the batch in the ring, then
    Context.interval_ring_rank ranks the groups where their frames lie.  Keeps the device state (of which only the ring is used) of
    the last area and `cap` between calls.  Nothing in the ring is read that an earlier call of the same clip did not write, so a new
    clip needs no reset; the area or cap may change only where a clip starts."""

    def __call__(self, frames, area, cap, fed, n, groups):
        y0, y1, x0, x1 = area
        key = (y1 - y0, x1 - x0, cap)
        if fed and self._key != key:
            raise ValueError(f"EngineRingRanker: the area or cap changed to {key} after {fed} frames of a clip")
        self._fresh(key, self.ctx.interval_stream_state)
        if n:
            self.ctx.interval_stream(self._device(frames), area, self._state, cap, fed, [], fed + 1, "min")
        return self.ctx.interval_ring_rank(self._state, y1 - y0, x1 - x0, cap, fed + n, groups)


class StreamingQuantile:
    """IntervalQuantile's pictures without its pass over the clip, hence also from a pipe: a selector given this as `compositor` hands
    it every staged batch while that is still on the device; the area band of EVERY frame is parked in a ring of `cap` bands there
    (frame f in slot f % cap), and when a subtitle's end is known its samples, fuse_samples' frames as IntervalQuantile reads them,
    are ranked where they lie (vse_interval_ring_rank).  The second look at frames already gone costs device memory, not a decode.
    `ring_seconds` is a policy, not a measurement: with R = round(ring_seconds * fps), T = round(trim_seconds * fps), L the selector's
    lag and B its batch, cap = R + T + L + B + 1, and every interval whose TRIMMED range has at most R + 1 frames is ranked on exactly
    IntervalQuantile's samples.  The argument: an interval (start, end) closes in the call that brings the row of frame end + 1, so
    end >= t', the last row seen before this call, and t' >= fed - L for the frames `fed` handed over before it (asserted); the call
    stores n <= B frames first, after which the ring holds oldest = fed + n - cap + 1 onwards.  The first sample is first = last -
    (frames - 1) with last >= end - T, so first >= fed - L - T - (frames - 1) >= fed + n - cap + 1 whenever frames <= R + 1.
    A longer interval whose first sample has left the ring is sampled over [oldest, last] instead: K = min(samples, last - oldest +
    1) frames oldest + (i (last - oldest)) // (K - 1), and for K == 1 the frame of the ring nearest to rep; it counts in `clamped`
    and one warning is logged per clip, the treatment the extractor's retain_bytes gets.  Its picture then describes the end of the
    subtitle only; its times are untouched.  A 1080p default band is 1.18 MB, so 60 s at 24 fps are about 1.8 GB of device memory.
    That every frame named is in the ring is asserted on every call.

    ring_fn(frames [n,h,w,3] uint8, area (y0, y1, x0, x1) in their pixels, cap, fed, n, groups) -> [len(groups), y1-y0, x1-x0, 3] uint8:
    the n frames are frames fed + 1 .. fed + n of the clip and are stored first; then for each group (frame numbers, rank) per byte
    element `rank` (0-based) of the named frames' values sorted ascending; at most INTERVAL_RING_MAX_GROUPS groups per call (more go
    in further calls with n = 0).  Default: EngineRingRanker on the shim's device.  `patches`: {rep: uint8 ndarray [ah, aw, 3]}, a
    plain dict as IntervalQuantile's, read back once per batch in which a subtitle ends."""

    def __init__(self, ring_fn=None, quantile=0.5, samples=15, trim_seconds=0.25, ring_seconds=60.0, batch=64):
        if not 0 <= quantile <= 1:
            raise ValueError(f"StreamingQuantile: quantile must be in [0, 1], not {quantile!r}")
        if samples < 1 or samples > INTERVAL_RANK_MAX:
            raise ValueError(f"StreamingQuantile: samples must be 1..{INTERVAL_RANK_MAX}, not {samples}: an interval is ranked in one "
                             f"group of at most {INTERVAL_RANK_MAX} frames")
        if not ring_seconds >= 0:
            raise ValueError(f"StreamingQuantile: ring_seconds must not be negative, not {ring_seconds!r}")
        self.ring_fn, self.quantile, self.samples, self.trim_seconds = ring_fn, quantile, int(samples), trim_seconds
        self.ring_seconds, self.batch = ring_seconds, int(batch)
        self.area = None              # the area in the band's own pixels (0, y1 - y0, x0, x1), once a batch has been seen
        self.patches = {}
        self.cap = self.peak_ring = None
        self.clamped = 0              # intervals of the last clip that reached back beyond the ring

    def begin(self, fps, lag):
        """A clip starts: its frame rate and the frames by which the selector's rows trail its frames."""
        if self.ring_fn is None:
            from . import shim
            self.ring_fn = EngineRingRanker(shim._context())
        self.fps, self.lag = fps, int(lag)
        self.trim = int(round(self.trim_seconds * fps))
        self.whole = int(round(self.ring_seconds * fps))          # R: trimmed ranges of up to R + 1 frames are certainly in the ring
        self.cap, self.peak_ring, self.clamped = self.whole + self.trim + self.lag + self.batch + 1, 0, 0
        self.patches = {}
        self._fed = 0                 # frames handed over (and stored) so far
        self._seen = 0                # tracker.fed after the last call: no interval that closes later ends before it

    def _samples(self, start, end, rep, oldest):
        """-> (the frames ranked for this interval, whether the ring cut them short)."""
        nos, _pos = fuse_samples(start, end, rep, self.fps, self.samples, self.trim_seconds)
        if nos[0] >= oldest:
            return nos, False
        first, last = trim_range(start, end, self.fps, self.trim_seconds)
        assert last - first + 1 > self.whole + 1 and oldest <= last, \
            f"StreamingQuantile: {start}..{end} (trimmed {first}..{last}) is not in the ring from {oldest}, cap {self.cap}"
        m = last - oldest + 1
        k = min(self.samples, m)
        return ([max(rep, oldest)] if k <= 1 else [oldest + (i * (m - 1)) // (k - 1) for i in range(k)]), True

    def __call__(self, data, area, n, tracker, closed):
        import numpy as np
        fed, after = self._fed, self._fed + n
        assert n <= self.batch, f"StreamingQuantile: a batch of {n} frames, the ring was sized for {self.batch}"
        assert after - tracker.fed <= self.lag or n == 0, \
            f"StreamingQuantile: the rows trail by {after - tracker.fed} frames, more than the lag {self.lag}"
        oldest = max(1, after - self.cap + 1)         # what the ring holds once this batch is stored: oldest .. after
        groups, reps = [], []
        for start, end, rep in closed:
            assert self._seen <= end <= after, f"StreamingQuantile: {start}..{end} closed after the rows up to {self._seen} had been seen"
            nos, cut = self._samples(start, end, rep, oldest)
            assert all(oldest <= f <= after for f in nos) and all(a < b for a, b in zip(nos, nos[1:])), \
                f"StreamingQuantile: the samples {nos} of {start}..{end} are not in the ring {oldest}..{after}"
            if cut:
                self.clamped += 1
                if self.clamped == 1:
                    import logging
                    logging.getLogger(__name__).warning(
                        "streaming quantile: the interval %d..%d reaches back beyond the ring of %d frames (ring_seconds=%s); its picture "
                        "is made of the frames %d..%d (its times are untouched; further such intervals are counted in clamped)",
                        start, end, self.cap, self.ring_seconds, nos[0], nos[-1])
            self.peak_ring = max(self.peak_ring, after - nos[0] + 1)
            groups.append((nos, quantile_rank(self.quantile, len(nos))))
            reps.append(rep)
        outs = []
        for k in range(0, max(len(groups), 1), INTERVAL_RING_MAX_GROUPS):
            part = groups[k:k + INTERVAL_RING_MAX_GROUPS]
            if k == 0 and (n or part):                    # the batch is stored by the first call
                res = self.ring_fn(data, area, self.cap, fed, n, part)
            elif part:
                res = self.ring_fn(data[:0], area, self.cap, after, 0, part)
            if part:
                outs.append(res)
        if outs:                                          # one read-back per batch in which a subtitle ends
            if hasattr(outs[0], "cpu"):
                import torch
                got = (outs[0] if len(outs) == 1 else torch.cat(outs)).cpu().numpy()
            else:
                got = np.concatenate([np.asarray(o) for o in outs])
            assert len(got) == len(reps)
            self.patches.update((rep, np.array(got[j])) for j, rep in enumerate(reps))      # (copies: a patch keeps no other alive)
        self.area, self._fed, self._seen = tuple(area), after, tracker.fed
