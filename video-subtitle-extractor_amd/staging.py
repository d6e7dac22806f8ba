"""Host -> HBM frame staging for the callers of the hot path (extractor.py, frame_select.py).

The reference hands one decoded frame at a time to paddle, which copies it to the device itself (ocr.py:27); its producer
thread (subtitle_ocr.py:163-208) only keeps the decoder busy while the consumer recognises.  A batched engine needs the
same overlap at batch granularity, and a 1080p batch is 400 MB: `np.stack` + a pageable copy costs more than the detector +
recogniser of the mobile models.  Here a batch is assembled ONCE, frame by frame, in a pinned slab (a small thread pool: numpy
releases the GIL while it copies), sent with one asynchronous copy on a copy stream, and the next batch is staged by a
producer thread while the current one is recognised (`prefetch`).

    up = Uploader(device)                         # torch.device / "cuda:0"
    for items, batch in prefetch(batches, up):    # batches: iterable of lists of (key, frame) with equal frame shapes
        dev = batch.tensor()                      # uint8 [n,H,W,3] on the device, ordered after the copy on the current stream
    for items, data in staged_batches(batches, up_or_none):     # the same, for a caller that also runs without an uploader:
        ...                                       # data is that device tensor, or np.stack of the frames when up_or_none is None

Frames that are still YUV 4:2:0 (ingest.Yuv420Frame, from a source's read_raw / raw_frames) are packed into the slab as they are — 1.5
bytes per pixel, half the slab copy and half the PCIe bytes of a BGR frame — and converted to BGR by one kernel on the copy stream
(vse_yuv420_to_bgr, or vse_yuv_to_bgr_matrix for frames that say matrix="bt709"), so a consumer sees the same uint8 [n,H,W,3] tensor
either way.  Frames of any other format (ingest.YuvFrame: 10-bit, 4:2:2, 4:4:4, grey, full range, P010) go the same way through
vse_yuv_to_bgr_format, keyed by shape, format, row parity and tone map (frames with an ingest.ToneMap, HDR material, convert through
vse_yuv_to_bgr_tonemap; the map's table is uploaded once per context).  Interlaced pictures (ingest.InterlacedYuvFrame) are uploaded as they are,
each beside its previous picture unless that is the frame before it in the batch, deinterlaced on the device (vse_yuv_deinterlace, or
vse_yuv_field_match for frames of mode "match") and
converted by the same call as the others.  Frames that carry an ingest.Resample (anamorphic video) are uploaded with their stored
columns and resampled to square pixels on the device (vse_yuv_resample) between those two steps; the batch key gains the resample.
Frames that carry an ingest.VScale (UHD and other oversized video) are uploaded as the band of stored rows that their output rows need
(YuvFrame.band()) and scaled down on the device first (vse_yuv_vscale): vertical, then horizontal, then the conversion, all on the copy
stream; the batch key gains the vscale and the first output row.
"""
import queue
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np


class StagedBatch:
    def __init__(self, dev, event):
        self._dev, self._event = dev, event

    def tensor(self):
        import torch
        cur = torch.cuda.current_stream(self._dev.device)
        cur.wait_event(self._event)
        self._dev.record_stream(cur)
        return self._dev


class Uploader:
    def __init__(self, device, depth=3, workers=4, ctx=None):
        """ctx: the engine.Context of `device` that converts YUV 4:2:0 batches (default: the shim's, obtained on the first such batch)."""
        import torch
        self.device = torch.device(device)
        self._ctx = ctx
        self.depth, self.workers = depth, workers
        self._slabs = [None] * depth            # pinned uint8 buffers, grown on demand
        self._busy = [None] * depth             # event of the last copy out of each slab
        self._k = 0
        self._stream = torch.cuda.Stream(device=self.device)
        self._pool = ThreadPoolExecutor(workers)
        self._lock = threading.Lock()

    def _slab(self, nbytes):
        import torch
        with self._lock:
            k = self._k
            self._k = (k + 1) % self.depth
        if self._busy[k] is not None:
            self._busy[k].synchronize()         # the copy that last read this slab has finished
        if self._slabs[k] is None or self._slabs[k].numel() < nbytes:
            self._slabs[k] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return k, self._slabs[k]

    def stage(self, frames):
        """list of equal-shaped uint8 frames (views are fine) -> StagedBatch"""
        import torch
        if hasattr(frames[0], "deinterlaced_planes"):
            return self._stage_interlaced(frames)
        if hasattr(frames[0], "fmt"):
            return self._stage_yuv(frames)
        if hasattr(frames[0], "pack_into"):
            return self._stage_yuv420(frames)
        shape = tuple(frames[0].shape)
        per = int(np.prod(shape))
        k, slab = self._slab(per * len(frames))
        host = slab[:per * len(frames)].view(len(frames), *shape)
        dst = host.numpy()
        list(self._pool.map(lambda i: np.copyto(dst[i], frames[i]), range(len(frames))))
        with torch.cuda.stream(self._stream):
            dev = torch.empty((len(frames),) + shape, dtype=torch.uint8, device=self.device)
            dev.copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._busy[k] = ev
        return StagedBatch(dev, ev)

    def _context(self):
        if self._ctx is None:
            from . import shim
            self._ctx = shim._context()
        if self.device.index is not None and self._ctx.tdev.index != self.device.index:
            raise ValueError(f"Uploader on {self.device} was given the engine context of {self._ctx.tdev}")
        return self._ctx

    def _stage_yuv420(self, frames):
        """Yuv420Frames of one shape, layout, row parity and matrix -> StagedBatch of their BGR conversion: packed into the slab (frame
        stride rounded up to 16 bytes, which the 16-byte kernel needs), one copy, one vse_yuv420_to_bgr (BT.601) or vse_yuv_to_bgr_matrix
        (BT.709) on the copy stream."""
        import torch
        first = frames[0]
        key = (tuple(first.shape), first.layout, first.row_parity, first.matrix)
        for f in frames:
            if not hasattr(f, "pack_into") or (tuple(f.shape), f.layout, f.row_parity, f.matrix) != key:
                raise ValueError("Uploader.stage: the YUV 4:2:0 frames of a batch must share shape, layout, row parity (y0 & 1) and matrix: "
                                 f"{key} and {(tuple(f.shape), getattr(f, 'layout', None), getattr(f, 'row_parity', None), getattr(f, 'matrix', None))}")
        ctx = self._context()
        n, (h, w, _) = len(frames), first.shape
        per = (first.packed_bytes + 15) & ~15
        k, slab = self._slab(per * n)
        host = slab[:per * n].view(n, per)
        dst = host.numpy()
        list(self._pool.map(lambda i: frames[i].pack_into(dst[i]), range(n)))
        with torch.cuda.stream(self._stream):
            # `packed` is allocated, filled and read on the copy stream alone: the caching allocator hands its block out again only to
            # this stream, behind the conversion, so it may be dropped here (`dev` crosses streams: StagedBatch.tensor records that)
            packed = torch.empty((n, per), dtype=torch.uint8, device=self.device)
            packed.copy_(host, non_blocking=True)
            dev = ctx.yuv420_to_bgr(packed, n, h, w, first.layout, first.row_parity, matrix=first.matrix)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._busy[k] = ev
        return StagedBatch(dev, ev)

    def _stage_yuv(self, frames):
        """ingest.YuvFrames of one shape, format, row parity, tone map and resample -> StagedBatch of their BGR conversion: packed into the
        slab as they are (3 bytes per pixel for 10-bit 4:2:0; frame stride rounded up to 16 bytes), one copy, with a resample one
        vse_yuv_resample, one vse_yuv_to_bgr_format (with a tone map: vse_yuv_to_bgr_tonemap) on the copy stream.  Frames with a vscale
        (shared too, as is their first output row) pack band(), and one vse_yuv_vscale runs in front of the others."""
        import torch
        first = frames[0]

        def key_of(f):
            key = (tuple(f.shape), getattr(f, "fmt", None), getattr(f, "row_parity", None), getattr(f, "tone", None), getattr(f, "resample", None))
            scale = getattr(f, "vscale", None)
            return key if scale is None else key + (scale, getattr(f, "y0", None))
        key = key_of(first)
        vscale = getattr(first, "vscale", None)
        for f in frames:
            if key_of(f) != key:
                raise ValueError("Uploader.stage: the YUV frames of a batch must share shape, format, row parity (y0 & sub_y), tone map and "
                                 f"resample{'' if vscale is None and getattr(f, 'vscale', None) is None else ', vscale and first row (y0)'}: "
                                 f"{key} and {key_of(f)}")
        ctx = self._context()
        n, (h, w, _) = len(frames), first.shape
        resample = getattr(first, "resample", None)
        parity = first.row_parity
        per = (first.packed_bytes + 15) & ~15
        k, slab = self._slab(per * n)
        host = slab[:per * n].view(n, per)
        dst = host.numpy()
        list(self._pool.map(lambda i: frames[i].pack_into(dst[i]), range(n)))
        with torch.cuda.stream(self._stream):
            packed = torch.empty((n, per), dtype=torch.uint8, device=self.device)          # (dropped here: see _stage_yuv420)
            packed.copy_(host, non_blocking=True)
            if vscale is not None:                     # vertical, then horizontal, then convert; the band becomes output rows y0:y1
                packed = ctx.yuv_vscale(packed, n, first.height, first.width, first.fmt, vscale, *first.band(), first.y0, first.y1)
                parity = first.y0 & first.fmt.sub_y
            if resample is not None:                   # (the resampled pictures are dropped here too)
                packed = ctx.yuv_resample(packed, n, h, first.width, first.fmt, resample, parity)
            dev = ctx.yuv_to_bgr(packed, n, h, w, first.fmt, parity, tone=first.tone)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._busy[k] = ev
        return StagedBatch(dev, ev)

    def _stage_interlaced(self, frames):
        """ingest.InterlacedYuvFrames of one shape, format, first row, field order, mode, threshold and tone map -> StagedBatch of the BGR conversion
        of their deinterlaced rows.  Each frame's band() (the rows asked for, widened so that every plane starts on a top-field row and the
        band's edge rows are none of those asked for) is packed into one slot of the slab; a frame whose prev is the planes of the frame
        before it in the batch takes that frame's slot as its previous picture, any other frame with a prev packs it into the slot in
        front of its own.  One copy; then one vse_yuv_deinterlace per run of frames whose slots are laid out alike (frames without prev:
        NULL; chained frames: the slot before, stride of one slot; frames with their prev beside them: stride of two; frames of mode
        "match", which share their comb threshold and limit too: vse_yuv_field_match in the same runs), one
        vse_yuv_to_bgr_format (with a tone map: vse_yuv_to_bgr_tonemap) over all the progressive bands, and the rows asked for cut out of it.
        Frames with a resample (shared too) get one vse_yuv_resample over all the progressive bands in front of the conversion."""
        import torch
        first = frames[0]

        def key_of(f):
            return (tuple(f.shape), getattr(f, "fmt", None), getattr(f, "y0", None), getattr(f, "height", None), getattr(f, "field_order", None),
                    getattr(f, "mode", None), getattr(f, "thresh", None), getattr(f, "tone", None), getattr(f, "comb_thresh", None),
                    getattr(f, "comb_limit", None), getattr(f, "resample", None))
        key = key_of(first)
        for f in frames:
            if not hasattr(f, "deinterlaced_planes") or key_of(f) != key:
                raise ValueError("Uploader.stage: the interlaced YUV frames of a batch must share shape, format, first row, picture height, "
                                 f"field order, mode, threshold, tone map, comb threshold, comb limit and resample: {key} and {key_of(f)}")
        from .ingest import _same_planes
        ctx = self._context()
        n, w = len(frames), first.width
        a, b = first.band()
        per = (first.band_bytes + 15) & ~15
        # runs: [kind, index of the first frame, slot of its picture, frames]; kind 0 no prev, 1 the slot before (stride 1), 2 pairs (stride 2)
        runs, jobs, slot = [], [], 0
        for i, f in enumerate(frames):
            if f.prev is None or f.mode == "interpolate":
                kind = 0
            elif i > 0 and _same_planes(f.prev, frames[i - 1].planes):
                kind = 1
            else:
                kind = 2
                jobs.append((slot, f, True))
                slot += 1
            if runs and runs[-1][0] == kind:
                runs[-1][3] += 1
            else:
                runs.append([kind, i, slot, 1])
            jobs.append((slot, f, False))
            slot += 1
        k, slab = self._slab(per * slot)
        host = slab[:per * slot].view(slot, per)
        dst = host.numpy()
        list(self._pool.map(lambda j: j[1].pack_band_into(dst[j[0]], prev=j[2]), jobs))
        with torch.cuda.stream(self._stream):
            packed = torch.empty((slot, per), dtype=torch.uint8, device=self.device)        # (dropped here, like prog: see _stage_yuv420)
            packed.copy_(host, non_blocking=True)
            prog = torch.empty((n, per), dtype=torch.uint8, device=self.device)
            stats = torch.empty((n, 4), dtype=torch.int32, device=self.device) if first.mode == "match" else None      # (dropped here too)
            for kind, i, at, count in runs:
                step = 2 if kind == 2 else 1
                cur = packed[at:].as_strided((count, per), (step * per, 1))
                before = None if kind == 0 else packed[at - 1]
                if first.mode == "match":
                    ctx.yuv_field_match(cur, count, b - a, w, first.fmt, prev=before, prev_stride=step * per, keep=first.keep,
                                        comb_thresh=first.comb_thresh, comb_limit=first.comb_limit, thresh=first.thresh, out=prog[i:i + count],
                                        stats=stats[i:i + count])
                    continue
                ctx.yuv_deinterlace(cur, count, b - a, w, first.fmt, prev=before, prev_stride=step * per,
                                    keep=first.keep, mode=first.mode, thresh=first.thresh, out=prog[i:i + count])
            if first.resample is not None:             # deinterlace or match, then resample over all the progressive bands, then convert
                prog, w = ctx.yuv_resample(prog, n, b - a, w, first.fmt, first.resample, 0), first.resample.out_width
            dev = ctx.yuv_to_bgr(prog, n, b - a, w, first.fmt, 0, tone=first.tone)
            if (first.y0 - a, first.y1 - a) != (0, b - a):
                dev = dev[:, first.y0 - a:first.y1 - a].contiguous()
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._busy[k] = ev
        return StagedBatch(dev, ev)

    def sibling(self):
        """Another Uploader on the same device and context, with slabs of its own: stage() hands its slabs out in turn and is meant for
        ONE producer thread; a second producer at the same time (one pass: the selector's bands and the recogniser's frames) takes this."""
        return Uploader(self.device, self.depth, self.workers, self._ctx)

    def bind_thread(self):
        """called once by a thread that is going to stage batches"""
        import torch
        torch.cuda.set_device(self.device)

    def close(self):
        self._pool.shutdown(wait=False)


def default_uploader():
    """An Uploader on the shim's device when there is a GPU, else None (callers then stack frames on the host)."""
    try:
        import torch
    except ImportError:
        return None
    if not torch.cuda.is_available():
        return None
    from . import shim
    return Uploader(shim._context().tdev)


_END = object()


def prefetch(batches, uploader, ahead=2):
    """Iterate (items, StagedBatch) while a producer thread reads + stages up to `ahead` batches in advance.  `batches` yields
    lists of (key, frame); an exception of the producer (a failing decoder) is re-raised in the consumer."""
    q = queue.Queue(maxsize=max(1, ahead))
    stop = threading.Event()

    def produce():
        try:
            uploader.bind_thread()
            for items in batches:
                if stop.is_set():
                    return
                q.put((items, uploader.stage([f for _, f in items])))
            q.put(_END)
        except BaseException as e:             # noqa: BLE001 - handed to the consumer
            q.put(e)

    th = threading.Thread(target=produce, daemon=True)
    th.start()
    try:
        while True:
            got = q.get()
            if got is _END:
                break
            if isinstance(got, BaseException):
                raise got
            yield got
    finally:
        stop.set()
        while th.is_alive():                   # unblock a producer waiting on a full queue
            try:
                q.get_nowait()
            except queue.Empty:
                th.join(0.01)


def staged_batches(batches, uploader):
    """Iterate (items, data) over `batches` (lists of (key, frame)) for a consumer that takes its frames stacked: with an uploader
    `data` is the device tensor of `prefetch`'s StagedBatch, without one np.stack of the frames on the host.  Closing the generator
    closes `prefetch`, which stops its producer thread."""
    if uploader is None:
        for items in batches:
            yield items, np.stack([np.asarray(f) for _, f in items])
        return
    staged = prefetch(batches, uploader)
    try:
        for items, sb in staged:
            yield items, sb.tensor()
    finally:
        staged.close()
