"""Timeline sync: shift a subtitle script made for one release onto another release's audio (the reference GUI's "Timeline Sync"
tab, ui/timeline_sync_interface.py:156-172, which runs the bundled Sushi, backend/sushi/).

A restatement of Sushi's WAV path with its numbers: the same uint8 streams, search windows, grouping, smoothing and averaging,
so a script comes out byte for byte as Sushi writes it.  The one hot step, the template search of a group's source audio in a
window of the destination audio (WavStream.find_substream, backend/sushi/wav.py:179-189), runs on the GPU
(vse_audio_match, csrc/audio_match.hip); the three searches of one step of the loop go to the device as one call.

Sushi's second half is here too: shifted lines snap to scene cuts ("keyframes") of both releases, so a subtitle starts on the cut
it started on in the source (snap_groups_to_keyframes and what it calls, with the same float operations in the same order).
Keyframes come as files in Sushi's format or as lists of frame numbers, frame times from a constant fps or a timecodes file (v1 /
v2); `python -m vse_amd.keyframes` finds a video's cuts on the GPU and writes such a file.

Inputs are WAV files only: the project has no demuxer, so chapters, stream selection and keyframes made on the fly stay out.

    python -m vse_amd.timeline_sync --src a.wav --dst b.wav --script in.srt --output out.srt [--stream-build device]
        [--src-keyframes a.kf.txt --dst-keyframes b.kf.txt --src-fps 23.976 --dst-fps 23.976]
"""
import argparse
import bisect
import logging
import math
import os
import re
import struct
import sys
from itertools import chain, takewhile

import numpy as np

log = logging.getLogger("vse_amd.timeline_sync")

ALLOWED_ERROR = 0.01
PADDING_SECONDS = 10
SMALL_WINDOW = 1.5


class TimelineSyncError(Exception):
    """A refused input or option (the CLI exits with status 2, as Sushi does on SushiError)."""


# ---- WAV -> uint8 stream (backend/sushi/wav.py:17-165) ----------------------------------------------------------------------

WAVE_FORMAT_PCM = 0x0001
WAVE_FORMAT_EXTENSIBLE = 0xFFFE


def _read_wav_header(f, path):
    """-> (channels, framerate, sample_width, frames_count); the file is left at the first data byte."""
    def chunk_header():
        h = f.read(8)
        if len(h) < 8:
            return None, 0
        return h[:4], struct.unpack("<I", h[4:])[0]

    name, _ = chunk_header()
    if name != b"RIFF":
        raise TimelineSyncError(f"{path}: file does not start with RIFF id")
    if f.read(4) != b"WAVE":
        raise TimelineSyncError(f"{path}: not a WAVE file")
    fmt = None
    while True:
        name, size = chunk_header()
        if name is None:
            break
        if name == b"fmt ":
            body = f.read(size)
            if len(body) < 16:
                raise TimelineSyncError(f"{path}: truncated fmt chunk")
            tag, channels, rate, _, _ = struct.unpack("<HHLLH", body[:14])
            if tag not in (WAVE_FORMAT_PCM, WAVE_FORMAT_EXTENSIBLE):
                raise TimelineSyncError(f"{path}: unknown format: {tag}")
            bits = struct.unpack("<H", body[14:16])[0]
            fmt = (channels, rate, (bits + 7) // 8)
            if size & 1:
                f.read(1)
        elif name == b"data":
            if fmt is None:
                raise TimelineSyncError(f"{path}: invalid WAV file (data before fmt)")
            channels, rate, width = fmt
            if width != 2:
                raise TimelineSyncError(f"{path}: {8 * width}-bit samples are not supported (16-bit PCM only)")
            if channels < 1 or rate < 1:
                raise TimelineSyncError(f"{path}: invalid fmt chunk ({channels} channels, {rate} Hz)")
            file_size = os.path.getsize(path)
            if file_size > 0xFFFFFFFF:             # a large broken WAV: the data runs to the end of the file
                frames = (file_size - f.tell()) // (channels * width)
            else:
                frames = size // (channels * width)
            return channels, rate, width, frames
        else:
            f.seek(size + (size & 1), 1)
    raise TimelineSyncError(f"{path}: invalid WAV file")


def _downmix(raw, channels):
    """int16 interleaved bytes -> float32 mono: channels summed left to right, then divided by their count."""
    x = np.frombuffer(raw, dtype=np.int16).astype("float32")
    if channels == 1:
        return x
    n = len(x) // channels
    out = x[0::channels][:n]
    for c in range(1, channels):
        out = out[:n] + x[c::channels][:n]
    out /= float(channels)
    return out


def _resize_nearest(x, new_length):
    """Nearest-neighbour resampling with cv2.resize's INTER_NEAREST index rule: src index = min(floor(j / (dst / src)), src - 1)."""
    src = len(x)
    scale = 1.0 / (new_length / src)
    idx = np.minimum(np.floor(np.arange(new_length) * scale).astype(np.int64), src - 1)
    return x[idx]


class AudioStream:
    """A WAV file as Sushi's uint8 search stream: downmixed, resampled per second to `sample_rate`, padded with 10 s of the
    FILE's rate on each side, clipped to 3x the medians of its non-negative and non-positive samples, scaled to 0..255."""

    def __init__(self, path, sample_rate=12000):
        with open(path, "rb") as f:
            channels, framerate, width, frames = _read_wav_header(f, path)
            if framerate < sample_rate:
                raise TimelineSyncError(f"{path}: the sample rate {framerate} Hz is below the search rate {sample_rate} Hz")
            total_seconds = frames / float(framerate)
            rate_ratio = sample_rate / float(framerate)
            self.sample_rate = sample_rate
            self.sample_count = math.ceil(total_seconds * sample_rate)
            self.padding_size = 10 * framerate
            # zero-filled, so a sample no chunk writes (the lengths can sum to one short) holds 0.0
            data = np.zeros(int(PADDING_SECONDS * 2 * framerate + self.sample_count), np.float32)
            seconds_read = 0
            at = self.padding_size
            while seconds_read < total_seconds:
                chunk = _downmix(f.read(framerate * channels * width), channels)
                new_length = int(round(len(chunk) * rate_ratio))
                if rate_ratio != 1:
                    if new_length == 0:     # as cv2.resize, which refuses an empty size
                        raise TimelineSyncError(f"{path}: the last {len(chunk)} frames are too few to resample")
                    chunk = _resize_nearest(chunk, new_length)
                dst = data[at:at + new_length]
                if len(dst) != len(chunk):
                    raise TimelineSyncError(f"{path}: the data chunk does not match its length")
                dst[:] = chunk
                at += new_length
                seconds_read += 1
        data[0:self.padding_size] = data[self.padding_size]
        data[-self.padding_size:] = data[-self.padding_size - 1]
        hi = np.median(data[data >= 0], overwrite_input=True) * 3
        lo = np.median(data[data <= 0], overwrite_input=True) * 3
        if not (np.isfinite(hi) and np.isfinite(lo)) or hi - lo == 0:
            raise TimelineSyncError(f"{path}: the audio is (almost) all silence; its level range is empty")
        np.clip(data, lo, hi, out=data)
        data -= lo
        data /= (hi - lo)
        data *= 255.0
        data += 0.5
        self.data = data.astype("uint8")

    @property
    def duration_seconds(self):
        return self.sample_count / self.sample_rate

    def sample_for_time(self, t):
        return int(self.sample_rate * t) + self.padding_size

    def substream(self, start, end):
        """(offset, length) of data[sample(start):sample(end)], with Python's slice rules."""
        s, e, _ = slice(self.sample_for_time(start), self.sample_for_time(end)).indices(len(self.data))
        return s, max(e - s, 0)

    def window(self, center, size, m):
        """Search window of a pattern of m samples around `center` s, +-size s -> (start time, offset, length)."""
        start_time = max(min(center - size, self.duration_seconds), -PADDING_SECONDS)
        end_time = max(min(center + size, self.duration_seconds + PADDING_SECONDS), 0)
        s, e, _ = slice(self.sample_for_time(start_time), self.sample_for_time(end_time) + m).indices(len(self.data))
        return start_time, s, max(e - s, 0)


# ---- WAV -> uint8 stream on the device (include/vse_hip.h, the vse_audio_stream_* section) ---------------------------------------

PIECE_BYTES = 64 << 20         # PCM bytes per staging buffer, at most (a second that is larger goes alone)
MAX_DEVICE_CHANNELS = 8


class _GpuStreamBuild:
    """The product `build` of DeviceAudioStream: feed(pcm int16 [n, C], first_second) copies the piece into one of two pinned
    buffers, uploads it and gathers it on the current stream while the host fills the other buffer; finish() counts, selects and
    writes the stream, and reads the result record back (the one wait for the device)."""

    def __init__(self, ctx, frames, channels, rate, sample_rate):
        self.ctx = ctx
        self.args = (frames, channels, rate, sample_rate)
        self.ws = ctx.audio_stream_workspace(*self.args)
        self.slabs = [None, None]        # (pinned int16, device int16, event recorded behind the upload that reads the pinned one)
        self.turn = 0

    def feed(self, pcm, first_second):
        t = self.ctx.torch
        n = int(pcm.shape[0]) * int(pcm.shape[1])
        i, self.turn = self.turn, self.turn ^ 1
        slab = self.slabs[i]
        if slab is not None:
            slab[2].synchronize()        # the upload out of this pinned buffer is done
        if slab is None or slab[0].numel() < n:
            slab = self.slabs[i] = (t.empty(n, dtype=t.int16, pin_memory=True), t.empty(n, dtype=t.int16, device=self.ctx.tdev),
                                    t.cuda.Event())
        host, dev, event = slab
        host.numpy()[:n] = np.asarray(pcm).reshape(-1)
        dev[:n].copy_(host[:n], non_blocking=True)
        event.record()
        self.ctx.audio_stream_feed(dev[:n], first_second, *self.args, self.ws)

    def finish(self):
        out, record = self.ctx.audio_stream_finish(*self.args, self.ws)
        r = record.cpu().numpy()
        lo, hi = r[:2].copy().view(np.float32)
        status = int(r[4])
        return (out if status == 0 else None), lo, hi, int(r[2]), int(r[3]), status


class DeviceAudioStream(AudioStream):
    """AudioStream built on the device: the WAV's PCM is memory-mapped, fed in pieces of whole seconds and turned into the same
    uint8 stream there, so `data` is a cuda uint8 tensor that GpuSearch takes as it is.  `levels` = (lo, hi), the float32 clip
    levels.  build(frames, channels, rate, sample_rate) -> an object with feed(pcm int16 [n, C], first_second) and finish() ->
    (stream, lo, hi, size of the >= 0 set, size of the <= 0 set, status); None: the device one on `ctx`.  A file the device path
    does not take (a data chunk shorter than its header claims, more than 8 channels, more than 4 GiB, no frame, a stream of
    2^31 elements or more) goes through AudioStream itself: `data` is then its host array and `levels` is None.
    piece_seconds: seconds per piece (None: what fits PIECE_BYTES); piece_order: a function of the list of pieces' first seconds
    that returns the order to feed them in."""

    def __init__(self, path, sample_rate=12000, ctx=None, build=None, *, piece_seconds=None, piece_order=None):
        with open(path, "rb") as f:
            channels, framerate, width, frames = _read_wav_header(f, path)
            offset = f.tell()
        if framerate < sample_rate:
            raise TimelineSyncError(f"{path}: the sample rate {framerate} Hz is below the search rate {sample_rate} Hz")
        file_size = os.path.getsize(path)
        why = None
        if channels > MAX_DEVICE_CHANNELS:
            why = f"{channels} channels"
        elif file_size > 0xFFFFFFFF:
            why = "a file over 4 GiB"
        elif file_size - offset < frames * channels * width:
            why = "a data chunk shorter than its header claims"
        elif frames < 1:
            why = "no audio frame"
        elif 2 * PADDING_SECONDS * framerate + math.ceil(frames / float(framerate) * sample_rate) > 2 ** 31 - 1:
            why = "a stream of 2^31 elements or more"
        self.levels = None
        if why is not None:
            log.info("%s: %s, the stream is built on the host", path, why)
            super().__init__(path, sample_rate)
            return
        self.sample_rate = sample_rate
        self.sample_count = math.ceil(frames / float(framerate) * sample_rate)
        self.padding_size = 10 * framerate
        seconds = -(-frames // framerate)
        last = frames - (seconds - 1) * framerate
        if sample_rate != framerate and int(round(last * (sample_rate / float(framerate)))) == 0:
            raise TimelineSyncError(f"{path}: the last {last} frames are too few to resample")
        if build is None:
            if ctx is None:
                from . import engine
                ctx = engine.Context(0)
            build = lambda *a: _GpuStreamBuild(ctx, *a)           # noqa: E731
        builder = build(frames, channels, framerate, sample_rate)
        if piece_seconds is None:
            piece_seconds = max(PIECE_BYTES // (framerate * channels * width), 1)
        pcm = np.memmap(path, dtype="<i2", mode="r", offset=offset, shape=(frames, channels))
        firsts = list(range(0, seconds, piece_seconds))
        for first in (piece_order(firsts) if piece_order else firsts):
            builder.feed(pcm[first * framerate:(first + piece_seconds) * framerate], first)
        del pcm
        data, lo, hi, _, _, status = builder.finish()
        if status != 0:
            raise TimelineSyncError(f"{path}: the audio is (almost) all silence; its level range is empty")
        self.data = data
        self.levels = (np.float32(lo), np.float32(hi))


# ---- searchers --------------------------------------------------------------------------------------------------------------

class GpuSearch:
    """The product searcher: load(src, dst) uploads both uint8 streams once (a cuda uint8 tensor, DeviceAudioStream's, is taken as it
    is); __call__([(src_off, m, dst_off, win_len)] * 1..3) -> [(first argmin offset, float32 value)] from one vse_audio_match call
    (a grown workspace is reused)."""

    def __init__(self, ctx=None):
        if ctx is None:
            from . import engine
            ctx = engine.Context(0)
        self.ctx = ctx
        self.ws = None

    def load(self, src, dst):
        t = self.ctx.torch

        def device(x):
            if isinstance(x, t.Tensor) and x.is_cuda and x.dtype == t.uint8 and x.is_contiguous():
                return x
            return t.from_numpy(np.ascontiguousarray(x, np.uint8)).to(self.ctx.tdev)

        self.src, self.dst = device(src), device(dst)

    def __call__(self, queries):
        need = self.ctx.audio_match_workspace_bytes(queries)
        if self.ws is None or self.ws.numel() < need:
            self.ws = self.ctx.torch.empty(max(need, 256), dtype=self.ctx.torch.uint8, device=self.ctx.tdev)
        out = self.ctx.audio_match(self.src, self.dst, queries, workspace=self.ws).cpu().numpy()
        vals = out[:, 1].copy().view(np.float32)
        return [(int(k), vals[i]) for i, k in enumerate(out[:, 0])]


class _Searcher:
    """Sushi's find_substream over a searcher; every search is appended to `log` as (src_off, m, dst_off, win_len, index, value)."""

    def __init__(self, search, src, dst):
        self.search, self.src, self.dst = search, src, dst
        self.log = []
        search.load(src.data, dst.data)

    def find(self, pattern, centers, size):
        """pattern: [(src_off, m)], centers: their window centres (s) -> [(diff float32, time s)], one device call."""
        queries, starts = [], []
        for (so, m), c in zip(pattern, centers):
            if m < 1:
                raise TimelineSyncError("a search group holds no audio samples")
            start_time, do, wl = self.dst.window(c, size, m)
            if wl < m:
                raise TimelineSyncError("a search window is shorter than its group's audio")
            queries.append((so, m, do, wl))
            starts.append(start_time)
        res = self.search(queries)
        out = []
        for q, st, (idx, val) in zip(queries, starts, res):
            val = np.float32(val)
            self.log.append((*q, int(idx), val))
            out.append((val, st + (idx / float(self.dst.sample_rate))))
        return out


# ---- scripts (backend/sushi/subs.py, common.py:23-39) --------------------------------------------------------------------------

def format_srt_time(seconds):
    ms = round(seconds * 1000)
    return "{0:02d}:{1:02d}:{2:02d},{3:03d}".format(int(ms // 3600000), int((ms // 60000) % 60), int((ms // 1000) % 60), int(ms % 1000))


def format_time(seconds):
    cs = round(seconds * 100)
    return "{0}:{1:02d}:{2:02d}.{3:02d}".format(int(cs // 360000), int((cs // 6000) % 60), int((cs // 100) % 60), int(cs % 100))


def _parse_time(s):
    h, m, sec = map(float, s.split(":"))
    return h * 3600 + m * 60 + sec


class Event:
    """One script line with Sushi's shift state: a linked event takes its shift and diff from the event it links to."""
    is_comment = False

    def __init__(self, index, start, end, text):
        self.source_index, self.start, self.end, self.text = index, start, end, text
        self._shift, self._diff, self._link = 0, 1, None
        self._start_shift = self._end_shift = 0

    @property
    def linked(self):
        return self._link is not None

    @property
    def shift(self):
        return self._link.shift if self.linked else self._shift

    @property
    def diff(self):
        return self._link.diff if self.linked else self._diff

    @property
    def duration(self):
        return self.end - self.start

    def set_shift(self, shift, diff):
        assert not self.linked
        self._shift, self._diff = shift, diff

    def chain_end(self):
        return self._link.chain_end() if self.linked else self

    def link_event(self, other):
        assert other.chain_end() is not self, "circular link"
        self._link = other

    def resolve_link(self):
        assert self.linked
        self._shift, self._diff = self._link.shift, self._link.diff
        self._link = None

    def adjust_shift(self, value):
        assert not self.linked
        self._shift += value

    def adjust_additional_shifts(self, start_shift, end_shift):
        assert not self.linked
        self._start_shift += start_shift
        self._end_shift += end_shift

    @property
    def shifted_start(self):
        return self.start + self.shift + self._start_shift

    @property
    def shifted_end(self):
        return self.end + self.shift + self._end_shift

    def apply_shift(self):
        self.start, self.end = self.shifted_start, self.shifted_end


_SRT_TIME = r"\d{1,2}:\d{1,2}:\d{1,2},\d+"
_SRT_EVENT = re.compile(r"(\d+?)\s+?(" + _SRT_TIME + r")\s-->\s(" + _SRT_TIME + r").(.+?)(?=(?:\d+?\s+?" + _SRT_TIME + r"\s-->\s" +
                        _SRT_TIME + r")|$)", re.DOTALL)


def _read_utf8(path):
    try:
        with open(path, "rb") as f:
            raw = f.read()
    except OSError:
        raise TimelineSyncError(f"Script {path} not found")
    try:
        return raw.decode("utf-8-sig")
    except UnicodeDecodeError:
        raise TimelineSyncError(f"{path}: only UTF-8 scripts (with or without a BOM) are supported")


class SrtEvent(Event):
    def __str__(self):
        return f"{self.source_index}\n{format_srt_time(self.start)} --> {format_srt_time(self.end)}\n{self.text}"


class SrtScript:
    def __init__(self, events):
        self.events = events

    @classmethod
    def from_file(cls, path):
        return cls.from_text(_read_utf8(path))

    @classmethod
    def from_text(cls, text):
        return cls([SrtEvent(int(m.group(1)), _parse_time(m.group(2).replace(",", ".")), _parse_time(m.group(3).replace(",", ".")),
                             m.group(4).strip()) for m in _SRT_EVENT.finditer(text)])

    def to_text(self):
        return "\n\n".join(map(str, self.events))

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.to_text().encode("utf-8"))


class AssEvent(Event):
    def __init__(self, line, position):
        kind, _, rest = line.partition(":")
        f = [x.strip() for x in rest.split(",", 9)]
        super().__init__(position, _parse_time(f[1]), _parse_time(f[2]), f[9])
        self.kind = kind
        self.is_comment = kind.lower() == "comment"
        self.layer, self.style, self.name = f[0], f[3], f[4]
        self.margins = f[5:8]
        self.effect = f[8]

    def __str__(self):
        return "{0}: {1},{2},{3},{4},{5},{6},{7},{8},{9},{10}".format(self.kind, self.layer, format_time(self.start), format_time(self.end),
                                                                      self.style, self.name, *self.margins, self.effect, self.text)


ASS_STYLE_FORMAT = ("Format: Name, Fontname, Fontsize, PrimaryColour, SecondaryColour, OutlineColour, BackColour, Bold, Italic, "
                    "Underline, StrikeOut, ScaleX, ScaleY, Spacing, Angle, BorderStyle, Outline, Shadow, Alignment, MarginL, MarginR, "
                    "MarginV, Encoding")
ASS_EVENT_FORMAT = "Format: Layer, Start, End, Style, Name, MarginL, MarginR, MarginV, Effect, Text"


class AssScript:
    def __init__(self, info, styles, events, other):
        self.info, self.styles, self.events, self.other = info, styles, events, other

    @classmethod
    def from_file(cls, path):
        return cls.from_text(_read_utf8(path))

    @classmethod
    def from_text(cls, text):
        info, styles, events, other = [], [], [], {}
        target = None
        for no, line in enumerate(text.splitlines()):
            line = line.strip()
            if not line:
                continue
            low = line.lower()
            if low == "[script info]":
                target = info
            elif low == "[v4+ styles]":
                target = styles
            elif low == "[events]":
                target = events
            elif re.match(r"\[.+?\]", low):
                if line in other:
                    raise TimelineSyncError("Duplicate section detected, invalid script?")
                target = other[line] = []
            elif target is None:
                raise TimelineSyncError("That's some invalid ASS script")
            elif target is events:
                if not line.startswith("Format:"):
                    try:
                        events.append(AssEvent(line, len(events) + 1))
                    except (IndexError, ValueError) as e:
                        raise TimelineSyncError(f"That's some invalid ASS script: {e} [line {no}]")
            elif target is info or target is styles:
                if not line.startswith("Format:"):
                    target.append(line)
            else:
                target.append(line)
        return cls(info, styles, events, other)

    def to_text(self):
        lines = []
        if self.info:
            lines += ["[Script Info]", *self.info, ""]
        if self.styles:
            lines += ["[V4+ Styles]", ASS_STYLE_FORMAT, *self.styles, ""]
        if self.events:
            lines += ["[Events]", ASS_EVENT_FORMAT, *map(str, sorted(self.events, key=lambda e: e.source_index))]
        for name, body in self.other.items():
            lines += ["", name, *body]
        return os.linesep.join(lines)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.to_text().encode("utf-8-sig"))


# ---- the algorithm (backend/sushi/__init__.py) -----------------------------------------------------------------------------------

def running_median(values, window_size):
    if window_size % 2 != 1:
        raise TimelineSyncError("Median window size should be odd")
    half = window_size // 2
    n = len(values)
    out = []
    for i in range(n):
        r = min(half, i, n - i - 1)
        out.append(np.median(values[i - r:i + r + 1]))
    return out


def smooth_events(events, radius):
    if not radius:
        return
    smoothed = running_median([e.shift for e in events], radius * 2 + 1)
    for e, s in zip(events, smoothed):
        e.set_shift(s, e.diff)


def detect_groups(events):
    it = iter(events)
    groups = [[next(it)]]
    for e in it:
        if abs(e.shift - groups[-1][-1].shift) > ALLOWED_ERROR:
            groups.append([])
        groups[-1].append(e)
    return groups


def fix_near_borders(events):
    """Lines at either end whose diff is off by more than 5x (or below 1/5) of the typical diff take the shift of the first good
    line after them."""
    def fix_border(seq, median_diff):
        first_ten = np.median([x.diff for x in seq[:10]], overwrite_input=True)
        limit = min(first_ten, median_diff)
        broken = []
        for e in seq:
            if not 0.2 < (e.diff / limit) < 5:
                broken.append(e)
            else:
                for x in broken:
                    x.link_event(e)
                return len(broken)
        return 0

    median_diff = np.median([x.diff for x in events], overwrite_input=True)
    if fix_border(events, median_diff):
        log.info("fixed border events after %s", format_time(events[0].start))
    if fix_border(list(reversed(events)), median_diff):
        log.info("fixed border events before %s", format_time(events[-1].end))


def average_shifts(events):
    events = [e for e in events if not e.linked]
    shifts = [e.shift for e in events]
    weights = [1 - e.diff for e in events]
    avg = np.average(shifts, weights=weights)
    for e in events:
        e.set_shift(avg, e.diff)
    return avg


def merge_short_lines_into_groups(events, chapter_times, max_ts_duration, max_ts_distance):
    groups = []
    chapters = iter(chapter_times[1:] + [100000000])
    next_chapter = next(chapters)
    events = list(events)
    done = set()
    for i, e in enumerate(events):
        if i in done:
            continue
        while e.end > next_chapter:
            next_chapter = next(chapters)
        if e.duration > max_ts_duration:
            groups.append([e])
            done.add(i)
            continue
        group, group_end = [e], e.end
        j = i + 1
        while j < len(events) and abs(group_end - events[j].start) < max_ts_distance:
            if events[j].end < next_chapter and events[j].duration <= max_ts_duration:
                done.add(j)
                group.append(events[j])
                group_end = max(group_end, events[j].end)
            j += 1
        groups.append(group)
    return groups


def prepare_search_groups(events, source_duration, chapter_times, max_ts_duration, max_ts_distance):
    last_unlinked = None
    for i, e in enumerate(events):
        if e.is_comment:
            e.link_event(events[i + 1] if i + 1 < len(events) else last_unlinked)
            continue
        if (e.start + e.duration / 2.0) > source_duration:
            log.info("event outside of the audio range, ignored: %s", format_time(e.start))
            e.link_event(last_unlinked)
            continue
        if e.end == e.start:
            e.link_event(events[i + 1] if i + 1 < len(events) else last_unlinked)
            continue
        same = next((x for x in takewhile(lambda x: e.start == x.start, reversed(events[:i])) if not x.linked and x.end == e.end), None)
        if same:
            e.link_event(same)
        else:
            last_unlinked = e

    groups = merge_short_lines_into_groups((e for e in events if not e.linked), chapter_times, max_ts_duration, max_ts_distance)
    passed = []
    for i, g in enumerate(groups):
        outer = next((x for x in reversed(groups[:i]) if x[0].start <= g[0].start and x[-1].end >= g[-1].end), None)
        if outer is None:
            passed.append(g)
        else:
            for e in g:
                e.link_event(outer[0])
    return passed


def calculate_shifts(searcher, src, dst, groups, normal_window, max_window, rewind_thresh):
    """Sushi's search loop: a small window around the last committed shift first; otherwise the whole group and its two halves
    (one device call), from the last committed and, if that fails, from the last uncommitted shift; rewind to `max_window`
    after `rewind_thresh` uncommitted groups."""
    idx = 0
    committed, uncommitted = [], []
    window = normal_window
    while idx < len(groups):
        g = groups[idx]
        so, m = src.substream(g[0].start, g[-1].end)
        original = g[0].start
        state = {"start_time": g[0].start, "end_time": g[-1].end, "shift": None, "diff": None}
        last = committed[-1]["shift"] if committed else 0
        diff = new_time = None

        if not uncommitted:
            if original + last > dst.duration_seconds:
                for h in groups[idx:]:
                    committed.append({"start_time": h[0].start, "end_time": h[-1].end, "shift": None, "diff": None})
                break
            if SMALL_WINDOW < window:
                diff, new_time = searcher.find([(so, m)], [original + last], SMALL_WINDOW)[0]
            if new_time is not None and abs((new_time - original) - last) <= ALLOWED_ERROR:
                state.update({"shift": new_time - original, "diff": diff})
                committed.append(state)
                window = normal_window
                idx += 1
                continue

        half = m // 2
        right_offset = half / float(src.sample_rate)
        parts = [(so, m), (so, half), (so + half, m - half)]
        terminate = False

        def step(offset):
            (d, t), (_, lt), (_, rt) = searcher.find(parts, [original + offset, original + offset, original + offset + right_offset], window)
            rt -= right_offset
            return d, t, abs(lt - rt) <= ALLOWED_ERROR and abs(t - lt) <= ALLOWED_ERROR

        if original + last < dst.duration_seconds:
            diff, new_time, terminate = step(last)
        if not terminate and uncommitted and uncommitted[-1]["shift"] is not None and \
                original + uncommitted[-1]["shift"] < dst.duration_seconds:
            diff, new_time, terminate = step(uncommitted[-1]["shift"])

        shift = new_time - original
        if not terminate:
            state.update({"shift": shift, "diff": diff})
            uncommitted.append(state)
            idx += 1
            if rewind_thresh == len(uncommitted) and window < max_window:
                log.warning("possibly broken segment from %s: window %s -> %s", format_time(uncommitted[0]["start_time"]), window, max_window)
                window = max_window
                idx = len(committed)
                del uncommitted[:]
            continue
        if uncommitted:
            log.warning("events from %s to %s will most likely be broken", format_time(uncommitted[0]["start_time"]),
                        format_time(uncommitted[-1]["end_time"]))
        uncommitted.append(state)
        for s in uncommitted:
            s.update({"shift": shift, "diff": diff})
        committed.extend(uncommitted)
        del uncommitted[:]
        idx += 1

    for i, (g, s) in enumerate(zip(groups, chain(committed, uncommitted))):
        if s["shift"] is None:
            for prev in reversed(groups[:i]):
                to = next((x for x in reversed(prev) if not x.linked), None)
                if to:
                    for e in g:
                        e.link_event(to)
                    break
        else:
            for e in g:
                e.set_shift(s["shift"], s["diff"])


# ---- frame times (backend/sushi/demux.py:138-227) ---------------------------------------------------------------------------------

class CfrTimecodes:
    """Constant frame rate: frame n starts at n * (1 / fps)."""

    def __init__(self, fps):
        self.frame_duration = 1.0 / fps

    def get_frame_time(self, number):
        return number * self.frame_duration

    def get_frame_size(self, timestamp):
        return self.frame_duration

    def get_frame_number(self, timestamp):
        return int(timestamp / self.frame_duration)


class Timecodes:
    """Frame start times from a timecodes file.  v2 lists every frame's time in ms and has no default rate: a frame past the list
    takes the last time.  v1 gives a default fps and `first,last,fps` overrides: the list covers the frames up to the last
    override (empty without overrides) and the default rate continues it."""

    def __init__(self, times, default_fps):
        self.times = times
        self.default_frame_duration = 1.0 / default_fps if default_fps else None

    def get_frame_time(self, number):
        if -len(self.times) <= number < len(self.times):
            return self.times[number]          # (a negative number counts from the end, as it does in Sushi's list lookup)
        if not self.default_frame_duration:
            if not self.times:
                raise TimelineSyncError("The timecodes file lists no frame")
            return self.times[-1]
        if self.times:
            return self.times[-1] + self.default_frame_duration * (number - len(self.times) + 1)
        return number * self.default_frame_duration

    def get_frame_number(self, timestamp):
        if (not self.times or self.times[-1] < timestamp) and self.default_frame_duration:
            return int((timestamp - sum(self.times)) / self.default_frame_duration)         # (the sum is Sushi's)
        return bisect.bisect_left(self.times, timestamp)

    def get_frame_size(self, timestamp):
        number = bisect.bisect_left(self.times, timestamp)
        c = self.get_frame_time(number)
        if number == len(self.times):
            return c - self.get_frame_time(number - 1)
        return self.get_frame_time(number + 1) - c

    @classmethod
    def cfr(cls, fps):
        return CfrTimecodes(fps)

    @classmethod
    def parse(cls, text):
        lines = text.splitlines()
        first = lines[0].lower().lstrip() if lines else ""
        try:
            if first.startswith("# timecode format v2") or first.startswith("# timestamp format v2"):
                return cls([float(x) / 1000.0 for x in lines[1:]], None)
            if first.startswith("# timecode format v1"):
                default = float(lines[1].lower().replace("assume ", ""))
                overrides = [(int(x[0]), int(x[1]), float(x[2])) for x in (ln.split(",") for ln in lines[2:])]
                times = []
                if overrides:
                    fps = [default] * (overrides[-1][1] + 1)
                    for a, b, f in overrides:
                        fps[a:b + 1] = [f] * (b - a + 1)
                    times = [0]
                    for d in (1.0 / f for f in fps):
                        times.append(times[-1] + d)
                return cls(times, default)
        except (ValueError, IndexError) as e:
            raise TimelineSyncError(f"Malformed timecodes file: {e}")
        raise TimelineSyncError("This timecodes format is not supported")

    @classmethod
    def from_file(cls, path):
        try:
            with open(path) as f:
                return cls.parse(f.read())
        except OSError:
            raise TimelineSyncError(f"Timecodes file {path} not found")


# ---- keyframe snapping (backend/sushi/__init__.py:33-56, 180-268) --------------------------------------------------------------------

def interpolate_nones(data, points):
    """The None entries of `data` take the value interpolated linearly over `points` from the entries that have one; [] when none
    has."""
    known = {p: v for p, v in zip(points, data) if v is not None}
    if not known:
        return []
    missing = {p for p, v in zip(points, data) if v is None}
    if not missing:
        return data
    table = sorted(known.items())
    missing = sorted(x for x in missing if x not in known)
    known.update(zip(missing, np.interp(x=missing, xp=[p for p, _ in table], fp=[v for _, v in table])))
    return [known[p] if v is None else v for p, v in zip(points, data)]


def get_distance_to_closest_kf(timestamp, keytimes):
    """Signed distance to the nearest keyframe time (the earlier one on a tie)."""
    idx = bisect.bisect_left(keytimes, timestamp)
    if idx == 0:
        kf = keytimes[0]
    elif idx == len(keytimes):
        kf = keytimes[-1]
    else:
        before, after = keytimes[idx - 1], keytimes[idx]
        kf = after if after - timestamp < timestamp - before else before
    return kf - timestamp


def find_keyframe_shift(group, src_keytimes, dst_keytimes, src_timecodes, dst_timecodes, max_kf_distance):
    """-> (start correction, end correction) of a group, None where the destination keyframe is further than the limit or the
    correction itself would reach it."""
    def distance(src_distance, dst_distance, limit):
        if abs(dst_distance) > limit:
            return None
        shift = dst_distance - src_distance
        return shift if abs(shift) < limit else None

    first, last = group[0], group[-1]
    src_start = get_distance_to_closest_kf(first.start, src_keytimes)
    src_end = get_distance_to_closest_kf(last.end + src_timecodes.get_frame_size(last.end), src_keytimes)
    dst_start = get_distance_to_closest_kf(first.shifted_start, dst_keytimes)
    dst_end = get_distance_to_closest_kf(last.shifted_end + dst_timecodes.get_frame_size(last.end), dst_keytimes)
    limit_start = src_timecodes.get_frame_size(first.start) * max_kf_distance
    limit_end = src_timecodes.get_frame_size(first.end) * max_kf_distance
    return distance(src_start, dst_start, limit_start), distance(src_end, dst_end, limit_end)


def find_keyframes_distances(event, src_keytimes, dst_keytimes, timecodes, max_kf_distance):
    """-> (start, end): how much further the destination keyframe is than the source one, 0 unless both and their difference are
    within the limit."""
    def distance(src_time, dst_time):
        src = get_distance_to_closest_kf(src_time, src_keytimes)
        dst = get_distance_to_closest_kf(dst_time, dst_keytimes)
        limit = timecodes.get_frame_size(src_time) * max_kf_distance
        if abs(src) < limit and abs(dst) < limit and abs(src - dst) < limit:
            return dst - src
        return 0

    return distance(event.start, event.shifted_start), distance(event.end, event.shifted_end)


def snap_groups_to_keyframes(events, chapter_times, max_ts_duration, max_ts_distance, src_keytimes, dst_keytimes, src_timecodes,
                             dst_timecodes, max_kf_distance, kf_mode):
    if not max_kf_distance:
        return
    groups = merge_short_lines_into_groups(events, chapter_times, max_ts_duration, max_ts_distance)

    if kf_mode in ("all", "shift"):
        # step 1: move whole lines without changing their duration (corrects a slightly imprecise audio shift)
        shifts, times = [], []
        for g in groups:
            shifts.extend(find_keyframe_shift(g, src_keytimes, dst_keytimes, src_timecodes, dst_timecodes, max_kf_distance))
            times.extend((g[0].shifted_start, g[-1].shifted_end))
        shifts = interpolate_nones(shifts, times)
        if len(shifts):
            mean_shift = np.mean(shifts)
            log.info("group %s-%s corrected by %s", format_time(events[0].start), format_time(events[-1].end), mean_shift)
            for g, (start_shift, end_shift) in zip(groups, zip(*[iter(shifts)] * 2)):
                if abs(start_shift - end_shift) > 0.001 and len(g) > 1:
                    actual = min(start_shift, end_shift, key=lambda x: abs(x - mean_shift))
                    log.warning("typesetting group at %s had different shifts at its start and end (%s and %s), shifting by %s",
                                format_time(g[0].start), start_shift, end_shift, actual)
                    for e in g:
                        e.adjust_shift(actual)
                else:
                    for e in g:
                        e.adjust_additional_shifts(start_shift, end_shift)

    if kf_mode in ("all", "snap"):
        # step 2: snap start and end separately (Sushi snaps the first line of a typesetting group too)
        for g in groups:
            start_shift, end_shift = find_keyframes_distances(g[0], src_keytimes, dst_keytimes, src_timecodes, max_kf_distance)
            if abs(start_shift) > 0.01 or abs(end_shift) > 0.01:
                log.info("snapping %s to keyframes, start by %s, end by %s", format_time(g[0].start), start_shift, end_shift)
                g[0].adjust_additional_shifts(start_shift, end_shift)


KF_OPTIONS = ("src_keyframes", "dst_keyframes", "src_fps", "dst_fps", "src_timecodes", "dst_timecodes")


def _flag(name):
    return "--" + name.replace("_", "-")


def check_keyframe_options(src_keyframes=None, dst_keyframes=None, src_fps=None, dst_fps=None, src_timecodes=None, dst_timecodes=None,
                           also_given=()):
    """Refuse (TimelineSyncError naming the option) what Sushi refuses, and what it silently ignores.  also_given: further options
    the caller saw (--kf-mode, --max-kf-distance) that have no effect without keyframes."""
    v = dict(src_keyframes=src_keyframes, dst_keyframes=dst_keyframes, src_fps=src_fps, dst_fps=dst_fps, src_timecodes=src_timecodes,
             dst_timecodes=dst_timecodes)
    have = [k for k in ("src_keyframes", "dst_keyframes") if v[k] is not None]
    if len(have) == 1:
        other = "dst_keyframes" if have[0] == "src_keyframes" else "src_keyframes"
        raise TimelineSyncError(f"{_flag(have[0])} without {_flag(other)}: either none or both of src and dst keyframes should be provided")
    if not have:
        useless = [_flag(k) for k in KF_OPTIONS[2:] if v[k] is not None] + list(also_given)
        if useless:
            raise TimelineSyncError(f"{', '.join(useless)}: no effect without --src-keyframes and --dst-keyframes")
        return False
    for side in ("src", "dst"):
        kf, fps, tc = v[side + "_keyframes"], v[side + "_fps"], v[side + "_timecodes"]
        if isinstance(kf, str):
            if kf in ("auto", "make"):
                raise TimelineSyncError(f"{_flag(side + '_keyframes')} {kf}: the inputs are WAV files, there is no video to make keyframes "
                                        "from; make the file with `python -m vse_amd.keyframes VIDEO -o keyframes.txt`")
            if not os.path.exists(kf):
                raise TimelineSyncError(f"{_flag(side + '_keyframes')}: file {kf} doesn't exist")
        if tc is not None and not os.path.exists(tc):
            raise TimelineSyncError(f"{_flag(side + '_timecodes')}: file {tc} doesn't exist")
        if fps is not None and tc is not None:
            raise TimelineSyncError(f"{_flag(side + '_fps')} and {_flag(side + '_timecodes')}: both fps and timecodes file cannot be specified "
                                    "at the same time")
        if fps is None and tc is None:
            raise TimelineSyncError(f"{_flag(side + '_keyframes')} needs {_flag(side + '_fps')} or {_flag(side + '_timecodes')}: fps or "
                                    "timecodes must be provided if keyframes are used")
        if fps is not None and not fps > 0:
            raise TimelineSyncError(f"{_flag(side + '_fps')} {fps}: not a frame rate")
    return True


def _keytimes(keyframes, fps, timecodes_path):
    """-> (timecodes, keyframe times) of one side; keyframes: a path (Sushi's file format) or a list of frame numbers."""
    tc = Timecodes.cfr(fps) if fps else Timecodes.from_file(timecodes_path)
    if isinstance(keyframes, str):
        from .keyframes import parse_keyframes
        frames = parse_keyframes(keyframes)
    else:
        frames = [int(f) for f in keyframes]
        if 0 not in frames:
            frames.insert(0, 0)
    return tc, [tc.get_frame_time(f) for f in frames]


def _extension(path):
    return os.path.splitext(path)[1].lower()


def sync(src_wav, dst_wav, script_path, output_path, *, window=10, max_window=30, rewind_thresh=5, grouping=True, smooth_radius=3,
         max_ts_duration=1001.0 / 24000.0 * 10, max_ts_distance=1001.0 / 24000.0 * 10, sample_rate=12000, search=None,
         src_keyframes=None, dst_keyframes=None, src_fps=None, dst_fps=None, src_timecodes=None, dst_timecodes=None, max_kf_distance=2,
         kf_mode="all", stream_build="host"):
    """Retime `script_path` (.srt or .ass) from the audio of `src_wav` onto that of `dst_wav`, write `output_path` (same type).
    search: the searcher (None: the GPU one, GpuSearch).  Returns the searches made, in order:
    [(src_off, m, dst_off, win_len, index, float32 value)] over the two uint8 streams.
    src_keyframes / dst_keyframes (both or none): a keyframes file or a list of frame numbers; each side then needs src_fps /
    dst_fps or src_timecodes / dst_timecodes (a v1 / v2 file).  Lines whose start or end lies within max_kf_distance frames of a
    keyframe on both sides snap to it; kf_mode: "shift" (whole lines), "snap" (start and end separately) or "all".
    stream_build: "host" builds the two uint8 streams with numpy (AudioStream), "device" on the GPU (DeviceAudioStream: the same
    bytes); "device" needs the GPU searcher."""
    use_kf = check_keyframe_options(src_keyframes, dst_keyframes, src_fps, dst_fps, src_timecodes, dst_timecodes)
    if kf_mode not in ("all", "shift", "snap"):
        raise TimelineSyncError(f"--kf-mode {kf_mode}: one of shift, snap, all")
    if stream_build not in ("host", "device"):
        raise TimelineSyncError(f"--stream-build {stream_build}: one of host, device")
    if stream_build == "device" and search is not None and not isinstance(search, GpuSearch):
        raise TimelineSyncError("--stream-build device needs the GPU searcher: its streams stay on the device")
    for path, what in ((src_wav, "Source"), (dst_wav, "Destination"), (script_path, "Script")):
        if not os.path.exists(path):
            raise TimelineSyncError(f"{what} file doesn't exist")
    for path in (src_wav, dst_wav):
        if _extension(path) != ".wav":
            raise TimelineSyncError(f"{path}: only WAV audio is supported (there is no demuxer)")
    ext = _extension(script_path)
    if ext not in (".ass", ".srt"):
        raise TimelineSyncError("Unknown script type")
    if _extension(output_path) != ext:
        raise TimelineSyncError(f"Source and destination script file types don't match ({ext} vs {_extension(output_path)})")

    if use_kf:
        src_timecodes, src_keytimes = _keytimes(src_keyframes, src_fps, src_timecodes)
        dst_timecodes, dst_keytimes = _keytimes(dst_keyframes, dst_fps, dst_timecodes)

    def snap(part):
        snap_groups_to_keyframes(part, [], max_ts_duration, max_ts_distance, src_keytimes, dst_keytimes, src_timecodes, dst_timecodes,
                                 max_kf_distance, kf_mode)

    script = (AssScript if ext == ".ass" else SrtScript).from_file(script_path)
    script.events.sort(key=lambda e: e.start)
    if stream_build == "device":
        if search is None:
            search = GpuSearch()
        src = DeviceAudioStream(src_wav, sample_rate, ctx=search.ctx)
        dst = DeviceAudioStream(dst_wav, sample_rate, ctx=search.ctx)
    else:
        src = AudioStream(src_wav, sample_rate)
        dst = AudioStream(dst_wav, sample_rate)
    searcher = _Searcher(GpuSearch() if search is None else search, src, dst)

    groups = prepare_search_groups(script.events, src.duration_seconds, [], max_ts_duration, max_ts_distance)
    calculate_shifts(searcher, src, dst, groups, window, max_window, rewind_thresh if grouping else 0)
    events = script.events
    fix_near_borders(events)
    if grouping:
        smooth_events([e for e in events if not e.linked], smooth_radius)
        groups = detect_groups(events)
        for g in groups:
            avg = average_shifts(g)
            log.info("group %s-%s: %d lines, shift %s", format_time(g[0].start), format_time(g[-1].end), len(g), avg)
    else:
        groups = [events]
    if use_kf:
        for e in events:
            if e.linked:
                e.resolve_link()
        for g in groups:
            snap(g)
    for e in events:
        e.apply_shift()
    script.save(output_path)
    return searcher.log


# ---- CLI -----------------------------------------------------------------------------------------------------------------------

_REFUSED = ["--test-shift-plot", "--src-audio", "--src-script", "--dst-audio", "--no-cleanup", "--temp-dir", "--chapters"]


def _parser():
    p = argparse.ArgumentParser(prog="python -m vse_amd.timeline_sync",
                                description="Shift a subtitle script to another release's audio (Sushi's WAV path on the GPU).")
    p.add_argument("--src", required=True, help="source audio (.wav) the script is timed to")
    p.add_argument("--dst", required=True, help="destination audio (.wav) to retime the script to")
    p.add_argument("--script", required=True, help="script to retime (.srt or .ass)")
    p.add_argument("-o", "--output", default=None, help="output script [<dst>.sushi.<ext>]")
    p.add_argument("--window", default=10, type=int)
    p.add_argument("--max-window", default=30, type=int)
    p.add_argument("--rewind-thresh", default=5, type=int)
    p.add_argument("--no-grouping", action="store_false", dest="grouping")
    p.add_argument("--smooth-radius", default=3, type=int)
    p.add_argument("--max-ts-duration", default=1001.0 / 24000.0 * 10, type=float)
    p.add_argument("--max-ts-distance", default=1001.0 / 24000.0 * 10, type=float)
    p.add_argument("--sample-rate", default=12000, type=int)
    p.add_argument("--sample-type", default="uint8")
    p.add_argument("--stream-build", default="host", choices=["host", "device"],
                   help="where the two uint8 streams are built from the WAVs: numpy on the host, or the GPU (the same bytes) [host]")
    p.add_argument("--src-keyframes", default=None, help="source keyframes file (python -m vse_amd.keyframes writes one)")
    p.add_argument("--dst-keyframes", default=None, help="destination keyframes file")
    p.add_argument("--src-fps", default=None, type=float, help="fps of the source video (or --src-timecodes)")
    p.add_argument("--dst-fps", default=None, type=float, help="fps of the destination video (or --dst-timecodes)")
    p.add_argument("--src-timecodes", default=None, help="timecodes file (v1 / v2) of the source video")
    p.add_argument("--dst-timecodes", default=None, help="timecodes file (v1 / v2) of the destination video")
    p.add_argument("--max-kf-distance", default=None, type=float, help="maximum keyframe snapping distance in frames [2]")
    p.add_argument("--kf-mode", default=None, choices=["shift", "snap", "all"], help="keyframe correction mode [all]")
    p.add_argument("-v", "--verbose", action="store_true")
    for flag in _REFUSED:
        p.add_argument(flag, nargs="?", const=True, default=None, help=argparse.SUPPRESS)
    return p


def main(argv=None):
    args = _parser().parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.INFO, format="%(message)s")
    given = [f for f in _REFUSED if getattr(args, f[2:].replace("-", "_")) is not None]
    if args.sample_type != "uint8":
        given.append(f"--sample-type {args.sample_type}")
    if given:
        print(f"timeline_sync: not supported: {', '.join(given)} (WAV inputs and uint8 streams only)", file=sys.stderr)
        return 2
    output = args.output or args.dst + ".sushi" + _extension(args.script)
    kf = {k: getattr(args, k) for k in KF_OPTIONS}
    try:
        # the option checks come before the WAV and script existence checks
        check_keyframe_options(**kf, also_given=[f for f, x in (("--kf-mode", args.kf_mode), ("--max-kf-distance", args.max_kf_distance))
                                                 if x is not None])
        sync(args.src, args.dst, args.script, output, window=args.window, max_window=args.max_window, rewind_thresh=args.rewind_thresh,
             grouping=args.grouping, smooth_radius=args.smooth_radius, max_ts_duration=args.max_ts_duration,
             max_ts_distance=args.max_ts_distance, sample_rate=args.sample_rate, **kf,
             max_kf_distance=2 if args.max_kf_distance is None else args.max_kf_distance, kf_mode=args.kf_mode or "all",
             stream_build=args.stream_build)
    except TimelineSyncError as e:
        print(f"timeline_sync: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
