"""Frame ingest without a codec library (row N3 of SURVEY §8(f), the part that can exist here).

The reference decodes with cv2.VideoCapture (FFmpeg underneath): sequential reads in the frame selectors
(backend/main.py:228-376) and random seeks per OCR task (backend/tools/subtitle_ocr.py:173-204).  Neither cv2 nor ffmpeg
exists on the build or the GPU box, so compressed video cannot be decoded by anything in this repository; what CAN be read
bit-exactly is uncompressed video: AVI with 24-bit BGR DIB frames ('DIB ' / BI_RGB — what `ffmpeg -c:v rawvideo -pix_fmt bgr24
out.avi` writes and cv2 reads back unchanged), and a stack of frames in a .npy file.  Both give the frame-source interface of
extractor.py: frame_count, fps, read(frame_no) (1-based random access, like CAP_PROP_POS_FRAMES = frame_no - 1 then read()),
frames() (decode order), pos_msec(frame_no) (what the SRT writer asks for, see AviBgr24Source.pos_msec).

Round 3: Motion-JPEG AVI (`ffmpeg -c:v mjpeg`, what many capture devices write) is the ONE compressed format that can be read here —
every frame is a stand-alone baseline JPEG, and Pillow (libjpeg-turbo; importable on both boxes) decodes it.  The reference decodes
the same stream with FFmpeg's own MJPEG decoder through cv2.VideoCapture: its IDCT / chroma up-sampling differ from libjpeg's by
+-1..2 grey levels on some pixels, so this source is NOT bit-identical to the reference's decode (the uncompressed sources are).

YUV 4:2:0 (Y4mSource, Yuv420Source): what every decoder produces before any colour conversion, at 1.5 bytes per pixel — `ffmpeg -pix_fmt
yuv420p -f yuv4mpegpipe` (YUV4MPEG2, self-describing), `-f rawvideo` (headerless I420) and a hardware decoder's NV12 surfaces.  The files
are memory-mapped; read() converts to BGR on the host (Yuv420Frame.to_bgr), read_raw() hands out the planes themselves (Yuv420Frame), which
staging.Uploader packs into its pinned slab, uploads at half the bytes of a BGR frame and converts on the device (vse_yuv420_to_bgr): the
same integers on both routes.  The conversion is BT.601 limited range with NEAREST chroma (the fixed-point constants of cv2.cvtColor
COLOR_YUV2BGR_I420 / _NV12; the formula is in include/vse_hip.h).  The reference's cv2.VideoCapture converts with swscale: the same
matrix, but a chroma up-sampling filter instead of the nearest sample, so these frames are NOT swscale's bits at chroma edges (luma-only
content is).  matrix="bt709" on a frame or a source swaps the chroma factors for BT.709's (vse_yuv_to_bgr_matrix; HD encodes normally carry
it); the default stays "bt601" because Y4M has no matrix tag.  Full-range (JPEG) YUV, 4:2:2 / 4:4:4 and more than 8 bits are refused.

Other formats (YuvFormat, YuvFrame, YuvSource; Y4mSource / Y4mStream / open_source with wide=True): 9 to 16 bits, 4:2:2, 4:4:4, grey, full
range, BT.2020 and P010-style semi-planar surfaces are accepted only when asked for, so that the refusals above stand.  A YuvFormat is the
integers of include/vse_hip.h vse_yuv_to_bgr_format; YuvFrame.to_bgr and the device convert with the same integers (the 8-bit ones with
factors scaled to the depth, nearest chroma, no transfer function: PQ / HLG material comes out flat, its text and edges remain).

HDR video (ToneMap; transfer="pq" | "hlg" on those readers): the frames carry a ToneMap, and YuvFrame.to_bgr and the device
(vse_yuv_to_bgr_tonemap) convert by the same integers at 12 bits, then through the map's tables: the EOTF and a tone curve to linear light
relative to SDR white, BT.2020 to BT.709 in linear light, the output gamma.  Y4M carries no transfer tag: it is the caller's to say.

Interlaced video (InterlacedYuvFrame; deinterlace="adaptive" | "interpolate" on those readers, on top of wide=True): the pictures are two
woven fields.  A frame carries the previous picture's planes beside its own; to_bgr() and the device (vse_yuv_deinterlace, through
staging.Uploader) keep the first field's rows, weave what did not change since the previous picture and interpolate the rest, by the same
integers.  Without the keyword interlaced headers are refused as before.  deinterlace="match" is for film carried in interlaced video
(3:2 pulldown, fields shifted by one): every picture of the film is still in the stream, its second field in the neighbouring frame, and
each frame is woven whole with the partner field that combs least (vse_yuv_field_match), which gives the film's pictures back byte for
byte; a frame that combs with every partner falls back to the adaptive rule.  Frame count and times stay one to one.

Pipes (Y4mStream): `ffmpeg -i film.mkv -pix_fmt yuv420p -f yuv4mpegpipe - | python -m vse_amd.extractor -` puts compressed video of any
codec through a decoder that is not ours; the stream is read once, front to back, never seeks and has no read(): its absence is how
SubtitleExtractor sees that it must work in one pass.
"""
import logging
import mmap
import os
import re
import struct
from collections import namedtuple
from fractions import Fraction

import numpy as np


def write_avi_bgr24(path, frames, fps, riff_frames=None, dropped=()):
    """Uncompressed AVI (one 'vids' stream, BI_RGB 24 bit, bottom-up rows padded to 4 bytes, idx1 index).
    riff_frames: start a new `RIFF....AVIX` segment (OpenDML, what ffmpeg's muxer does after ~1 GiB) every that many frames;
    dropped: 0-based frame indices written as zero-length chunks (a dropped frame: the previous picture is shown again)."""
    frames = [np.asarray(f) for f in frames]
    h, w, _ = frames[0].shape
    stride = (w * 3 + 3) & ~3
    size = stride * h
    rate, scale = int(round(fps * 1000)), 1000

    def chunk(tag, data):
        return tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")

    def lst(tag, data):
        return b"LIST" + struct.pack("<I", len(data) + 4) + tag + data
    avih = struct.pack("<14I", int(1e6 / fps), size * int(fps + 1), 0, 0x10, len(frames), 0, 1, size, w, h, 0, 0, 0, 0)
    strh = b"vids" + b"DIB " + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, len(frames), size, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, size, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    segments, movi, idx = [], b"", b""
    for k, f in enumerate(frames):
        assert f.shape == (h, w, 3) and f.dtype == np.uint8
        if riff_frames and k and k % riff_frames == 0:
            segments.append(movi)
            movi = b""
        if k in dropped:
            data = b""
        else:
            rows = np.zeros((h, stride), np.uint8)
            rows[:, :w * 3] = f[::-1].reshape(h, w * 3)
            data = rows.tobytes()
        if not segments:
            idx += b"00db" + struct.pack("<III", 0x10, 4 + len(movi), len(data))       # idx1 covers the first RIFF only
        movi += chunk(b"00db", data)
    segments.append(movi)
    body = b"AVI " + hdrl + lst(b"movi", segments[0]) + chunk(b"idx1", idx)
    with open(path, "wb") as fp:
        fp.write(b"RIFF" + struct.pack("<I", len(body)) + body)
        for seg in segments[1:]:
            body = b"AVIX" + lst(b"movi", seg)
            fp.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def write_avi_mjpeg(path, frames, fps, quality=90):
    """Motion-JPEG AVI (one 'vids' stream, fourcc MJPG, every frame a baseline JPEG encoded by Pillow)."""
    import io
    from PIL import Image
    frames = [np.asarray(f) for f in frames]
    h, w, _ = frames[0].shape
    rate, scale = int(round(fps * 1000)), 1000
    blobs = []
    for f in frames:
        bio = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(bio, format="JPEG", quality=quality)
        blobs.append(bio.getvalue())
    big = max(len(b) for b in blobs)

    def chunk(tag, data):
        return tag + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")

    def lst(tag, data):
        return b"LIST" + struct.pack("<I", len(data) + 4) + tag + data
    avih = struct.pack("<14I", int(1e6 / fps), big * int(fps + 1), 0, 0x10, len(frames), 0, 1, big, w, h, 0, 0, 0, 0)
    strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, scale, rate, 0, len(frames), big, 0xFFFFFFFF, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + lst(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf)))
    movi, idx = b"", b""
    for b in blobs:
        idx += b"00dc" + struct.pack("<III", 0x10, 4 + len(movi), len(b))
        movi += chunk(b"00dc", b)
    body = b"AVI " + hdrl + lst(b"movi", movi) + chunk(b"idx1", idx)
    with open(path, "wb") as fp:
        fp.write(b"RIFF" + struct.pack("<I", len(body)) + body)


class AviBgr24Source:
    """Random-access reader of uncompressed BGR24 AVI (write_avi_bgr24 / ffmpeg rawvideo bgr24) and of Motion-JPEG AVI
    (write_avi_mjpeg / ffmpeg -c:v mjpeg; frames decoded by Pillow); any other codec is refused."""

    def __init__(self, path):
        self.path = path
        self._fp = open(path, "rb")
        head = self._fp.read(12)
        if head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError(f"{path}: not a RIFF AVI file")
        self._offsets = []
        self.width = self.height = None
        self.fps = None
        self.mjpeg = False
        # every top-level RIFF chunk: the 'AVI ' one, then the OpenDML 'AVIX' segments a muxer opens about every GiB (170 frames
        # of 1080p bgr24) — a reader that stops after the first would silently see the first seconds of a clip only
        self._fp.seek(0, 2)
        size, pos = self._fp.tell(), 0
        while pos + 12 <= size:
            self._fp.seek(pos)
            tag, n, kind = struct.unpack("<4sI4s", self._fp.read(12))
            if tag != b"RIFF" or kind not in (b"AVI ", b"AVIX"):
                raise ValueError(f"{path}: {size - pos} bytes behind the last RIFF chunk are not an AVI segment ({tag!r} {kind!r})")
            self._walk(pos + 12, min(pos + 8 + n, size))
            pos += 8 + n + (n & 1)
        if self.width is None or self.fps is None:
            raise ValueError(f"{path}: no video stream header")
        self.frame_count = len(self._offsets)
        self._stride = (self.width * 3 + 3) & ~3

    def _walk(self, pos, end):
        fp = self._fp
        while pos + 8 <= end:
            fp.seek(pos)
            tag, n = struct.unpack("<4sI", fp.read(8))
            if tag == b"LIST":
                kind = fp.read(4)
                if kind in (b"hdrl", b"strl", b"movi"):
                    self._walk(pos + 12, pos + 8 + n)
            elif tag == b"strh":
                d = fp.read(n)
                if d[:4] == b"vids":
                    self.fourcc = d[4:8]
                    if d[4:8].upper() in (b"MJPG", b"JPEG"):
                        self.mjpeg = True
                    elif d[4:8] not in (b"DIB ", b"\0\0\0\0", b"RAW "):
                        raise ValueError(f"{self.path}: compressed video ({d[4:8]!r}) needs a codec; only uncompressed BGR24 and "
                                         "Motion-JPEG AVI can be read here")
                    scale, rate = struct.unpack("<II", d[20:28])
                    self.fps = rate / float(scale)
            elif tag == b"strf":
                d = fp.read(n)
                _sz, w, h, _planes, bits, comp = struct.unpack("<IiiHHI", d[:20])
                if getattr(self, "mjpeg", False):
                    self.width, self.height, self._bottom_up = w, abs(h), False
                elif bits != 24 or comp != 0:
                    raise ValueError(f"{self.path}: only BI_RGB 24-bit frames are supported (bits={bits}, compression={comp})")
                self.width, self.height, self._bottom_up = w, abs(h), h > 0
            elif tag in (b"00db", b"00dc"):
                self._offsets.append((pos + 8, n))
            pos += 8 + n + (n & 1)

    def read(self, frame_no):
        if not 1 <= frame_no <= self.frame_count:
            return None
        off, n = self._offsets[frame_no - 1]
        while n == 0 and frame_no > 1:          # zero-length chunk = dropped frame: the previous picture stays on screen
            frame_no -= 1
            off, n = self._offsets[frame_no - 1]
        if self.mjpeg:
            if n == 0:
                return None
            import io
            from PIL import Image
            self._fp.seek(off)
            img = Image.open(io.BytesIO(self._fp.read(n)))
            rgb = np.asarray(img.convert("RGB"))
            if rgb.shape[:2] != (self.height, self.width):
                raise ValueError(f"{self.path}: frame {frame_no} is {rgb.shape[1]}x{rgb.shape[0]}, the stream header says {self.width}x{self.height}")
            return np.ascontiguousarray(rgb[:, :, ::-1])            # BGR like cv2
        if n < self._stride * self.height:
            return None
        self._fp.seek(off)
        rows = np.frombuffer(self._fp.read(n), np.uint8)[:self._stride * self.height].reshape(self.height, self._stride)
        img = rows[:, :self.width * 3].reshape(self.height, self.width, 3)
        return np.ascontiguousarray(img[::-1] if self._bottom_up else img)

    def frames(self):
        for no in range(1, self.frame_count + 1):
            yield self.read(no)

    def pos_msec(self, frame_no):
        """main.py:738-743: cap.set(CAP_PROP_POS_FRAMES, frame_no); cap.read(); cap.get(CAP_PROP_POS_MSEC) — the time stamp of
        the frame with 0-based index frame_no (constant frame rate here); None when that read fails (past the end)."""
        return None if not 0 <= frame_no < self.frame_count else frame_no * 1000.0 / self.fps

    def close(self):
        self._fp.close()


class NpySource:
    """Frames stacked in one .npy file [N,H,W,3] uint8 (memory-mapped)."""

    def __init__(self, path, fps):
        self._a = np.load(path, mmap_mode="r")
        if self._a.ndim != 4 or self._a.shape[3] != 3 or self._a.dtype != np.uint8:
            raise ValueError(f"{path}: expected uint8 [N,H,W,3]")
        self.frame_count, self.fps = int(self._a.shape[0]), float(fps)

    def read(self, frame_no):
        return np.ascontiguousarray(self._a[frame_no - 1]) if 1 <= frame_no <= self.frame_count else None

    def frames(self):
        for no in range(1, self.frame_count + 1):
            yield self.read(no)

    pos_msec = None


# ---- YUV 4:2:0 ------------------------------------------------------------------------------------------------------------------
YUV_LAYOUTS = ("i420", "nv12")
# chroma factors (B from u, G from u, G from v, R from v) of include/vse_hip.h: vse_yuv420_to_bgr / vse_yuv_to_bgr_matrix
YUV_MATRICES = {"bt601": (2116026, -409993, -852492, 1673527), "bt709": (2215014, -223607, -558796, 1879825)}


def _check_matrix(matrix):
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix must be one of {tuple(YUV_MATRICES)}, not {matrix!r}")
    return matrix


def _chroma_size(height, width):
    return (height + 1) >> 1, (width + 1) >> 1


class Yuv420Frame:
    """Rows [y0, y1) of one 4:2:0 picture that has not been converted: the planes (views, e.g. into a file mapping) with `height`,
    `width` and `layout` ("i420": planes = (Y [H,W], U [ch,cw], V [ch,cw]); "nv12": planes = (Y [H,W], UV [ch,2 cw])).
    It stands where a BGR frame stands in the callers that only look at `.shape` and cut row bands: shape == (y1 - y0, width, 3),
    frame[a:b] narrows the row range (one slice, step 1, Python slice rules; any other index is a TypeError), to_bgr() gives the
    uint8 BGR ndarray, pack_into() the packed sub-frame vse_yuv420_to_bgr takes.  `matrix` ("bt601" | "bt709") names the conversion
    and travels with the slices."""

    def __init__(self, planes, height, width, layout="i420", y0=0, y1=None, matrix="bt601"):
        if layout not in YUV_LAYOUTS:
            raise ValueError(f"layout must be one of {YUV_LAYOUTS}, not {layout!r}")
        self.matrix = _check_matrix(matrix)
        self.planes, self.height, self.width, self.layout = tuple(planes), int(height), int(width), layout
        self.y0, self.y1 = int(y0), int(self.height if y1 is None else y1)
        ch, cw = _chroma_size(self.height, self.width)
        want = [(self.height, self.width)] + ([(ch, cw)] * 2 if layout == "i420" else [(ch, 2 * cw)])
        if [tuple(p.shape) for p in self.planes] != want or not 0 <= self.y0 <= self.y1 <= self.height:
            raise ValueError(f"{layout} planes of a {self.height} x {self.width} picture are {want}, rows {self.y0}:{self.y1} asked of "
                             f"{[tuple(p.shape) for p in self.planes]}")

    @property
    def shape(self):
        return (self.y1 - self.y0, self.width, 3)

    def __getitem__(self, idx):
        if not isinstance(idx, slice):
            raise TypeError(f"a Yuv420Frame takes one row slice, not {idx!r}")
        a, b, step = idx.indices(self.y1 - self.y0)
        if step != 1:
            raise TypeError(f"a Yuv420Frame takes a row slice of step 1, not {idx!r}")
        return Yuv420Frame(self.planes, self.height, self.width, self.layout, self.y0 + a, self.y0 + max(a, b), self.matrix)

    @property
    def row_parity(self):
        return self.y0 & 1

    def _chroma_rows(self):
        return self.y0 >> 1, (self.y1 + 1) >> 1

    @property
    def packed_bytes(self):
        c0, c1 = self._chroma_rows()
        return (self.y1 - self.y0) * self.width + 2 * (c1 - c0) * ((self.width + 1) >> 1)

    def pack_into(self, dst_u8):
        """The packed sub-frame (luma rows y0..y1, then chroma rows y0 >> 1 .. (y1 + 1) >> 1 of each plane; row parity y0 & 1) into the
        first packed_bytes bytes of the 1-D uint8 array dst_u8: three contiguous copies for I420, two for NV12."""
        c0, c1 = self._chroma_rows()
        pos = 0
        for plane, (a, b) in zip(self.planes, [(self.y0, self.y1)] + [(c0, c1)] * (len(self.planes) - 1)):
            part = plane[a:b]
            np.copyto(dst_u8[pos:pos + part.size].reshape(part.shape), part)
            pos += part.size
        return pos

    def to_bgr(self, matrix=None):
        """uint8 BGR [y1 - y0, W, 3]: limited range, nearest chroma, the integers of vse_yuv420_to_bgr / vse_yuv_to_bgr_matrix
        (include/vse_hip.h) for `matrix` (default: the frame's own)."""
        bu, gu, gv, rv = YUV_MATRICES[_check_matrix(self.matrix if matrix is None else matrix)]
        rows, cols = np.arange(self.y0, self.y1) >> 1, np.arange(self.width) >> 1
        y = self.planes[0][self.y0:self.y1].astype(np.int32)
        if self.layout == "i420":
            u, v = (np.asarray(p)[rows][:, cols].astype(np.int32) for p in self.planes[1:])
        else:
            uv = np.asarray(self.planes[1])[rows]
            u, v = uv[:, 2 * cols].astype(np.int32), uv[:, 2 * cols + 1].astype(np.int32)
        c = np.maximum(y - 16, 0) * 1220542 + (1 << 19)
        u -= 128
        v -= 128
        out = np.empty(self.shape, np.uint8)
        out[..., 0] = np.clip((c + bu * u) >> 20, 0, 255)
        out[..., 1] = np.clip((c + gu * u + gv * v) >> 20, 0, 255)
        out[..., 2] = np.clip((c + rv * v) >> 20, 0, 255)
        return out


# ---- any planar / semi-planar YUV (vse_yuv_to_bgr_format) --------------------------------------------------------------------------
YUV_FORMAT_MATRICES = ("bt601", "bt709", "bt2020")
YUV_RANGES = ("auto", "limited", "full")
# (KY, BU, GU, GV, RV)_0 of include/vse_hip.h vse_yuv_to_bgr_format, by (full_range, matrix)
YUV_K0 = {(0, "bt601"): (1220542,) + YUV_MATRICES["bt601"], (0, "bt709"): (1220542,) + YUV_MATRICES["bt709"],
          (0, "bt2020"): (1220542, 2245811, -196426, -682019, 1760217),
          (1, "bt601"): (1 << 20, 1858077, -360853, -748826, 1470104), (1, "bt709"): (1 << 20, 1945738, -196424, -490864, 1651297),
          (1, "bt2020"): (1 << 20, 1972791, -172546, -599107, 1546230)}
_SUBSAMPLING = {"444": (0, 0), "422": (1, 0), "420": (1, 1)}
_PIX_FMT = re.compile(r"yuv(j?)(420|422|444)p(9|10|12|14|16)?(le|be)?$")
_PIX_FMT_GRAY = re.compile(r"gr[ae]y(8|9|10|12|14|16)?(le|be)?$")
_PIX_FMT_P0 = re.compile(r"p0(10|12|16)(le|be)?$")
_Y4M_C = re.compile(r"(?:(420)(?:jpeg|mpeg2|paldv)|(420|422|444)(?:p(9|10|12|14|16))?|(mono)(?:p?(9|10|12|14|16))?)$")


class YuvFormat(namedtuple("YuvFormat", "sub_x sub_y chroma depth msb matrix full_range")):
    """A pixel format as the integers of include/vse_hip.h vse_yuv_to_bgr_format: sub_x, sub_y (log2 chroma subsampling), chroma (0 grey,
    1 planar U then V, 2 interleaved UV), depth (8..16; 2-byte little-endian samples above 8), msb (1: the value in the word's high bits,
    P010-style), matrix (a name of YUV_FORMAT_MATRICES) and full_range (0 | 1).  A tuple: equal formats compare and hash equal."""
    __slots__ = ()

    def __new__(cls, sub_x=1, sub_y=1, chroma=1, depth=8, msb=0, matrix="bt601", full_range=0):
        self = super().__new__(cls, int(sub_x), int(sub_y), int(chroma), int(depth), int(msb), matrix, int(bool(full_range)))
        if ((self.sub_x, self.sub_y) not in _SUBSAMPLING.values() or self.chroma not in (0, 1, 2) or not 8 <= self.depth <= 16
                or self.msb not in ((0,) if self.depth == 8 else (0, 1)) or (self.chroma == 0 and (self.sub_x, self.sub_y) != (0, 0))
                or (self.chroma == 2 and (self.sub_x, self.sub_y) != (1, 1))):
            raise ValueError(f"not a YUV format: subsampling {self.sub_x}, {self.sub_y} of 0, 0 | 1, 0 | 1, 1, chroma {self.chroma} of 0 (4:4:4 "
                             f"only) | 1 | 2 (4:2:0 only), depth {self.depth} of 8..16, msb {self.msb} of 0 | 1 (0 at depth 8)")
        if matrix not in YUV_FORMAT_MATRICES:
            raise ValueError(f"matrix must be one of {YUV_FORMAT_MATRICES}, not {matrix!r}")
        return self

    @property
    def sample_bytes(self):
        return 1 if self.depth == 8 else 2

    @property
    def sample_dtype(self):
        return np.dtype(np.uint8) if self.depth == 8 else np.dtype("<u2")

    def chroma_size(self, height, width):
        return (height + self.sub_y) >> self.sub_y, (width + self.sub_x) >> self.sub_x

    def plane_shapes(self, height, width):
        """The planes of a height x width picture, in samples: [Y], [Y, U, V] or [Y, UV]."""
        ch, cw = self.chroma_size(height, width)
        return [(height, width)] + ([], [(ch, cw)] * 2, [(ch, 2 * cw)])[self.chroma]

    def frame_bytes(self, height, width):
        return self.sample_bytes * sum(r * c for r, c in self.plane_shapes(height, width))

    def factors(self):
        """-> (shift, maxv, yoff, coff, KY_s, BU_s, GU_s, GV_s, RV_s): sample = min(word >> shift, maxv) and the integers of the formula."""
        s = self.depth - 8

        def scaled(k):
            m = (abs(k) + ((1 << s) >> 1)) >> s
            return -m if k < 0 else m
        return ((16 - self.depth if self.msb else 0), (1 << self.depth) - 1, 0 if self.full_range else 16 << s, 128 << s) + \
            tuple(scaled(k) for k in YUV_K0[self.full_range, self.matrix])

    @classmethod
    def from_pix_fmt(cls, name, matrix="bt601", range="auto"):
        """FFmpeg's name of a pixel format (yuv420p, yuvj420p, nv12, yuv422p, yuv444p, gray, yuv420p10le, yuv422p10le, yuv444p12le, gray10le,
        p010le, p016le ...; i420 for yuv420p; 9, 10, 12, 14 and 16 bits; the `le` may be left out).  range: "auto" is limited, full for
        the yuvj names; "limited" | "full" override it.  Big-endian samples and every other name are refused."""
        if range not in YUV_RANGES:
            raise ValueError(f"range must be one of {YUV_RANGES}, not {range!r}")
        text = str(name).lower()
        text = {"i420": "yuv420p", "p010": "p010le", "p012": "p012le", "p016": "p016le"}.get(text, text)
        full, msb, chroma = 0, 0, 1
        m = _PIX_FMT.match(text)
        if m:
            full, (sx, sy), depth, end = int(bool(m.group(1))), _SUBSAMPLING[m.group(2)], int(m.group(3) or 8), m.group(4)
            ok = not (full and depth != 8) and not (depth == 8 and end)
        elif text == "nv12":
            (sx, sy), chroma, depth, end, ok = (1, 1), 2, 8, None, True
        elif _PIX_FMT_P0.match(text):
            m = _PIX_FMT_P0.match(text)
            (sx, sy), chroma, depth, msb, end, ok = (1, 1), 2, int(m.group(1)), 1, m.group(2), True
        elif _PIX_FMT_GRAY.match(text):
            m = _PIX_FMT_GRAY.match(text)
            (sx, sy), chroma, depth, end = (0, 0), 0, int(m.group(1) or 8), m.group(2)
            ok = not (depth == 8 and end)
        else:
            ok, end = False, None
        if end == "be":
            raise ValueError(f"pixel format {name!r}: big-endian samples are not supported")
        if not ok:
            raise ValueError(f"pixel format {name!r} is not supported: planar yuv420p / yuv422p / yuv444p and gray at 8, 9, 10, 12, 14 or 16 "
                             "bits (little-endian), yuvj420p / yuvj422p / yuvj444p, nv12, p010le / p012le / p016le")
        if range != "auto":
            full = int(range == "full")
        return cls(sx, sy, chroma, depth, msb, matrix, full)

    @classmethod
    def from_y4m_tokens(cls, c_token=None, range_token=None, matrix="bt601", range="auto"):
        """The format a YUV4MPEG2 header names: its C token (None: C420jpeg) and its XCOLORRANGE token (None: limited), both whole,
        e.g. "C420p10" and "XCOLORRANGE=FULL".  range: "limited" | "full" override the header's.  ValueError names the token refused."""
        if range not in YUV_RANGES:
            raise ValueError(f"range must be one of {YUV_RANGES}, not {range!r}")
        val = "420jpeg" if c_token is None else c_token[1:]
        if "alpha" in val:
            raise ValueError(f"an alpha plane ({c_token}) is not supported")
        m = _Y4M_C.match(val)
        if not m:
            raise ValueError(f"chroma format {c_token} is not supported, only C420 (jpeg, mpeg2, paldv), C422, C444 and Cmono, each also at 9, "
                             "10, 12, 14 or 16 bits (C420p10 ... Cmono10)")
        sub, depth = m.group(1) or m.group(2) or m.group(4), int(m.group(3) or m.group(5) or 8)
        if range_token not in (None, "XCOLORRANGE=FULL", "XCOLORRANGE=LIMITED"):
            raise ValueError(f"colour range {range_token} is not supported, only XCOLORRANGE=FULL and XCOLORRANGE=LIMITED")
        full = int(range_token == "XCOLORRANGE=FULL") if range == "auto" else int(range == "full")
        sx, sy = _SUBSAMPLING.get(sub, (0, 0))
        return cls(sx, sy, 0 if sub == "mono" else 1, depth, 0, matrix, full)


# ---- HDR: PQ / HLG -> SDR (vse_yuv_to_bgr_tonemap) ----------------------------------------------------------------------------------
TONE_TRANSFERS = ("pq", "hlg")
TONE_PRIMARIES = ("bt2020", "bt709")
TONE_CURVES = ("knee", "clip")
TONE_CODES, TONE_GAMMA_ENTRIES, TONE_PEAK_CODE = 4096, 7936, 4080           # A's and T's lengths; the 12-bit code of R'G'B' = 1
_CHROMATICITIES = {"bt709": ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06)), "bt2020": ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046))}
_D65 = (0.3127, 0.3290)
_HLG_A = 0.17883277
_HLG_B, _HLG_C = 1.0 - 4.0 * _HLG_A, 0.5 - _HLG_A * np.log(4.0 * _HLG_A)
_PQ_M1, _PQ_M2, _PQ_C1, _PQ_C2, _PQ_C3 = 2610.0 / 16384, 2523.0 / 4096 * 128, 3424.0 / 4096, 2413.0 / 4096 * 32, 2392.0 / 4096 * 32


def _rgb_to_xyz(primaries):
    xy = np.array(_CHROMATICITIES[primaries], np.float64)
    cols = np.stack([xy[:, 0] / xy[:, 1], np.ones(3), (1.0 - xy[:, 0] - xy[:, 1]) / xy[:, 1]])
    white = np.array([_D65[0] / _D65[1], 1.0, (1.0 - _D65[0] - _D65[1]) / _D65[1]])
    return cols * np.linalg.solve(cols, white)


def bt2020_to_bt709():
    """The 3 x 3 matrix from linear BT.2020 RGB to linear BT.709 RGB (float64, rows and columns R G B), from the chromaticities and D65."""
    return np.linalg.solve(_rgb_to_xyz("bt709"), _rgb_to_xyz("bt2020"))


def pq_eotf(e):
    """SMPTE ST 2084: the non-linear signal 0..1 -> nits, 0..10 000 (float64)."""
    p = np.power(np.clip(np.asarray(e, np.float64), 0.0, 1.0), 1.0 / _PQ_M2)
    return 10000.0 * np.power(np.maximum(p - _PQ_C1, 0.0) / (_PQ_C2 - _PQ_C3 * p), 1.0 / _PQ_M1)


def pq_inverse_eotf(nits):
    y = np.power(np.clip(np.asarray(nits, np.float64) / 10000.0, 0.0, 1.0), _PQ_M1)
    return np.power((_PQ_C1 + _PQ_C2 * y) / (1.0 + _PQ_C3 * y), _PQ_M2)


def hlg_nits(e):
    """BT.2100 HLG, PER CHANNEL: the inverse OETF, then 1000 * E ** 1.2 nits (a 1000-nit display's system gamma).  The true OOTF applies
    that gamma to the luminance of the three channels together; per channel it shifts saturated colours (a known limit)."""
    e = np.clip(np.asarray(e, np.float64), 0.0, 1.0)
    scene = np.where(e <= 0.5, e * e / 3.0, (np.exp((e - _HLG_C) / _HLG_A) + _HLG_B) / 12.0)
    return 1000.0 * np.power(scene, 1.2)


def hlg_inverse_nits(nits):
    """The inverse of hlg_nits: nits 0..1000 -> the HLG signal 0..1."""
    scene = np.power(np.clip(np.asarray(nits, np.float64) / 1000.0, 0.0, 1.0), 1.0 / 1.2)
    return np.where(scene <= 1.0 / 12.0, np.sqrt(3.0 * scene), _HLG_A * np.log(np.maximum(12.0 * scene - _HLG_B, 1e-300)) + _HLG_C)


class ToneMap(namedtuple("ToneMap", "transfer primaries white_nits peak_nits curve knee gamma")):
    """How HDR material becomes the SDR BGR the detector and the recogniser were made for: the data of include/vse_hip.h
    vse_yuv_to_bgr_tonemap.  transfer "pq" | "hlg"; primaries "bt2020" (mapped to BT.709 in linear light) | "bt709" (left alone); white_nits
    the luminance that becomes SDR white (BT.2408's 203); curve "clip" cuts there, "knee" is linear up to `knee` of white and rolls
    everything from there to peak_nits off into the rest; gamma the output gamma.  A tuple: equal maps compare and hash equal, and the
    tables are built once per distinct map.  Tone mapping is per channel (saturated highlights shift in hue), there is no dynamic metadata
    and no constant-luminance BT.2020; 203, 1000 and 0.8 are conventions and guesses, not measurements."""
    __slots__ = ()

    def __new__(cls, transfer, primaries="bt2020", white_nits=203.0, peak_nits=1000.0, curve="knee", knee=0.8, gamma=2.4):
        if transfer not in TONE_TRANSFERS:
            raise ValueError(f"transfer must be one of {TONE_TRANSFERS}, not {transfer!r}")
        if primaries not in TONE_PRIMARIES:
            raise ValueError(f"primaries must be one of {TONE_PRIMARIES}, not {primaries!r}")
        if curve not in TONE_CURVES:
            raise ValueError(f"curve must be one of {TONE_CURVES}, not {curve!r}")
        try:
            white_nits, peak_nits, knee, gamma = float(white_nits), float(peak_nits), float(knee), float(gamma)
        except (TypeError, ValueError):
            raise ValueError(f"white_nits, peak_nits, knee and gamma are numbers, not {(white_nits, peak_nits, knee, gamma)!r}") from None
        if not (1.0 <= white_nits <= 10000.0 and white_nits <= peak_nits <= 10000.0):
            raise ValueError(f"white_nits {white_nits} and peak_nits {peak_nits} must be 1 <= white_nits <= peak_nits <= 10000")
        if not 0.0 < knee < 1.0:
            raise ValueError(f"knee {knee} must lie inside (0, 1)")
        if not 1.0 <= gamma <= 4.0:
            raise ValueError(f"gamma {gamma} must be 1..4")
        return super().__new__(cls, transfer, primaries, white_nits, peak_nits, curve, knee, gamma)

    def nits(self, e):
        """The signal 0..1 of one channel -> nits."""
        return pq_eotf(e) if self.transfer == "pq" else hlg_nits(e)

    def tone_curve(self, x):
        """Light relative to white_nits -> light relative to SDR white, 0..1."""
        x = np.asarray(x, np.float64)
        if self.curve == "clip":
            return np.minimum(x, 1.0)
        p = self.peak_nits / self.white_nits
        s = (p - self.knee) / (1.0 - self.knee)
        t = np.minimum(np.maximum(x - self.knee, 0.0) / (p - self.knee), 1.0)
        return np.where(x <= self.knee, x, self.knee + (1.0 - self.knee) * s * t / (1.0 + (s - 1.0) * t))

    def tables(self):
        """-> (A uint16[4096], T uint8[7936], M int32[3, 3]) of vse_yuv_to_bgr_tonemap, read-only, built once per map."""
        return _tone_tables(self)

    def packed(self):
        """The 16 128 bytes the device takes: A (little-endian), then T."""
        a, t, _ = self.tables()
        return a.astype("<u2").tobytes() + t.tobytes()


_TONE_TABLES = {}


def _tone_tables(tone):
    hit = _TONE_TABLES.get(tone)
    if hit is None:
        code = np.minimum(np.arange(TONE_CODES, dtype=np.float64) / TONE_PEAK_CODE, 1.0)
        a = np.round(65535.0 * tone.tone_curve(tone.nits(code) / tone.white_nits)).astype(np.uint16)
        j = np.arange(TONE_GAMMA_ENTRIES, dtype=np.float64)
        lin = np.where(j < 4096, j, (j - 3840.0) * 16.0 + 8.0) / 65535.0
        t = np.round(255.0 * np.power(lin, 1.0 / tone.gamma)).astype(np.uint8)
        if tone.primaries == "bt709":
            m = np.eye(3, dtype=np.int32) * 16384
        else:
            m = np.round(16384.0 * bt2020_to_bt709()).astype(np.int32)
            for r in range(3):
                m[r, r] += 16384 - int(m[r].sum())            # every row sums to exactly 1: grey stays grey
        check_gamut(m)
        for arr in (a, t, m):
            arr.setflags(write=False)
        hit = _TONE_TABLES[tone] = (a, t, m)
    return hit


def check_gamut(m):
    """The bounds vse_yuv_to_bgr_tonemap puts on M (int32 stays exact): per row, positive entries sum to <= 32767, negative ones to >= -32768."""
    m = np.asarray(m, np.int64).reshape(3, 3)
    for r in range(3):
        if m[r][m[r] > 0].sum() > 32767 or m[r][m[r] < 0].sum() < -32768:
            raise ValueError(f"gamut row {r} {m[r].tolist()}: positive entries may sum to at most 32767, negative ones to at least -32768")
    return m


def _check_tone(tone):
    if tone is not None and not (hasattr(tone, "tables") and hasattr(tone, "packed")):
        raise ValueError(f"tone must be None or a ToneMap, not {tone!r}")
    return tone


def _source_tone(name, transfer, tone_params, matrix, takes):
    """The ToneMap a YUV source attaches to its frames (None without transfer).  primaries default to the matrix's.  takes: whether the
    source yields YuvFrames."""
    if transfer is None:
        if tone_params:
            raise ValueError(f"{name}: tone_params {sorted(tone_params)} belong to transfer='pq' | 'hlg'")
        return None
    if transfer not in TONE_TRANSFERS:
        raise ValueError(f"{name}: transfer must be None or one of {TONE_TRANSFERS}, not {transfer!r}")
    if not takes:
        raise ValueError(f"{name}: transfer={transfer!r} needs wide=True or pix_fmt (the frames are YuvFrames; 8-bit 4:2:0 Yuv420Frames "
                         "and BGR sources carry no tone map)")
    params = dict(tone_params or {})
    unknown = set(params) - set(ToneMap._fields[1:])
    if unknown:
        raise ValueError(f"{name}: tone_params takes {ToneMap._fields[1:]}, not {sorted(unknown)}")
    params.setdefault("primaries", "bt2020" if matrix == "bt2020" else "bt709")
    return ToneMap(transfer, **params)


# ---- anamorphic pictures -> square pixels (vse_yuv_resample) -------------------------------------------------------------------------
RESAMPLE_FILTERS = ("bicubic", "bilinear", "lanczos")
RESAMPLE_MAX_TAPS = 16
_FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0, "lanczos": 3.0}
_log = logging.getLogger(__name__)


def display_width(width, num, den):
    """The columns a picture of `width` stored columns is shown with at the sample aspect ratio num:den: the nearest even number."""
    return 2 * ((int(width) * int(num) + int(den)) // (2 * int(den)))


def _filter_kernel(name, t):
    a = np.abs(np.asarray(t, np.float64))
    if name == "bilinear":
        return np.maximum(1.0 - a, 0.0)
    if name == "bicubic":                 # Catmull-Rom: B = 0, C = 1/2
        return np.where(a < 1.0, (1.5 * a - 2.5) * a * a + 1.0, np.where(a < 2.0, ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0, 0.0))
    return np.where(a < 3.0, np.sinc(a) * np.sinc(a / 3.0), 0.0)


def resample_taps(pw_in, pw_out, name):
    """The taps a table of `name` from pw_in to pw_out columns needs: the smallest even number >= 2 support max(1, pw_in / pw_out)."""
    need = int(np.ceil(2.0 * _FILTER_SUPPORT[name] * max(1.0, pw_in / pw_out)))
    return need + (need & 1)


def _check_taps(pw_in, pw_out, name):
    taps = resample_taps(pw_in, pw_out, name)
    if taps > RESAMPLE_MAX_TAPS:
        raise ValueError(f"resample filter {name!r} from {pw_in} to {pw_out} columns needs {taps} taps, more than the {RESAMPLE_MAX_TAPS} "
                         "the device takes: choose a narrower filter or a smaller reduction")
    return taps


def check_resample_table(left, coef):
    """The bounds vse_yuv_resample's int32 sums rest on: taps even and 2..16, |left| <= 2^30, every row's sum of |coef| <= 32767."""
    left, coef = np.asarray(left), np.asarray(coef)
    if coef.ndim != 2 or left.shape != coef.shape[:1] or coef.shape[1] % 2 or not 2 <= coef.shape[1] <= RESAMPLE_MAX_TAPS:
        raise ValueError(f"a resample table is left[P] and coef[P][K] with K even and 2..{RESAMPLE_MAX_TAPS}, not {left.shape} and {coef.shape}")
    worst = int(np.abs(coef.astype(np.int64)).sum(axis=1).max())
    if worst > 32767 or int(np.abs(left.astype(np.int64)).max()) > 1 << 30:
        raise ValueError(f"a resample table's rows may sum to at most 32767 in absolute values (here {worst}) and |left| <= 2^30")


def resample_table(pw_in, pw_out, name):
    """-> (left int32[pw_out], coef int16[pw_out, K]) of include/vse_hip.h vse_yuv_resample for one plane, built in float64: centre c =
    (x + 1/2) pw_in / pw_out - 1/2, the filter stretched by max(1, pw_in / pw_out), left = floor(c - support stretch) + 1, the weights
    normalised, rounded to Q14 and the rounding remainder added to the largest tap, so that every row sums to exactly 16384."""
    taps = _check_taps(pw_in, pw_out, name)
    stretch = max(1.0, pw_in / pw_out)
    c = (np.arange(pw_out, dtype=np.float64) + 0.5) * pw_in / pw_out - 0.5
    left = np.floor(c - _FILTER_SUPPORT[name] * stretch).astype(np.int64) + 1
    w = _filter_kernel(name, (left[:, None] + np.arange(taps)[None, :] - c[:, None]) / stretch)
    w /= w.sum(axis=1, keepdims=True)
    q = np.rint(w * 16384.0).astype(np.int64)
    q[np.arange(pw_out), np.argmax(w, axis=1)] += 16384 - q.sum(axis=1)
    left, coef = left.astype(np.int32), q.astype(np.int16)
    check_resample_table(left, coef)
    for a in (left, coef):
        a.setflags(write=False)
    return left, coef


def resample_rows(rows, left, coef, comps=1, shift=0, maxv=255):
    """The arithmetic of vse_yuv_resample on rows [r, pw * comps] of stored words (comps 2: an interleaved UV plane) -> [r, P * comps] of
    the same dtype: acc = sum coef[x][k] S[clamp(left[x] + k, 0, pw - 1)], out = clip(0, maxv, (acc + 8192) >> 14), S = word >> shift and
    the result << shift."""
    rows = np.asarray(rows)
    s = rows.astype(np.int32) >> shift
    pw = s.shape[1] // comps
    out = np.empty((s.shape[0], len(left) * comps), rows.dtype)
    idx = np.clip(left.astype(np.int64)[:, None] + np.arange(coef.shape[1])[None, :], 0, pw - 1)
    for e in range(comps):
        acc = np.zeros((s.shape[0], len(left)), np.int32)
        for k in range(coef.shape[1]):
            acc += s[:, idx[:, k] * comps + e] * coef[:, k].astype(np.int32)
        out[:, e::comps] = np.clip((acc + np.int32(8192)) >> 14, 0, maxv) << shift
    return out


_RESAMPLE_TABLES = {}


class Resample(namedtuple("Resample", "in_width out_width filter")):
    """How pictures of in_width stored columns become pictures of out_width columns (anamorphic video shown with square pixels): the data
    of include/vse_hip.h vse_yuv_resample.  filter "bicubic" (Catmull-Rom) | "bilinear" | "lanczos" (a = 3).  A tuple: equal resamples
    compare and hash equal, and the tables are built once per distinct one.  ValueError when the filter needs more than 16 taps."""
    __slots__ = ()

    def __new__(cls, in_width, out_width, filter="bicubic"):
        if filter not in RESAMPLE_FILTERS:
            raise ValueError(f"resample filter must be one of {RESAMPLE_FILTERS}, not {filter!r}")
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in (in_width, out_width)):
            raise ValueError(f"a resample takes widths of at least 1 column, not {in_width!r} -> {out_width!r}")
        self = super().__new__(cls, int(in_width), int(out_width), filter)
        _check_taps(self.in_width, self.out_width, filter)
        return self

    @classmethod
    def from_sar(cls, width, num, den, filter="bicubic"):
        """The resample that shows `width` stored columns at the sample aspect ratio num:den (display_width)."""
        out = display_width(width, num, den)
        if out < 2:
            raise ValueError(f"sample aspect ratio {num}:{den} shows {width} columns as {out}")
        return cls(width, out, filter)

    def tables(self, fmt):
        """-> ((left, coef) of luma, (left, coef) of the chroma planes or None for grey), read-only (resample_table)."""
        key = (self, fmt.sub_x, bool(fmt.chroma))
        hit = _RESAMPLE_TABLES.get(key)
        if hit is None:
            chroma = None
            if fmt.chroma:
                chroma = resample_table(fmt.chroma_size(1, self.in_width)[1], fmt.chroma_size(1, self.out_width)[1], self.filter)
            hit = _RESAMPLE_TABLES[key] = (resample_table(self.in_width, self.out_width, self.filter), chroma)
        return hit

    def packed(self, fmt):
        """The tables as the device takes them: (luma bytes, chroma bytes or None), each left (little-endian int32) then coef (int16)."""
        return tuple(None if t is None else t[0].astype("<i4").tobytes() + t[1].astype("<i2").tobytes() for t in self.tables(fmt))

    def planes(self, fmt, planes):
        """Plane rows of `fmt` (stored words) -> the same rows resampled, by the integers of vse_yuv_resample in numpy."""
        shift, maxv = (16 - fmt.depth if fmt.msb else 0), (1 << fmt.depth) - 1
        luma, chroma = self.tables(fmt)
        return tuple(resample_rows(p, *(chroma if k else luma), comps=2 if k and fmt.chroma == 2 else 1, shift=shift, maxv=maxv)
                     for k, p in enumerate(planes))


# ---- UHD and other oversized pictures -> fewer rows (vse_yuv_vscale) ------------------------------------------------------------------
def vscale_rows(plane, top, coef, r0, r1, shift=0, maxv=255):
    """The arithmetic of vse_yuv_vscale on one whole stored plane [ph, row samples] -> rows [r0, r1) of the output plane, same dtype: acc
    = sum coef[y][k] S[clamp(top[y] + k, 0, ph - 1)], out = clip(0, maxv, (acc + 8192) >> 14), S = word >> shift and the result << shift."""
    plane = np.asarray(plane)
    s = plane.astype(np.int32) >> shift
    idx = np.clip(top[r0:r1].astype(np.int64)[:, None] + np.arange(coef.shape[1])[None, :], 0, s.shape[0] - 1)
    acc = np.zeros((max(r1 - r0, 0), s.shape[1]), np.int32)
    for k in range(coef.shape[1]):
        acc += s[idx[:, k]] * coef[r0:r1, k].astype(np.int32)[:, None]
    return (np.clip((acc + np.int32(8192)) >> 14, 0, maxv) << shift).astype(plane.dtype)


def table_support(top, coef, ph):
    """-> (lo int64[Q], hi int64[Q]): the stored rows [lo[y], hi[y]) of a plane of ph rows that output row y of a vertical table reads with
    a coefficient other than zero, after the clamp to the picture; lo = ph and hi = 0 for a row whose coefficients are all zero."""
    top, coef = np.asarray(top, np.int64), np.asarray(coef)
    idx = np.clip(top[:, None] + np.arange(coef.shape[1])[None, :], 0, ph - 1)
    used = coef != 0
    return np.where(used, idx, ph).min(axis=1), np.where(used, idx + 1, 0).max(axis=1)


def band_for_support(spans, sub_y, height):
    """spans: [(lo, hi) of luma rows, (lo, hi) of chroma rows or None], each the union of a band's support in whole-picture rows of its
    plane (lo >= hi: nothing is read) -> (s0, s1), the smallest band of stored luma rows whose luma rows [s0, s1) and chroma rows [s0 >>
    sub_y, ((s1 - 1) >> sub_y) + 1) hold both; (0, 1) where nothing is read at all."""
    (lo, hi), chroma = spans[0], spans[1]
    if chroma is not None and chroma[0] < chroma[1]:
        c_lo, c_hi = (chroma[0] << sub_y) + sub_y, ((chroma[1] - 1) << sub_y) + 1          # the last s0 and the first s1 that hold them
        lo, hi = (min(lo, c_lo), max(hi, c_hi)) if lo < hi else (c_lo, c_hi)
    if lo >= hi:
        return 0, 1
    return int(lo), int(min(hi, height))


_VSCALE_TABLES = {}


class VScale(namedtuple("VScale", "in_height out_height filter")):
    """How pictures of in_height stored rows become pictures of out_height rows (UHD and other oversized video): the data of
    include/vse_hip.h vse_yuv_vscale.  The tables are resample_table(in_height, out_height, filter) and the same over the chroma heights:
    same centres, stretch, Q14 rounding and rows summing to 16384 as the horizontal Resample's.  A tuple: equal scales compare and hash
    equal, and the tables are built once per distinct one.  ValueError when the filter needs more than 16 taps."""
    __slots__ = ()

    def __new__(cls, in_height, out_height, filter="bicubic"):
        if filter not in RESAMPLE_FILTERS:
            raise ValueError(f"vscale filter must be one of {RESAMPLE_FILTERS}, not {filter!r}")
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in (in_height, out_height)):
            raise ValueError(f"a vscale takes heights of at least 1 row, not {in_height!r} -> {out_height!r}")
        self = super().__new__(cls, int(in_height), int(out_height), filter)
        _check_taps(self.in_height, self.out_height, filter)
        return self

    def tables(self, fmt):
        """-> ((top, coef) of luma, (top, coef) of the chroma planes or None for grey), read-only (resample_table over the rows)."""
        key = (self, fmt.sub_y, bool(fmt.chroma))
        hit = _VSCALE_TABLES.get(key)
        if hit is None:
            chroma = None
            if fmt.chroma:
                chroma = resample_table(fmt.chroma_size(self.in_height, 1)[0], fmt.chroma_size(self.out_height, 1)[0], self.filter)
            hit = _VSCALE_TABLES[key] = (resample_table(self.in_height, self.out_height, self.filter), chroma)
        return hit

    def packed(self, fmt):
        """The tables as the device takes them: (luma bytes, chroma bytes or None), each top (little-endian int32) then coef (int16)."""
        return tuple(None if t is None else t[0].astype("<i4").tobytes() + t[1].astype("<i2").tobytes() for t in self.tables(fmt))

    def _chroma_rows(self, fmt, y0, y1):
        return y0 >> fmt.sub_y, (((y1 - 1) >> fmt.sub_y) + 1 if y1 > y0 else y0 >> fmt.sub_y)

    def planes(self, fmt, planes, y0=0, y1=None):
        """The whole stored planes of a picture of `fmt` (stored words, in_height rows) -> the planes of the packed band of output rows
        [y0, y1): luma rows y0..y1 and chroma rows y0 >> sub_y .. ((y1 - 1) >> sub_y) + 1, by the integers of vse_yuv_vscale in numpy."""
        y1 = self.out_height if y1 is None else y1
        shift, maxv = (16 - fmt.depth if fmt.msb else 0), (1 << fmt.depth) - 1
        luma, chroma = self.tables(fmt)
        c0, c1 = self._chroma_rows(fmt, y0, y1)
        return tuple(vscale_rows(p, *(chroma if k else luma), *((c0, c1) if k else (y0, y1)), shift=shift, maxv=maxv) for k, p in enumerate(planes))

    def source_rows(self, fmt, y0, y1):
        """-> (s0, s1): the smallest band of stored luma rows whose luma rows and chroma rows (s0 >> sub_y .. ((s1 - 1) >> sub_y) + 1) hold
        every row that output rows [y0, y1) read with a coefficient other than zero, in every plane."""
        if not 0 <= y0 < y1 <= self.out_height:
            return 0, 0
        luma, chroma = self.tables(fmt)
        spans = []
        for tab, ph, (a, b) in ((luma, self.in_height, (y0, y1)),
                                (chroma, fmt.chroma_size(self.in_height, 1)[0] if fmt.chroma else 0, self._chroma_rows(fmt, y0, y1))):
            if tab is None:
                spans.append(None)
                continue
            lo, hi = table_support(tab[0][a:b], tab[1][a:b], ph)
            spans.append((int(lo.min()), int(hi.max())))
        return band_for_support(spans, fmt.sub_y, self.in_height)


def _check_vscale(vscale, height):
    if vscale is not None:
        if not (hasattr(vscale, "tables") and hasattr(vscale, "packed") and hasattr(vscale, "out_height") and hasattr(vscale, "source_rows")):
            raise ValueError(f"vscale must be None or a VScale, not {vscale!r}")
        if vscale.in_height != height:
            raise ValueError(f"the vscale is for {vscale.in_height} stored rows, the picture has {height}")
    return vscale


def _check_resample(resample, width):
    if resample is not None:
        if not (hasattr(resample, "tables") and hasattr(resample, "packed") and hasattr(resample, "out_width")):
            raise ValueError(f"resample must be None or a Resample, not {resample!r}")
        if resample.in_width != width:
            raise ValueError(f"the resample is for {resample.in_width} stored columns, the picture has {width}")
    return resample


def parse_y4m_aspect(line):
    """The sample aspect ratio (num, den) of a YUV4MPEG2 stream header's A token; None without one, for A0:0 (unknown) and for anything
    that is not a ratio of integers."""
    for tok in (line or b"")[10:].decode("ascii", "replace").split():
        m = re.match(r"A(\d+):(\d+)$", tok)
        if m:
            num, den = int(m.group(1)), int(m.group(2))
            return (num, den) if num > 0 and den > 0 else None
    return None


def _check_sar(name, square_pixels, sar, resample_filter, scale=None):
    """The sources' options that resample, checked -> whether square_pixels / sar is on."""
    if resample_filter not in RESAMPLE_FILTERS:
        raise ValueError(f"{name}: resample_filter must be one of {RESAMPLE_FILTERS}, not {resample_filter!r}")
    if sar is not None:
        if (not isinstance(sar, (tuple, list)) or len(sar) != 2
                or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in sar)):
            raise ValueError(f"{name}: sar must be None or (num, den) of positive integers, not {sar!r}")
    if scale is not None:
        sizes = scale if isinstance(scale, (tuple, list)) else (scale,)
        if not 1 <= len(sizes) <= 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in sizes):
            raise ValueError(f"{name}: scale must be None, a height or (width, height) of positive integers, not {scale!r}")
    if not (square_pixels or sar is not None or scale is not None) and resample_filter != "bicubic":
        raise ValueError(f"{name}: resample_filter belongs to square_pixels=True, sar=(num, den) or scale=")
    return bool(square_pixels) or sar is not None


def _y4m_size_token(line, letter):
    """The W or H token of a YUV4MPEG2 stream header as an integer; None where the header has none (its parser then says so)."""
    for tok in (line or b"")[10:].decode("ascii", "replace").split():
        if tok[0] == letter and tok[1:].isdigit():
            return int(tok[1:])
    return None


def _y4m_width(line):
    return _y4m_size_token(line, "W")


def _y4m_height(line):
    return _y4m_size_token(line, "H")


def _source_resample(name, width, header, square_pixels, sar, resample_filter, scale=None):
    """The one decision of a source's three options: the Resample its frames carry, from sar, else with square_pixels from the header's
    ratio; None with the option off, and None with exactly one log line where it is on and there is nothing to do: no ratio, 1:1, or a
    ratio that shows the stored width.  width None (a header without one): None, the header's parser refuses it."""
    if not _check_sar(name, square_pixels, sar, resample_filter, scale) or not width:
        return None
    ratio = tuple(int(v) for v in sar) if sar is not None else header
    if ratio is None or ratio[0] == ratio[1]:
        _log.info("%s: %s: the frames are left as stored", name, "no sample aspect ratio" if ratio is None else "square pixels (1:1)")
        return None
    r = Resample.from_sar(width, ratio[0], ratio[1], resample_filter)
    if r.out_width == width:
        _log.info("%s: sample aspect ratio %d:%d shows %d columns as %d: the frames are left as stored", name, ratio[0], ratio[1], width, width)
        return None
    return r


def _source_scale(name, width, height, header, square_pixels, sar, resample_filter, scale, deinterlace=None):
    """The one decision of a source's scale= beside its square_pixels / sar -> (the VScale, the Resample) its frames carry.  scale None:
    (None, _source_resample's).  scale=H keeps the display aspect: the width is the nearest even number to display width * H / height,
    the display width being the stored one or the one square_pixels / sar gives; scale=(W, H) says both.  One horizontal table goes from
    the stored width straight to W.  A scale that asks for the size the picture already has attaches nothing and logs exactly one line.
    width or height None (a header without one): nothing, the header's parser refuses it."""
    square = _source_resample(name, width, header, square_pixels, sar, resample_filter, scale)
    if scale is None:
        return None, square
    if deinterlace is not None:
        raise ValueError(f"{name}: scale does not go with deinterlace={deinterlace!r}: interlaced pictures are not scaled vertically")
    if not width or not height:
        return None, None
    shown = width if square is None else square.out_width
    if isinstance(scale, (tuple, list)) and len(scale) == 2:
        out_w, out_h = int(scale[0]), int(scale[1])
    else:
        out_h = int(scale[0] if isinstance(scale, (tuple, list)) else scale)
        out_w = max(2, 2 * ((shown * out_h + height) // (2 * height)))
    vscale = VScale(height, out_h, resample_filter) if out_h != height else None
    resample = Resample(width, out_w, resample_filter) if out_w != width else None
    if vscale is None and resample is None:
        _log.info("%s: scale to %d x %d is the stored size: the frames are left as stored", name, out_w, out_h)
    return vscale, resample


class YuvFrame:
    """Yuv420Frame for any YuvFormat `fmt`: rows [y0, y1) of one picture that has not been converted.  planes are views of samples (uint8,
    or little-endian uint16 above 8 bits) of fmt.plane_shapes(height, width).  shape == (y1 - y0, width, 3), frame[a:b] narrows the row
    range, to_bgr() gives the uint8 BGR ndarray by the integers of vse_yuv_to_bgr_format, pack_into() the packed sub-frame it takes.
    tone: a ToneMap; to_bgr() and the device then convert by the integers of vse_yuv_to_bgr_tonemap; it travels with the slices.
    resample: a Resample whose in_width is `width` (anamorphic video): every plane's rows are resampled to resample.out_width columns by
    the integers of vse_yuv_resample before the conversion, on the host in to_bgr() and on the device in staging.Uploader; shape then
    reports the output width, while width, the planes and the packing stay the stored ones.
    vscale: a VScale whose in_height is `height` (UHD and other oversized video): every plane is scaled down its columns by the integers of
    vse_yuv_vscale first (vertical, then horizontal, then the conversion).  shape, y0, y1 and frame[a:b] then count OUTPUT rows; height,
    width, the planes and the packing stay the stored ones: band() is the stored rows that output rows [y0, y1) need, and packed_bytes,
    pack_into() and row_parity describe that band.  f[a:b].to_bgr() == f.to_bgr()[a:b] for every slice."""

    def __init__(self, planes, height, width, fmt, y0=0, y1=None, tone=None, resample=None, vscale=None):
        if not isinstance(fmt, YuvFormat):
            raise ValueError(f"fmt must be a YuvFormat, not {fmt!r}")
        self.tone = _check_tone(tone)
        self.resample = _check_resample(resample, int(width))
        self.vscale = _check_vscale(vscale, int(height))
        self.planes, self.height, self.width, self.fmt = tuple(planes), int(height), int(width), fmt
        rows = self.height if vscale is None else int(vscale.out_height)           # y0, y1 count output rows
        self.y0, self.y1 = int(y0), int(rows if y1 is None else y1)
        want = fmt.plane_shapes(self.height, self.width)
        if ([tuple(p.shape) for p in self.planes] != want or any(p.dtype.itemsize != fmt.sample_bytes or p.dtype.kind != "u" for p in self.planes)
                or not 0 <= self.y0 <= self.y1 <= rows):
            raise ValueError(f"the planes of a {self.height} x {self.width} picture of {fmt} are {want} of {fmt.sample_dtype}, rows "
                             f"{self.y0}:{self.y1} asked of {[(tuple(p.shape), str(p.dtype)) for p in self.planes]}")

    @property
    def shape(self):
        return (self.y1 - self.y0, self.width if self.resample is None else self.resample.out_width, 3)

    @property
    def matrix(self):
        return self.fmt.matrix

    def __getitem__(self, idx):
        if not isinstance(idx, slice):
            raise TypeError(f"a YuvFrame takes one row slice, not {idx!r}")
        a, b, step = idx.indices(self.y1 - self.y0)
        if step != 1:
            raise TypeError(f"a YuvFrame takes a row slice of step 1, not {idx!r}")
        return YuvFrame(self.planes, self.height, self.width, self.fmt, self.y0 + a, self.y0 + max(a, b), self.tone, self.resample, self.vscale)

    def _stored_rows(self):          # (InterlacedYuvFrame has a band() of its own; this is what the packing of THIS class goes by)
        return (self.y0, self.y1) if self.vscale is None else self.vscale.source_rows(self.fmt, self.y0, self.y1)

    def band(self):
        """(a, b): the stored luma rows packed for the device: [y0, y1) itself, or with a vscale the smallest band that holds what output
        rows [y0, y1) read in every plane (VScale.source_rows)."""
        return self._stored_rows()

    @property
    def row_parity(self):
        return self._stored_rows()[0] & self.fmt.sub_y

    def _chroma_rows(self):
        a, b = self._stored_rows()
        c0 = a >> self.fmt.sub_y
        return c0, (((b - 1) >> self.fmt.sub_y) + 1 if b > a else c0)

    @property
    def packed_bytes(self):
        (a, b), (c0, c1) = self._stored_rows(), self._chroma_rows()
        return self.fmt.sample_bytes * ((b - a) * self.width + sum((c1 - c0) * p.shape[1] for p in self.planes[1:]))

    def pack_into(self, dst_u8):
        """The packed sub-frame (luma rows y0..y1, then chroma rows y0 >> sub_y .. ((y1 - 1) >> sub_y) + 1 of each plane; row parity
        y0 & sub_y; with a vscale the same of band() in y0, y1's place) into the first packed_bytes bytes of the 1-D uint8 array dst_u8:
        one contiguous copy per plane, the samples as they are (2 bytes each above 8 bits)."""
        c0, c1 = self._chroma_rows()
        pos = 0
        for plane, (a, b) in zip(self.planes, [self._stored_rows()] + [(c0, c1)] * (len(self.planes) - 1)):
            part = plane[a:b]
            nbytes = part.size * part.dtype.itemsize
            np.copyto(dst_u8[pos:pos + nbytes].view(part.dtype).reshape(part.shape), part)
            pos += nbytes
        return pos

    def to_bgr(self):
        """uint8 BGR [y1 - y0, W, 3]: nearest chroma, the integers of vse_yuv_to_bgr_format (include/vse_hip.h) in int32, or with a
        tone those of vse_yuv_to_bgr_tonemap; with a resample the rows of every plane go through the integers of vse_yuv_resample first,
        and with a vscale the columns go through those of vse_yuv_vscale before that: vertical, then horizontal, then the conversion."""
        if self.vscale is not None:
            rows, width = self.vscale.planes(self.fmt, self.planes, self.y0, self.y1), self.width
            if self.resample is not None:
                rows, width = self.resample.planes(self.fmt, rows), self.resample.out_width
            return _rows_to_bgr(self.fmt, rows[0], rows[1:], (np.arange(self.y0, self.y1) >> self.fmt.sub_y) - (self.y0 >> self.fmt.sub_y), width,
                                self.tone)
        if self.resample is not None:
            c0, c1 = self._chroma_rows()
            rows = self.resample.planes(self.fmt, (self.planes[0][self.y0:self.y1],) + tuple(p[c0:c1] for p in self.planes[1:]))
            return _rows_to_bgr(self.fmt, rows[0], rows[1:], (np.arange(self.y0, self.y1) >> self.fmt.sub_y) - c0, self.resample.out_width,
                                self.tone)
        return _rows_to_bgr(self.fmt, self.planes[0][self.y0:self.y1], self.planes[1:], np.arange(self.y0, self.y1) >> self.fmt.sub_y, self.width,
                            self.tone)


def _rows_to_bgr(fmt, luma, chroma, rows, width, tone=None):
    """YuvFrame.to_bgr on luma rows `luma` [n, width] whose chroma stands in row rows[k] of the planes `chroma` -> uint8 BGR [n, width, 3]."""
    shift, maxv, yoff, coff, ky, bu, gu, gv, rv = fmt.factors()
    half, down, top = (1 << 19, 20, 255) if tone is None else (1 << 15, 16, TONE_CODES - 1)

    def samples(a):
        return np.minimum(np.asarray(a).astype(np.int32) >> shift, maxv)
    c = np.maximum(samples(luma) - yoff, 0) * np.int32(ky) + np.int32(half)
    if fmt.chroma == 0:
        codes = [np.clip(c >> down, 0, top)] * 3
    else:
        cols = np.arange(width) >> fmt.sub_x
        if fmt.chroma == 1:
            u, v = (samples(np.asarray(p)[rows][:, cols]) - coff for p in chroma)
        else:
            uv = np.asarray(chroma[0])[rows]
            u, v = samples(uv[:, 2 * cols]) - coff, samples(uv[:, 2 * cols + 1]) - coff
        codes = [np.clip((c + np.int32(bu) * u) >> down, 0, top), np.clip((c + np.int32(gu) * u + np.int32(gv) * v) >> down, 0, top),
                 np.clip((c + np.int32(rv) * v) >> down, 0, top)]
    out = np.empty((len(rows), width, 3), np.uint8)
    if tone is None:
        for k in range(3):
            out[..., k] = codes[k]
        return out
    # vse_yuv_to_bgr_tonemap: A, the gamut matrix in linear light (rows and columns R G B; the codes are B G R), T; int32 throughout
    table_a, table_t, m = tone.tables()
    lb, lg, lr = (table_a[e].astype(np.int32) for e in codes)
    for k, r in ((2, 0), (1, 1), (0, 2)):
        p = np.clip((np.int32(m[r][0]) * lr + np.int32(m[r][1]) * lg + np.int32(m[r][2]) * lb + np.int32(1 << 13)) >> 14, 0, 65535)
        out[..., k] = table_t[np.where(p < 4096, p, 3840 + (p >> 4))]
    return out


# ---- interlaced pictures (vse_yuv_deinterlace) ----------------------------------------------------------------------------------------
DEINTERLACE_MODES = ("adaptive", "interpolate", "match")
FIELD_ORDERS = ("tff", "bff")
MATCH_CHOICES = ("c", "p1", "p2", "adaptive")          # vse_yuv_field_match's choices 0..3


def _check_match(comb_thresh, comb_limit):
    """mode "match"'s comb threshold (8-bit levels) and fallback limit (per mille of the luma samples tested; None: never fall back)
    -> (comb_thresh, comb_limit) as integers."""
    if isinstance(comb_thresh, bool) or not isinstance(comb_thresh, (int, np.integer)) or not 0 <= comb_thresh <= 255:
        raise ValueError(f"the comb threshold is an integer of 0..255 (8-bit levels), not {comb_thresh!r}")
    if comb_limit is not None and (isinstance(comb_limit, bool) or not isinstance(comb_limit, (int, np.integer)) or not 0 <= comb_limit <= 1000):
        raise ValueError(f"the comb limit is None or an integer of 0..1000 (per mille), not {comb_limit!r}")
    return int(comb_thresh), None if comb_limit is None else int(comb_limit)


def comb_count(mid, above, below, t):
    """How many samples of the rows `mid` stand out of the rows above and below them by more than t, the same way (int64 arrays of one
    shape): the comb test of include/vse_hip.h vse_yuv_field_match."""
    d1, d2 = mid - above, mid - below
    return int(np.count_nonzero(((d1 > t) & (d2 > t)) | ((d1 < -t) & (d2 < -t))))


def field_match_counts(cur, prev, keep, t):
    """The comb counts (c, p1, p2) of vse_yuv_field_match's three candidates over the luma rows `cur` of a picture (or band) and `prev` of
    the previous one (None: (c, 0, 0)), whose row 0 is a top-field row; t in word units."""
    rows = cur.shape[0]
    if rows < 3:
        return 0, 0, 0
    c = np.asarray(cur).astype(np.int64)
    counts = [comb_count(c[1:-1], c[:-2], c[2:], t), 0, 0]
    if prev is not None:
        p = np.asarray(prev).astype(np.int64)
        first = (np.arange(rows) & 1) == keep                  # the rows of the field first in time
        for k, own in ((1, first), (2, ~first)):               # p1: those rows from the picture; p2: the other rows
            w = np.where(own[:, None], c, p)
            counts[k] = comb_count(w[1:-1], w[:-2], w[2:], t)
    return tuple(counts)


def field_match_choice(counts, rows, width, comb_limit, paired=True):
    """vse_yuv_field_match's choice 0..3 from the three counts: the smallest (ties: c, p1, p2; without a previous picture only c), or 3
    where it exceeds comb_limit per mille of width * (rows - 2) samples (None: never)."""
    best, choice = counts[0], 0
    for k in ((1, 2) if paired else ()):
        if counts[k] < best:
            best, choice = counts[k], k
    return 3 if comb_limit is not None and best * 1000 > comb_limit * width * (rows - 2) else choice


def _check_deinterlace(deinterlace, field_order, thresh, orders=("auto",) + FIELD_ORDERS):
    if deinterlace is not None and deinterlace not in DEINTERLACE_MODES:
        raise ValueError(f"deinterlace must be None or one of {DEINTERLACE_MODES}, not {deinterlace!r}")
    if field_order not in orders:
        raise ValueError(f"field_order must be one of {orders}, not {field_order!r}")
    if isinstance(thresh, bool) or int(thresh) != thresh or not 0 <= thresh <= 255:
        raise ValueError(f"the deinterlace threshold is an integer of 0..255 (8-bit levels), not {thresh!r}")
    return int(thresh)


def deinterlace_rows(cur, prev, keep, thresh_words, a=0, b=None):
    """Rows [a, b) of one plane deinterlaced by the rule of include/vse_hip.h vse_yuv_deinterlace: cur, prev (None: every sample moved)
    are the whole plane's stored words, keep the parity of the rows that stay, thresh_words the threshold T in word units."""
    rows = cur.shape[0]
    b = rows if b is None else b
    out = np.array(cur[a:b], copy=True)
    if rows == 1 or b <= a:
        return out
    lo, hi = max(a - 1, 0), min(b + 1, rows)
    c = np.asarray(cur[lo:hi]).astype(np.int32)
    moved = np.ones(c.shape, bool) if prev is None else np.abs(c - np.asarray(prev[lo:hi]).astype(np.int32)) > thresh_words
    for y in range(a + ((a ^ keep ^ 1) & 1), b, 2):              # the rows of the other field
        up, down = (y - 1 if y >= 1 else y + 1), (y + 1 if y + 1 < rows else y - 1)
        m = moved[max(y - 1, 0) - lo:min(y + 1, rows - 1) + 1 - lo].any(axis=0)
        out[y - a] = np.where(m, (c[up - lo] + c[down - lo] + 1) >> 1, c[y - lo]).astype(out.dtype)
    return out


def _same_planes(a, b):
    """Whether two plane tuples are the same memory (views made twice of one buffer are)."""
    return a is b or (len(a) == len(b) and all(p.shape == q.shape and p.strides == q.strides and p.dtype == q.dtype
                                               and p.__array_interface__["data"][0] == q.__array_interface__["data"][0] for p, q in zip(a, b)))


class InterlacedYuvFrame(YuvFrame):
    """A YuvFrame whose picture is two woven fields: rows [y0, y1) of the picture vse_yuv_deinterlace makes of `planes` and `prev`, the
    plane tuple of the previous picture (None: the clip's first frame, interpolated throughout).  field_order "tff" | "bff" names the field
    that comes first in time (its rows are kept), mode is "adaptive" (weave what did not change by more than `thresh` 8-bit levels) or
    "interpolate".  frame[a:b] is the same class with the same prev; to_bgr() deinterlaces on the host by the same integers and converts
    as YuvFrame does, so f[a:b].to_bgr() == f.to_bgr()[a:b]; staging.Uploader deinterlaces and converts on the device.  With a resample
    (YuvFrame's) the order is deinterlace or match, then resample, then convert.
    mode "match" (film carried in interlaced video: 3:2 pulldown, shifted fields) follows vse_yuv_field_match instead: the whole frame is
    woven from its own fields or with a field of prev, whichever combs least by `comb_thresh` 8-bit levels (match_stats()), and a frame
    that combs by more than `comb_limit` per mille (None: never) with every partner is video and gets the adaptive rule with `thresh`.
    The counts are taken over the luma rows of band(), which is what the device is handed, so the host and the device agree; a slice may
    therefore choose differently from the whole frame, and f[a:b].to_bgr() == f.to_bgr()[a:b] is promised only where both make the same
    choice (always in a static band, where the candidates are equal)."""

    def __init__(self, planes, height, width, fmt, prev=None, field_order="tff", mode="adaptive", thresh=10, y0=0, y1=None, tone=None,
                 comb_thresh=10, comb_limit=20, resample=None, vscale=None):
        if vscale is not None:
            raise ValueError("an InterlacedYuvFrame takes no vscale: interlaced pictures are not scaled vertically")
        super().__init__(planes, height, width, fmt, y0, y1, tone, resample)
        self.thresh = _check_deinterlace(mode, field_order, thresh, FIELD_ORDERS)
        self.comb_thresh, self.comb_limit = _check_match(comb_thresh, comb_limit)
        self._stats = None
        if mode is None:
            raise ValueError(f"mode must be one of {DEINTERLACE_MODES}, not None")
        self.field_order, self.mode = field_order, mode
        self.prev = None if prev is None else tuple(prev)
        if self.prev is not None and [(tuple(p.shape), p.dtype.itemsize, p.dtype.kind) for p in self.prev] != \
                [(tuple(p.shape), p.dtype.itemsize, p.dtype.kind) for p in self.planes]:
            raise ValueError(f"the previous picture's planes {[(tuple(p.shape), str(p.dtype)) for p in self.prev]} are not the picture's "
                             f"{[(tuple(p.shape), str(p.dtype)) for p in self.planes]}")

    @property
    def keep(self):
        return FIELD_ORDERS.index(self.field_order)

    @property
    def thresh_words(self):
        return self.thresh << (self.fmt.depth - 8 + (16 - self.fmt.depth if self.fmt.msb else 0))

    def __getitem__(self, idx):
        if not isinstance(idx, slice):
            raise TypeError(f"an InterlacedYuvFrame takes one row slice, not {idx!r}")
        a, b, step = idx.indices(self.y1 - self.y0)
        if step != 1:
            raise TypeError(f"an InterlacedYuvFrame takes a row slice of step 1, not {idx!r}")
        return InterlacedYuvFrame(self.planes, self.height, self.width, self.fmt, self.prev, self.field_order, self.mode, self.thresh,
                                  self.y0 + a, self.y0 + max(a, b), self.tone, self.comb_thresh, self.comb_limit, self.resample)

    def match_stats(self):
        """mode "match": (count c, count p1, count p2, choice 0..3) of vse_yuv_field_match over the luma rows of band()."""
        if self.mode != "match":
            raise ValueError(f"match_stats() belongs to mode \"match\", not {self.mode!r}")
        if self._stats is None:
            a, b = self.band()
            t = self.comb_thresh << (self.fmt.depth - 8 + (16 - self.fmt.depth if self.fmt.msb else 0))
            counts = field_match_counts(self.planes[0][a:b], None if self.prev is None else self.prev[0][a:b], self.keep, t)
            self._stats = counts + (field_match_choice(counts, b - a, self.width, self.comb_limit, self.prev is not None),)
        return self._stats

    def _deinterlaced(self, k, a, b):
        if self.mode == "match":
            choice = self.match_stats()[3]
            if choice < 3:
                out = np.array(self.planes[k][a:b], copy=True)
                if choice:                                         # p1: the other field's rows from prev; p2: the first field's
                    rows = ((np.arange(a, a + len(out)) & 1) == self.keep) == (choice == 2)
                    out[rows] = self.prev[k][a:b][rows]
                return out
        prev = None if self.prev is None or self.mode == "interpolate" else self.prev[k]
        return deinterlace_rows(self.planes[k], prev, self.keep, self.thresh_words, a, b)

    def deinterlaced_planes(self):
        """The whole progressive picture's planes (not only rows [y0, y1)), in numpy by the rule."""
        return tuple(self._deinterlaced(k, 0, None) for k in range(len(self.planes)))

    def to_bgr(self):
        c0, c1 = self._chroma_rows()
        chroma = [self._deinterlaced(k, c0, c1) for k in range(1, len(self.planes))]
        luma, width = self._deinterlaced(0, self.y0, self.y1), self.width
        if self.resample is not None:                              # deinterlace or match, then resample, then convert
            rows = self.resample.planes(self.fmt, [luma] + chroma)
            luma, chroma, width = rows[0], rows[1:], self.resample.out_width
        return _rows_to_bgr(self.fmt, luma, chroma, (np.arange(self.y0, self.y1) >> self.fmt.sub_y) - c0, width, self.tone)

    def band(self):
        """(a, b): the rows packed for the device in place of [y0, y1): two more on either side, a rounded down to a multiple of 4 and b up to
        even (both inside the picture), so that every plane of the packed band begins on a top-field row and the rows that get the band's
        edge rule in place of the picture's are none of [y0, y1)."""
        a = max(0, self.y0 - 2) & ~3
        return a, min(self.height, (min(self.height, self.y1 + 2) + 1) & ~1)

    @property
    def band_bytes(self):
        return self._band_frame(*self.band()).packed_bytes

    def _band_frame(self, a, b, prev=False):
        return YuvFrame(self.prev if prev else self.planes, self.height, self.width, self.fmt, a, b)

    def pack_band_into(self, dst_u8, prev=False):
        """YuvFrame.pack_into of rows band() of the picture (prev: of the previous picture) -> bytes written."""
        return self._band_frame(*self.band(), prev=prev).pack_into(dst_u8)


def _planes_at(buf, off, height, width, fmt):
    """The planes of one packed picture of `fmt` that starts at byte `off` of the 1-D uint8 array buf, as views (2-byte samples need no
    alignment: numpy reads them where they are)."""
    planes = []
    for shp in fmt.plane_shapes(height, width):
        nbytes = shp[0] * shp[1] * fmt.sample_bytes
        planes.append(buf[off:off + nbytes].view(fmt.sample_dtype).reshape(shp))
        off += nbytes
    return tuple(planes)


def write_yuv(path, frames_planes, fmt, fps=None, y4m=False, interlace="p", aspect=(1, 1)):
    """Frames given as plane tuples of `fmt` (fmt.plane_shapes, samples as integers) -> a headerless file (`ffmpeg -f rawvideo -pix_fmt
    ...`), or with y4m=True and a frame rate the YUV4MPEG2 file `ffmpeg -f yuv4mpegpipe -strict -1` writes for that format (planar or grey,
    value in the low bits).  interlace: the header's I token, "p" progressive | "t" top field first | "b" bottom field first; aspect:
    its A token, the sample aspect ratio (num, den)."""
    if interlace not in ("p", "t", "b"):
        raise ValueError(f"interlace must be one of 'p', 't', 'b', not {interlace!r}")
    frames_planes = [tuple(np.ascontiguousarray(p, fmt.sample_dtype) for p in f) for f in frames_planes]
    h, w = frames_planes[0][0].shape
    with open(path, "wb") as fp:
        if y4m:
            if fmt.chroma == 2 or fmt.msb:
                raise ValueError(f"YUV4MPEG2 has no semi-planar or high-bit formats: {fmt}")
            rate = Fraction(fps).limit_denominator(100000)
            name = "mono" if fmt.chroma == 0 else {v: k for k, v in _SUBSAMPLING.items()}[fmt.sub_x, fmt.sub_y]
            if fmt.depth > 8:
                name += ("" if fmt.chroma == 0 else "p") + str(fmt.depth)
            elif name == "420":
                name = "420jpeg"
            fp.write(b"YUV4MPEG2 W%d H%d F%d:%d I%s A%d:%d C%s XCOLORRANGE=%s\n" % (w, h, rate.numerator, rate.denominator, interlace.encode(),
                                                                                   int(aspect[0]), int(aspect[1]), name.encode(),
                                                                                   b"FULL" if fmt.full_range else b"LIMITED"))
        for f in frames_planes:
            if [p.shape for p in f] != fmt.plane_shapes(h, w):
                raise ValueError(f"the planes of a {h} x {w} picture of {fmt} are {fmt.plane_shapes(h, w)}, got {[p.shape for p in f]}")
            if y4m:
                fp.write(b"FRAME\n")
            for p in f:
                fp.write(p.tobytes())


def bgr_to_yuv420(frame):
    """uint8 BGR [H,W,3] -> (Y [H,W], U [ch,cw], V [ch,cw]) uint8: plain BT.601 limited-range forward transform, chroma the mean of
    each 2 x 2 block (edge blocks of an odd size: of the pixels that exist).  Turns synthetic clips into test input; nothing is
    specified about its rounding."""
    f = np.asarray(frame, np.float64)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    h, w = b.shape
    ch, cw = _chroma_size(h, w)

    def mean2(p):
        q = np.pad(p, ((0, 2 * ch - h), (0, 2 * cw - w)), mode="edge")
        return q.reshape(ch, 2, cw, 2).mean(axis=(1, 3))
    y = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    u = 128.0 + mean2(-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    v = 128.0 + mean2(112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    return tuple(np.clip(np.rint(p), 16, hi).astype(np.uint8) for p, hi in ((y, 235), (u, 240), (v, 240)))


def _plane_bytes(frame_yuv, layout):
    y, u, v = (np.ascontiguousarray(p, np.uint8) for p in frame_yuv)
    ch, cw = _chroma_size(*y.shape)
    if u.shape != (ch, cw) or v.shape != (ch, cw):
        raise ValueError(f"chroma planes of a {y.shape[0]} x {y.shape[1]} picture are {ch} x {cw}, got {u.shape} and {v.shape}")
    if layout == "i420":
        return y.tobytes() + u.tobytes() + v.tobytes()
    if layout == "nv12":
        return y.tobytes() + np.stack([u, v], axis=2).tobytes()
    raise ValueError(f"layout must be one of {YUV_LAYOUTS}, not {layout!r}")


def write_y4m(path, frames_yuv, fps):
    """YUV4MPEG2 file (what `ffmpeg -pix_fmt yuv420p -f yuv4mpegpipe` writes) of (Y, U, V) plane triples."""
    frames_yuv = list(frames_yuv)
    h, w = np.asarray(frames_yuv[0][0]).shape
    rate = Fraction(fps).limit_denominator(100000)
    with open(path, "wb") as fp:
        fp.write(b"YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C420jpeg\n" % (w, h, rate.numerator, rate.denominator))
        for f in frames_yuv:
            if np.asarray(f[0]).shape != (h, w):
                raise ValueError("all frames of a Y4M file have one size")
            fp.write(b"FRAME\n" + _plane_bytes(f, "i420"))


def write_yuv420(path, frames_yuv, layout="i420"):
    """Headerless file of consecutive frames (`ffmpeg -f rawvideo -pix_fmt yuv420p` / `nv12`) of (Y, U, V) plane triples."""
    with open(path, "wb") as fp:
        for f in frames_yuv:
            fp.write(_plane_bytes(f, layout))


class _Yuv420FileSource:
    """The frame-source interface over a memory-mapped file whose frames start at self._offsets (packed I420 or NV12 pictures)."""

    matrix = "bt601"
    fmt = None                    # a YuvFormat: the frames are YuvFrames of it (YuvSource, Y4mSource(wide=True)); None: 8-bit 4:2:0 Yuv420Frames
    deinterlace = None            # "adaptive" | "interpolate" with field_order "tff" | "bff": the frames are InterlacedYuvFrames
    field_order = None
    deinterlace_thresh = 10
    comb_thresh, comb_limit = 10, 20      # deinterlace "match"'s (InterlacedYuvFrame)
    tone = None                   # a ToneMap (transfer="pq" | "hlg" on the readers of YuvFrames): the frames carry it
    resample = None               # a Resample (square_pixels=True | sar=(num, den) on the readers of YuvFrames): the frames carry it
    vscale = None                 # a VScale (scale=H | (W, H) on the same readers): the frames carry it
    _last = None                  # (frame number, planes) of the last read_raw: the next frame's prev is then the same views

    def _planes(self, frame_no):
        if self._last is None or self._last[0] != frame_no:
            self._last = (frame_no, _planes_at(self._buf, self._offsets[frame_no - 1], self.height, self.width, self.fmt))
        return self._last[1]

    def _map(self, path):
        self.path = path
        self._fp = open(path, "rb")
        size = os.fstat(self._fp.fileno()).st_size
        self._mm = mmap.mmap(self._fp.fileno(), 0, access=mmap.ACCESS_READ) if size else None
        self._buf = np.frombuffer(self._mm, np.uint8) if size else np.zeros(0, np.uint8)
        return size

    def _frame_bytes(self):
        if self.fmt is not None:
            return self.fmt.frame_bytes(self.height, self.width)
        ch, cw = _chroma_size(self.height, self.width)
        return self.height * self.width + 2 * ch * cw

    def read_raw(self, frame_no):
        """The planes of frame frame_no (1-based) as a Yuv420Frame of views into the mapping; None outside the clip."""
        if not 1 <= frame_no <= self.frame_count:
            return None
        h, w = self.height, self.width
        ch, cw = _chroma_size(h, w)
        off = self._offsets[frame_no - 1]
        if self.fmt is not None and self.field_order is not None:
            prev = self._planes(frame_no - 1) if frame_no > 1 else None
            return InterlacedYuvFrame(self._planes(frame_no), h, w, self.fmt, prev, self.field_order, self.deinterlace, self.deinterlace_thresh,
                                      tone=self.tone, comb_thresh=self.comb_thresh, comb_limit=self.comb_limit, resample=self.resample)
        if self.fmt is not None:
            return YuvFrame(_planes_at(self._buf, off, h, w, self.fmt), h, w, self.fmt, tone=self.tone, resample=self.resample, vscale=self.vscale)
        luma = self._buf[off:off + h * w].reshape(h, w)
        off += h * w
        if self.layout == "i420":
            planes = (luma, self._buf[off:off + ch * cw].reshape(ch, cw), self._buf[off + ch * cw:off + 2 * ch * cw].reshape(ch, cw))
        else:
            planes = (luma, self._buf[off:off + 2 * ch * cw].reshape(ch, 2 * cw))
        return Yuv420Frame(planes, h, w, self.layout, matrix=self.matrix)

    def read(self, frame_no):
        raw = self.read_raw(frame_no)
        return None if raw is None else raw.to_bgr()

    def frames(self):
        for no in range(1, self.frame_count + 1):
            yield self.read(no)

    def raw_frames(self):
        for no in range(1, self.frame_count + 1):
            yield self.read_raw(no)

    def pos_msec(self, frame_no):
        """As AviBgr24Source.pos_msec: the time stamp of the frame with 0-based index frame_no at a constant frame rate."""
        return None if not 0 <= frame_no < self.frame_count else frame_no * 1000.0 / self.fps

    def close(self):
        self._buf = self._last = None
        if self._mm is not None:
            try:
                self._mm.close()
            except BufferError:           # frames handed out still view the mapping: it goes when they do
                pass
            self._mm = None
        self._fp.close()


def parse_y4m_header(line, name, fps=None, what="file"):
    """The stream header `line` (bytes up to, not including, its newline; None when there is none within 4096 bytes) of the YUV4MPEG2
    file or stream `name` -> (width, height, fps).  8-bit 4:2:0 progressive limited-range only: the tokens W H F (F0:0 or none: pass
    fps) I (p, ? or absent) A (ignored) C (absent, 420, 420jpeg, 420mpeg2, 420paldv; the siting they name is ignored, see the module
    docstring) X... (ignored, except XCOLORRANGE=FULL, which is refused)."""
    if line is None or line[:10] != b"YUV4MPEG2 ":
        raise ValueError(f"{name}: not a YUV4MPEG2 {what}")
    width = height = rate = None
    for tok in line[10:].decode("ascii", "replace").split():
        key, val = tok[0], tok[1:]
        if key == "W":
            width = int(val)
        elif key == "H":
            height = int(val)
        elif key == "F":
            num, _, den = val.partition(":")
            if int(num) > 0 and int(den or 1) > 0:
                rate = int(num) / float(int(den or 1))
        elif key == "I":
            if val not in ("p", "?"):
                raise ValueError(f"{name}: interlaced video ({tok}) is not supported")
        elif key == "C":
            if val not in ("420", "420jpeg", "420mpeg2", "420paldv"):
                raise ValueError(f"{name}: chroma format {tok} is not supported, only 8-bit 4:2:0 (C420, C420jpeg, C420mpeg2, C420paldv)")
        elif tok == "XCOLORRANGE=FULL":
            raise ValueError(f"{name}: full-range video ({tok}) needs other conversion constants and is not supported")
    if not width or not height or width < 1 or height < 1:
        raise ValueError(f"{name}: the YUV4MPEG2 header carries no frame size")
    if fps is not None:
        rate = float(fps)
    if rate is None:
        raise ValueError(f"{name}: the YUV4MPEG2 header carries no frame rate (F0:0 or no F token): pass fps")
    return width, height, rate


def parse_y4m_header_wide(line, name, fps=None, what="file", matrix="bt601", range="auto"):
    """parse_y4m_header for what `ffmpeg -f yuv4mpegpipe` (with -strict -1 above 8 bits) writes -> (width, height, fps, YuvFormat): C420*,
    C422, C444 and Cmono, each also at 9, 10, 12, 14 or 16 bits, and XCOLORRANGE=FULL | LIMITED (range="limited" | "full" overrides the
    header's; "auto" without a token is limited).  Refused, naming the token: interlaced video (It, Ib, Im), C411, an alpha plane, any other
    C or XCOLORRANGE value and any parameter that is none of W H F I A C X."""
    return parse_y4m_header_fields(line, name, fps, what, matrix, range, None)[:4]


def parse_y4m_header_fields(line, name, fps=None, what="file", matrix="bt601", range="auto", field_order="auto"):
    """parse_y4m_header_wide for a reader that deinterlaces -> (width, height, fps, YuvFormat, order): order is "tff" | "bff" when the
    pictures are woven fields, None when they are progressive.  field_order "auto" takes the header's word: It is "tff", Ib "bff", Ip, I?
    and no I token progressive, and Im (mixed; the frames' own flags are not read) is refused; "tff" | "bff" say it in the header's place,
    whatever its I token (mis-flagged files).  field_order None refuses every interlaced header, as parse_y4m_header_wide does."""
    if line is None or line[:10] != b"YUV4MPEG2 ":
        raise ValueError(f"{name}: not a YUV4MPEG2 {what}")
    width = height = rate = c_token = range_token = order = None
    for tok in line[10:].decode("ascii", "replace").split():
        key, val = tok[0], tok[1:]
        if key == "W" and val.isdigit():
            width = int(val)
        elif key == "H" and val.isdigit():
            height = int(val)
        elif key == "F":
            num, _, den = val.partition(":")
            if not (num.isdigit() and (den or "1").isdigit()):
                raise ValueError(f"{name}: the frame rate {tok} is not a ratio of integers")
            if int(num) > 0 and int(den or 1) > 0:
                rate = int(num) / float(int(den or 1))
        elif key == "I":
            if val not in ("p", "?"):
                if field_order is None or val not in ("t", "b", "m"):
                    raise ValueError(f"{name}: interlaced video ({tok}) is not supported")
                if val == "m" and field_order == "auto":
                    raise ValueError(f"{name}: mixed interlacing ({tok}) names no field order: pass field_order \"tff\" or \"bff\"")
                order = {"t": "tff", "b": "bff"}.get(val)
        elif key == "C":
            c_token = tok
        elif tok.startswith("XCOLORRANGE="):
            range_token = tok
        elif key not in ("A", "X"):
            raise ValueError(f"{name}: the YUV4MPEG2 header's parameter {tok} is not known")
    try:
        fmt = YuvFormat.from_y4m_tokens(c_token, range_token, matrix, range)
    except ValueError as e:
        raise ValueError(f"{name}: {e}") from None
    if not width or not height:
        raise ValueError(f"{name}: the YUV4MPEG2 header carries no frame size")
    if fps is not None:
        rate = float(fps)
    if rate is None:
        raise ValueError(f"{name}: the YUV4MPEG2 header carries no frame rate (F0:0 or no F token): pass fps")
    return width, height, rate, fmt, (field_order if field_order in FIELD_ORDERS else order)


class Y4mSource(_Yuv420FileSource):
    """YUV4MPEG2 (.y4m) reader, memory-mapped, frames indexed once at open.  The header is parse_y4m_header's: 8-bit 4:2:0 limited range,
    Yuv420Frames.  wide=True: parse_y4m_header_wide's, with `range` and a matrix of YUV_FORMAT_MATRICES; the frames are YuvFrames of
    self.fmt (10-bit, 4:2:2, 4:4:4, grey, full range ...).  deinterlace="adaptive" | "interpolate" | "match" (needs wide=True; "match",
    for film carried in interlaced video, takes comb_thresh and comb_limit, None: never fall back: InterlacedYuvFrame) accepts interlaced
    headers as parse_y4m_header_fields reads them with `field_order`; the frames of woven fields are InterlacedYuvFrames, each with the
    frame before it as its prev, read() and frames() deinterlace on the host.  transfer="pq" | "hlg" (needs wide=True; Y4M carries no tag for
    it) with tone_params (ToneMap's fields but transfer; primaries default to "bt2020" under matrix="bt2020", else "bt709") attaches a
    ToneMap to the frames: HDR material comes out as SDR.  square_pixels=True (the header's A token), sar=(num, den) (in its place) and
    resample_filter attach a Resample from the stored width to display_width() of it: the frames are then YuvFrames whatever `wide` says,
    their shape is the display size and to_bgr() / the Uploader resample every plane along its rows before the conversion; a ratio of
    1:1, no ratio, or one that shows the stored width changes nothing (one line is logged).  scale=H | (W, H) (UHD and other oversized
    video; not with deinterlace) attaches a VScale from the stored height to H and one Resample from the stored width straight to W; H
    alone keeps the display aspect: W is the nearest even number to display width * H / height.  The frames' shape is then (H, W, 3),
    to_bgr() / the Uploader scale vertically, then horizontally, then convert; the size the picture already has changes nothing (one
    line is logged).  The source's width and height stay the stored ones; vscale and resample say what the frames carry."""

    layout = "i420"

    def __init__(self, path, fps=None, matrix="bt601", wide=False, range="auto", deinterlace=None, field_order="auto", deinterlace_thresh=10,
                 transfer=None, tone_params=None, comb_thresh=10, comb_limit=20, square_pixels=False, sar=None, resample_filter="bicubic",
                 scale=None):
        self.deinterlace_thresh = _check_deinterlace(deinterlace, field_order, deinterlace_thresh)
        self.comb_thresh, self.comb_limit = _check_match(comb_thresh, comb_limit)
        _check_sar(path, square_pixels, sar, resample_filter, scale)
        if deinterlace is not None and not wide:
            raise ValueError(f"{path}: deinterlace={deinterlace!r} needs wide=True (the frames are YuvFrames)")
        self.deinterlace = deinterlace
        if wide:
            YuvFormat(matrix=matrix)        # a bad matrix is refused before the file is opened
        else:
            _check_matrix(matrix)
        self.tone = _source_tone(path, transfer, tone_params, matrix, wide)
        self.matrix = matrix
        size = self._map(path)
        mm = self._mm
        end = mm.find(b"\n", 0, 4096) if size else -1
        line = mm[:end] if end >= 0 else None
        # decided before the parser is chosen: where nothing is attached the header goes to today's parser, with today's refusals
        self.vscale, self.resample = _source_scale(path, _y4m_width(line), _y4m_height(line), parse_y4m_aspect(line), square_pixels, sar,
                                                   resample_filter, scale, deinterlace)
        if wide or self.resample is not None or self.vscale is not None:       # resampled frames are YuvFrames whatever `wide` says
            self.width, self.height, self.fps, self.fmt, self.field_order = parse_y4m_header_fields(
                line, path, fps, "file", matrix, range, None if deinterlace is None else field_order)
        else:
            self.width, self.height, self.fps = parse_y4m_header(line, path, fps)
        nbytes = self._frame_bytes()
        self._offsets = []
        pos = end + 1
        while pos < size:
            head = mm[pos:pos + 6]
            if len(head) < 6 and b"FRAME"[:len(head)] == head[:5]:
                break                      # the file ends inside a frame header: a truncated last frame
            if head[:5] != b"FRAME" or head[5:6] not in (b" ", b"\n"):
                raise ValueError(f"{path}: bytes at offset {pos} are neither a FRAME header nor the end of the file")
            nl = mm.find(b"\n", pos + 5, pos + 4096)
            if nl < 0:
                if size - pos <= 4096:
                    break                  # truncated inside the frame header's parameters
                raise ValueError(f"{path}: the FRAME header at offset {pos} does not end")
            if nl + 1 + nbytes > size:
                break                      # a truncated last frame is not a frame
            self._offsets.append(nl + 1)
            pos = nl + 1 + nbytes
        self.frame_count = len(self._offsets)


class Y4mStream:
    """Y4mSource for a pipe: YUV4MPEG2 from any binary file object (sys.stdin.buffer, a pipe, a socket file), read once, front to back.
    It never seeks and never asks for a size.  raw_frames() yields the Yuv420Frames in decode order, each owning its bytes (one buffer per
    frame, filled by readinto until it is full: short reads are normal on a pipe); frames() yields their to_bgr().  There is no read /
    read_raw: their absence is how a caller sees that the source is sequential.  frame_count is None until the stream is exhausted, then
    the number of whole frames read; a stream that ends inside a FRAME header or inside a frame drops that partial frame, as Y4mSource
    does; anything else where FRAME should stand is a ValueError naming the byte offset in the stream."""

    layout = "i420"

    fmt = None                        # wide=True: the YuvFormat of the header; raw_frames() then yields YuvFrames (see Y4mSource)

    deinterlace = field_order = None      # as Y4mSource's; the stream keeps the last frame's planes, the next frame's prev

    tone = None                       # as Y4mSource's (transfer, tone_params)

    resample = None                   # as Y4mSource's (square_pixels, sar, resample_filter)
    vscale = None                     # as Y4mSource's (scale)

    def __init__(self, fileobj, fps=None, matrix="bt601", name="<stream>", wide=False, range="auto", deinterlace=None, field_order="auto",
                 deinterlace_thresh=10, transfer=None, tone_params=None, comb_thresh=10, comb_limit=20, square_pixels=False, sar=None,
                 resample_filter="bicubic", scale=None):
        self.deinterlace_thresh = _check_deinterlace(deinterlace, field_order, deinterlace_thresh)
        self.comb_thresh, self.comb_limit = _check_match(comb_thresh, comb_limit)
        _check_sar(name, square_pixels, sar, resample_filter, scale)
        if deinterlace is not None and not wide:
            raise ValueError(f"{name}: deinterlace={deinterlace!r} needs wide=True (the frames are YuvFrames)")
        self.deinterlace = deinterlace
        if wide:
            YuvFormat(matrix=matrix)
        else:
            _check_matrix(matrix)
        self.tone = _source_tone(name, transfer, tone_params, matrix, wide)
        self.matrix = matrix
        self._fp, self.name = fileobj, name
        self._pos = 0                 # bytes of the stream consumed
        self._started = False
        line = self._line(4096)
        self.vscale, self.resample = _source_scale(name, _y4m_width(line), _y4m_height(line), parse_y4m_aspect(line), square_pixels, sar,
                                                   resample_filter, scale, deinterlace)
        if wide or self.resample is not None or self.vscale is not None:
            self.width, self.height, self.fps, self.fmt, self.field_order = parse_y4m_header_fields(
                line, name, fps, "stream", matrix, range, None if deinterlace is None else field_order)
        else:
            self.width, self.height, self.fps = parse_y4m_header(line, name, fps, what="stream")
        self.frame_count = None

    def _fill(self, view):
        """readinto until `view` is full -> bytes read (less than len(view): the stream ended)."""
        got = 0
        while got < len(view):
            n = self._fp.readinto(view[got:])
            if not n:
                break
            got += n
        self._pos += got
        return got

    def _line(self, limit):
        """Bytes up to the next newline (consumed, not returned), at most `limit` of them; None when there is none (the stream ended, or
        the line is longer); self._short then tells which."""
        out = bytearray()
        one = memoryview(bytearray(1))
        self._short = False
        while len(out) < limit:
            if self._fill(one) < 1:
                self._short = True
                return None
            if one[0] == 10:
                return bytes(out)
            out.append(one[0])
        return None

    def raw_frames(self):
        if self._started:
            raise ValueError(f"{self.name}: a Y4mStream is read once")
        self._started = True
        h, w = self.height, self.width
        ch, cw = _chroma_size(h, w)
        nbytes, count = (h * w + 2 * ch * cw if self.fmt is None else self.fmt.frame_bytes(h, w)), 0
        head = memoryview(bytearray(6))
        last = None
        while True:
            pos = self._pos
            got = self._fill(head)
            if got < 6 and b"FRAME"[:got] == bytes(head[:min(got, 5)]):
                break                      # the stream ends here, or inside a frame header: a truncated last frame
            if bytes(head[:5]) != b"FRAME" or bytes(head[5:6]) not in (b" ", b"\n"):
                raise ValueError(f"{self.name}: bytes at offset {pos} are neither a FRAME header nor the end of the stream")
            if head[5] != 10 and self._line(4096 - 6) is None:
                if self._short:
                    break                  # truncated inside the frame header's parameters
                raise ValueError(f"{self.name}: the FRAME header at offset {pos} does not end")
            buf = np.empty(nbytes, np.uint8)
            if self._fill(memoryview(buf)) < nbytes:
                break                      # a truncated last frame is not a frame
            count += 1
            if self.fmt is not None and self.field_order is not None:
                planes = _planes_at(buf, 0, h, w, self.fmt)
                yield InterlacedYuvFrame(planes, h, w, self.fmt, last, self.field_order, self.deinterlace, self.deinterlace_thresh, tone=self.tone,
                                         comb_thresh=self.comb_thresh, comb_limit=self.comb_limit, resample=self.resample)
                last = planes
                continue
            if self.fmt is not None:
                yield YuvFrame(_planes_at(buf, 0, h, w, self.fmt), h, w, self.fmt, tone=self.tone, resample=self.resample, vscale=self.vscale)
                continue
            planes = (buf[:h * w].reshape(h, w), buf[h * w:h * w + ch * cw].reshape(ch, cw), buf[h * w + ch * cw:].reshape(ch, cw))
            yield Yuv420Frame(planes, h, w, "i420", matrix=self.matrix)
        self.frame_count = count

    def frames(self):
        for raw in self.raw_frames():
            yield raw.to_bgr()

    def pos_msec(self, frame_no):
        """As _Yuv420FileSource.pos_msec once the stream is exhausted; before that every frame number from 0 up has a time stamp."""
        if frame_no < 0 or (self.frame_count is not None and frame_no >= self.frame_count):
            return None
        return frame_no * 1000.0 / self.fps


class Yuv420Source(_Yuv420FileSource):
    """Headerless file of consecutive 8-bit 4:2:0 frames (layout "i420": Y, U, V planes; "nv12": Y plane, interleaved UV plane), memory-
    mapped.  A partial last frame is dropped."""

    def __init__(self, path, width, height, fps, layout="i420", matrix="bt601"):
        if layout not in YUV_LAYOUTS:
            raise ValueError(f"layout must be one of {YUV_LAYOUTS}, not {layout!r}")
        self.matrix = _check_matrix(matrix)
        self.width, self.height, self.fps, self.layout = int(width), int(height), float(fps), layout
        if self.width < 1 or self.height < 1:
            raise ValueError(f"{path}: frame size {width} x {height}")
        size = self._map(path)
        nbytes = self._frame_bytes()
        self.frame_count = size // nbytes
        self._offsets = range(0, self.frame_count * nbytes, nbytes)


class YuvSource(_Yuv420FileSource):
    """Yuv420Source for any YuvFormat: a headerless file of consecutive packed pictures of `fmt` (`ffmpeg -f rawvideo -pix_fmt NAME`, a
    hardware decoder's P010 surfaces), memory-mapped; read_raw / raw_frames hand out YuvFrames.  A partial last frame is dropped.
    deinterlace="adaptive" | "interpolate" | "match" (with comb_thresh, comb_limit): the pictures are woven fields and the frames InterlacedYuvFrames; a headerless file names no
    field order, so field_order must be "tff" or "bff".  transfer, tone_params: as Y4mSource's.  sar=(num, den), resample_filter: as
    Y4mSource's; a headerless file carries no ratio, so square_pixels=True alone changes nothing."""

    def __init__(self, path, width, height, fps, fmt, deinterlace=None, field_order="auto", deinterlace_thresh=10, transfer=None, tone_params=None,
                 comb_thresh=10, comb_limit=20, square_pixels=False, sar=None, resample_filter="bicubic", scale=None):
        if not isinstance(fmt, YuvFormat):
            raise ValueError(f"fmt must be a YuvFormat, not {fmt!r}")
        _check_sar(path, square_pixels, sar, resample_filter, scale)
        self.tone = _source_tone(path, transfer, tone_params, fmt.matrix, True)
        self.deinterlace_thresh = _check_deinterlace(deinterlace, field_order, deinterlace_thresh)
        self.comb_thresh, self.comb_limit = _check_match(comb_thresh, comb_limit)
        if deinterlace is not None:
            if field_order == "auto":
                raise ValueError(f"{path}: a headerless YUV file names no field order: pass field_order \"tff\" or \"bff\"")
            self.deinterlace, self.field_order = deinterlace, field_order
        self.fmt, self.matrix = fmt, fmt.matrix
        self.width, self.height, self.fps = int(width), int(height), float(fps)
        if self.width < 1 or self.height < 1:
            raise ValueError(f"{path}: frame size {width} x {height}")
        self.vscale, self.resample = _source_scale(path, self.width, self.height, None, square_pixels, sar, resample_filter, scale,
                                                   deinterlace)      # (no header: sar says the ratio)
        size = self._map(path)
        nbytes = self._frame_bytes()
        self.frame_count = size // nbytes
        self._offsets = range(0, self.frame_count * nbytes, nbytes)


_RAW_YUV_EXT = {".yuv": "i420", ".i420": "i420", ".nv12": "nv12"}
_RAW_PIX_FMT_EXT = {".p010": "p010le"}


def open_source(path, fps=None, size=None, layout=None, matrix="bt601", wide=False, range="auto", pix_fmt=None, deinterlace=None,
                field_order="auto", deinterlace_thresh=10, transfer=None, tone_params=None, comb_thresh=10, comb_limit=20, square_pixels=False,
                sar=None, resample_filter="bicubic", scale=None):
    """The source of a file by its extension: .npy (needs fps), .y4m, .yuv / .i420 / .nv12 (headerless: need size=(width, height) and
    fps; `layout` overrides the extension's), anything else an AVI; "-" is a Y4mStream over standard input.  `matrix` goes to the
    YUV sources.  wide=True lets the Y4M readers accept what parse_y4m_header_wide does, with `range` ("auto": the header's).  pix_fmt
    (a name of YuvFormat.from_pix_fmt; .p010 implies p010le) reads a headerless file of that format through YuvSource, with `range`
    ("auto": the name's own) and any matrix of YUV_FORMAT_MATRICES; it needs size and fps.  deinterlace ("adaptive" | "interpolate" |
    "match", the last with comb_thresh and comb_limit), field_order and deinterlace_thresh go to the Y4M readers (with wide=True) and to YuvSource (with pix_fmt and a field order); no other
    source takes them.  transfer ("pq" | "hlg") and tone_params (ToneMap's other fields) go to the same readers under the same
    conditions: HDR material is tone-mapped to SDR; every other source refuses them.  square_pixels (use the Y4M header's sample aspect
    ratio), sar=(num, den) (say it in its place; the only way for a headerless file) and resample_filter ("bicubic" | "bilinear" |
    "lanczos") go to the Y4M readers and to the headerless YUV files: anamorphic video is resampled to square pixels, the frames are
    YuvFrames whatever `wide` says (a headerless 8-bit 4:2:0 file is then read through YuvSource), and a ratio of 1:1 or none changes
    nothing; the other sources refuse them.  scale=H | (W, H) goes to the same readers, shares resample_filter and does not go with
    deinterlace: every frame is scaled to H rows on the device before anything else sees it (UHD to 1080 rows, say), H alone keeping the
    display aspect; the size the picture already has changes nothing."""
    if range not in YUV_RANGES:
        raise ValueError(f"range must be one of {YUV_RANGES}, not {range!r}")
    _check_deinterlace(deinterlace, field_order, deinterlace_thresh)
    _check_match(comb_thresh, comb_limit)
    if deinterlace != "match" and (comb_thresh, comb_limit) != (10, 20):
        raise ValueError(f"comb_thresh and comb_limit belong to deinterlace=\"match\", not to deinterlace={deinterlace!r}")
    fields = {} if deinterlace is None else dict(deinterlace=deinterlace, field_order=field_order, deinterlace_thresh=deinterlace_thresh)
    if deinterlace == "match":
        fields.update(comb_thresh=comb_thresh, comb_limit=comb_limit)
    if transfer is not None or tone_params:
        fields.update(transfer=transfer, tone_params=tone_params)
    square = {}
    if _check_sar(path, square_pixels, sar, resample_filter, scale) or scale is not None:
        square = dict(square_pixels=square_pixels, sar=sar, resample_filter=resample_filter)
        if scale is not None:
            square["scale"] = scale
            if deinterlace is not None:
                raise ValueError(f"{path}: scale does not go with deinterlace={deinterlace!r}: interlaced pictures are not scaled vertically")
    if str(path) == "-":
        import sys
        return Y4mStream(sys.stdin.buffer, fps, matrix, name="<stdin>", wide=wide, range=range, **fields, **square)
    ext = os.path.splitext(str(path))[1].lower()
    if square and ext != ".y4m" and pix_fmt is None and ext not in _RAW_PIX_FMT_EXT and ext not in _RAW_YUV_EXT:
        if scale is not None:
            raise ValueError(f"{path}: scale takes YUV4MPEG2 and headerless YUV files; BGR sources are not scaled")
        raise ValueError(f"{path}: square_pixels / sar resample YUV4MPEG2 and headerless YUV files; BGR sources have square pixels")
    if fields and ext != ".y4m" and pix_fmt is None and (layout is not None or ext not in _RAW_PIX_FMT_EXT):
        if deinterlace is None:
            _source_tone(path, transfer, tone_params, matrix, False)         # raises, naming the option
        raise ValueError(f"{path}: deinterlace={deinterlace!r} reads YUV4MPEG2 (with wide=True) or a headerless YUV file named by pix_fmt")
    if str(path).endswith(".npy"):
        if fps is None:
            raise ValueError("a .npy frame stack carries no frame rate: pass fps")
        return NpySource(path, fps)
    if ext == ".y4m":
        return Y4mSource(path, fps, matrix, wide=wide, range=range, **fields, **square)
    if pix_fmt is None and layout is None:
        pix_fmt = _RAW_PIX_FMT_EXT.get(ext)
    if pix_fmt is not None or ext in _RAW_YUV_EXT:
        if size is None:
            raise ValueError(f"{path}: a headerless YUV file carries no frame size: pass size=(width, height)")
        if fps is None:
            raise ValueError(f"{path}: a headerless YUV file carries no frame rate: pass fps")
        if pix_fmt is not None:
            if layout is not None:
                raise ValueError(f"{path}: pix_fmt {pix_fmt!r} names the plane layout; layout {layout!r} was given as well")
            return YuvSource(path, size[0], size[1], fps, YuvFormat.from_pix_fmt(pix_fmt, matrix, range), **fields, **square)
        vscale, resample = _source_scale(path, int(size[0]), int(size[1]), None, square_pixels, sar, resample_filter, scale)  # decided, and logged, here
        if resample is not None or vscale is not None:
            name = {"i420": "yuv420p", "nv12": "nv12"}.get(layout or _RAW_YUV_EXT[ext])
            if name is None:
                raise ValueError(f"layout must be one of {YUV_LAYOUTS}, not {layout!r}")
            src = YuvSource(path, size[0], size[1], fps, YuvFormat.from_pix_fmt(name, _check_matrix(matrix)))
            src.vscale, src.resample = vscale, resample
            return src
        return Yuv420Source(path, size[0], size[1], fps, layout or _RAW_YUV_EXT[ext], matrix)
    return AviBgr24Source(path)
