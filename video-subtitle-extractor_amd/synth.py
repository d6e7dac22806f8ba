"""Seeded synthetic video frames for tests and the benchmark: there is no decodable
video on either box, so frames are generated: noisy dark background with a vertical gradient and 1-2 subtitle
lines (white fill, black outline) inside the reference's default subtitle area
(y in [0.78,0.99]*H, x in [0.05,0.95]*W; backend/config.py:49)."""
import struct

import numpy as np

_WORDS = ("the quick brown fox jumps over a lazy dog while seven wizards quietly box with grumpy elves "
          "near frozen lakes and bright morning light shines across silent hills").split()


def _font(size):
    from PIL import ImageFont
    for p in ("/usr/share/fonts/truetype/dejavu/DejaVuSans-Bold.ttf", "DejaVuSans-Bold.ttf"):
        try:
            return ImageFont.truetype(p, size)
        except Exception:
            continue
    return None


def render_line(text, height, rng):
    """-> (uint8 [h,w] fill mask, uint8 [h,w] outline mask)"""
    from PIL import Image, ImageDraw
    font = _font(int(height * 0.8))
    if font is None:
        # pseudo-glyph fallback: vertical strokes
        w = len(text) * height // 2
        fill = np.zeros((height, w), np.uint8)
        for i in range(0, w - 6, max(6, height // 3)):
            fill[rng.integers(2, height // 3):height - rng.integers(2, height // 3), i:i + 4] = 255
        outline = np.zeros_like(fill)
        return fill, outline
    tmp = Image.new("L", (4096, height * 2), 0)
    d = ImageDraw.Draw(tmp)
    d.text((8, height // 4), text, fill=255, font=font, stroke_width=2, stroke_fill=128)
    a = np.asarray(tmp)
    ys, xs = np.nonzero(a)
    a = a[max(ys.min() - 1, 0):ys.max() + 2, max(xs.min() - 1, 0):xs.max() + 2]
    return (a == 255).astype(np.uint8) * 255, (a == 128).astype(np.uint8) * 255


def make_frames(n, height=1080, width=1920, seed=0, p_two_lines=0.2, return_truth=False):
    """uint8 BGR [n,height,width,3] (+ list of ground-truth (x0,y0,x1,y1,text) per frame)."""
    rng = np.random.default_rng(seed)
    frames = np.empty((n, height, width, 3), np.uint8)
    truth = []
    grad = np.linspace(0, 40, height, dtype=np.float32)[:, None, None]
    scale = height / 1080.0
    for f in range(n):
        base = rng.integers(30, 91, size=((height + 3) // 4, (width + 3) // 4, 3), dtype=np.uint8)
        img = np.repeat(np.repeat(base, 4, 0), 4, 1)[:height, :width].astype(np.float32) + grad
        lines = 2 if rng.random() < p_two_lines else 1
        gh = int(rng.integers(54, 67) * scale)
        y_lo, y_hi = int(0.78 * height), int(0.99 * height)
        ys = [y_hi - gh - 8] if lines == 1 else [y_lo + 6, y_lo + gh + 26]
        tr = []
        for y in ys:
            nwords = int(rng.integers(3, 8))
            text = " ".join(rng.choice(_WORDS, nwords))
            fill, outline = render_line(text, gh, rng)
            lh, lw = fill.shape
            lw = min(lw, int(0.88 * width))
            fill, outline = fill[:, :lw], outline[:, :lw]
            x = (width - lw) // 2
            y = min(y, height - lh - 2)
            reg = img[y:y + lh, x:x + lw]
            reg[outline > 0] = 0
            reg[fill > 0] = 255
            tr.append((x, y, x + lw, y + lh, text))
        frames[f] = np.clip(img, 0, 255).astype(np.uint8)
        truth.append(tr)
    return (frames, truth) if return_truth else frames


def make_clip(schedule, height=360, width=640, seed=0):
    """A clip with held subtitles for the subtitle-change selector: uint8 BGR [n,height,width,3] + the true
    [(start, end, text)] (1-based frame numbers, one entry per shown subtitle).

    schedule: list of (text, frames) or (text, frames, fade); text None is a gap without a subtitle, `fade` > 0 blends the
    first `fade` frames of that subtitle in at alpha (k + 1) / (fade + 1).  Every frame draws its background noise afresh
    (the noise of make_frames); a text is rendered once and always drawn at the same place, one line centred in the
    lower subtitle band, so back-to-back changes, gaps and the same text again after a gap are what the schedule says."""
    rng = np.random.default_rng(seed)
    n = sum(int(s[1]) for s in schedule)
    frames = np.empty((n, height, width, 3), np.uint8)
    grad = np.linspace(0, 40, height, dtype=np.float32)[:, None, None]
    gh = max(12, int(60 * height / 1080.0))
    y = int(0.99 * height) - gh - 8
    glyphs = {}
    truth = []
    f = 0
    for item in schedule:
        text, count = item[0], int(item[1])
        fade = int(item[2]) if len(item) > 2 else 0
        if text is not None:
            if text not in glyphs:
                fill, outline = render_line(text, gh, np.random.default_rng([seed, *text.encode()]))
                lw = min(fill.shape[1], int(0.88 * width))
                glyphs[text] = (fill[:, :lw], outline[:, :lw])
            truth.append((f + 1, f + count, text))
        for k in range(count):
            base = rng.integers(30, 91, size=((height + 3) // 4, (width + 3) // 4, 3), dtype=np.uint8)
            img = np.repeat(np.repeat(base, 4, 0), 4, 1)[:height, :width].astype(np.float32) + grad
            if text is not None:
                fill, outline = glyphs[text]
                lh, lw = fill.shape
                x = (width - lw) // 2
                yy = min(y, height - lh - 2)
                a = (k + 1) / (fade + 1) if k < fade else 1.0
                reg = img[yy:yy + lh, x:x + lw]
                reg[outline > 0] *= 1.0 - a
                reg[fill > 0] = reg[fill > 0] * (1.0 - a) + 255.0 * a
            frames[f] = np.clip(img, 0, 255).astype(np.uint8)
            f += 1
    return frames, truth


def make_moving_clip(schedule, height=120, width=320, pan=(2, 3), amp=(110, 60), cells=(16, 4), noise=3, seed=0, text_bgr=(255, 255, 255),
                     outline=True, chroma=False):
    """A clip with held subtitles over a textured background that moves, for the held-edge selector: uint8 BGR [n,height,width,3] +
    the true [(start, end, text)] (1-based frame numbers).  make_clip's background has no edge at the selectors' threshold; this one
    has hundreds in the subtitle band, and they move every frame.

    schedule: list of (text, frames); text None is a gap.  The background is a window into one grey world of random cells
    (`cells` pixels wide with amplitudes `amp`, summed around 128 and clipped to 8..247) that moves by |pan| = (dy, dx) pixels per
    frame, plus fresh noise of +-`noise` levels per frame; a text is one line of height 20 (white, its outline black) that always
    stands at the same place, centred, 10 pixels above the bottom edge.
    text_bgr: the fill colour (B, G, R); outline=False leaves the outline's pixels to the background; chroma=True draws the random cells
    with three channels instead of one, so the world is coloured (what a colour key tells from the text, frame_select.ColourKey).  The
    defaults give the grey clip, draw for draw."""
    rng = np.random.default_rng(seed)
    n = sum(int(s[1]) for s in schedule)
    dy, dx = abs(int(pan[0])), abs(int(pan[1]))
    wh, ww = height + dy * n + 1, width + dx * n + 1
    world = np.full((wh, ww, 3), 128, np.int32)
    for cell, a in zip(cells, amp):
        t = rng.integers(-a, a + 1, (-(-wh // cell), -(-ww // cell), 3 if chroma else 1))
        world += np.repeat(np.repeat(t, cell, 0), cell, 1)[:wh, :ww]
    np.clip(world, 8, 247, out=world)
    frames = np.empty((n, height, width, 3), np.uint8)
    glyphs = {}
    truth = []
    f = 0
    for text, count in schedule:
        count = int(count)
        if text is not None:
            if text not in glyphs:
                fill, edge = render_line(text, 20, np.random.default_rng([seed, *text.encode()]))
                lw = min(fill.shape[1], int(0.88 * width))
                glyphs[text] = (fill[:, :lw], edge[:, :lw])
            truth.append((f + 1, f + count, text))
        for _ in range(count):
            img = world[dy * f:dy * f + height, dx * f:dx * f + width] + rng.integers(-noise, noise + 1, (height, width, 3))
            if text is not None:
                fill, edge = glyphs[text]
                lh, lw = fill.shape
                x, y = (width - lw) // 2, height - lh - 10
                reg = img[y:y + lh, x:x + lw]
                if outline:
                    reg[edge > 0] = 0
                reg[fill > 0] = text_bgr
            frames[f] = np.clip(img, 0, 255).astype(np.uint8)
            f += 1
    return frames, truth


def interlace_yuv420(field_rate_bgr, field_order="tff"):
    """Pictures rendered at field rate (uint8 BGR [2 n, H, W, 3]; an odd last one is dropped) -> n interlaced 4:2:0 frames as (Y, U, V)
    plane triples: each picture goes through ingest.bgr_to_yuv420 on its own, then the rows of every plane are woven: of frame k's two
    pictures the earlier one gives the rows of the field that comes first (the even rows for "tff", the odd ones for "bff"), the later
    one the others.  Chroma rows alternate between the fields as luma rows do, which is how interlaced 4:2:0 is stored."""
    from .ingest import FIELD_ORDERS, bgr_to_yuv420
    keep = FIELD_ORDERS.index(field_order)
    out = []
    for k in range(len(field_rate_bgr) // 2):
        first, second = bgr_to_yuv420(field_rate_bgr[2 * k]), bgr_to_yuv420(field_rate_bgr[2 * k + 1])
        woven = []
        for a, b in zip(first, second):
            p = np.array(b, copy=True)
            p[keep::2] = a[keep::2]
            woven.append(p)
        out.append(tuple(woven))
    return out


TELECINE_PATTERNS = {"32": ((0, 0), (1, 1), (1, 2), (2, 3), (3, 3)), "32b": ((0, 0), (1, 1), (2, 1), (3, 2), (3, 3))}


def telecine(planes_list, pattern="32", field_order="tff"):
    """Progressive pictures (plane tuples of one format, e.g. ingest.bgr_to_yuv420's) dealt into interlaced frames, as film is carried in
    interlaced video -> (the woven plane tuples, per stored frame the indices (picture of its first field, picture of its second field)).
    The first field is the one first in time: the top one (the even rows of every plane) for "tff", the bottom one for "bff".
      "32"     3:2 pulldown, four pictures A B C D to five frames: At Ab, Bt Bb, Bt Cb, Ct Db, Dt Db (t the first field, b the second)
      "32b"    its other phase, the second field running ahead: At Ab, Bt Bb, Ct Bb, Dt Cb, Dt Db
      "shift"  fields shifted by one: frame k holds the first field of picture k and the second field of picture k - 1 (frame 0: picture 0)
    A pulldown cycle that the pictures end in is cut where a field's picture is missing."""
    from .ingest import FIELD_ORDERS
    if field_order not in FIELD_ORDERS:
        raise ValueError(f"field_order must be one of {FIELD_ORDERS}, not {field_order!r}")
    if pattern != "shift" and pattern not in TELECINE_PATTERNS:
        raise ValueError(f"pattern must be one of {sorted(TELECINE_PATTERNS) + ['shift']}, not {pattern!r}")
    keep = FIELD_ORDERS.index(field_order)
    n = len(planes_list)
    if pattern == "shift":
        pairs = [(k, max(k - 1, 0)) for k in range(n)]
    else:
        pairs = [(base + a, base + b) for base in range(0, n, 4) for a, b in TELECINE_PATTERNS[pattern] if max(base + a, base + b) < n]
    woven = []
    for first, second in pairs:
        frame = []
        for a, b in zip(planes_list[first], planes_list[second]):
            p = np.array(b, copy=True)
            p[keep::2] = np.asarray(a)[keep::2]
            frame.append(p)
        woven.append(tuple(frame))
    return woven, pairs


def hdr_grade(frames_bgr, white_nits=203.0, transfer="pq", depth=10, sub=(1, 1)):
    """SDR frames (uint8 BGR [n, H, W, 3]) graded as HDR video -> n (Y, U, V) plane triples of BT.2020 non-constant-luminance limited-range
    samples at `depth` bits (uint16; uint8 at depth 8), chroma subsampled by sub = (sub_x, sub_y) as the mean of each block.  The inverse
    of what ingest.ToneMap undoes, in float64: BGR -> gamma 2.4 linear light -> BT.709 to BT.2020 primaries -> nits (SDR white at
    white_nits) -> the PQ inverse EOTF, or the inverse of ingest.hlg_nits per channel.  For tests and benchmarks; nothing is specified
    about its rounding."""
    from . import ingest
    if transfer not in ingest.TONE_TRANSFERS:
        raise ValueError(f"transfer must be one of {ingest.TONE_TRANSFERS}, not {transfer!r}")
    sub_x, sub_y = sub
    to2020 = np.linalg.inv(ingest.bt2020_to_bt709())
    kr, kb = 0.2627, 0.0593
    kg = 1.0 - kr - kb
    scale = float(1 << (depth - 8))
    dtype = np.uint8 if depth == 8 else np.dtype("<u2")
    out = []
    for f in frames_bgr:
        lin = np.power(np.asarray(f, np.float64)[..., ::-1] / 255.0, 2.4)                       # R G B
        nits = np.clip(lin @ to2020.T, 0.0, None) * white_nits
        e = ingest.pq_inverse_eotf(nits) if transfer == "pq" else ingest.hlg_inverse_nits(nits)
        r, g, b = e[..., 0], e[..., 1], e[..., 2]
        y = kr * r + kg * g + kb * b
        h, w = y.shape
        ch, cw = (h + sub_y) >> sub_y, (w + sub_x) >> sub_x

        def mean(p):
            q = np.pad(p, ((0, (ch << sub_y) - h), (0, (cw << sub_x) - w)), mode="edge")
            return q.reshape(ch, 1 << sub_y, cw, 1 << sub_x).mean(axis=(1, 3))
        planes = ((219.0 * y + 16.0) * scale, (224.0 * mean((b - y) / (2.0 * (1.0 - kb))) + 128.0) * scale,
                  (224.0 * mean((r - y) / (2.0 * (1.0 - kr))) + 128.0) * scale)
        out.append(tuple(np.clip(np.rint(p), 0, (1 << depth) - 1).astype(dtype) for p in planes))
    return out


def make_scenes(scenes, height=360, width=640, seed=0):
    """A clip of camera shots for the scene-cut finder: uint8 BGR [n,height,width,3] + the 0-based number of each scene's first frame.

    scenes: a list of dicts, one per scene:
      frames  number of frames;
      pan     (dy, dx) source pixels the camera moves per frame, or a list of per-frame (dy, dx) steps (frame k of the scene is
              displaced by the sum of the first k steps; a short list repeats its last step); default (0, 0);
      hold    in-scene frame indices (>= 1) that repeat the frame before them byte for byte (a held frame);
      text    (text, first, last): a subtitle line drawn over in-scene frames first..last, centred in the lower band.
    A scene is a window into its own textured world (random 32- and 8-pixel cells around the scene's own mean colour), so a pan
    shows the same texture displaced; every frame that is not held gets fresh noise of +-3 levels.  make_clip redraws its whole
    background every frame and so has no motion to find."""
    rng = np.random.default_rng(seed)
    n = sum(int(sc["frames"]) for sc in scenes)
    out = np.empty((n, height, width, 3), np.uint8)
    cuts, f = [], 0
    for sc in scenes:
        count = int(sc["frames"])
        pan = sc.get("pan", (0, 0))
        steps = [tuple(pan)] if isinstance(pan[0], (int, np.integer)) else [tuple(p) for p in pan]
        pos = [(0, 0)]
        for k in range(1, count):
            dy, dx = steps[min(k - 1, len(steps) - 1)]
            pos.append((pos[-1][0] + int(dy), pos[-1][1] + int(dx)))
        y_min, x_min = min(p[0] for p in pos), min(p[1] for p in pos)
        wh = height + max(p[0] for p in pos) - y_min
        ww = width + max(p[1] for p in pos) - x_min
        mean = rng.integers(70, 186, size=3)
        world = np.zeros((wh, ww, 3), np.int32) + mean
        for cell, amp in ((32, 50), (8, 25)):
            t = rng.integers(-amp, amp + 1, size=((wh + cell - 1) // cell, (ww + cell - 1) // cell, 1))
            world += np.repeat(np.repeat(t, cell, 0), cell, 1)[:wh, :ww]
        np.clip(world, 8, 247, out=world)
        glyph = None
        if sc.get("text"):
            text, first, last = sc["text"]
            gh = max(12, int(60 * height / 1080.0))
            fill, outline = render_line(text, gh, np.random.default_rng([seed, *text.encode()]))
            lw = min(fill.shape[1], int(0.88 * width))
            glyph = (fill[:, :lw], outline[:, :lw], int(first), int(last))
        hold = set(sc.get("hold", ()))
        cuts.append(f)
        for k in range(count):
            if k in hold and k > 0:
                out[f] = out[f - 1]
            else:
                y, x = pos[k][0] - y_min, pos[k][1] - x_min
                img = world[y:y + height, x:x + width] + rng.integers(-3, 4, size=(height, width, 3))
                if glyph is not None and glyph[2] <= k <= glyph[3]:
                    fill, outline = glyph[0], glyph[1]
                    lh, lw = fill.shape
                    yy = min(int(0.99 * height) - lh - 8, height - lh - 2)
                    reg = img[yy:yy + lh, (width - lw) // 2:(width - lw) // 2 + lw]
                    reg[outline > 0] = 0
                    reg[fill > 0] = 255
                out[f] = np.clip(img, 0, 255).astype(np.uint8)
            f += 1
    return out, cuts


# ---- audio for timeline sync ---------------------------------------------------------------------------------------------------
# Built from the bit generator's raw 64-bit words and integer arithmetic only, so a seed gives the same samples (and WAV bytes)
# on any numpy.  Content is made at AUDIO_BASE_RATE and held (sample-and-hold) to any output rate, so two renders of the same
# content at different rates line up after resampling.

AUDIO_BASE_RATE = 12000


def _raw(seed, n):
    return np.random.PCG64(seed).random_raw(n)


def speech_content(seconds, seed, floor=200, syllable_ms=(80, 260), gap_ms=(30, 320), amp=(1500, 12000)):
    """int32 [seconds * AUDIO_BASE_RATE]: syllable-like bursts of noise (random length, gap and loudness, with a 10 ms ramp on
    each side) over a noise floor of +-floor."""
    n = int(seconds * AUDIO_BASE_RATE)
    words = _raw(seed, n + 3 * (n // 300 + 8))
    noise = (words[:n] >> np.uint64(48)).astype(np.int64) - 32768             # uniform in [-32768, 32768)
    env = np.full(n, floor, np.int64)
    params = words[n:].reshape(-1, 3)
    ms = AUDIO_BASE_RATE // 1000
    at = 0
    for w_len, w_gap, w_amp in params:
        at += (gap_ms[0] + int(w_gap % np.uint64(gap_ms[1] - gap_ms[0]))) * ms
        if at >= n:
            break
        length = (syllable_ms[0] + int(w_len % np.uint64(syllable_ms[1] - syllable_ms[0]))) * ms
        a = amp[0] + int(w_amp % np.uint64(amp[1] - amp[0]))
        ramp = 10 * ms
        idx = np.arange(length)
        shape = np.minimum(np.minimum(idx + 1, length - idx), ramp) * a // ramp
        end = min(at + length, n)
        env[at:end] = np.maximum(env[at:end], shape[:end - at])
        at = end
    return (noise * env) >> 15


def noise_content(seconds, seed, level):
    """int32 [seconds * AUDIO_BASE_RATE]: uniform noise of +-level (an inserted segment, or noise to add)."""
    return _noise(int(seconds * AUDIO_BASE_RATE), seed, level)


def _noise(n, seed, level):
    return (((_raw(seed, n) >> np.uint64(48)).astype(np.int64) - 32768) * level) >> 15


def render_audio(content, rate, channels=1, gain=(1, 1)):
    """int32 content at AUDIO_BASE_RATE -> int16 [n, channels] at `rate` (sample-and-hold), scaled by gain[0] / gain[1]; the
    channels after the first are the first at 3/4 and 1/2 ... of its level."""
    content = np.asarray(content, np.int64)
    n = len(content) * rate // AUDIO_BASE_RATE
    x = content[np.arange(n, dtype=np.int64) * AUDIO_BASE_RATE // rate] * gain[0] // gain[1]
    cols = [x * (4 - min(c, 3)) // 4 for c in range(channels)]
    return np.clip(np.stack(cols, axis=1), -32768, 32767).astype(np.int16)


def wav_bytes(samples, rate, extensible=False, chunks_before_data=()):
    """int16 [n, channels] -> a 16-bit PCM WAV file (fmt EXTENSIBLE if asked; extra (id, payload) chunks before the data)."""
    samples = np.asarray(samples, np.int16)
    ch = samples.shape[1]
    if extensible:
        fmt = struct.pack("<HHIIHHHHIH14s", 0xFFFE, ch, rate, rate * 2 * ch, 2 * ch, 16, 22, 16, 0, 1,
                          b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71")
    else:
        fmt = struct.pack("<HHIIHH", 1, ch, rate, rate * 2 * ch, 2 * ch, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for cid, payload in chunks_before_data:
        body += cid + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")
    data = samples.astype("<i2").tobytes()
    body += b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def audio_from_recipe(r):
    """A WAV file (bytes) from a JSON-able recipe:
    {"pieces": [["speech", seed, seconds, from_s, to_s] | ["noise", seed, seconds, level], ...],   # concatenated content
     "rate": Hz, "channels": 1, "gain": [num, den], "noise": [seed, level] or None,               # noise added to the content
     "trim": output samples dropped at the end, "extensible": bool, "list_chunk": bool}"""
    parts = []
    for p in r["pieces"]:
        if p[0] == "speech":
            _, seed, seconds, a, b = p
            parts.append(speech_content(seconds, seed)[int(a * AUDIO_BASE_RATE):int(b * AUDIO_BASE_RATE)])
        else:
            _, seed, seconds, level = p
            parts.append(noise_content(seconds, seed, level))
    content = np.concatenate(parts)
    if r.get("noise"):
        seed, level = r["noise"]
        content = content + _noise(len(content), seed, level)
    x = render_audio(content, r.get("rate", AUDIO_BASE_RATE), r.get("channels", 1), tuple(r.get("gain", (1, 1))))
    if r.get("trim"):
        x = x[:len(x) - r["trim"]]
    extra = [(b"LIST", b"INFOISFT\x05\x00\x00\x00synth\x00")] if r.get("list_chunk") else []
    return wav_bytes(x, r.get("rate", AUDIO_BASE_RATE), extensible=r.get("extensible", False), chunks_before_data=extra)
