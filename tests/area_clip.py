"""The clip the subtitle-area locator's tests share: synth.make_clip with a held-subtitle schedule, a constant logo and a flickering
bar pattern painted over it, and where its texts are."""
import numpy as np

from vse_amd import synth

H, W = 360, 640
TEXT_A, TEXT_B, TEXT_C = "the quick brown fox", "seven wizards quietly box", "near frozen lakes"
SCHEDULE = [(None, 6), (TEXT_A, 14), (TEXT_B, 12), (None, 5), (TEXT_C, 16, 3), (TEXT_A, 9), (None, 4)]
LOGO = (8, 40, 8, 72)                   # rows 8:40, columns 8:72: constant, high contrast, in every frame
BARS = (170, 186, 256, 384)             # mid-frame bar pattern, present in a random half of the frames
FPS = 10.0
LOCATOR = dict(min_seconds=0.5, max_seconds=4.0)       # min_frames 5, max_frames 40 at 10 fps


def text_boxes(schedule=SCHEDULE, height=H, width=W, seed=3):
    """(y0, y1, x0, x1) of every text make_clip draws: where it pastes the rendered line."""
    gh = max(12, int(60 * height / 1080.0))
    out = []
    for text in sorted({s[0] for s in schedule if s[0] is not None}):
        fill, _ = synth.render_line(text, gh, np.random.default_rng([seed, *text.encode()]))
        lh, lw = fill.shape[0], min(fill.shape[1], int(0.88 * width))
        yy = min(int(0.99 * height) - gh - 8, height - lh - 2)
        out.append((yy, yy + lh, (width - lw) // 2, (width - lw) // 2 + lw))
    return out


def decorated_clip(schedule=SCHEDULE):
    """make_clip at 360 x 640, seed 3, plus the logo and the flickering bars -> (frames, truth)."""
    frames, truth = synth.make_clip(schedule, H, W, seed=3)
    y0, y1, x0, x1 = LOGO
    yy, xx = np.mgrid[y0:y1, x0:x1]
    frames[:, y0:y1, x0:x1] = np.where(((yy // 4 + xx // 4) & 1)[..., None] == 1, 255, 0).astype(np.uint8)
    on = np.random.default_rng(17).permutation(len(frames)) < len(frames) // 2
    y0, y1, x0, x1 = BARS
    frames[on, y0:y1, x0:x1] = np.where((np.arange(x0, x1) // 4) & 1, 255, 0).astype(np.uint8)[None, None, :, None]
    return frames, truth


def as_tuple(area):
    return None if area is None else (area.ymin, area.ymax, area.xmin, area.xmax)
