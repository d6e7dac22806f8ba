"""The colour key on the host: the integers of vse_colour_key (tests/colour_key_ref.py, frame_select.ColourKey), the colour parser, the
selectors with and without the key on a coloured clip (yellow text without an outline over random cells drawn per channel, panning and
standing still), where the bytes go that key_fn returns (count_fn, focus_fn, cells_fn) and where they do not (compositor, recogniser),
the locator on the keyed clip, SubtitleExtractor(change_params={"text_colour": ...}) in several passes and in one, and the two command
lines' flags.  CPU only: numpy counters and a scripted recogniser."""
import numpy as np
import pytest

import colour_key_ref as ref
from area_cells_ref import NumpyCells
from frame_change_ref import NumpyCounter, edge_mask
from frame_focus_ref import NumpyFocus
from frame_hold_ref import NumpyHoldCounter
from frame_masks_hold_ref import NumpyCellsHoldMasks
from frame_masks_ref import NumpyCellsMasks
from test_change_select import stamped
from test_frame_hold import BAND, MOVING, BandOcr, spans
from vse_amd import area_locator, extractor, frame_select, srt, synth

YELLOW = (0, 255, 255)                    # B, G, R
TRUE = [(8, 27), (28, 45), (52, 76), (77, 90)]
PANS = ((2, 3), (0, 0))
AREA = (60, 120, 0, 320)                  # BAND in frame pixels
_cache = {}


def coloured_clip(pan):
    """test_frame_hold's schedule in colour: yellow text without an outline over cells drawn per channel at amplitudes (120, 120)."""
    if pan not in _cache:
        _cache[pan] = synth.make_moving_clip(MOVING, pan=pan, amp=(120, 120), text_bgr=YELLOW, outline=False, chroma=True)
    return _cache[pan]


# ---- the integers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", (1, 2, 24, 48, 127, 255))
def test_key_of_distance(tol):
    slope = ref.slope_of(tol)
    assert slope == frame_select.ColourKey(YELLOW, tol).slope and 256 <= slope <= 65280
    d = np.arange(256)
    k = ref.key_of_distance(d, slope)
    assert 255 * slope < 1 << 24
    assert k[0] == 255 and np.all(k[tol:] == 0) and np.all(np.diff(k) <= 0) and k.min() >= 0
    assert np.all(k[:tol] > 0) or tol == 255          # (tol 255: slope 256, K = 255 - d, 0 only at d = 255)
    assert [int(max(0, 255 - ((int(v) * slope) >> 8))) for v in d] == k.tolist()


def test_luma_of_a_keyed_band_is_the_key():
    frames, _ = coloured_clip((2, 3))
    key = frame_select.ColourKey("yellow", 48)
    keyed = ref.colour_key(frames[:12], AREA, key.bgr, key.slope)
    k = ref.key_plane(frames[:12, 60:120, 0:320], key.bgr, key.slope)
    assert np.array_equal(keyed[:, 60:120, :, 0], k) and np.array_equal(keyed[..., 0], keyed[..., 1]) and np.array_equal(keyed[..., 0], keyed[..., 2])
    assert not keyed[:, :60].any()
    for thresh in (1, 64, 128, 192, 255):
        grad = np.maximum(np.abs(k[:, 1:-1, 2:] - k[:, 1:-1, :-2]), np.abs(k[:, 2:, 1:-1] - k[:, :-2, 1:-1]))
        assert np.array_equal(edge_mask(keyed, AREA, thresh), grad >= thresh)


@pytest.mark.parametrize("area", (AREA, (61, 64, 3, 6), (0, 120, 0, 320), (119, 120, 319, 320)))
def test_apply_equals_the_reference(area):
    frames, _ = coloured_clip((2, 3))
    for colour, tol in (("yellow", 48), ((12, 200, 7), 1), ("#102030", 255)):
        key = frame_select.ColourKey(colour, tol)
        got = key.apply(frames[5:9], area)
        assert got.dtype == np.uint8 and np.array_equal(got, ref.colour_key(frames[5:9], area, key.bgr, key.slope))
        assert np.array_equal(got, ref.NumpyKey(key.bgr, tol)(frames[5:9], area))


def test_parser():
    assert frame_select.parse_colour("#FFFF00") == frame_select.parse_colour("ffff00") == frame_select.parse_colour("yellow") == YELLOW
    assert frame_select.parse_colour(" White ") == (255, 255, 255)
    assert frame_select.parse_colour("#0A141E") == (30, 20, 10)           # RRGGBB -> (B, G, R)
    assert frame_select.parse_colour((1, 2, 3)) == frame_select.parse_colour(np.array([1, 2, 3], np.uint8)) == (1, 2, 3)
    for bad in ("", "#FFFF0", "FFFF000", "#GGGGGG", "mauve", (1, 2), (1, 2, 256), (-1, 2, 3), (1.5, 2, 3), None, 7):
        with pytest.raises(ValueError):
            frame_select.parse_colour(bad)
    for tol in (0, 256, -3, 1.5, "48", True):
        with pytest.raises((ValueError, TypeError)):
            frame_select.ColourKey("yellow", tol)
    assert frame_select.ColourKey("yellow").tol == 48 and frame_select.ColourKey("yellow").bgr == YELLOW


# ---- the selectors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pan", PANS)
def test_the_plain_change_selector_misses_the_truth(pan):
    frames, truth = coloured_clip(pan)
    assert [(s, e) for s, e, _t in truth] == TRUE
    for thresh in (64, 128, 192):
        got = spans(frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=thresh).run(list(frames), BAND))
        assert got != TRUE and len(got) <= 1, (thresh, got)              # nothing over the pan, one merged interval over the still cells


@pytest.mark.parametrize("pan", PANS)
def test_the_keyed_change_selector_finds_the_truth(pan):
    frames, _ = coloured_clip(pan)
    key = ref.NumpyKey(YELLOW, 48)
    sel = frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=128, key_fn=key, batch=16)
    got = sel.run(list(frames), BAND)
    assert spans(got) == TRUE and all(r == (s + e) // 2 for s, e, r in got)
    assert len(key.calls) == (len(frames) + 15) // 16 and all(area == (0, 60, 0, 320) for _shape, area in key.calls)
    assert spans(frame_select.ChangeFrameSelector(NumpyCounter(), key_fn=frame_select.ColourKey("yellow", 48).apply).run(list(frames), BAND)) == TRUE


@pytest.mark.parametrize("pan", PANS)
def test_the_keyed_hold_selector_finds_the_truth(pan):
    frames, _ = coloured_clip(pan)
    sel = frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=3, key_fn=ref.NumpyKey(YELLOW, 48), batch=16)
    assert spans(sel.run(list(frames), BAND, 25.0)) == TRUE


# ---- the hook ---------------------------------------------------------------------------------------------------------------
class Recorder:
    """Wraps a callable and keeps the first argument of every call."""

    def __init__(self, fn):
        self.fn, self.seen = fn, []

    def __call__(self, data, *a, **kw):
        self.seen.append(data)
        return self.fn(data, *a, **kw)

    def __getattr__(self, name):
        return getattr(self.fn, name)


class RecordingCompositor:
    def __init__(self):
        self.seen = []

    def begin(self, fps, lag):
        pass

    def __call__(self, data, area, n, tracker, closed):
        self.seen.append(data)


def staged_objects(monkeypatch):
    """Every `data` staging.staged_batches hands out, in order."""
    out = []
    real = frame_select.staging.staged_batches

    def spy(batches, uploader=None):
        for items, data in real(batches, uploader):
            out.append(data)
            yield items, data
    monkeypatch.setattr(frame_select.staging, "staged_batches", spy)
    return out


def keyed_ref(data, area):
    return ref.colour_key(data, area, YELLOW, ref.slope_of(48))


@pytest.mark.parametrize("keyed", (True, False))
def test_interval_selector_hook(keyed, monkeypatch):
    frames, _ = coloured_clip((2, 3))
    staged = staged_objects(monkeypatch)
    count, focus, comp = Recorder(NumpyCounter()), Recorder(NumpyFocus()), RecordingCompositor()
    sel = frame_select.ChangeFrameSelector(count, focus_fn=focus, compositor=comp, batch=32, key_fn=ref.NumpyKey(YELLOW, 48) if keyed else None)
    sel.run(list(frames), BAND, 25.0)
    assert len(staged) == len(count.seen) == len(focus.seen) == 3 and len(comp.seen) == 4
    for k, data in enumerate(staged):
        assert comp.seen[k] is data                                          # pictures are made of the original band
        if keyed:
            assert count.seen[k] is focus.seen[k] and np.array_equal(count.seen[k], keyed_ref(data, (0, 60, 0, 320)))
            assert not np.array_equal(count.seen[k], data)
        else:
            assert count.seen[k] is data and focus.seen[k] is data


@pytest.mark.parametrize("keyed", (True, False))
def test_calibrating_selector_hook(keyed, monkeypatch):
    from test_streaming_calibration import NumpyCellsCounts
    frames, _ = coloured_clip((0, 0))
    staged = staged_objects(monkeypatch)
    count, cells = Recorder(NumpyCounter()), Recorder(NumpyCellsCounts())
    sel = frame_select.CalibratingChangeSelector(count, cells, lambda area, q, _c: cells.fn.export(area, q, count.fn), window=40, batch=32,
                                                 key_fn=ref.NumpyKey(YELLOW, 48) if keyed else None)
    sel.run(list(frames), BAND, 25.0)
    area = (0, 60, 0, 320)
    parts = [staged[0], staged[1][:8], staged[1][8:], staged[2]]         # the window of 40 frames splits the second batch
    got = [d for d in cells.seen if d is not None] + count.seen
    assert len(got) == 4
    for data, seen in zip(parts, got):
        assert np.array_equal(seen, keyed_ref(data, area) if keyed else data)
    if not keyed:
        assert got[0] is staged[0] and got[3] is staged[2]
    else:
        # the choice falls on the keyed cells, and from there on this is the keyed change selector at the chosen threshold
        plain = frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=sel.edge_thresh, key_fn=ref.NumpyKey(YELLOW, 48))
        assert sel.edge_thresh is not None and sel.intervals == plain.run(list(frames), BAND) and np.array_equal(sel.counts, plain.counts)


@pytest.mark.parametrize("cls, cells_cls, count_cls, more", (
    (frame_select.LocatingChangeSelector, NumpyCellsMasks, NumpyCounter, {}),
    (frame_select.LocatingHoldSelector, NumpyCellsHoldMasks, NumpyHoldCounter, {"hold_frames": 3})))
@pytest.mark.parametrize("keyed", (True, False))
def test_locating_selector_hook(cls, cells_cls, count_cls, more, keyed, monkeypatch):
    frames, _ = coloured_clip((0, 0))
    staged = staged_objects(monkeypatch)
    count, cells = Recorder(count_cls()), Recorder(cells_cls())
    key = ref.NumpyKey(YELLOW, 48) if keyed else None
    sel = cls(count, cells, lambda area, q, rect, _c, *a: cells.fn.replay(area, q, rect, count.fn, *a), window=64, batch=32, key_fn=key, locator_params={"min_seconds": 0.2, "min_edges": 8}, **more)
    for _ in sel.iter_run(list(frames), None, 25.0):
        pass
    whole = (0, 120, 0, 320)
    fed = [d for d in cells.seen if d is not None]
    assert len(fed) == 2 and sel.decided
    for data, seen in zip(staged[:2], fed):
        assert np.array_equal(seen, keyed_ref(data, whole)) if keyed else seen is data
    if keyed:
        assert sel.area is not None                                      # the keyed window shows the text and nothing else
        y0, y1, x0, x1 = frame_select.clip_area(sel.area, 120, 320)
        target = (0, y1 - y0, x0, x1)
        assert key.calls[:2] == [((32, 120, 320, 3), whole)] * 2 and key.calls[2:] == [((len(frames) - 64, y1 - y0, 320, 3), target)]
        rest = [d for d in count.seen if len(d)]
        assert len(rest) == 1 and np.array_equal(rest[0], keyed_ref(staged[2], target))          # keyed over the located rectangle
    elif sel.area is not None:
        assert [d for d in count.seen if len(d)][0] is staged[2]


@pytest.mark.parametrize("keyed", (True, False))
def test_area_locator_hook(keyed, monkeypatch):
    frames, _ = coloured_clip((2, 3))
    staged = staged_objects(monkeypatch)
    cells = Recorder(NumpyCells())
    loc = area_locator.AreaLocator(cells, batch=32, min_seconds=0.2, min_edges=8, key_fn=ref.NumpyKey(YELLOW, 48) if keyed else None)
    loc.run(list(frames), 25.0)
    fed = [d for d in cells.seen if d is not None]
    assert len(fed) == len(staged) == 3
    for data, seen in zip(staged, fed):
        assert np.array_equal(seen, keyed_ref(data, (0, 120, 0, 320))) if keyed else seen is data


# ---- the locator on the keyed clip ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pan", PANS)
def test_the_keyed_locator_finds_the_text(pan):
    """Run with the numpy cells reference first: on both pans the rectangle contains the text's rows and columns, so that is asserted.
    The text is one line of height 20 that ends 10 pixels above the bottom edge; its widest line fills the columns measured here."""
    frames, _ = coloured_clip(pan)
    k = ref.key_plane(frames, YELLOW, ref.slope_of(1))                   # 255 exactly where a pixel is the fill colour
    text = (k == 255).sum(0) >= 14                                       # ... in at least the shortest subtitle's frames
    rows, cols = np.flatnonzero(text.any(1)), np.flatnonzero(text.any(0))
    assert 85 <= rows[0] and rows[-1] < 110
    loc = area_locator.AreaLocator(NumpyCells(), min_seconds=0.2, key_fn=ref.NumpyKey(YELLOW, 48))
    area = loc.run(list(frames), 25.0)
    print("located", area, "text rows", rows[0], rows[-1], "columns", cols[0], cols[-1])
    assert area is not None
    assert area.ymin <= rows[0] and rows[-1] < area.ymax and area.xmin <= cols[0] and cols[-1] < area.xmax
    assert area.ymin >= 60                                               # ... and not the upper half of the picture


# ---- the extractor ----------------------------------------------------------------------------------------------------------
def host_key(monkeypatch):
    """The extractor's default key_fn is EngineKey on the shim's device; here the same ColourKey is applied in numpy."""
    made = []

    def engine_key(ctx, key):
        made.append(key)
        return key.apply
    monkeypatch.setattr(frame_select, "EngineKey", engine_key)
    return made


@pytest.mark.parametrize("pan", PANS)
@pytest.mark.parametrize("selector, counter, params", (("change", NumpyCounter, {}), ("hold", NumpyHoldCounter, {"hold_frames": 3})))
def test_extractor_text_colour(selector, counter, params, pan, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    made = host_key(monkeypatch)
    frames, truth = coloured_clip(pan)
    shown = stamped(frames)
    want = [(s, e, (s + e) // 2) for s, e, _t in truth]
    texts = {}
    for one_pass in (False, True):
        src = extractor.ArraySource(list(shown), 25.0)
        ocr = BandOcr(truth, True)
        handed = []
        predict = ocr.predict
        ocr.predict = lambda img: (handed.append(np.array(img)), predict(img))[1]
        ocr.predict_batch = lambda imgs: [ocr.predict(np.asarray(f)) for f in imgs]
        ex = extractor.SubtitleExtractor(src, ocr, sub_area=BAND, mode="fast", frame_selector=selector, change_counter=counter(),
                                         change_params={"text_colour": "#FFFF00", "colour_tol": 48, **params}, drop_score=0.0, batch=8,
                                         one_pass=one_pass)
        texts[one_pass] = ex.run()
        assert ex.intervals == want and ex.colour_key.bgr == YELLOW and ex.colour_key.tol == 48
        assert sorted(ocr.seen) == [r for _s, _e, r in want]
        for img in handed:                                               # the recogniser reads the yellow-on-colour frames themselves
            no = int(img[0, 0, 0]) | (int(img[0, 0, 1]) << 8)
            assert np.array_equal(img, shown[no - 1])
    assert made and all(k.bgr == YELLOW for k in made)
    text = texts[False]
    assert texts[True] == text and text.count(" --> ") == 4
    for (s, e, t) in truth:
        assert f"{srt.frame_to_timecode(s, 25.0)} --> {srt.frame_to_timecode(e, 25.0)}" in text and t in text
    plain = extractor.SubtitleExtractor(extractor.ArraySource(list(shown), 25.0), BandOcr(truth, True), sub_area=BAND, mode="fast",
                                        frame_selector="change", change_counter=NumpyCounter(), drop_score=0.0, batch=8)
    plain.run()
    assert plain.intervals != want and plain.colour_key is None          # without the key the luma selector misses them


def test_extractor_area_params_take_the_colour_from_change_params(monkeypatch):
    host_key(monkeypatch)
    frames, truth = coloured_clip((2, 3))
    src = extractor.ArraySource(list(frames), 25.0)
    kw = dict(sub_area="auto", mode="fast", frame_selector="change", change_counter=NumpyCounter())
    ex = extractor.SubtitleExtractor(src, BandOcr(truth, True), change_params={"text_colour": "yellow"},
                                     area_params={"cells_fn": NumpyCells(), "min_seconds": 0.2}, **kw)
    loc = ex._locator()
    assert loc.key_fn is ex.key_fn and ex.key_fn is not None
    ex = extractor.SubtitleExtractor(src, BandOcr(truth, True), change_params={"text_colour": "yellow"},
                                     area_params={"cells_fn": NumpyCells(), "text_colour": "white", "colour_tol": 24}, **kw)
    assert ex._locator().key_fn is not ex.key_fn
    own = ex._locator().key_fn(frames[:1], (0, 120, 0, 320))
    assert np.array_equal(own, ref.colour_key(frames[:1], (0, 120, 0, 320), (255, 255, 255), ref.slope_of(24)))
    ex = extractor.SubtitleExtractor(src, BandOcr(truth, True), **kw)
    assert ex.key_fn is None and ex._locator().key_fn is None
    for bad in ({"change_params": {"colour_tol": 24}}, {"change_params": {"text_colour": "mauve"}},
                {"change_params": {"text_colour": "yellow", "colour_tol": 0}}, {"frame_selector": "fps", "change_params": {"text_colour": "yellow"}},
                {"change_params": {"text_colour": "yellow", "key_fn": lambda d, a: d}},
                {"area_params": {"text_colour": "white", "streaming_locate": True, "locate_seconds": 2}}):
        with pytest.raises(ValueError):
            extractor.SubtitleExtractor(src, BandOcr(truth, True), **{**kw, **bad})


# ---- the command lines ------------------------------------------------------------------------------------------------------
def test_extractor_command_line(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = coloured_clip((2, 3))
    clip = tmp_path / "clip.npy"
    np.save(clip, stamped(frames))
    made = []

    def key_fn(key):
        made.append(key)
        return key.apply
    argv = [str(clip), "--fps", "25", "--area", "60,120,0,320", "--selector", "change", "--batch", "8"]
    rc = extractor.main(argv + ["--text-colour", "FFFF00", "--colour-tol", "48"], ocr=BandOcr(truth, True), counter=NumpyCounter(), key_fn=key_fn)
    out = capsys.readouterr().out
    assert rc == 0 and out.count(" --> ") == 4 and made[0].bgr == YELLOW and made[0].tol == 48
    for (s, e, _t) in truth:
        assert f"{srt.frame_to_timecode(s, 25.0)} --> {srt.frame_to_timecode(e, 25.0)}" in out
    rc = extractor.main(argv + ["--text-colour", "yellow"], ocr=BandOcr(truth, True), counter=NumpyCounter(), key_fn=key_fn)
    assert rc == 0 and capsys.readouterr().out == out and made[1].tol == 48
    for bad, option in ((["--text-colour", "mauve"], "--text-colour"), (["--text-colour", "yellow", "--colour-tol", "0"], "--colour-tol"),
                        (["--text-colour", "yellow", "--colour-tol", "x"], "--colour-tol"), (["--colour-tol", "24"], "--colour-tol"),
                        (["--text-colour", "#12345"], "--text-colour")):
        assert extractor.main(argv + bad, ocr=BandOcr(truth, True), counter=NumpyCounter(), key_fn=key_fn) == 2
        assert option in capsys.readouterr().err
    assert extractor.main([str(clip), "--fps", "25", "--text-colour", "yellow"], ocr=BandOcr(truth, True), key_fn=key_fn) == 2
    assert "--text-colour" in capsys.readouterr().err


def test_area_locator_command_line(tmp_path, capsys):
    frames, _ = coloured_clip((2, 3))
    clip = tmp_path / "clip.npy"
    np.save(clip, frames)
    made = []

    def key_fn(key):
        made.append(key)
        return key.apply
    rc = area_locator.main([str(clip), "--fps", "25", "--text-colour", "#ffff00", "--colour-tol", "48"], cells_fn=NumpyCells(), key_fn=key_fn)
    out = capsys.readouterr().out.split()
    assert rc == 0 and len(out) == 4 and made[0].bgr == YELLOW
    want = area_locator.AreaLocator(NumpyCells(), key_fn=ref.NumpyKey(YELLOW, 48)).run(list(frames), 25.0)
    assert [int(v) for v in out] == [want.ymin, want.ymax, want.xmin, want.xmax]
    for bad, option in ((["--text-colour", "mauve"], "--text-colour"), (["--text-colour", "yellow", "--colour-tol", "256"], "--colour-tol"),
                        (["--colour-tol", "24"], "--colour-tol")):
        assert area_locator.main([str(clip), "--fps", "25"] + bad, cells_fn=NumpyCells(), key_fn=key_fn) == 2
        assert option in capsys.readouterr().err


def test_synth_defaults_are_the_grey_clip():
    a, _ = synth.make_moving_clip(MOVING[:3], seed=4)
    b, _ = synth.make_moving_clip(MOVING[:3], seed=4, text_bgr=(255, 255, 255), outline=True, chroma=False)
    assert np.array_equal(a, b)
    import hashlib
    assert hashlib.sha256(synth.make_moving_clip(MOVING)[0].tobytes()).hexdigest() == GREY_SHA256       # the bytes before the three options
    c, _ = synth.make_moving_clip(MOVING[:3], seed=4, chroma=True, noise=0)
    g, _ = synth.make_moving_clip(MOVING[:3], seed=4, noise=0)
    assert np.array_equal(g[:7, ..., 0], g[:7, ..., 1]) and not np.array_equal(c[:7, ..., 0], c[:7, ..., 1])      # (the gap in front: no text)


GREY_SHA256 = "9ee8afc3caf68446446cfa05459a28abbb726c852650f2d3f4fa496244ae7378"
