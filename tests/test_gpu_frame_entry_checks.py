"""The argument checks the ten vse_frame_* entry points that take frames share (check_frames / check_area / check_rule / check_thresholds /
check_hold / check_hold_bounded in csrc/vse_runtime.hip), through the C ABI: every refusal returns -1 in the entry point's own name before
anything is enqueued, and the same call with good arguments runs."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

BAD_AREAS = [(0, 2, 0, 10), (0, 10, 5, 7), (-1, 5, 0, 10), (0, 11, 0, 10), (0, 10, 0, 21), (4, 4, 0, 10)]
# entry point -> what its messages call the rectangle
NOUNS = {"vse_frame_change": "area", "vse_frame_cells": "region", "vse_frame_cells_multi": "region", "vse_frame_hold": "area",
         "vse_frame_focus": "area", "vse_frame_cells_counts": "region", "vse_frame_cells_masks": "region",
         "vse_frame_hold_bounded": "area", "vse_frame_cells_hold": "region", "vse_frame_cells_hold_bounded": "region"}
TAKES_THRESHOLDS = ["vse_frame_cells_multi", "vse_frame_cells_counts", "vse_frame_cells_masks", "vse_frame_cells_hold",
                    "vse_frame_cells_hold_bounded"]
# (thresholds or None, nt) -> the message behind the entry point's name
BAD_THRESHOLDS = [
    (None, 2, "2 thresholds (1..8, not NULL)"),
    ((32, 128), 0, "0 thresholds (1..8, not NULL)"),
    ((1, 2, 3, 4, 5, 6, 7, 8, 9), 9, "9 thresholds (1..8, not NULL)"),
    ((0, 128), 2, "threshold 0 of 2 is 0 (each 1..255, ascending and distinct)"),
    ((32, 256), 2, "threshold 1 of 2 is 256 (each 1..255, ascending and distinct)"),
    ((128, 32), 2, "threshold 1 of 2 is 32 (each 1..255, ascending and distinct)"),
    ((32, 32), 2, "threshold 1 of 2 is 32 (each 1..255, ascending and distinct)"),
]
BAD_HOLDS = {
    "vse_frame_hold": [(dict(hold=0), "hold 0 outside 1..32"), (dict(hold=33), "hold 33 outside 1..32")],
    "vse_frame_cells_hold": [(dict(hold=0), "hold 0 outside 1..32"), (dict(hold=33), "hold 33 outside 1..32")],
}
for _name in ("vse_frame_hold_bounded", "vse_frame_cells_hold_bounded"):
    BAD_HOLDS[_name] = [(dict(hold=h, max_hold=m), f"hold {h} outside 1..32, or max_hold {m} outside hold..4000")
                        for h, m in ((0, 4), (33, 40), (3, 2), (2, 4001))]


def test_frame_entry_points_refuse_before_launching(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # a 10 x 20 frame at pitch 60 needs 600 bytes
    st = torch.zeros(1 << 14, dtype=torch.uint8, device=ctx.tdev)         # the largest state below takes 2608 bytes
    out = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)       # the largest output below takes 8 ints
    aux = torch.full((64,), -7, dtype=torch.int64, device=ctx.tdev)       # the second output of _counts (6 ints) and _masks (16 words)

    def call(name, n=1, area=(0, 10, 0, 20), state=st, ths=(32, 128), nt=2, hold=2, max_hold=4):
        frames = (ctx.handle, C.c_void_p(buf.data_ptr()), n, 10, 20, 60, 600, *area)
        state = C.c_void_p(state.data_ptr()) if state is not None else None
        res, more, stream = C.c_void_p(out.data_ptr()), C.c_void_p(aux.data_ptr()), ctx.stream()
        ths = (C.c_int * len(ths))(*ths) if ths is not None else None
        rule = (16, 1, 2, 2, 5)
        if name == "vse_frame_change":
            return lib.vse_frame_change(*frames, 128, state, 1, res, stream)
        if name == "vse_frame_focus":
            return lib.vse_frame_focus(*frames, 128, state, 1, res, stream)
        if name == "vse_frame_cells":
            return lib.vse_frame_cells(*frames, 128, *rule, state, 1, 1, res, None, stream)
        if name == "vse_frame_cells_multi":
            return lib.vse_frame_cells_multi(*frames, ths, nt, *rule, state, 1, 1, res, stream)
        if name == "vse_frame_cells_counts":
            return lib.vse_frame_cells_counts(*frames, ths, nt, *rule, state, 1, 1, res, more, stream)
        if name == "vse_frame_cells_masks":
            return lib.vse_frame_cells_masks(*frames, ths, nt, *rule, state, 1, 1, res, more, 1, 0, stream)
        if name == "vse_frame_hold":
            return lib.vse_frame_hold(*frames, 128, hold, state, 0, 1, res, stream)
        if name == "vse_frame_hold_bounded":
            return lib.vse_frame_hold_bounded(*frames, 128, hold, max_hold, state, 0, 1, res, stream)
        if name == "vse_frame_cells_hold":
            return lib.vse_frame_cells_hold(*frames, ths, nt, hold, *rule, state, 0, 1, res, None, stream)
        assert name == "vse_frame_cells_hold_bounded"
        return lib.vse_frame_cells_hold_bounded(*frames, ths, nt, hold, max_hold, *rule, state, 0, 1, res, None, stream)

    for name, noun in NOUNS.items():
        for area in BAD_AREAS:
            assert call(name, area=area) == -1, (name, area)
            msg = lib.vse_last_error().decode()
            assert msg.startswith(name + ":") and noun in msg, msg
        for kw in (dict(n=-1), dict(state=None)):
            assert call(name, **kw) == -1, (name, kw)
            msg = lib.vse_last_error().decode()
            assert msg.startswith(name + ":") and "bad arguments" in msg, msg
    for name in TAKES_THRESHOLDS:
        for ths, nt, text in BAD_THRESHOLDS:
            assert call(name, ths=ths, nt=nt) == -1, (name, ths, nt)
            assert lib.vse_last_error().decode() == f"{name}: {text}"
    for name, cases in BAD_HOLDS.items():
        for kw, text in cases:
            assert call(name, **kw) == -1, (name, kw)
            assert lib.vse_last_error().decode() == f"{name}: {text}"
    torch.cuda.synchronize()
    assert set(out.cpu().tolist()) == {-7} and set(aux.cpu().tolist()) == {-7} and int(st.count_nonzero()) == 0      # nothing was enqueued
    for name in NOUNS:
        assert call(name) == 0, (name, lib.vse_last_error().decode())
    torch.cuda.synchronize()
    assert out.cpu().tolist()[:3] == [0, 0, 0]                                   # a black frame has no edges
