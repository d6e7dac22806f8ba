"""The argument checks the four vse_frame_* entry points share (check_frames / check_area / check_rule in csrc/vse_runtime.hip),
through the C ABI: every refusal returns -1 in the entry point's own name before anything is enqueued, and the same call with good
arguments runs."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

BAD_AREAS = [(0, 2, 0, 10), (0, 10, 5, 7), (-1, 5, 0, 10), (0, 11, 0, 10), (0, 10, 0, 21), (4, 4, 0, 10)]
# entry point -> what its messages call the rectangle
NOUNS = {"vse_frame_change": "area", "vse_frame_cells": "region", "vse_frame_cells_multi": "region", "vse_frame_hold": "area"}


def test_frame_entry_points_refuse_before_launching(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)        # a 10 x 20 frame at pitch 60 needs 600 bytes
    st = torch.zeros(1 << 14, dtype=torch.uint8, device=ctx.tdev)         # the largest state below takes 144 bytes
    out = torch.full((64,), -7, dtype=torch.int32, device=ctx.tdev)       # the largest output below takes 8 ints
    ths = (C.c_int * 2)(32, 128)

    def call(name, n=1, area=(0, 10, 0, 20), state=st):
        frames = (ctx.handle, C.c_void_p(buf.data_ptr()), n, 10, 20, 60, 600, *area)
        state = C.c_void_p(state.data_ptr()) if state is not None else None
        res, stream = C.c_void_p(out.data_ptr()), ctx.stream()
        if name == "vse_frame_change":
            return lib.vse_frame_change(*frames, 128, state, 1, res, stream)
        if name == "vse_frame_cells":
            return lib.vse_frame_cells(*frames, 128, 16, 1, 2, 2, 5, state, 1, 1, res, None, stream)
        if name == "vse_frame_cells_multi":
            return lib.vse_frame_cells_multi(*frames, ths, 2, 16, 1, 2, 2, 5, state, 1, 1, res, stream)
        return lib.vse_frame_hold(*frames, 128, 2, state, 0, 1, res, stream)

    for name, noun in NOUNS.items():
        for area in BAD_AREAS:
            assert call(name, area=area) == -1, (name, area)
            msg = lib.vse_last_error().decode()
            assert msg.startswith(name + ":") and noun in msg, msg
        for kw in (dict(n=-1), dict(state=None)):
            assert call(name, **kw) == -1, (name, kw)
            msg = lib.vse_last_error().decode()
            assert msg.startswith(name + ":") and "bad arguments" in msg, msg
    torch.cuda.synchronize()
    assert set(out.cpu().tolist()) == {-7} and int(st.count_nonzero()) == 0      # nothing was enqueued
    for name in NOUNS:
        assert call(name) == 0, (name, lib.vse_last_error().decode())
    torch.cuda.synchronize()
    assert out.cpu().tolist()[:3] == [0, 0, 0]                                   # a black frame has no edges
