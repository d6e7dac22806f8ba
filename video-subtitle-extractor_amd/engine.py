"""ctypes binding of libvse_hip.so (include/vse_hip.h) + plan cache on top of the graph compiler.

PyTorch is plumbing here: device memory (torch.empty on cuda), streams and torch.distributed.  All compute
goes through the C ABI; there is NO fallback — if the library or a gfx950 GPU is missing, calls raise.
"""
import ctypes as C
import os
import threading
from collections import namedtuple

import numpy as np

from . import compiler, ir

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VSE_LIB_PATH") or os.path.join(_HERE, "libvse_hip.so")      # (VSE_LIB_PATH: a library built elsewhere)

EXPORTS = [
    "vse_init", "vse_destroy", "vse_last_error", "vse_sizeof_op", "vse_sizeof_view", "vse_abi_version",
    "vse_weights_upload", "vse_weights_free", "vse_plan_create", "vse_plan_destroy", "vse_plan_run", "vse_plan_run_ragged",
    "vse_plan_width_levels", "vse_plan_profile", "vse_op_kernel_name", "vse_det_preprocess", "vse_db_workspace_bytes",
    "vse_db_postprocess", "vse_rec_preprocess", "vse_rec_preprocess_scratch_bytes", "vse_ctc_collapse", "vse_ctc_collapse_ragged",
    "vse_det_forward", "vse_rec_forward", "vse_plan_set_source", "vse_plan_takes_frames",
    "vse_rec_graph_create", "vse_graph_launch", "vse_graph_destroy", "vse_frame_change_state_bytes", "vse_frame_change",
    "vse_audio_match_workspace_bytes", "vse_audio_match", "vse_scene_change_state_bytes", "vse_scene_change_workspace_bytes",
    "vse_scene_change", "vse_frame_cells_dims", "vse_frame_cells_state_bytes", "vse_frame_cells",
    "vse_interval_state_bytes", "vse_interval_accumulate", "vse_interval_composite", "vse_interval_rank", "vse_frame_hold_state_bytes",
    "vse_frame_hold",
    "vse_audio_stream_length", "vse_audio_stream_workspace_bytes", "vse_audio_stream_feed", "vse_audio_stream_finish", "vse_ctc_fuse",
    "vse_yuv_to_bgr_matrix", "vse_frame_cells_multi_state_bytes", "vse_frame_cells_multi",
    "vse_frame_cells_hold_state_bytes", "vse_frame_cells_hold", "vse_frame_focus",
    "vse_frame_hold_bounded_state_bytes", "vse_frame_hold_bounded",
    "vse_frame_cells_hold_bounded_state_bytes", "vse_frame_cells_hold_bounded",
    "vse_interval_stream_state_bytes", "vse_interval_stream", "vse_interval_ring_rank",
    "vse_yuv_frame_bytes", "vse_yuv_to_bgr_format", "vse_yuv_deinterlace", "vse_yuv_field_match",
    "vse_yuv_tonemap_table_bytes", "vse_yuv_to_bgr_tonemap", "vse_yuv_resample_table_bytes", "vse_yuv_resample",
    "vse_yuv_vscale", "vse_frame_cells_counts", "vse_frame_cells_export_state",
    "vse_frame_masks_bytes", "vse_frame_cells_masks", "vse_frame_masks_replay",
    "vse_frame_cells_hold_masks", "vse_frame_masks_replay_hold",
    "vse_frame_cells_hold_bounded_masks", "vse_frame_masks_replay_hold_bounded", "vse_colour_key",
]
# Entry points whose names carry a digit.  tests/test_abi.py reads the header's function names with a letters-only pattern and holds
# them equal to EXPORTS, so these are listed apart; load_library checks both lists, tests/test_yuv_ingest.py holds header = library =
# this list for them (exactly these two, which is why vse_yuv_to_bgr_matrix is spelled without the 420).
EXPORTS_NUMBERED = ["vse_yuv420_frame_bytes", "vse_yuv420_to_bgr"]


class VseError(RuntimeError):
    pass


# The integer parameters of vse_frame_cells (include/vse_hip.h): the edge threshold and the per-cell interval rule.
CellParams = namedtuple("CellParams", "edge_thresh min_edges ratio_num ratio_den min_frames max_frames")


class CellsState:
    """What vse_frame_cells carries from one call to the next: `words` (the cells' last masks and open runs) and `totals`, cuda int32
    [gy,gx,4] = covered, runs, present, cuts per cell so far."""

    def __init__(self, words, totals):
        self.words, self.totals = words, totals


class MasksBuffer:
    """The mask buffer of vse_frame_cells_masks (include/vse_hip.h): `words`, cuda uint8 of vse_frame_masks_bytes(area_h, area_w, nt, cap),
    `cap` frame slots of the edge masks of a region of area_h x area_w pixels at nt thresholds, one bit per interior pixel."""

    def __init__(self, words, area_h, area_w, nt, cap):
        self.words, self.area_h, self.area_w, self.nt, self.cap = words, int(area_h), int(area_w), int(nt), int(cap)


class DeviceState:
    """Base of the callables that run a stateful kernel on a Context batch by batch (frame_select.EngineCounter, EngineHoldCounter,
    EngineCompositor, EngineStreamer, area_locator.EngineCells, keyframes.EngineSceneCounter): host frames become a device tensor, and the device
    state is allocated afresh when the geometry it was made for changes."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._key = self._state = None

    def _device(self, frames):
        t = self.ctx.torch
        return frames if t.is_tensor(frames) else t.from_numpy(np.ascontiguousarray(frames)).to(self.ctx.tdev)

    def _fresh(self, key, make):
        """-> True when `key` is not the last call's: the state is then a new make(*key), and the caller resets."""
        if self._key == key:
            return False
        self._key, self._state = key, make(*key)
        return True


class IntervalSeg(C.Structure):
    """vse_interval_seg (include/vse_hip.h)."""
    _fields_ = [("first", C.c_int64), ("last", C.c_int64), ("flags", C.c_int32), ("frames", C.c_int32), ("out", C.c_int32)]


class IntervalRingGroup(C.Structure):
    """vse_interval_ring_group (include/vse_hip.h)."""
    _fields_ = [("n", C.c_int32), ("rank", C.c_int32), ("out", C.c_int32), ("frames", C.c_int64 * 63)]


class DbParams(C.Structure):
    _fields_ = [("box_thresh", C.c_double), ("unclip_ratio", C.c_double), ("thresh", C.c_float),
                ("max_candidates", C.c_int), ("min_size", C.c_int)]


class Box(C.Structure):
    _fields_ = [("pts", C.c_float * 2 * 4), ("score", C.c_float), ("frame", C.c_int)]


class Crop(C.Structure):
    _fields_ = [("quad", C.c_float * 2 * 4), ("frame", C.c_int), ("crop_w", C.c_int), ("crop_h", C.c_int),
                ("resized_w", C.c_int), ("rotate", C.c_int)]


CROP_DT = np.dtype([("quad", "<f4", (4, 2)), ("frame", "<i4"), ("crop_w", "<i4"), ("crop_h", "<i4"), ("resized_w", "<i4"),
                    ("rotate", "<i4")])
assert CROP_DT.itemsize == C.sizeof(Crop)

_lib = None


def load_library(path=None):
    """dlopen the C-ABI library and bind signatures.  Works without a GPU (used by the CPU test-suite to check
    that every symbol of include/vse_hip.h is exported and that the record layouts agree)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must be imported BEFORE libvse_hip.so: the torch wheel bundles its own libamdhip64; if ours (linked against
    # /opt/rocm) initialises first, two HIP runtimes end up in the process and one of them sees no device
    import torch  # noqa: F401
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise VseError(f"{path} not found: run `python __graft_entry__.py` (hipcc --offload-arch=gfx950) first; "
                       "there is no CPU fallback for the OCR hot path")
    lib = C.CDLL(path)
    for name in EXPORTS + EXPORTS_NUMBERED:
        if not hasattr(lib, name):
            raise VseError(f"libvse_hip.so does not export {name}")

    lib.vse_last_error.restype = C.c_char_p
    lib.vse_sizeof_op.restype = C.c_size_t
    lib.vse_sizeof_view.restype = C.c_size_t
    lib.vse_db_workspace_bytes.restype = C.c_size_t
    lib.vse_db_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_rec_preprocess_scratch_bytes.restype = C.c_size_t
    lib.vse_rec_preprocess_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_init.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.vse_destroy.argtypes = [C.c_void_p]
    lib.vse_destroy.restype = None
    lib.vse_weights_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.vse_weights_free.argtypes = [C.c_void_p, C.c_int]
    lib.vse_plan_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.vse_plan_destroy.argtypes = [C.c_void_p]
    lib.vse_plan_destroy.restype = None
    lib.vse_plan_run.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
    lib.vse_plan_run_ragged.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p]
    lib.vse_plan_width_levels.argtypes = [C.c_void_p]
    lib.vse_rec_graph_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.vse_graph_launch.argtypes = [C.c_void_p, C.c_void_p]
    lib.vse_graph_destroy.argtypes = [C.c_void_p]
    lib.vse_graph_destroy.restype = None
    lib.vse_plan_set_source.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64]
    lib.vse_plan_takes_frames.argtypes = [C.c_void_p]
    lib.vse_det_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vse_rec_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vse_plan_profile.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_float)]
    lib.vse_op_kernel_name.argtypes = [C.c_void_p]
    lib.vse_op_kernel_name.restype = C.c_char_p
    lib.vse_det_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.c_void_p]
    lib.vse_db_postprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(DbParams), C.c_void_p, C.c_size_t, C.POINTER(Box), C.c_int,
                                       C.POINTER(C.c_int), C.c_void_p]
    lib.vse_rec_preprocess.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                       C.POINTER(Crop), C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_size_t, C.c_void_p]
    lib.vse_ctc_collapse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    lib.vse_ctc_collapse_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    lib.vse_ctc_fuse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p]
    lib.vse_frame_change_state_bytes.restype = C.c_size_t
    lib.vse_frame_change_state_bytes.argtypes = [C.c_int, C.c_int]
    lib.vse_frame_change.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.vse_frame_focus.argtypes = lib.vse_frame_change.argtypes
    lib.vse_colour_key.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.vse_frame_cells_dims.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.vse_frame_cells_state_bytes.restype = C.c_size_t
    lib.vse_frame_cells_state_bytes.argtypes = [C.c_int, C.c_int]
    lib.vse_frame_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vse_frame_cells_multi_state_bytes.restype = C.c_size_t
    lib.vse_frame_cells_multi_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_frame_cells_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.vse_frame_cells_counts.argtypes = lib.vse_frame_cells_multi.argtypes[:-1] + [C.c_void_p, C.c_void_p]
    lib.vse_frame_cells_export_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.vse_frame_masks_bytes.restype = C.c_size_t
    lib.vse_frame_masks_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.vse_frame_cells_masks.argtypes = lib.vse_frame_cells_multi.argtypes[:-1] + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.vse_frame_masks_replay.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 12 + [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vse_frame_hold_state_bytes.restype = C.c_size_t
    lib.vse_frame_hold_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_frame_hold.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    lib.vse_frame_hold_bounded_state_bytes.restype = C.c_size_t
    lib.vse_frame_hold_bounded_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_frame_hold_bounded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    lib.vse_frame_cells_hold_state_bytes.restype = C.c_size_t
    lib.vse_frame_cells_hold_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.vse_frame_cells_hold.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vse_frame_cells_hold_masks.argtypes = lib.vse_frame_cells_hold.argtypes[:-1] + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.vse_frame_masks_replay_hold.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 12 + [C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                                                                              C.c_void_p]
    lib.vse_frame_cells_hold_bounded_state_bytes.restype = C.c_size_t
    lib.vse_frame_cells_hold_bounded_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.vse_frame_cells_hold_bounded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.vse_frame_cells_hold_bounded_masks.argtypes = lib.vse_frame_cells_hold_bounded.argtypes[:-1] + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.vse_frame_masks_replay_hold_bounded.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 13 + [C.c_void_p, C.c_int64, C.c_int, C.c_void_p,
                                                                                                      C.c_void_p]
    lib.vse_interval_state_bytes.restype = C.c_size_t
    lib.vse_interval_state_bytes.argtypes = [C.c_int, C.c_int]
    lib.vse_interval_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.vse_interval_composite.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.vse_interval_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    lib.vse_interval_stream_state_bytes.restype = C.c_size_t
    lib.vse_interval_stream_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_interval_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int, C.c_int64, C.POINTER(IntervalSeg), C.c_int, C.c_int64, C.c_int,
                                        C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.vse_interval_ring_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_int64, C.c_int64, C.c_void_p]
    lib.vse_audio_match_workspace_bytes.restype = C.c_size_t
    lib.vse_audio_match_workspace_bytes.argtypes = [C.c_void_p, C.c_int]
    lib.vse_audio_match.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_void_p]
    lib.vse_audio_stream_length.restype = C.c_int64
    lib.vse_audio_stream_length.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
    lib.vse_audio_stream_workspace_bytes.restype = C.c_size_t
    lib.vse_audio_stream_workspace_bytes.argtypes = [C.c_int64, C.c_int, C.c_int, C.c_int]
    lib.vse_audio_stream_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_size_t, C.c_void_p]
    lib.vse_audio_stream_finish.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    lib.vse_scene_change_state_bytes.restype = C.c_size_t
    lib.vse_scene_change_state_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_scene_change_workspace_bytes.restype = C.c_size_t
    lib.vse_scene_change_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.vse_scene_change.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.vse_yuv420_frame_bytes.restype = C.c_size_t
    lib.vse_yuv420_frame_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.vse_yuv420_to_bgr.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                      C.c_int64, C.c_int64, C.c_void_p]
    lib.vse_yuv_to_bgr_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                          C.c_int64, C.c_int64, C.c_int, C.c_void_p]
    lib.vse_yuv_frame_bytes.restype = C.c_size_t
    lib.vse_yuv_frame_bytes.argtypes = [C.c_int] * 7
    lib.vse_yuv_to_bgr_format.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 11 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.vse_yuv_tonemap_table_bytes.restype = C.c_size_t
    lib.vse_yuv_tonemap_table_bytes.argtypes = []
    lib.vse_yuv_to_bgr_tonemap.argtypes = lib.vse_yuv_to_bgr_format.argtypes[:-1] + [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
    lib.vse_yuv_resample_table_bytes.restype = C.c_size_t
    lib.vse_yuv_resample_table_bytes.argtypes = [C.c_int, C.c_int]
    lib.vse_yuv_resample.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 10 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                     C.c_int64, C.c_void_p]
    lib.vse_yuv_vscale.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 13 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p,
                                   C.c_int64, C.c_void_p]
    lib.vse_yuv_deinterlace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 11 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    lib.vse_yuv_field_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 12 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                                                                 C.c_void_p]
    if lib.vse_sizeof_op() != ir.OP_DT.itemsize or lib.vse_sizeof_view() != ir.VIEW_DT.itemsize:
        raise VseError(f"ABI mismatch: vse_op {lib.vse_sizeof_op()} vs {ir.OP_DT.itemsize}, "
                       f"vse_view {lib.vse_sizeof_view()} vs {ir.VIEW_DT.itemsize}")
    _lib = lib
    return lib


def op_kernel_names(ops):
    """The kernel each record of an ir.OP_DT array launches, as rocprofv3 names it (vse_op_kernel_name; no GPU needed)."""
    lib = load_library()
    ops = np.ascontiguousarray(ops)
    base = ops.ctypes.data
    return [lib.vse_op_kernel_name(C.c_void_p(base + i * ops.itemsize)).decode() for i in range(len(ops))]


def profiled_kernel_names(ops, ms):
    """op_kernel_names for a profiled run.  A plan runs a 3x3 conv and the max-pool record behind it as ONE kernel where it may
    (conv_pool_select, csrc/conv_select.hip); vse_plan_profile then gives the whole time to the conv and exactly 0 to the pool, and
    here the conv is named as rocprofv3 names that launch: conv_c3pool_kernel<couts per tile of the conv's own kernel>."""
    names = op_kernel_names(ops)
    for i in range(1, len(names)):
        if (int(ops[i]["kind"]) == ir.OP_POOL and int(ops[i - 1]["kind"]) == ir.OP_CONV and float(ms[i]) == 0.0
                and names[i - 1].startswith("conv_patch_kernel<")):
            names[i - 1] = "conv_c3pool_kernel<%s>" % names[i - 1].split(",")[1].strip()
    return names


def _check(rc, what):
    if rc < 0:
        raise VseError(f"{what} failed (rc={rc}): {load_library().vse_last_error().decode(errors='replace')}")
    return rc


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise VseError("no HIP device visible: the OCR hot path runs only on MI355X (gfx950); no CPU fallback")
    return torch


def _packed_stride(a, n, frame, what):
    """The frame stride in bytes of the uint8 tensor `a` that holds n packed pictures of `frame` bytes: 1-D (back to back) or 2-D
    [n, stride]."""
    assert str(a.dtype) == "torch.uint8" and a.dim() in (1, 2) and a.stride(-1) == 1, what
    if a.dim() == 2:
        assert a.shape[0] == n and a.shape[1] >= frame, (what, tuple(a.shape), n, frame)
        return a.stride(0) if n > 1 else max(a.stride(0), frame)
    assert a.numel() >= n * frame, (what, a.numel(), n, frame)
    return frame


def _prev_pictures(prev, prev_stride, n, sstride):
    """(pointer, frame stride) of the previous pictures of yuv_deinterlace / yuv_field_match; (None, 0) without any"""
    if prev is None:
        return None, 0
    assert str(prev.dtype) == "torch.uint8" and prev.stride(-1) == 1
    return C.c_void_p(prev.data_ptr()), int(prev_stride) if prev_stride is not None else (prev.stride(0) if prev.dim() == 2 and n > 1 else sstride)


class Context:
    """One per (process, device)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.torch = _torch()
        self.device = device
        self.handle = C.c_void_p()
        _check(self.lib.vse_init(device, C.byref(self.handle)), "vse_init")
        self.tdev = self.torch.device("cuda", device)
        self._tone_tables = {}            # ingest.ToneMap -> (cuda uint8 [16128] table, its gamut as int32[9]): uploaded once
        self._tone_lock = threading.Lock()
        self._resample_tables = {}        # (ingest.Resample, sub_x, has chroma) -> ((cuda uint8 luma table, taps), (chroma table, taps) | None)
        self._vscale_tables = {}          # (ingest.VScale, sub_y, has chroma) -> the same, each with its rows' support (lo, hi) on the host

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.tdev).cuda_stream)

    def _frames_args(self, frames_u8, allow_empty=False):
        """cuda uint8 [n,H,W,3] with packed pixels (any row pitch / frame stride) -> (pointer, n, h, w, pitch, frame stride) as the
        entry points that read frames take them.  allow_empty: n == 0 (a flush alone) passes a NULL pointer and the strides of
        packed frames: no frames, no strides to speak of."""
        assert frames_u8.dtype == self.torch.uint8 and frames_u8.dim() == 4 and frames_u8.shape[3] == 3
        n, h, w, _ = frames_u8.shape
        if allow_empty and not n:
            return None, 0, h, w, 3 * w, 3 * w * h
        assert frames_u8.stride(3) == 1 and frames_u8.stride(2) == 3
        return C.c_void_p(frames_u8.data_ptr()), n, h, w, frames_u8.stride(1), frames_u8.stride(0)

    # ---- streams ----------------------------------------------------------------------------------------
    def streams_concurrent(self, a, b, spin_cycles=1_500_000):
        """Do streams a and b really run side by side?  torch hands streams out of a round-robin pool of 32 per priority and the HIP
        runtime multiplexes them over a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default; a queue is bound at a stream's
        FIRST use): two streams on one hardware queue execute in order whatever the program says.  Measured: a short kernel on b is
        launched behind a long spin on a; concurrent = it finishes while the spin still runs."""
        t = self.torch
        x = self.__dict__.setdefault("_probe_buf", t.zeros(64, device=self.tdev))
        for s in (a, b):                       # bind both streams to their hardware queues first (a first use costs milliseconds)
            with t.cuda.stream(s):
                x.add_(1)
        t.cuda.synchronize(self.tdev)
        a0, a1, b1 = (t.cuda.Event(enable_timing=True) for _ in range(3))
        with t.cuda.stream(a):
            a0.record()
            t.cuda._sleep(spin_cycles)
            a1.record()
        with t.cuda.stream(b):
            x.add_(1)
            b1.record()
        t.cuda.synchronize(self.tdev)
        return a0.elapsed_time(b1) < 0.5 * a0.elapsed_time(a1)

    def side_streams(self, n, priority=0, tries=24, role="default"):
        """n streams of the given priority that run concurrently with each other AND with the current stream (verified by
        streams_concurrent), cached per (priority, role): every pipeline of the process gets the same ones for the same role, and two
        roles — the detector batches in flight ("det") and the recogniser's width groups ("rec") — never receive the same stream objects,
        whatever their priorities (with one list per priority, equal priorities made the detector / recogniser overlap serialise
        silently).  A candidate is also checked against the streams of the OTHER roles: preferred when it runs beside all of them
        (the device has a handful of hardware queues: not always possible), accepted after half the tries when it only runs beside
        its own list and the main stream (`side_streams_cross_verified` tells)."""
        t = self.torch
        cache = self.__dict__.setdefault("_side_streams", {})
        have = cache.setdefault((priority, role), [])
        others = [s for k, lst in cache.items() if k != (priority, role) for s in lst]
        main = t.cuda.current_stream(self.tdev)
        budget = tries
        while len(have) < n and tries > 0:
            tries -= 1
            s = t.cuda.Stream(device=self.tdev, priority=priority)
            if any(s.cuda_stream == h.cuda_stream for h in have + others):
                continue
            if not (self.streams_concurrent(main, s) and all(self.streams_concurrent(h, s) for h in have)):
                continue
            cross = all(self.streams_concurrent(o, s) for o in others)
            if cross or tries < budget // 2:
                if not cross:
                    self.side_streams_cross_verified = False
                have.append(s)
        if len(have) < n:
            # nothing on this device runs side by side right now — a profiler that serialises dispatches (rocprofv3 --pmc), one hardware
            # queue, a debugger: concurrency is an optimisation, not a requirement, so the plain pool streams do (results are identical)
            import warnings
            warnings.warn(f"only {len(have)} of {n} HIP streams of priority {priority} verified to run concurrently; using unverified ones")
            self.side_streams_verified = False
            while len(have) < n:
                s = t.cuda.Stream(device=self.tdev, priority=priority)
                if not any(s.cuda_stream == h.cuda_stream for h in have + others) or tries < -64:
                    have.append(s)
                tries -= 1
        return have[:n]

    def close(self):
        if self.handle:
            self.lib.vse_destroy(self.handle)
            self.handle = C.c_void_p()

    # ---- stand-alone stages ---------------------------------------------------------------------------
    def det_preprocess(self, frames_u8, dst_h, dst_w, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), raw=False):
        """frames_u8: cuda uint8 [N,H,W,3] (contiguous or row-pitched view) -> fp16 [N,dst_h,dst_w,8].
        raw=True: resized uint8 values + a ones channel for a net built with input_norm (see vse_det_preprocess)."""
        t = self.torch
        assert frames_u8.dtype == t.uint8 and frames_u8.dim() == 4 and frames_u8.shape[3] == 3
        assert frames_u8.stride(3) == 1 and frames_u8.stride(2) == 3
        n, h, w, _ = frames_u8.shape
        out = t.empty((n, dst_h, dst_w, 8), dtype=t.float16, device=self.tdev)
        m = None if raw else (C.c_float * 3)(*mean)
        s = None if raw else (C.c_float * 3)(*std)
        _check(self.lib.vse_det_preprocess(self.handle, C.c_void_p(frames_u8.data_ptr()), n, h, w,
                                           frames_u8.stride(1), frames_u8.stride(0), C.c_void_p(out.data_ptr()),
                                           dst_h, dst_w, m, s, self.stream()), "vse_det_preprocess")
        return out

    def db_postprocess(self, prob, src_h, src_w, thresh=0.3, box_thresh=0.6, unclip_ratio=1.5, max_candidates=1000,
                       min_size=3, max_boxes=None):
        """prob: cuda fp32 [N,H,W] -> list (per frame) of (ndarray[k,4,2] float32, ndarray[k] float32)."""
        t = self.torch
        assert prob.dtype == t.float32 and prob.is_contiguous()
        n, h, w = prob.shape
        nbytes = self.lib.vse_db_workspace_bytes(n, h, w)
        if getattr(self, "_db_ws", None) is None or self._db_ws.numel() < nbytes:
            self._db_ws = t.empty(nbytes, dtype=t.uint8, device=self.tdev)
        max_boxes = max_boxes or n * 1024
        if getattr(self, "_db_boxes_cap", 0) < max_boxes:           # reused across calls (2.6 MB for 64 frames; only nb.value
            self._db_boxes = (Box * max_boxes)()                    # records are read back, and they are copied below)
            self._db_boxes_cap = max_boxes
        boxes = self._db_boxes
        nb = C.c_int(0)
        prm = DbParams(box_thresh, unclip_ratio, thresh, max_candidates, min_size)
        _check(self.lib.vse_db_postprocess(self.handle, C.c_void_p(prob.data_ptr()), n, h, w, src_h, src_w,
                                           C.byref(prm), C.c_void_p(self._db_ws.data_ptr()), nbytes, boxes,
                                           max_boxes, C.byref(nb), self.stream()), "vse_db_postprocess")
        arr = np.frombuffer(boxes, dtype=np.dtype([("pts", "<f4", (4, 2)), ("score", "<f4"), ("frame", "<i4")]),
                            count=nb.value)
        # records come grouped by frame in ascending order: split by counts instead of 64 boolean masks
        out = []
        if nb.value and np.all(np.diff(arr["frame"]) >= 0):
            cnt = np.bincount(arr["frame"], minlength=n)
            end = np.cumsum(cnt)
            pts, sc = arr["pts"].copy(), arr["score"].copy()
            for f in range(n):
                out.append((pts[end[f] - cnt[f]:end[f]], sc[end[f] - cnt[f]:end[f]]))
        else:
            for f in range(n):
                sel = arr[arr["frame"] == f]
                out.append((sel["pts"].copy(), sel["score"].copy()))
        return out

    def rec_preprocess(self, frames_u8, crops, rec_h, rec_w, out=None):
        """crops: list of dict(quad[4][2], frame, crop_w, crop_h, resized_w, rotate) -> fp16 [n,rec_h,rec_w,8].
        out: write into this contiguous fp16 [n,rec_h,rec_w,8] tensor (rows of a larger batch whose other rows are cut from
        another frame tensor) instead of allocating one."""
        t = self.torch
        n = len(crops)
        # the vse_crop records are filled through a numpy view of the ctypes array (same bytes, no per-field Python loop:
        # this sits on the GPU-idle path between the detector's boxes and the first recogniser launch)
        arr = (Crop * n)()
        rec = np.frombuffer(arr, dtype=CROP_DT, count=n)
        rec["quad"] = np.asarray([c["quad"] for c in crops], dtype=np.float32).reshape(n, 4, 2)
        for name in ("frame", "crop_w", "crop_h", "resized_w", "rotate"):
            rec[name] = [c[name] for c in crops]
        mw = max(1, int(rec["crop_w"].max())) if n else 1
        mh = max(1, int(rec["crop_h"].max())) if n else 1
        nbytes = self.lib.vse_rec_preprocess_scratch_bytes(n, mw, mh)
        crop_ws = t.empty(nbytes, dtype=t.uint8, device=self.tdev)     # per call: groups may run on different streams
        if out is None:
            out = t.empty((n, rec_h, rec_w, 8), dtype=t.float16, device=self.tdev)
        assert out.dtype == t.float16 and out.is_contiguous() and tuple(out.shape) == (n, rec_h, rec_w, 8)
        nf, h, w, _ = frames_u8.shape
        _check(self.lib.vse_rec_preprocess(self.handle, C.c_void_p(frames_u8.data_ptr()), nf, h, w,
                                           frames_u8.stride(1), frames_u8.stride(0), arr, n,
                                           C.c_void_p(out.data_ptr()), rec_h, rec_w,
                                           C.c_void_p(crop_ws.data_ptr()), nbytes, self.stream()),
               "vse_rec_preprocess")
        return out

    def ctc_collapse(self, idx_maxp, tlen=None):
        """idx_maxp: cuda [B,1,T,2] (int32 idx / fp32 prob bit-pairs, as float32 tensor) ->
        (idx int32 [B,T], len int32 [B], conf fp32 [B]) cuda tensors.  tlen: cuda int32 [B] sequence lengths of a ragged batch."""
        t = self.torch
        b, tt = idx_maxp.shape[0], idx_maxp.shape[2]
        oi = t.zeros((b, tt), dtype=t.int32, device=self.tdev)
        ol = t.empty((b,), dtype=t.int32, device=self.tdev)
        oc = t.empty((b,), dtype=t.float32, device=self.tdev)
        if tlen is not None:
            assert tlen.dtype == t.int32 and tlen.is_contiguous() and tlen.numel() == b
        _check(self.lib.vse_ctc_collapse_ragged(self.handle, C.c_void_p(idx_maxp.data_ptr()), b, tt,
                                                C.c_void_p(tlen.data_ptr()) if tlen is not None else None,
                                                C.c_void_p(oi.data_ptr()), C.c_void_p(ol.data_ptr()),
                                                C.c_void_p(oc.data_ptr()), self.stream()), "vse_ctc_collapse")
        return oi, ol, oc

    def _upload_i32(self, tab):
        """Stream-ordered upload of a small int32 host table through a ring of pinned buffers, as Net._upload_i32 does for the width
        tables (a pageable copy would stall the host behind the recogniser launches queued on the stream)."""
        t = self.torch
        ring = self.__dict__.setdefault("_pin_ring", {"slots": [None] * 8, "next": 0})
        i = ring["next"] % len(ring["slots"])
        ring["next"] += 1
        slot = ring["slots"][i]
        if slot is not None:
            slot[1].synchronize()             # the copy that last read this slot (8 uploads ago) has long finished
        if slot is None or slot[0].numel() < tab.size:
            slot = ring["slots"][i] = (t.empty(max(int(tab.size), 1024), dtype=t.int32).pin_memory(), t.cuda.Event())
        pin = slot[0][:tab.size]
        pin.numpy()[...] = tab
        dev = t.empty(tab.shape, dtype=t.int32, device=self.tdev)
        dev.copy_(pin, non_blocking=True)
        slot[1].record(t.cuda.current_stream(self.tdev))
        return dev

    CTC_FUSE_MAX = 64         # member rows per group of ctc_fuse (include/vse_hip.h vse_ctc_fuse)

    def ctc_fuse(self, probs, group, tlen=None):
        """probs: cuda float32 [B,1,T,ncls], the probability output of a recogniser net built with want_probs=True (its last dimension
        may be a view with a larger stride); group: host sequence of g + 1 row offsets, strictly ascending inside 0 .. B, group j =
        rows group[j] .. group[j + 1] - 1, at most 64 of them; tlen: cuda int32 [g] sequence length per group (None: T) ->
        idx_maxp cuda float32 [g,1,T,2] as ctc_collapse takes it: per step the arg-max and the value of the members' mean probabilities
        (include/vse_hip.h vse_ctc_fuse).  The table is uploaded on the current stream."""
        t = self.torch
        assert probs.dtype == t.float32 and probs.dim() == 4 and probs.shape[1] == 1 and probs.stride(3) == 1, (probs.dtype, tuple(probs.shape))
        b, _, tt, ncls = probs.shape
        stride = probs.stride(2) if tt > 1 else max(probs.stride(2), ncls)
        assert b < 2 or probs.stride(0) == tt * stride, "the (row, step) rows of probs must be evenly spaced"
        tab = np.asarray(group, dtype=np.int64).reshape(-1)
        g = tab.size - 1
        if g < 1 or tab[0] < 0 or tab[-1] > b or np.any(np.diff(tab) < 1) or np.any(np.diff(tab) > self.CTC_FUSE_MAX):
            raise VseError(f"ctc_fuse: group offsets {tab.tolist()} must ascend strictly inside 0 .. {b} in steps of at most {self.CTC_FUSE_MAX}")
        if tlen is not None:
            assert tlen.dtype == t.int32 and tlen.is_contiguous() and tlen.numel() == g
        dev = self._upload_i32(tab.astype(np.int32))
        out = t.empty((g, 1, tt, 2), dtype=t.float32, device=self.tdev)
        _check(self.lib.vse_ctc_fuse(self.handle, C.c_void_p(probs.data_ptr()), b, tt, ncls, stride, C.c_void_p(dev.data_ptr()), g,
                                     C.c_void_p(tlen.data_ptr()) if tlen is not None else None, C.c_void_p(out.data_ptr()), self.stream()),
               "vse_ctc_fuse")
        return out

    # ---- subtitle-change frame selector -------------------------------------------------------------------------
    def frame_change_state(self, area_h, area_w):
        """A fresh (zero-filled) state for frame_change over an area of area_h x area_w pixels."""
        nbytes = self.lib.vse_frame_change_state_bytes(area_h, area_w)
        if not nbytes:
            raise VseError(f"frame_change: an area of {area_h} x {area_w} pixels has no interior")
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.tdev)

    def frame_change(self, frames_u8, area, edge_thresh, state, reset=False):
        """frames_u8: cuda uint8 [n,H,W,3] (any row pitch / frame stride, pixels packed), area = (y0, y1, x0, x1) in its pixels,
        state: frame_change_state of the area's size (carries the last frame's edge mask to the next call) ->
        cuda int32 [n,3]: edges, appeared, vanished per frame (include/vse_hip.h vse_frame_change)."""
        t = self.torch
        frames = self._frames_args(frames_u8)
        y0, y1, x0, x1 = (int(v) for v in area)
        assert state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= self.lib.vse_frame_change_state_bytes(y1 - y0, x1 - x0)
        out = t.empty((frames[1], 3), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_frame_change(self.handle, *frames, y0, y1, x0, x1, int(edge_thresh), C.c_void_p(state.data_ptr()),
                                         int(bool(reset)), C.c_void_p(out.data_ptr()), self.stream()), "vse_frame_change")
        return out

    def frame_focus(self, frames_u8, area, edge_thresh, state, reset=False):
        """frames_u8, area and state as for frame_change (the state is frame_change_state's and may pass between the two calls) ->
        cuda int32 [n,2]: kept, focus per frame: the edge pixels that were edge pixels one frame earlier, and the sum of their
        gradients (include/vse_hip.h vse_frame_focus)."""
        t = self.torch
        frames = self._frames_args(frames_u8)
        y0, y1, x0, x1 = (int(v) for v in area)
        assert state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= self.lib.vse_frame_change_state_bytes(y1 - y0, x1 - x0)
        out = t.empty((frames[1], 2), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_frame_focus(self.handle, *frames, y0, y1, x0, x1, int(edge_thresh), C.c_void_p(state.data_ptr()),
                                        int(bool(reset)), C.c_void_p(out.data_ptr()), self.stream()), "vse_frame_focus")
        return out

    def colour_key(self, frames_u8, area, key, out=None):
        """frames_u8 and area as for frame_change (an area of 1 x 1 is allowed); key: .bgr = (B, G, R) and .slope (frame_select.ColourKey)
        -> cuda uint8 of the input's shape (`out`, or a new tensor; pixels packed, any row pitch / frame stride): inside the area, and
        where the call widens its columns, every pixel is (K, K, K), K = max(0, 255 - ((max |channel - key| * slope) >> 8)); the other
        bytes are not written (include/vse_hip.h vse_colour_key).  The frames are only read."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        y0, y1, x0, x1 = (int(v) for v in area)
        if out is None:
            out = t.empty(tuple(frames_u8.shape), dtype=t.uint8, device=self.tdev)
        assert out.dtype == t.uint8 and tuple(out.shape) == tuple(frames_u8.shape) and out.is_cuda, (out.dtype, tuple(out.shape))
        dst = self._frames_args(out, allow_empty=True)
        b, g, r = (int(v) for v in key.bgr)
        _check(self.lib.vse_colour_key(self.handle, *frames, y0, y1, x0, x1, b, g, r, int(key.slope), dst[0], dst[4], dst[5], self.stream()),
               "vse_colour_key")
        return out

    # ---- subtitle-area locator ------------------------------------------------------------------------------------
    def frame_cells_dims(self, area_h, area_w):
        """(gy, gx): the cells of a region of area_h x area_w pixels (8 x 64 interior pixels each)."""
        gy, gx = C.c_int(), C.c_int()
        if self.lib.vse_frame_cells_dims(int(area_h), int(area_w), C.byref(gy), C.byref(gx)) != 0:
            raise VseError(f"frame_cells: a region of {area_h} x {area_w} pixels has no interior")
        return gy.value, gx.value

    def frame_cells_state(self, area_h, area_w):
        """A fresh CellsState (zero-filled) for frame_cells over a region of area_h x area_w pixels."""
        gy, gx = self.frame_cells_dims(area_h, area_w)
        t = self.torch
        return CellsState(t.zeros(self.lib.vse_frame_cells_state_bytes(int(area_h), int(area_w)), dtype=t.uint8, device=self.tdev),
                          t.zeros((gy, gx, 4), dtype=t.int32, device=self.tdev))

    def frame_cells(self, frames_u8, area, params, state, reset=False, flush=False, want_counts=False):
        """frames_u8: cuda uint8 [n,H,W,3] (any row pitch / frame stride, pixels packed; n may be 0, for a flush alone),
        area = (y0, y1, x0, x1) in its pixels, params: CellParams, state: frame_cells_state of the area's size -> state.totals, the
        cuda int32 [gy,gx,4] covered / runs / present / cuts per cell accumulated since the last reset (include/vse_hip.h
        vse_frame_cells); with want_counts (totals, cuda int32 [n,gy,gx,3] edges / appeared / vanished per frame and cell)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        assert state.words.numel() >= self.lib.vse_frame_cells_state_bytes(y1 - y0, x1 - x0) and tuple(state.totals.shape) == (gy, gx, 4)
        counts = t.empty((n, gy, gx, 3), dtype=t.int32, device=self.tdev) if want_counts else None
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells(self.handle, *frames, y0, y1, x0, x1, p.edge_thresh, p.min_edges, p.ratio_num, p.ratio_den,
                                        p.min_frames, p.max_frames, C.c_void_p(state.words.data_ptr()), int(bool(reset)),
                                        int(bool(flush)), C.c_void_p(state.totals.data_ptr()),
                                        C.c_void_p(counts.data_ptr()) if want_counts and n else None, self.stream()), "vse_frame_cells")
        return (state.totals, counts) if want_counts else state.totals

    # ---- edge-threshold calibration -------------------------------------------------------------------------------
    def frame_cells_multi_state(self, area_h, area_w, nt):
        """A fresh CellsState (zero-filled) for frame_cells_multi over a region of area_h x area_w pixels with nt thresholds; its
        totals are cuda int32 [nt,gy,gx,4]."""
        gy, gx = self.frame_cells_dims(area_h, area_w)
        nbytes = self.lib.vse_frame_cells_multi_state_bytes(int(area_h), int(area_w), int(nt))
        if not nbytes:
            raise VseError(f"frame_cells_multi: {nt} thresholds (1..8)")
        t = self.torch
        return CellsState(t.zeros(nbytes, dtype=t.uint8, device=self.tdev), t.zeros((int(nt), gy, gx, 4), dtype=t.int32, device=self.tdev))

    def frame_cells_multi(self, frames_u8, area, thresholds, params, state, reset=False, flush=False):
        """frame_cells for every edge threshold of `thresholds` (1..8 of them, ascending, each 1..255) in one pass over the frames:
        frames_u8, area, reset and flush as there, params: CellParams whose edge_thresh is ignored, state: frame_cells_multi_state of
        the area's size and len(thresholds) -> state.totals, cuda int32 [nt,gy,gx,4], slice k being frame_cells' totals at
        thresholds[k] (include/vse_hip.h vse_frame_cells_multi)."""
        frames = self._frames_args(frames_u8, allow_empty=True)
        y0, y1, x0, x1 = (int(v) for v in area)
        th = [int(v) for v in thresholds]
        nt = len(th)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        nbytes = self.lib.vse_frame_cells_multi_state_bytes(y1 - y0, x1 - x0, nt)
        assert nbytes and state.words.numel() >= nbytes and tuple(state.totals.shape) == (nt, gy, gx, 4)
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells_multi(self.handle, *frames, y0, y1, x0, x1, (C.c_int * nt)(*th), nt, p.min_edges, p.ratio_num,
                                              p.ratio_den, p.min_frames, p.max_frames, C.c_void_p(state.words.data_ptr()),
                                              int(bool(reset)), int(bool(flush)), C.c_void_p(state.totals.data_ptr()), self.stream()),
               "vse_frame_cells_multi")
        return state.totals

    def frame_cells_counts(self, frames_u8, area, thresholds, params, state, reset=False, flush=False):
        """frame_cells_multi that also counts for the selector: every argument as there, and the state is that call's
        (frame_cells_multi_state; it may pass between the two) -> (state.totals, cuda int32 [n,nt,3]): row [f][q] is frame_change's
        edges / appeared / vanished of frame f on the same area at edge_thresh = thresholds[q] (include/vse_hip.h
        vse_frame_cells_counts)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        th = [int(v) for v in thresholds]
        nt = len(th)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        nbytes = self.lib.vse_frame_cells_multi_state_bytes(y1 - y0, x1 - x0, nt)
        assert nbytes and state.words.numel() >= nbytes and tuple(state.totals.shape) == (nt, gy, gx, 4)
        counts = t.empty((n, nt, 3), dtype=t.int32, device=self.tdev)
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells_counts(self.handle, *frames, y0, y1, x0, x1, (C.c_int * nt)(*th), nt, p.min_edges, p.ratio_num,
                                               p.ratio_den, p.min_frames, p.max_frames, C.c_void_p(state.words.data_ptr()),
                                               int(bool(reset)), int(bool(flush)), C.c_void_p(state.totals.data_ptr()),
                                               C.c_void_p(counts.data_ptr()) if n else None, self.stream()), "vse_frame_cells_counts")
        return state.totals, counts

    def frame_cells_export_state(self, state, area_h, area_w, q, out=None):
        """Slice q of a frame_cells_multi_state of an area_h x area_w region -> a frame_change state of the same area (`out`, or a new
        one) holding that threshold's last mask, so that frame_change / frame_focus at thresholds[q] continue the clip (include/vse_hip.h
        vse_frame_cells_export_state)."""
        t = self.torch
        nt = int(state.totals.shape[0])
        nbytes = self.lib.vse_frame_change_state_bytes(int(area_h), int(area_w))
        if out is None and nbytes:
            out = t.zeros(nbytes, dtype=t.uint8, device=self.tdev)
        assert out is None or (out.dtype == t.uint8 and out.is_contiguous() and out.numel() >= nbytes)
        assert state.words.numel() >= self.lib.vse_frame_cells_multi_state_bytes(int(area_h), int(area_w), nt)
        _check(self.lib.vse_frame_cells_export_state(self.handle, C.c_void_p(state.words.data_ptr()), int(area_h), int(area_w), nt, int(q),
                                                     C.c_void_p(out.data_ptr()) if out is not None else None, self.stream()),
               "vse_frame_cells_export_state")
        return out

    # ---- the locator's masks, kept for a rectangle decided later ------------------------------------------------------
    def frame_masks_buffer(self, area_h, area_w, nt, cap):
        """A MasksBuffer of `cap` frame slots for frame_cells_masks over a region of area_h x area_w pixels with nt thresholds.  It is
        not cleared: frame_cells_masks writes every word of the slots it fills, and frame_masks_replay reads only filled slots."""
        nbytes = self.lib.vse_frame_masks_bytes(int(area_h), int(area_w), int(nt), int(cap))
        if not nbytes:
            raise VseError(f"frame_masks_buffer: a region of {area_h} x {area_w} pixels, {nt} thresholds (1..8), {cap} slots (at least 1)")
        return MasksBuffer(self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.tdev), area_h, area_w, nt, cap)

    def frame_cells_masks(self, frames_u8, area, thresholds, params, state, masks, slot0, reset=False, flush=False):
        """frame_cells_multi that also keeps the masks: every argument as there, and the state is that call's (frame_cells_multi_state;
        it may pass between the two); masks: frame_masks_buffer of the area's size and len(thresholds), whose slots slot0 .. slot0 + n - 1
        take the n frames -> state.totals (include/vse_hip.h vse_frame_cells_masks)."""
        frames = self._frames_args(frames_u8, allow_empty=True)
        y0, y1, x0, x1 = (int(v) for v in area)
        th = [int(v) for v in thresholds]
        nt = len(th)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        nbytes = self.lib.vse_frame_cells_multi_state_bytes(y1 - y0, x1 - x0, nt)
        assert nbytes and state.words.numel() >= nbytes and tuple(state.totals.shape) == (nt, gy, gx, 4)
        assert (masks.area_h, masks.area_w, masks.nt) == (y1 - y0, x1 - x0, nt)
        assert masks.words.numel() >= self.lib.vse_frame_masks_bytes(masks.area_h, masks.area_w, nt, masks.cap)
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells_masks(self.handle, *frames, y0, y1, x0, x1, (C.c_int * nt)(*th), nt, p.min_edges, p.ratio_num,
                                              p.ratio_den, p.min_frames, p.max_frames, C.c_void_p(state.words.data_ptr()),
                                              int(bool(reset)), int(bool(flush)), C.c_void_p(state.totals.data_ptr()),
                                              C.c_void_p(masks.words.data_ptr()), masks.cap, int(slot0), self.stream()),
               "vse_frame_cells_masks")
        return state.totals

    def frame_masks_replay(self, masks, q, f0, f1, rect, reset=True, out=None):
        """Slots [f0, f1) of a MasksBuffer at threshold index q, counted on rect = (ry0, ry1, rx0, rx1) in the region's pixels ->
        (cuda int32 [f1 - f0, 3], change_state): frame_change's edges / appeared / vanished of those frames on that rectangle, and a
        frame_change state of the rectangle (`out`, or a new one) holding slot f1 - 1's mask, so that frame_change / frame_focus
        continue the clip.  reset: nothing precedes slot f0; else slot f0 - 1 does (include/vse_hip.h vse_frame_masks_replay)."""
        t = self.torch
        ry0, ry1, rx0, rx1 = (int(v) for v in rect)
        nbytes = self.lib.vse_frame_change_state_bytes(ry1 - ry0, rx1 - rx0)
        if out is None and nbytes:
            out = t.zeros(nbytes, dtype=t.uint8, device=self.tdev)
        assert out is None or (out.dtype == t.uint8 and out.is_contiguous() and out.numel() >= nbytes)
        assert masks.words.numel() >= self.lib.vse_frame_masks_bytes(masks.area_h, masks.area_w, masks.nt, masks.cap)
        counts = t.empty((max(0, int(f1) - int(f0)), 3), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_frame_masks_replay(self.handle, C.c_void_p(masks.words.data_ptr()), masks.area_h, masks.area_w, masks.nt,
                                               masks.cap, int(q), int(f0), int(f1), ry0, ry1, rx0, rx1, int(bool(reset)),
                                               C.c_void_p(counts.data_ptr()) if counts.numel() else None,
                                               C.c_void_p(out.data_ptr()) if out is not None else None, self.stream()),
               "vse_frame_masks_replay")
        return counts, out

    # ---- held-edge frame selector ---------------------------------------------------------------------------------
    def frame_hold_state(self, area_h, area_w, hold):
        """A fresh (zero-filled) state for frame_hold over an area of area_h x area_w pixels with this `hold`."""
        nbytes = self.lib.vse_frame_hold_state_bytes(int(area_h), int(area_w), int(hold))
        if not nbytes:
            raise VseError(f"frame_hold: an area of {area_h} x {area_w} pixels has no interior, or hold {hold} is outside 1..32")
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.tdev)

    def frame_hold(self, frames_u8, area, edge_thresh, hold, state, fed, flush=False):
        """frames_u8: cuda uint8 [n,H,W,3] (any row pitch / frame stride, pixels packed; n may be 0, for a flush alone), the next
        frames of a clip of which `fed` went to earlier calls (0 starts a clip), area = (y0, y1, x0, x1) in its pixels, state:
        frame_hold_state of the area's size and `hold` -> cuda int32 [rows,3]: held edges, appeared, vanished of the frames whose
        held mask this call completes, which trail the frames fed by hold - 1 until `flush` (include/vse_hip.h vse_frame_hold)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        hold, fed = int(hold), int(fed)
        nbytes = self.lib.vse_frame_hold_state_bytes(y1 - y0, x1 - x0, hold)
        assert nbytes and state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= nbytes
        rows = (fed + n if flush else max(0, fed + n - hold + 1)) - max(0, fed - hold + 1)
        out = t.empty((n + hold - 1, 3), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_frame_hold(self.handle, *frames, y0, y1, x0, x1, int(edge_thresh), hold, C.c_void_p(state.data_ptr()),
                                       fed, int(bool(flush)), C.c_void_p(out.data_ptr()), self.stream()), "vse_frame_hold")
        return out[:rows]

    # ---- held-edge frame selector with bounded runs -----------------------------------------------------------------
    def frame_hold_bounded_state(self, area_h, area_w, max_hold):
        """A fresh (zero-filled) state for frame_hold_bounded over an area of area_h x area_w pixels with this `max_hold`."""
        nbytes = self.lib.vse_frame_hold_bounded_state_bytes(int(area_h), int(area_w), int(max_hold))
        if not nbytes:
            raise VseError(f"frame_hold_bounded: an area of {area_h} x {area_w} pixels has no interior, or max_hold {max_hold} is "
                           f"outside 1..{FRAME_HOLD_BOUNDED_MAX}")
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.tdev)

    def frame_hold_bounded(self, frames_u8, area, edge_thresh, hold, max_hold, state, fed, flush=False):
        """frame_hold counting only the edge pixels whose run is hold .. max_hold frames long: frames_u8, area, hold, fed and flush as
        there, state: frame_hold_bounded_state of the area's size and `max_hold` -> cuda int32 [rows,3]: bounded edges, appeared,
        vanished of the frames whose row this call completes, which trail the frames fed by max_hold until `flush` (include/vse_hip.h
        vse_frame_hold_bounded)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        hold, max_hold, fed = int(hold), int(max_hold), int(fed)
        nbytes = self.lib.vse_frame_hold_bounded_state_bytes(y1 - y0, x1 - x0, max_hold)
        assert nbytes and state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= nbytes
        rows = (fed + n if flush else max(0, fed + n - max_hold)) - max(0, fed - max_hold)
        out = t.empty((n + max_hold, 3), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_frame_hold_bounded(self.handle, *frames, y0, y1, x0, x1, int(edge_thresh), hold, max_hold,
                                               C.c_void_p(state.data_ptr()), fed, int(bool(flush)), C.c_void_p(out.data_ptr()),
                                               self.stream()), "vse_frame_hold_bounded")
        return out[:rows]

    # ---- locator and calibration on held edges ---------------------------------------------------------------------
    def frame_cells_hold_state(self, area_h, area_w, nt, hold):
        """A fresh CellsState (zero-filled) for frame_cells_hold over a region of area_h x area_w pixels with nt thresholds and this
        `hold`; its totals are cuda int32 [nt,gy,gx,4]."""
        gy, gx = self.frame_cells_dims(area_h, area_w)
        nbytes = self.lib.vse_frame_cells_hold_state_bytes(int(area_h), int(area_w), int(nt), int(hold))
        if not nbytes:
            raise VseError(f"frame_cells_hold: {nt} thresholds (1..8) or hold {hold} (1..32)")
        t = self.torch
        return CellsState(t.zeros(nbytes, dtype=t.uint8, device=self.tdev), t.zeros((int(nt), gy, gx, 4), dtype=t.int32, device=self.tdev))

    def frame_cells_hold(self, frames_u8, area, thresholds, hold, params, state, fed, flush=False, want_counts=False):
        """frame_cells_multi on the held masks of frame_hold: frames_u8, area, thresholds and params as there, `hold` and `fed` (the
        frames of this clip that went to earlier calls; 0 starts a clip) as for frame_hold, state: frame_cells_hold_state of the area's
        size, len(thresholds) and `hold` -> state.totals, cuda int32 [nt,gy,gx,4]: the frames whose held mask is complete, all of them
        after `flush` (include/vse_hip.h vse_frame_cells_hold); with want_counts (totals, cuda int32 [nt,rows,gy,gx,3] held edges /
        appeared / vanished per cell of the frames this call completes, frame_hold's rows cell by cell)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        th = [int(v) for v in thresholds]
        nt, hold, fed = len(th), int(hold), int(fed)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        nbytes = self.lib.vse_frame_cells_hold_state_bytes(y1 - y0, x1 - x0, nt, hold)
        assert nbytes and state.words.numel() >= nbytes and tuple(state.totals.shape) == (nt, gy, gx, 4)
        rows = (fed + n if flush else max(0, fed + n - hold + 1)) - max(0, fed - hold + 1)
        counts = t.empty((nt, n + hold - 1, gy, gx, 3), dtype=t.int32, device=self.tdev) if want_counts else None
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells_hold(self.handle, *frames, y0, y1, x0, x1, (C.c_int * nt)(*th), nt, hold, p.min_edges, p.ratio_num,
                                             p.ratio_den, p.min_frames, p.max_frames, C.c_void_p(state.words.data_ptr()), fed,
                                             int(bool(flush)), C.c_void_p(state.totals.data_ptr()),
                                             C.c_void_p(counts.data_ptr()) if want_counts and counts.numel() else None, self.stream()),
               "vse_frame_cells_hold")
        return (state.totals, counts[:, :rows]) if want_counts else state.totals

    # ---- the held locator's edge masks, kept for a rectangle decided later ---------------------------------------------
    def frame_cells_hold_masks(self, frames_u8, area, thresholds, hold, params, state, masks, slot0, fed, flush=False, want_counts=False):
        """frame_cells_hold that also keeps the EDGE masks: every argument as there, and the state is that call's
        (frame_cells_hold_state; it may pass between the two); masks: frame_masks_buffer of the area's size and len(thresholds), whose
        slots slot0 .. slot0 + n - 1 take the n frames exactly as frame_cells_masks fills them (a flush's steps take none) ->
        frame_cells_hold's result (include/vse_hip.h vse_frame_cells_hold_masks)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        th = [int(v) for v in thresholds]
        nt, hold, fed = len(th), int(hold), int(fed)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        nbytes = self.lib.vse_frame_cells_hold_state_bytes(y1 - y0, x1 - x0, nt, hold)
        assert nbytes and state.words.numel() >= nbytes and tuple(state.totals.shape) == (nt, gy, gx, 4)
        assert (masks.area_h, masks.area_w, masks.nt) == (y1 - y0, x1 - x0, nt)
        assert masks.words.numel() >= self.lib.vse_frame_masks_bytes(masks.area_h, masks.area_w, nt, masks.cap)
        rows = (fed + n if flush else max(0, fed + n - hold + 1)) - max(0, fed - hold + 1)
        counts = t.empty((nt, n + hold - 1, gy, gx, 3), dtype=t.int32, device=self.tdev) if want_counts else None
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells_hold_masks(self.handle, *frames, y0, y1, x0, x1, (C.c_int * nt)(*th), nt, hold, p.min_edges,
                                                   p.ratio_num, p.ratio_den, p.min_frames, p.max_frames, C.c_void_p(state.words.data_ptr()),
                                                   fed, int(bool(flush)), C.c_void_p(state.totals.data_ptr()),
                                                   C.c_void_p(counts.data_ptr()) if want_counts and counts.numel() else None,
                                                   C.c_void_p(masks.words.data_ptr()), masks.cap, int(slot0), self.stream()),
               "vse_frame_cells_hold_masks")
        return (state.totals, counts[:, :rows]) if want_counts else state.totals

    def frame_masks_replay_hold(self, masks, q, f0, f1, rect, hold, state, fed, flush=False):
        """Slots [f0, f1) of a MasksBuffer at threshold index q on rect = (ry0, ry1, rx0, rx1) in the region's pixels, as the next
        f1 - f0 frames of a clip of which `fed` went to earlier calls; state: frame_hold_state of the rectangle's size and `hold` ->
        cuda int32 [rows,3]: frame_hold's rows for those frames on that rectangle, and the state is left as frame_hold leaves it, so
        that frame_hold continues the clip (include/vse_hip.h vse_frame_masks_replay_hold)."""
        t = self.torch
        ry0, ry1, rx0, rx1 = (int(v) for v in rect)
        hold, fed, n = int(hold), int(fed), int(f1) - int(f0)
        nbytes = self.lib.vse_frame_hold_state_bytes(ry1 - ry0, rx1 - rx0, hold)
        assert nbytes and state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= nbytes
        assert masks.words.numel() >= self.lib.vse_frame_masks_bytes(masks.area_h, masks.area_w, masks.nt, masks.cap)
        rows = (fed + n if flush else max(0, fed + n - hold + 1)) - max(0, fed - hold + 1)
        out = t.empty((max(0, n) + hold - 1, 3), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_frame_masks_replay_hold(self.handle, C.c_void_p(masks.words.data_ptr()), masks.area_h, masks.area_w, masks.nt,
                                                    masks.cap, int(q), int(f0), int(f1), ry0, ry1, rx0, rx1, hold,
                                                    C.c_void_p(state.data_ptr()), fed, int(bool(flush)),
                                                    C.c_void_p(out.data_ptr()) if out.numel() else None, self.stream()),
               "vse_frame_masks_replay_hold")
        return out[:max(0, rows)]

    # ---- locator and calibration on bounded runs -------------------------------------------------------------------
    def frame_cells_hold_bounded_state(self, area_h, area_w, nt, max_hold):
        """A CellsState for frame_cells_hold_bounded over a region of area_h x area_w pixels with nt thresholds and this `max_hold`; its
        totals are cuda int32 [nt,gy,gx,4]."""
        gy, gx = self.frame_cells_dims(area_h, area_w)
        nbytes = self.lib.vse_frame_cells_hold_bounded_state_bytes(int(area_h), int(area_w), int(nt), int(max_hold))
        if not nbytes:
            raise VseError(f"frame_cells_hold_bounded: {nt} thresholds (1..8) or max_hold {max_hold} (1..{FRAME_HOLD_BOUNDED_MAX})")
        t = self.torch
        return CellsState(t.zeros(nbytes, dtype=t.uint8, device=self.tdev), t.zeros((int(nt), gy, gx, 4), dtype=t.int32, device=self.tdev))

    def frame_cells_hold_bounded(self, frames_u8, area, thresholds, hold, max_hold, params, state, fed, flush=False, want_counts=False):
        """frame_cells_hold on the bounded masks of frame_hold_bounded: frames_u8, area, thresholds, hold, params and fed as there,
        `max_hold` as for frame_hold_bounded, state: frame_cells_hold_bounded_state of the area's size, len(thresholds) and `max_hold`
        -> state.totals, cuda int32 [nt,gy,gx,4]: the frames whose row is final, which trail the frames fed by max_hold, all of them
        after `flush` (include/vse_hip.h vse_frame_cells_hold_bounded); with want_counts (totals, cuda int32 [nt,rows,gy,gx,3] bounded
        edges / appeared / vanished per cell of the frames this call completes, frame_hold_bounded's rows cell by cell)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        th = [int(v) for v in thresholds]
        nt, hold, max_hold, fed = len(th), int(hold), int(max_hold), int(fed)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        nbytes = self.lib.vse_frame_cells_hold_bounded_state_bytes(y1 - y0, x1 - x0, nt, max_hold)
        assert nbytes and state.words.numel() >= nbytes and tuple(state.totals.shape) == (nt, gy, gx, 4)
        rows = (fed + n if flush else max(0, fed + n - max_hold)) - max(0, fed - max_hold)
        counts = t.empty((nt, n + max_hold, gy, gx, 3), dtype=t.int32, device=self.tdev) if want_counts else None
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells_hold_bounded(self.handle, *frames, y0, y1, x0, x1, (C.c_int * nt)(*th), nt, hold, max_hold,
                                                     p.min_edges, p.ratio_num, p.ratio_den, p.min_frames, p.max_frames,
                                                     C.c_void_p(state.words.data_ptr()), fed, int(bool(flush)),
                                                     C.c_void_p(state.totals.data_ptr()),
                                                     C.c_void_p(counts.data_ptr()) if want_counts and counts.numel() else None,
                                                     self.stream()),
               "vse_frame_cells_hold_bounded")
        return (state.totals, counts[:, :rows]) if want_counts else state.totals

    # ---- the bounded locator's edge masks, kept for a rectangle decided later ------------------------------------------
    def frame_cells_hold_bounded_masks(self, frames_u8, area, thresholds, hold, max_hold, params, state, masks, slot0, fed, flush=False,
                                       want_counts=False):
        """frame_cells_hold_bounded that also keeps the EDGE masks: every argument as there, and the state is that call's
        (frame_cells_hold_bounded_state; it may pass between the two); masks: frame_masks_buffer of the area's size and len(thresholds),
        whose slots slot0 .. slot0 + n - 1 take the n frames exactly as frame_cells_masks fills them (the flush step takes none) ->
        frame_cells_hold_bounded's result (include/vse_hip.h vse_frame_cells_hold_bounded_masks)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        n = frames[1]
        y0, y1, x0, x1 = (int(v) for v in area)
        th = [int(v) for v in thresholds]
        nt, hold, max_hold, fed = len(th), int(hold), int(max_hold), int(fed)
        gy, gx = self.frame_cells_dims(y1 - y0, x1 - x0)
        nbytes = self.lib.vse_frame_cells_hold_bounded_state_bytes(y1 - y0, x1 - x0, nt, max_hold)
        assert nbytes and state.words.numel() >= nbytes and tuple(state.totals.shape) == (nt, gy, gx, 4)
        assert (masks.area_h, masks.area_w, masks.nt) == (y1 - y0, x1 - x0, nt)
        assert masks.words.numel() >= self.lib.vse_frame_masks_bytes(masks.area_h, masks.area_w, nt, masks.cap)
        rows = (fed + n if flush else max(0, fed + n - max_hold)) - max(0, fed - max_hold)
        counts = t.empty((nt, n + max_hold, gy, gx, 3), dtype=t.int32, device=self.tdev) if want_counts else None
        p = CellParams(*(int(v) for v in params))
        _check(self.lib.vse_frame_cells_hold_bounded_masks(self.handle, *frames, y0, y1, x0, x1, (C.c_int * nt)(*th), nt, hold, max_hold,
                                                           p.min_edges, p.ratio_num, p.ratio_den, p.min_frames, p.max_frames,
                                                           C.c_void_p(state.words.data_ptr()), fed, int(bool(flush)),
                                                           C.c_void_p(state.totals.data_ptr()),
                                                           C.c_void_p(counts.data_ptr()) if want_counts and counts.numel() else None,
                                                           C.c_void_p(masks.words.data_ptr()), masks.cap, int(slot0), self.stream()),
               "vse_frame_cells_hold_bounded_masks")
        return (state.totals, counts[:, :rows]) if want_counts else state.totals

    def frame_masks_replay_hold_bounded(self, masks, q, f0, f1, rect, hold, max_hold, state, fed, flush=False):
        """Slots [f0, f1) of a MasksBuffer at threshold index q on rect = (ry0, ry1, rx0, rx1) in the region's pixels, as the next
        f1 - f0 frames of a clip of which `fed` went to earlier calls; state: frame_hold_bounded_state of the rectangle's size and
        `max_hold` -> cuda int32 [rows,3]: frame_hold_bounded's rows for those frames on that rectangle, and the state is left as
        frame_hold_bounded leaves it, so that frame_hold_bounded continues the clip (include/vse_hip.h
        vse_frame_masks_replay_hold_bounded)."""
        t = self.torch
        ry0, ry1, rx0, rx1 = (int(v) for v in rect)
        hold, max_hold, fed, n = int(hold), int(max_hold), int(fed), int(f1) - int(f0)
        nbytes = self.lib.vse_frame_hold_bounded_state_bytes(ry1 - ry0, rx1 - rx0, max_hold)
        assert nbytes and state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= nbytes
        assert masks.words.numel() >= self.lib.vse_frame_masks_bytes(masks.area_h, masks.area_w, masks.nt, masks.cap)
        rows = (fed + n if flush else max(0, fed + n - max_hold)) - max(0, fed - max_hold)
        out = t.empty((max(0, n) + max_hold, 3), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_frame_masks_replay_hold_bounded(self.handle, C.c_void_p(masks.words.data_ptr()), masks.area_h, masks.area_w,
                                                            masks.nt, masks.cap, int(q), int(f0), int(f1), ry0, ry1, rx0, rx1, hold,
                                                            max_hold, C.c_void_p(state.data_ptr()), fed, int(bool(flush)),
                                                            C.c_void_p(out.data_ptr()), self.stream()),
               "vse_frame_masks_replay_hold_bounded")
        return out[:max(0, rows)]

    # ---- interval composite ---------------------------------------------------------------------------------------
    def interval_state(self, area_h, area_w):
        """A state for interval_accumulate over an area of area_h x area_w pixels (its first call passes reset=True)."""
        nbytes = self.lib.vse_interval_state_bytes(int(area_h), int(area_w))
        if not nbytes:
            raise VseError(f"interval_accumulate: an area of {area_h} x {area_w} pixels is empty")
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.tdev)

    def interval_accumulate(self, frames_u8, area, state, reset=False):
        """frames_u8: cuda uint8 [n,H,W,3] (any row pitch / frame stride, pixels packed), area = (y0, y1, x0, x1) in its pixels,
        state: interval_state of the area's size -> state, now holding the per-byte min, max and sum of the area over the frames
        since the last reset (include/vse_hip.h vse_interval_accumulate)."""
        t = self.torch
        frames = self._frames_args(frames_u8)
        y0, y1, x0, x1 = (int(v) for v in area)
        assert state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= max(self.lib.vse_interval_state_bytes(y1 - y0, x1 - x0), 1)
        _check(self.lib.vse_interval_accumulate(self.handle, *frames, y0, y1, x0, x1, C.c_void_p(state.data_ptr()), int(bool(reset)),
                                                self.stream()), "vse_interval_accumulate")
        return state

    def interval_composite(self, state, area_h, area_w, frames, mode, out=None):
        """state: what interval_accumulate left for an area of area_h x area_w pixels, frames: how many it accumulated since the last
        reset, mode: "min" | "max" | "mean" -> cuda uint8 [area_h, area_w, 3] (include/vse_hip.h vse_interval_composite).  out: write
        into this tensor instead (it may be a strided view with packed pixels; its row pitch is taken from it)."""
        t = self.torch
        area_h, area_w = int(area_h), int(area_w)
        if mode not in INTERVAL_MODES:
            raise VseError(f"interval_composite: mode {mode!r} is not one of {sorted(INTERVAL_MODES)}")
        assert state.dtype == t.uint8 and state.is_contiguous() and state.numel() >= max(self.lib.vse_interval_state_bytes(area_h, area_w), 1)
        if out is None:
            out = t.empty((max(area_h, 0), max(area_w, 0), 3), dtype=t.uint8, device=self.tdev)
        assert out.dtype == t.uint8 and tuple(out.shape) == (area_h, area_w, 3) and out.stride(2) == 1 and out.stride(1) == 3
        _check(self.lib.vse_interval_composite(self.handle, C.c_void_p(state.data_ptr()), area_h, area_w, int(frames), INTERVAL_MODES[mode],
                                               C.c_void_p(out.data_ptr()), out.stride(0) if area_h > 1 else max(out.stride(0), 3 * area_w),
                                               self.stream()), "vse_interval_composite")
        return out

    def interval_rank(self, frames_u8, area, rank, out=None):
        """frames_u8: cuda uint8 [n,H,W,3], 1 <= n <= INTERVAL_RANK_MAX (any row pitch / frame stride, pixels packed), area = (y0, y1,
        x0, x1) in its pixels, 0 <= rank < n -> cuda uint8 [y1-y0, x1-x0, 3]: per byte, element `rank` of the n frames' values sorted
        ascending (include/vse_hip.h vse_interval_rank; rank 0 the minimum, n - 1 the maximum).  out: write into this tensor instead
        (it may be a strided view with packed pixels; its row pitch is taken from it)."""
        t = self.torch
        frames = self._frames_args(frames_u8)
        y0, y1, x0, x1 = (int(v) for v in area)
        area_h, area_w = y1 - y0, x1 - x0
        if out is None:
            out = t.empty((max(area_h, 0), max(area_w, 0), 3), dtype=t.uint8, device=self.tdev)
        assert out.dtype == t.uint8 and tuple(out.shape) == (area_h, area_w, 3) and out.stride(2) == 1 and out.stride(1) == 3
        _check(self.lib.vse_interval_rank(self.handle, *frames, y0, y1, x0, x1, int(rank), C.c_void_p(out.data_ptr()),
                                          out.stride(0) if area_h > 1 else max(out.stride(0), 3 * area_w), self.stream()),
               "vse_interval_rank")
        return out

    def interval_stream_state(self, area_h, area_w, cap):
        """A state for interval_stream over an area of area_h x area_w pixels with a ring of `cap` frames."""
        nbytes = self.lib.vse_interval_stream_state_bytes(int(area_h), int(area_w), int(cap))
        if not nbytes:
            raise VseError(f"interval_stream: an area of {area_h} x {area_w} pixels is empty, or cap {cap} is below 1")
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.tdev)

    def interval_stream(self, frames_u8, area, state, cap, fed, segs, store_from, mode, out=None):
        """frames_u8: cuda uint8 [n,H,W,3], n >= 0: the frames fed + 1 .. fed + n of the clip (any row pitch / frame stride, pixels
        packed), area = (y0, y1, x0, x1) in its pixels, state: interval_stream_state of the area's size and `cap`, segs: up to
        INTERVAL_STREAM_MAX_SEGS of (first, last, flags, frames[, out]) with absolute 1-based frame numbers and flags of
        INTERVAL_SEG_CONTINUE | INTERVAL_SEG_EMIT (without `out`, the EMITs are numbered 0, 1, .. in order), store_from: the batch
        frames from this number on are parked in the ring, mode: "min" | "max" | "mean" -> cuda uint8 [patches, y1-y0, x1-x0, 3], one
        composite per EMIT (include/vse_hip.h vse_interval_stream).  out: write into this tensor instead (it may be a strided view
        with packed pixels; its row pitch and patch stride are taken from it)."""
        t = self.torch
        frames = self._frames_args(frames_u8, allow_empty=True)
        y0, y1, x0, x1 = (int(v) for v in area)
        area_h, area_w = y1 - y0, x1 - x0
        if mode not in INTERVAL_MODES:
            raise VseError(f"interval_stream: mode {mode!r} is not one of {sorted(INTERVAL_MODES)}")
        assert state.dtype == t.uint8 and state.is_contiguous()
        assert state.numel() >= max(self.lib.vse_interval_stream_state_bytes(area_h, area_w, int(cap)), 1)
        recs, emits = (IntervalSeg * max(len(segs), 1))(), 0
        for k, g in enumerate(segs):
            emit = bool(int(g[2]) & INTERVAL_SEG_EMIT)
            recs[k] = IntervalSeg(int(g[0]), int(g[1]), int(g[2]), int(g[3]), int(g[4]) if len(g) > 4 else (emits if emit else 0))
            emits = max(emits, recs[k].out + 1) if emit else emits
        if out is None:
            out = t.empty((emits, max(area_h, 0), max(area_w, 0), 3), dtype=t.uint8, device=self.tdev)
        assert out.dtype == t.uint8 and tuple(out.shape[1:]) == (area_h, area_w, 3) and out.shape[0] >= emits
        assert out.stride(3) == 1 and out.stride(2) == 3
        _check(self.lib.vse_interval_stream(self.handle, *frames, y0, y1, x0, x1, C.c_void_p(state.data_ptr()), int(cap), int(fed), recs,
                                            len(segs), int(store_from), INTERVAL_MODES[mode], C.c_void_p(out.data_ptr()) if emits else None,
                                            out.stride(1) if area_h > 1 else max(out.stride(1), 3 * area_w), out.stride(0), self.stream()),
               "vse_interval_stream")
        return out

    def interval_ring_rank(self, state, area_h, area_w, cap, fed, groups, out=None):
        """state: an interval_stream_state of area_h x area_w pixels and `cap`, into whose ring interval_stream has stored the frames
        up to `fed`; groups: up to INTERVAL_RING_MAX_GROUPS of (frame numbers, rank[, out]): 1 .. INTERVAL_RANK_MAX absolute 1-based
        frame numbers, strictly ascending, inside (fed - cap, fed], and 0 <= rank < their count (without `out`, group k writes patch
        k) -> cuda uint8 [patches, area_h, area_w, 3]: per byte, element `rank` of the named frames' values sorted ascending
        (include/vse_hip.h vse_interval_ring_rank).  The state is only read.  out: write into this tensor instead (it may be a
        strided view with packed pixels; its row pitch and patch stride are taken from it)."""
        t = self.torch
        area_h, area_w = int(area_h), int(area_w)
        assert state.dtype == t.uint8 and state.is_contiguous()
        assert state.numel() >= max(self.lib.vse_interval_stream_state_bytes(area_h, area_w, int(cap)), 1)
        if len(groups) > INTERVAL_RING_MAX_GROUPS:
            raise VseError(f"interval_ring_rank: {len(groups)} groups, at most {INTERVAL_RING_MAX_GROUPS} go in one call")
        recs, patches = (IntervalRingGroup * max(len(groups), 1))(), 0
        for k, g in enumerate(groups):
            nos = [int(v) for v in g[0]]
            if len(nos) > INTERVAL_RANK_MAX:
                raise VseError(f"interval_ring_rank: group {k} names {len(nos)} frames, at most {INTERVAL_RANK_MAX} are ranked")
            recs[k].n, recs[k].rank, recs[k].out = len(nos), int(g[1]), int(g[2]) if len(g) > 2 else k
            recs[k].frames[:len(nos)] = nos
            patches = max(patches, recs[k].out + 1)
        if out is None:
            out = t.empty((patches, max(area_h, 0), max(area_w, 0), 3), dtype=t.uint8, device=self.tdev)
            if not groups:
                return out                                # (no patch, no memory to name as d_out: nothing to ask the library for)
        assert out.dtype == t.uint8 and tuple(out.shape[1:]) == (area_h, area_w, 3) and out.shape[0] >= patches
        assert out.stride(3) == 1 and out.stride(2) == 3
        _check(self.lib.vse_interval_ring_rank(self.handle, C.c_void_p(state.data_ptr()), area_h, area_w, int(cap), int(fed), recs, len(groups),
                                               C.c_void_p(out.data_ptr()), out.stride(1) if area_h > 1 else max(out.stride(1), 3 * area_w),
                                               out.stride(0), self.stream()), "vse_interval_ring_rank")
        return out

    # ---- timeline sync: audio template search ---------------------------------------------------------------------
    def audio_match_workspace_bytes(self, queries):
        """Workspace bytes of one audio_match call with these (src_off, m, dst_off, win_len) queries (0 if one is invalid)."""
        q = _audio_queries(queries)
        return self.lib.vse_audio_match_workspace_bytes(C.c_void_p(q.ctypes.data), len(q))

    def audio_match(self, src_u8, dst_u8, queries, workspace=None):
        """src_u8, dst_u8: contiguous cuda uint8 streams; queries: 1..3 of (src_off, m, dst_off, win_len) ->
        cuda int32 [nq, 2]: first argmin offset, float32 bits of its value (.view(float32)[:, 1]), on the current stream
        (include/vse_hip.h vse_audio_match).  workspace: cuda uint8 of at least audio_match_workspace_bytes (allocated if None)."""
        t = self.torch
        assert src_u8.dtype == t.uint8 and src_u8.is_contiguous() and dst_u8.dtype == t.uint8 and dst_u8.is_contiguous()
        q = _audio_queries(queries)
        if workspace is None:
            need = self.lib.vse_audio_match_workspace_bytes(C.c_void_p(q.ctypes.data), len(q))
            workspace = t.empty(max(need, 256), dtype=t.uint8, device=self.tdev)
        out = t.empty((len(q), 2), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_audio_match(self.handle, C.c_void_p(src_u8.data_ptr()), src_u8.numel(), C.c_void_p(dst_u8.data_ptr()),
                                        dst_u8.numel(), C.c_void_p(q.ctypes.data), len(q), C.c_void_p(workspace.data_ptr()),
                                        workspace.numel(), C.c_void_p(out.data_ptr()), self.stream()), "vse_audio_match")
        return out

    # ---- timeline sync: WAV PCM -> uint8 search stream --------------------------------------------------------------
    def audio_stream_length(self, frames, channels, rate, sample_rate):
        """Elements of the uint8 stream of a WAV of `frames` frames (0 for what audio_stream_feed refuses)."""
        return int(self.lib.vse_audio_stream_length(int(frames), int(channels), int(rate), int(sample_rate)))

    def audio_stream_workspace(self, frames, channels, rate, sample_rate):
        """A workspace for audio_stream_feed / audio_stream_finish of such a file (it needs no content and serves later files that
        need no more bytes)."""
        nbytes = self.lib.vse_audio_stream_workspace_bytes(int(frames), int(channels), int(rate), int(sample_rate))
        if not nbytes:
            raise VseError(f"audio_stream: {frames} frames of {channels} channels at {rate} Hz for a {sample_rate} Hz stream: 1..8 channels, "
                           "a rate of at least the search rate, at least one frame and at most 2^31 - 1 stream elements")
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device=self.tdev)

    def audio_stream_feed(self, pcm_i16, first_second, frames, channels, rate, sample_rate, workspace):
        """pcm_i16: contiguous cuda int16 holding whole frames of the file from second `first_second` on (whole seconds, or up to the
        file's end) -> their samples in `workspace`, on the current stream (include/vse_hip.h vse_audio_stream_feed)."""
        t = self.torch
        channels = int(channels)
        assert pcm_i16.dtype == t.int16 and pcm_i16.is_contiguous() and (channels < 1 or pcm_i16.numel() % channels == 0)
        assert workspace.dtype == t.uint8 and workspace.is_contiguous()
        _check(self.lib.vse_audio_stream_feed(self.handle, C.c_void_p(pcm_i16.data_ptr()), pcm_i16.numel() // max(channels, 1), int(first_second),
                                              int(frames), int(channels), int(rate), int(sample_rate), C.c_void_p(workspace.data_ptr()),
                                              workspace.numel(), self.stream()), "vse_audio_stream_feed")

    def audio_stream_finish(self, frames, channels, rate, sample_rate, workspace, out=None, result=None):
        """-> (cuda uint8 [L] stream, cuda int32 [8] record: lo and hi as float32 bits, the sizes of the >= 0 and <= 0 sets, status) on
        the current stream (include/vse_hip.h vse_audio_stream_finish).  With status 1 (an empty level range) `out` is not written.
        out: a contiguous cuda uint8 tensor of L elements (any alignment) to write into."""
        t = self.torch
        length = self.audio_stream_length(frames, channels, rate, sample_rate)
        if out is None:
            out = t.empty(length, dtype=t.uint8, device=self.tdev)
        if result is None:
            result = t.empty(8, dtype=t.int32, device=self.tdev)
        assert out.dtype == t.uint8 and out.is_contiguous() and out.numel() == length
        assert result.dtype == t.int32 and result.is_contiguous() and result.numel() == 8
        assert workspace.dtype == t.uint8 and workspace.is_contiguous()
        _check(self.lib.vse_audio_stream_finish(self.handle, int(frames), int(channels), int(rate), int(sample_rate),
                                                C.c_void_p(workspace.data_ptr()), workspace.numel(), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(result.data_ptr()), self.stream()), "vse_audio_stream_finish")
        return out, result

    # ---- timeline sync: scene cuts for keyframe snapping ----------------------------------------------------------
    def scene_change_state(self, h, w, scale):
        """A fresh (zero-filled) state for scene_change over frames of h x w pixels at this scale."""
        nbytes = self.lib.vse_scene_change_state_bytes(int(h), int(w), int(scale))
        if not nbytes:
            raise VseError(f"scene_change: scale {scale} on {h} x {w} frames: the plane must be 16 x 16 .. 2^23 pixels, the scale 1..8")
        return self.torch.zeros(nbytes, dtype=self.torch.uint8, device=self.tdev)

    def scene_change(self, frames_u8, scale, search, bias, state, reset=False, workspace=None):
        """frames_u8: cuda uint8 [n,H,W,3] (any row pitch / frame stride, pixels packed), state: scene_change_state of this frame
        size and scale (carries the last frame's plane to the next call) -> cuda int32 [n,3]: changed macroblocks, sum of the
        blocks' best inter SADs, sum of their intra deviations per frame (include/vse_hip.h vse_scene_change).
        workspace: cuda uint8 of at least vse_scene_change_workspace_bytes (allocated if None)."""
        t = self.torch
        frames = self._frames_args(frames_u8)
        _, n, h, w = frames[:4]
        assert state.dtype == t.uint8 and state.is_contiguous()
        assert state.numel() >= max(self.lib.vse_scene_change_state_bytes(h, w, int(scale)), 1)
        if workspace is None:
            workspace = t.empty(max(self.lib.vse_scene_change_workspace_bytes(n, h, w, int(scale)), 256), dtype=t.uint8, device=self.tdev)
        out = t.empty((n, 3), dtype=t.int32, device=self.tdev)
        _check(self.lib.vse_scene_change(self.handle, *frames, int(scale), int(search), int(bias), C.c_void_p(state.data_ptr()), int(bool(reset)),
                                         C.c_void_p(workspace.data_ptr()), workspace.numel(), C.c_void_p(out.data_ptr()), self.stream()),
               "vse_scene_change")
        return out

    # ---- frame ingest: YUV 4:2:0 -> BGR ---------------------------------------------------------------------------
    def yuv420_to_bgr(self, packed_u8, n, h, w, layout="i420", row_parity=0, out=None, matrix=0):
        """packed_u8: cuda uint8 holding n packed 4:2:0 (sub-)frames of h x w pixels (include/vse_hip.h vse_yuv420_to_bgr: luma rows,
        then the chroma rows of layout "i420" | "nv12"), 1-D (frames back to back) or 2-D [n, stride] (frame stride = its row stride)
        -> cuda uint8 [n,h,w,3] BGR on the current stream.  out: write into this tensor instead (it may be a strided view with packed
        pixels; its pitch and frame stride are taken from it).  matrix: 0 | "bt601" (vse_yuv420_to_bgr's integers) or 1 | "bt709"
        (vse_yuv_to_bgr_matrix)."""
        t = self.torch
        n, h, w, row_parity = int(n), int(h), int(w), int(row_parity)
        matrix = YUV_MATRICES.get(matrix, matrix)
        if matrix not in (0, 1):
            raise VseError(f"yuv420_to_bgr: matrix {matrix!r} is not one of {sorted(YUV_MATRICES)} (0 | 1)")
        if layout not in YUV_LAYOUTS:
            raise VseError(f"yuv420_to_bgr: layout {layout!r} is not one of {sorted(YUV_LAYOUTS)}")
        frame = self.lib.vse_yuv420_frame_bytes(h, w, row_parity)
        sstride = _packed_stride(packed_u8, n, frame, "packed_u8")
        if out is None:
            out = t.empty((max(n, 0), max(h, 0), max(w, 0), 3), dtype=t.uint8, device=self.tdev)
        assert out.dtype == t.uint8 and tuple(out.shape) == (n, h, w, 3) and out.stride(3) == 1 and out.stride(2) == 3
        dstride = out.stride(0) if n > 1 else max(out.stride(0), (h - 1) * out.stride(1) + 3 * w)
        if matrix == 0:
            _check(self.lib.vse_yuv420_to_bgr(self.handle, C.c_void_p(packed_u8.data_ptr()), n, h, w, YUV_LAYOUTS[layout], row_parity, sstride,
                                              C.c_void_p(out.data_ptr()), out.stride(1), dstride, self.stream()), "vse_yuv420_to_bgr")
        else:
            _check(self.lib.vse_yuv_to_bgr_matrix(self.handle, C.c_void_p(packed_u8.data_ptr()), n, h, w, YUV_LAYOUTS[layout], row_parity, sstride,
                                                  C.c_void_p(out.data_ptr()), out.stride(1), dstride, matrix, self.stream()),
                   "vse_yuv_to_bgr_matrix")
        return out

    def tone_table(self, tone):
        """The device copy of an ingest.ToneMap's table (anything hashable with packed() -> the 16128 bytes and tables() -> (A, T, M)) and
        its gamut as ctypes int32[9], uploaded on first use and kept for the context's life."""
        with self._tone_lock:
            hit = self._tone_tables.get(tone)
            if hit is None:
                t = self.torch
                host = np.frombuffer(tone.packed(), np.uint8)
                if host.size != self.lib.vse_yuv_tonemap_table_bytes():
                    raise VseError(f"tone_table: a table of {host.size} bytes, not {self.lib.vse_yuv_tonemap_table_bytes()}")
                dev = t.from_numpy(host.copy()).to(self.tdev)
                t.cuda.current_stream(self.tdev).synchronize()          # any stream may read it from here on
                hit = self._tone_tables[tone] = (dev, (C.c_int32 * 9)(*[int(v) for v in np.asarray(tone.tables()[2]).reshape(-1)]))
            return hit

    def yuv_to_bgr(self, packed, n, h, w, fmt, row_parity=0, out=None, tone=None):
        """packed: cuda uint8 holding n packed (sub-)frames of h x w pixels of the format `fmt` (an ingest.YuvFormat, or anything with its
        integer attributes sub_x, sub_y, chroma, depth, msb, matrix, full_range; include/vse_hip.h vse_yuv_to_bgr_format), 1-D (frames back
        to back) or 2-D [n, stride in bytes] -> cuda uint8 [n,h,w,3] BGR on the current stream.  out: as yuv420_to_bgr's.  tone: an
        ingest.ToneMap: convert HDR material to SDR with its tables (vse_yuv_to_bgr_tonemap; see tone_table)."""
        t = self.torch
        n, h, w, row_parity = int(n), int(h), int(w), int(row_parity)
        matrix = YUV_FORMAT_MATRICES.get(fmt.matrix, fmt.matrix)
        if matrix not in (0, 1, 2):
            raise VseError(f"yuv_to_bgr: matrix {fmt.matrix!r} is not one of {sorted(YUV_FORMAT_MATRICES)} (0 | 1 | 2)")
        frame = self.lib.vse_yuv_frame_bytes(h, w, int(fmt.sub_x), int(fmt.sub_y), int(fmt.chroma), int(fmt.depth), row_parity)
        sstride = _packed_stride(packed, n, frame, "packed")
        if out is None:
            out = t.empty((max(n, 0), max(h, 0), max(w, 0), 3), dtype=t.uint8, device=self.tdev)
        assert out.dtype == t.uint8 and tuple(out.shape) == (n, h, w, 3) and out.stride(3) == 1 and out.stride(2) == 3
        dstride = out.stride(0) if n > 1 else max(out.stride(0), (h - 1) * out.stride(1) + 3 * w)
        if tone is not None:
            table, gamut = self.tone_table(tone)
            _check(self.lib.vse_yuv_to_bgr_tonemap(self.handle, C.c_void_p(packed.data_ptr()), n, h, w, int(fmt.sub_x), int(fmt.sub_y),
                                                   int(fmt.chroma), int(fmt.depth), int(fmt.msb), matrix, int(fmt.full_range), row_parity, sstride,
                                                   C.c_void_p(out.data_ptr()), out.stride(1), dstride, C.c_void_p(table.data_ptr()), gamut,
                                                   self.stream()), "vse_yuv_to_bgr_tonemap")
            return out
        _check(self.lib.vse_yuv_to_bgr_format(self.handle, C.c_void_p(packed.data_ptr()), n, h, w, int(fmt.sub_x), int(fmt.sub_y), int(fmt.chroma),
                                              int(fmt.depth), int(fmt.msb), matrix, int(fmt.full_range), row_parity, sstride,
                                              C.c_void_p(out.data_ptr()), out.stride(1), dstride, self.stream()), "vse_yuv_to_bgr_format")
        return out

    def yuv_deinterlace(self, packed, n, h, w, fmt, prev=None, prev_stride=None, keep=0, mode=0, thresh=10, out=None):
        """packed: cuda uint8 holding n packed interlaced pictures of h x w pixels of the format `fmt` (as yuv_to_bgr's, row parity 0), 1-D
        (back to back) or 2-D [n, stride in bytes] -> cuda uint8 [n, stride] of the progressive pictures in the same packing, on the current
        stream (include/vse_hip.h vse_yuv_deinterlace).  prev: a cuda uint8 tensor whose first byte is the previous picture of frame 0 (None:
        no frame has one, all are interpolated); frame f's previous picture lies f * prev_stride bytes behind it (default: prev's own row
        stride when it is 2-D, else packed's frame stride), so a run of consecutive frames in one buffer passes the view that starts one
        frame earlier.  keep: 0 top field first | 1 bottom field first; mode: 0 | "adaptive", 1 | "interpolate"; thresh in 8-bit levels.
        out: write into this uint8 tensor (1-D or [n, stride]) instead; it must not overlap the inputs."""
        t = self.torch
        n, h, w = int(n), int(h), int(w)
        mode = DEINTERLACE_MODES.get(mode, mode)
        if mode not in (0, 1):
            raise VseError(f"yuv_deinterlace: mode {mode!r} is not one of {sorted(DEINTERLACE_MODES)} (0 | 1)")
        frame = self.lib.vse_yuv_frame_bytes(h, w, int(fmt.sub_x), int(fmt.sub_y), int(fmt.chroma), int(fmt.depth), 0)
        sstride = _packed_stride(packed, n, frame, "packed")
        if out is None:
            out = t.empty((max(n, 0), (frame + 15) & ~15), dtype=t.uint8, device=self.tdev)
        ostride = _packed_stride(out, n, frame, "out")
        pptr, pstride = _prev_pictures(prev, prev_stride, n, sstride)
        _check(self.lib.vse_yuv_deinterlace(self.handle, C.c_void_p(packed.data_ptr()), pptr, n, h, w, int(fmt.sub_x), int(fmt.sub_y),
                                            int(fmt.chroma), int(fmt.depth), int(fmt.msb), int(keep), mode, int(thresh), sstride, pstride,
                                            C.c_void_p(out.data_ptr()), ostride, self.stream()), "vse_yuv_deinterlace")
        return out

    def yuv_field_match(self, packed, n, h, w, fmt, prev=None, prev_stride=None, keep=0, comb_thresh=10, comb_limit=20, thresh=10, out=None,
                        stats=None):
        """yuv_deinterlace's arguments and layouts -> (cuda uint8 [n, stride] of the field-matched pictures, cuda int32 [n, 4] of each
        frame's comb counts of the candidates c, p1, p2 and its choice 0..3), on the current stream (include/vse_hip.h vse_yuv_field_match):
        each frame is woven from its own fields or with a field of the previous picture, whichever combs least; a frame that combs by
        more than comb_limit per mille (None: never) of its luma samples with every partner gets the adaptive rule with `thresh`.
        prev None: no frame has a previous picture.  stats: write into this int32 [n, 4] tensor instead (the uint32 words of the device)."""
        t = self.torch
        n, h, w = int(n), int(h), int(w)
        frame = self.lib.vse_yuv_frame_bytes(h, w, int(fmt.sub_x), int(fmt.sub_y), int(fmt.chroma), int(fmt.depth), 0)
        sstride = _packed_stride(packed, n, frame, "packed")
        if out is None:
            out = t.empty((max(n, 0), (frame + 15) & ~15), dtype=t.uint8, device=self.tdev)
        ostride = _packed_stride(out, n, frame, "out")
        if stats is None:
            stats = t.empty((max(n, 0), 4), dtype=t.int32, device=self.tdev)
        assert stats.dtype == t.int32 and tuple(stats.shape) == (n, 4) and stats.is_contiguous()
        pptr, pstride = _prev_pictures(prev, prev_stride, n, sstride)
        _check(self.lib.vse_yuv_field_match(self.handle, C.c_void_p(packed.data_ptr()), pptr, n, h, w, int(fmt.sub_x), int(fmt.sub_y),
                                            int(fmt.chroma), int(fmt.depth), int(fmt.msb), int(keep), int(comb_thresh),
                                            -1 if comb_limit is None else int(comb_limit), int(thresh), sstride, pstride,
                                            C.c_void_p(out.data_ptr()), ostride, C.c_void_p(stats.data_ptr()), self.stream()),
               "vse_yuv_field_match")
        return out, stats

    def _upload_tables(self, who, cache, key, source, fmt, axis, edge, lengths, support=None):
        """resample_tables and vscale_tables: source.tables(fmt) / source.packed(fmt) checked, uploaded once under `key` and kept in
        `cache`.  axis, edge: the words of the messages ("columns", "left" | "rows", "top"); lengths: the entries of the luma and the
        chroma table; support: the stored rows of the two planes, where each entry gets its ingest.table_support(edge, coef, rows)."""
        with self._tone_lock:
            hit = cache.get(key)
            if hit is None:
                t = self.torch
                devs = []
                for p, (what, tab, raw, size) in enumerate(zip(("luma", "chroma"), source.tables(fmt), source.packed(fmt), lengths)):
                    if tab is None:
                        devs.append(None)
                        continue
                    first, coef = np.asarray(tab[0]), np.asarray(tab[1])
                    taps = int(coef.shape[1]) if coef.ndim == 2 else 0
                    host = np.frombuffer(raw, np.uint8)
                    want = self.lib.vse_yuv_resample_table_bytes(size, taps)
                    if not want or first.shape != (size,) or coef.shape != (size, taps) or host.size != want:
                        raise VseError(f"{who}: the {what} table of {size} {axis} has {edge} {first.shape}, coef {coef.shape} (taps even, "
                                       f"2..16) and {host.size} bytes of {want}")
                    if np.abs(first.astype(np.int64)).max() > 1 << 30 or np.abs(coef.astype(np.int64)).sum(axis=1).max() > 32767:
                        raise VseError(f"{who}: the {what} table breaks |{edge}| <= 2^30 or a row's sum of |coef| <= 32767 (max "
                                       f"{int(np.abs(coef.astype(np.int64)).sum(axis=1).max())}): int32 would not be exact")
                    dev = (t.from_numpy(host.copy()).to(self.tdev), taps)
                    if support is not None:
                        from .ingest import table_support
                        dev += table_support(first, coef, support[p])
                    devs.append(dev)
                if devs[0] is None or (devs[1] is None) != (not fmt.chroma):
                    raise VseError(f"{who}: {fmt} takes a luma table and {'a' if fmt.chroma else 'no'} chroma table")
                t.cuda.current_stream(self.tdev).synchronize()          # any stream may read them from here on
                hit = cache[key] = tuple(devs)
            return hit

    def resample_tables(self, resample, fmt):
        """The device copies of an ingest.Resample's tables for the format `fmt` (anything hashable with in_width, out_width, tables(fmt)
        -> ((left, coef), (left, coef) | None) and packed(fmt) -> (luma bytes, chroma bytes | None)): ((cuda uint8 table, taps), the same
        for chroma or None), uploaded on first use and kept for the context's life.  vse_yuv_resample cannot read them, so the bounds
        that keep its int32 sums exact are checked here: |left| <= 2^30 and every row's sum of |coef| <= 32767."""
        sx, w_out = int(fmt.sub_x), int(resample.out_width)
        return self._upload_tables("resample_tables", self._resample_tables, (resample, sx, bool(fmt.chroma)), resample, fmt, "columns", "left",
                                   (w_out, (w_out + sx) >> sx))

    def yuv_resample(self, packed, n, h, w_in, fmt, resample, row_parity=0, out=None):
        """packed: cuda uint8 holding n packed (sub-)frames of h x w_in pixels of the format `fmt` (as yuv_to_bgr's), 1-D (back to back) or
        2-D [n, stride in bytes] -> cuda uint8 [n, stride] of the pictures resampled along their rows to resample.out_width columns, in the
        same packing, on the current stream (include/vse_hip.h vse_yuv_resample).  resample: an ingest.Resample (see resample_tables) whose
        in_width is w_in.  out: write into this uint8 tensor (1-D or [n, stride]) instead; it must not overlap the input or the tables."""
        t = self.torch
        n, h, w_in, row_parity = int(n), int(h), int(w_in), int(row_parity)
        if int(resample.in_width) != w_in:
            raise VseError(f"yuv_resample: the tables are for {resample.in_width} stored columns, the pictures have {w_in}")
        w_out = int(resample.out_width)
        form = (int(fmt.sub_x), int(fmt.sub_y), int(fmt.chroma), int(fmt.depth))
        frame_in = self.lib.vse_yuv_frame_bytes(h, w_in, *form, row_parity)
        frame_out = self.lib.vse_yuv_frame_bytes(h, w_out, *form, row_parity)
        sstride = _packed_stride(packed, n, frame_in, "packed")
        if out is None:
            out = t.empty((max(n, 0), (frame_out + 15) & ~15), dtype=t.uint8, device=self.tdev)
        ostride = _packed_stride(out, n, frame_out, "out")
        luma, chroma = self.resample_tables(resample, fmt)
        _check(self.lib.vse_yuv_resample(self.handle, C.c_void_p(packed.data_ptr()), n, h, w_in, w_out, *form, int(fmt.msb), row_parity,
                                         C.c_void_p(luma[0].data_ptr()), luma[1], None if chroma is None else C.c_void_p(chroma[0].data_ptr()),
                                         0 if chroma is None else chroma[1], sstride, C.c_void_p(out.data_ptr()), ostride, self.stream()),
               "vse_yuv_resample")
        return out

    def vscale_tables(self, vscale, fmt):
        """The device copies of an ingest.VScale's tables for the format `fmt` (anything hashable with in_height, out_height, tables(fmt)
        -> ((top, coef), (top, coef) | None) and packed(fmt) -> (luma bytes, chroma bytes | None)): ((cuda uint8 table, taps, lo, hi), the
        same for chroma or None), uploaded on first use and kept for the context's life.  lo, hi: per output row the stored rows [lo, hi)
        of the plane that it reads with a coefficient other than zero (ingest.table_support), for the band check of yuv_vscale.
        vse_yuv_vscale cannot read the tables, so the bounds that keep its int32 sums exact are checked here: |top| <= 2^30 and every
        row's sum of |coef| <= 32767."""
        sy, h_in, h_out = int(fmt.sub_y), int(vscale.in_height), int(vscale.out_height)
        return self._upload_tables("vscale_tables", self._vscale_tables, (vscale, sy, bool(fmt.chroma)), vscale, fmt, "rows", "top",
                                   (h_out, (h_out + sy) >> sy), support=(h_in, (h_in + sy) >> sy))

    def yuv_vscale(self, packed, n, h_in, w, fmt, vscale, s0, s1, y0, y1, out=None):
        """packed: cuda uint8 holding n packed bands of stored luma rows [s0, s1) of pictures of h_in x w pixels of the format `fmt` (what
        ingest.YuvFrame.pack_into writes), 1-D (back to back) or 2-D [n, stride in bytes] -> cuda uint8 [n, stride] of the packed bands of
        output rows [y0, y1) of the pictures scaled to vscale.out_height rows, same width, on the current stream (include/vse_hip.h
        vse_yuv_vscale).  vscale: an ingest.VScale (see vscale_tables) whose in_height is h_in.  The band must hold every stored row that
        rows [y0, y1) read in every plane (VScale.source_rows gives the smallest one): the device clamps to the band, and a band that is
        too small would give other rows than the whole picture's.  out: write into this uint8 tensor (1-D or [n, stride]) instead; it
        must not overlap the input or the tables."""
        t = self.torch
        n, h_in, w, s0, s1, y0, y1 = (int(v) for v in (n, h_in, w, s0, s1, y0, y1))
        if int(vscale.in_height) != h_in:
            raise VseError(f"yuv_vscale: the tables are for {vscale.in_height} stored rows, the pictures have {h_in}")
        h_out, sy = int(vscale.out_height), int(fmt.sub_y)
        form = (int(fmt.sub_x), sy, int(fmt.chroma), int(fmt.depth))
        luma, chroma = self.vscale_tables(vscale, fmt)
        if not (0 <= s0 < s1 <= h_in and 0 <= y0 < y1 <= h_out):
            raise VseError(f"yuv_vscale: stored rows {s0}:{s1} of {h_in} and output rows {y0}:{y1} of {h_out} must lie inside their pictures "
                           "and not be empty")
        for what, tab, (a, b), (r0, r1) in (("luma", luma, (s0, s1), (y0, y1)),
                                            ("chroma", chroma, (s0 >> sy, ((s1 - 1) >> sy) + 1), (y0 >> sy, ((y1 - 1) >> sy) + 1))):
            if tab is None:
                continue
            lo, hi = int(tab[2][r0:r1].min()), int(tab[3][r0:r1].max())
            if lo < hi and not (a <= lo and hi <= b):
                raise VseError(f"yuv_vscale: the band of stored rows {s0}:{s1} holds {what} rows {a}:{b}, output rows {y0}:{y1} read {what} "
                               f"rows {lo}:{hi}: the band does not cover the support")
        frame_in = self.lib.vse_yuv_frame_bytes(s1 - s0, w, *form, s0 & sy)
        frame_out = self.lib.vse_yuv_frame_bytes(y1 - y0, w, *form, y0 & sy)
        sstride = _packed_stride(packed, n, frame_in, "packed")
        if out is None:
            out = t.empty((max(n, 0), (frame_out + 15) & ~15), dtype=t.uint8, device=self.tdev)
        ostride = _packed_stride(out, n, frame_out, "out")
        _check(self.lib.vse_yuv_vscale(self.handle, C.c_void_p(packed.data_ptr()), n, w, h_in, h_out, s0, s1, y0, y1, *form, int(fmt.msb),
                                       C.c_void_p(luma[0].data_ptr()), luma[1], None if chroma is None else C.c_void_p(chroma[0].data_ptr()),
                                       0 if chroma is None else chroma[1], sstride, C.c_void_p(out.data_ptr()), ostride, self.stream()),
               "vse_yuv_vscale")
        return out


YUV_LAYOUTS = {"i420": 0, "nv12": 1}
YUV_MATRICES = {"bt601": 0, "bt709": 1}
YUV_FORMAT_MATRICES = {"bt601": 0, "bt709": 1, "bt2020": 2}      # vse_yuv_to_bgr_format's
DEINTERLACE_MODES = {"adaptive": 0, "interpolate": 1}            # vse_yuv_deinterlace's
INTERVAL_MODES = {"min": 0, "max": 1, "mean": 2}
INTERVAL_SEG_CONTINUE, INTERVAL_SEG_EMIT = 1, 2          # vse_interval_seg.flags (include/vse_hip.h)
INTERVAL_STREAM_MAX_SEGS = 32   # VSE_INTERVAL_STREAM_MAX_SEGS: the segments of one vse_interval_stream call
INTERVAL_RANK_MAX = 63          # VSE_INTERVAL_RANK_MAX (include/vse_hip.h): the frames of one vse_interval_rank call
INTERVAL_RING_MAX_GROUPS = 8    # VSE_INTERVAL_RING_MAX_GROUPS: the groups of one vse_interval_ring_rank call
FRAME_HOLD_BOUNDED_MAX = 4000   # the largest max_hold of vse_frame_hold_bounded (include/vse_hip.h)


def _audio_queries(queries):
    q = np.ascontiguousarray(np.array([[int(v) for v in x] for x in queries], dtype=np.int64).reshape(-1, 4))
    return q


class Net:
    """One model (descriptor + fp32 weights) with plans compiled per static input shape."""

    def __init__(self, ctx: Context, desc, weights, fetch_cols=(0,), want_probs=True, hilo=False, ragged=False, input_norm=None,
                 fuse_preprocess=False, chain=None, tail2=True, limits=None):
        """hilo=True: conv weights as fp16 hi + lo pairs (compiler.compile_model): ~22-bit weights, twice the MFMA work.
        ragged=True (recognisers): every plan takes a per-sample width vector (run(x, widths=...)); a sample's outputs do
        not depend on the batch it rides in (compiler.compile_model(ragged=True))."""
        self.ctx = ctx
        self.ragged = bool(ragged)
        self.input_norm = input_norm          # (mean3, std3): the net takes det_preprocess(raw=True) input (compiler.compile_model)
        # the stem conv resizes the uint8 frames itself (needs input_norm): the plans take FRAMES — det_forward / profile_frames;
        # run(x) with a pre-processed tensor is refused by the library
        self.fuse_preprocess = bool(fuse_preprocess) and input_norm is not None
        self.desc = desc
        self.weights = weights
        self.fetch_cols = fetch_cols
        self.want_probs = want_probs
        self.hilo = bool(hilo)
        self.tail2 = tail2                    # False: the server detector's two head deconvs as separate launches (compiler F_TAIL2; tests)
        self.chain = chain                    # None: 1x1 / depthwise chains (OP_CHAIN) for hi + lo nets; False / True forces it
        self.limits = limits                  # None: the product's conv routing thresholds (conv_route.RouteLimits; tools/bench_conv.py)
        self.store = compiler.WeightStore()
        self.plans = {}
        self.wid = None
        self.wbytes = 0
        self.ws = {}          # one workspace per plan: plans of one net may run concurrently on different streams
        self.ws_budget = int(float(os.environ.get("VSE_WS_BUDGET_GB", "64")) * (1 << 30))     # per net; LRU beyond it
        self.ws_evictions = 0 # workspaces dropped by that LRU so far (tools/soak.py reports it)
        self.fallbacks = {}   # rewrites compile_model had to abandon for this graph (tail2 / se_lateral): remembered for the next shape

    def program(self, n, h, w):
        key = (n, h, w)
        if key not in self.plans:
            try:
                prog = compiler.compile_model(self.desc, self.weights, n, h, w, self.fetch_cols, self.want_probs,
                                              self.store, hilo=self.hilo, ragged=self.ragged, input_norm=self.input_norm,
                                              fuse_preprocess=self.fuse_preprocess, chain=self.chain,
                                              tail2=self.fallbacks.get("tail2", self.tail2),
                                              se_lateral=self.fallbacks.get("se_lateral", True), fallbacks=self.fallbacks, limits=self.limits)
            except compiler.UnsupportedGraph:
                if not self.fuse_preprocess or self.plans:
                    raise
                self.fuse_preprocess = False      # a graph whose feed is not read by one 3x3 stem conv: keep the pre-processing pass
                return self.program(n, h, w)
            self.plans[key] = [prog, None]
        return self.plans[key][0]

    def _ensure(self, key):
        prog, handle = self.plans[key]
        lib = self.ctx.lib
        if self.wid is None or len(self.store.blob) != self.wbytes:
            # (re-)upload the shared weight blob; plans created against an older blob are rebuilt lazily
            blob = self.store.array()
            self._drop_graphs()               # captured graphs replay kernels against the plan handles / weight blob freed below
            if self.wid is not None:
                for k, (p_, h_) in self.plans.items():
                    if h_ is not None:
                        lib.vse_plan_destroy(h_)
                        self.plans[k][1] = None
                lib.vse_weights_free(self.ctx.handle, self.wid)
            self.wid = _check(lib.vse_weights_upload(self.ctx.handle, blob.ctypes.data_as(C.c_void_p), blob.nbytes),
                              "vse_weights_upload")
            self.wbytes = len(self.store.blob)
            handle = None
        if handle is None:
            h = C.c_void_p()
            ops = np.ascontiguousarray(prog.ops)
            _check(lib.vse_plan_create(self.ctx.handle, self.wid, ops.ctypes.data_as(C.c_void_p), len(ops),
                                       prog.ws_bytes, C.byref(h)), "vse_plan_create")
            self.plans[key][1] = h
            handle = h
        return prog, handle

    GRAPH_CACHE_MAX = 32      # captured recogniser graphs kept per net (each pins input, workspace and output buffers)

    def _drop_graphs(self, keep=0):
        """Destroy captured recogniser graphs, oldest first, until `keep` are left (after a device synchronisation: they may be
        in flight)."""
        graphs = self.__dict__.get("_graphs")
        if not graphs or len(graphs) <= keep:
            return
        self.ctx.torch.cuda.synchronize(self.ctx.tdev)
        while len(graphs) > keep:
            bufs = graphs.pop(next(iter(graphs)))
            if bufs["graph"] is not None:
                self.ctx.lib.vse_graph_destroy(bufs["graph"])

    def _workspace(self, key, prog, slot):
        """One workspace per (plan, slot): a plan is stateless between runs, so the same plan may run concurrently on
        several streams as long as every in-flight run has its own slot."""
        t = self.ctx.torch
        k = (key, slot)
        ent = self.ws.pop(k, None)            # (view handed to the plan, stream of its last use)
        cur = t.cuda.current_stream(self.ctx.tdev)
        if ent is None:
            # a long video meets many recogniser shapes (crops x width bucket), each with a workspace of its own (they are
            # zero-initialised and their padding regions must stay zero, so plans cannot share one): the total is kept under a
            # budget, least recently used first.  No device synchronisation and, where possible, no allocator round trip:
            #  * a victim last used on THIS stream and large enough is re-zeroed and reused in place — the memset and the new plan's
            #    launches queue behind its last launch on that stream (a recogniser slot always runs on the same side stream);
            #  * otherwise victims are dropped (every use records its stream, so the caching allocator holds the memory back until
            #    its launches finished) and a fresh buffer is allocated.
            # (Round 6: a synchronising eviction drained the detector batches in flight, -4 % on a stream at its budget; dropping
            # without reuse made a host that runs a span ahead wait in hipMalloc for blocks still held back: -4 % again.)
            need = max(prog.ws_bytes, 256)
            total = sum(int(e[0].untyped_storage().nbytes()) for e in self.ws.values())
            ws = None
            if self.ws and total + need > self.ws_budget:
                for vk, (vws, vstream) in self.ws.items():           # least recently used first
                    cap = int(vws.untyped_storage().nbytes())
                    if vstream == cur.cuda_stream and need <= cap <= 4 * need:
                        del self.ws[vk]
                        self.ws_evictions += 1
                        base = t.empty(0, dtype=t.uint8, device=self.ctx.tdev).set_(vws.untyped_storage(), 0, (cap,))
                        ws = base[:need]
                        ws.zero_()
                        break
            if ws is None:
                while self.ws and total + need > self.ws_budget:
                    total -= int(self.ws.pop(next(iter(self.ws)))[0].untyped_storage().nbytes())
                    self.ws_evictions += 1
                ws = t.zeros(need, dtype=t.uint8, device=self.ctx.tdev)
        else:
            ws = ent[0]
        ws.record_stream(cur)
        self.ws[k] = (ws, cur.cuda_stream)    # (re-)inserted last: dict order = least recently used first
        return ws

    def _ext(self, prog, x):
        t = self.ctx.torch
        outs = [t.empty((o["n"], o["h"], o["w"], o["ld"]), dtype=t.float32, device=self.ctx.tdev)
                for o in prog.outputs]
        ptrs = (C.c_void_p * (1 + len(outs)))(x.data_ptr(), *[o.data_ptr() for o in outs])
        return outs, ptrs

    def _width_table(self, prog, widths, n, w):
        """Device int32 [levels][n] for a ragged plan (None for an ordinary one)."""
        if not self.ragged:
            if widths is not None:
                raise VseError("per-sample widths given to a net that was not built with ragged=True")
            return None
        if widths is None:
            widths = np.full(n, w, np.int32)          # a uniform batch: every sample as wide as the tensor
        return self._upload_i32(prog.width_table(widths))

    def _upload_i32(self, tab, out=None):
        """Stream-ordered upload of a small int32 host table through a ring of reusable pinned buffers.  A pageable
        `tensor.to(device)` blocks the host until the stream has drained (every recogniser group would wait for the previous
        group's ~80 kernels); a pinned buffer allocated per call costs as much as that stall (round 3 log) — the ring costs
        neither: slot i is reused after 8 further uploads, guarded by the event recorded behind its last copy."""
        t = self.ctx.torch
        ring = self.__dict__.setdefault("_pin_ring", {"slots": [None] * 8, "next": 0})
        i = ring["next"] % len(ring["slots"])
        ring["next"] += 1
        slot = ring["slots"][i]
        if slot is None or slot[0].numel() < tab.size:
            if slot is not None:
                slot[1].synchronize()
            slot = ring["slots"][i] = (t.empty(max(int(tab.size), 1024), dtype=t.int32).pin_memory(), t.cuda.Event())
        else:
            slot[1].synchronize()             # the copy that last read this slot (8 uploads ago) has long finished
        pin = slot[0][:tab.size].view(tab.shape)
        pin.numpy()[...] = tab
        dev = out if out is not None else t.empty(tab.shape, dtype=t.int32, device=self.ctx.tdev)
        dev.copy_(pin, non_blocking=True)
        slot[1].record(t.cuda.current_stream(self.ctx.tdev))
        return dev

    def run(self, x, slot=0, widths=None):
        """x: cuda fp16 [N,H,W,8] NHWC (3 real channels).  Returns list of fp32 cuda tensors (prog.outputs order).
        widths (ragged nets): per-sample input width (<= W; x is zero right of it); self.last_tlen then holds the device
        int32 [N] sequence lengths of the head's output."""
        t = self.ctx.torch
        assert x.dtype == t.float16 and x.is_contiguous() and x.shape[3] == 8, (x.dtype, x.shape)
        n, h, w, _ = x.shape
        self.program(n, h, w)
        prog, handle = self._ensure((n, h, w))
        outs, ptrs = self._ext(prog, x)
        ws = self._workspace((n, h, w), prog, slot)
        wt = self._width_table(prog, widths, n, w)
        self.last_tlen = wt[prog.out_level] if wt is not None else None
        _check(self.ctx.lib.vse_plan_run_ragged(handle, C.c_void_p(ws.data_ptr()), ptrs, len(ptrs),
                                                C.c_void_p(wt.data_ptr()) if wt is not None else None, self.ctx.stream()),
               "vse_plan_run")
        return outs

    def det_forward(self, frames_u8, dst_h, dst_w, slot=0):
        """Model-level call of a detector net (vse_det_forward): cuda uint8 [N,H,W,3] -> cuda fp32 probability maps [N,dst_h,dst_w]."""
        t = self.ctx.torch
        assert frames_u8.dtype == t.uint8 and frames_u8.dim() == 4 and frames_u8.shape[3] == 3
        assert frames_u8.stride(3) == 1 and frames_u8.stride(2) == 3
        n, h, w, _ = frames_u8.shape
        self.program(n, dst_h, dst_w)
        prog, handle = self._ensure((n, dst_h, dst_w))
        assert len(prog.outputs) == 1 and prog.outputs[0]["kind"] == "map" and prog.outputs[0]["ld"] == 1, "not a one-map detector plan"
        x = None if self.fuse_preprocess else t.empty((n, dst_h, dst_w, 8), dtype=t.float16, device=self.ctx.tdev)
        prob = t.empty((n, dst_h, dst_w), dtype=t.float32, device=self.ctx.tdev)
        ws = self._workspace((n, dst_h, dst_w), prog, slot)
        _check(self.ctx.lib.vse_det_forward(self.ctx.handle, handle, C.c_void_p(ws.data_ptr()), C.c_void_p(frames_u8.data_ptr()), n, h, w,
                                            frames_u8.stride(1), frames_u8.stride(0), dst_h, dst_w, 1 if self.input_norm is not None else 0,
                                            C.c_void_p(x.data_ptr()) if x is not None else None, C.c_void_p(prob.data_ptr()),
                                            self.ctx.stream()), "vse_det_forward")
        return prob

    def profile_frames(self, frames_u8, dst_h, dst_w, slot=0):
        """profile() of a detector net fed FRAMES: pre-processing pass + plan for an ordinary net, the plan alone when its stem
        pre-processes.  -> (ms per op, program, kernel names); self.last_outs = the outputs."""
        if not self.fuse_preprocess:
            return self.profile(self.ctx.det_preprocess(frames_u8, dst_h, dst_w, raw=self.input_norm is not None), slot)
        t = self.ctx.torch
        n, h, w, _ = frames_u8.shape
        self.program(n, dst_h, dst_w)
        prog, handle = self._ensure((n, dst_h, dst_w))
        _check(self.ctx.lib.vse_plan_set_source(handle, h, w, frames_u8.stride(1), frames_u8.stride(0)), "vse_plan_set_source")
        outs = [t.empty((o["n"], o["h"], o["w"], o["ld"]), dtype=t.float32, device=self.ctx.tdev) for o in prog.outputs]
        ptrs = (C.c_void_p * (1 + len(outs)))(frames_u8.data_ptr(), *[o.data_ptr() for o in outs])
        ms = (C.c_float * len(prog.ops))()
        ws = self._workspace((n, dst_h, dst_w), prog, slot)
        self.last_outs = outs
        _check(self.ctx.lib.vse_plan_profile(handle, C.c_void_p(ws.data_ptr()), ptrs, len(ptrs), None, self.ctx.stream(), ms),
               "vse_plan_profile")
        names = profiled_kernel_names(prog.ops, ms)
        return np.array(ms[:], dtype=np.float32), prog, names

    def rec_forward(self, x, widths=None, slot=0):
        """Model-level call of a recogniser net built with want_probs=False (vse_rec_forward): fp16 [B,h,w,8] (+ per-sample widths of
        a ragged net) -> (class ids int32 [B,T], lengths int32 [B], mean confidences fp32 [B]) cuda tensors."""
        t = self.ctx.torch
        assert x.dtype == t.float16 and x.is_contiguous() and x.shape[3] == 8
        n, h, w, _ = x.shape
        self.program(n, h, w)
        prog, handle = self._ensure((n, h, w))
        assert len(prog.outputs) == 1 and prog.outputs[0]["kind"] == "idx_maxp"
        tt = prog.outputs[0]["w"]
        wt = self._width_table(prog, widths, n, w)
        idx_maxp = t.empty((n, 1, tt, 2), dtype=t.float32, device=self.ctx.tdev)
        oi = t.zeros((n, tt), dtype=t.int32, device=self.ctx.tdev)
        ol = t.empty((n,), dtype=t.int32, device=self.ctx.tdev)
        oc = t.empty((n,), dtype=t.float32, device=self.ctx.tdev)
        ws = self._workspace((n, h, w), prog, slot)
        _check(self.ctx.lib.vse_rec_forward(self.ctx.handle, handle, C.c_void_p(ws.data_ptr()), C.c_void_p(x.data_ptr()),
                                            C.c_void_p(wt.data_ptr()) if wt is not None else None, prog.out_level,
                                            C.c_void_p(idx_maxp.data_ptr()), n, tt, C.c_void_p(oi.data_ptr()), C.c_void_p(ol.data_ptr()),
                                            C.c_void_p(oc.data_ptr()), self.ctx.stream()), "vse_rec_forward")
        return oi, ol, oc

    def rec_graph_buffers(self, n, h, w, slot=0):
        """Fixed buffers of the HIP-graph form of rec_forward for plan key (n, h, w) and workspace slot: the caller fills
        bufs["x"] (recogniser input, e.g. rec_preprocess(out=bufs["x"])) and calls rec_forward_graph(bufs, widths)."""
        t = self.ctx.torch
        key = (n, h, w, slot)
        if not hasattr(self, "_graphs"):
            self._graphs = {}
        if key in self._graphs:
            self._graphs[key] = self._graphs.pop(key)      # most recently used last
        else:
            self._drop_graphs(keep=self.GRAPH_CACHE_MAX - 1)
            self.program(n, h, w)
            prog, handle = self._ensure((n, h, w))
            tt = prog.outputs[0]["w"]
            dev = self.ctx.tdev
            self._graphs[key] = dict(
                x=t.zeros((n, h, w, 8), dtype=t.float16, device=dev), wt=t.zeros((len(prog.wlevels), n), dtype=t.int32, device=dev),
                idx_maxp=t.empty((n, 1, tt, 2), dtype=t.float32, device=dev), oi=t.zeros((n, tt), dtype=t.int32, device=dev),
                ol=t.zeros((n,), dtype=t.int32, device=dev), oc=t.zeros((n,), dtype=t.float32, device=dev), graph=None, tt=tt,
                wsbuf=t.zeros(max(prog.ws_bytes, 256), dtype=t.uint8, device=dev), prog=prog, handle=handle)
        return self._graphs[key]

    def rec_forward_graph(self, bufs, widths):
        """rec_forward through a HIP graph captured on first use (on the CURRENT stream, which must not be the default one);
        -> clones of (class ids, lengths, confidences) (the fixed output buffers are overwritten by the next launch)."""
        t = self.ctx.torch
        prog = bufs["prog"]
        self._upload_i32(prog.width_table(widths), out=bufs["wt"])
        if bufs["graph"] is None:
            g = C.c_void_p()
            n = bufs["x"].shape[0]
            _check(self.ctx.lib.vse_rec_graph_create(self.ctx.handle, bufs["handle"], C.c_void_p(bufs["wsbuf"].data_ptr()),
                                                     C.c_void_p(bufs["x"].data_ptr()), C.c_void_p(bufs["wt"].data_ptr()), prog.out_level,
                                                     C.c_void_p(bufs["idx_maxp"].data_ptr()), n, bufs["tt"], C.c_void_p(bufs["oi"].data_ptr()),
                                                     C.c_void_p(bufs["ol"].data_ptr()), C.c_void_p(bufs["oc"].data_ptr()), self.ctx.stream(),
                                                     C.byref(g)), "vse_rec_graph_create")
            bufs["graph"] = g
        _check(self.ctx.lib.vse_graph_launch(bufs["graph"], self.ctx.stream()), "vse_graph_launch")
        return bufs["oi"].clone(), bufs["ol"].clone(), bufs["oc"].clone()

    def profile(self, x, slot=0, widths=None):
        """Per-op milliseconds (HIP events) for one run; returns (ms ndarray, program, kernel name per op)."""
        n, h, w, _ = x.shape
        self.program(n, h, w)
        prog, handle = self._ensure((n, h, w))
        outs, ptrs = self._ext(prog, x)
        ms = (C.c_float * len(prog.ops))()
        ws = self._workspace((n, h, w), prog, slot)
        wt = self._width_table(prog, widths, n, w)
        self.last_tlen = wt[prog.out_level] if wt is not None else None
        self.last_outs = outs                 # the profiled run's outputs (same values as run())
        _check(self.ctx.lib.vse_plan_profile(handle, C.c_void_p(ws.data_ptr()), ptrs, len(ptrs),
                                             C.c_void_p(wt.data_ptr()) if wt is not None else None, self.ctx.stream(), ms),
               "vse_plan_profile")
        variants = profiled_kernel_names(prog.ops, ms)
        return np.array(ms[:], dtype=np.float32), prog, variants
