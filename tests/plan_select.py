"""What a plan decides at vse_plan_create about record PAIRS (csrc/conv_select.hip: conv_gap_select, scale_add_select), asked of the
selectors themselves: tests/plan_select_host.cpp includes conv_select.hip, is built once per session for the host alone and prints the
pairs it accepts for a file of records.  The library needs no export for it, and nothing here needs a GPU."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_exe = None


def host_program():
    global _exe
    if _exe is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        out = os.path.join(tempfile.mkdtemp(prefix="plan_select_"), "plan_select_host")
        subprocess.run([hipcc, "--offload-host-only", "-x", "hip", "-O1", "-std=c++17", os.path.join(HERE, "plan_select_host.cpp"), "-o", out],
                       check=True, capture_output=True, text=True)
        _exe = out
    return _exe


def decisions(ops):
    """-> ({conv index: dict(bm, tiles, slots, atomic, off, moved)}, {scale index: 'in0' | 'in1' (the add's residual operand)})."""
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        np.ascontiguousarray(ops).tofile(f.name)
        text = subprocess.run([host_program(), f.name], check=True, capture_output=True, text=True).stdout
    gaps, adds = {}, {}
    for ln in text.splitlines():
        t = ln.split()
        if t[0] == "gap":
            gaps[int(t[1])] = {t[k]: int(t[k + 1]) for k in range(2, len(t), 2)}
        elif t[0] == "scale_add":
            adds[int(t[1])] = t[3]
    return gaps, adds
