#!/usr/bin/env python3
"""One sha256 per compiled program, to show that a compiler change leaves the programs as they were: run it on two revisions and
compare the outputs line for line.  Pure compile (numpy): no library, context or GPU.

usage: python tools/program_digest.py [--skip-4k] [--skip-grid]

A digest covers the bytes of Program.ops, the weight blob of the WeightStore the program was compiled into, and ws_bytes, outputs,
wlevels, names and op_gmacs.  Configurations: the product's detector programs at 64 x 544 x 960 (tests/test_kernel_names.py
det_programs: chain None / False, normalised input / raw frames), the server detector at 32 x 2176 x 3840, every recogniser as a
ragged plan and again at a wider width through the SAME store (the weight cache keys), and the single-conv grids of
tests/test_kernel_names.py (grid_cases, dot1_cases)."""
import hashlib
import itertools
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import net_ref
from tests import test_kernel_names as tk
from vse_amd import compiler


def digest(prog, store=None):
    h = hashlib.sha256()
    h.update(prog.ops.tobytes())
    h.update(bytes((store or prog.weights).blob))
    meta = [prog.ws_bytes, prog.outputs, prog.wlevels, prog.names, [repr(float(g)) for g in prog.op_gmacs]]
    h.update(json.dumps(meta, sort_keys=True, default=str).encode())
    return h.hexdigest()


def main():
    total = hashlib.sha256()

    def show(label, prog, store=None):
        d = digest(prog, store)
        total.update(d.encode())
        print(f"{d}  {label}", flush=True)
    for mid in tk.DETECTORS:
        for n, prog in enumerate(tk.det_programs(mid)):
            show(f"{mid} 64x544x960 chain={(None, False)[n // 2]} raw_frames={bool(n % 2)}", prog)
    if "--skip-4k" not in sys.argv:
        desc, w = net_ref.get_weights("V4_ch_det")
        show("V4_ch_det 32x2176x3840", compiler.compile_model(desc, w, 32, 2176, 3840))
    for mid, h, wmax in tk.RECOGNISERS:
        desc, w = net_ref.get_weights(mid)
        store = compiler.WeightStore()
        for width in (wmax, 2 * wmax + 37):
            show(f"{mid} ragged 3x{h}x{width}", compiler.compile_model(desc, w, 3, h, width, ragged=True, store=store), store)
    if "--skip-grid" not in sys.argv:
        for case in itertools.chain(tk.grid_cases(), tk.dot1_cases()):
            show("grid " + tk.case_id(case), tk.compile_case(case))
    print(f"{total.hexdigest()}  all of the above")


if __name__ == "__main__":
    main()
