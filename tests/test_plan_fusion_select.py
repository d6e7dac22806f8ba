"""The pairs of records a plan runs as one pass, counted over the product's programs (CPU only; tests/plan_select.py asks the
selectors of csrc/conv_select.hip through a host program):

  * conv_gap_select: a 1x1 conv of conv_gemm_kernel's unmasked form sums the partials of the global-average pool behind it.  The server
    detector (V4_ch_det, 64 x 544 x 960) has five such pairs, its stage-end aggregation convs, records 10, 20, 30, 40 and 52, all on
    the 256 x 256 tile, each with at most two row tiles per slot.  The compiler lays the pool's scratch of records 21, 31 and 53 over the
    conv's own INPUT (dead behind the conv in the unfused program): those three keep their partials in other dead workspace bytes.
  * scale_add_select: the gate multiply + residual add at the end of the second stage-3 block, records 43 -> 44, of the server detector
    and of the server recogniser (V4_ch_rec, ragged), once each.
  * The mobile detectors (V2_ch_det: no pool; V3_ch_det_fast: 8 pools, V4_ch_det_fast: 10) and the other recognisers give NO pair of either
    kind: their SE convs are depthwise / pointwise kernels or conv_smallm_kernel, never conv_gemm_kernel, and their gate multiplies carry
    F_RES or feed a depthwise conv."""
import numpy as np
import pytest

import plan_select
from oracle import net_ref
from test_kernel_names import DETECTORS, RECOGNISERS, det_programs
from vse_amd import compiler, ir


def kinds(prog, kind):
    return [i for i, o in enumerate(prog.ops) if int(o["kind"]) == kind]


@pytest.mark.parametrize("mid", DETECTORS)
def test_detector_pairs(built_lib, mid):
    for prog in det_programs(mid):
        gaps, adds = plan_select.decisions(prog.ops)
        pools = kinds(prog, ir.OP_GAP)
        print(mid, len(prog.ops), "records,", len(pools), "pools:", gaps, adds)
        if mid != "V4_ch_det":
            assert not gaps and not adds
            assert len(pools) == {"V2_ch_det": 0, "V3_ch_det_fast": 8, "V4_ch_det_fast": 10}[mid]
            continue
        assert sorted(gaps) == [10, 20, 30, 40, 52] == [i - 1 for i in pools]
        assert [gaps[i]["tiles"] for i in sorted(gaps)] == [128, 32, 8, 8, 2]
        assert [gaps[i]["slots"] for i in sorted(gaps)] == [64, 31, 7, 7, 1]
        assert all(g["bm"] == 256 and g["atomic"] == 1 for g in gaps.values())
        assert [gaps[i]["moved"] for i in sorted(gaps)] == [0, 1, 1, 0, 1]
        assert adds == {43: "in1"}
        for i, g in gaps.items():
            # wherever the partials go, they lie in the workspace and apart from everything the pair touches
            c, q = prog.ops[i], prog.ops[i + 1]
            nbytes = int(q["in2"]["n"]) * int(q["in2"]["h"]) * int(q["in2"]["c"]) * 4
            lo, hi = g["off"], g["off"] + nbytes
            assert 0 <= lo and hi <= prog.ws_bytes and lo % 16 == 0
            for v in (c["in0"], c["out"], q["out"]):
                a = int(v["off"])
                b = a + ((int(v["n"]) * int(v["h"]) * int(v["w"]) - 1) * int(v["ld"]) + int(v["c"])) * int(v["esize"])
                assert b <= lo or hi <= a, (i, lo, hi, a, b)


def test_server_detector_at_4k(built_lib):
    """32 x 2176 x 3840: stage 1's map has 522 240 pixels, 2 040 row tiles for 64 slots, so that pair stays two launches."""
    desc, w = net_ref.get_weights("V4_ch_det")
    prog = compiler.compile_model(desc, w, 32, 2176, 3840)
    gaps, adds = plan_select.decisions(prog.ops)
    pools = kinds(prog, ir.OP_GAP)
    print(gaps, adds)
    assert len(pools) == 5 and pools[0] - 1 not in gaps
    assert all(g["tiles"] <= 2 * g["slots"] for g in gaps.values())
    assert len(adds) == 1


@pytest.mark.parametrize("mid,h,wmax", RECOGNISERS)
def test_ragged_recogniser_pairs(built_lib, mid, h, wmax):
    desc, w = net_ref.get_weights(mid)
    prog = compiler.compile_model(desc, w, 3, h, wmax, ragged=True)
    gaps, adds = plan_select.decisions(prog.ops)
    print(mid, len(kinds(prog, ir.OP_GAP)), "pools:", gaps, adds)
    assert not gaps                                   # ragged pools sum row by row (gap_rows_kernel)
    assert adds == ({43: "in1"} if mid == "V4_ch_rec" else {})
    if adds:
        s, b = prog.ops[43], prog.ops[44]
        assert int(s["kind"]) == ir.OP_SCALE and int(b["kind"]) == ir.OP_BINARY and np.array_equal(s["out"], b["in0"])
