"""CPU half of the one-record conv tests (tests/conv_cases.py; the GPU half is tests/test_gpu_conv_ops.py):

  1. every case on the emulator (oracle/ir_emul.py) under the same two checks as on the GPU: the exact run bit for bit — which is the check
     that the dyadic inputs meet their condition — and the real-valued run under op_harness.ratio;
  2. completeness: every instantiation of the CONV_INST / GEMM_INST tables of csrc/conv_*.hip is selected (op_harness.conv_name) by at
     least one case, but for the NOT_REACHED table;
  3. the hand-built records against the compiler's: conv_op reproduces every OP_CONV record of the product programs and of the
     single-conv graphs of tests/test_gpu_nets.py, and conv_pack reproduces its weight stream from the matrix the emulator decodes;
  4. the checks bite: six mutations of what the kernel is handed, not of the reference, must fail;
  5. the weight blob of every product program is byte-identical to the parent commit's (the packers of F_HLSUM, F_DWPRE and F_TAIL2
     were lifted into static methods for conv_pack)."""
import glob
import hashlib
import os
import re

import numpy as np
import pytest

import conv_cases as CC
import op_harness as H
import test_kernel_names as TK
from oracle import ir_emul, net_ref
from test_gpu_nets import CONVS
from vse_amd import compiler, ir

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-subtitle-extractor_amd", "csrc")


# ---- 1. the emulator leg ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(CC.GROUPS))
def test_emulator_matches_fp64_reference(built_lib, group):
    worst, n = 0.0, 0
    for sp in CC.GROUPS[group]():
        assert CC.selected(sp) == sp.expect, (sp.name, "selects", CC.selected(sp), "and was written for", sp.expect)
        r = H.run_case(CC.case(sp), H.run_emulator)
        assert r is not None, sp.name
        worst, n = max(worst, r), n + 1
    print(f"{group}: {n} cases, {len(CC.instantiations(group))} instantiations, worst error / bound {worst:.3f}")
    assert n > 0


@pytest.mark.parametrize("group", sorted(CC.REFUSED))
def test_refused_records_build(built_lib, group):
    """The records the library must refuse (GPU test) are well-formed OP_CONV records; the selector already names the refusals that
    need no launch check."""
    for sp in CC.REFUSED[group]():
        c = CC.case(sp)
        assert c.refused and len(c.runs) == 1 and c.runs[0].ops.dtype == ir.OP_DT and sp.rc < 0
        name = CC.selected(sp)
        assert name == f"(refused: {sp.rc})" or name.startswith("conv_pw_kernel<"), (sp.name, name)     # (conv_pw: launch_conv's own checks)


# ---- 2. completeness ------------------------------------------------------------------------------------------------------------------
NOT_REACHED = {
    "conv_stem_kernel<2, 2, true, true>": "F_U8SRC needs a frame source; bit-identical to the plain stem: test_stem_with_fused_preprocessing_is_bit_identical",
    "conv_stem_kernel<2, 2, false, true>": "F_U8SRC, as above",
    "conv_stem_kernel<1, 1, true, true>": "F_U8SRC, as above",
    "conv_stem_kernel<1, 1, false, true>": "F_U8SRC, as above",
    "conv_head_up2_kernel": "chosen by an environment variable read once per process: test_detector_head_forms_are_identical_and_race_free",
    "conv_c3pool_kernel<128>": "a conv record + the pool record behind it: tests/test_gpu_conv_pool_fusion.py",
    "conv_c3pool_kernel<64>": "a conv record + the pool record behind it: tests/test_gpu_conv_pool_fusion.py",
}


def table_instantiations():
    """The names of the CONV_INST / GEMM_INST entries, as the macros spell them (conv_common.h, conv_gemm.hip)."""
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "conv_*.hip"))):
        src = open(path).read()
        for m in re.finditer(r"^\s*(?:static const ConvInst \w+\[\] = \{)?\s*((?:(?:CONV|GEMM)_INST\(.*?\)\s*,?\s*)+)(?:\};)?\s*$", src, re.M):
            for e in re.finditer(r"CONV_INST\(\s*-?\d+\s*,\s*-?\d+\s*,\s*-?\d+\s*,\s*([A-Za-z_0-9]+(?:<[^>]*>)?)\s*\)", m.group(1)):
                names.add(e.group(1))
            for e in re.finditer(r"GEMM_INST\(\s*\d+\s*,\s*([0-9 ,]+?)\s*\)", m.group(1)):
                names |= {f"conv_gemm_kernel<{e.group(1)}, 1>", f"conv_gemm_kernel<{e.group(1)}, 0>"}
    return names


def test_every_instantiation_is_selected_by_a_case(built_lib):
    table = table_instantiations()
    assert len(table) >= 85 and "conv_col_kernel<9, 64>" in table and "conv_gemm_kernel<256, 192, 8, 2, 64, 2, 0>" in table, len(table)
    assert set(NOT_REACHED) <= table, sorted(set(NOT_REACHED) - table)
    reached = set()
    for group in CC.GROUPS:
        for sp in CC.GROUPS[group]():
            reached.add(CC.selected(sp))
    assert reached <= table, sorted(reached - table)
    assert not reached & set(NOT_REACHED), sorted(reached & set(NOT_REACHED))
    missing = table - reached - set(NOT_REACHED)
    assert not missing, ("no case selects", sorted(missing))


# ---- 3. the hand-built records against the compiler's -----------------------------------------------------------------------------------
def _family(r):
    f = int(r["flags"])
    if f & ir.F_UP2HEAD:
        return "head"
    if f & ir.F_PW:
        return "pw"
    if f & ir.F_COL:
        return "hlsum" if f & ir.F_HLSUM else "col"
    if f & ir.F_PATCH:
        return "patch"
    if f & ir.F_STEM:
        return "stem"
    return "tile32" if f & ir.F_WK32 else "tile64"


def _absent(v):
    return None if int(v["n"]) == 0 else v


def check_conv_records(prog, what):
    """-> the families seen."""
    emu = ir_emul.Emulator(H._StubProgram(prog.ops, prog.weights.array(), 16, False), round_f16=True)
    blob = prog.weights.array()
    seen = set()
    for i, r in enumerate(prog.ops):
        if int(r["kind"]) != ir.OP_CONV:
            continue
        p, f, flags = r["p"], r["f"], int(r["flags"])
        mine = H.conv_op(r["in0"], r["out"], (int(p[0]), int(p[1])), (int(p[2]), int(p[3])), (int(p[4]), int(p[5])), int(p[ir.P_COUT]),
                         int(p[ir.P_KTOT]), int(p[ir.P_CINP]), int(r["w_off"]), int(r["b_off"]), flags=flags, act=int(p[ir.P_ACT]),
                         act2=int(p[ir.P_ACT2]), act_a=f[ir.FS_ACT_A], act_b=f[ir.FS_ACT_B], post_a=f[ir.FS_POST_A], post_b=f[ir.FS_POST_B],
                         inshift=int(p[ir.P_INSHIFT]), res=_absent(r["in1"]), resshift=int(p[ir.P_RESSHIFT]), in2=_absent(r["in2"]),
                         in2shift=int(p[ir.P_IN2SHIFT]), out2=_absent(r["out2"]), aux_off=int(r["aux_off"]), dotact=int(p[ir.P_DOTACT]),
                         pre_b=f[ir.FS_PRE_B], lo_out=int(p[ir.P_LO_OUT]), lo_res=int(p[ir.P_LO_RES]), lo_in=int(p[ir.P_LO_IN]),
                         wl=(int(p[ir.P_WLIN]), int(p[ir.P_WLOUT])))
        for fld in ("kind", "flags", "p", "f", "in0", "in1", "in2", "out", "out2", "w_off", "b_off", "aux_off"):
            assert np.array_equal(r[fld], mine[0][fld]), (what, i, fld, r[fld], mine[0][fld])
        fam = _family(r)
        seen.add(fam)
        if fam == "head":
            continue            # (folded taps: the stream does not determine the 3x3 matrix; Compiler.head_up2_weights is called by conv_pack as it is)
        kh, kw = (1, 1) if flags & ir.F_DWPRE else (int(p[0]), int(p[1]))
        cinp, hilo = int(p[ir.P_CINP]), bool(flags & ir.F_HILO) or fam == "hlsum"
        wmat = emu.conv_wmat(r, kh, kw).astype(np.float64)
        if fam == "stem":
            assert cinp == 8
        ptaps = int(p[ir.P_KTOT]) // CC.rup(cinp, 32) if fam == "patch" else 0
        stream, ktot = H.conv_pack(fam, wmat, kh, kw, cinp, hilo=hilo, ptaps=ptaps)
        assert ktot == int(p[ir.P_KTOT]), (what, i, fam, ktot, int(p[ir.P_KTOT]))
        theirs = blob[int(r["w_off"]):int(r["w_off"]) + stream.nbytes]
        if not hilo:
            assert np.array_equal(theirs, np.ascontiguousarray(stream).view(np.uint8)), (what, i, fam, "the repacked stream differs")
        else:
            # hi + lo: the split of the SUM need not be the compiler's split of the fp64 weight; the sums are compared
            re_emu = ir_emul.Emulator(H._StubProgram(prog.ops[i:i + 1], np.ascontiguousarray(stream).view(np.uint8), 16, False), round_f16=True)
            r0 = r.copy()
            r0["w_off"] = 0
            assert np.array_equal(re_emu.conv_wmat(r0, kh, kw), wmat.astype(np.float32)), (what, i, fam, "hi + lo of the repacked stream differs")
    return seen


def _single_conv_graph(cin, cout, k, s, p):
    desc, w = TK.conv_graph(cin, cout, k, 1, False)
    desc["ops"][2]["attrs"].update(strides=list(s), paddings=list(p))
    return desc, w


def test_conv_records_and_streams_match_the_compiler():
    seen = set()
    for mid in TK.DETECTORS:
        for k, prog in enumerate(TK.det_programs(mid)):
            seen |= check_conv_records(prog, (mid, k))
    for mid, h, w in TK.RECOGNISERS:
        desc, wt = net_ref.get_weights(mid)
        seen |= check_conv_records(compiler.compile_model(desc, wt, 3, h, w, ragged=True), mid)
    for cin, cout, k, s, p, h, w, n in CONVS:
        for hilo in (False, True):
            desc, wt = _single_conv_graph(cin, cout, k, s, p)
            seen |= check_conv_records(compiler.compile_model(desc, wt, n, h, w, hilo=hilo, want_probs=False), ("conv", cin, cout, k, s, h, w, hilo))
    assert seen == {"head", "pw", "hlsum", "col", "patch", "stem", "tile32", "tile64"}, seen


# ---- 4. the checks bite ---------------------------------------------------------------------------------------------------------------
# One case per family and mutation where the mutation means something: a single-tap family has no taps to swap, a family of <= 32 couts no
# rows to swap across a 32-boundary, only ragged cases have a width.  (group, case name): the mutations applied to it.
MUTATED = {
    ("gemm", "gemm0 masked 3x3 s2"): ("taps", "chunk", "cout", "bias"),
    ("gemm", "gemm0 unmasked imgw 2 tiles"): ("chunk", "cout"),
    ("smallm", "smallk 72ch hilo kt64"): ("chunk", "cout", "res", "bias"),
    ("mfma", "mfma Np72 up"): ("taps", "chunk", "cout", "res", "bias"),
    ("patch", "patch 3x3 light 128"): ("taps", "chunk", "cout", "res", "bias"),
    ("patch", "patch 3x3 src2 shift1"): ("taps", "chunk", "cout", "bias"),
    ("patch", "patch 3x3 dot1 f32"): ("taps", "chunk", "cout", "bias"),
    ("col", "col 5x5 up + res"): ("taps", "chunk", "cout", "res", "bias"),
    ("col", "col 5x3 ragged"): ("width",),
    ("c3", "c3 rw8 96 couts"): ("taps", "chunk", "cout", "bias"),
    ("c3", "c3n32 rw4"): ("taps", "res"),
    ("c3", "c3 hlsum"): ("taps", "chunk", "bias"),
    ("c3", "c3 ragged"): ("width", "cout"),
    ("pw", "pw ks3 hilo"): ("chunk", "cout", "bias"),
    ("pw", "pw tail ks4"): ("chunk", "cout", "bias"),
    ("stem", "stem s1 hilo 4ch 40 couts"): ("taps", "chunk", "cout", "bias"),      # (chunk: its one 8-channel chunk)
    ("stem", "stem s2 even map ragged"): ("width",),
    ("dwpw", "dwpw rows ks3 s1"): ("chunk", "cout", "res", "bias"),
    ("dwpw", "dwpw tile ks4 pair"): ("chunk", "cout", "bias"),
    ("head", "head u ld1"): ("taps", "chunk", "cout", "bias"),
    ("epilogue", "ep pw ragged widths OW 1"): ("width", "res"),
    ("epilogue", "ep gemm resshift 1 odd map"): ("res", "taps"),
    ("epilogue", "ep pw pair residual"): ("res",),
}
REAL_MUST_FAIL = ("taps", "chunk", "res")


def _spec(group, name):
    return next(sp for sp in CC.GROUPS[group]() if sp.name == name)


def test_every_family_and_mutation_is_covered():
    fams = {g.split("_")[0] for g in CC.GROUPS}
    assert {g for g, _ in MUTATED} == fams, fams - {g for g, _ in MUTATED}
    for m in CC.MUTATIONS:
        assert any(m in ms for ms in MUTATED.values()), m
    for fam in fams - {"epilogue"}:
        have = set().union(*[ms for (g, _), ms in MUTATED.items() if g == fam])
        want = {"chunk", "bias"} | ({"taps"} if fam not in ("smallm", "pw", "dwpw") else set())      # (1x1 families: one tap)
        assert want <= have, (fam, want - have)


@pytest.mark.parametrize("group,name", sorted(MUTATED))
def test_mutations_fail_the_checks(built_lib, group, name):
    sp = _spec(group, name)
    assert H.run_case(CC.case(sp), H.run_emulator) is not None          # (unmutated: passes)
    for m in MUTATED[(group, name)]:
        for mode in ("exact", "real") if m in REAL_MUST_FAIL else ("exact",):
            mutated = CC.case(sp, mutate=m, modes=(mode,))          # (a mutation that does not apply to the case raises ValueError here)
            with pytest.raises(AssertionError):
                H.run_case(mutated, H.run_emulator)
                print(f"{name}: mutation {m} passed the {mode} run")


# ---- 5. the packer refactor changed no byte -------------------------------------------------------------------------------------------------
# sha256 (first 16 hex digits) of Program.weights.array() at the parent commit: TK.det_programs(mid) in order, and the ragged recogniser
# programs of TK.RECOGNISERS at batch 3.
PARENT_BLOBS = {
    "V2_ch_det": ["651e1562cce03e85", "bb952cd36e57a22e", "651e1562cce03e85", "bb952cd36e57a22e"],
    "V3_ch_det_fast": ["8b1fbb0c71e8ea64", "5551f438ce2c5d6e", "bc43379cf144e65f", "f7de0f005eb64af8"],
    "V4_ch_det": ["01c849d08458f540", "d31a417c0cb6a614", "01c849d08458f540", "d31a417c0cb6a614"],
    "V4_ch_det_fast": ["4cbfa742ba61fd86", "844d97a870015dae", "7f29dbb61d3d7b00", "2593bac741814b44"],
    "V4_ch_rec": ["0c59c8358b82929f"], "V4_en_rec_fast": ["3e992688062430c7"], "V3_ch_rec_fast": ["ccf9956d6a4eb7a7"],
    "V2_ch_rec": ["5a45f4ef8591e7c3"],
}


def _digest(prog):
    return hashlib.sha256(prog.weights.array().tobytes()).hexdigest()[:16]


@pytest.mark.parametrize("mid", sorted(PARENT_BLOBS))
def test_weight_blobs_are_byte_identical_to_the_parent_commit(mid):
    if mid in TK.DETECTORS:
        got = [_digest(p) for p in TK.det_programs(mid)]
    else:
        h, w = next((h, w) for m, h, w in TK.RECOGNISERS if m == mid)
        desc, wt = net_ref.get_weights(mid)
        got = [_digest(compiler.compile_model(desc, wt, 3, h, w, ragged=True))]
    assert got == PARENT_BLOBS[mid], (mid, got)
    progs_with = {"V4_ch_det": "F_TAIL2", "V4_ch_det_fast": "F_DWPRE / F_HLSUM", "V3_ch_det_fast": "F_HLSUM"}
    if mid in progs_with:           # the lifted packers are on the path of these programs
        flags = 0
        for p in TK.det_programs(mid):
            for r in p.ops:
                flags |= int(r["flags"]) if int(r["kind"]) == ir.OP_CONV else 0
        want = {"V4_ch_det": ir.F_TAIL2, "V4_ch_det_fast": ir.F_DWPRE | ir.F_HLSUM, "V3_ch_det_fast": ir.F_HLSUM}[mid]
        assert flags & want == want, (mid, progs_with[mid], hex(flags))
