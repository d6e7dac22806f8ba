"""The compiler packs each conv record's weights for the kernel it expects the library to choose: conv_route.route_conv decides the
family, and the helpers of conv_route.py restate the rules of conv_select (csrc/conv_select.hip) that packing and flags depend on.
Here the library names its choice for every OP_CONV record (vse_op_kernel_name: no plan, context or GPU), and the test checks that
the choice is the kernel the record was packed for: over the product's programs, and over a grid of single-conv graphs that reaches
every conv kernel family beyond the shapes the product compiles.  CPU only."""
import itertools
import re

import numpy as np

import pytest

from oracle import net_ref
from vse_amd import compiler, engine, ir, pipeline

DETECTORS = ["V2_ch_det", "V3_ch_det_fast", "V4_ch_det", "V4_ch_det_fast"]
RECOGNISERS = [("V4_ch_rec", 48, 131), ("V4_en_rec_fast", 48, 160), ("V3_ch_rec_fast", 48, 123), ("V2_ch_rec", 32, 101)]


def rup(x, m):
    return (x + m - 1) // m * m


def det_programs(mid):
    """The detector programs OcrPipeline builds at 544 x 960, batch 64: its weight mode (hi + lo pairs for the fast models), with the
    1x1 / depthwise chains on and off, on normalised input and on raw frames (input_norm + fuse_preprocess)."""
    desc, w = net_ref.get_weights(mid)
    hilo = pipeline.resolve_det_weights("auto", w) == "fp16x2"
    for chain in (None, False):
        yield compiler.compile_model(desc, w, 64, 544, 960, hilo=hilo, chain=chain)
        yield compiler.compile_model(desc, w, 64, 544, 960, hilo=hilo, chain=chain, input_norm=pipeline.DET_NORM, fuse_preprocess=True)


def check_conv_names(prog):
    names = engine.op_kernel_names(prog.ops)
    assert len(names) == len(prog.ops)
    nconv = 0
    for o, name in zip(prog.ops, names):
        if int(o["kind"]) != ir.OP_CONV:
            assert name and not name.startswith("conv_"), name
            continue
        nconv += 1
        f, p = int(o["flags"]), o["p"]
        kh, kw, cinp, coutp = int(p[ir.P_KH]), int(p[ir.P_KW]), int(p[ir.P_CINP]), int(p[ir.P_COUT])
        tf = lambda flag: "true" if f & flag else "false"          # noqa: E731
        assert not name.startswith("(refused"), (name, f, list(p))
        if f & ir.F_UP2HEAD:
            assert name in ("conv_head_up2r_kernel", "conv_head_up2_kernel"), name
        elif f & ir.F_STEM:
            s = int(p[ir.P_SH])
            assert name == f"conv_stem_kernel<{s}, {s}, {tf(ir.F_HILO)}, {tf(ir.F_U8SRC)}>", name
        elif f & ir.F_DWPRE:
            assert name.startswith(("conv_dwpw_rows_kernel<", "conv_dwpw_kernel<")), name
        elif f & ir.F_PW:
            if f & ir.F_TAIL2:
                assert name == f"conv_pw_tail_kernel<{-(-cinp // 16)}>", name
            else:
                assert name == f"conv_pw_kernel<{-(-cinp // 16)}, {tf(ir.F_HILO)}>", name
        elif f & ir.F_COL and (kh, kw) == (3, 3):
            n32 = coutp <= 32 and not f & ir.F_HLSUM
            assert re.fullmatch(r"conv_c3%s_kernel<\d, \d>" % ("n32" if n32 else ""), name), name
        elif f & ir.F_COL:
            assert name.startswith(f"conv_col_kernel<{kh}, "), name
        elif f & ir.F_PATCH:
            m = re.fullmatch(r"conv_patch_kernel<(\d+), (\d+), (\d)>", name)
            assert m, name
            th, bn, mode = map(int, m.groups())
            assert int(p[ir.P_KTOT]) // rup(cinp, 32) == rup(kh * kw, 2 if mode == 2 else 4), (name, kh, kw, int(p[ir.P_KTOT]))
            if f & ir.F_DOT1:
                assert th == 16 and bn >= coutp, name
        if f & ir.F_WK32:          # 32-deep weight tiles: conv_gemm_kernel reads them at either K depth (it tests the flag)
            assert re.fullmatch(r"conv_gemm_kernel<(\d+, ){6}\d>|conv_smallm(_hl)?_kernel<32>", name), name
    assert nconv > 0
    return names


@pytest.mark.parametrize("mid", DETECTORS)
def test_detector_conv_records_name_the_kernel_they_were_packed_for(built_lib, mid):
    for prog in det_programs(mid):
        check_conv_names(prog)


def test_server_detector_at_4k_names_its_kernels(built_lib):
    desc, w = net_ref.get_weights("V4_ch_det")
    check_conv_names(compiler.compile_model(desc, w, 32, 2176, 3840))


@pytest.mark.parametrize("mid,h,wmax", RECOGNISERS)
def test_ragged_recogniser_conv_records_name_their_kernels(built_lib, mid, h, wmax):
    desc, w = net_ref.get_weights(mid)
    check_conv_names(compiler.compile_model(desc, w, 3, h, wmax, ragged=True))


# ---- single-conv graphs: a 1x1 lift of the 3-channel feed to `cin`, then the conv under test (the graph of tools/bench_conv.py) ----
GRID_K = [(1, 1), (3, 3), (5, 5), (7, 7), (9, 9), (1, 5), (5, 1), (3, 7)]
GRID_CIN = [8, 16, 24, 32, 64, 128]
GRID_COUT = [8, 64, 72, 192, 224]
GRID_HW = [(17, 30), (68, 120), (136, 240), (16, 32), (48, 33)]
# every instantiation of conv_patch_kernel, and every other conv kernel family up to its template arguments
GRID_MUST_REACH = {"conv_patch_kernel<8, 64, 0>", "conv_patch_kernel<8, 64, 2>", "conv_patch_kernel<8, 128, 2>", "conv_patch_kernel<16, 64, 0>",
                   "conv_patch_kernel<16, 64, 1>", "conv_patch_kernel<16, 32, 1>", "conv_c3_kernel", "conv_c3n32_kernel", "conv_col_kernel",
                   "conv_gemm_kernel", "conv_mfma_kernel", "conv_smallm_kernel", "conv_smallm_hl_kernel", "conv_pw_kernel"}


def grid_cases():
    """(k, cin, cout, (h, w), hilo, stride, dot1): 'same' padding; stride 2 for the 1x1 and 3x3 filters too."""
    for k, cin, cout, hw, hilo in itertools.product(GRID_K, GRID_CIN, GRID_COUT, GRID_HW, (False, True)):
        for s in ((1, 2) if k in ((1, 1), (3, 3)) else (1,)):
            yield k, cin, cout, hw, hilo, s, False


def dot1_cases():
    """The conv under test in front of a 1x1 conv to ONE channel + sigmoid (the DB head's form), which conv_patch_kernel may fuse."""
    for k, cin, cout, hw, hilo in itertools.product([(3, 3), (5, 5), (9, 9), (1, 5)], [32, 128], [24, 64, 72],
                                                    [(17, 30), (136, 240), (16, 32)], (False, True)):
        yield k, cin, cout, hw, hilo, 1, True


def case_id(case):
    k, cin, cout, hw, hilo, s, dot1 = case
    return f"{k[0]}x{k[1]} s{s} {cin}->{cout} @{hw[0]}x{hw[1]}{' hilo' if hilo else ''}{' dot1' if dot1 else ''}"


def conv_graph(cin, cout, k, s, dot1):
    ops = [{"type": "feed", "in": {"X": ["feed"]}, "out": {"Out": ["x"]}, "attrs": {"col": 0}},
           {"type": "conv2d", "in": {"Input": ["x"], "Filter": ["w0"]}, "out": {"Output": ["t0"]},
            "attrs": {"strides": [1, 1], "paddings": [0, 0], "groups": 1}},
           {"type": "conv2d", "in": {"Input": ["t0"], "Filter": ["w1"]}, "out": {"Output": ["t1"]},
            "attrs": {"strides": [s, s], "paddings": [k[0] // 2, k[1] // 2], "groups": 1}},
           {"type": "elementwise_add", "in": {"X": ["t1"], "Y": ["b1"]}, "out": {"Out": ["t2"]}, "attrs": {"axis": 1}},
           {"type": "relu", "in": {"X": ["t2"]}, "out": {"Out": ["t3"]}, "attrs": {}}]
    params = {"w0": (cin, 3, 1, 1), "w1": (cout, cin, k[0], k[1]), "b1": (cout,)}
    shapes = {"t0": [-1, cin, -1, -1], "t1": [-1, cout, -1, -1]}
    last = "t3"
    if dot1:
        ops += [{"type": "conv2d", "in": {"Input": ["t3"], "Filter": ["w2"]}, "out": {"Output": ["t4"]},
                 "attrs": {"strides": [1, 1], "paddings": [0, 0], "groups": 1}},
                {"type": "sigmoid", "in": {"X": ["t4"]}, "out": {"Out": ["t5"]}, "attrs": {}}]
        params["w2"] = (1, cout, 1, 1)
        shapes.update({"t3": [-1, cout, -1, -1], "t4": [-1, 1, -1, -1]})
        last = "t5"
    ops.append({"type": "fetch", "in": {"X": [last]}, "out": {"Out": ["fetch"]}, "attrs": {"col": 0}})
    rng = np.random.default_rng(1)
    desc = {"model": "unit", "ops": ops, "params": {n: {"dims": list(d), "dtype": 5} for n, d in params.items()}, "var_shapes": shapes}
    return desc, {n: (rng.standard_normal(d) / np.sqrt(np.prod(d[1:]))).astype(np.float32) for n, d in params.items()}


def compile_case(case):
    k, cin, cout, hw, hilo, s, dot1 = case
    desc, w = conv_graph(cin, cout, k, s, dot1)
    return compiler.compile_model(desc, w, 2, hw[0], hw[1], hilo=hilo, want_probs=False)


def test_single_conv_grid_names_the_kernel_each_record_was_packed_for(built_lib):
    """3 000 compiles at batch 2: 19 s measured on one CPU core.  The full grid this one is cut from (cin also 96 and 256, cout also 24, 32 and 128,
    maps also 34x60, 12x256, 6x192, 3x192 and 40x70: 12 800 compiles) reaches the same 44 kernel instantiations.  A grid that reaches fewer families
    than GRID_MUST_REACH fails."""
    reached = set()
    for case in grid_cases():
        name = check_conv_names(compile_case(case))[1]
        reached |= {name, name.split("<")[0]}
    assert GRID_MUST_REACH <= reached, sorted(GRID_MUST_REACH - reached)


def test_fused_projection_is_flagged_only_where_the_library_picks_16_row_tiles(built_lib):
    """F_DOT1 off the product path: check_conv_names asserts th == 16 and one cout tile for every fused record; here both outcomes must
    occur, the projection fused into a patch conv and left as its own launch behind one."""
    fused = unfused = 0
    for case in dot1_cases():
        prog = compile_case(case)
        check_conv_names(prog)
        f = int(prog.ops[1]["flags"])
        fused += bool(f & ir.F_DOT1)
        unfused += bool(f & ir.F_PATCH and not f & ir.F_DOT1)
        assert (len(prog.ops) == 2) == bool(f & ir.F_DOT1), (case_id(case), len(prog.ops))       # fused: no launch of its own
    assert fused and unfused, (fused, unfused)
