"""The compiler packs each conv record's weights for the kernel it expects the library to choose (compiler.lower_conv mirrors
conv_select, csrc/conv_select.hip).  Here the library names its choice for every OP_CONV record of the product's programs
(vse_op_kernel_name: no plan, context or GPU), and the test checks that the choice is the kernel the record was packed for.
CPU only."""
import re

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
