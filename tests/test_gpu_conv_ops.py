"""Every conv kernel instantiation ALONE (the CONV_INST / GEMM_INST tables of csrc/conv_*.hip): a one-record OP_CONV plan (tests/op_harness.py:
conv_op, conv_pack, ref_conv) against a plain fp64 reference of the whole record, at the smallest shapes that reach each instantiation and
each branch of conv_epilogue_tile (tests/conv_cases.py).  Two runs per case:

    exact   dyadic inputs and sparse weights whose every partial sum is exact in fp32: got == float16(ref64) / float32(ref64) BIT FOR BIT
    real    seeded normal inputs, nonlinear activations, under op_harness.ratio:
            fp16 output: |got - ref64| <= ulp16(|ref64|) + 8 e32      fp32 output: 16 ulp32 + 8 e32      pair output: 2^-20 |ref64| + 2^-24 + 8 e32
            e32 = the larger of two float32 evaluations of ref_conv against float64: numpy's, and one strictly sequential over taps and
            16-channel chunks (op_harness.conv_reference)

Each case asserts the instantiation the library names for its record (vse_op_kernel_name).  tests/test_conv_records.py runs the same cases on
the CPU emulator, proves that every instantiation but its NOT_REACHED table has a case, and that six mutations fail these checks.

Worst error / bound of the real run per group, measured on MI355X (the emulator's figure beside it; 0.5 = half an fp16 step, a correctly rounded
result; the exact runs are bit-identical on both):

    group (tests/conv_cases.py GROUPS)                                         cases  instantiations   MI355X   emulator
    gemm       configurations 0 / 1 / 2, masked and unmasked, F_HILO, F_IMGW     11         6          0.499     0.499
    gemm_m65k  configuration 3 (65 536 pixels)                                    2         2          0.498     0.498
    gemm_n192  configurations 5 / 7 (49 152 pixels, 129 .. 192 couts)             4         4          0.498     0.498
    gemm_n256  configurations 4 / 6 (49 152 pixels, 193 .. 256 couts)             4         4          0.497     0.497
    smallm     conv_smallm(_hl)_kernel<32 | 64>, the 4096-tile boundary           8         4 + 1      0.499     0.499
    mfma       three tiles x inshift 0 / 1                                        8         6          0.499     0.500
    patch      six instantiations, F_SRC2, F_DOT1                                14         6          0.499     0.499
    col        <9 | 7 | 5, 64 | 32>, packed and ragged batches                    8         6          0.497     0.497
    c3         conv_c3 / conv_c3n32, rw 8 / 4 / 2, F_HILO, F_HLSUM, ragged       14         6          0.498     0.499
    pw         ks 1 .. 4, hi + lo 1 .. 6, pixel shuffle, F_ONECH, F_TAIL2        16        12          0.499     0.499
    stem       the four instantiations without F_U8SRC                            5         4          0.498     0.498
    dwpw       tile form ks 1 .. 6 x plain / pair, row form ks 1 .. 3 x s 1 / 2  19        18          0.498     0.498
    head       conv_head_up2r_kernel, u at ld 1 / 8, half-empty column tile       3         1          0.499     0.499
    epilogue   18 branches of conv_epilogue_tile on conv_pw and conv_gemm        36         2          0.499     0.499

The unmasked forms of conv_gemm_kernel's 32-deep configurations 4 and 5 are reachable, and stay in kGemmInst: the selector's `Kp % 64` test
lies behind the F_IMGW branch, which takes the unmasked mode alone, so per-image weights with Kp = cinp = 96 select them ("gemm5 / gemm4
unmasked imgw K96").  No compiled program does (P_KTOT is a multiple of 64).  A 5x5 filter's 16-row patch has 720 pixels: it runs on
conv_patch_kernel<16, 64, 1>, and <16, 64, 0> is reached by a 3x3 with a second source or a fused projection.

Every case passes on MI355X and on the emulator: this suite found no wrong kernel.  No family needs more than the rule, and the factor 8 on
e32 is not what holds them: over these cases (K up to 12 544, outputs up to 8 in magnitude) e32 is 9e-8 .. 4e-6, median 7e-7, against
fp16 steps of 5e-4 .. 4e-3, so the figures are the rounding of the stored fp16 value (0.5) and what a kernel's summation order adds is
below a hundredth of the bound; the fp32 and pair outputs (F_ONECH 0.035, P_LO_OUT 0.098 of their bounds) measure the arithmetic itself.
What finds a wrong tap, chunk, cout tile or pixel is the exact run, with no tolerance at all.

The whole file: 15 tests, 10.9 s on one MI355X (the slowest, the 256-cout big-M group, 3.1 s — most of it the float64 and float32
references of four 49 152-pixel x 256-cout outputs on the CPU).
"""
import pytest

import conv_cases as CC
import op_harness as H

pytestmark = pytest.mark.gpu


def _runner(ctx):
    return lambda ops, blob, tensors, widths, ws_bytes: H.run_gpu(ctx, ops, blob, tensors, widths, ws_bytes)


@pytest.mark.parametrize("group", sorted(CC.GROUPS))
def test_conv_kernel_matches_fp64_reference(ctx, group):
    worst, n, failed = 0.0, 0, []
    for sp in CC.GROUPS[group]():
        name = CC.selected(sp)
        assert name == sp.expect, (sp.name, "selects", name, "and was written for", sp.expect)
        try:
            r = H.run_case(CC.case(sp), _runner(ctx))
        except AssertionError as e:             # (every case of the group runs: the list says which kernels are wrong, and by how much)
            failed.append(f"{sp.name} [{name}]: {e}")
            continue
        assert r is not None, sp.name
        print(f"  {sp.name} [{name}]: {r:.3f}")
        worst, n = max(worst, r), n + 1
    print(f"{group}: {n} cases, {len(CC.instantiations(group))} instantiations, worst error / bound {worst:.3f}")
    assert not failed, "\n".join(failed)
    assert n > 0


@pytest.mark.parametrize("group", sorted(CC.REFUSED))
def test_malformed_conv_records_are_refused(ctx, group):
    """Each record is well-formed but for one property: the code the library must answer, and no launch."""
    for sp in CC.REFUSED[group]():
        case = CC.case(sp)
        assert H.run_case(case, _runner(ctx)) is None
        assert case.note["rc"] == sp.rc, (sp.name, case.note, sp.rc)
        print(f"{sp.name}: rc={case.note['rc']}")
