"""Every kernel that launch_simple_op (csrc/simple_ops.hip) dispatches, and csrc/lstm.hip, ALONE: a one-record plan on seeded tensors
(tests/op_harness.py) against a plain fp64 reference of the same operation, at the shapes where these kernels can go wrong — vector and
tile tails, more than one block, the thresholds between two kernel forms, ragged widths — under the bound of op_harness.ratio:

    fp16 output: |got - ref64| <= ulp16(|ref64|) + 8 e32        fp32 output: |got - ref64| <= 16 ulp32(|ref64|) + 8 e32

(e32 = the distance of a plain float32 evaluation of the reference from its float64 evaluation, measured at test time).  Bit-exact: max
pool, resize / copy, the zeros right of a sample's width, the soft-max arg-max, batch independence.  The cases are tests/op_cases.py;
tests/test_op_records.py runs the same records on the CPU emulator under the same bound.

Worst error / bound per op, measured on MI355X (the emulator's figure beside it; 0.5 = half a unit of the stored format, a correctly
rounded result):

    op (groups of tests/op_cases.py)                                          cases   MI355X   emulator
    class soft-max, 13 (esize, ncls, ld) x with / without probabilities         26     0.079     0.167
    layer norm, C 8 / 64 / 120 / 128                                            68     0.499     0.499
    attention, (8,15) (8,16) (4,8), T 1 .. 300, ragged; T 513 and 1280          23     0.497     0.497
    LSTM, MFMA form, modes 0 / 1 / 2                                            51     0.499     0.499
    LSTM, scalar form, H 48 / 96 / 256                                          12     0.499     0.499
    depthwise conv, column-walk form, k 3 / 5 x sh 1 / 2                       104     0.499     0.499
    depthwise conv, row form (sw 2, gates, hi + lo pairs, kh != kw)             14     0.498     0.498
    depthwise conv, generic form (kw 1, kw 7)                                    4     0.498     0.498
    average pooling (max pooling: bit-exact, 24 cases)                          44     0.500     0.500
    global average pooling, split and row forms                                 30     0.500     0.500
    element-wise kernels (scale, binary, resize, unary, wscale)                 27     0.500     0.500

No op needs more than the rule.  The fp16 outputs sit at 0.5 because the ulp term allows a full fp16 step and a correctly rounded result is
half a step off: what the kernels add on top (summation order, __expf, rsqrtf, the hi + lo state of the MFMA LSTM) is below a thousandth
of the bound at these shapes.  The soft-max outputs are fp32, where the figure is the arithmetic itself: 0.03 - 0.08 of 16 ulps + 8 e32.

Attention above 64 KiB of dynamic LDS: T = 513 (65 664 bytes) and T = 1280 (160 KiB, the largest the launcher accepts) launch as the
launcher stands — it does not raise the function's dynamic-LDS limit and the HIP runtime does not ask for it on gfx950 — and match the
reference (0.486); T = 1281 is refused with VSE_E_UNSUPPORTED.

The whole file: 40 tests, 5.0 s on one MI355X (the slowest, the two-direction MFMA LSTM group, 0.7 s).
"""
import pytest

import op_cases
import op_harness as H

pytestmark = pytest.mark.gpu


def _runner(ctx):
    return lambda ops, blob, tensors, widths, ws_bytes: H.run_gpu(ctx, ops, blob, tensors, widths, ws_bytes)


@pytest.mark.parametrize("group", sorted(op_cases.GROUPS))
def test_kernel_matches_fp64_reference(ctx, group):
    worst, n, notes = 0.0, 0, []
    for case in op_cases.GROUPS[group]():
        r = H.run_case(case, _runner(ctx))
        if r is None:                       # (attention-lds only: refused with VSE_E_UNSUPPORTED)
            assert case.may_refuse and case.note["rc"] == H.VSE_E_UNSUPPORTED, (case.name, case.note)
            notes.append(f"{case.name}: refused, rc={case.note['rc']}")
            continue
        worst, n = max(worst, r), n + 1
    print(f"{group}: {n} cases, worst error / bound {worst:.3f}" + "".join("; " + s for s in notes))
    assert n > 0 or notes


@pytest.mark.parametrize("group", sorted(op_cases.REFUSED))
def test_unsupported_records_are_refused(ctx, group):
    """C = 136 layer norm, head dim 32, T = 1281 attention, a 512-unit scalar LSTM: a negative code, no launch."""
    for case in op_cases.REFUSED[group]():
        assert H.run_case(case, _runner(ctx)) is None
        assert case.note["rc"] < 0, (case.name, case.note)
        print(f"{case.name}: rc={case.note['rc']}")
