"""Exact tests of the MXFP8 kernels on the device: the case table of tests/conv_f8_ref.py (E4M3 integers, E8M0 block scales as part
of the exact data, float64 references; see its docstring) through HipOps.  Every case asserts the dispatch path it exists for
(its guard, dg_last_conv_kernels() == 32, dg_conv3x3_dgrad_launches, dg_last_wgrad_kernel() == 7), compares the destination BIT
FOR BIT with the reference and checks the guards around the destination and the other channels of a slab.
tests/test_conv_f8_exact_cpu.py runs the same table through the CPU oracle.

The first two tests measure what the method rests on and no guide documents: that v_mfma_scale_f32_16x16x128_f8f6f4 (forward /
data gradient) and v_mfma_scale_f32_32x32x64_f8f6f4 (weight gradient) return the exact integer for a chain of E4M3 integers with
power-of-two block scales whose partial sums stay below F8_INT_LIMIT.  Observed: DESIGN.md section 7, "Exact fp8 tests"."""
import pytest

from downgan_amd import ops as ops_mod
from downgan_amd.ops import HipOps
from tests import conv_f8_ref as F
from tests.elementwise_ref import assert_bits

pytestmark = pytest.mark.gpu

_OPS = {}


def hip(case=None):
    gen = case is not None and case.net == "T"
    if gen not in _OPS:
        _OPS[gen] = HipOps("bf16", f8_generator=True) if gen else HipOps("bf16", f8_critic=True)
    return _OPS[gen]


@pytest.mark.parametrize("D", [F.D_DEFAULT, F.D_FAR], ids=["D7", "D40"])
@pytest.mark.parametrize("positive", [False, True], ids=["signed", "one-sign"])
def test_scaled_mfma_integer_chain_is_exact(positive, D):
    """The smallest case with the plain epilogue (first in the file: a failure here is about the instruction or the data budget,
    not about a kernel).  With operands of one sign the sums pass 2^23, where odd integers need all 24 bits of the accumulator;
    D = 40 puts the x scales at 2^-40 and the w scales at 2^40, which only a joint application of the two scales keeps exact."""
    F.run_f8_conv_case(hip, F.BY_ID[F.FIRST], "wide", only="plain", positive=positive, D=D)


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow-exponents", "wide-exponents"])
@pytest.mark.parametrize("positive", [False, True], ids=["signed", "one-sign"])
def test_scaled_mfma_wgrad_chain_is_exact(positive, narrow):
    """The same for the 32x32x64 instruction of wg3w_f8_kernel on the smallest weight-gradient case: exponents within 8 of 127 or
    drawn from [100, 150), signed or one-sign operands.  The one-sign data (120 and odd integers below 16) needs 1024 pixels for
    its sums to pass 2^23 while the products of one MFMA stay inside the 2^14 window within which the instruction adds exactly
    (tests/conv_f8_ref.py, F8_PRODUCT_BITS; 240 instead of 120 over 256 pixels comes back up to 14 units short)."""
    F.run_f8_wgrad_case(hip(), F.WBY_ID[F.FIRST_WGRAD_ONE_SIGN if positive else F.FIRST_WGRAD], positive=positive, narrow=narrow)


@pytest.mark.parametrize("cid,regime", F.PARAMS, ids=[f"{c}-{r}" for c, r in F.PARAMS])
def test_case_is_exact(cid, regime):
    F.run_f8_conv_case(hip, F.BY_ID[cid], regime)


@pytest.mark.parametrize("cid", F.SELFQ)
def test_self_quantised_route_gives_the_same_bits(cid):
    """Without xq= / wq= dg_quant_mxfp8 forms the operands from the dequantised bf16 tensors: lossless on such data, the same bits."""
    for regime in ("wide", "fine"):
        F.run_f8_conv_case(hip, F.BY_ID[cid], regime, only="plain", selfq=True)


@pytest.mark.parametrize("cid", [c.id for c in F.WCASES])
def test_wgrad_case_is_exact(cid):
    F.run_f8_wcase(hip(), F.WBY_ID[cid])


def test_wgrad_split_k_atomics_equal_the_deterministic_workspace():
    """Integer partial sums commute exactly: the split-K atomics and the deterministic-workspace mode of the fp8 weight-gradient
    kernel give the same bits (each of them equal to the reference inside the runner)."""
    case = F.WBY_ID[F.SPLIT_K]
    assert ops_mod._DET["refs"] == 0, "another test left the deterministic mode on"
    plain = hip()
    assert not plain.deterministic
    a = F.run_f8_wgrad_case(plain, case)
    det = HipOps("bf16", f8_critic=True, deterministic=True)
    try:
        assert det.deterministic
        b = F.run_f8_wgrad_case(det, case)
    finally:
        det.close()
    assert not plain.deterministic
    assert_bits(a, b, "atomics vs deterministic workspace")
