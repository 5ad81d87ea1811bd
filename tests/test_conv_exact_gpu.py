"""Exact tests of the MFMA kernels on the device: the case table of tests/conv_ref.py (integer operands, float64 references, see
its docstring) through HipOps.  Every case asserts the dispatch path it exists for (its guard and the library's probes), compares
the destination BIT FOR BIT with the reference, and checks the guards around the destination and the other channels of a slab.
tests/test_conv_exact_cpu.py runs the same table through the CPU oracle."""
import pytest

from downgan_amd import ops as ops_mod
from downgan_amd.ops import HipOps
from tests import conv_ref as R
from tests.elementwise_ref import assert_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("positive", [False, True], ids=["signed", "one-sign"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_integer_mfma_chain_is_exact(dtype, positive):
    """The assumption everything below rests on, on the smallest halo case with the plain epilogue: an MFMA chain whose operands
    and partial sums are integers below 2^24 returns that integer (first in the file: a failure here is about the hardware
    assumption or the data budget, not about a kernel).  With operands of one sign the fp32 sums pass 2^23, where odd integers
    need all 24 bits of the accumulator."""
    R.run_conv_case(HipOps(dtype), R.BY_ID[R.FIRST], dtype, only="plain", positive=positive)


@pytest.mark.parametrize("cid,dtype", R.PARAMS, ids=[f"{c}-{d}" for c, d in R.PARAMS])
def test_case_is_exact(cid, dtype):
    R.run_case(HipOps(dtype), R.BY_ID[cid], dtype)


def test_wgrad_split_k_atomics_equal_the_deterministic_workspace():
    """Integer partial sums commute exactly: the split-K atomics and the deterministic-workspace mode of the wide weight-gradient
    kernel give the same bits (each of them equal to the reference inside run_case)."""
    case = R.BY_ID["wgrad-wide-320-192-16x64"]
    assert ops_mod._DET["refs"] == 0, "another test left the deterministic mode on"
    plain = HipOps("bf16")
    assert not plain.deterministic
    a = R.run_case(plain, case, "bf16")
    det = HipOps("bf16", deterministic=True)
    try:
        assert det.deterministic
        b = R.run_case(det, case, "bf16")
    finally:
        det.close()
    assert not plain.deterministic
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert_bits(x, y, "atomics vs deterministic workspace")


def test_mask_c0_is_refused_behind_a_pixel_shuffle():
    """The kernels compare the packed GEMM column with mask_c0, which is not the channel of a pixel-shuffled destination: the
    library refuses the combination (dg_epilogue) instead of masking other channels than the oracle."""
    hip = HipOps("bf16")
    cv = R.Conv(1, 8, 8, 128, 256, 1, True)
    y = hip.zeros(*hip.out_shape(cv))
    with pytest.raises(RuntimeError, match="DG_ERR_BAD_SHAPE"):
        hip.conv_fwd(cv, hip.zeros(1, 8, 8, 128), hip.zeros(256 * 9 * 128), y, mask=hip.zeros(*y.shape), mask_slope=0.25, mask_c0=16)
    hip.conv_fwd(cv, hip.zeros(1, 8, 8, 128), hip.zeros(256 * 9 * 128), y, mask=hip.zeros(*y.shape), mask_slope=0.25)
