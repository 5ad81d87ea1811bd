"""The exact-test case table of tests/conv_ref.py through the CPU oracle (oracle/emu_ops.py): every case must be bit-equal between
EmuOps and the float64 references, and every integer budget must hold.  That validates the references, the data and the case
guards without a GPU, and pins the oracle itself bit for bit.  The mutation checks at the end prove that the comparator notices a
one-unit error at a border pixel and two swapped weight taps, and that it names the pixel."""
import re

import pytest
import torch

from oracle.emu_ops import EmuOps
from tests import conv_ref as R


@pytest.mark.parametrize("cid,dtype", R.PARAMS, ids=[f"{c}-{d}" for c, d in R.PARAMS])
def test_case_is_exact_on_the_oracle(cid, dtype):
    R.run_case(EmuOps(dtype), R.BY_ID[cid], dtype)


def test_every_path_of_the_table_has_a_case():
    """Each dispatch path the tests name is reached by at least one case (its guard asserts that the case really takes it); the
    "f8" entries belong to the table of tests/conv_f8_ref.py, which must reach every fp8 path and both fp8 weight-gradient entries."""
    from tests import conv_f8_ref as F
    seen = set()
    for c in R.CASES:
        seen |= set(c.expect.values()) if isinstance(c.expect, dict) else {c.expect}
    assert "f8" not in seen
    assert set(R.PATH_BITS) - {"f8"} <= seen and set(R.WGRAD_CODE) - {"f8"} <= seen and {"dx_narrow", "dx_wide"} <= seen
    assert {c.expect for c in F.CASES} == set(F.F8_PATHS) and {c.kind for c in F.WCASES} == {"wgrad", "dense"}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_sign_data_reaches_the_budget(dtype):
    """The data of the device's first test: exact on the oracle, and in fp32 its sums pass 2^23 and include odd integers."""
    case = R.BY_ID[R.FIRST]
    R.run_conv_case(EmuOps(dtype), case, dtype, only="plain", positive=True)
    acc = R.conv_data(case, dtype, ["plain"], positive=True)[3]
    assert float(acc.abs().max()) < 2 ** 24
    if dtype == "f32":
        big = acc[acc.abs() > 2 ** 23]
        assert big.numel() > 100 and bool((big % 2 == 1).any())


def test_budget_is_asserted():
    with pytest.raises(AssertionError):
        R.int_operands(9 * 1024, 3, "f32", preload=1 << 24)
    assert R.int_operands(9 * 128, 3, "f32") >= 2047 and R.int_operands(9 * 128, 3, "bf16") == 127
    m = R.int_operands(9 * 128, 3, "bf16", bias=64, residuals=128, preload=64, f=6)
    assert m * 3 * 9 * 128 + 256 < 2 ** 18 and (m + 1) * 3 * 9 * 128 + 256 >= 2 ** 18
    with pytest.raises(AssertionError):
        R.ints((4,), 128, torch.Generator().manual_seed(0), "bf16")


def test_pack_bits_is_the_documented_packing():
    pos = torch.zeros(1, 1, 1, 128, dtype=torch.bool)
    pos[..., 0] = pos[..., 15] = pos[..., 16 + 3] = pos[..., 64 + 48 + 15] = True
    w = R.pack_bits(pos).to(torch.int32) & 0xffff
    assert w.shape == (1, 1, 1, 2, 4)
    assert w[0, 0, 0].tolist() == [[0x8001, 0x0008, 0, 0], [0, 0, 0, 0x8000]]
    emu = EmuOps("f32")
    rnd = torch.rand(2, 3, 5, 192, generator=torch.Generator().manual_seed(3)) > 0.5
    mine = R.pack_bits(rnd)
    assert torch.equal(emu._unpack_bits(mine, 192), rnd)


def _first_diff(a, b):
    i = int((a.double() != b.double()).flatten().nonzero()[0])
    return tuple(int(v) for v in torch.unravel_index(torch.tensor(i), a.shape))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("what", ["unit_at_border", "swapped_taps"])
def test_mutations_are_caught_and_located(dtype, what):
    """A launch whose operand differs by ONE unit at the last (bottom-right) pixel of the image, or whose weight has taps 0 and 8
    swapped, must fail the comparison, at the first pixel where the float64 reference of the mutated operands differs."""
    case = R.BY_ID["halo-128-128-24x40-slab"]
    cv, master, src, acc, pre, dshape, _ = R.conv_data(case, dtype, ["plain"])

    def mutate(x, w):
        if what == "unit_at_border":
            x[-1, -1, -1, 5] += 1
        else:
            w[:, [0, 8], :] = w[:, [8, 0], :]
        return x, w
    xm, wm = mutate(src.clone(), master.clone())
    good = R.ref_fwd(cv, src, master, pre, dtype)[1]
    bad = R.ref_fwd(cv, xm, wm, pre, dtype)[1]
    at = _first_diff(good, bad)
    if what == "unit_at_border":       # a 3x3 neighbour of the perturbed pixel, in the last image
        assert at[0] == cv.N - 1 and at[1] >= cv.H - 2 and at[2] >= cv.W - 2
    R.run_conv_case(EmuOps(dtype), case, dtype, only="plain")             # the unmutated launch passes
    with pytest.raises(AssertionError) as err:
        R.run_conv_case(EmuOps(dtype), case, dtype, only="plain", mutate=mutate)
    msg = str(err.value)
    m = re.search(r"(\d+) of \d+ elements differ, first at \((\d+), (\d+), (\d+), (\d+)\)", msg)
    assert m, msg
    assert tuple(int(v) for v in m.groups()[1:]) == at, (msg, at)
    assert int(m.group(1)) == int((good.double() != bad.double()).sum()), msg


def test_oracle_refuses_mask_c0_behind_a_pixel_shuffle():
    """dg_epilogue: mask_c0 != 0 with a pixel-shuffled destination is refused by the library; the oracle asserts the same."""
    emu = EmuOps("f32")
    cv = R.Conv(1, 8, 8, 16, 64, 1, True)
    y = torch.zeros(emu.out_shape(cv))
    with pytest.raises(AssertionError, match="mask_c0"):
        emu.conv_fwd(cv, torch.zeros(1, 8, 8, 16), torch.zeros(64 * 9 * 16), y, mask=torch.zeros_like(y), mask_slope=0.25, mask_c0=16)
