"""The exact fp8 case table of tests/conv_f8_ref.py through the CPU oracle (oracle/emu_ops.py): every case, in both data regimes,
must be bit-equal between EmuOps and the float64 references, every budget must hold and every case guard must name the path the
case is there for.  That validates the operands, the references and the guards without a GPU.  The mutation checks prove that the
comparator notices two swapped scale bytes, a weight-scale row taken from the neighbouring tap, one E4M3 unit at a border pixel
and a block exponent off by one, each at the place where it acts; the generator tests that the budget assertions fire, that the
fine regime stays within the integers of bf16 and that the hand-written E4M3 table is torch's."""
import dataclasses
import re

import pytest
import torch

from oracle.emu_ops import EmuOps
from tests import conv_f8_ref as F

_OPS = {}


def emu(case=None):
    gen = case is not None and case.net == "T"
    if gen not in _OPS:
        _OPS[gen] = EmuOps("bf16", f8_generator=True) if gen else EmuOps("bf16", f8_critic=True)
    return _OPS[gen]


@pytest.mark.parametrize("cid,regime", F.PARAMS, ids=[f"{c}-{r}" for c, r in F.PARAMS])
def test_case_is_exact_on_the_oracle(cid, regime):
    F.run_f8_conv_case(emu, F.BY_ID[cid], regime)


@pytest.mark.parametrize("cid", F.SELFQ)
def test_self_quantised_route_gives_the_same_bits(cid):
    """Without xq= / wq= the library quantises the dequantised bf16 tensors itself: the MX quantiser is lossless on such data (other
    scale bytes, the same values), so the same reference bits come out."""
    for regime in ("wide", "fine"):
        F.run_f8_conv_case(emu, F.BY_ID[cid], regime, only="plain", selfq=True)


@pytest.mark.parametrize("cid", [c.id for c in F.WCASES])
def test_wgrad_case_is_exact_on_the_oracle(cid):
    F.run_f8_wcase(emu(), F.WBY_ID[cid])


def test_every_f8_path_has_a_case():
    assert {c.expect for c in F.CASES} == set(F.F8_PATHS)
    assert {c.kind for c in F.WCASES} == {"wgrad", "dense"}


@pytest.mark.parametrize("D", [F.D_DEFAULT, F.D_FAR])
@pytest.mark.parametrize("positive", [False, True], ids=["signed", "one-sign"])
def test_assumption_data_is_exact_and_reaches_the_budget(positive, D):
    """The data of the device's first test: exact on the oracle; with one sign its sums pass 2^23 and include odd integers."""
    case = F.BY_ID[F.FIRST]
    F.run_f8_conv_case(emu, case, "wide", only="plain", positive=positive, D=D)
    acc = F.f8_data(case, "wide", ["plain"], positive, D).acc
    assert float(acc.abs().max()) < F.F8_INT_LIMIT
    if positive:
        big = acc[acc.abs() > F.F8_INT_LIMIT // 2]
        assert big.numel() > 100 and bool((big % 2 == 1).any())


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow-exponents", "wide-exponents"])
@pytest.mark.parametrize("positive", [False, True], ids=["signed", "one-sign"])
def test_wgrad_assumption_data_is_exact(positive, narrow):
    """The data of the device's second test: exact on the oracle; with one sign the sums, in units of their block pair's scale, pass
    2^23 and include odd integers."""
    case = F.WBY_ID[F.FIRST_WGRAD_ONE_SIGN if positive else F.FIRST_WGRAD]
    F.run_f8_wgrad_case(emu(), case, positive=positive, narrow=narrow)
    units = F.f8_wgrad_data(case, positive, narrow)[7]
    assert float(units.abs().max()) < F.F8_INT_LIMIT
    if positive:
        big = units[units.abs() > F.F8_INT_LIMIT // 2]
        assert big.numel() > 1000 and bool((big % 2 == 1).any())


# ---------------------------------------------------------------------------------------------------------------- generators
def test_decode_table_is_torchs():
    b = torch.arange(256, dtype=torch.uint8)
    t = b.view(torch.float8_e4m3fn).double()
    nan = torch.isnan(F.E4M3)
    assert torch.equal(nan, torch.isnan(t)) and int(nan.sum()) == 2
    assert torch.equal(F.E4M3[~nan], t[~nan])
    assert torch.equal(torch.signbit(F.E4M3[~nan]), torch.signbit(t[~nan]))
    v = torch.arange(-16, 17)
    assert torch.equal(F.encode(v).view(torch.float8_e4m3fn).double(), v.double())
    assert float(F.E4M3[0x7e]) == 448.0 and float(F.E4M3[0x01]) == 2.0 ** -9


def test_budgets_are_asserted():
    sx, sw = F.wide_spreads(9 * 128, 0)
    assert 8 * 3 * 2 ** (sx + sw) * 9 * 128 + 256 < 2 ** 24 <= 8 * 3 * 2 ** (sx + sw + 1) * 9 * 128 + 256 and sx - sw in (0, 1)
    assert sum(F.wide_spreads(9 * 1024, 2)) == 4 and sum(F.wide_spreads(9 * 128, 0, limit=1 << 16)) == 1
    with pytest.raises(AssertionError, match="no integer budget"):
        F.assert_wide_budget(9 * 128, sx + 1, sw, 0)
    with pytest.raises(AssertionError, match="no integer budget"):
        F.assert_wide_budget(9 * 1024, 0, 0, 8)
    with pytest.raises(AssertionError, match="fine regime"):
        F.assert_fine_budget(torch.tensor([3.0, -249.0]))
    F.assert_fine_budget(torch.tensor([3.0, -248.0]))
    with pytest.raises(AssertionError, match="no integer budget"):
        F.assert_wgrad_budget(1 << 18)
    F.assert_wgrad_budget(1024, F.MAG_ONE_SIGN)
    with pytest.raises(AssertionError, match="no integer budget: 2048 pixels"):
        F.assert_wgrad_budget(2048, F.MAG_ONE_SIGN)
    with pytest.raises(AssertionError, match="span more than"):
        F.assert_wgrad_budget(256, 240)
    with pytest.raises(AssertionError, match="span more than"):
        F.assert_wide_budget(9, 5, 5, 0)
    assert sum(F.wide_spreads(9, 0)) == 9                    # a short reduction: the product window binds, not the sum
    with pytest.raises(AssertionError, match="not an integer E4M3 holds"):
        F.encode(torch.tensor([17]))
    assert F.encode(torch.tensor([-240, 448, 0])).tolist() == [0xf7, 0x7e, 0x00]


def test_fine_regime_stays_within_bf16_integers():
    """max |v| <= 256 - 8 for every case of the table (the generator asserts it too), and the stored values of the plain epilogue
    are the accumulator itself."""
    for c in F.CASES:
        if "fine" in c.regimes:
            d = F.f8_data(c, "fine")
            m = float(d.acc.abs().max())
            assert 16 <= m <= F.FINE_MAX - F.FINE_ADD, (c.id, m)
            assert torch.equal(d.acc.to(torch.bfloat16).double(), d.acc), c.id


def test_wide_regime_is_mostly_not_representable_in_bf16():
    """Why the fine regime exists: the final rounding of the wide regime can hide a one-unit error."""
    acc = F.f8_data(F.BY_ID["f8-halo-256-192-24x40-slab"], "wide").acc
    assert float((acc.to(torch.bfloat16).double() != acc).double().mean()) > 0.8


def test_guard_fails_when_a_shape_is_edited_onto_another_path():
    """192 outputs are no whole 256-channel tiles: the eight-wave case would run on the four-wave instance, and its guard says so."""
    case = dataclasses.replace(F.BY_ID["f8-s2-128-256-48x80"], shape=(1, 48, 80, 128, 192, 2))
    with pytest.raises(AssertionError, match="case guard: .* would take f8_s2_4w, the case is there for f8_s2_8w"):
        F.run_f8_conv_case(emu, case, "fine", only="plain")
    case = dataclasses.replace(F.BY_ID["f8-classes-dgrad-128-128-32x32-rowstep"], big_ldy=False)
    with pytest.raises(AssertionError, match="would take f8_seg_interleaved"):
        F.run_f8_conv_case(emu, case, "fine", only="plain")
    with pytest.raises(AssertionError, match="case guard"):
        F.run_f8_wgrad_case(emu(), dataclasses.replace(F.WBY_ID[F.FIRST_WGRAD], shape=(1, 4, 32, 128, 128, 1)))


# ---------------------------------------------------------------------------------------------------------------- mutations
def _diff(a, b):
    return (a.double() != b.double()).nonzero()


def _caught(case, regime, mutate):
    """Runs the mutated launch; returns (reported count, reported first index, diff indices of the reference of the mutated operands)."""
    d = F.f8_data(case, regime, ["plain"])
    xq, xs, wq, ws = mutate(d.xq.clone(), d.xs.clone(), d.wq.clone(), d.ws.clone())
    xv, _, master = F.operand_values(case, F.encode(xq), xs, F.encode(wq), ws)
    good, _ = F.reference(case, d, "plain", {}, None)
    bad, _ = F.reference(case, d, "plain", {}, None, acc=F.accumulator(case, xv, master))
    at = _diff(good, bad)
    assert at.numel() > 0
    F.run_f8_conv_case(emu, case, regime, only="plain")                     # the unmutated launch passes
    with pytest.raises(AssertionError) as err:
        F.run_f8_conv_case(emu, case, regime, only="plain", mutate=mutate)
    m = re.search(r"(\d+) of \d+ elements differ, first at \((\d+), (\d+), (\d+), (\d+)\)", str(err.value))
    assert m, str(err.value)
    assert int(m.group(1)) == at.shape[0] and tuple(int(v) for v in m.groups()[1:]) == tuple(at[0].tolist()), (str(err.value), at[0])
    return at


@pytest.mark.parametrize("cid", ["f8-halo-128-80-16x24", "f8-s2-128-128-48x80"])
def test_swapped_scale_bytes_of_one_pixel_are_caught(cid):
    """Two scale bytes of ONE source pixel swapped: at stride 1 the 3x3 output pixels that read it change, at stride 2 (an even
    source pixel) the one output pixel whose centre tap it is."""
    case = F.BY_ID[cid]
    d = F.f8_data(case, "wide", ["plain"])
    h, w = 6, 8
    b0, b1 = next((i, j) for i in range(4) for j in range(i + 1, 4) if int(d.xs[0, h, w, i]) != int(d.xs[0, h, w, j]))

    def mutate(xq, xs, wq, ws):
        xs[0, h, w, [b0, b1]] = xs[0, h, w, [b1, b0]]
        return xq, xs, wq, ws
    at = _caught(case, "wide", mutate)
    st = case.shape[5]
    if st == 1:
        assert bool(((at[:, 1] - h).abs() <= 1).all() and ((at[:, 2] - w).abs() <= 1).all()) and len({(int(a[1]), int(a[2])) for a in at}) == 9
    else:
        assert {(int(a[1]), int(a[2])) for a in at} == {(h // 2, w // 2)}


def test_weight_scale_row_of_the_neighbouring_tap_is_caught():
    """The scale row of (output channel 77, tap 4) replaced by the one of tap 5: only channel 77 changes."""
    case = F.BY_ID["f8-halo-128-80-16x24"]

    def mutate(xq, xs, wq, ws):
        v = ws.view(80, 9, 4)
        assert not torch.equal(v[77, 4], v[77, 5])
        v[77, 4] = v[77, 5].clone()
        return xq, xs, wq, ws
    at = _caught(case, "wide", mutate)
    assert set(at[:, 3].tolist()) == {77} and at.shape[0] > 16 * 24 // 2


def test_one_e4m3_unit_at_a_border_pixel_is_caught_in_the_fine_regime():
    """One unit at the last (bottom-right) source pixel: a 2x2 corner of the last image changes -- in the fine regime every changed
    accumulator shows in the stored bf16 value."""
    case = F.BY_ID["f8-halo-256-192-24x40-slab"]
    d = F.f8_data(case, "fine", ["plain"])

    def mutate(xq, xs, wq, ws):
        xq[-1, -1, -1, 5] += 1
        return xq, xs, wq, ws
    at = _caught(case, "fine", mutate)
    cv = d.cv
    assert bool((at[:, 0] == cv.N - 1).all() and (at[:, 1] >= cv.H - 2).all() and (at[:, 2] >= cv.W - 2).all())
    # every output whose weight at that tap and channel is not zero changed: nothing was hidden by the final rounding
    w = d.wq.view(cv.Cout, 9, cv.Cin)[:, :, 5]
    assert at.shape[0] == sum(int((w[:, t] != 0).sum()) for t in (4, 5, 7, 8))


def test_block_exponent_off_by_one_is_caught_in_a_weight_gradient():
    case = F.WBY_ID[F.FIRST_WGRAD]

    def mutate(ex, ey):
        ex[1] += 1
        return ex, ey
    F.run_f8_wgrad_case(emu(), case)
    with pytest.raises(AssertionError) as err:
        F.run_f8_wgrad_case(emu(), case, mutate=mutate)
    m = re.search(r"(\d+) of \d+ elements differ, first at \((\d+), (\d+), (\d+)\)", str(err.value))
    assert m, str(err.value)
    co, tap, ci = (int(v) for v in m.groups()[1:])
    assert (co, tap) == (0, 0) and 32 <= ci < 64 and int(m.group(1)) <= 128 * 9 * 32
