"""The references and comparators of tests/elementwise_ref.py, proven on the host before anything runs on a GPU:

* ``EmuOps`` -- the fp32 restatement of the op contracts the CPU suite already trusts -- passes every small and view case of the
  GPU test's case table through the same comparators: the references and bounds are satisfiable by correct fp32 code;
* each mutant below, a subtly wrong kernel applied to the float64 reference output, is rejected."""
import pytest
import torch

from oracle.emu_ops import EmuOps
from tests import elementwise_ref as R

HOST_CASES = [c for c in R.CASES if c[3] in ("small", "view")]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_emu_ops_pass_every_small_and_view_case(case, dtype):
    _, fn, kw, _ = case
    fn(EmuOps(dtype), dtype, **kw)


def test_case_table_has_the_three_sizes_and_unique_ids():
    ids = [c[0] for c in R.CASES]
    assert len(set(ids)) == len(ids)
    assert {c[3] for c in R.CASES} == {"small", "view", "large"}
    for cid, _, kw, size in R.CASES:
        assert (size == "large") == ("expect" in kw), cid


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_size_guards_follow_the_shape_a_case_runs(dtype):
    """The guards are computed from the arguments a case runs with: each case, asked for its size property at a shape one step too
    small for it, refuses before it launches anything (the large shapes of the table pass theirs on the GPU)."""
    ops = EmuOps(dtype)
    e = R.epc(dtype)
    shrunk = [(R.case_mask_mul, dict(shape=(1, 512, 512, 4 * e))), (R.case_axpby, dict(shape=(1, 512, 512, 4 * e))),
              (R.case_gp_interp, dict(shape=(2, 512, 512, 4 * e))), (R.case_scale_rows, dict(shape=(2, 512, 512, 4 * e))),
              (R.case_layout, dict(N=1, C=2, H=728, W=720, cpad=16)), (R.case_nhwc_to_nchw_full, dict(shape=(1, 256, 256, 16))),
              (R.case_cast, dict(n=R.EW_THREADS)), (R.case_compact, dict(shape=(1, 1024, 2048, 8))),
              (R.case_repack, dict(cout=512, cin=224)), (R.case_gather, dict(hw=(128, 256), c_pad=16)),
              (R.case_adam, dict(n=4 * R.EW_THREADS))]
    for fn, kw in shrunk:
        with pytest.raises(AssertionError, match="size guard: .* one grid-stride trip"):
            fn(ops, dtype, expect="second_trip", **kw)
    capped = [(R.case_sumsq, dict(shape=(2, 512, 2048, e))), (R.case_l1, dict(shape=(1, 1024, 2048, e))),
              (R.case_l1, dict(shape=(1, 1024, 2048, e), sq=True)), (R.case_colsum, dict(rows=128 * 256, C=16)),
              (R.case_colsum_ps, dict(shape=(2, 256, 256, 24))), (R.case_colsum_multi, dict(shape=(1, 128, 256, 640), nseg=5))]
    for fn, kw in capped:
        with pytest.raises(AssertionError, match="size guard: .* cap of .* is not reached"):
            fn(ops, dtype, expect="cap", **kw)
    with pytest.raises(AssertionError, match="size guard: .* no ragged last workgroup"):
        R.case_colsum(ops, dtype, rows=129 * 256, C=16, expect="cap")


# ------------------------------------------------------------------------------------------------------------------ mutants
def _rne(x64, dtype):
    """A correct kernel's output for the float64 value: one rounding to fp32, one to the storage dtype."""
    return x64.float().to(R.TD[dtype])


def _toward_zero(x64):
    """fp32 -> bf16 by dropping the low 16 bits."""
    b = x64.float().contiguous().view(torch.int32) & ~0xffff
    return b.view(torch.float32).to(torch.bfloat16)


BOUND, BITS, SUMS, NONFINITE = "outside the bound", "differ in bits", "sums differ", "non-finite mismatch"


def _rejects(fn, why):
    """The comparator must refuse the mutant for the intended reason, not through a shape or dtype assert."""
    with pytest.raises(AssertionError, match=why):
        fn()


def _data(dtype, shape=R.S_SHAPE, seed=7, n=3):
    gen = torch.Generator().manual_seed(seed)
    return [R.randn(shape, dtype, gen) for _ in range(n)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mutant_mask_slope_zero(dtype):
    u, y, _ = _data(dtype)
    ref, M = R.ref_mask_mul(u, y, 0.01)
    R.check_elem(_rne(ref, dtype), ref, M, "mask_mul")
    _rejects(lambda: R.check_elem(_rne(R.ref_mask_mul(u, y, 0.0)[0], dtype), ref, M, "mask_mul with slope 0"), BOUND)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mutant_l1_gradient_scale(dtype):
    a, b, add = _data(dtype)
    _, ref, M = R.ref_l1(a, b, 0.37, add)
    R.check_elem(_rne(ref, dtype), ref, M, "l1 gradient")
    _rejects(lambda: R.check_elem(_rne(R.ref_l1(a, b, 0.33, add)[1], dtype), ref, M, "l1 gradient with scale 0.33"), BOUND)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mutant_alpha_swapped(dtype):
    real, fake, _ = _data(dtype)
    alpha = torch.tensor([0.3, 0.45, 0.9])
    ref, M = R.ref_interp(real, fake, alpha)
    R.check_elem(_rne(ref, dtype), ref, M, "gp_interp")
    _rejects(lambda: R.check_elem(_rne(R.ref_interp(real, fake, alpha, swap=True)[0], dtype), ref, M, "gp_interp with alpha and 1 - alpha swapped"), BOUND)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mutant_last_chunk_not_written(dtype):
    x, y, old = _data(dtype)
    ref, M = R.ref_axpby(x, 0.2, y, -1.7)
    out = _rne(ref, dtype)
    n = R.epc(dtype)
    out.view(-1)[-n:] = old.view(-1)[-n:]                   # the last 16 bytes keep the buffer's old content
    _rejects(lambda: R.check_elem(out, ref, M, "axpby with the last 16-byte chunk left"), BOUND)
    # and for a copy: the exact comparator
    src = torch.randn(1037, generator=torch.Generator().manual_seed(3))
    good = src.to(R.TD[dtype])
    R.assert_bits(good, src.to(R.TD[dtype]), "cast")
    bad = good.clone(); bad[-n:] = 1.0
    _rejects(lambda: R.assert_bits(bad, good, "cast with the last 16-byte chunk left"), BITS)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("mutant", ["row_dropped", "row_twice"])
def test_mutant_colsum_row(dtype, mutant):
    gen = torch.Generator().manual_seed(11)
    rows, C = 234, 48
    _, x = R.int_data((rows, C), -4, 4, gen, dtype, terms=rows, preload=64)
    db0 = torch.randint(-64, 65, (C,), generator=gen).float()
    ref, _ = R.ref_colsum(x, db0)
    R.check_exact_sum(ref.float(), ref, "colsum")
    # a row of zeros would hide either mutant: take a row that has none
    row = int((x.float() != 0).all(1).nonzero()[0]) if bool((x.float() != 0).all(1).any()) else int(x.float().abs().sum(1).argmax())
    bad, _ = R.ref_colsum(x, db0, **({"drop_row": row} if mutant == "row_dropped" else {"twice_row": row}))
    assert not torch.equal(bad, ref)
    _rejects(lambda: R.check_exact_sum(bad.float(), ref, "colsum " + mutant), SUMS)
    # the same mutants on N(0,1) data under the 1e-5 * sum |t| criterion
    xn = R.randn((rows, C), dtype, gen)
    refn, sabs = R.ref_colsum(xn, db0)
    R.check_sum(refn.float(), refn, sabs, "colsum N(0,1)")
    badn, _ = R.ref_colsum(xn, db0, **({"drop_row": 5} if mutant == "row_dropped" else {"twice_row": 5}))
    _rejects(lambda: R.check_sum(badn.float(), refn, sabs, "colsum N(0,1) " + mutant), "x the bound")


def test_mutant_round_toward_zero():
    x, y, _ = _data("bf16")
    ref, M = R.ref_axpby(x, 0.2, y, -1.7)
    R.check_elem(_rne(ref, "bf16"), ref, M, "axpby")
    _rejects(lambda: R.check_elem(_toward_zero(ref), ref, M, "axpby rounded toward zero"), BOUND)


def test_bf16_half_ulp_term_is_reached_but_not_exceeded_by_correct_rounding():
    """fp32 arithmetic followed by round-to-nearest-even reaches almost all of the half-ulp term at the bottom of a binade (where
    2^-8 |ref| alone would be too tight by a factor of up to two at the top, and this term is exactly tight)."""
    v = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20, 1.9921875 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float64)
    out = v.float().to(torch.bfloat16)
    err = (out.double() - v).abs()
    h = R.half_ulp_bf16(v, out.double())
    assert bool((err <= h).all()) and float((err / h).max()) > 0.99
    assert bool((err > 2.0 ** -8 * v.abs() * 0.5).all())
    assert float(R.half_ulp_bf16(torch.tensor([0.0], dtype=torch.float64), torch.tensor([0.5], dtype=torch.float64))) == 0.0


def _adam_state(n=4160, seed=5):
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-2
    m, v = g * 0.1, g * g * 0.01
    return p, g, m, v


@pytest.mark.parametrize("mutant", ["no_grad_scale", "bc2_at_step_minus_1"])
def test_mutant_adam(mutant):
    p, g, m, v = _adam_state()
    hp = (2.5e-4, 0.9, 0.99, 1e-8)
    step = 2
    ref = R.ref_adam(p, g, m, v, *hp, step, grad_scale=0.5)
    for k in ("p", "m", "v"):
        R.check_abs(ref[k][0].float(), *ref[k], "adam " + k, family="adam")
    if mutant == "no_grad_scale":
        bad = R.ref_adam(p, g, m, v, *hp, step, grad_scale=0.5, use_grad_scale=False)
        for k in ("p", "m", "v"):
            _rejects(lambda: R.check_abs(bad[k][0].float(), *ref[k], f"adam {k} without grad_scale", family="adam"), BOUND)
    else:
        bad = R.ref_adam(p, g, m, v, *hp, step, grad_scale=0.5, bc2_step=step - 1)
        _rejects(lambda: R.check_abs(bad["p"][0].float(), *ref["p"], "adam p with bc2 at step - 1", family="adam"), BOUND)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mutant_repack_without_tap_mirror(dtype):
    master = torch.randn(48 * 9 * 16, generator=torch.Generator().manual_seed(13))
    good = R.ref_repack(master, 48, 16, 2, R.TD[dtype])
    bad = R.ref_repack(master, 48, 16, 2, R.TD[dtype], mirror=False)
    R.assert_bits(good.clone(), good, "repack kind 2")
    _rejects(lambda: R.assert_bits(bad, good, "repack kind 2 without the tap mirror"), BITS)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_mutant_gather_reads_previous_index(dtype):
    gen = torch.Generator().manual_seed(17)
    store = R.randn((7, 8, 12, 3), dtype, gen)
    idx = torch.tensor([6, 0, 6, 3, 1])
    good = R.ref_gather(store, idx, 8)
    bad = R.ref_gather(store, idx, 8, shift=1)              # sample b from idx[b - 1]
    R.assert_bits(good.clone(), good, "gather_samples")
    _rejects(lambda: R.assert_bits(bad, good, "gather_samples reading idx[b - 1]"), BITS)


def test_nonfinite_values_must_match_in_kind_and_sign():
    ref = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.0], dtype=torch.float64)
    M = torch.ones(4, dtype=torch.float64)
    R.check_elem(ref.float(), ref, M, "non-finite")
    for bad in ([float("-inf"), float("-inf"), float("nan"), 1.0], [float("inf"), float("-inf"), 0.0, 1.0],
                [float("inf"), float("-inf"), float("nan"), float("inf")], [float("nan"), float("-inf"), float("nan"), 1.0]):
        _rejects(lambda: R.check_elem(torch.tensor(bad), ref, M, "non-finite mismatch"), NONFINITE)


def test_integer_generator_refuses_sums_that_fp32_would_round():
    gen = torch.Generator().manual_seed(1)
    R.int_data((4, 4), -4, 4, gen, "bf16", terms=300001, preload=64)
    with pytest.raises(AssertionError):
        R.int_data((4, 4), -4, 4, gen, "bf16", terms=2 ** 22, preload=0)
