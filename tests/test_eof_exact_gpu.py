"""EXACT tests of the EOF kernels on the MI355X (csrc/eof.hip): the case table of tests/eof_ref.py through HipOps("f32"), every
output compared bit for bit with its float64 reference on integer data, guards around every destination and workspace checked.
The first test states the assumption (an integer f32 MFMA chain below 2^24 is exact): a failure THERE is about the assumption or
the budget, a failure after it about a kernel."""
import numpy as np
import pytest
import torch

from downgan_amd.ops import HipOps
from tests import eof_ref as R
from tests.elementwise_ref import INT_LIMIT, assert_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    return HipOps("f32", DEV)


@pytest.mark.parametrize("cid", R.FIRST)
def test_integer_f32_mfma_chain_is_exact(ops, cid):
    """T = 5, C = 1, P = 64, one slice, one chunk, one tile of v_mfma_f32_32x32x2_f32: signed deviations, and deviations of one sign
    whose sums stand near 64 * 192^2."""
    R.run_case(ops, R.BY_ID[cid])


@pytest.mark.parametrize("cid", [c.id for c in R.CASES if c.id not in R.FIRST])
def test_case(ops, cid):
    R.run_case(ops, R.BY_ID[cid])


def test_one_sign_slabs_stay_below_2_24_and_the_total_lies_above(ops):
    """What the one-sign case is there for, read from the device's own result: the slice sum is fp64."""
    case = R.ONE_SIGN
    inp = R.inputs(case)
    (_, mu), = inp["mus"]
    assert R.budget(case) < INT_LIMIT
    src, f = R.stage(ops, inp["x"], case.fmt)
    G = torch.empty(case.C, case.T, case.T, dtype=torch.float64, device=DEV)
    R.gram_explicit(ops, f, R._dev(ops, mu), case.nslice, G)
    diag = torch.diagonal(G, dim1=1, dim2=2).cpu().numpy()
    assert diag.min() > INT_LIMIT, diag.min()
    assert np.array_equal(diag, np.diagonal(R.ref_gram(inp["x"], mu), axis1=1, axis2=2))


def test_wrappers_give_the_bits_of_the_explicit_calls(ops):
    """HipOps.eof_gram / eof_project choose their own nslice (64-pixel slices here); integer partial sums commute exactly, so the
    results equal those of one long slice bit for bit."""
    case = R.BY_ID[f"gram-T77-C2-P{R.P0}-ns1"]
    inp = R.inputs(case)
    ns_wrapper, _ = ops.eof_gram_slices(case.T, case.C, case.P)
    assert ns_wrapper != case.nslice and R.slice_len(case.P, ns_wrapper) == 64
    src, f = R.stage(ops, inp["x"], case.fmt)
    for name, mu in inp["mus"]:
        mu_d = R._dev(ops, mu)
        a = torch.empty(case.C, case.T, case.T, dtype=torch.float64, device=DEV)
        b = torch.empty_like(a)
        R.gram_explicit(ops, f, mu_d, case.nslice, a)
        ops.eof_gram(f, mu_d, b)
        assert_bits(b, a, f"{case.id} {name}: HipOps.eof_gram against nslice = {case.nslice}")
    case = next(c for c in R.CASES if c.kind == "project" and c.T == 70 and c.K == 33 and c.C == 5 and c.nslice == 1)
    inp = R.inputs(case)
    src, f = R.stage(ops, inp["y"], case.fmt)
    store, ld_k, ld_c = R.e_store(inp["E"], case.layout)
    E_d, m_d = store.to(DEV), R._dev(ops, inp["m"])
    a = torch.empty(case.T, case.C, case.K, dtype=torch.float32, device=DEV)
    b = torch.empty_like(a)
    R.project_explicit(ops, f, m_d, E_d, case.K, ld_k, ld_c, case.nslice, a)
    ops.eof_project(f, m_d, E_d, case.K, ld_k, ld_c, b)
    assert_bits(b, a, f"{case.id}: HipOps.eof_project against nslice = {case.nslice}")


def test_mean_then_gram_of_the_device_mean(ops):
    """The fit's own sequence on zero-sum data: dg_eof_mean returns the integer mean, and the Gram about THAT buffer is exact."""
    case = R.BY_ID[f"gram-T77-C2-P{R.P0}-ns5"]
    inp = R.inputs(case)
    name, mu = inp["mus"][0]
    assert name == "true-mean"
    src, f = R.stage(ops, inp["x"], case.fmt)
    mu_d = torch.empty(case.C, case.P, dtype=torch.float32, device=DEV)
    ops.eof_mean(f, mu_d)
    assert_bits(mu_d, torch.from_numpy(mu.astype(np.float32)), "the mean of zero-sum data")
    G = torch.empty(case.C, case.T, case.T, dtype=torch.float64, device=DEV)
    R.gram_explicit(ops, f, mu_d, case.nslice, G)
    assert_bits(G, torch.from_numpy(R.ref_gram(inp["x"], mu)), case.id)
