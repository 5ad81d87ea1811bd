"""The elementwise, reduction and layout kernels of csrc/elementwise.hip on the GPU, per element and at scale: every case of
tests/elementwise_ref.py (float64 references; 4 * 2^-24 * M plus one bf16 rounding per element; bit equality for copies; exact
integer sums) at small shapes, on channel slices of wider slabs, and at shapes where the grid-stride loops take a second trip and
the block caps of the reductions are reached -- then the reductions again in deterministic mode."""
import gc

import pytest
import torch

from downgan_amd import ops as ops_mod
from downgan_amd.ops import HipOps
from tests import elementwise_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_case(case, dtype):
    _, fn, kw, size = case
    assert size != "large" or kw.get("expect"), "a large case states what its size is for, and asserts it from its shape"
    fn(HipOps(dtype), dtype, **kw)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_colsum_wider_than_256_chunks_is_refused(dtype):
    """C = 1032 fp32 is 258 16-byte chunks, more than a workgroup has threads: bad shape, not a launch."""
    ops = HipOps(dtype)
    dy = torch.ones(16, 1032, device=ops.device)
    db = torch.zeros(1032, device=ops.device)
    with pytest.raises(RuntimeError, match="dg_colsum failed: DG_ERR_BAD_SHAPE"):
        ops.colsum(dy, db)
    torch.cuda.synchronize()
    assert bool((db == 0).all())


# ------------------------------------------------------------------------------------------------------------------ deterministic mode
DET = [
    # expect="cap": asserted by the case from the shape it runs (tests/elementwise_ref.py, guard_cap)
    ("sumsq", R.case_sumsq, dict(shape=(2, 728, 736, 16), expect="cap")),
    ("l1", R.case_l1, dict(shape=(1, 728, 736, 32), with_grad=False, expect="cap")),
    ("sqdiff", R.case_l1, dict(shape=(1, 728, 736, 32), sq=True, expect="cap")),
    ("colsum-300001x16", R.case_colsum, dict(rows=300001, C=16, expect="cap")),
    ("colsum-view", R.case_colsum, dict(view=True)),
    ("colsum-c256", R.case_colsum_c256, dict()),
    ("colsum_ps", R.case_colsum_ps, dict(shape=(2, 362, 364, 24), expect="cap")),
    ("colsum_multi-640x5", R.case_colsum_multi, dict(shape=(1, 182, 184, 640), nseg=5, expect="cap")),
    # one workgroup: a single copy, written straight into the target
    ("colsum_ps-small", R.case_colsum_ps, dict(shape=(2, 10, 14, 24))),
    ("colsum_multi-128x8-small", R.case_colsum_multi, dict(shape=(1, 9, 13, 128), nseg=8)),
]


def _no_deterministic_holder():
    gc.collect()
    assert ops_mod._DET["refs"] == 0 and ops_mod._DET["ws"] is None, "a deterministic HipOps of an earlier test is still open"


@pytest.mark.parametrize("data", ["int", "normal"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", DET, ids=[c[0] for c in DET])
def test_deterministic_mode(case, dtype, data):
    """Exact-integer data: the result is exact and two runs are bit-identical; N(0,1) data: two runs are bit-identical and the
    result is within 1e-5 of the column's sum of |terms| (rtol 1e-5 for the sums of non-negative terms)."""
    _, fn, kw = case
    refs = ops_mod._DET["refs"]
    ops = HipOps(dtype, deterministic=True)
    try:
        assert ops.deterministic
        fn(ops, dtype, data=data, runs=2, **kw)
    finally:
        ops.close()
    assert ops_mod._DET["refs"] == refs


def test_deterministic_colsum_multi_with_a_workspace_too_small_for_its_copies():
    """bf16 [110,001 rows, 640] in 5 segments wants 110001 / 256 = 429 copies of 640 floats; a 1 MiB workspace holds 409, so
    colsum_launch re-partitions the rows over 409 workgroups.  Still exact on integer data, and repeatable."""
    rows, C, nseg, mb = 110001, 640, 5, 1
    want = min(rows // 256, 128 * nseg)
    fit = (mb << 20) // 4 // C
    assert want == 429 and fit == 409 and fit < want
    _no_deterministic_holder()
    ops = HipOps("bf16", deterministic=True, det_workspace_mb=mb)
    try:
        assert ops.deterministic and ops_mod._DET["ws"].numel() == mb << 20
        R.case_colsum_multi(ops, "bf16", shape=(1, 1, rows, C), nseg=nseg, data="int", runs=2)
    finally:
        ops.close()
    assert not ops.deterministic
