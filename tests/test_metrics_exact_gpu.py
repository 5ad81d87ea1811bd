"""The MS-SSIM / physics kernels (csrc/metrics.hip), the low-pass pair (csrc/freqsep.hip) and the staging kernels
(csrc/preprocess.hip) on the GPU against the definitions restated in tests/metrics_ref.py: bits on integer data and on fixed
chains of correctly rounded steps, exact counts and double sums, located windows, derived bounds for random data -- at small
shapes, on slab views, and at shapes where every grid-stride loop takes a second trip or a block cap is reached."""
import ctypes as C

import pytest
import torch

from downgan_amd import _lib
from downgan_amd.ops import HipOps
from tests import metrics_ref as M

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", M.CASES, ids=[c[0] for c in M.CASES])
def test_case(case, dtype):
    _, fn, kw, size = case
    assert size != "large" or kw.get("expect"), "a large case states what its size is for, and asserts it from its shape"
    fn(HipOps(dtype), dtype, **kw)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_rejections_return_the_error_code_without_a_launch():
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    inp, out = torch.ones(1, 8, 8, device=dev), torch.full((64,), 7.0, device=dev)
    for H, W in ((1, 8), (8, 1), (1, 1)):
        assert lib.dg_avgpool2(_ptr(inp), _ptr(out), 1, H, W, st) == -1
    X = torch.rand(1, 16, 16, device=dev)
    sums = torch.full((2,), 7.0, device=dev)
    assert lib.dg_ssim_level(_ptr(X), _ptr(X), 1, 16, 16, C.byref(M.ssim_params([1.0 / 12] * 11, 0.1, 0.1)), _ptr(sums), st) == 0
    torch.cuda.synchronize()
    after = sums.clone()
    p12 = _lib.SsimParams(win=12, C1=0.1, C2=0.1)
    assert lib.dg_ssim_level(_ptr(X), _ptr(X), 1, 16, 16, C.byref(p12), _ptr(sums), st) == -1            # win > 11
    p7 = M.ssim_params(M.gauss(7), 0.1, 0.1)
    assert lib.dg_ssim_level(_ptr(X), _ptr(X), 1, 6, 16, C.byref(p7), _ptr(sums), st) == -1             # H < win
    assert lib.dg_ssim_level(_ptr(X), _ptr(X), 1, 16, 6, C.byref(p7), _ptr(sums), st) == -1             # W < win
    assert lib.dg_ssim_level(_ptr(X), _ptr(X), 65536, 16, 16, C.byref(p7), _ptr(sums), st) == -1        # planes > 65535
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(sums, after)


def test_moments_refuses_a_pointer_off_16_byte_alignment():
    ops = HipOps("f32")
    x = torch.ones(9, device=ops.device)
    acc = torch.zeros(3, dtype=torch.float64, device=ops.device)
    with pytest.raises(RuntimeError, match="dg_moments failed: DG_ERR_BAD_ARG"):
        ops.moments(x[1:], acc)
    torch.cuda.synchronize()
    assert bool((acc == 0).all())
