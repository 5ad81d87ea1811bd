"""The weight-stationary streaming kernel for the stride-2 data gradient of the 128 -> 128 channel layer (csrc/conv_s2dgrad.hip):
bit-identical to the merged halo launch it replaces, within the bf16 tolerance of tests/test_kernels_gpu.py::test_conv_dgrad of
the CPU oracle, and it writes nothing outside dx."""
import ctypes as C

import pytest
import torch

from tests.test_kernels_gpu import close, pair, rnd

from downgan_amd.ops import Conv

pytestmark = pytest.mark.gpu

CASES = [
    # dx (N, H, W): dy is H/2 x W/2
    (1, 16, 16),     # dy 8 x 8: narrower than one fragment
    (2, 32, 32),     # dy 16 x 16: exactly one strip
    (3, 48, 80),     # dy 24 x 40: ragged columns and rows, image stride
    (2, 34, 66),     # dy 17 x 33: odd sizes
    (3, 64, 288),    # dy 32 x 144: 27 strips; also run with the launch capped at 4 workgroups, so the persistent walk wraps unevenly
]
EPILOGUES = ["plain", "mask_bits"]
GUARD = 8192         # elements of sentinel in front of and behind dx
SENTINEL = -77.0     # exactly representable in bf16

_inputs = {}
_refs = {}


def inputs(shape):
    """dy ~ N(0,1), w ~ 0.05 N(0,1) in bf16, random mask words -- one set per shape, on the CPU."""
    if shape not in _inputs:
        N, H, W = shape
        g = torch.Generator().manual_seed(1000 + H * W + N)
        dy = rnd((N, H // 2, W // 2, 128), torch.bfloat16, g)
        w = rnd((128 * 9 * 128,), torch.bfloat16, g, 0.05)
        bits = torch.randint(-32768, 32768, (N, H, W, 2, 4), generator=g, dtype=torch.int32).to(torch.int16)
        _inputs[shape] = (dy, w, bits)
    return _inputs[shape]


def epilogue(shape, kind, device):
    return {} if kind == "plain" else dict(mask_bits=inputs(shape)[2].to(device), mask_slope=0.2)


def reference(shape, kind):
    """The oracle's data gradient (what test_conv_dgrad compares with), computed once per (shape, epilogue)."""
    if (shape, kind) not in _refs:
        N, H, W = shape
        _, emu = pair("bf16")
        dy, w, _ = inputs(shape)
        dx = torch.zeros(N, H, W, 128, dtype=torch.bfloat16)
        emu.conv_dgrad(Conv(N, H, W, 128, 128, 2, False), dy, w, dx, **epilogue(shape, kind, "cpu"))
        _refs[(shape, kind)] = dx
    return _refs[(shape, kind)]


def run(hip, shape, kind, mode):
    """One data gradient into a sentinel-filled buffer with guard bands; returns (dx, front guard, back guard, kernel mask)."""
    N, H, W = shape
    cv = Conv(N, H, W, 128, 128, 2, False)
    dy, w, _ = inputs(shape)
    n = N * H * W * 128
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    dx = buf[GUARD:GUARD + n].view(N, H, W, 128)
    prev = hip.lib.dg_set_s2_dgrad_stream(mode)
    try:
        hip.conv_dgrad(cv, dy.cuda(), w.cuda(), dx, **epilogue(shape, kind, "cuda"))
        kinds = hip.lib.dg_last_conv_kernels()
        torch.cuda.synchronize()
    finally:
        hip.lib.dg_set_s2_dgrad_stream(prev)
    return dx, buf[:GUARD], buf[GUARD + n:], kinds


@pytest.mark.parametrize("kind", EPILOGUES)
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_stream_kernel_equals_the_halo_launch_and_the_oracle(shape, kind):
    hip, _ = pair("bf16")
    N, H, W = shape
    cv = Conv(N, H, W, 128, 128, 2, False)
    assert hip.lib.dg_set_s2_dgrad_stream(1) == 1, "the streaming kernel is the default"
    dx0 = torch.empty(N, H, W, 128, dtype=torch.bfloat16, device="cuda")
    g, e = hip._geom(cv, 128, 128), hip._epilogue(dx0, **epilogue(shape, kind, "cuda"))
    eligible = hip.lib.dg_conv3x3_dgrad_stream_eligible(C.byref(g), C.byref(e))
    assert eligible == 1, "every case of this table is inside the rule"
    seg, f0, b0, k0 = run(hip, shape, kind, 0)
    assert k0 == 8
    modes = [1, 4] if shape == (3, 64, 288) else [1]
    for mode in modes:
        dx, front, back, kinds = run(hip, shape, kind, mode)
        assert kinds == (64 if eligible else 8), (mode, kinds)
        assert torch.equal(dx, seg), (shape, kind, mode, int((dx != seg).sum()))
        sent = torch.full((), SENTINEL, dtype=torch.bfloat16, device="cuda")
        assert bool((front == sent).all()) and bool((back == sent).all()), (shape, kind, mode, "guard band written")
    assert bool((f0 == SENTINEL).all()) and bool((b0 == SENTINEL).all())
    close(dx, reference(shape, kind), "bf16", f"stream dgrad {shape} {kind}")


def test_other_stride2_data_gradients_stay_on_the_halo_kernel():
    """Outside the rule (here: 256 reduction channels; an activation-tensor mask) the merged halo launch serves the call."""
    hip, _ = pair("bf16")
    g = torch.Generator().manual_seed(7)
    for ci, co, ep in ((128, 256, {}), (128, 128, "mask")):
        cv = Conv(1, 32, 32, ci, co, 2, False)
        dy = rnd((1, 16, 16, co), torch.bfloat16, g).cuda()
        w = rnd((co * 9 * ci,), torch.bfloat16, g, 0.05).cuda()
        dx = torch.zeros(1, 32, 32, ci, dtype=torch.bfloat16, device="cuda")
        kw = dict(mask=rnd((1, 32, 32, ci), torch.bfloat16, g).cuda(), mask_slope=0.2) if ep == "mask" else {}
        ge, ee = hip._geom(cv, ci, co), hip._epilogue(dx, **kw)
        assert hip.lib.dg_conv3x3_dgrad_stream_eligible(C.byref(ge), C.byref(ee)) == 0
        hip.conv_dgrad(cv, dy, w, dx, **kw)
        assert hip.lib.dg_last_conv_kernels() == 8
