"""Measurement behind F8_PRODUCT_BITS (tests/conv_f8_ref.py; DESIGN.md section 7, "Exact fp8 tests"): where does
v_mfma_scale_f32_32x32x64_f8f6f4, as wg3w_f8_kernel uses it, stop returning the exact integer?  One launch of
dg_conv3x3_wgrad_f8 (1 x H x 64 pixels, 128 -> 128 channels, zero preload) per setting: seven of eight elements are B, the others
odd integers below 16 (``mix``) or all are B; one sign or random signs.  Prints the largest reference sum, the number of
mismatches and the error range, all in units of the block pair's scale.  Needs a GPU:  python tools/f8_product_window_check.py

Seen on an MI355X: every setting with B <= 120 is exact (products 1 ... 2^13.8 in one MFMA; sums to 2^23.55 with H = 16); B = 240
alone is exact at 2^23.8; B = 240 mixed with small odd integers (products 1 ... 2^15.8) loses up to 7 units in ONE 64-pixel step
(H = 1, sums of 2^21.8) and up to 14 over four, always towards zero."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from downgan_amd.ops import Conv, HipOps  # noqa: E402
from tests import conv_f8_ref as F  # noqa: E402
from tests.conv_ref import ref_wgrad  # noqa: E402

ops = HipOps("bf16", f8_critic=True)


def one(H, B, mix, signed, narrow=True):
    gen = torch.Generator().manual_seed(H * 1000 + B + 7 * mix + 3 * signed)
    cv = Conv(1, H, 64, 128, 128, 1, net="C")
    rnd = lambda lo, hi, sh: torch.randint(lo, hi + 1, sh, generator=gen, dtype=torch.int64)

    def data(sh):
        v = torch.where(rnd(0, 7, sh) > 0, B, 2 * rnd(0, 7, sh) + 1) if mix else torch.full(sh, B, dtype=torch.int64)
        return v * (2 * rnd(0, 1, sh) - 1) if signed else v
    xb, dyb = F.encode(data((1, H, 64, 128))), F.encode(data((1, H, 64, 128)))
    ex, ey = F._exponents(gen, 4, narrow, False), F._exponents(gen, 4, narrow, True)
    rw, _ = ref_wgrad(cv, F.dequant(xb, ex), F.dequant(dyb, ey), torch.zeros(128 * 9 * 128))
    unit = F._unit(128, 128, ex, ey)
    dw = torch.zeros(128 * 9 * 128, device="cuda")
    ops.conv_wgrad_f8(cv, xb.cuda(), ex.cuda(), dyb.cuda(), ey.cuda(), dw)
    ru = rw.view(128, 9, 128) / unit
    err = dw.cpu().double().view(128, 9, 128) / unit - ru
    print(f"H={H:2d} B={B:3d} mix={int(mix)} signed={int(signed)} narrow={int(narrow)}: largest product 2^{torch.tensor(float(B * B)).log2():.1f}, "
          f"largest sum 2^{float(ru.abs().max().log2()):.2f}, mismatches {int((err != 0).sum())}/{err.numel()}, error {float(err.min()):.0f} ... {float(err.max()):.0f}")


for H in (1, 4):
    for B, mix in ((240, True), (240, False), (120, True), (60, True), (30, True), (16, True), (8, True)):
        one(H, B, mix, False)
    one(H, 240, True, True)
one(4, 240, True, False, narrow=False)
one(16, 120, True, False)
