"""MXFP8 conv path (BASELINE configs[4]) through the C ABI: dg_quant_mxfp8 bit-exact against the emulation, the fp8
forward / stride-2 forward / data-gradient convs of the critic's wide layers (critic.py:25-88) against fp32 convolutions of
the SAME dequantised operands (products of E4M3 values are exact in fp32, so only accumulation order and the bf16 rounding
of the result differ), and one critic + generator iteration of the engine in fp8 mode against the emulated engine."""
import json
import os

import pytest
import torch

from downgan_amd.ops import Conv, HipOps
from oracle.emu_ops import EmuOps

pytestmark = pytest.mark.gpu


def close(a, b, what, tol=1.6e-2):
    a, b = a.float().cpu(), b.float().cpu()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} (scale {scale:.3e}) at {(a - b).abs().argmax().item()}"


@pytest.mark.parametrize("src_dtype", [torch.bfloat16, torch.float32])
def test_quantiser_matches_emulation_bit_for_bit(src_dtype):
    hip = HipOps("bf16")
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(3, 9, 13, 384, generator=g) * torch.logspace(-7, 3, 384)).to(src_dtype)
    x[0, 0, 0, :128] = 0
    x[1, 2, 3, 200] = 3e4
    x[2, :, :, 256:] *= 1e-30                                   # deep underflow: scale byte clamps at 0
    q_ref, s_ref, _ = EmuOps.mx_quant(x)
    q, s = hip.quant_mxfp8(x.cuda())
    assert torch.equal(s.cpu(), s_ref), (s.cpu().int() - s_ref.int()).abs().max()
    same = q.cpu() == q_ref
    zeros = (q.cpu() & 0x7f) == 0                               # +0 / -0 are the same value
    assert bool((same | (zeros & ((q_ref & 0x7f) == 0))).all()), int((~same).sum())
    # a channel-slice view with a wider pixel stride
    slab = torch.randn(2, 4, 4, 640, generator=g).to(src_dtype).cuda()
    q2, s2 = hip.quant_mxfp8(slab[..., 128:384])
    q2r, s2r, _ = EmuOps.mx_quant(slab[..., 128:384].cpu())
    assert torch.equal(q2.cpu(), q2r) and torch.equal(s2.cpu(), s2r)


def test_quantiser_keeps_nan_and_inf_visible():
    """A NaN or an Inf must not be clamped into a finite fp8 value (every later fp8 layer reads only the quantised copy): the
    whole 32-channel block becomes E4M3 NaN -- stand-alone quantiser and fused conv epilogue alike, bit-equal to the emulation --
    and an fp8 conv fed such a block returns NaN for the pixels that read it."""
    hip = HipOps("bf16", f8_critic=True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 8, 256, generator=g).to(torch.bfloat16)
    x[0, 1, 2, 37] = float("nan"); x[1, 3, 3, 200] = float("inf"); x[1, 7, 0, 64] = float("-inf")
    q_ref, s_ref, deq = EmuOps.mx_quant(x)
    q, s = hip.quant_mxfp8(x.cuda())
    assert torch.equal(q.cpu(), q_ref) and torch.equal(s.cpu(), s_ref)
    for (n, h, w, c) in ((0, 1, 2, 37), (1, 3, 3, 200), (1, 7, 0, 64)):
        blk = q.cpu()[n, h, w, 32 * (c // 32):32 * (c // 32) + 32]
        assert bool((blk == 0x7F).all()) and bool(torch.isnan(deq[n, h, w, c]))
    assert int((q.cpu() == 0x7F).sum()) == 3 * 32                      # nothing else was touched
    # fused epilogue: a conv whose OUTPUT has a NaN (NaN bias -> every pixel of that channel) writes NaN blocks in its fp8 copy
    cv = Conv(1, 16, 16, 128, 128, 1, False)
    xin = torch.randn(1, 16, 16, 128, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(128 * 9 * 128, generator=g) * 0.05).to(torch.bfloat16).cuda()
    b = torch.zeros(128); b[70] = float("nan")
    y = torch.zeros(1, 16, 16, 128, dtype=torch.bfloat16).cuda()
    oq = (torch.zeros(1, 16, 16, 128, dtype=torch.uint8).cuda(), torch.zeros(1, 16, 16, 4, dtype=torch.uint8).cuda())
    hip.conv_fwd(cv, xin, w, y, bias=b.cuda(), out_q=oq)
    assert bool(torch.isnan(y[..., 70].float()).all())
    assert bool((oq[0][..., 64:96] == 0x7F).all()) and not bool((oq[0][..., :64] == 0x7F).all())
    q2, s2 = hip.quant_mxfp8(y)
    assert torch.equal(oq[0], q2) and torch.equal(oq[1], s2)
    # and the next fp8 layer sees it: NaN in, NaN out
    cvn = Conv(1, 16, 16, 128, 128, 1, False, net="C")
    out = torch.zeros(1, 16, 16, 128, dtype=torch.bfloat16).cuda()
    hip.conv_fwd(cvn, y, w, out, xq=oq)
    assert bool(torch.isnan(out.float()).all())


F8_CONVS = [
    # N, H, W, Cin, Cout, stride  -- the critic's wide layers at cfg2 widths (critic.py:25-88), small grids; ragged tiles
    (1, 32, 32, 128, 128, 2),
    (1, 32, 32, 128, 256, 1),
    (2, 48, 80, 256, 256, 2),
    (1, 32, 32, 256, 512, 1),
    (1, 32, 32, 512, 512, 2),
    (1, 16, 16, 512, 1024, 1),
    (1, 32, 32, 1024, 1024, 2),
    (2, 24, 40, 128, 192, 1),      # partial output-channel tile
]


@pytest.mark.parametrize("cfg", F8_CONVS)
def test_fp8_conv_fwd_and_dgrad(cfg):
    """Realistic data (channels over three decades, the library's own quantiser) against the emulation, to 1.6e-2 of the LARGEST
    entry.  That gate cannot see an error confined to the small input channels (every channel below ~0.1, more than a third of
    them, contributes less than the tolerance), a scale byte fetched from a neighbouring pixel / block / tap row among similar
    scales, or a clamped weight row on a partial channel tile: those are pinned bit for bit, per input-channel block and with the
    block scales as exact data, by tests/test_conv_f8_exact_gpu.py (tests/conv_f8_ref.py).  This test keeps what those cannot
    give: real-valued operands through dg_quant_mxfp8 at the critic's layer shapes."""
    N, H, W, ci, co, st = cfg
    hip, emu = HipOps("bf16", f8_critic=True), EmuOps("bf16", f8_critic=True)
    g = torch.Generator().manual_seed(21)
    cv = Conv(N, H, W, ci, co, st, False, net="C")
    x = (torch.randn(N, H, W, ci, generator=g) * torch.logspace(-2, 1, ci)).to(torch.bfloat16)
    w = (torch.randn(co * 9 * ci, generator=g) * 0.05).to(torch.bfloat16)
    osh = emu.out_shape(cv)
    # forward: LeakyReLU + out_bits (critic forward) / 1-bit mask (penalty tangent forward)
    bits_shape = emu.bits_shape(osh) if co % 64 == 0 else None
    y_ref = torch.zeros(osh, dtype=torch.bfloat16)
    ob_ref = torch.zeros(bits_shape, dtype=torch.int16) if bits_shape else None
    emu.conv_fwd(cv, x, w, y_ref, act=0.2, out_bits=ob_ref)
    y = torch.zeros(osh, dtype=torch.bfloat16).cuda()
    ob = torch.zeros(bits_shape, dtype=torch.int16).cuda() if bits_shape else None
    hip.conv_fwd(cv, x.cuda(), w.cuda(), y, act=0.2, out_bits=ob)
    assert hip.lib.dg_last_conv_kernels() == 32                    # the fp8 kernel served the call
    close(y, y_ref, f"fp8 fwd {cfg}")
    if bits_shape:
        y2_ref, y2 = torch.zeros(osh, dtype=torch.bfloat16), torch.zeros(osh, dtype=torch.bfloat16).cuda()
        emu.conv_fwd(cv, x, w, y2_ref, mask_bits=ob_ref, mask_slope=0.2)
        hip.conv_fwd(cv, x.cuda(), w.cuda(), y2, mask_bits=ob_ref.cuda(), mask_slope=0.2)
        close(y2, y2_ref, f"fp8 fwd mask_bits {cfg}")
    # data gradient (tiny adjoints, as in the train step: the block scales carry the range)
    if ci % 64 == 0 and ci > 64:
        dy = (torch.randn(osh, generator=g) * 1e-4 * torch.logspace(-1, 1, co)).to(torch.bfloat16)
        wd = (torch.randn(co * 9 * ci, generator=g) * 0.05).to(torch.bfloat16)
        mb = (torch.randint(0, 1 << 15, emu.bits_shape((N, H, W, ci)), generator=g)).to(torch.int16)
        dx_ref = torch.zeros(N, H, W, ci, dtype=torch.bfloat16)
        emu.conv_dgrad(cv, dy, wd, dx_ref, mask_bits=mb, mask_slope=0.2)
        dx = torch.zeros(N, H, W, ci, dtype=torch.bfloat16).cuda()
        hip.conv_dgrad(cv, dy.cuda(), wd.cuda(), dx, mask_bits=mb.cuda(), mask_slope=0.2)
        a, b = dx.float().cpu(), dx_ref.float()
        assert float((a - b).abs().max()) <= 1.6e-2 * float(b.abs().max()), (cfg, float((a - b).abs().max()), float(b.abs().max()))


def test_fp8_engine_iteration_matches_emulated_engine():
    """One critic + one generator iteration with the critic's wide convs in fp8, HIP against the emulated engine (bf16
    storage on both sides); F = 128 so that every critic layer but the first is eligible."""
    from downgan_amd import synthetic
    from downgan_amd.engine import HyperParams, TrainEngine
    from downgan_amd.layout import nchw_to_nhwc_padded
    torch.set_num_threads(8)
    B, S, F_, cin, nrb = 1, 16, 128, 2, 1
    pg, pc = synthetic.generator_params(F_, cin, 2, nrb), synthetic.critic_params(F_, 8 * S, 2)
    coarse, fine = synthetic.tiles(B, cin, S)
    alpha = torch.from_numpy(synthetic.alpha(B, 0))
    res = {}
    for name in ("emu", "hip"):
        ops = EmuOps("bf16", f8_critic=True) if name == "emu" else HipOps("bf16", f8_critic=True)
        eng = TrainEngine(ops, S, F_, cin, B, HyperParams(batch_size=B), num_res_blocks=nrb)
        eng.G.load_state_dict(pg); eng.C.load_state_dict(pc)
        if name == "emu":
            xc = nchw_to_nhwc_padded(torch.from_numpy(coarse), 16, torch.bfloat16)
            xf = nchw_to_nhwc_padded(torch.from_numpy(fine), 16, torch.bfloat16)
            al = alpha
        else:
            xc = ops.zeros(B, S, S, 16); ops.nchw_to_nhwc(torch.from_numpy(coarse).cuda(), xc)
            xf = ops.zeros(B, 8 * S, 8 * S, 16); ops.nchw_to_nhwc(torch.from_numpy(fine).cuda(), xf)
            al = alpha.cuda()
        eng.critic_iteration(xc, xf, al, apply_update=False, save_g=True)
        eng.generator_iteration(xc, xf, apply_update=False, reuse_fake=True)
        res[name] = eng.read_scalars(True)
    for k in ("c_real_mean", "c_fake_mean", "gp_ret", "critic_loss", "g_loss", "content_loss"):
        a, b = res["hip"][k], res["emu"][k]
        assert abs(a - b) <= 2e-2 * max(abs(b), 0.05), (k, a, b)


@pytest.mark.parametrize("f8", [False, True])
def test_pixel_shuffled_output_with_mxfp8_copy(f8):
    """An up-sampling conv (generator.py:69-81: conv 128 -> 512, LeakyReLU, PixelShuffle(2)) whose epilogue also writes the MXFP8
    form of the SHUFFLED tensor [N, 2H, 2W, 128] (scale bytes per destination pixel): bf16 kernel and fp8 kernel (net "T"), against
    the emulation and bit for bit against dg_quant_mxfp8 of the stored tensor; skip_y leaves the bf16 tensor alone and writes the
    same copy.  Ragged tile edges included."""
    g = torch.Generator().manual_seed(41)
    hip, emu = HipOps("bf16", f8_generator=True), EmuOps("bf16", f8_generator=True)
    cv = Conv(2, 24, 40, 128, 512, 1, True, net="T" if f8 else "")
    assert bool(hip.f8_eligible(cv, "fwd")) == f8
    x = torch.randn(cv.N, cv.H, cv.W, cv.Cin, generator=g).to(torch.bfloat16)
    w = (torch.randn(cv.Cout * 9 * cv.Cin, generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn(cv.Cout, generator=g)
    osh = hip.out_shape(cv)
    assert osh == (2, 48, 80, 128)
    qpair = lambda dev: (torch.zeros(osh, dtype=torch.uint8, device=dev), torch.zeros(osh[:-1] + (4,), dtype=torch.uint8, device=dev))
    y_ref, oq_ref = torch.zeros(osh, dtype=torch.bfloat16), qpair("cpu")
    emu.conv_fwd(cv, x, w, y_ref, bias=b, act=0.2, out_q=oq_ref)
    y, oq = torch.zeros(osh, dtype=torch.bfloat16).cuda(), qpair("cuda")
    hip.conv_fwd(cv, x.cuda(), w.cuda(), y, bias=b.cuda(), act=0.2, out_q=oq)
    assert hip.lib.dg_last_conv_kernels() == (32 if f8 else 8)
    close(y, y_ref, f"pixel-shuffled forward f8={f8}")
    q_ref, s_ref = hip.quant_mxfp8(y)
    assert torch.equal(oq[1], s_ref), int((oq[1] != s_ref).sum())
    assert torch.equal(oq[0], q_ref), int((oq[0] != q_ref).sum())
    y2 = torch.full(osh, 7.0, dtype=torch.bfloat16).cuda()
    oq2 = qpair("cuda")
    hip.conv_fwd(cv, x.cuda(), w.cuda(), y2, bias=b.cuda(), act=0.2, out_q=oq2, skip_y=True)
    assert bool((y2 == 7.0).all()) and torch.equal(oq2[0], oq[0]) and torch.equal(oq2[1], oq[1])
    # the consumer: a conv that reads the shuffled form (conv3.0 / the next up-sampling conv)
    if f8:
        cn = Conv(2, 48, 80, 128, 128, 1, False, net="T")
        wn = (torch.randn(128 * 9 * 128, generator=g) * 0.05).to(torch.bfloat16)
        z_ref, z = torch.zeros(2, 48, 80, 128, dtype=torch.bfloat16), torch.zeros(2, 48, 80, 128, dtype=torch.bfloat16).cuda()
        emu.conv_fwd(cn, y.cpu(), wn, z_ref, act=0.2, xq=tuple(t.cpu() for t in oq))
        hip.conv_fwd(cn, y2, wn.cuda(), z, act=0.2, xq=oq)            # y2 holds garbage: only the fp8 form is read
        close(z, z_ref, "consumer of the shuffled fp8 form")


@pytest.mark.parametrize("case", ["halo_bf16", "im2col_first_layer", "fp8_producer", "s2_dgrad_classes", "general_epilogue"])
def test_fused_mxfp8_output_equals_quantised_store(case):
    """dg_epilogue.out_q / out_qs: the MXFP8 copy a conv epilogue writes beside its bf16 output is bit-identical to
    dg_quant_mxfp8 of that output (so the consumer's results do not depend on who quantised)."""
    g = torch.Generator().manual_seed(31)
    f8 = case == "fp8_producer"
    hip = HipOps("bf16", f8_critic=True)
    if case == "im2col_first_layer":          # critic features.0: 2 real input channels, 128 outputs (critic.py:21-24)
        cv = Conv(2, 48, 80, 16, 128, 1, False, cin_real=2, net="C")
    elif case == "s2_dgrad_classes":
        cv = Conv(1, 64, 96, 128, 256, 2, False, net="C")
    else:
        cv = Conv(2, 40, 56, 128, 256, 1, False, net="C" if f8 else "")
    def qpair(shape):
        return torch.zeros(shape, dtype=torch.uint8).cuda(), torch.zeros(tuple(shape[:-1]) + (shape[-1] // 32,), dtype=torch.uint8).cuda()
    if case == "s2_dgrad_classes":
        dy = (torch.randn(hip.out_shape(cv), generator=g) * 1e-3).to(torch.bfloat16).cuda()
        wd = (torch.randn(cv.Cout * 9 * cv.Cin, generator=g) * 0.05).to(torch.bfloat16).cuda()
        mb = torch.randint(0, 1 << 15, hip.bits_shape((cv.N, cv.H, cv.W, cv.Cin)), generator=g).to(torch.int16).cuda()
        y = torch.zeros(cv.N, cv.H, cv.W, cv.Cin, dtype=torch.bfloat16).cuda()
        oq = qpair(y.shape)
        hip.conv_dgrad(cv, dy, wd, y, mask_bits=mb, mask_slope=0.2, out_q=oq)
    else:
        x = torch.randn(cv.N, cv.H, cv.W, cv.Cin, generator=g).to(torch.bfloat16)
        if cv.cin_real:
            x[..., cv.cin_real:] = 0
        w = (torch.randn(cv.Cout * 9 * cv.Cin, generator=g) * 0.05).to(torch.bfloat16).cuda()
        y = torch.zeros(hip.out_shape(cv), dtype=torch.bfloat16).cuda()
        oq = qpair(y.shape)
        ob = torch.zeros(hip.bits_shape(y.shape), dtype=torch.int16).cuda()
        if case == "general_epilogue":     # residual + activation: not one of the straight-line epilogue instances
            r1 = torch.randn(y.shape, generator=g).to(torch.bfloat16).cuda()
            hip.conv_fwd(cv, x.cuda(), w, y, act=0.2, r1=r1, s1=0.5, out_q=oq)
        else:
            b = torch.randn(cv.Cout, generator=g).cuda() if cv.cin_real else None
            hip.conv_fwd(cv, x.cuda(), w, y, bias=b, act=0.2, out_bits=ob, out_q=oq)
            assert hip.lib.dg_last_conv_kernels() == (32 if f8 else 16 if cv.cin_real else 8)
    q_ref, s_ref = hip.quant_mxfp8(y)
    assert float(y.float().abs().max()) > 0
    assert torch.equal(oq[1], s_ref), int((oq[1] != s_ref).sum())
    assert torch.equal(oq[0], q_ref), int((oq[0] != q_ref).sum())


def test_fp8_generator_trunk_matches_emulation():
    """HipOps(f8_generator=True): the generator's dense-block trunk forward on the fp8 kernel with slab-sliced fp8 forms
    (strided scale rows, epilogue-written slices) against the emulated engine, and its backward (fp8 data gradients of the dense
    blocks, bf16 weight gradients) against the emulated backward."""
    from downgan_amd import synthetic
    from downgan_amd.engine import NativeGenerator
    from downgan_amd.layout import nchw_to_nhwc_padded
    torch.set_num_threads(8)
    B, S, F_, cin, nrb = 2, 16, 128, 2, 2
    pg = synthetic.generator_params(F_, cin, 2, nrb)
    coarse, _ = synthetic.tiles(B, cin, S)
    emu = NativeGenerator(EmuOps("bf16", f8_generator=True), F_, cin, B, S, num_res_blocks=nrb)
    emu.load_state_dict(pg)
    ref = emu.forward(nchw_to_nhwc_padded(torch.from_numpy(coarse), 16, torch.bfloat16), save=True).float()
    ops = HipOps("bf16", f8_generator=True)
    G = NativeGenerator(ops, F_, cin, B, S, num_res_blocks=nrb)
    assert G.f8
    G.load_state_dict(pg)
    xc = ops.zeros(B, S, S, 16); ops.nchw_to_nhwc(torch.from_numpy(coarse).cuda(), xc)
    # The trunk (residual paths) agrees to accumulation order; behind it every further MXFP8 stage turns the 0.4 % the two engines
    # differ by into E4M3 code flips (~1.6 % of noise per stage): with the four tail layers in fp8 too (f8_gtail) the outputs differ
    # by 0.06 of the largest value where the trunk-only mode differs by 0.007, and by 0.09 from the bf16 generator
    # (tools/f8_tail_check.py).  Tight bound with the bf16 tail, loose with the fp8 tail -- whose layers are checked one by one,
    # bit for bit, in test_pixel_shuffled_output_with_mxfp8_copy.
    outs = []
    for save in (False, True):
        got = G.forward(xc, save=save).float().cpu()
        err = float((got - ref)[..., :2].abs().max()) / max(1e-6, float(ref[..., :2].abs().max()))
        assert G.f8_tail and err < 0.12, (save, err)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])              # the unsaved forward skips the bf16 up-sampled tensors, nothing else
    close(G.trunk, emu.trunk, "fp8 trunk", tol=3e-2)
    o2, e2 = HipOps("bf16", f8_generator=True), EmuOps("bf16", f8_generator=True)
    o2.f8_gtail = e2.f8_gtail = False
    G2, emu2 = NativeGenerator(o2, F_, cin, B, S, num_res_blocks=nrb), NativeGenerator(e2, F_, cin, B, S, num_res_blocks=nrb)
    G2.load_state_dict(pg); emu2.load_state_dict(pg)
    ref2 = emu2.forward(nchw_to_nhwc_padded(torch.from_numpy(coarse), 16, torch.bfloat16), save=False).float()
    got2 = G2.forward(xc, save=False).float().cpu()
    assert not G2.f8_tail and float((got2 - ref2)[..., :2].abs().max()) < 3e-2 * float(ref2[..., :2].abs().max())
    del G2, emu2
    # backward: the dense blocks' data gradients on the MXFP8 kernel too (f8_gbwd: adjoint-slab forms written by the epilogues
    # with the activation mask / the residual, quantised virtual packs), weight gradients bf16 from the saved slabs
    assert G.f8_bwd and emu.f8_bwd
    dfake = (torch.randn(G.fake.shape, generator=torch.Generator().manual_seed(5)) * (torch.arange(G.fake.shape[-1]) < 2)).to(torch.bfloat16)
    emu.P.zero_grad()
    emu.backward(nchw_to_nhwc_padded(torch.from_numpy(coarse), 16, torch.bfloat16), dfake)
    G.P.zero_grad()
    G.backward(xc, dfake.cuda())
    assert bool(torch.isfinite(G.P.g).all())
    ge, gg = emu.grad_dict(), G.grad_dict()
    # Yardsticks (tools/f8_gbwd_check.py on one box): the two engines' FORWARD states already differ by E4M3 code flips, which a
    # random dfake turns into 0.05-0.14 of rel-l2 on these gradients with bf16 data gradients too (conv3.0 0.05, dense blocks
    # 0.11-0.14); the fp8 data gradients add <= 0.015 to that, and the format's own error (fp8 vs bf16 data gradients on ONE
    # engine) is 0.042-0.063 on both engines alike.  So: the same format error on both sides, and nothing beyond the yardstick.
    ops16 = HipOps("bf16", f8_generator=True); ops16.f8_gbwd = False
    G16 = NativeGenerator(ops16, F_, cin, B, S, num_res_blocks=nrb)
    assert G16.f8 and not G16.f8_bwd
    G16.load_state_dict(pg)
    G16.forward(xc, save=True)
    G16.P.zero_grad(); G16.backward(xc, dfake.cuda())
    emu16_ops = EmuOps("bf16", f8_generator=True); emu16_ops.f8_gbwd = False
    emu16 = NativeGenerator(emu16_ops, F_, cin, B, S, num_res_blocks=nrb)
    emu16.load_state_dict(pg)
    xe = nchw_to_nhwc_padded(torch.from_numpy(coarse), 16, torch.bfloat16)
    emu16.forward(xe, save=True)
    emu16.P.zero_grad(); emu16.backward(xe, dfake)
    g16, e16 = G16.grad_dict(), emu16.grad_dict()
    rel = lambda a, b: float((a.float().cpu() - b.float().cpu()).norm() / max(1e-12, float(a.float().norm())))
    for name, a in ge.items():
        if not name.endswith("weight"):
            continue
        d8, d16 = rel(a, gg[name]), rel(e16[name], g16[name])
        assert d8 <= d16 + 0.03, (name, d8, d16)                                 # hip vs emulation: no worse than with bf16 data gradients
        if name.startswith("res_blocks"):
            fe, fh = rel(e16[name], a), rel(g16[name], gg[name])                 # the format's error, emulated / native
            assert 0.02 < fh < 0.09 and abs(fh - fe) < 0.25 * fe, (name, fe, fh)
        elif not name.startswith("conv1"):
            assert rel(g16[name], gg[name]) < 1e-5, name                          # upstream of the dense blocks' backward: untouched (atomic order only)


def test_fp8_generator_weight_gradients_second_iteration():
    """f8_gwgrad on the native engine: the first generator iteration collects the slabs' block exponents (bf16 weight-gradient kernel),
    the second writes the uniform-scale copies in the conv epilogues (forward: bias + LeakyReLU / residuals + copies; backward:
    activation mask / residual + copies) and runs dg_conv3x3_wgrad_dense_f8.  Against the same engine with f8_gwgrad off: bias
    gradients and everything outside the dense blocks agree to atomic order, weight gradients to the format's error -- the same
    error the emulated engine shows (tests/test_fp8_cpu.py)."""
    from downgan_amd import synthetic
    from downgan_amd.engine import NativeGenerator
    B, S, F_, cin, nrb = 2, 64, 128, 2, 1
    pg = synthetic.generator_params(F_, cin, 2, nrb, num_upsample=0)
    coarse, _ = synthetic.tiles(B, cin, S)
    res = {}
    for wg in (False, True):
        ops = HipOps("bf16", f8_generator=True)
        ops.f8_gwgrad = wg
        G = NativeGenerator(ops, F_, cin, B, S, num_res_blocks=nrb, num_upsample=0)
        assert G.f8_bwd and G.f8_wg == wg
        G.load_state_dict(pg)
        xc = ops.zeros(B, S, S, 16); ops.nchw_to_nhwc(torch.from_numpy(coarse).cuda(), xc)
        out = []
        for it in range(2):
            fake = G.forward(xc, save=True)
            dfake = (torch.randn(fake.shape, generator=torch.Generator().manual_seed(3 + it)) * (torch.arange(fake.shape[-1]) < 2)).to(torch.bfloat16).cuda()
            G.P.zero_grad()
            G.backward(xc, dfake)
            out.append({k: v.float().cpu() for k, v in G.grad_dict().items()})
        res[wg] = out
        assert wg == bool(G._u_ok)
    rel = lambda a, b: float((a - b).norm() / max(1e-20, float(a.norm())))
    for name, g0 in res[False][0].items():
        assert rel(g0, res[True][0][name]) < 1e-5, name                              # first iteration: bf16 kernel in both
    worst = 0.0
    for name, ga in res[False][1].items():
        d = rel(ga, res[True][1][name])
        if name.startswith("res_blocks") and name.endswith("weight"):
            assert 1e-4 < d < 0.08, (name, d)
            worst = max(worst, d)
        else:
            assert d < 1e-4, (name, d)
    assert worst > 1e-3


def test_dense_block_data_gradient_on_slab_slices_fp8():
    """One virtual data gradient of a dense block (engine.py NativeGenerator.backward; autograd of generator.py:24-41) on the MXFP8
    kernel: the adjoint operand is a channel slice [kF, 5F) of the slab's fp8 form with strided scale rows, the epilogue applies
    the ACTIVATION mask of a slab slice and writes the bf16 slice plus its MXFP8 copy into slice k-1 (straight-line instance 288);
    and the block's last one: residual + copy into another slab's slice (264).  Against the emulation on the same quantised
    operands (accumulation order only) and, for the copies, dg_quant_mxfp8 of the stored slice bit for bit."""
    B, S, F_ = 2, 24, 128
    g = torch.Generator().manual_seed(77)
    hip, emu = HipOps("bf16", f8_generator=True), EmuOps("bf16", f8_generator=True)
    us = (torch.randn(B, S, S, 5 * F_, generator=g) * 1e-3 * torch.logspace(-1, 1, 5 * F_)).to(torch.bfloat16)
    slab = torch.randn(B, S, S, 5 * F_, generator=g).to(torch.bfloat16)
    usd = us.cuda()
    usq = (torch.zeros(B, S, S, 5 * F_, dtype=torch.uint8).cuda(), torch.zeros(B, S, S, 5 * F_ // 32, dtype=torch.uint8).cuda())
    hip.quant_mxfp8(usd, *usq)
    usq_e = tuple(t.cpu().clone() for t in usq)
    for k in (3, 0):
        cv = Conv(B, S, S, F_, (5 - k) * F_, net="G")
        assert hip.f8_eligible(cv, "dgrad")
        wd = (torch.randn(F_ * 9 * (5 - k) * F_, generator=g) * 0.05).to(torch.bfloat16)
        wq = hip.quant_mxfp8(wd.cuda().view(F_ * 9, (5 - k) * F_))
        wq_e = tuple(t.cpu() for t in wq)
        sl = lambda t, c0, c1: (t[0][..., c0:c1], t[1][..., c0 // 32:c1 // 32])
        if k:       # u_k = LeakyReLU'(b_k) * sum ...: slice k-1 of the SAME slab
            ep = lambda dev: dict(mask=(slab.cuda() if dev else slab)[..., k * F_:(k + 1) * F_], mask_slope=0.2)
            out_h, out_e = usd[..., (k - 1) * F_:k * F_], us[..., (k - 1) * F_:k * F_]
            oq_h, oq_e = sl(usq, (k - 1) * F_, k * F_), sl(usq_e, (k - 1) * F_, k * F_)
        else:       # d x_drb: residual of the block's own u5, stored into another slab's top slice
            nxt_h = torch.zeros(B, S, S, 5 * F_, dtype=torch.bfloat16).cuda(); nxt_e = torch.zeros(B, S, S, 5 * F_, dtype=torch.bfloat16)
            nq_h = (torch.zeros(B, S, S, 5 * F_, dtype=torch.uint8).cuda(), torch.zeros(B, S, S, 5 * F_ // 32, dtype=torch.uint8).cuda())
            nq_e = tuple(t.cpu().clone() for t in nq_h)
            ep = lambda dev: dict(r1=(usd if dev else us)[..., 4 * F_:], s1=0.2)
            out_h, out_e = nxt_h[..., 4 * F_:], nxt_e[..., 4 * F_:]
            oq_h, oq_e = sl(nq_h, 4 * F_, 5 * F_), sl(nq_e, 4 * F_, 5 * F_)
        emu.conv_dgrad(cv, us[..., k * F_:], wd, out_e, xq=sl(usq_e, k * F_, 5 * F_), wq=wq_e, out_q=oq_e, **ep(False))
        hip.conv_dgrad(cv, usd[..., k * F_:], wd.cuda(), out_h, xq=sl(usq, k * F_, 5 * F_), wq=wq, out_q=oq_h, **ep(True))
        assert hip.lib.dg_last_conv_kernels() == 32
        a, b = out_h.float().cpu(), out_e.float()
        assert float(b.abs().max()) > 0 and float((a - b).abs().max()) <= 1.6e-2 * float(b.abs().max()), (k, float((a - b).abs().max()), float(b.abs().max()))
        q_ref, s_ref = hip.quant_mxfp8(out_h.contiguous())
        assert torch.equal(oq_h[1].contiguous(), s_ref), (k, int((oq_h[1] != s_ref).sum()))
        assert torch.equal(oq_h[0].contiguous(), q_ref), (k, int((oq_h[0] != q_ref).sum()))
        if k:       # the rest of the slab's form is untouched, and the new slice feeds the next data gradient
            us = usd.cpu(); usq_e = tuple(t.cpu().clone() for t in usq)


def test_mirrors_accept_fp8_dtype():
    """Generator / Critic / WassersteinGAN mirrors with dtype="fp8": the drop-in API reaches the MXFP8 path."""
    import math
    from downgan_amd import synthetic
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    B, S, F_ = 2, 16, 128
    G = Generator(F_, 8 * S, 2, 2, num_res_blocks=1, dtype="fp8")
    C = Critic(F_, 8 * S, 2, dtype="fp8")
    tr = WassersteinGAN(G, C)
    coarse, fine = synthetic.tiles(B, 2, S)
    out = tr._critic_train_iteration(torch.from_numpy(coarse), torch.from_numpy(fine), alpha=synthetic.alpha(B, 0), _keep_g=True)
    out.update(tr._generator_train_iteration(torch.from_numpy(coarse), torch.from_numpy(fine), _reuse_g=True))
    assert tr._engine.C.f8 and tr._engine.G.f8
    assert all(math.isfinite(v) for v in out.values()), out


def _quant_uniform(t, exps):
    """E4M3 copy of t [.., C] with one exponent byte per 32-channel block of the WHOLE tensor (q = t / 2^(e - 127), saturated at
    +-448, round to nearest even -- torch's float8_e4m3fn cast), and the fp32 values it stands for."""
    C = t.shape[-1]
    scale = torch.pow(2.0, exps.to(torch.float32) - 127.0).repeat_interleave(32)[:C]
    q = (t.float() / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), q.float() * scale


@pytest.mark.parametrize("cfg", [(2, 16, 64, 128, 128, 1), (1, 8, 128, 256, 128, 1), (1, 12, 64, 128, 384, 1), (3, 5, 64, 256, 256, 1),
                                 (2, 16, 128, 128, 128, 2), (1, 6, 256, 256, 128, 2), (1, 10, 128, 128, 256, 2)])
def test_wgrad_f8_uniform_scales(cfg):
    """dg_conv3x3_wgrad_f8 (contraction over pixels on v_mfma_scale_f32_32x32x64_f8f6f4; operands E4M3 with one exponent per
    32-channel block of the whole tensor) against the emulation's fp32 weight gradient of the DEQUANTISED operands: products of two
    E4M3 values are exact in fp32, so only the summation order differs (1e-5 of the largest entry).  Accumulates into dw.
    Reference math: autograd of DoWnGAN/networks/critic.py:34-88 (weight gradient of a 3x3 conv, padding 1)."""
    from oracle.emu_ops import EmuOps
    N, H, W, ci, co, st = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    hip, emu = HipOps("bf16"), EmuOps("f32")
    cv = Conv(N, H, W, ci, co, st)
    x = torch.randn(N, H, W, ci, generator=g) * torch.logspace(-2, 1, ci).view(1, 1, 1, ci)        # channels of very different size
    dy = torch.randn(N, H // st, W // st, co, generator=g) * 0.01
    # exponents: the block's floor(log2 amax) - 8 + 127 (the OCP MX rule applied to the whole tensor), one block deliberately too small (saturates)
    def exps(t):
        am = t.abs().reshape(-1, t.shape[-1] // 32, 32).amax(dim=(0, 2))
        return (torch.floor(torch.log2(am)) - 8 + 127).to(torch.uint8)
    ex, ey = exps(x), exps(dy)
    ex[0] -= 2
    xq, xd = _quant_uniform(x, ex)
    dq, dd = _quant_uniform(dy, ey)
    dw_ref = torch.randn(co * 9 * ci, generator=g) * 0.1
    dw = dw_ref.clone().cuda()
    emu.conv_wgrad(cv, xd, dd, dw_ref)
    hip.conv_wgrad_f8(cv, xq.cuda(), ex.cuda(), dq.cuda(), ey.cuda(), dw)
    scale = float(dw_ref.abs().max())
    err = float((dw.cpu() - dw_ref).abs().max())
    assert err <= 1e-5 * scale * 8, (cfg, err, scale)
    # operands that are channel slices of wider tensors (pixel stride > channels)
    xw = torch.zeros(N, H, W, ci + 128, dtype=torch.uint8); xw[..., 64:64 + ci] = xq
    dw2 = torch.zeros(co * 9 * ci).cuda()
    hip.conv_wgrad_f8(cv, xw.cuda()[..., 64:64 + ci], ex.cuda(), dq.cuda(), ey.cuda(), dw2)
    dw3 = torch.zeros(co * 9 * ci); emu.conv_wgrad(cv, xd, dd, dw3)
    assert float((dw2.cpu() - dw3).abs().max()) <= 1e-5 * float(dw3.abs().max()) * 8, cfg
    # shapes the kernel does not take are refused, not mis-computed
    for bad in (Conv(N, H, 32 * st, ci, co, st), Conv(N, H, W, 64, co, st)):
        with pytest.raises((RuntimeError, AssertionError)):
            hip.conv_wgrad_f8(bad, torch.zeros(bad.N, bad.H, bad.W, bad.Cin, dtype=torch.uint8).cuda(), torch.zeros(max(bad.Cin // 32, 1), dtype=torch.uint8).cuda(),
                              torch.zeros(bad.N, bad.Ho, bad.Wo, co, dtype=torch.uint8).cuda(), ey.cuda(), torch.zeros(co * 9 * bad.Cin).cuda())


@pytest.mark.parametrize("cfg", [(2, 16, 64, 5), (1, 9, 128, 5), (3, 7, 64, 3)])
def test_wgrad_dense_f8_uniform_scales(cfg):
    """dg_conv3x3_wgrad_dense_f8: the weight gradients of all convs of a dense block (autograd of DoWnGAN/networks/generator.py:24-41;
    conv k reads slab channels [0, k * 128), its adjoint is slice k - 1 of the adjoint slab) in one launch of the fp8 kernel, against
    the emulation's fp32 weight gradients of the dequantised slabs (summation order only); accumulates; deterministic mode agrees."""
    from oracle.emu_ops import EmuOps
    N, H, W, n = cfg
    F_ = 128
    g = torch.Generator().manual_seed(sum(cfg))
    hip, emu = HipOps("bf16"), EmuOps("f32")
    cvs = [Conv(N, H, W, k * F_, F_, net="G") for k in range(1, n + 1)]
    slab = torch.randn(N, H, W, n * F_, generator=g) * torch.logspace(-1, 1, n * F_)
    us = torch.randn(N, H, W, n * F_, generator=g) * 1e-3 * torch.logspace(0, 1, n * F_)
    def exps(t):
        am = t.abs().reshape(-1, t.shape[-1] // 32, 32).amax(dim=(0, 2))
        return (torch.floor(torch.log2(am)) - 8 + 127 + 1).to(torch.uint8)
    ex, eu = exps(slab), exps(us)
    sq, _ = _quant_uniform(slab, ex)
    uq, _ = _quant_uniform(us, eu)
    refs = [torch.randn(F_ * 9 * k * F_, generator=g) * 1e-3 for k in range(1, n + 1)]
    dws = [r.clone().cuda() for r in refs]
    emu.conv_wgrad_dense_f8(cvs, sq, ex, uq, eu, refs)
    hip.conv_wgrad_dense_f8(cvs, sq.cuda(), ex.cuda(), uq.cuda(), eu.cuda(), dws)
    for k in range(n):
        scale = float(refs[k].abs().max())
        err = float((dws[k].cpu() - refs[k]).abs().max())
        assert err <= 1e-5 * scale * 8, (cfg, k, err, scale)
    # the block's bias gradients in this mode: one pass of column sums over the bf16 adjoint slab (dg_colsum_multi), accumulated
    usb = us.to(torch.bfloat16)
    db0 = [torch.randn(F_, generator=g) for _ in range(n)]
    dbs = [t.clone().cuda() for t in db0]
    hip.colsum_multi(usb.cuda(), dbs)
    for k in range(n):
        ref = db0[k] + usb[..., k * F_:(k + 1) * F_].float().reshape(-1, F_).sum(0)
        assert float((dbs[k].cpu() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max())), (cfg, k)
    det = HipOps("bf16", deterministic=True)
    try:
        d1 = [torch.zeros(F_).cuda() for _ in range(n)]; d2 = [torch.zeros(F_).cuda() for _ in range(n)]
        det.colsum_multi(usb.cuda(), d1); det.colsum_multi(usb.cuda(), d2)
        assert all(torch.equal(a, b) for a, b in zip(d1, d2))
        assert all(float((d1[k].cpu() - usb[..., k * F_:(k + 1) * F_].float().reshape(-1, F_).sum(0)).abs().max()) <= 1e-4 for k in range(n))
        runs = []
        for _ in range(2):
            d2 = [torch.zeros_like(r).cuda() for r in refs]
            det.conv_wgrad_dense_f8(cvs, sq.cuda(), ex.cuda(), uq.cuda(), eu.cuda(), d2)
            runs.append(torch.cat([t.cpu() for t in d2]))
        assert torch.equal(runs[0], runs[1])
        z = [torch.zeros_like(r) for r in refs]
        emu.conv_wgrad_dense_f8(cvs, sq, ex, uq, eu, z)
        zc = torch.cat(z)
        assert float((runs[0] - zc).abs().max()) <= 1e-5 * float(zc.abs().max()) * 8
    finally:
        det.close()
    with pytest.raises((RuntimeError, AssertionError)):                       # rows that are not a multiple of 64 pixels: refused
        bad = [Conv(N, H, 32, k * F_, F_) for k in range(1, n + 1)]
        hip.conv_wgrad_dense_f8(bad, torch.zeros(N, H, 32, n * F_, dtype=torch.uint8).cuda(), ex.cuda(), torch.zeros(N, H, 32, n * F_, dtype=torch.uint8).cuda(), eu.cuda(), dws)


@pytest.mark.parametrize("case", ["fp8_s2_forward", "fp8_s2_dgrad_classes", "fp8_s1_forward_mask_bits", "bf16_halo", "general_epilogue"])
def test_fused_uniform_scale_copy_equals_quantised_store(case):
    """dg_epilogue.out_u / out_ue: the uniform-scale E4M3 copy (operand of dg_conv3x3_wgrad_f8) a conv epilogue writes beside its
    bf16 output and the MXFP8 copy is bit-identical to quantising the STORED tensor with the given per-block exponents
    (oracle/emu_ops.py::uq_quant) -- on the launches that produce the critic's activations (stride-2 fp8 forward), adjoints
    (merged stride-2 fp8 data gradient) and the penalty's tangents (fp8 forward with the 1-bit mask)."""
    from oracle.emu_ops import EmuOps
    g = torch.Generator().manual_seed(77)
    f8 = case.startswith("fp8")
    hip = HipOps("bf16", f8_critic=True)
    st = 2 if "s2" in case else 1
    cv = Conv(2, 32, 48, 128, 256, st, False, net="C" if f8 else "")
    qpair = lambda shape: (torch.zeros(shape, dtype=torch.uint8).cuda(), torch.zeros(tuple(shape[:-1]) + (shape[-1] // 32,), dtype=torch.uint8).cuda())
    if case == "fp8_s2_dgrad_classes":
        dy = (torch.randn(hip.out_shape(cv), generator=g) * 1e-3).to(torch.bfloat16).cuda()
        wd = (torch.randn(cv.Cout * 9 * cv.Cin, generator=g) * 0.05).to(torch.bfloat16).cuda()
        mb = torch.randint(0, 1 << 15, hip.bits_shape((cv.N, cv.H, cv.W, cv.Cin)), generator=g).to(torch.int16).cuda()
        y = torch.zeros(cv.N, cv.H, cv.W, cv.Cin, dtype=torch.bfloat16).cuda()
        exps = torch.tensor([127 - 12, 127 - 14, 127 - 13, 127 - 20], dtype=torch.uint8)      # the last block saturates
        oq, u = qpair(y.shape), torch.zeros(y.shape, dtype=torch.uint8).cuda()
        hip.conv_dgrad(cv, dy, wd, y, mask_bits=mb, mask_slope=0.2, out_q=oq, out_u=(u, exps.cuda()))
        assert hip.lib.dg_last_conv_kernels() == 32
    else:
        x = torch.randn(cv.N, cv.H, cv.W, cv.Cin, generator=g).to(torch.bfloat16).cuda()
        w = (torch.randn(cv.Cout * 9 * cv.Cin, generator=g) * 0.05).to(torch.bfloat16).cuda()
        y = torch.zeros(hip.out_shape(cv), dtype=torch.bfloat16).cuda()
        exps = (127 - 7 + torch.arange(cv.Cout // 32) % 3).to(torch.uint8)
        exps[1] = 127 - 12                                                                    # saturates
        oq, u = qpair(y.shape), torch.zeros(y.shape, dtype=torch.uint8).cuda()
        ob = torch.zeros(hip.bits_shape(y.shape), dtype=torch.int16).cuda()
        if case == "general_epilogue":
            r1 = torch.randn(y.shape, generator=g).to(torch.bfloat16).cuda()
            hip.conv_fwd(cv, x, w, y, act=0.2, r1=r1, s1=0.5, out_q=oq, out_u=(u, exps.cuda()))
        elif case == "fp8_s1_forward_mask_bits":
            mb = torch.randint(0, 1 << 15, hip.bits_shape(y.shape), generator=g).to(torch.int16).cuda()
            hip.conv_fwd(cv, x, w, y, mask_bits=mb, mask_slope=0.2, out_q=oq, out_u=(u, exps.cuda()))
        else:
            hip.conv_fwd(cv, x, w, y, act=0.2, out_bits=ob, out_q=oq, out_u=(u, exps.cuda()))
        assert hip.lib.dg_last_conv_kernels() == (32 if f8 else 8)
    q_ref, _ = EmuOps.uq_quant(y.cpu(), exps)
    assert float(y.float().abs().max()) > 0 and int((q_ref & 0x7f == 0x7e).sum()) > 0          # something did saturate at 448
    assert torch.equal(u.cpu(), q_ref), int((u.cpu() != q_ref).sum())
    s_ref = hip.quant_mxfp8(y)
    assert torch.equal(oq[0], s_ref[0]) and torch.equal(oq[1], s_ref[1])                       # the MXFP8 copy is unchanged by it


def test_block_exp_max_kernel():
    g = torch.Generator().manual_seed(5)
    hip = HipOps("bf16")
    for rows, nb, ld in ((1000, 4, 4), (77777, 8, 8), (4096, 32, 32), (333, 4, 20), (50000, 20, 20)):
        sc = torch.randint(90, 140, (rows, ld), generator=g).to(torch.uint8)
        r, b = int(torch.randint(0, rows, (1,), generator=g)), int(torch.randint(0, nb, (1,), generator=g))
        sc[r, b] = 200
        dev = sc.cuda()
        out = torch.zeros(nb, dtype=torch.uint8).cuda()
        for margin in (0, 1):
            hip.block_exp_max(dev[:, :nb], out, margin=margin)
            assert torch.equal(out.cpu(), (sc[:, :nb].int().amax(0) + margin).to(torch.uint8)), (rows, nb, ld, margin)
        assert int(hip._exp_scratch.abs().sum()) == 0                  # the scratch is left zero


def test_exponents_fall_by_at_most_one_per_update():
    """Passes over one buffer alternate between inputs of different size (real / generated samples); exponents taken from the smaller
    one would saturate the larger one's uniform-scale copy: dg_block_exp_max and dg_exp_from_amax lower an exponent by at most one per
    call, raise it at once (oracle/emu_ops.py::_exp_decay)."""
    hip, emu = HipOps("bf16"), EmuOps("f32")
    big = torch.full((64, 8), 130, dtype=torch.uint8); small = torch.full((64, 8), 120, dtype=torch.uint8)
    out, ref = torch.zeros(8, dtype=torch.uint8).cuda(), torch.zeros(8, dtype=torch.uint8)
    for sc, want in ((big, 131), (small, 130), (small, 129), (big, 131), (small, 130)):
        hip.block_exp_max(sc.cuda(), out, margin=1); emu.block_exp_max(sc, ref, margin=1)
        assert torch.equal(out.cpu(), ref) and int(out[0]) == want, (out.cpu(), ref, want)
    # the census form: bit patterns of the largest magnitudes; cleared by the call
    f2b = lambda v: torch.tensor(v, dtype=torch.float32).view(torch.int32)
    out2, ref2 = torch.zeros(4, dtype=torch.uint8).cuda(), torch.zeros(4, dtype=torch.uint8)
    for vals in ([3.0, 0.5, 100.0, 1e-3], [0.01, 0.5, 0.0, 2.0], [0.01, 0.6, 1e30, 0.0]):
        a, b = f2b(vals).cuda(), f2b(vals).clone()
        hip.exp_from_amax(a, out2, margin=1); emu.exp_from_amax(b, ref2, margin=1)
        assert torch.equal(out2.cpu(), ref2), (vals, out2.cpu(), ref2)
        assert int(a.abs().sum()) == 0
    assert int(ref2[1]) == 127 - 1 - 8 + 1 and int(ref2[2]) == 127 + 99 - 8 + 1


@pytest.mark.parametrize("tangent", [False, True])
def test_first_layer_uniform_scale_copy_alone(tangent):
    """critic features.0 (critic.py:21-24) writing ONLY the uniform-scale copy of its output (dg_epilogue.out_u without out_q, skip_y)
    plus the magnitude census (out_amax): the copy equals dg_quant_uniform of the tensor a plain launch stores, the census the bit
    patterns of its per-block maxima, the mask bits are unchanged; and the consumer -- layer 1's MXFP8 stride-2 conv reading the copy
    with the block exponents as ONE scale row for every pixel (dg_f8_operands.ldxs < 0) -- against the emulation.  `tangent`: the
    penalty's first tangent (mask_bits instead of activation + out_bits)."""
    g = torch.Generator().manual_seed(51)
    hip, emu = HipOps("bf16", f8_critic=True), EmuOps("bf16", f8_critic=True)
    cv = Conv(2, 48, 80, 16, 128, 1, False, cin_real=2, net="C")
    x = torch.randn(cv.N, cv.H, cv.W, 16, generator=g).to(torch.bfloat16); x[..., 2:] = 0
    w = (torch.randn(128 * 9 * 16, generator=g) * 0.3).to(torch.bfloat16).cuda()
    b = torch.randn(128, generator=g).cuda()
    osh = (cv.N, cv.H, cv.W, 128)
    y = torch.zeros(osh, dtype=torch.bfloat16).cuda()
    bits = torch.zeros(hip.bits_shape(osh), dtype=torch.int16).cuda()
    mb = torch.randint(0, 1 << 15, hip.bits_shape(osh), generator=g).to(torch.int16).cuda()
    ep = dict(mask_bits=mb, mask_slope=0.2) if tangent else dict(bias=b, act=0.2, out_bits=bits)
    hip.conv_fwd(cv, x.cuda(), w, y, **ep)
    assert hip.lib.dg_last_conv_kernels() == 16
    am = y.float().abs().reshape(-1, 4, 32).amax(dim=(0, 2))
    exps = ((am.view(torch.int32) >> 23) & 0xff).to(torch.uint8) - 8 + 1
    exps[3] -= 3                                                    # one block too small: saturates at +-448
    u_ref = torch.zeros(osh, dtype=torch.uint8).cuda()
    hip.quant_uniform(y, u_ref, exps)
    u = torch.zeros(osh, dtype=torch.uint8).cuda()
    census = torch.zeros(4, dtype=torch.int32).cuda()
    y2 = torch.full(osh, 3.0, dtype=torch.bfloat16).cuda()
    bits2 = torch.zeros_like(bits)
    ep2 = dict(mask_bits=mb, mask_slope=0.2) if tangent else dict(bias=b, act=0.2, out_bits=bits2)
    hip.conv_fwd(cv, x.cuda(), w, y2, out_u=(u, exps), out_amax=census, skip_y=True, **ep2)
    assert hip.lib.dg_last_conv_kernels() == 16
    assert bool((y2 == 3.0).all()) and torch.equal(u, u_ref), int((u != u_ref).sum())
    assert torch.equal(census.cpu(), am.cpu().view(torch.int32))
    if not tangent:
        assert torch.equal(bits2, bits)
    # a second launch only raises the census
    hip.conv_fwd(cv, (x * 0.5).cuda(), w, y2, out_u=(u, exps), out_amax=census, skip_y=True, **ep2)
    if tangent:
        assert torch.equal(census.cpu(), am.cpu().view(torch.int32))
    # consumer: layer 1 (128 -> 128, stride 2) on the MXFP8 kernel with the uniform-scale source
    hip.quant_uniform(y, u, exps)
    c1 = Conv(2, 48, 80, 128, 128, 2, False, net="C")
    w1 = (torch.randn(128 * 9 * 128, generator=g) * 0.05).to(torch.bfloat16)
    z_ref, z = torch.zeros(2, 24, 40, 128, dtype=torch.bfloat16), torch.zeros(2, 24, 40, 128, dtype=torch.bfloat16).cuda()
    emu.conv_fwd(c1, y.cpu(), w1, z_ref, act=0.2, xq=(u.cpu(), exps.cpu()))
    hip.conv_fwd(c1, y2, w1.cuda(), z, act=0.2, xq=(u, exps))
    assert hip.lib.dg_last_conv_kernels() == 32
    close(z, z_ref, "layer 1 on the uniform-scale copy")
    # other launches refuse both features instead of ignoring them
    cw = Conv(1, 16, 16, 128, 128, 1, False)
    xw = torch.zeros(1, 16, 16, 128, dtype=torch.bfloat16).cuda(); yw = torch.zeros_like(xw); uw = torch.zeros(1, 16, 16, 128, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError):
        hip.conv_fwd(cw, xw, w1.cuda(), yw, out_u=(uw, exps))
    with pytest.raises(RuntimeError):
        hip.conv_fwd(cw, xw, w1.cuda(), yw, out_amax=census)


def test_quant_uniform_kernel():
    """dg_quant_uniform == the emulation's uq_quant, bit for bit (bf16 and fp32 sources, a saturating block, a poisoned block)."""
    from oracle.emu_ops import EmuOps
    g = torch.Generator().manual_seed(9)
    hip = HipOps("bf16")
    for dt in (torch.bfloat16, torch.float32):
        x = (torch.randn(3, 7, 5, 256, generator=g) * torch.logspace(-3, 1, 256)).to(dt)
        x[1, 2, 3, 70] = float("nan")
        exps = torch.tensor([118, 120, 121, 122, 125, 126, 128, 124], dtype=torch.uint8)
        q = torch.zeros(x.shape, dtype=torch.uint8).cuda()
        hip.quant_uniform(x.cuda(), q, exps.cuda())
        ref, _ = EmuOps.uq_quant(x, exps)
        assert torch.equal(q.cpu(), ref), int((q.cpu() != ref).sum())


def test_fp8_weight_gradient_quality_at_cfg2_shapes():
    """GATE at BASELINE configs[1] shapes (batch 2): the critic's parameter gradients of the first iteration in fp8 mode against the
    fp32-parity mode, with the bf16 and with the fp8 weight-gradient kernels (tools/fp8_drift.py::first_step_gradients).  At the
    initial weights the gradient is a nearly cancelling difference of the real and the generated batch's terms, which amplifies every
    rounding (more so the fewer samples there are): bf16 is 2-13 % off (cosine >= 0.99), the MXFP8 activations / adjoints 11-43 %
    (cosine 0.907-0.997 at batch 2, 0.82-0.995 at batch 1; profiles/fp8_drift_cfg2.json).  What the fp8 WEIGHT GRADIENT (uniform-scale
    E4M3 operands, delayed per-block exponents) adds on top is gated: at most 0.02 of cosine on any conv weight (observed <= 0.016),
    none below 0.88 (observed >= 0.911)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fp8_drift", os.path.join(root, "tools", "fp8_drift.py"))
    fd = importlib.util.module_from_spec(spec); spec.loader.exec_module(fd)
    res = fd.first_step_gradients(2, 128, 128, 16)
    assert res.pop("_layers_on_the_fp8_weight_gradient_kernel") == [False, True, True, True, True, True, True, True]
    try:
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "fp8_wgrad_quality_cfg2.json"), "w") as f:
            json.dump(res, f, indent=1)
    except OSError:
        pass
    for k, v in res.items():
        assert v["bf16"]["cosine"] >= 0.985, (k, v)
        assert v["fp8"]["cosine"] >= v["fp8_bf16_wgrad"]["cosine"] - 0.02, (k, v)
        # (biases: sums over all pixels of a cancelling difference; since the generator's tail runs in fp8 too its `fake` differs from the
        # fp32 engine's by 5 % and `features.0.bias` reads 0.852-0.865 where it read 0.907 with a bf16 tail: profiles/fp8_wgrad_quality_cfg2.json)
        assert v["fp8"]["cosine"] >= (0.88 if k.startswith("features.") and k.endswith(".weight") else 0.80), (k, v)


@pytest.mark.parametrize("case", ["fp8_s2_forward", "fp8_s2_dgrad_classes", "fp8_s1_forward_mask_bits", "fp8_forward_no_u"])
def test_skip_y_leaves_the_output_alone_and_writes_the_same_copies(case):
    """dg_epilogue.skip_y (fp8 mode: a bf16 tensor whose only readers are the next fp8 conv, the fp8 weight gradient and the mask
    bits is not stored at all): the MXFP8 copy, the uniform-scale copy and the out_bits of such a launch are bit-identical to the
    ones of the launch that stores y, and y keeps whatever it held."""
    g = torch.Generator().manual_seed(78)
    hip = HipOps("bf16", f8_critic=True)
    st = 2 if "s2" in case else 1
    cv = Conv(2, 32, 48, 128, 256, st, False, net="C")
    qpair = lambda shape: (torch.zeros(shape, dtype=torch.uint8).cuda(), torch.zeros(tuple(shape[:-1]) + (shape[-1] // 32,), dtype=torch.uint8).cuda())
    out = {}
    for skip in (False, True):
        gg = torch.Generator().manual_seed(79)
        if case == "fp8_s2_dgrad_classes":
            dy = (torch.randn(hip.out_shape(cv), generator=gg) * 1e-3).to(torch.bfloat16).cuda()
            wd = (torch.randn(cv.Cout * 9 * cv.Cin, generator=gg) * 0.05).to(torch.bfloat16).cuda()
            mb = torch.randint(0, 1 << 15, hip.bits_shape((cv.N, cv.H, cv.W, cv.Cin)), generator=gg).to(torch.int16).cuda()
            y = torch.full((cv.N, cv.H, cv.W, cv.Cin), 7.0, dtype=torch.bfloat16).cuda()
            exps = torch.tensor([127 - 12, 127 - 14, 127 - 13, 127 - 15], dtype=torch.uint8).cuda()
            oq, u = qpair(y.shape), torch.zeros(y.shape, dtype=torch.uint8).cuda()
            hip.conv_dgrad(cv, dy, wd, y, mask_bits=mb, mask_slope=0.2, out_q=oq, out_u=(u, exps), skip_y=skip)
            ob = None
        else:
            x = torch.randn(cv.N, cv.H, cv.W, cv.Cin, generator=gg).to(torch.bfloat16).cuda()
            w = (torch.randn(cv.Cout * 9 * cv.Cin, generator=gg) * 0.05).to(torch.bfloat16).cuda()
            y = torch.full(hip.out_shape(cv), 7.0, dtype=torch.bfloat16).cuda()
            exps = (127 - 7 + torch.arange(cv.Cout // 32) % 3).to(torch.uint8).cuda()
            oq, u = qpair(y.shape), torch.zeros(y.shape, dtype=torch.uint8).cuda()
            ob = torch.zeros(hip.bits_shape(y.shape), dtype=torch.int16).cuda()
            if case == "fp8_s1_forward_mask_bits":
                mb = torch.randint(0, 1 << 15, hip.bits_shape(y.shape), generator=gg).to(torch.int16).cuda()
                hip.conv_fwd(cv, x, w, y, mask_bits=mb, mask_slope=0.2, out_q=oq, out_u=(u, exps), skip_y=skip)
                ob = None
            elif case == "fp8_forward_no_u":
                hip.conv_fwd(cv, x, w, y, act=0.2, out_bits=ob, out_q=oq, skip_y=skip)
            else:
                hip.conv_fwd(cv, x, w, y, act=0.2, out_bits=ob, out_q=oq, out_u=(u, exps), skip_y=skip)
        assert hip.lib.dg_last_conv_kernels() == 32
        out[skip] = (y, oq, u, ob)
    y0, q0, u0, b0 = out[False]
    y1, q1, u1, b1 = out[True]
    assert float((y0.float() - 7.0).abs().max()) > 0 and bool((y1 == 7.0).all())
    assert torch.equal(q0[0], q1[0]) and torch.equal(q0[1], q1[1]) and torch.equal(u0, u1)
    if b0 is not None:
        assert torch.equal(b0, b1) and int(b0.abs().sum()) > 0
    with pytest.raises((RuntimeError, AssertionError)):           # nothing would be left of the launch
        hip.conv_fwd(cv, torch.zeros(cv.N, cv.H, cv.W, cv.Cin, dtype=torch.bfloat16).cuda(), torch.zeros(cv.Cout * 9 * cv.Cin, dtype=torch.bfloat16).cuda(),
                     torch.zeros(hip.out_shape(cv), dtype=torch.bfloat16).cuda(), skip_y=True)
