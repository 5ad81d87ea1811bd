"""The fp8 quantisers on the tables of tests/fp8_quant_ref.py, byte for byte against its integer reference: the stand-alone
kernels (dg_quant_uniform, dg_quant_mxfp8; bf16 and fp32 sources, contiguous and as channel slices between sentinels), the fused
copies of the bf16 conv epilogues (out_q, out_u, out_amax; the reference is applied to the STORED output read back, not to the
stand-alone kernel's bytes) and the exponent chain (dg_block_exp_max, dg_block_exp_max_batch, dg_exp_from_amax).

Where the reference is +-0 either zero byte is accepted; everything else is equality of bytes.  Every fused launch asserts the
dispatch probe of the path it is there for and, on the halo kernels, the epilogue key computed from its flags: whether it runs one
of the straight-line instances or the general run-time-flag one (the probe is the same for both).  tests/test_fp8_quant_exact_cpu.py runs the same tables through the CPU oracle.

Out of scope: the second grid-stride trip of the stand-alone kernels.  Their grid is capped at 65 536 workgroups of 256 threads
(one thread per 32-channel block), so a second trip needs more than 5 x 10^8 elements -- not a test of a few seconds."""
import ctypes as C

import numpy as np
import pytest
import torch

from downgan_amd.ops import Conv, HipOps
from tests import fp8_quant_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
NROT = len(R.EXPS)


def table(name):
    return {"uniform_bf16": (R.uniform_bf16, "bf16"), "uniform_f32": (R.uniform_f32, "f32"),
            "mx_bf16": (R.mx_blocks_bf16, "bf16"), "mx_f32": (R.mx_blocks_f32, "f32")}[name]


def assert_bytes(got, ref, src, what, exps=None):
    msg = R.first_mismatch(got.cpu().numpy().reshape(ref.shape), ref, None if src is None else src.reshape(ref.shape), exps)
    assert msg is None, f"{what}: {msg}"


def col_exps(exps, shape):
    return np.broadcast_to(np.repeat(np.asarray(exps), 32), shape)


def dests(rows, layout, with_scales):
    """-> (q view [rows, 128], scales view [rows, 4] or None, check()): contiguous, or inside wider buffers of sentinel bytes with rows
    in front and behind; check() asserts that every byte outside the views still holds the sentinel."""
    if layout == "contiguous":
        q = torch.full((rows, 128), SENT, dtype=torch.uint8).cuda()
        s = torch.full((rows, 4), SENT, dtype=torch.uint8).cuda() if with_scales else None
        return q, s, lambda: None
    qw = torch.full((rows + 2, 320), SENT, dtype=torch.uint8).cuda()
    sw = torch.full((rows + 2, 12), SENT, dtype=torch.uint8).cuda()

    def check():
        a, b = qw.cpu().clone(), sw.cpu().clone()
        a[1:rows + 1, 64:192] = SENT
        assert bool((a == SENT).all()), "bytes of q outside the destination were written"
        if with_scales:
            b[1:rows + 1, 4:8] = SENT
        assert bool((b == SENT).all()), "scale bytes outside the destination were written"
    return qw[1:rows + 1, 64:192], (sw[1:rows + 1, 4:8] if with_scales else None), check


def source(tab, fmt, layout):
    x = R.to_torch(tab, fmt)
    if layout == "contiguous":
        return x.cuda()
    wide = torch.full((tab.shape[0] + 1, 384), 3.0, dtype=x.dtype)
    wide[:-1, 128:256] = x
    return wide.cuda()[:-1, 128:256]


@pytest.mark.parametrize("layout", ["contiguous", "slice"])
@pytest.mark.parametrize("name", ["uniform_bf16", "uniform_f32"])
def test_quant_uniform_on_every_pattern_and_scale_edge(name, layout):
    """dg_quant_uniform: every bf16 pattern (every fp32 cut and tail) under every scale byte of EXPS, over 16 rotated launches."""
    fn, fmt = table(name)
    tab = fn()
    hip = HipOps("bf16")
    x = source(tab, fmt, layout)
    assert x.shape[0] % 64 != 0                                   # the last workgroup is partial
    for rot in range(NROT):
        exps = R.rotated_exps(rot)
        q, _, check = dests(tab.shape[0], layout, False)
        hip.quant_uniform(x, q, torch.from_numpy(exps).cuda())
        ref = R.ref_uniform(tab.reshape(-1, 4, 32), exps, fmt).reshape(tab.shape)
        assert_bytes(q, ref, tab, f"dg_quant_uniform {name} {layout} rotation {rot}", col_exps(exps, tab.shape))
        check()


@pytest.mark.parametrize("layout", ["contiguous", "slice"])
@pytest.mark.parametrize("name", ["mx_bf16", "mx_f32", "uniform_bf16", "uniform_f32"])
def test_quant_mxfp8_on_the_block_tables(name, layout):
    """dg_quant_mxfp8: bytes and scale bytes of the leader / follower blocks (and of the uniform tables as blocks of neighbours)."""
    fn, fmt = table(name)
    tab = fn()
    hip = HipOps("bf16")
    x = source(tab, fmt, layout)
    assert x.shape[0] % 64 != 0                                   # the last workgroup is partial
    q, s, check = dests(tab.shape[0], layout, True)
    hip.quant_mxfp8(x, q, s)
    rq, rs = R.ref_mx(tab.reshape(-1, 4, 32), fmt)
    assert np.array_equal(s.cpu().numpy(), rs), f"dg_quant_mxfp8 {name} {layout}: scale bytes differ at {np.argwhere(s.cpu().numpy() != rs)[:4].tolist()}"
    assert_bytes(q, rq.reshape(tab.shape), tab, f"dg_quant_mxfp8 {name} {layout}", np.broadcast_to(np.repeat(rs, 32, axis=-1), tab.shape))
    check()


# ------------------------------------------------------------------------------------------------------------- fused copies
def qpair(shape):
    return (torch.full(shape, SENT, dtype=torch.uint8).cuda(), torch.full(tuple(shape[:-1]) + (shape[-1] // 32,), SENT, dtype=torch.uint8).cuda())


def stored(y):
    return R.from_torch(y.cpu()).reshape(-1, y.shape[-1])


def check_copies(y, oq, ou, exps, what):
    """The fused copies against the reference applied to the stored output."""
    yb = stored(y)
    nb = yb.shape[1] // 32
    if oq is not None:
        rq, rs = R.ref_mx(yb.reshape(-1, nb, 32))
        got_s = oq[1].cpu().numpy().reshape(rs.shape)
        assert np.array_equal(got_s, rs), f"{what}: out_qs differs at {np.argwhere(got_s != rs)[:4].tolist()}"
        assert_bytes(oq[0], rq.reshape(yb.shape), yb, what + " out_q", np.broadcast_to(np.repeat(rs, 32, axis=-1), yb.shape))
    if ou is not None:
        ref = R.ref_uniform(yb.reshape(-1, nb, 32), exps).reshape(yb.shape)
        assert_bytes(ou, ref, yb, what + " out_u", col_exps(exps, yb.shape))


def same_values(y, tab_grid):
    """y equals the table bit for bit, except -0 -> +0 and NaN payloads (NaN is compared as NaN)."""
    yb, tb = stored(y), tab_grid.reshape(-1, tab_grid.shape[-1])
    nan = lambda b: ((b & 0x7f80) == 0x7f80) & ((b & 0x7f) != 0)
    zero = lambda b: (b & 0x7fff) == 0
    return (yb == tb) | (nan(yb) & nan(tb)) | (zero(yb) & zero(tb))


# halo_epilogue (csrc/gg_common.h) compiles one straight-line epilogue per flag combination of this list and serves every other
# combination with the general instance, whose flags are read at run time.  The probe dg_last_conv_kernels() is the same for both
# and DG_FP8_SAT_ON / DG_FP8_SAT_OFF are ordered per compiled instance, so each fused launch below states the key it is there for.
STRAIGHT_LINE, epi_key = R.STRAIGHT_LINE, R.epi_key      # (tests/test_fp8_quant_exact_cpu.py holds the list against the switch itself)


def extra_flags(names, hip, shape):
    """Epilogue operands that leave the stored value unchanged: LeakyReLU of slope 1, a 1-bit mask of ones, an activation mask of
    ones (factor 1), a second residual of zeros, out_bits."""
    ep = {}
    for n in names:
        if n == "act":
            ep["act"] = 1.0
        elif n == "out_bits":
            ep["out_bits"] = torch.zeros(hip.bits_shape(shape), dtype=torch.int16).cuda()
        elif n == "mask_bits":
            ep.update(mask_bits=torch.full(hip.bits_shape(shape), -1, dtype=torch.int16).cuda(), mask_slope=0.2)
        elif n == "mask":
            ep.update(mask=torch.ones(shape, dtype=torch.bfloat16).cuda(), mask_slope=0.2)
        elif n == "r2":
            ep.update(r2=torch.zeros(shape, dtype=torch.bfloat16).cuda(), s2=1.0)
        else:
            raise KeyError(n)
    return ep


def residual_launch(hip, grid, y, key, f8=False, **ep):
    """Residual steering: zero input and weights, r1 = the table, s1 = 1: the epilogue stores 0 * 1 + r1."""
    _, H, W, _ = grid.shape
    cv = Conv(1, H, W, 128, 128, 1, False, net="C" if f8 else "")
    assert bool(hip.f8_eligible(cv, "fwd")) == f8
    x = torch.zeros(1, H, W, 128, dtype=torch.bfloat16).cuda()
    w = torch.zeros(128 * 9 * 128, dtype=torch.bfloat16).cuda()
    r1 = R.to_torch(grid.reshape(-1, 128), "bf16").reshape(1, H, W, 128).cuda()
    assert epi_key(r1=r1, **ep) == key
    hip.conv_fwd(cv, x, w, y, r1=r1, s1=1.0, **ep)
    assert hip.lib.dg_last_conv_kernels() == (32 if f8 else 8)


# (flags beside r1 + out_q + out_u, key, straight-line instance?)
RESIDUAL_CASES = [((), 2312, True), (("r2",), 2328, True), (("act",), 2313, False), (("act", "out_bits"), 2317, False)]


@pytest.mark.parametrize("flags,key,straight", RESIDUAL_CASES, ids=[str(c[1]) for c in RESIDUAL_CASES])
@pytest.mark.parametrize("f8", [False, True], ids=["halo_bf16", "fp8_kernel"])
@pytest.mark.parametrize("name", ["mx_bf16", "uniform_bf16"])
def test_epilogue_copies_by_residual_steering(name, f8, flags, key, straight):
    """out_q and out_u on the whole table, non-finite blocks included, through the straight-line residual instances (2312, 2328) and
    through the GENERAL run-time-flag instance (2313 = residual + LeakyReLU of slope 1, 2317 = ... + out_bits: no straight-line
    instance has these keys) of the halo kernel and of the MXFP8 kernel; out_u under every scale byte of EXPS (rotated launches on
    the uniform table, one launch on the block table).  y must equal the table bit for bit (-0 -> +0 and NaN payloads aside)."""
    assert (key in STRAIGHT_LINE) == straight
    tab = table(name)[0]()
    H, W = R.grid_for(tab.shape[0])
    grid = R.as_grid(tab, H, W)
    hip = HipOps("bf16", f8_critic=True)
    for rot in range(NROT if name == "uniform_bf16" else 1):
        exps = R.rotated_exps(rot)
        y = torch.zeros(1, H, W, 128, dtype=torch.bfloat16).cuda()
        oq, u = qpair(y.shape), torch.full(y.shape, SENT, dtype=torch.uint8).cuda()
        residual_launch(hip, grid, y, key, f8, out_q=oq, out_u=(u, torch.from_numpy(exps).cuda()), **extra_flags(flags, hip, y.shape))
        assert bool(same_values(y, grid).all()), "residual steering did not store the table"
        check_copies(y, oq, u, exps, f"residual steering key {key} f8={f8} {name} rotation {rot}")


@pytest.mark.parametrize("flags,key", [((), 264), (("r2",), 280), (("act",), 265)], ids=["264", "280", "265_general"])
def test_slab_destination(flags, key):
    """y, out_q and out_qs as channel slices of wider tensors (dg_epilogue.ldqs, qs_shift addressing), through the straight-line
    instances 264 / 280 and the general one (265): the copies are right and no byte outside the slices is written."""
    assert (key in STRAIGHT_LINE) == (key != 265)
    tab = R.mx_blocks_bf16()
    H, W = R.grid_for(tab.shape[0])
    grid = R.as_grid(tab, H, W)
    hip = HipOps("bf16")
    yw = torch.full((1, H, W, 384), 3.0, dtype=torch.bfloat16).cuda()
    qw = torch.full((1, H, W, 384), SENT, dtype=torch.uint8).cuda()
    sw = torch.full((1, H, W, 12), SENT, dtype=torch.uint8).cuda()
    y, oq = yw[..., 128:256], (qw[..., 128:256], sw[..., 4:8])
    residual_launch(hip, grid, y, key, out_q=oq, **extra_flags(flags, hip, y.shape))
    assert bool(same_values(y, grid).all())
    check_copies(y, oq, None, None, f"slab destination key {key}")
    a, b, c = qw.cpu().clone(), sw.cpu().clone(), yw.cpu().clone()
    a[..., 128:256] = SENT; b[..., 4:8] = SENT; c[..., 128:256] = 3.0
    assert bool((a == SENT).all()) and bool((b == SENT).all()) and bool((c == 3.0).all())


@pytest.mark.parametrize("part", range(3))
def test_every_scale_byte_on_every_bf16_pattern(part):
    """All 255 scale bytes (85 per case), the same byte on the four column blocks, against all 65 536 bf16 patterns: dg_quant_uniform
    and the fused out_u of the straight-line residual instance (2312) and of the general instance (2313), one reference for the
    three (the residual launches store the table itself)."""
    tab = R.uniform_bf16()
    H, W = R.grid_for(tab.shape[0])
    grid = R.as_grid(tab, H, W)
    hip = HipOps("bf16")
    x = R.to_torch(tab, "bf16").cuda()
    for e in range(85 * part, 85 * part + 85):
        exps = np.full(4, e, dtype=np.uint8)
        et = torch.from_numpy(exps).cuda()
        ref = R.ref_uniform(grid.reshape(-1, 4, 32), exps).reshape(-1, 128)
        q = torch.full(tab.shape, SENT, dtype=torch.uint8).cuda()
        hip.quant_uniform(x, q, et)
        assert_bytes(q, ref[:tab.shape[0]], tab, f"dg_quant_uniform scale byte {e}")
        for flags, key in (((), 2312), (("act",), 2313)):
            y = torch.zeros(1, H, W, 128, dtype=torch.bfloat16).cuda()
            oq, u = qpair(y.shape), torch.full(y.shape, SENT, dtype=torch.uint8).cuda()
            residual_launch(hip, grid, y, key, out_q=oq, out_u=(u, et), **extra_flags(flags, hip, y.shape))
            assert bool(same_values(y, grid).all())
            assert_bytes(u, ref, grid.reshape(-1, 128), f"out_u key {key} scale byte {e}")


def identity_weights(cout=128, scale_per_quarter=False):
    w = torch.zeros(cout, 9, 128)
    for q in range(cout // 128):
        w[q * 128 + torch.arange(128), 4, torch.arange(128)] = 2.0 ** (-q) if scale_per_quarter else 1.0
    return w.reshape(-1).to(torch.bfloat16).cuda()


def finite_grid(name):
    tab = R.finite_rows(table(name)[0](), "bf16")
    H, W = R.grid_for(tab.shape[0])
    return R.as_grid(tab, H, W), H, W


# (flags beside the copies, out_u too?, key of the storing launch, key of the skip_y launch or None)
IDENTITY_CASES = [((), True, 2304, None),                                  # no straight-line instance: the general one
                  (("act",), False, 257, 4353), (("act",), True, 2305, None),
                  (("mask_bits",), False, 258, 4354), (("mask_bits",), True, 2306, 6402),
                  (("act", "out_bits"), False, 261, 4357), (("act", "out_bits"), True, 2309, 6405),
                  (("mask",), False, 288, None), (("mask",), True, 2336, None)]


@pytest.mark.parametrize("flags,with_u,key,skip_key", IDENTITY_CASES, ids=[str(c[2]) for c in IDENTITY_CASES])
@pytest.mark.parametrize("f8", [False, True], ids=["halo_bf16", "fp8_producer"])
@pytest.mark.parametrize("name", ["mx_bf16", "uniform_bf16"])
def test_epilogue_copies_by_identity_steering(name, f8, flags, with_u, key, skip_key):
    """x = the finite part of the table, weights = the identity on the centre tap, on the halo kernel (8) and the fp8 producer (32),
    through every straight-line instance that writes a copy and can be steered to the identity -- LeakyReLU of slope 1 (257 / 2305),
    the 1-bit mask of ones (258 / 2306), LeakyReLU + out_bits (261 / 2309: the critic forward), the activation mask of ones
    (288 / 2336), each again without the bf16 store where that instance exists (4353, 4354, 4357, 6402, 6405) -- and, with no flag
    beside the copies (2304), through the general instance.  On the bf16 kernel every normal pattern comes back unchanged; on the
    fp8 kernel y is the dequantised x.  Either way the copies must be the reference's bytes for what y holds, and the skip_y launch
    must write the same bytes and leave y alone."""
    assert (key in STRAIGHT_LINE) == (key != 2304) and (skip_key is None or skip_key in STRAIGHT_LINE)
    grid, H, W = finite_grid(name)
    hip = HipOps("bf16", f8_critic=True)
    cv = Conv(1, H, W, 128, 128, 1, False, net="C" if f8 else "")
    assert bool(hip.f8_eligible(cv, "fwd")) == f8
    x = R.to_torch(grid.reshape(-1, 128), "bf16").reshape(1, H, W, 128).cuda()
    w = identity_weights()
    for rot in range(NROT if (name == "uniform_bf16" and with_u) else 1):
        exps = R.rotated_exps(rot)
        y = torch.zeros(1, H, W, 128, dtype=torch.bfloat16).cuda()
        oq, u = qpair(y.shape), (torch.full(y.shape, SENT, dtype=torch.uint8).cuda() if with_u else None)
        ep = dict(extra_flags(flags, hip, y.shape), out_q=oq)
        if with_u:
            ep["out_u"] = (u, torch.from_numpy(exps).cuda())
        assert epi_key(**ep) == key
        hip.conv_fwd(cv, x, w, y, **ep)
        assert hip.lib.dg_last_conv_kernels() == (32 if f8 else 8)
        if not f8:
            normal = ((grid.reshape(-1, 128) >> 7) & 0xff) != 0
            assert bool((same_values(y, grid) | ~normal).all()), "a normal bf16 pattern did not come back unchanged"
        check_copies(y, oq, u, exps if with_u else None, f"identity steering key {key} f8={f8} {name} rotation {rot}")
        if skip_key is not None:
            y2 = torch.full(y.shape, 3.0, dtype=torch.bfloat16).cuda()
            oq2, u2 = qpair(y.shape), (torch.full(y.shape, SENT, dtype=torch.uint8).cuda() if with_u else None)
            ep2 = dict(ep, out_q=oq2, skip_y=True)
            if with_u:
                ep2["out_u"] = (u2, ep["out_u"][1])
            if "out_bits" in ep2:
                ep2["out_bits"] = torch.zeros_like(ep["out_bits"])
            assert epi_key(**ep2) == skip_key
            hip.conv_fwd(cv, x, w, y2, **ep2)
            assert hip.lib.dg_last_conv_kernels() == (32 if f8 else 8)
            assert bool((y2 == 3.0).all()) and torch.equal(oq2[0], oq[0]) and torch.equal(oq2[1], oq[1])
            assert not with_u or torch.equal(u2, u)
            assert "out_bits" not in ep2 or torch.equal(ep2["out_bits"], ep["out_bits"])


@pytest.mark.parametrize("act,key", [(None, 256), (1.0, 257)], ids=["256_general", "257"])
def test_pixel_shuffled_destination(act, key):
    """An up-sampling conv (128 -> 512, pixel shuffle) steered by the identity, sub-pixel q scaled by 2^-q: out_q / out_qs of the
    SHUFFLED tensor (scale bytes per destination pixel), through the general instance (256: out_q alone has no straight-line instance)
    and through 257 (LeakyReLU of slope 1)."""
    assert (key in STRAIGHT_LINE) == (key == 257)
    grid, H, W = finite_grid("mx_bf16")
    hip = HipOps("bf16")
    cv = Conv(1, H, W, 128, 512, 1, True)
    x = R.to_torch(grid.reshape(-1, 128), "bf16").reshape(1, H, W, 128).cuda()
    y = torch.zeros(hip.out_shape(cv), dtype=torch.bfloat16).cuda()
    oq = qpair(y.shape)
    ep = dict(out_q=oq) if act is None else dict(out_q=oq, act=act)
    assert epi_key(**ep) == key
    hip.conv_fwd(cv, x, identity_weights(512, True), y, **ep)
    assert hip.lib.dg_last_conv_kernels() == 8
    yb = stored(y).reshape(H, 2, W, 2, 128)
    normal = (((grid >> 7) & 0xff) > 3).reshape(H, W, 128)          # still normal after 2^-3
    for i in range(2):
        for j in range(2):
            want = np.where(normal, grid.reshape(H, W, 128) - ((2 * i + j) << 7), yb[:, i, :, j])
            assert np.array_equal(yb[:, i, :, j], want), f"sub-pixel ({i}, {j}) is not the table times 2^-{2 * i + j}"
    check_copies(y, oq, None, None, "pixel-shuffled destination")


def census_ref(y):
    yb = stored(y)
    return ((yb & 0x7fff).reshape(-1, yb.shape[1] // 32, 32).max(axis=(0, 2)) << 16).astype(np.int64)


def test_first_layer_copies_and_census():
    """The im2col first layer (16 -> 128, two real input channels), steered by power-of-two weights per output channel and table
    values per pixel (R.first_layer_steering; the 1-bit mask all ones, so its factor is 1): out_q / out_u / out_amax beside a stored
    y, then out_u alone with skip_y, against the reference on the stored y; the census equals the largest stored magnitude per block and a second launch only raises it.  (One
    channel would hold 2^100 at any pixel computed behind the end of the tensor; the kernel as it stands computes none -- its last
    workgroup stops at its last 16-pixel group -- so that channel only pins this.)"""
    xg, w, bias, d, drop_c = R.first_layer_steering()
    _, H, W, _ = xg.shape
    hip = HipOps("bf16", f8_critic=True)
    cv = Conv(1, H, W, 16, 128, 1, False, cin_real=2, net="C")
    x = R.to_torch(xg.reshape(-1, 16), "bf16").reshape(1, H, W, 16).cuda()
    wt, bt = torch.from_numpy(w).reshape(-1).to(torch.bfloat16).cuda(), torch.from_numpy(bias).cuda()
    osh = (1, H, W, 128)
    mk = dict(mask_bits=torch.full(hip.bits_shape(osh), -1, dtype=torch.int16).cuda(), mask_slope=0.2)
    pairs = set()
    for rot in range(NROT):
        exps = R.rotated_exps(rot)
        et = torch.from_numpy(exps).cuda()
        y = torch.zeros(osh, dtype=torch.bfloat16).cuda()
        oq, u = qpair(osh), torch.full(osh, SENT, dtype=torch.uint8).cuda()
        census = torch.zeros(4, dtype=torch.int32).cuda()
        hip.conv_fwd(cv, x, wt, y, bias=bt, out_q=oq, out_u=(u, et), out_amax=census, **mk)
        assert hip.lib.dg_last_conv_kernels() == 16
        assert int((stored(y)[:, drop_c] & 0x7fff).max()) == 0
        check_copies(y, oq, u, exps, f"first layer rotation {rot}")
        cref = census_ref(y)
        assert np.array_equal(census.cpu().numpy().astype(np.int64), cref), (census.cpu().tolist(), cref.tolist())
        # alone: no out_q, y not stored
        y2 = torch.full(osh, 3.0, dtype=torch.bfloat16).cuda()
        u2 = torch.full(osh, SENT, dtype=torch.uint8).cuda()
        hip.conv_fwd(cv, x, wt, y2, bias=bt, out_u=(u2, et), out_amax=census, skip_y=True, **mk)
        assert hip.lib.dg_last_conv_kernels() == 16
        assert bool((y2 == 3.0).all()) and torch.equal(u2, u), int((u2 != u).sum())
        assert np.array_equal(census.cpu().numpy().astype(np.int64), cref)          # the same values again: unchanged
        if rot == 0:
            pairs = R.dm_pairs(stored(y).reshape(-1, 4, 32))
            # a second launch may only raise the census: a quarter of the input first, the full input raises it to its own maxima,
            # the quarter again leaves it there
            c2 = torch.zeros(4, dtype=torch.int32).cuda()
            xs = x.clone(); xs[..., 0] *= 0.25                            # (the 1.0 of channel 1 stays: the detector channel still cancels)
            ys = torch.zeros(osh, dtype=torch.bfloat16).cuda()
            hip.conv_fwd(cv, xs, wt, ys, bias=bt, out_q=qpair(osh), out_u=(u2, et), out_amax=c2, **mk)
            small = census_ref(ys)
            assert np.array_equal(c2.cpu().numpy().astype(np.int64), small) and bool((small < cref).all())
            hip.conv_fwd(cv, x, wt, y2, bias=bt, out_u=(u2, et), out_amax=c2, skip_y=True, **mk)
            assert np.array_equal(c2.cpu().numpy().astype(np.int64), cref)
            hip.conv_fwd(cv, xs, wt, y2, bias=bt, out_u=(u2, et), out_amax=c2, skip_y=True, **mk)
            assert np.array_equal(c2.cpu().numpy().astype(np.int64), cref)
    assert len(pairs) == 21 * 128, len(pairs)      # every (d, mantissa) pair, d = 0 .. 20; the random first-layer case offers 2001


def test_first_layer_census_with_a_non_finite_block():
    """The activation + out_bits instance (slope 1: the identity).  A NaN bias makes block 0 of every pixel non-finite: its copies are
    poisoned, the census of that block holds a NaN pattern (the unsigned maximum of the magnitude patterns), and the exponent derived
    from it is 247 + margin."""
    xg, w, bias, d, drop_c = R.first_layer_steering()
    _, H, W, _ = xg.shape
    bias = bias.copy(); bias[5] = np.nan
    hip = HipOps("bf16", f8_critic=True)
    cv = Conv(1, H, W, 16, 128, 1, False, cin_real=2, net="C")
    x = R.to_torch(xg.reshape(-1, 16), "bf16").reshape(1, H, W, 16).cuda()
    osh = (1, H, W, 128)
    y = torch.zeros(osh, dtype=torch.bfloat16).cuda()
    exps = np.array([127, 120, 9, 247], dtype=np.uint8)
    oq, u = qpair(osh), torch.full(osh, SENT, dtype=torch.uint8).cuda()
    census = torch.zeros(4, dtype=torch.int32).cuda()
    hip.conv_fwd(cv, x, torch.from_numpy(w).reshape(-1).to(torch.bfloat16).cuda(), y, bias=torch.from_numpy(bias).cuda(), out_q=oq,
                 out_u=(u, torch.from_numpy(exps).cuda()), out_amax=census, act=1.0, out_bits=torch.zeros(hip.bits_shape(osh), dtype=torch.int16).cuda())
    assert hip.lib.dg_last_conv_kernels() == 16
    yb = stored(y)
    assert bool(((yb[:, 5] & 0x7fff) > 0x7f80).all()) and bool((((yb[:, 32:] >> 7) & 0xff) != 255).all())
    check_copies(y, oq, u, exps, "first layer with a NaN")
    assert bool((u.cpu().reshape(-1, 128)[:, :32] == 0x7f).all()) and bool((oq[1].cpu().reshape(-1, 4)[:, 0] == R.POISON_SCALE).all())
    cref = census_ref(y)
    assert np.array_equal(census.cpu().numpy().astype(np.int64), cref) and cref[0] > 0x7f800000
    out = torch.zeros(4, dtype=torch.uint8).cuda()
    hip.exp_from_amax(census, out, margin=1)
    assert out.cpu().tolist() == (R.scale_byte_of_bits(cref) + 1).tolist() and int(out[0]) == 248 and int(census.abs().sum()) == 0


BIG_LDY = 1 << 18      # pixel stride of the bf16 adjoint at which the merged launch's row step is refused (tests/conv_f8_ref.py)


@pytest.mark.parametrize("per_class", [False, True], ids=["merged", "per_class"])
def test_stride2_data_gradient_copies(per_class):
    """The stride-2 data gradient 256 -> 128 on the MXFP8 kernel, steered (R.s2_dgrad_steering) so that every input pixel holds a table
    value times 2^-d(channel): out_q and out_u against the reference on the stored dx, under every scale byte of EXPS -- the four
    parity classes merged into one launch, and one launch per class (the adjoint is a channel slice of a 2^18-channel tensor, whose
    row step the merged launch refuses; the copies of a strided destination are complete after the last class)."""
    dyg, wd, d, vals = R.s2_dgrad_steering()
    _, Ho, Wo, _ = dyg.shape
    hip = HipOps("bf16", f8_critic=True)
    cv = Conv(1, 2 * Ho, 2 * Wo, 128, 256, 2, False, net="C")
    assert hip.f8_eligible(cv, "dgrad")
    dy = R.to_torch(dyg.reshape(-1, 256), "bf16").reshape(1, Ho, Wo, 256).cuda()
    if per_class:
        wide = torch.zeros(1, Ho, Wo, BIG_LDY, dtype=torch.bfloat16, device="cuda")[..., :256]
        wide.copy_(dy)
        dy = wide
    g = hip._geom(cv, 128, dy.stride(2))
    assert hip.lib.dg_conv3x3_dgrad_launches(C.byref(g)) == (4 if per_class else 1)
    wt = torch.from_numpy(wd).reshape(-1).to(torch.bfloat16).cuda()
    mb = torch.full(hip.bits_shape((1, 2 * Ho, 2 * Wo, 128)), -1, dtype=torch.int16).cuda()
    v = np.zeros(Ho * Wo, dtype=np.int64); v[:vals.size] = vals
    want = (R.to_torch(v.reshape(-1, 1), "bf16").float().reshape(1, Ho, Wo, 1) * torch.from_numpy(np.ldexp(np.float32(1), -d))).to(torch.bfloat16)
    want = want.repeat_interleave(2, 1).repeat_interleave(2, 2)
    for rot in range(NROT if not per_class else 4):
        exps = R.rotated_exps(4 * rot if per_class else rot)
        dx = torch.zeros(1, 2 * Ho, 2 * Wo, 128, dtype=torch.bfloat16).cuda()
        oq, u = qpair(dx.shape), torch.full(dx.shape, SENT, dtype=torch.uint8).cuda()
        hip.conv_dgrad(cv, dy, wt, dx, mask_bits=mb, mask_slope=0.2, out_q=oq, out_u=(u, torch.from_numpy(exps).cuda()))
        assert hip.lib.dg_last_conv_kernels() == 32
        assert torch.equal(dx.cpu(), want), "the steering is exact: dx = table value * 2^-d"
        check_copies(dx, oq, u, exps, f"stride-2 data gradient per_class={per_class} rotation {rot}")
    assert len(R.dm_pairs(stored(dx).reshape(-1, 4, 32))) == 21 * 128       # the random case of test_fp8_gpu.py offers 2004 pairs


# ----------------------------------------------------------------------------------------------------------- exponent chain
def nsub_rows(nb):
    return 64 * (256 // (nb // 4))


@pytest.mark.parametrize("nb", [12, 28, 64])
def test_block_exp_max_against_the_integer_rule(nb):
    """dg_block_exp_max: dword column counts that do not divide 256 (3, 7) and the maximum (16); one row, three rows and more rows
    than one workgroup's 64 trips; margins 0, 1, 8 with the clamp at 254; scale bytes 0 and 254; the decay rule at old = 0, 1, v + 1,
    v + 2 and 254; a row stride wider than the blocks; the scratch zero at rest."""
    hip = HipOps("bf16")
    for rows in (1, 3, nsub_rows(nb) + 37):
        for margin in (0, 1, 8):
            for ld in (nb, nb + 8):
                sc, old, want = R.exp_case(rows, nb, ld, margin, seed=rows + margin)
                out = torch.from_numpy(old.copy()).cuda()
                hip.block_exp_max(torch.from_numpy(sc).cuda()[:, :nb], out, margin=margin)
                assert np.array_equal(out.cpu().numpy(), want), (rows, nb, ld, margin, out.cpu().tolist(), want.tolist(), old.tolist())
                assert int(hip._exp_scratch.abs().sum()) == 0


def test_block_exp_max_entry_point():
    """dg_block_exp_max itself (HipOps goes through dg_block_exp_max_batch): one tensor, strided rows, margin 8 with the clamp."""
    hip = HipOps("bf16")
    rows, nb, ld = nsub_rows(28) + 11, 28, 36
    sc, old, want = R.exp_case(rows, nb, ld, 8, seed=7)
    dev, out = torch.from_numpy(sc).cuda(), torch.from_numpy(old.copy()).cuda()
    scratch = torch.zeros(64 * 16, dtype=torch.int32).cuda()
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = hip.lib.dg_block_exp_max(vp(dev), rows, ld, nb, 8, vp(out), vp(scratch), hip._stream())
    assert rc == 0
    assert np.array_equal(out.cpu().numpy(), want), (out.cpu().tolist(), want.tolist())
    assert int(scratch.abs().sum()) == 0 and int(want.max()) == 254


def test_block_exp_max_batch_of_mixed_sizes():
    """Sixteen tensors in one launch, from one row to more than a workgroup's trips: most workgroups of the small ones do nothing."""
    hip = HipOps("bf16")
    shapes = [(1, 4), (3, 12), (nsub_rows(28) + 5, 28), (2, 64), (nsub_rows(12) * 3 + 1, 12), (7, 8), (1, 64), (nsub_rows(64) + 1, 64),
              (5, 20), (64, 32), (1, 28), (300, 4), (2, 12), (nsub_rows(4) + 3, 4), (9, 16), (1000, 64)]
    assert len(shapes) == 16
    pairs, wants = [], []
    for i, (rows, nb) in enumerate(shapes):
        sc, old, want = R.exp_case(rows, nb, nb, 1, seed=100 + i)
        pairs.append((torch.from_numpy(sc).cuda(), torch.from_numpy(old.copy()).cuda()))
        wants.append(want)
    hip.block_exp_max_batch(pairs, margin=1)
    for (sc, out), want, shp in zip(pairs, wants, shapes):
        assert np.array_equal(out.cpu().numpy(), want), (shp, out.cpu().tolist(), want.tolist())
    assert int(hip._exp_scratch.abs().sum()) == 0


@pytest.mark.parametrize("nb", [4, 17, 64])
def test_exp_from_amax_against_the_integer_rule(nb):
    """dg_exp_from_amax on the edges of the census: zero, fp32 subnormals, exponent fields 8 and 9 (scale bytes 0 and 1), the largest
    finite value (246), Inf and NaN patterns (247); margins 0, 1, 8; the decay rule; the census is cleared."""
    hip = HipOps("bf16")
    for margin in (0, 1, 8):
        for seed in range(5):
            a, old, want = R.amax_case(nb, margin, seed)
            census = torch.from_numpy(a.astype(np.uint32).view(np.int32).copy()).cuda()
            out = torch.from_numpy(old.copy()).cuda()
            hip.exp_from_amax(census, out, margin=margin)
            assert np.array_equal(out.cpu().numpy(), want), (nb, margin, seed, out.cpu().tolist(), want.tolist())
            assert int(census.abs().sum()) == 0
