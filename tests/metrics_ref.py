"""References, comparators and the case table of the exact tests of the MS-SSIM / physics kernels (csrc/metrics.hip), the low-pass
pair (csrc/freqsep.hip) and the staging kernels (csrc/preprocess.hip): tests/test_metrics_exact_gpu.py on the device,
tests/test_metrics_exact_cpu.py on the emulation.  The machinery (``Buf`` guards and slab views, ``assert_bits``, ``check_elem``,
``check_exact_sum``, ``int_data``, ``guard_cap``) is that of tests/elementwise_ref.py.

Every ``ref_*`` restates one contract of include/downgan_hip.h from its definition, in Python integers / torch int64 / float64 /
numpy float32 on the host; none calls oracle/msssim.py, oracle/physics.py, ref_step.lowpass or EmuOps (those are what the CPU
file cross-checks).  For the "large" low-pass case alone the integer window sums are formed with torch on the device in int64
(exact in any order), channel by channel, so the case stays small in time and memory.

What is held to what:
* bits: low-pass low / high / adjoint on integer data, 2x2 pooling on integer data, the NHWC -> planar normalisation on any
  finite data (two subtractions and a division, no contraction possible), the staged store (one subtraction, one product);
* equality of values: min / max (selections; +-0 compare equal), the ten double sums of the divergence / vorticity pass, the
  three double moments, the SSIM / CS plane sums of X == Y (the count of valid pixels);
* derived bounds (each in the docstring of its case): low-pass of N(0,1) data, the located SSIM window, one-pixel SSIM maps;
* one measured quantity: the device ``powf`` inside dg_msssim_finish (``POW_REL``).
"""
from __future__ import annotations

import numpy as np
import torch

from downgan_amd import _lib
from downgan_amd.msssim import WEIGHTS, MsSsim, level_sizes
from tests import elementwise_ref as E
from tests.elementwise_ref import (Buf, TD, U, _cdiv, _gen, _report, assert_bits, check_elem, check_exact_sum, d, epc, guard_cap,
                                   int_data, randn)

# launch rules, restated next to their guards (csrc/*.hip)
FS_BLOCKS = 65535                    # freqsep.hip fs_blocks: at most 65535 workgroups of 256 threads, one 16-byte chunk per thread
POOL_THREADS = 8192 * 256            # metrics.hip dg_avgpool2 / dg_normalise_planar: at most 8192 x 256 threads, grid-stride
MINMAX_THREADS = _lib.MINMAX_PARTS * 256     # dg_minmax_partial: always DG_MINMAX_PARTS (256) workgroups of 256 threads
DV_THREADS = 1024 * 256              # dg_div_vort_sums: at most 1024 x 256 threads, one window pixel each per trip
MOM_BLOCKS = 2048                    # preprocess.hip dg_moments: at most 2048 workgroups, one float4 per thread per trip
STAGE_THREADS = 4096 * 256           # dg_stage_fields: at most 4096 x 256 threads, one pixel per trip
SSIM_TILE = 32                       # dg_ssim_level: one workgroup per 32 x 32 tile of the valid map
POW_REL = 16 * U                     # dg_msssim_finish: relative bound of prod_l powf(term_l, w_l), from a measurement; see case_finish


def guard_items(expect, what, items, threads):
    """expect="second_trip": ``items`` work items on a launch of at most ``threads`` threads -- the grid-stride loop runs again."""
    assert expect in (None, "second_trip"), expect
    if expect:
        assert items > threads, f"size guard: {what} has {items} work items, not more than {threads}: one grid-stride trip"


def assert_bits_nan(out, ref, what):
    """Bit equality wherever the reference is a number; NaN where it is NaN (the sign / payload of a NaN is not part of a contract)."""
    o, r = out.detach().cpu(), ref.detach().cpu()
    assert o.shape == r.shape and o.dtype == r.dtype, f"{what}: {tuple(o.shape)} {o.dtype} vs {tuple(r.shape)} {r.dtype}"
    no, nr = torch.isnan(o), torch.isnan(r)
    if not torch.equal(no, nr):
        i = int((no != nr).flatten().nonzero()[0])
        raise AssertionError(f"{what}: non-finite mismatch at flat index {i}: got {float(o.flatten()[i])!r}, reference {float(r.flatten()[i])!r}")
    z = torch.zeros((), dtype=o.dtype)
    assert_bits(torch.where(no, z, o), torch.where(nr, z, r), what)


def check_values(out, ref, what):
    """Equality of values (not bits: -0 == +0), element for element, for selections and exact double sums."""
    o, r = d(out), ref.double()
    assert o.shape == r.shape, f"{what}: {tuple(o.shape)} vs {tuple(r.shape)}"
    same = (o == r) | (torch.isnan(o) & torch.isnan(r))
    if not bool(same.all()):
        i = int((~same).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {o.numel()} sums differ; index {i}: got {float(o.flatten()[i])!r}, "
                             f"exact {float(r.flatten()[i])!r}")
    _report("metrics", what + " (exact)", 0.0)


def clamp_map(L, delta):
    """The index map p -> q = clamp(p + delta) of replication padding on an axis of length L, from its definition."""
    return [min(max(p + delta, 0), L - 1) for p in range(L)]


# ================================================================================================ 1. dg_lowpass5 / dg_lowpass5_adjoint
LP_SHAPES = [(1, 1, 1), (1, 1, 7), (2, 5, 1), (1, 2, 2), (1, 2, 5), (1, 3, 3), (1, 4, 6), (2, 5, 5), (1, 6, 9)]
LP_SLABS = ((112, 24), (80, 16), (56, 8))            # source, low / out, high: three different widths


def ref_window_sums(x):
    """S[n, y, x, c] = sum over the 5 x 5 offsets of x[n, clamp(y + dy), clamp(x + dx), c] (any dtype / device; integers exact)."""
    H, W = x.shape[1], x.shape[2]
    S = torch.zeros_like(x)
    for dy in range(-2, 3):
        rows = x[:, torch.tensor(clamp_map(H, dy), device=x.device)]
        for dx in range(-2, 3):
            S += rows[:, :, torch.tensor(clamp_map(W, dx), device=x.device)]
    return S


def ref_lowpass(xi, tdtype):
    """Integer input -> (low, high) as stored.  lo = fp32(S / 25): S / 25 in float64 followed by one rounding to fp32 IS the
    correctly rounded fp32 quotient, because a quotient of two fp32 numbers rounded to p = 53 >= 2 * 24 + 2 bits cannot sit on or
    next to an fp32 rounding boundary it was not on already (double rounding is innocuous for division at that precision).
    hi = fp32(ctr - lo): the float64 difference of an fp32 and a small integer is exact, so one rounding too.  A bf16 store is one
    more round-to-nearest-even."""
    lo = (ref_window_sums(xi).double() / 25.0).float()
    hi = (xi.double() - lo.double()).float()
    return lo.to(tdtype), hi.to(tdtype)


def ref_adjoint_sums(gi):
    """Transpose of the forward map, in integers: every pixel p scatters g[p] to q = (clamp(py + dy), clamp(px + dx)) for each of
    the 25 offsets -- the fold weights arise from the map itself, not from a formula for them."""
    N, H, W, C = gi.shape
    acc = torch.zeros(H, W, N, C, dtype=gi.dtype, device=gi.device)
    gp = gi.permute(1, 2, 0, 3).contiguous()
    for dy in range(-2, 3):
        qy = torch.tensor(clamp_map(H, dy), device=gi.device)[:, None].expand(H, W)
        for dx in range(-2, 3):
            qx = torch.tensor(clamp_map(W, dx), device=gi.device)[None, :].expand(H, W)
            acc.index_put_((qy, qx), gp, accumulate=True)
    return acc.permute(2, 0, 1, 3)


def ref_adjoint(gi, tdtype):
    return (ref_adjoint_sums(gi).double() / 25.0).float().to(tdtype)


def case_lowpass(ops, dtype, C=8, view=False):
    """Integers |v| <= 64: all 25 window sums (<= 1600) and the adjoint's folded sums (<= 9 * 25 * 64) are exact in fp32 in any
    order.  Every L in {1, 2, 3, 4, 5, >= 6} per axis; low only, high only, both; then the adjoint."""
    td = TD[dtype]
    gen = _gen(201)
    for shape in LP_SHAPES:
        full = shape + (C,)
        xi, x = int_data(full, -64, 64, gen, dtype, terms=9 * 25)
        lo_ref, hi_ref = ref_lowpass(xi.long(), td)
        xb = Buf(ops, x, slab=LP_SLABS[0] if view else None)
        for want_low, want_high in ((True, False), (False, True), (True, True)):
            lo = Buf(ops, randn(full, dtype, gen), slab=LP_SLABS[1] if view else None) if want_low else None
            hi = Buf(ops, randn(full, dtype, gen), slab=LP_SLABS[2] if view else None) if want_high else None
            ops.lowpass5(xb.dev, low=lo.dev if lo else None, high=hi.dev if hi else None)
            what = f"lowpass5 {shape} C={C} low={want_low} high={want_high}{' view' if view else ''}"
            if lo:
                assert_bits(lo.result(), lo_ref, what + ": low"); lo.check(what + ": low")
            if hi:
                assert_bits(hi.result(), hi_ref, what + ": high"); hi.check(what + ": high")
        out = Buf(ops, randn(full, dtype, gen), slab=LP_SLABS[1] if view else None)
        ops.lowpass5_adjoint(xb.dev, out.dev)
        assert_bits(out.result(), ref_adjoint(xi.long(), td), f"lowpass5_adjoint {shape} C={C}{' view' if view else ''}")
        out.check("lowpass5_adjoint out"); xb.check("lowpass5 x", written=False)


def _dev_same_bits(a, b):
    v = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.contiguous().view(v), b.contiguous().view(v)))


def lowpass_large_shape(dtype):
    """N * H * W * C / (elements per 16-byte chunk) must exceed 65535 * 256: two images for bf16, whose chunks hold 8 elements."""
    return (1, 2050, 2050) if dtype == "f32" else (2, 2050, 2050)


def case_lowpass_large(ops, dtype, shape=None, C=16, expect=None):
    """More 16-byte chunks than 65535 x 256 threads: the grid-stride loops of both kernels take a second trip.  The references
    are formed on the device, one channel at a time (int64 window sums / scatter), and compared there."""
    N, H, W = shape = tuple(shape or lowpass_large_shape(dtype))
    cch = C // epc(dtype)
    guard_cap(expect, "lowpass5 / lowpass5_adjoint", _cdiv(N * H * W * cch, 256), FS_BLOCKS)
    td = TD[dtype]
    gen = _gen(202)
    _, x = int_data(shape + (C,), -64, 64, gen, dtype, terms=9 * 25)
    xb = Buf(ops, x)
    del x
    out = Buf(ops, torch.zeros(1, dtype=td).expand(shape + (C,)))

    def compare(which):
        for n in range(N):
            for c in range(C):
                xc = xb.dev[n:n + 1, :, :, c:c + 1].long()
                ref = ref_adjoint(xc, td) if which == "adjoint" else ref_lowpass(xc, td)[0 if which == "low" else 1]
                assert _dev_same_bits(out.dev[n:n + 1, :, :, c:c + 1], ref), f"lowpass5 {which} {shape} C={C}: image {n} channel {c} differs in bits"
        out.check("lowpass5 large " + which)
    ops.lowpass5(xb.dev, low=out.dev)
    compare("low")
    ops.lowpass5(xb.dev, high=out.dev)
    compare("high")
    ops.lowpass5_adjoint(xb.dev, out.dev)
    compare("adjoint")
    assert bool((xb.raw[xb.nbytes:] == E.SENTINEL).all())


def case_lowpass_normal(ops, dtype, shape=(2, 7, 9), C=8):
    """N(0,1) data under the per-element comparator with M = sum |terms| / 25.  The kernel adds 25 terms to 0 (the first addition is
    exact, 24 round, each by at most 2^-24 of a partial sum that never exceeds sum |terms|) and divides once (2^-24 of the
    quotient): 25 roundings to first order; factor 26 absorbs the second-order terms (25 * 24 * 2^-48).  high = fp32(ctr - lo)
    adds one rounding of a value bounded by |ctr| + M: factor 27 on M_hi = |ctr| + M.  Any summation order obeys the same bound."""
    gen = _gen(203)
    x = randn(shape + (C,), dtype, gen)
    S, Sabs = ref_window_sums(d(x)), ref_window_sums(d(x).abs())
    lo_ref, M = S / 25.0, Sabs / 25.0
    xb, lo, hi = Buf(ops, x), Buf(ops, randn(shape + (C,), dtype, gen)), Buf(ops, randn(shape + (C,), dtype, gen))
    ops.lowpass5(xb.dev, low=lo.dev, high=hi.dev)
    check_elem(lo.result(), lo_ref, M, "lowpass5 N(0,1) low", family="lowpass", factor=26)
    check_elem(hi.result(), d(x) - lo_ref, d(x).abs() + M, "lowpass5 N(0,1) high", family="lowpass", factor=27)
    lo.check("low"); hi.check("high"); xb.check("x", written=False)


# ================================================================================================ 2. dg_avgpool2
POOL_SHAPES = [(2, 2), (2, 3), (3, 2), (3, 3), (5, 4), (7, 13), (64, 66), (65, 33)]


def ref_avgpool2(xi, pad_low=True):
    """Kernel 2, stride 2, padding = size % 2 on the TOP / LEFT (``pad_low``; False pads bottom / right, a mutant), padded zeros
    counted in the divisor of 4.  Index loops from the definition: output (ho, wo) covers rows 2 ho - ph + {0, 1}."""
    P, H, W = xi.shape
    ph, pw = H % 2, W % 2
    Ho, Wo = (H + 2 * ph - 2) // 2 + 1, (W + 2 * pw - 2) // 2 + 1
    oy, ox = (ph, pw) if pad_low else (0, 0)
    S = torch.zeros(P, Ho, Wo, dtype=torch.int64)
    for a in range(2):
        ys = [2 * ho - oy + a for ho in range(Ho)]
        for b in range(2):
            xs = [2 * wo - ox + b for wo in range(Wo)]
            for ho, y in enumerate(ys):
                if not 0 <= y < H:
                    continue
                ok = [(wo, x) for wo, x in enumerate(xs) if 0 <= x < W]
                S[:, ho, [w for w, _ in ok]] += xi[:, y, [x for _, x in ok]]
    return (S.double() / 4.0).float()


def case_avgpool(ops, dtype, shapes=POOL_SHAPES, planes=(1, 3, 70), expect=None):
    """Integers in [-64, 64]: the sum of at most four and the product with 0.25 are exact, so the output has the reference's bits."""
    gen = _gen(210)
    for H, W in shapes:
        for P in planes:
            Ho, Wo = level_sizes(H, W, 2)[1]
            guard_items(expect, f"avgpool2 {P} x {H} x {W}", P * Ho * Wo, POOL_THREADS)
            xi, x = int_data((1, P, H, W), -64, 64, gen, torch.float32, terms=4)
            ref = ref_avgpool2(xi[0].long())
            assert tuple(ref.shape) == (P, Ho, Wo), (tuple(ref.shape), (P, Ho, Wo))
            inp, out = Buf(ops, x), Buf(ops, torch.full((1, P, Ho, Wo), 7.0))
            ops.avgpool2(inp.dev, out.dev)
            assert_bits(out.result()[0], ref, f"avgpool2 {P} x {H} x {W}")
            out.check("avgpool2 out"); inp.check("avgpool2 in", written=False)


# ================================================================================================ 3. dg_minmax_partial + dg_minmax_finish
PAD_SPECIALS = (float("inf"), float("-inf"), float("nan"), 3e38, -3e38)


def ref_minmax(x, C):
    """[C, 2] float64: min / max of channel c over every pixel, NaN pixels skipped (fminf / fmaxf); no number at all: (+inf, -inf)."""
    v = d(x).reshape(-1, x.shape[-1])
    out = torch.empty(C, 2, dtype=torch.float64)
    for c in range(C):
        col = v[:, c][~torch.isnan(v[:, c])]
        out[c, 0] = col.min() if col.numel() else float("inf")
        out[c, 1] = col.max() if col.numel() else float("-inf")
    return out


def _with_pads(vals, ld):
    """[..., C] -> [..., ld] whose pad channels hold +-inf, NaN and +-3e38."""
    C = vals.shape[-1]
    out = torch.empty(tuple(vals.shape[:-1]) + (ld,), dtype=vals.dtype)
    out[..., :C] = vals
    for k in range(C, ld):
        out[..., k] = PAD_SPECIALS[(k - C) % len(PAD_SPECIALS)]
    return out


def _layout(ops, vals, layout, C, which=0):
    """dense: ld = C; ld16: 16 channels, the pads special; slab: channels of a wider random slab.  -> Buf whose .dev has >= C channels."""
    if layout == "dense":
        return Buf(ops, vals)
    if layout == "ld16":
        return Buf(ops, _with_pads(vals, 16))
    return Buf(ops, vals, slab=(E.V_SLAB, E.V_SLAB2)[which])


def _run_minmax(ops, x, C):
    partial = Buf(ops, torch.full((_lib.MINMAX_PARTS * C * 2,), 7.0))
    mm = Buf(ops, torch.full((2 * C,), 7.0))
    ops.minmax(x.dev, C, partial.dev, mm.dev)
    partial.check("minmax partial"); mm.check("minmax out"); x.check("minmax x", written=False)
    return mm.result().view(C, 2)


def case_minmax_located(ops, dtype, pixels=257, C=8, layout="dense", expect=None):
    """A field of ones with one planted minimum -(2 + c) and one planted maximum 3 + c per channel, at pixel 0, 255, 256, the last
    pixel, 65535 and 65536 (the last two straddle the first grid-stride trip of 256 x 256 threads), a different one per channel."""
    guard_items(expect, "minmax_partial", pixels, MINMAX_THREADS)
    cand = []
    for p in (0, 255, 256, pixels - 1, 65535, 65536):
        if p < pixels and p not in cand:
            cand.append(p)
    n = len(cand)
    base = torch.ones(1, 1, pixels, C)
    want = torch.empty(C, 2, dtype=torch.float64)
    for c in range(C):
        pmin, pmax = cand[c % n], cand[(c + max(1, n // 2)) % n]
        base[0, 0, pmin, c] = -(2.0 + c)
        want[c, 0] = -(2.0 + c)
        if pmax != pmin:
            base[0, 0, pmax, c] = 3.0 + c
        want[c, 1] = 3.0 + c if pmax != pmin else -(2.0 + c)
    vals = base.to(TD[dtype])
    assert torch.equal(ref_minmax(vals, C), want)
    got = _run_minmax(ops, _layout(ops, vals, layout, C), C)
    check_values(got, want, f"minmax located pixels={pixels} C={C} {layout}")


def case_minmax_values(ops, dtype, shape=(2, 9, 13), layout="ld16"):
    """Selections are exact on any finite data.  Channel 0: N(0,1); 1: N(0,1) with NaN pixels (skipped); 2: {+0, -0, 1, 2} (the minimum
    is a zero of either sign: fminf may return either, so zeros compare by value); 3: {-0, +0, -1}; 4: NaN alone -> (+inf, -inf)."""
    gen = _gen(221)
    C = 5
    v = torch.randn(shape + (C,), generator=gen)
    v[0, 3, 4, 1] = v[1, 8, 12, 1] = v[0, 0, 0, 1] = float("nan")
    pick = torch.randint(0, 4, shape, generator=gen)
    v[..., 2] = torch.tensor([0.0, -0.0, 1.0, 2.0])[pick]
    v[..., 3] = torch.tensor([-0.0, 0.0, -1.0, -1.0])[pick]
    v[..., 4] = float("nan")
    vals = v.to(TD[dtype])
    ref = ref_minmax(vals, C)
    assert float(ref[2, 0]) == 0.0 and float(ref[3, 1]) == 0.0 and float(ref[4, 0]) == float("inf")
    got = _run_minmax(ops, _layout(ops, vals, layout, C), C)
    check_values(got, ref, f"minmax values {layout}")


# ================================================================================================ 4. dg_normalise_planar
def ref_normalise(x, C, mm):
    """numpy float32, in the kernel's order: (x - mn) / (mx - mn) -- two subtractions and one division, each correctly rounded, and
    no pair of them can be contracted into a fused operation."""
    v = x[..., :C].float().numpy()
    mn, mx = mm[:, 0].float().numpy(), mm[:, 1].float().numpy()
    with np.errstate(all="ignore"):
        out = (v - mn) / (mx - mn)
    assert out.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 3, 1, 2)))


def case_normalise(ops, dtype, shape=(2, 5, 7), C=2, layout="ld16", data="normal", expect=None):
    """data: "normal" N(0,1); "index": every (n, c, h, w) holds its own flat planar index (the NHWC -> planar map); "const": channel
    0 is constant, so it comes out as 0 / 0 = NaN everywhere, the kind the float64 formula gives too."""
    N, H, W = shape
    guard_items(expect, "normalise_planar", N * H * W, POOL_THREADS)
    gen = _gen(230)
    if data == "index":
        total = N * C * H * W
        assert total <= (256 if dtype == "bf16" else E.INT_LIMIT), "the indices must be exact in the storage dtype"
        v = torch.arange(total, dtype=torch.float32).view(N, C, H, W).permute(0, 2, 3, 1).contiguous()
    else:
        v = torch.randn(N, H, W, C, generator=gen) * 3.0 + 1.0
        if data == "const":
            v[..., 0] = 0.75
    vals = v.to(TD[dtype])
    mm = ref_minmax(vals, C).float()
    x = _layout(ops, vals, layout, C)
    mmb, out = Buf(ops, mm.reshape(-1)), Buf(ops, torch.full((N, C, H, W), 7.0))
    ops.normalise_planar(x.dev, C, mmb.dev, out.dev)
    ref = ref_normalise(vals, C, mm)
    what = f"normalise_planar {shape} C={C} {layout} {data}"
    if data == "const":
        assert bool(torch.isnan(ref[:, 0]).all()) and not bool(torch.isnan(ref[:, 1:]).any())
    assert_bits_nan(out.result(), ref, what)
    out.check(what); x.check(what + " x", written=False); mmb.check(what + " minmax", written=False)


# ================================================================================================ 5. dg_ssim_level
K_REF = (0.01 ** 2, 0.03 ** 2)                        # the metric's own constants: (K1 L)^2, (K2 L)^2 with L = 1
G_ASYM = [v / 32.0 for v in (2, 3, 4, 5, 5, 6, 7)]    # asymmetric, dyadic, sums to one; no weight so small that its pixel stays at 1
COUNT_SHAPES = [(1, 1), (1, 33), (2, 31), (31, 2), (32, 32), (33, 1), (32, 33), (33, 64), (64, 65), (65, 31), (65, 65), (2, 64)]


def gauss(win, sigma=1.5):
    c = torch.arange(win, dtype=torch.float32) - win // 2
    g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).tolist()


def ssim_params(g, C1, C2):
    p = _lib.SsimParams(win=len(g), C1=C1, C2=C2)
    for i, v in enumerate(g):
        p.g[i] = v
    return p


def ref_ssim(X, Y, p):
    """Float64 maps of one scale from the definition, with the window and constants as the kernel receives them (fp32).
    X, Y: [P, H, W] -> dict of [P, Hv, Wv] tensors."""
    win = p.win
    g = [float(p.g[i]) for i in range(win)]
    C1, C2 = float(p.C1), float(p.C2)
    X, Y = X.double(), Y.double()
    Hv, Wv = X.shape[1] - win + 1, X.shape[2] - win + 1

    def filt(T):
        out = torch.zeros(T.shape[0], Hv, Wv, dtype=torch.float64)
        for a in range(win):
            for b in range(win):
                out += (g[a] * g[b]) * T[:, a:a + Hv, b:b + Wv]
        return out
    r = dict(mu1=filt(X), mu2=filt(Y), m2=filt(X * X), m3=filt(Y * Y), m4=filt(X * Y))
    r["s1"], r["s2"], r["s12"] = r["m2"] - r["mu1"] ** 2, r["m3"] - r["mu2"] ** 2, r["m4"] - r["mu1"] * r["mu2"]
    r["N"], r["D"] = 2 * r["s12"] + C2, r["s1"] + r["s2"] + C2
    r["A"], r["B"] = 2 * r["mu1"] * r["mu2"] + C1, r["mu1"] ** 2 + r["mu2"] ** 2 + C1
    r["cs"], r["l"] = r["N"] / r["D"], r["A"] / r["B"]
    r["ssim"] = r["l"] * r["cs"]
    return r


def ssim_eval_bound(r, win):
    """Absolute bounds (e_ssim, e_cs) of one pixel's fp32 evaluation, for data in [0, 1] and a non-negative window.

    Each of the five filtered quantities m is built by win fused steps along H and win along W, one rounding each, plus the rounding
    of the product x * y under it: at most 2 win + 1 roundings, each at most 2^-24 of a partial sum that never exceeds m itself (all
    terms are non-negative).  E(m) = (2 win + 2) * 2^-24 * m; the extra unit absorbs every second-order term.
      squares:  e(mu^2)  = 2 mu E(mu) + 2^-24 mu^2,    e(mu1 mu2) = mu1 E(mu2) + mu2 E(mu1) + 2^-24 mu1 mu2
      sigma:    e(s)     = E(m) + e(mu^2) + 2^-24 |s|  -- the cancellation in m - mu^2 is carried as an ABSOLUTE error of the order
                2^-24 (|m| + mu^2), which the quotient then divides by its denominator
      cs = N / D, N = 2 s12 + C2, D = s1 + s2 + C2:  e(N) = 2 e(s12) + 2^-24 |N|,  e(D) = e(s1) + e(s2) + 2 * 2^-24 |D|
                |N'/D' - N/D| <= (e(N) + |cs| e(D)) / (|D| - e(D)), plus 2^-24 |cs| for the division itself
      l = A / B the same with A = 2 mu1 mu2 + C1, B = mu1^2 + mu2^2 + C1;  ssim = l cs: |cs| e(l) + |l| e(cs) + e(l) e(cs) + 2^-24 |ssim|."""
    k = (2 * win + 2) * U
    mu1, mu2 = r["mu1"], r["mu2"]
    e1, e2 = k * mu1, k * mu2
    esq1, esq2 = 2 * mu1 * e1 + U * mu1 ** 2, 2 * mu2 * e2 + U * mu2 ** 2
    e12 = mu1 * e2 + mu2 * e1 + U * mu1 * mu2
    es1, es2 = k * r["m2"] + esq1 + U * r["s1"].abs(), k * r["m3"] + esq2 + U * r["s2"].abs()
    es12 = k * r["m4"] + e12 + U * r["s12"].abs()
    eN, eD = 2 * es12 + U * r["N"].abs(), es1 + es2 + 2 * U * r["D"].abs()
    assert bool((r["D"].abs() > 2 * eD).all()) and bool((r["B"] > 0).all()), "a denominator is within its own error of zero"
    ecs = (eN + r["cs"].abs() * eD) / (r["D"].abs() - eD) + U * r["cs"].abs()
    eA, eB = 2 * e12 + U * r["A"], esq1 + esq2 + 2 * U * r["B"]
    el = (eA + r["l"] * eB) / (r["B"] - eB) + U * r["l"]
    return r["cs"].abs() * el + r["l"].abs() * ecs + el * ecs + U * r["ssim"].abs(), ecs


def _run_ssim(ops, X, Y, p, preload=None):
    """X, Y [P, H, W] fp32 -> sums [P, 2] (SSIM, CS)."""
    P = X.shape[0]
    xb, yb = Buf(ops, X[None].contiguous()), Buf(ops, Y[None].contiguous())
    sums = Buf(ops, preload.clone() if preload is not None else torch.zeros(P, 2))
    ops.ssim_level(xb.dev, yb.dev, p, sums.dev.view(-1))
    sums.check("ssim_level sums"); xb.check("ssim_level X", written=False); yb.check("ssim_level Y", written=False)
    return sums.result()


def case_ssim_count(ops, dtype, win=7, rot=0, asym=False):
    """X == Y bit for bit: every pixel's two quotients have bit-identical numerator and denominator, with or without contraction
    (both sides run the same operations on the same values), so both plane sums EQUAL the number of valid pixels plus the integer
    the accumulator held.  Hv, Wv across the 31 / 32 / 33 and 64 / 65 tile edges, H = W = win included."""
    gen = _gen(240 + win)
    g = (G_ASYM if asym else gauss(win))
    assert len(g) == win
    p = ssim_params(g, *K_REF)
    for i, (Hv, Wv) in enumerate(COUNT_SHAPES):
        P = (1, 3, 70)[(i + rot) % 3]
        H, W = Hv + win - 1, Wv + win - 1
        X = torch.rand(P, H, W, generator=gen)
        r = ref_ssim(X, X, p)
        assert float(r["D"].min()) > 0 and float(r["B"].min()) > 0, "a float64 denominator is zero"
        pre = torch.randint(0, 50, (P, 2), generator=gen).float()
        assert Hv * Wv + 50 < E.INT_LIMIT
        got = _run_ssim(ops, X, X.clone(), p, preload=pre)
        check_exact_sum(got, pre.double() + Hv * Wv, f"ssim_level count win={win} valid {Hv} x {Wv} planes={P}", family="ssim")


LOC_HV = 40                                            # two tiles each way
# delta, the window and C1 = C2 are chosen so that the condition of located_reference holds (it is asserted there, from float64
# alone): with delta = 0.25 or a window whose smallest weight is 1 / 32 the least affected pixel moves by less than 8 x the bound
LOC_C = 2.0 ** -8
LOC_DELTA = 0.5


def located_positions(win=7, hv=LOC_HV):
    L = hv + win - 1
    m = L // 2
    return [(0, 0), (0, L - 1), (L - 1, 0), (L - 1, L - 1), (0, m), (m, 0), (L - 1, m), (m, L - 1),
            (31, 31), (32, 32), (33, 33), (31, 38), (38, 32), (37, 39), (33, 6), (6, 37), (L - 1, 33), (32, L - 1)]


def located_additions(hv=LOC_HV, wv=LOC_HV):
    """Non-integer additions a map value passes on its way into the plane sum: <= 4 inside a thread (1024 tile pixels / 256 threads),
    6 steps of the wave reduction, 3 across the 4 waves, one atomic per workgroup = per 32 x 32 tile of the plane."""
    return 4 + 6 + 3 + _cdiv(hv, SSIM_TILE) * _cdiv(wv, SSIM_TILE)


def located_reference(pos, p, hv=LOC_HV):
    """X = Y = 0.5 except Y[pos] = 0.5 + delta.  -> (sum of ssim - 1, sum of cs - 1, bound, smallest |map - 1|) over the affected
    pixels, from float64 alone.  Bound = additions * 2^-24 * count (every rounding of a partial sum, which never exceeds the count)
    plus the evaluation bounds of the affected pixels (ssim_eval_bound); an unaffected pixel is exactly 1 by the count argument."""
    win = p.win
    L = hv + win - 1
    X = torch.full((1, L, L), 0.5)
    Y = X.clone()
    Y[0, pos[0], pos[1]] = 0.5 + LOC_DELTA
    r = ref_ssim(X, Y, p)
    hit = torch.zeros(1, hv, hv, dtype=torch.bool)
    hit[0, max(0, pos[0] - win + 1):pos[0] + 1, max(0, pos[1] - win + 1):pos[1] + 1] = True
    assert bool((r["ssim"][~hit] == 1).all()) and bool((r["cs"][~hit] == 1).all())
    e_ss, e_cs = ssim_eval_bound(r, win)
    summing = located_additions(hv, hv) * U * hv * hv
    b_ss, b_cs = summing + float(e_ss[hit].sum()), summing + float(e_cs[hit].sum())
    small = min(float((r["ssim"][hit] - 1).abs().min()), float((r["cs"][hit] - 1).abs().min()))
    assert small >= 8 * max(b_ss, b_cs), f"located window at {pos}: the smallest |map - 1| = {small:.3e} is below 8 x the bound {max(b_ss, b_cs):.3e}"
    return X, Y, float((r["ssim"][hit] - 1).sum()), float((r["cs"][hit] - 1).sum()), b_ss, b_cs


def case_ssim_located(ops, dtype, flip=False):
    """One perturbed pixel under an asymmetric dyadic window: exactly the valid pixels whose window covers it leave 1, each by an
    amount set by g[i - r] g[j - c].  sums - count is compared with the float64 sum of (map - 1) over those pixels; three positions
    per launch, one per plane.  At the corners and edges the footprint is cut, so a flipped window index changes the sum."""
    p = ssim_params(G_ASYM, LOC_C, LOC_C)
    pos = located_positions()
    worst = 0.0
    for k in range(0, len(pos), 3):
        refs = [located_reference(q, p) for q in pos[k:k + 3]]
        X, Y = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
        got = _run_ssim(ops, X, Y, p).double() - LOC_HV * LOC_HV
        for j, (_, _, dss, dcs, bss, bcs) in enumerate(refs):
            for name, g_, w_, b_ in (("ssim", got[j, 0], dss, bss), ("cs", got[j, 1], dcs, bcs)):
                ratio = abs(float(g_) - w_) / b_
                worst = max(worst, ratio)
                assert ratio <= 1.0, (f"ssim_level located at {pos[k + j]}: sum of {name} - 1 is {float(g_)!r}, float64 {w_!r}: "
                                      f"error {abs(float(g_) - w_):.3e} outside the bound {b_:.3e}")
    _report("ssim", "located window", worst)


def case_ssim_one_pixel(ops, dtype, win=7, consts=K_REF, draws=32):
    """H = W = win: the plane sum is the single map value (0 + v through every addition is exact).  Random X, Y in [0, 1], one
    draw per plane, against float64 under ssim_eval_bound."""
    gen = _gen(260 + win)
    p = ssim_params(gauss(win), *consts)
    X, Y = torch.rand(draws, win, win, generator=gen), torch.rand(draws, win, win, generator=gen)
    r = ref_ssim(X, Y, p)
    e_ss, e_cs = ssim_eval_bound(r, win)
    got = _run_ssim(ops, X, Y, p).double()
    for name, o, ref, b in (("ssim", got[:, 0], r["ssim"].flatten(), e_ss.flatten()), ("cs", got[:, 1], r["cs"].flatten(), e_cs.flatten())):
        E.check_abs(o, ref, b, f"ssim_level one-pixel {name} win={win}", family="ssim")


# ================================================================================================ 6. dg_msssim_finish
def combine(inv_count, weights):
    c = _lib.MsssimCombine()
    for l, (i, w) in enumerate(zip(inv_count, weights)):
        c.inv_count[l], c.weight[l] = i, w
    return c


def ref_finish(sums, levels, planes, cmb):
    """float64: sum over planes of prod_l relu(sum_l * inv_count_l) ^ w_l (CS before the last scale, SSIM at it), NaN kept."""
    sm = d(sums).view(levels, planes, 2)
    v = torch.ones(planes, dtype=torch.float64)
    for l in range(levels):
        mean = sm[l, :, 0 if l == levels - 1 else 1] * float(cmb.inv_count[l])
        term = torch.where(mean < 0, torch.zeros_like(mean), mean)
        v = v * term ** float(cmb.weight[l])
    return v.sum()


def _run_finish(ops, sums, levels, planes, cmb):
    sb, out = Buf(ops, sums), Buf(ops, torch.full((1,), 7.0))
    ops.msssim_finish(sb.dev, levels, planes, cmb, out.dev)
    out.check("msssim_finish out"); sb.check("msssim_finish sums", written=False)
    return float(out.result()[0])


def case_finish(ops, dtype):
    """Against float64 within (POW_REL + planes * 2^-24) relative: the planes' values are non-negative, the final sum of ``planes``
    terms rounds at most planes times, and POW_REL covers the product of up to five powf's of one plane.  powf's error is not a
    derived number: it was measured on the device over this table and POW_REL is the power of two at or above
    4 x the worst seen, capped at 64 * 2^-24.  Exact where the arithmetic is: a negative CS mean or a zero term gives 0, terms of
    exactly 1 give exactly 1 per plane, a NaN sum gives NaN."""
    gen = _gen(270)
    count = 1600.0
    worst = 0.0
    table = [(lv, pl) for lv in (1, 3, 5) for pl in (1, 64, 65, 130)] + [(5, 1)] * 32
    for levels, planes in table:
        cmb = combine([1.0 / count] * levels, WEIGHTS if levels == 5 else (0.3001, 0.2363, 0.4636)[:levels])
        sums = ((torch.rand(levels, planes, 2, generator=gen) * 0.8 + 0.2) * count).float()
        ref = float(ref_finish(sums, levels, planes, cmb))
        got = _run_finish(ops, sums, levels, planes, cmb)
        rel = abs(got - ref) / ref
        worst = max(worst, rel / U)
        assert rel <= POW_REL + planes * U, f"msssim_finish levels={levels} planes={planes}: {got!r} vs {ref!r}, relative {rel / U:.2f} x 2^-24"
    _report("msssim_finish", "worst relative error of the value, in units of 2^-24 (not a ratio to the bound)", worst)
    # exact: count 64, inv_count 2^-6
    cmb = combine([1.0 / 64] * 3, (0.2, 0.3, 0.5))
    ones = torch.full((3, 130, 2), 64.0)
    assert _run_finish(ops, ones, 3, 130, cmb) == 130.0
    s = torch.full((3, 3, 2), 64.0)
    s[0, 1, 1] = -3.0          # plane 1: a negative CS mean at the first scale
    s[2, 2, 0] = 0.0           # plane 2: a zero SSIM mean at the last scale
    s[0, :, 0] = float("nan")  # the SSIM sum of a scale before the last is not read
    assert _run_finish(ops, s, 3, 3, cmb) == 1.0
    s[1, 0, 1] = float("nan")
    assert np.isnan(_run_finish(ops, s, 3, 3, cmb)), "a NaN mean must give NaN (torch.relu keeps it), not 0"


def case_chain(ops, dtype, c=2):
    """MsSsim(x, x) at 97 x 97, the smallest legal size: every plane sum is its count (case_ssim_count), count * fp32(1 / count) is
    within 2 * 2^-24 of 1, an exponent <= 1 and the running product keep each level within 4 * 2^-24, the five powf's are covered
    by POW_REL: |value - 1| <= levels * 4 * 2^-24 + POW_REL + planes * 2^-24.  A NaN pixel is skipped by min / max and reaches the
    value through the maps: the metric is NaN, as the reference's would be."""
    gen = _gen(280)
    x = randn((1, 97, 97, 16), dtype, gen).to(ops.device)
    ms = MsSsim(ops, 1, 97, 97, c_real=c)
    v = ms(x, x.clone())
    bound = ms.levels * 4 * U + POW_REL + c * U
    _report("msssim_finish", f"MsSsim(x, x) c={c}", abs(v - 1.0) / bound)
    assert abs(v - 1.0) <= bound, (v, bound)
    y = (x.float() + 0.3 * torch.randn(x.shape, generator=gen).to(ops.device)).to(x.dtype)
    assert 0.0 < ms(x, y) < 1.0
    xn = x.clone()
    xn[0, 40, 50, 0] = float("nan")
    assert np.isnan(ms(xn, y)), "MsSsim of a batch with a NaN"


# ================================================================================================ 7. dg_div_vort_sums
def ref_div_vort(hi, fi):
    """int64 restatement of the definition: u = channel 0 differenced along H, v = channel 1 along W, both on the [1:, 1:] window;
    {sum r, sum r^2, sum f, sum f^2, sum r f} of the divergence, then of the vorticity."""
    def dv(t):
        t = t.numpy().astype(np.int64)
        dudy = t[:, 1:, 1:, 0] - t[:, :-1, 1:, 0]
        dvdx = t[:, 1:, 1:, 1] - t[:, 1:, :-1, 1]
        return dudy + dvdx, dvdx - dudy
    (dr, vr), (df, vf) = dv(hi), dv(fi)
    five = lambda r, f: [int(r.sum()), int((r * r).sum()), int(f.sum()), int((f * f).sum()), int((r * f).sum())]
    return five(dr, df) + five(vr, vf)


def case_div_vort(ops, dtype, shape=(2, 9, 13), layout="dense", window_last=False, expect=None):
    """Integers |v| <= 64: |div|, |vort| <= 256, every product is below 2^17 and every double sum is an exact integer, so each of
    the ten sums EQUALS preload + reference.  Column 0 of channel 0 and row 0 of channel 1, which the definition never reads, hold
    NaN, and so do the pad channels."""
    N, H, W = shape
    guard_items(expect, "div_vort_sums", N * (H - 1) * (W - 1), DV_THREADS)
    gen = _gen(290)
    td = TD[dtype]
    bufs, ints = [], []
    for which in range(2):
        xi = torch.randint(-64, 65, (N, H, W, 2), generator=gen, dtype=torch.int8)
        v = xi.to(td)
        v[:, :, 0, 0] = float("nan")
        v[:, 0, :, 1] = float("nan")
        if layout == "ld16":
            full = torch.full((N, H, W, 16), float("nan"), dtype=td)
            full[..., :2] = v
            bufs.append(Buf(ops, full))
        else:
            bufs.append(Buf(ops, v, slab=(E.V_SLAB, E.V_SLAB2)[which] if layout == "slab" else None))
        ints.append(xi)
    pre = torch.arange(1000, 1010, dtype=torch.float64)
    sums = Buf(ops, pre)
    ops.div_vort_sums(bufs[0].dev, bufs[1].dev, sums.dev)
    ref = torch.tensor(ref_div_vort(*ints), dtype=torch.float64) + pre
    assert float(ref.abs().max()) < 2.0 ** 53
    check_values(sums.result(), ref, f"div_vort_sums {shape} {layout}")
    sums.check("div_vort sums"); bufs[0].check("hr", written=False); bufs[1].check("fake", written=False)


# ================================================================================================ 8. dg_moments / dg_stage_fields
MOM_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024)


def case_moments(ops, dtype, sizes=MOM_SIZES, expect=None):
    """Integer data (|v| <= 64: the sum of squares stays far below 2^53) with NaN at element 0, in the four-wide body and in the
    tail; the three double moments EQUAL the integer reference over the other elements, on top of an integer preload.  A +inf
    element gives inf / inf and is counted."""
    gen = _gen(300)
    for n in sizes:
        guard_cap(expect, f"moments n={n}", _cdiv(n // 4, 256), MOM_BLOCKS)
        for nans in (False, True):
            xi = torch.randint(-64, 65, (n,), generator=gen, dtype=torch.int64)
            x = xi.float()
            keep = torch.ones(n, dtype=torch.bool)
            if nans:
                for i in {0, n // 2, (n // 4) * 4 - 1, n - 1}:        # element 0, the body, its last element, the tail (or the end)
                    if 0 <= i < n:
                        keep[i] = False
                x[~keep] = float("nan")
            pre = torch.tensor([17.0, 23.0, 5.0], dtype=torch.float64)
            xb, acc = Buf(ops, x), Buf(ops, pre)
            ops.moments(xb.dev, acc.dev)
            k = xi[keep]
            ref = pre + torch.tensor([int(k.sum()), int((k * k).sum()), int(k.numel())], dtype=torch.float64)
            check_values(acc.result(), ref, f"moments n={n} nans={nans}")
            acc.check("moments acc"); xb.check("moments x", written=False)
    x = torch.tensor([1.0, float("inf"), float("nan"), -2.0, 3.0])
    acc = Buf(ops, torch.zeros(3, dtype=torch.float64))
    ops.moments(x.to(ops.device), acc.dev)
    check_values(acc.result(), torch.tensor([float("inf"), float("inf"), 4.0], dtype=torch.float64), "moments with +inf")


def ref_stage(planes, mean, inv_std, tdtype):
    """numpy float32: (plane - mean) * inv_std, one subtraction and one product (they cannot fuse), then one RNE for bf16."""
    cols = []
    with np.errstate(all="ignore"):
        for t, m, s in zip(planes, mean, inv_std):
            cols.append((t.numpy().reshape(-1) - np.float32(m)) * np.float32(s))
    out = np.stack(cols, axis=1)
    assert out.dtype == np.float32
    return torch.from_numpy(out).to(tdtype)


def case_stage(ops, dtype, npix=257, c=3, identity=False, expect=None):
    guard_items(expect, "stage_fields", npix, STAGE_THREADS)
    gen = _gen(310 + c)
    planes = [torch.randn(npix, generator=gen) * (k + 1) + 270.0 * (k % 2) for k in range(c)]
    for k, t in enumerate(planes):
        if npix > 1:
            t[(7 * k) % npix] = float("nan")          # NaN passes through in place
    mean = [0.0] * c if identity else [E.f32(float(t[~torch.isnan(t)].mean())) + 0.125 * k for k, t in enumerate(planes)]
    inv = [1.0] * c if identity else [E.f32(1.0 / (0.37 + k)) for k in range(c)]
    pb = [Buf(ops, t) for t in planes]
    dst = Buf(ops, randn((npix, c), dtype, gen))
    ops.stage_fields([b.dev for b in pb], mean, inv, dst.dev)
    what = f"stage_fields npix={npix} c={c}{' identity' if identity else ''}"
    assert_bits_nan(dst.result(), ref_stage(planes, mean, inv, TD[dtype]), what)
    if identity and dtype == "f32":
        assert_bits_nan(dst.result(), torch.stack(planes, 1), what + ": identity statistics copy bits")
    dst.check(what)
    for b in pb:
        b.check(what + " plane", written=False)


# ================================================================================================ the table
def _c(cid, fn, size, **kw):
    return (cid, fn, kw, size)


CASES = [
    _c("lowpass-c8", case_lowpass, "small", C=8),
    _c("lowpass-c16", case_lowpass, "small", C=16),
    _c("lowpass-c24", case_lowpass, "small", C=24),
    _c("lowpass-c8-view", case_lowpass, "view", C=8, view=True),
    _c("lowpass-c24-view", case_lowpass, "view", C=24, view=True),
    _c("lowpass-normal", case_lowpass_normal, "small"),
    _c("avgpool", case_avgpool, "small"),
    _c("minmax-values-ld16", case_minmax_values, "small", layout="ld16"),
    _c("minmax-values-dense", case_minmax_values, "small", layout="dense"),
    _c("minmax-values-slab", case_minmax_values, "view", layout="slab"),
    _c("normalise-1x1x1", case_normalise, "small", shape=(1, 1, 1), C=1, layout="dense"),
    _c("normalise-index-c2", case_normalise, "small", shape=(2, 5, 7), C=2, layout="ld16", data="index"),
    _c("normalise-c8-ld16", case_normalise, "small", shape=(3, 33, 47), C=8, layout="ld16"),
    _c("normalise-c2-dense", case_normalise, "small", shape=(2, 5, 7), C=2, layout="dense"),
    _c("normalise-c8-slab", case_normalise, "view", shape=(3, 33, 47), C=8, layout="slab"),
    _c("normalise-c1-slab", case_normalise, "view", shape=(2, 5, 7), C=1, layout="slab"),
    _c("normalise-const", case_normalise, "small", shape=(2, 5, 7), C=2, layout="ld16", data="const"),
    _c("ssim-count-win1", case_ssim_count, "small", win=1, rot=0),
    _c("ssim-count-win3", case_ssim_count, "small", win=3, rot=1),
    _c("ssim-count-win7", case_ssim_count, "small", win=7, rot=2),
    _c("ssim-count-win7-asym", case_ssim_count, "small", win=7, rot=0, asym=True),
    _c("ssim-count-win11", case_ssim_count, "small", win=11, rot=1),
    _c("ssim-located", case_ssim_located, "small"),
    _c("ssim-one-pixel-win3", case_ssim_one_pixel, "small", win=3),
    _c("ssim-one-pixel-win7", case_ssim_one_pixel, "small", win=7),
    _c("ssim-one-pixel-win11", case_ssim_one_pixel, "small", win=11),
    _c("msssim-finish", case_finish, "small"),
    _c("msssim-chain-c1", case_chain, "small", c=1),
    _c("msssim-chain-c2", case_chain, "small", c=2),
    _c("moments", case_moments, "small"),
    _c("moments-cap-filled", case_moments, "small", sizes=(4 * 256 * 2048 + 3,)),
    # large: GPU only; each asserts from its own shape what it is there for
    _c("lowpass-large", case_lowpass_large, "large", expect="cap"),
    _c("avgpool-large", case_avgpool, "large", shapes=[(1675, 1675)], planes=(3,), expect="second_trip"),
    _c("minmax-located-second-trip", case_minmax_located, "large", pixels=65536 + 257, C=8, layout="ld16", expect="second_trip"),
    _c("normalise-large", case_normalise, "large", shape=(1, 1449, 1449), C=2, layout="dense", expect="second_trip"),
    _c("div_vort-513x514", case_div_vort, "large", shape=(1, 513, 514), layout="dense", expect="second_trip"),
    _c("moments-cap", case_moments, "large", sizes=(4 * 256 * (2048 + 1) + 3,), expect="cap"),
    _c("stage-large", case_stage, "large", npix=4096 * 256 + 257, c=3, expect="second_trip"),
]
for _px in (1, 255, 256, 257):
    for _C, _lay in ((1, "dense"), (2, "ld16"), (5, "dense"), (8, "ld16")):
        CASES.append(_c(f"minmax-located-{_px}-c{_C}-{_lay}", case_minmax_located, "small", pixels=_px, C=_C, layout=_lay))
    CASES.append(_c(f"minmax-located-{_px}-c5-slab", case_minmax_located, "view", pixels=_px, C=5, layout="slab"))
for _shape in ((1, 2, 2), (1, 2, 9), (3, 7, 2), (2, 9, 13)):
    for _lay in ("dense", "ld16"):
        CASES.append(_c(f"div_vort-{'x'.join(map(str, _shape))}-{_lay}", case_div_vort, "small", shape=_shape, layout=_lay))
    CASES.append(_c(f"div_vort-{'x'.join(map(str, _shape))}-slab", case_div_vort, "view", shape=_shape, layout="slab"))
for _c_ in (1, 3, 8):
    for _np in (1, 255, 257):
        CASES.append(_c(f"stage-{_np}-c{_c_}", case_stage, "small", npix=_np, c=_c_))
CASES.append(_c("stage-identity", case_stage, "small", npix=257, c=3, identity=True))

