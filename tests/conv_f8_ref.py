"""Exact integer-data tests of the MXFP8 kernels: operands, float64 references and the case table shared by
tests/test_conv_f8_exact_gpu.py (HipOps) and tests/test_conv_f8_exact_cpu.py (EmuOps).  The method is that of tests/conv_ref.py,
whose references, epilogues, destinations and comparator are reused; what is new is that the BLOCK SCALES are part of the exact data.

Kernels: gg_halo4w_f8_kernel<S2, NW, SEG> (csrc/conv_halo_f8.hip) behind dg_conv3x3_fwd_f8 / dg_conv3x3_dgrad_f8 and gg_launch_f8
(csrc/conv_plan.hip), and wg3w_f8_kernel<S2> with its dense-block mode (csrc/wgrad.hip) behind dg_conv3x3_wgrad_f8 /
dg_conv3x3_wgrad_dense_f8.

Why bits.  E4M3 holds the integers up to 16 exactly and an E8M0 scale is a power of two.  Operands are built directly in the
kernels' input format: E4M3 bytes of integers (|xq| <= 8, |wq| <= 3), scale bytes per (pixel, 32-channel block) of the source and
per (row = output channel x tap, block) of the weight pack, handed over as ``xq=(q, s)`` / ``wq=(q, s)``.  The x scales lie D
below 127 and the w scales D above, so every product is an integer multiple of 2^0 and the budget of ``wide_spreads`` keeps every
partial sum IN ANY ORDER, and every epilogue step, below 2^24 in units of 2^-f: fp32 holds all of it exactly and the stored bf16
value must EQUAL the float64 reference.  A scale byte taken from the wrong pixel, block, tap row or (on a partial channel tile)
neighbouring row, two scale bytes swapped, or the x scale of block b applied to block b+-1 gives another integer.  D = 40 in one
case checks that the two scales are applied jointly (2^-40 * 2^40), not one after the other in a narrower format.

Two data regimes per forward / data-gradient case.  "wide": the above with the largest scale spreads the budget allows; its sums
reach 1e5 and most are not representable in bf16, so the final rounding can hide a one-unit error.  "fine": xq, wq in {-1, 0, 1},
scale spreads {0, 1}, a sparse source, float64 accumulator within 256 - (the largest addend): every stored bf16 value is then the
exact integer (or multiple of 2^-f) and a single wrong unit anywhere shows.

The reference dequantises with its OWN 256-entry E4M3 table written from the OCP definition (``E4M3``; cross-checked against
torch.float8_e4m3fn in the CPU file), multiplies by 2^(s - 127) in float64 and applies conv_ref's float64 convolution and epilogue;
it does not go through EmuOps.mx_dequant or _gather_gemm.

The assumption behind it -- v_mfma_scale_f32_16x16x128_f8f6f4 / _32x32x64_ return the exact integer for such chains -- is measured
first on the device by the smallest case with the plain epilogue (signed and one-sign data, D = 7 and D = 40; the one-sign sums pass
2^23 and include odd integers) and by the smallest weight-gradient case (signed |v| <= 8 over 256 pixels; one-sign data of 120 and
odd integers below 16 over 1024 pixels, the fewest at which such sums pass 2^23 in units of the block pair's scale; exponents within
8 of 127 and from [100, 150)).  ``F8_INT_LIMIT`` is the budget those tests support.  MEASURED on the MI355X: all eight variants
return the exact integer, so F8_INT_LIMIT = 2^24 and neither regime is narrowed.  What is NOT exact, found with a first version of
the one-sign weight-gradient data (240 instead of 120): products of ONE MFMA that span more than about 2^14 -- 1 ... 120^2 = 2^13.8
inside a 32-element scale block is exact, 1 ... 240^2 = 2^15.8 loses up to 7 units per 64-pixel step by truncation towards zero,
whatever the size of the sum (all-240 data is exact at 2^23.8).  Hence the second budget ``F8_PRODUCT_BITS``: the largest product of a
launch stays below 2^14 times the smallest unit (the wide regime reaches 24 * 2^9 = 2^13.6 across scale blocks, exactly).
DESIGN.md section 7, "Exact fp8 tests".

Weight gradients: |xq|, |dyq| <= 8, block exponents ex[Cin/32], ey[Cout/32] drawn independently from [100, 150) -- they factor out
of the pixel contraction, so any exponents stay exact --, preload dw = integer x 2^(ex + ey - 254) per (co-block, ci-block) inside
guards, fp32 bits against ``ref_wgrad`` of the dequantised operands.

Case table: every case names the path it exists for; the guard restates dg_conv3x3_fwd_f8 / _dgrad_f8 / gg_launch_f8 /
gg_launch_halo_f8 on the planner's own descriptors.  One listed shape does not take the path it was proposed for: a stride-2 data
gradient with 80 outputs is ACCEPTED by seg_dgrad_desc (it refuses <= 64), so (1,32,32,80,128,2) is a merged launch with a partial
channel tile ("f8-seg-dgrad-80-128-32x32").  With fp8 operands the only way to four per-class launches is the row-step test of
seg_dgrad_desc on the bf16 tensor's pixel stride (Ws * ldy * 2 >= 2^23): "f8-classes-dgrad-128-128-32x32-rowstep" hands over an
adjoint that is a channel slice of a tensor 2^18 channels wide (the kernel itself reads the fp8 form, whose stride is 128).
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import torch

from downgan_amd.ops import Conv, pix_layout
from tests.conv_ref import (EP_F, MAG_ADD, PATH_BITS, WGRAD_CODE, Dest, _gen, assert_bits_at, build_epilogue, case_epilogues, conv_acc,
                            dev, dgrad_acc, ints, plan, ref_dgrad, ref_fwd, ref_wgrad)

F8_INT_LIMIT = 1 << 24      # integer budget of a scaled-MFMA chain (see the module docstring)
F8_PRODUCT_BITS = 14        # ... whose products, within one MFMA, span less than 2^14 from the smallest unit to the largest product
MAG_XQ, MAG_WQ = 8, 3       # E4M3 integers of the source / adjoint and of the weight pack in the wide regime
FINE_ADD = 8                # addends of the fine regime
FINE_MAX = 256              # bf16 holds every integer up to here
D_DEFAULT, D_FAR = 7, 40
SRC_PAD, SRC_LO = 256, 128  # slab cases: the fp8 source is bytes [128, 128 + C) of a tensor C + 256 wide,
XS_PAD, XS_LO = 8, 4        # its scale rows bytes [4, 4 + C/32) of rows C/32 + 8 wide
BIG_LDY = 1 << 18           # pixel stride of the bf16 adjoint that makes seg_dgrad_desc refuse a 16-pixel row (16 * 2^18 * 2 = 2^23)
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- E4M3 / E8M0
def _e4m3_table():
    """OCP 8-bit floating point, E4M3: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 = subnormals m/8 * 2^-6; no
    infinities; S.1111.111 = NaN."""
    t = []
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if b & 0x7f == 0x7f:
            v = float("nan")
        elif e == 0:
            v = m / 8.0 * 2.0 ** -6
        else:
            v = (1 + m / 8.0) * 2.0 ** (e - 7)
        t.append(-v if b & 0x80 else v)
    return torch.tensor(t, dtype=torch.float64)


E4M3 = _e4m3_table()
_ENC_MAX = 448
_ENC = torch.full((_ENC_MAX + 1,), 0xff, dtype=torch.uint8)       # E4M3 byte of every non-negative integer the format holds (0xff: none)
for _b in range(0x7f):
    if float(E4M3[_b]) == int(E4M3[_b]):
        _ENC[int(E4M3[_b])] = _b


def encode(v):
    """int64 integers the format holds exactly (every |v| <= 16, then 18, 20, ... 448) -> their E4M3 bytes (0 -> +0)."""
    assert int(v.abs().max()) <= _ENC_MAX
    q = _ENC[v.abs()] | ((v < 0).to(torch.uint8) << 7)
    assert torch.equal(E4M3[q.long()], v.double()), "not an integer E4M3 holds"
    return q


def decode(q):
    return E4M3[q.long()]


def scale_of(s):
    """E8M0 bytes [..., nb] -> float64 2^(s - 127) per channel [..., 32 * nb]."""
    return torch.ldexp(torch.ones(s.shape, dtype=torch.float64), s.to(torch.int32) - 127).repeat_interleave(32, dim=-1)


def dequant(q, s):
    """(E4M3 bytes [..., C], E8M0 bytes [..., C/32] or one row [C/32] for every pixel) -> float64 values."""
    return decode(q) * scale_of(s)


# ---------------------------------------------------------------------------------------------------------------- budgets
def assert_wide_budget(K, sx, sw, f, addends=4 * MAG_ADD, limit=None):
    """Sum budget and product window (F8_PRODUCT_BITS) of a wide-regime launch."""
    limit = (F8_INT_LIMIT if limit is None else limit) >> f
    assert sx >= 0 and sw >= 0 and MAG_XQ * MAG_WQ * (1 << (sx + sw)) * K + addends < limit, \
        f"no integer budget: K={K} spreads {sx}+{sw} addends={addends} f={f} limit=2^{limit.bit_length() - 1}"
    assert MAG_XQ * MAG_WQ * (1 << (sx + sw)) < (1 << F8_PRODUCT_BITS), f"no integer budget: products of one MFMA span more than 2^{F8_PRODUCT_BITS}"


def wide_spreads(K, f, limit=None):
    """The largest scale spreads (sx, sw) of a launch that adds K products |xq * wq| <= 8 * 3 * 2^(sx + sw) and then the addends
    (bias, two residuals, preload: 4 * MAG_ADD), with f fractional bits from the epilogue's scalars; the largest product stays
    below 2^F8_PRODUCT_BITS times the smallest."""
    t = 0
    while (MAG_XQ * MAG_WQ * (1 << (t + 1)) * K + 4 * MAG_ADD < ((F8_INT_LIMIT if limit is None else limit) >> f)
           and MAG_XQ * MAG_WQ * (1 << (t + 1)) < (1 << F8_PRODUCT_BITS)):
        t += 1
    sx, sw = (t + 1) // 2, t // 2
    assert_wide_budget(K, sx, sw, f, limit=limit)
    return sx, sw


def assert_fine_budget(acc, what=""):
    """A condition on the float64 reference alone: the accumulator plus the largest addend of any epilogue (bias OR preload at
    FINE_ADD; residuals enter behind a scalar of 0.5) stays within the integers bf16 holds."""
    m = float(acc.abs().max())
    assert m <= FINE_MAX - FINE_ADD, f"fine regime {what}: max |v| = {m} above {FINE_MAX - FINE_ADD}; lower the case's density"


def assert_wgrad_budget(Mpix, mag=MAG_XQ, limit=None):
    assert mag * mag * Mpix + MAG_ADD < (F8_INT_LIMIT if limit is None else limit), f"no integer budget: {Mpix} pixels of |xq|, |dyq| <= {mag}"
    assert mag * mag < (1 << F8_PRODUCT_BITS), f"no integer budget: products of one MFMA span more than 2^{F8_PRODUCT_BITS}"


# ---------------------------------------------------------------------------------------------------------------- dispatch
def _f8_desc_path(d, ldxq):
    """gather_gemm_impl's fp8 checks, gg_launch_f8 and gg_launch_halo_f8 for one planned descriptor whose source stride is ldxq."""
    if d.Cred % 128 or ldxq % 16 or (d.Cred // 16) % 8 or d.Nout <= 64 or d.Hg < 8 or d.Wg < 8 or d.src_ps:
        return "refused"
    if d.sy_mul == 1 and d.sx_mul == 1 and d.Hs == d.Hg and d.Ws == d.Wg:
        return "f8_halo"
    if d.sy_mul == 2 and d.sx_mul == 2 and d.Hs == 2 * d.Hg and d.Ws == 2 * d.Wg and d.dy_mul == 1 and d.dx_mul == 1 and not d.dst_ps:
        return "f8_s2_8w" if d.Nout % 256 == 0 and 2 * d.Ws * ldxq < (1 << 23) else "f8_s2_4w"
    return "refused"


def _seg_ok(ds):
    """seg_dgrad_desc (csrc/conv_plan.hip) on the bf16 plan: its row-step test sees the bf16 tensor's pixel stride."""
    d0 = ds[0]
    return (len(ds) == 4 and not d0.src_ps and not d0.dst_ps and (d0.Cred // 8) % 8 == 0 and d0.Nout > 64 and d0.Hg >= 8 and d0.Wg >= 8
            and [d.ntaps for d in ds] == [1, 2, 2, 4] and d0.Ws * d0.lds * 2 < (1 << 23))


def f8_conv_path(cv, kind, ldxq, ldx, ldy):
    """The path dg_conv3x3_fwd_f8 (kind 0) / dg_conv3x3_dgrad_f8 (kind 1) takes, from the planner's descriptors."""
    _, ds = plan(cv, "bf16", kind, ldx, ldy)
    if kind == 0:
        return "refused" if cv.Cin % 128 else _f8_desc_path(ds[0], ldxq)
    if cv.pixel_shuffle or cv.Cout % 128 or cv.Cin % 16:
        return "refused"
    if _seg_ok(ds) and ds[0].Cred % 128 == 0:
        return "f8_seg_interleaved" if ds[0].Cred * ds[0].Nout * 18 <= (2 << 20) else "f8_seg_per_image"
    paths = {_f8_desc_path(d, ldxq) for d in ds}
    if len(ds) == 1:
        return paths.pop()
    return "f8_per_class" if paths == {"f8_halo"} else "refused"


def f8_wgrad_path(cv, ldx, ldy):
    """dg_conv3x3_wgrad_f8's acceptance (csrc/wgrad.hip)."""
    ok = (not cv.pixel_shuffle and cv.Cin % 128 == 0 and cv.Cout % 128 == 0 and cv.Wo % 64 == 0 and ldx >= cv.Cin and ldy >= cv.Cout
          and ldx % 16 == 0 and ldy % 16 == 0)
    return "f8" if ok else "refused"


F8_PATHS = ("f8_halo", "f8_s2_4w", "f8_s2_8w", "f8_seg_interleaved", "f8_seg_per_image", "f8_per_class")


# ---------------------------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass(frozen=True)
class F8Case:
    id: str
    kind: str                      # "fwd", "dgrad"
    shape: tuple                   # (N, H, W, Cin, Cout, stride)
    expect: str                    # a name of F8_PATHS
    eps: tuple = ()                # names of EPILOGUES ("" = all the path accepts)
    slab: bool = False             # source a channel slice of wider byte / scale tensors, destination a slab slice
    ps: bool = False               # pixel-shuffled destination (net "T", ops built with f8_generator=True)
    uniform: bool = False          # uniform-scale source: ONE scale row for every pixel (ldxs < 0)
    D: int = D_DEFAULT
    regimes: tuple = ("wide", "fine")
    big_ldy: bool = False          # data gradient: the bf16 adjoint has a pixel stride of BIG_LDY
    density: float = 1.0           # fine regime: factor on the default share of non-zero source elements

    @property
    def net(self):
        return "T" if self.ps else "C"

    def conv(self):
        N, H, W, ci, co, st = self.shape
        return Conv(N, H, W, ci, co, st, self.ps, net=self.net)


@dataclasses.dataclass(frozen=True)
class F8WCase:
    id: str
    kind: str                      # "wgrad": shape (N, H, W, Cin, Cout, stride); "dense": (N, H, W, n)
    shape: tuple
    sliced: bool = False           # operands are channel slices of wider byte tensors


@dataclasses.dataclass
class F8Data:
    cv: Conv
    xq: torch.Tensor               # int64 integers of the source [N, Hs, Ws, Cred]
    xs: torch.Tensor               # uint8 scale bytes [N, Hs, Ws, Cred/32], or [Cred/32] for a uniform source
    wq: torch.Tensor               # int64 integers of the weight pack [Nout * 9, Cred]
    ws: torch.Tensor               # uint8 [Nout * 9, Cred/32]
    acc: torch.Tensor              # float64 accumulator of the reference
    pre: torch.Tensor
    dshape: tuple
    mag_add: int
    gstate: torch.Tensor


def operand_values(case, xb, xs, wb, ws):
    """float64 (source, weight pack, master weight [Cout][9][Cin]) of E4M3 / E8M0 bytes; a data gradient's pack is [Cin][9][Cout]
    with scale blocks along Cout, the master its transpose."""
    cv = case.conv()
    xv, wv = dequant(xb, xs), dequant(wb, ws)
    master = wv.view(cv.Cout, 9, cv.Cin) if case.kind == "fwd" else wv.view(cv.Cin, 9, cv.Cout).permute(2, 1, 0).contiguous()
    return xv, wv, master


def accumulator(case, xv, master):
    cv = case.conv()
    return conv_acc(cv, xv, master) if case.kind == "fwd" else dgrad_acc(cv, xv, master)


_f8_data = {}


def f8_data(case, regime, names=None, positive=False, D=None):
    """Operands and the float64 accumulator of a case for the epilogues ``names``, built once.  ``positive`` (wide regime): operands of
    one sign near the top of their range, with most scales at the top of their spread and one in sixteen at its bottom -- the sums
    come close to the budget and still take odd values."""
    names = tuple(names or case_epilogues(case, "bf16"))
    f = max(EP_F[n] for n in names)
    D = case.D if D is None else D
    key = (case, regime, f, positive, D, F8_INT_LIMIT)
    if key in _f8_data:
        return _f8_data[key]
    cv, fwd = case.conv(), case.kind == "fwd"
    gen = _gen(sum(map(ord, case.id)) * 8 + 4 * (regime == "fine") + 2 * positive + (D != D_DEFAULT))
    nout, cred = (cv.Cout, cv.Cin) if fwd else (cv.Cin, cv.Cout)
    nb = cred // 32
    oshape = (cv.N, 2 * cv.Ho, 2 * cv.Wo, cv.Cout // 4) if cv.pixel_shuffle else (cv.N, cv.Ho, cv.Wo, cv.Cout)
    sshape, dshape = ((cv.N, cv.H, cv.W, cv.Cin), oshape) if fwd else ((cv.N, cv.Ho, cv.Wo, cv.Cout), (cv.N, cv.H, cv.W, cv.Cin))
    xs_shape = (nb,) if case.uniform else sshape[:-1] + (nb,)
    rnd = lambda lo, hi, shape: torch.randint(lo, hi + 1, tuple(shape), generator=gen, dtype=torch.int64)
    if regime == "wide":
        sx, sw = wide_spreads(9 * cred, f)
        mag_add = MAG_ADD
        if positive:
            top = lambda s, shape: torch.where(rnd(0, 15, shape) > 0, s, 0)
            xq, wq = rnd(MAG_XQ - 1, MAG_XQ, sshape), torch.where(rnd(0, 7, (nout * 9, cred)) > 0, MAG_WQ, MAG_WQ - 1)
            xo, wo = top(sx, xs_shape), top(sw, (nout * 9, nb))
        else:
            xq, wq = rnd(-MAG_XQ, MAG_XQ, sshape), rnd(-MAG_WQ, MAG_WQ, (nout * 9, cred))
            xo, wo = rnd(0, sx, xs_shape), rnd(0, sw, (nout * 9, nb))
    else:
        assert regime == "fine" and not positive
        mag_add = FINE_ADD
        share = min(1.0, 32.0 / cred * case.density * (2.25 if not fwd and cv.stride == 2 else 1.0))
        xq = torch.where(torch.rand(sshape, generator=gen) < share, 2 * rnd(0, 1, sshape) - 1, 0)
        wq = rnd(-1, 1, (nout * 9, cred))
        xo, wo = rnd(0, 1, xs_shape), rnd(0, 1, (nout * 9, nb))
    xs, ws = (127 - D + xo).to(torch.uint8), (127 + D + wo).to(torch.uint8)
    xv, _, master = operand_values(case, encode(xq), xs, encode(wq), ws)
    acc = accumulator(case, xv, master)
    assert torch.equal(acc, acc.round()), "the accumulator of integer data is an integer"
    if regime == "wide":
        assert float(acc.abs().max()) + 4 * MAG_ADD < (F8_INT_LIMIT >> f)
    else:
        assert_fine_budget(acc, case.id)
    pre = ints(dshape, mag_add, gen, "bf16")
    _f8_data[key] = F8Data(cv, xq, xs, wq, ws, acc, pre, dshape, mag_add, gen.get_state())
    return _f8_data[key]


def reference(case, d, name, kw, sign, acc=None):
    """(stored bf16 tensor, expected out_bits or None) of one epilogue."""
    refkw = {k: v for k, v in kw.items() if k not in ("mask_bits", "out_bits")}
    fn = ref_fwd if case.kind == "fwd" else ref_dgrad
    _, stored, bits = fn(d.cv, None, None, d.pre, "bf16", acc=d.acc if acc is None else acc, mask_sign=sign, want_bits="out_bits" in kw, **refkw)
    return stored, bits


def _garbage(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed), dtype=torch.int64)


def run_f8_conv_case(make_ops, case, regime, only=None, positive=False, D=None, mutate=None, selfq=False):
    """One forward / data-gradient case for every epilogue it takes (``only``: one of them) on ``make_ops(case)``.
    ``mutate(xq, xs, wq, ws)`` (CPU mutation checks) returns the operands handed over instead of the ones the reference was computed
    from.  ``selfq``: the self-quantised route -- the call gets the dequantised bf16 tensors only and the library quantises them."""
    ops = make_ops(case)
    hip = ops.name == "hip"
    names = case_epilogues(case, "bf16") if only is None else [only]
    d = f8_data(case, regime, names, positive, D)
    cv, fwd = d.cv, case.kind == "fwd"
    nout, cred = (cv.Cout, cv.Cin) if fwd else (cv.Cin, cv.Cout)
    assert ops.f8_eligible(cv, case.kind), f"{case.id}: the ops object would not take the fp8 path"
    xq, xs, wq, ws = (d.xq, d.xs, d.wq, d.ws) if mutate is None else mutate(d.xq.clone(), d.xs.clone(), d.wq.clone(), d.ws.clone())
    xb, wb = encode(xq), encode(wq)
    xv, wv, _ = operand_values(case, xb, xs, wb, ws)
    x16, w16 = xv.to(BF16), wv.reshape(-1).to(BF16)          # the bf16 arguments hold the same values, exactly
    assert torch.equal(x16.double(), xv) and torch.equal(w16.double(), wv.reshape(-1))
    if case.slab:
        assert not case.uniform and not selfq
        wide = encode(_garbage(xb.shape[:-1] + (cred + SRC_PAD,), -MAG_XQ, MAG_XQ, 13))
        wide[..., SRC_LO:SRC_LO + cred] = xb
        swide = _garbage(xs.shape[:-1] + (cred // 32 + XS_PAD,), 100, 150, 17).to(torch.uint8)
        swide[..., XS_LO:XS_LO + cred // 32] = xs
        xq_dev, xs_dev = dev(ops, wide)[..., SRC_LO:SRC_LO + cred], dev(ops, swide)[..., XS_LO:XS_LO + cred // 32]
    else:
        xq_dev, xs_dev = dev(ops, xb), dev(ops, xs)
    if case.big_ldy:
        assert not fwd
        x_dev = torch.zeros(x16.shape[:-1] + (BIG_LDY,), dtype=BF16, device=ops.device)[..., :cred]
        x_dev.copy_(x16)
    else:
        x_dev = dev(ops, x16)
    w_dev, wq_dev, ws_dev = dev(ops, w16), dev(ops, wb), dev(ops, ws)
    f8_args = {} if selfq else dict(xq=(xq_dev, xs_dev), wq=(wq_dev, ws_dev))
    gen = torch.Generator()
    gen.set_state(d.gstate)
    for name in names:
        kw, sign = build_epilogue(name, d.dshape, nout, "bf16", gen, ps=fwd and cv.pixel_shuffle, mag=d.mag_add)
        what = f"{case.id} {regime} {name}" + (" one-sign" if positive else "") + (f" D={D}" if D is not None else "") + (" self-quantised" if selfq else "")
        dst = Dest(ops, d.pre, slab=case.slab)
        ldsrc, lddst = pix_layout(x_dev)[0], pix_layout(dst.dev)[0]
        ldx, ldy = (ldsrc, lddst) if fwd else (lddst, ldsrc)
        ldxq = cred if selfq else xq_dev.stride(2)
        path = f8_conv_path(cv, 0 if fwd else 1, ldxq, ldx, ldy)
        assert path == case.expect, f"case guard: {what} would take {path}, the case is there for {case.expect}"
        if case.slab:
            assert ldxq > cred and xs_dev.stride(2) > cred // 32 and xs_dev.stride(2) % 4 == 0
        kwd = {k: (dev(ops, v) if torch.is_tensor(v) else v) for k, v in kw.items()}
        (ops.conv_fwd if fwd else ops.conv_dgrad)(cv, x_dev, w_dev, dst.dev, **f8_args, **kwd)
        if hip:
            kinds = ops.lib.dg_last_conv_kernels()
            assert kinds == PATH_BITS["f8"], f"{what}: dg_last_conv_kernels() = {kinds}, the fp8 kernel leaves {PATH_BITS['f8']}"
            if not fwd:
                g, ds = plan(cv, "bf16", 1, ldx, ldy)
                merged = path.startswith("f8_seg") or len(ds) == 1
                assert (path == "f8_per_class") == (not merged)
                assert ops.lib.dg_conv3x3_dgrad_launches(C.byref(g)) == (1 if merged else 4), what
        stored, bits = reference(case, d, name, kw, sign)
        assert_bits_at(dst.result(), stored, what)
        dst.check(what)
        if bits is not None:
            assert_bits_at(kwd["out_bits"].cpu(), bits, f"{what}: out_bits")


# ---------------------------------------------------------------------------------------------------------------- weight gradients
def _wide_slice(ops, q, pad=128, lo=64, seed=19):
    """``q`` as channels [lo, lo + C) of a byte tensor C + pad wide on the device."""
    Cc = q.shape[-1]
    wide = encode(_garbage(q.shape[:-1] + (Cc + pad,), -MAG_XQ, MAG_XQ, seed))
    wide[..., lo:lo + Cc] = q
    return dev(ops, wide)[..., lo:lo + Cc]


def _exponents(gen, n, narrow, hi):
    if narrow:      # within 8 of 127, x below and dy above: the products' scales stay near 1
        return torch.randint(127, 135, (n,), generator=gen).to(torch.uint8) if hi else torch.randint(120, 128, (n,), generator=gen).to(torch.uint8)
    return torch.randint(100, 150, (n,), generator=gen).to(torch.uint8)


def _unit(cout, cin, ex, ey):
    """2^(ex + ey - 254) per (co-block, ci-block) as float64 [cout, 1, cin]: the unit the sums of that block pair are integers of."""
    return torch.ldexp(torch.ones(cout, 1, cin, dtype=torch.float64),
                       (ey.int().repeat_interleave(32)[:, None, None] + ex.int().repeat_interleave(32)[None, None, :] - 254))


def _preload(gen, cout, cin, ex, ey):
    """integers in [-64, 64] x 2^(ex + ey - 254) per (co-block, ci-block), [cout, 9, cin] in fp32 (exactly)."""
    v = ints((cout, 9, cin), MAG_ADD, gen, torch.float32).double() * _unit(cout, cin, ex, ey)
    assert torch.equal(v.float().double(), v)
    return v.float()


MAG_ONE_SIGN = 120          # 15 * 8: the E4M3 integer of the one-sign weight-gradient data (120^2 = 2^13.8; * 1024 pixels = 0.88 * 2^24)
_f8_wdata = {}


def f8_wgrad_data(case, positive=False, narrow=False):
    """(cv, xb, dyb, ex, ey, dw0, float64 reference, the reference in units of its block pair's scale) of a weight-gradient case.
    ``positive``: the data of the assumption test -- seven of eight elements are 120, the others odd integers below 16, all of one
    sign, so that over 1024 pixels the sums pass 2^23 and take odd values while one MFMA's products span 1 ... 2^13.8."""
    key = (case, positive, narrow)
    if key not in _f8_wdata:
        N, H, W, ci, co, st = case.shape
        cv = Conv(N, H, W, ci, co, st, net="C")
        gen = _gen(sum(map(ord, case.id)) * 4 + 2 * positive + narrow)
        rnd = lambda lo, hi, shape: torch.randint(lo, hi + 1, tuple(shape), generator=gen, dtype=torch.int64)
        xshape, yshape = (N, H, W, ci), (N, cv.Ho, cv.Wo, co)
        if positive:
            assert_wgrad_budget(cv.N * cv.Ho * cv.Wo, MAG_ONE_SIGN)
            xq, dyq = (torch.where(rnd(0, 7, sh) > 0, MAG_ONE_SIGN, 2 * rnd(0, 7, sh) + 1) for sh in (xshape, yshape))
        else:
            assert_wgrad_budget(cv.N * cv.Ho * cv.Wo)
            xq, dyq = rnd(-MAG_XQ, MAG_XQ, xshape), rnd(-MAG_XQ, MAG_XQ, yshape)
        ex, ey = _exponents(gen, ci // 32, narrow, False), _exponents(gen, co // 32, narrow, True)
        dw0 = _preload(gen, co, ci, ex, ey).reshape(-1)
        xb, dyb = encode(xq), encode(dyq)
        rw, _ = ref_wgrad(cv, dequant(xb, ex), dequant(dyb, ey), dw0)
        assert torch.equal(rw.float().double(), rw), "the reference of integer data is exact in fp32"
        units = rw.view(co, 9, ci) / _unit(co, ci, ex, ey)
        assert torch.equal(units, units.round()) and float(units.abs().max()) < F8_INT_LIMIT
        _f8_wdata[key] = (cv, xb, dyb, ex, ey, dw0, rw, units)
    return _f8_wdata[key]


def run_f8_wgrad_case(ops, case, positive=False, narrow=False, mutate=None):
    """dg_conv3x3_wgrad_f8 on integer operands: fp32 bits of dw against ref_wgrad of the dequantised operands.  ``mutate(ex, ey)``
    returns the exponents handed over instead of the ones the reference uses.  Returns dw as stored."""
    cv, xb, dyb, ex, ey, dw0, rw, _ = f8_wgrad_data(case, positive, narrow)
    ci, co = cv.Cin, cv.Cout
    x_dev, dy_dev = (_wide_slice(ops, xb), _wide_slice(ops, dyb, seed=23)) if case.sliced else (dev(ops, xb), dev(ops, dyb))
    ldx, ldy = pix_layout(x_dev)[0], pix_layout(dy_dev)[0]
    assert f8_wgrad_path(cv, ldx, ldy) == "f8", f"case guard: {case.id} is not a shape dg_conv3x3_wgrad_f8 takes"
    assert not case.sliced or (ldx > ci and ldy > co)
    exd, eyd = (ex, ey) if mutate is None else mutate(ex.clone(), ey.clone())
    what = f"{case.id}" + (" one-sign" if positive else "") + (" narrow exponents" if narrow else "")
    dw = Dest(ops, dw0)
    ops.conv_wgrad_f8(cv, x_dev, dev(ops, exd), dy_dev, dev(ops, eyd), dw.dev)
    if ops.name == "hip":
        code = ops.lib.dg_last_wgrad_kernel()
        assert code == WGRAD_CODE["f8"], f"{what}: dg_last_wgrad_kernel() = {code}, the fp8 kernel is {WGRAD_CODE['f8']}"
    assert_bits_at(dw.result().view(co, 9, ci), rw.float().view(co, 9, ci), f"{what}: dw")
    dw.check(what)
    return dw.result()


def run_f8_dense_case(ops, case):
    """dg_conv3x3_wgrad_dense_f8 for n convs of 128 channels on shared uniform-scale slabs whose pixel strides exceed n * 128."""
    N, H, W, n = case.shape
    F_ = 128
    gen = _gen(sum(map(ord, case.id)))
    assert_wgrad_budget(N * H * W)
    sq = torch.randint(-MAG_XQ, MAG_XQ + 1, (N, H, W, n * F_), generator=gen, dtype=torch.int64)
    uq = torch.randint(-MAG_XQ, MAG_XQ + 1, (N, H, W, n * F_), generator=gen, dtype=torch.int64)
    ex, eu = _exponents(gen, n * 4, False, False), _exponents(gen, n * 4, False, True)
    cvs = [Conv(N, H, W, (k + 1) * F_, F_, net="G") for k in range(n)]
    dws0 = [_preload(gen, F_, (k + 1) * F_, ex[:(k + 1) * 4], eu[k * 4:(k + 1) * 4]).reshape(-1) for k in range(n)]
    sb, ub = encode(sq), encode(uq)
    s_dev, u_dev = _wide_slice(ops, sb), _wide_slice(ops, ub, pad=64, lo=32, seed=29)
    assert pix_layout(s_dev)[0] > n * F_ and pix_layout(u_dev)[0] > n * F_
    dws = [Dest(ops, t) for t in dws0]
    ops.conv_wgrad_dense_f8(cvs, s_dev, dev(ops, ex), u_dev, dev(ops, eu), [t.dev for t in dws])
    if ops.name == "hip":
        assert ops.lib.dg_last_wgrad_kernel() == WGRAD_CODE["f8"], (case.id, ops.lib.dg_last_wgrad_kernel())
    xv, uv = dequant(sb, ex), dequant(ub, eu)
    for k, c in enumerate(cvs):
        rw, _ = ref_wgrad(c, xv[..., :(k + 1) * F_], uv[..., k * F_:(k + 1) * F_], dws0[k])
        assert torch.equal(rw.float().double(), rw)
        assert_bits_at(dws[k].result().view(F_, 9, c.Cin), rw.float().view(F_, 9, c.Cin), f"{case.id} dw[{k}]")
        dws[k].check(case.id)


# ---------------------------------------------------------------------------------------------------------------- the table
def _fwd(cid, shape, expect, **kw):
    return F8Case(cid, "fwd", shape, expect, **kw)


def _dg(cid, shape, expect, **kw):
    return F8Case(cid, "dgrad", shape, expect, **kw)


WIDEST = dict(eps=("plain", "mask_bits"), regimes=("wide",))
FIRST = "f8-halo-128-128-8x8"               # the case that measures the scaled-MFMA assumption; run before anything else
FIRST_WGRAD = "f8-wgrad-128-128-4x64"
FIRST_WGRAD_ONE_SIGN = "f8-wgrad-128-128-16x64"     # the smallest at which one-sign sums pass 2^23 inside the product window

CASES = [
    # stride 1, four waves: one partly filled tile; ragged tiles, two images, two K-blocks, partial channel tile, slab source and
    # destination; 80 outputs (the row clamp of the weight and scale DMA); pixel-shuffled destination; uniform-scale source, far scales
    _fwd(FIRST, (1, 8, 8, 128, 128, 1), "f8_halo"),
    _fwd("f8-halo-256-192-24x40-slab", (2, 24, 40, 256, 192, 1), "f8_halo", slab=True),
    _fwd("f8-halo-128-80-16x24", (1, 16, 24, 128, 80, 1), "f8_halo"),
    _fwd("f8-halo-128-512ps-16x24", (1, 16, 24, 128, 512, 1), "f8_halo", ps=True),
    _fwd("f8-halo-uniform-128-128-24x24", (1, 24, 24, 128, 128, 1), "f8_halo", uniform=True, D=D_FAR),
    _dg("f8-halo-dgrad-128-256-24x40", (2, 24, 40, 128, 256, 1), "f8_halo"),
    # stride-2 forward over the parity planes: four waves, partial tile + slab, eight waves
    _fwd("f8-s2-128-128-48x80", (1, 48, 80, 128, 128, 2), "f8_s2_4w"),
    _fwd("f8-s2-128-192-48x80-slab", (1, 48, 80, 128, 192, 2), "f8_s2_4w", slab=True),
    _fwd("f8-s2-128-256-48x80", (1, 48, 80, 128, 256, 2), "f8_s2_8w"),
    # merged stride-2 data gradient: interleaved class order, per-image order (Cred * Nout * 18 B above 2 MiB), a partial channel tile
    _dg("f8-seg-dgrad-256-128-32x48", (2, 32, 48, 256, 128, 2), "f8_seg_interleaved"),
    _dg("f8-seg-dgrad-256-512-16x16", (2, 16, 16, 256, 512, 2), "f8_seg_per_image"),
    _dg("f8-seg-dgrad-80-128-32x32", (1, 32, 32, 80, 128, 2), "f8_seg_interleaved"),
    # four launches per parity class: seg_dgrad_desc refuses the bf16 adjoint's row step
    _dg("f8-classes-dgrad-128-128-32x32-rowstep", (1, 32, 32, 128, 128, 2), "f8_per_class", big_ldy=True),
    # the widest layers
    _fwd("f8-halo-512-1024-16x16", (1, 16, 16, 512, 1024, 1), "f8_halo", **WIDEST),
    _fwd("f8-s2-1024-1024-16x16", (1, 16, 16, 1024, 1024, 2), "f8_s2_8w", **WIDEST),
    _dg("f8-seg-dgrad-1024-1024-16x16", (1, 16, 16, 1024, 1024, 2), "f8_seg_per_image", **WIDEST),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
PARAMS = [(c.id, r) for c in CASES for r in c.regimes]
SELFQ = ("f8-halo-128-80-16x24", "f8-s2-128-128-48x80", "f8-seg-dgrad-256-128-32x48")       # one s1, one s2 forward, one SEG dgrad

WCASES = [
    F8WCase(FIRST_WGRAD, "wgrad", (1, 4, 64, 128, 128, 1)),
    F8WCase(FIRST_WGRAD_ONE_SIGN, "wgrad", (1, 16, 64, 128, 128, 1)),
    F8WCase("f8-wgrad-256-384-5x64-sliced", "wgrad", (2, 5, 64, 256, 384, 1), sliced=True),
    F8WCase("f8-wgrad-s2-128-256-wo64", "wgrad", (2, 8, 128, 128, 256, 2)),
    F8WCase("f8-wgrad-s2-256-128-wo128", "wgrad", (1, 6, 256, 256, 128, 2)),
    # 96 tiles per pixel range (> 72): the grouped launch order, 2 splits x 2 units of 48 tiles in 8 unit slots, half of the workgroups padding
    F8WCase("f8-wgrad-512-1024-8x64", "wgrad", (1, 8, 64, 512, 1024, 1)),
    F8WCase("f8-wgrad-dense-1", "dense", (1, 4, 64, 1)),
    F8WCase("f8-wgrad-dense-3", "dense", (2, 3, 64, 3)),
    F8WCase("f8-wgrad-dense-5", "dense", (1, 4, 128, 5)),
]
WBY_ID = {c.id: c for c in WCASES}
SPLIT_K = "f8-wgrad-256-384-5x64-sliced"


def run_f8_wcase(ops, case):
    return run_f8_wgrad_case(ops, case) if case.kind == "wgrad" else run_f8_dense_case(ops, case)
