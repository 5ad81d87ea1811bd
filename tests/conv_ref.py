"""Float64 references, integer data and the shared case table of the EXACT tests of the MFMA kernels: the forward / data-gradient
gather-GEMMs (csrc/conv_rows.hip, conv_halo.hip, conv_small.hip, conv_s2dgrad.hip), the weight gradients (csrc/wgrad.hip) and the
head's Linear kernels (csrc/linear.hip).  tests/test_conv_exact_gpu.py runs the table through HipOps, tests/test_conv_exact_cpu.py
through EmuOps; both require equality of the bit patterns with the references below.

Why bits.  With integer operands, integer addends and power-of-two scalars (0.25, 0.5) every product, every partial sum IN ANY
ORDER and every epilogue step of a launch is a multiple of 2^-f below 2^(24-f) in magnitude, which fp32 holds exactly
(``int_operands`` asserts that budget per launch; f = the fractional bits the epilogue's scalars can introduce).  The one rounding
left is the final round-to-nearest-even of a bf16 store, which is deterministic.  The output must then EQUAL the float64
reference: a dropped, duplicated or misrouted term, a padding column applied late, a wrong epilogue order or an intermediate
narrowed to bf16 gives another integer.  fp32 operands use as many mantissa bits as the budget leaves (|x| in the thousands at 128
channels), so an fp32 operand narrowed to bf16 on its way to the MFMA shows as well; bf16 operands use [-127, 127].

The assumption behind it -- an MFMA chain whose operands and partial sums are integers below 2^24 returns that integer -- is checked
first on the device by the smallest halo case ("halo-128-128-8x8", plain epilogue, both dtypes).  It holds on the MI355X in fp32
and in bf16 (fp32 operands up to 4853 in magnitude, sums up to 2^24), so the budget ``INT_LIMIT`` stays at 2^24.

One finding of these tests is written into the contract instead of the table: the kernels compare the PACKED output channel with
``mask_c0``, which behind a pixel shuffle is not the destination's channel; the library now refuses that combination
(dg_epilogue), the oracle asserts the same, and pixel-shuffled cases run the mask_last epilogue with mask_c0 = 0.

References.  ``ref_fwd`` / ``ref_dgrad`` / ``ref_wgrad`` / ``ref_linear_*`` restate the contracts of include/downgan_hip.h with
torch float64 convolutions and matmuls, independent of ``EmuOps._gather_gemm``: conv2d on the master weight [Cout][9][Cin], the
pixel-shuffle placement (packed channel q*cps + c, q = 2i + j -> y[n, 2h+i, 2w+j, c]; the bias is indexed by the PACKED channel),
then the epilogue in the documented order (bias, act, r1/s1, r2/s2, mask, accumulate; mask_last moves the mask behind the
accumulate, mask_c0 limits its channels); mask bits in the documented little-endian packing.

Case table.  ``CASES`` lists every case once; a case names the dispatch path it exists for (``expect=``, a name of ``PATH_BITS`` for
the gather-GEMMs, of ``WGRAD_CODE`` for the weight gradients, a shape rule for the Linear kernels).  The runner asserts that name
against a restatement of the dispatch rules evaluated on the planner's own descriptors (CPU and GPU) and, on the GPU, against the
library's probes (dg_last_conv_kernels, dg_conv3x3_dgrad_launches, dg_conv3x3_dgrad_stream_eligible, dg_last_wgrad_kernel) -- an
edit of a shape or of the dispatch cannot quietly turn a case into a second test of another kernel.  Destinations sit inside
buffers with ``GUARD`` sentinel elements in front and behind; "slab" cases read and write channel slices of wider tensors.

The MXFP8 kernels (csrc/conv_halo_f8.hip, the fp8 kernel of csrc/wgrad.hip; the "f8" entries of ``PATH_BITS`` / ``WGRAD_CODE``) have
their own operands and table in tests/conv_f8_ref.py, which reuses the references, epilogues, destinations and comparator of this file.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import torch
import torch.nn.functional as F

from downgan_amd import _lib
from downgan_amd.ops import Conv, pix_layout
from tests.elementwise_ref import INT_LIMIT, TD, assert_bits

GUARD = 8192            # sentinel elements in front of and behind every destination
SENTINEL = -77.0        # exactly representable in bf16
SLAB_PAD, SLAB_LO = 48, 16   # slab cases: the destination is channels [16, 16 + C) of a tensor C + 48 channels wide
MAG_W = 3               # weights are integers in [-3, 3]
MAG_ADD = 64            # bias, residuals and preloaded destinations are integers in [-64, 64]
MAG_BF16 = 127          # integers a bf16 operand may hold here (8 significant bits, sign apart)
MAG_F32 = 1 << 20       # ceiling of an fp32 operand's magnitude where the budget would allow more


# ---------------------------------------------------------------------------------------------------------------- data
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def int_operands(K, mag_w, dtype, bias=0, residuals=0, preload=0, f=0):
    """Largest operand magnitude ``mag_x`` for a launch that adds ``K`` products |x * w| <= mag_x * mag_w and then addends of the
    given magnitudes (``residuals``: their sum), with ``f`` fractional bits from the epilogue's power-of-two scalars (scalars <= 1
    only shrink a value): mag_x * mag_w * K + addends < 2^(24 - f).  bf16 operands stay within [-127, 127]."""
    addends = bias + residuals + preload
    limit = INT_LIMIT >> f
    mag_x = (limit - 1 - addends) // (mag_w * K)
    mag_x = min(mag_x, MAG_BF16 if dtype == "bf16" else MAG_F32)
    assert mag_x >= 1 and mag_x * mag_w * K + addends < limit, f"no integer budget: K={K} mag_w={mag_w} addends={addends} f={f}"
    if dtype == "bf16":
        assert mag_x <= MAG_BF16 and mag_w <= MAG_BF16 and max(bias, preload) <= MAG_BF16
    return int(mag_x)


def ints(shape, mag, gen, dtype):
    """Integers in [-mag, mag] in ``dtype`` ("f32" / "bf16" or a torch dtype), exactly."""
    td = TD[dtype] if isinstance(dtype, str) else dtype
    assert td != torch.bfloat16 or mag <= MAG_BF16
    v = torch.randint(-mag, mag + 1, tuple(shape), generator=gen, dtype=torch.int64)
    t = v.to(td)
    assert torch.equal(t.double(), v.double())
    return t


def pack_bits(pos):
    """bool [..., C] -> int16 [..., C/64, 4]: bit b of word (block, g) = channel 64*block + 16*g + b (dg_epilogue)."""
    Cc = pos.shape[-1]
    assert Cc % 64 == 0
    w = (pos.reshape(*pos.shape[:-1], Cc // 16, 16).to(torch.int64) << torch.arange(16)).sum(-1)
    w = torch.where(w >= 32768, w - 65536, w).to(torch.int16)
    return w.reshape(*pos.shape[:-1], Cc // 64, 4).contiguous()


# ---------------------------------------------------------------------------------------------------------------- comparator
def assert_bits_at(out, ref, what):
    """``assert_bits`` with the first differing index unravelled over the tensor's shape: (n, h, w, c) for an activation,
    (co, tap, ci) for a weight gradient."""
    try:
        assert_bits(out, ref, what)
    except AssertionError as e:
        o, r = out.detach().cpu(), ref.detach().cpu()
        if o.shape != r.shape or o.dtype != r.dtype:
            raise
        ne = (o.double() != r.double()) | (torch.signbit(o.float()) != torch.signbit(r.float()))
        idx = ne.flatten().nonzero().flatten()
        if idx.numel() == 0:
            raise
        i = int(idx[0])
        at = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), o.shape))
        raise AssertionError(f"{what}: {idx.numel()} of {o.numel()} elements differ, first at {at}: "
                             f"got {float(o.flatten()[i])!r}, reference {float(r.flatten()[i])!r}") from e


# ---------------------------------------------------------------------------------------------------------------- references
def _widen(cv, x):
    if cv.cin_real and x.shape[-1] == 2 and cv.Cin > 2:
        return F.pad(x, (0, cv.Cin - 2))
    return x


def _w_oihw(cv, master_w):
    return master_w.double().view(cv.Cout, 3, 3, cv.Cin).permute(0, 3, 1, 2)


def _shuffle(v):          # [N, Ho, Wo, 4*cps] packed (2i+j)*cps + c  ->  [N, 2Ho, 2Wo, cps]
    N, H, W, Cc = v.shape
    return v.view(N, H, W, 2, 2, Cc // 4).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, Cc // 4)


def _unshuffle(v):
    N, H2, W2, cps = v.shape
    return v.view(N, H2 // 2, 2, W2 // 2, 2, cps).permute(0, 1, 3, 2, 4, 5).reshape(N, H2 // 2, W2 // 2, 4 * cps)


def conv_acc(cv, x, master_w):
    """The float64 convolution [N, Ho, Wo, Cout] (packed channels, before any placement)."""
    xx = _widen(cv, x).double().permute(0, 3, 1, 2)
    return F.conv2d(xx, _w_oihw(cv, master_w), stride=cv.stride, padding=1).permute(0, 2, 3, 1).contiguous()


def dgrad_acc(cv, dy, master_w):
    """The float64 transpose [N, H, W, Cin] of ``conv_acc`` applied to dy (un-shuffled first when the layer shuffles)."""
    u = _unshuffle(dy.double()) if cv.pixel_shuffle else dy.double()
    return F.conv_transpose2d(u.permute(0, 3, 1, 2), _w_oihw(cv, master_w), stride=cv.stride, padding=1,
                              output_padding=cv.stride - 1).permute(0, 2, 3, 1).contiguous()


def _lgrad(m, slope):
    return torch.where(m.double() > 0, torch.ones((), dtype=torch.float64), torch.full((), float(slope), dtype=torch.float64))


def epilogue(v, pre, dtype, act=None, r1=None, s1=1.0, r2=None, s2=1.0, mask=None, mask_slope=1.0, accumulate=False,
             mask_sign=None, mask_c0=0, mask_last=False, want_bits=False):
    """dg_epilogue after the bias, on float64 ``v`` of the destination's shape.  ``mask_sign``: the bool tensor a ``mask_bits``
    argument encodes.  Returns (float64 value, value as stored, expected out_bits or None)."""
    if act is not None:
        v = torch.where(v > 0, v, v * act)
    if r1 is not None:
        v = v * s1 + r1.double()
    if r2 is not None:
        v = v * s2 + r2.double()

    def masked(v):
        f = _lgrad(mask, mask_slope)
        return v * torch.where(torch.arange(v.shape[-1]) >= mask_c0, f, torch.ones((), dtype=torch.float64))
    if mask is not None and not mask_last:
        v = masked(v)
    if mask_sign is not None:
        v = v * torch.where(mask_sign, torch.ones((), dtype=torch.float64), torch.full((), float(mask_slope), dtype=torch.float64))
    if accumulate:
        v = v + pre.double()
    if mask is not None and mask_last:
        v = masked(v)
    stored = v.to(TD[dtype])
    assert torch.equal(stored.double(), v) or dtype == "bf16", "an fp32 destination must hold the reference exactly"
    return v, stored, (pack_bits(stored.float() > 0) if want_bits else None)


def ref_fwd(cv, x, master_w, y_preload, dtype, bias=None, acc=None, **ep):
    v = conv_acc(cv, x, master_w) if acc is None else acc
    if bias is not None:
        v = v + bias.double()[:cv.Cout]
    if cv.pixel_shuffle:
        v = _shuffle(v)
    return epilogue(v, y_preload, dtype, **ep)


def ref_dgrad(cv, dy, master_w, dx_preload, dtype, bias=None, acc=None, **ep):
    v = dgrad_acc(cv, dy, master_w) if acc is None else acc
    if bias is not None:
        v = v + bias.double()[:cv.Cin]
    return epilogue(v, dx_preload, dtype, **ep)


def ref_wgrad(cv, x, dy, dw_preload, db_preload=None):
    """(dw [Cout*9*Cin], db [Cout] or None) in float64: autograd of the float64 forward, added to the preloads."""
    xx = _widen(cv, x).double().permute(0, 3, 1, 2)
    u = (_unshuffle(dy.double()) if cv.pixel_shuffle else dy.double())
    w = torch.zeros(cv.Cout, cv.Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xx, w, stride=cv.stride, padding=1)
    (g,) = torch.autograd.grad(y, w, grad_outputs=u.permute(0, 3, 1, 2))
    dw = dw_preload.double() + g.permute(0, 2, 3, 1).reshape(-1)
    db = None if db_preload is None else db_preload.double() + torch.cat([u.reshape(-1, cv.Cout).sum(0), torch.zeros(db_preload.numel() - cv.Cout, dtype=torch.float64)])
    return dw, db


def ref_linear_fwd(x, w, y_preload):
    y = y_preload.double().clone()
    y[:, :w.shape[0]] += x.double() @ w.double().t()
    return y


def ref_linear_dx(dy, w, mask=None, mask_slope=1.0):
    v = dy.double()[:, :w.shape[0]] @ w.double()
    return v if mask is None else v * _lgrad(mask, mask_slope)


def ref_linear_dw(dy, x, dw_preload):
    return dw_preload.double() + dy.double()[:, :dw_preload.shape[0]].t() @ x.double()


def ref_linear_dw_wide(dy, x, dw_preload, accumulate):
    r = dy.double()[:, :dw_preload.shape[0]].t() @ x.double()
    return dw_preload.double() + r if accumulate else r


# ---------------------------------------------------------------------------------------------------------------- destinations
class Dest:
    """``values`` (the preloaded content) on ``ops.device`` between two guards of ``GUARD`` sentinel elements; with ``slab`` the values
    are channels [SLAB_LO, SLAB_LO + C) of a tensor C + SLAB_PAD channels wide (integers elsewhere) and ``dev`` is that view."""

    def __init__(self, ops, values, slab=False):
        self.cpu = values.contiguous()
        if slab:
            Cc = values.shape[-1]
            self.host = ints(tuple(values.shape[:-1]) + (Cc + SLAB_PAD,), 50, _gen(Cc + 7), values.dtype)
            self.sl = slice(SLAB_LO, SLAB_LO + Cc)
            self.host[..., self.sl] = self.cpu
        else:
            self.host, self.sl = self.cpu, None
        n = self.host.numel()
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=values.dtype, device=ops.device)
        self.full = self.buf[GUARD:GUARD + n].view(self.host.shape)
        self.full.copy_(self.host)
        self.dev = self.full if self.sl is None else self.full[..., self.sl]
        self.n = n

    def result(self):
        return self.dev.detach().to("cpu", copy=True).contiguous()

    def check(self, what):
        """The guards in front and behind keep their bits, and so does every channel of the slab outside the written slice."""
        sent = torch.full((GUARD,), SENTINEL, dtype=self.buf.dtype)
        assert_bits(self.buf[:GUARD].cpu(), sent, f"{what}: the guard in front of the destination")
        assert_bits(self.buf[GUARD + self.n:].cpu(), sent, f"{what}: the guard behind the destination")
        if self.sl is not None:
            after = self.full.detach().cpu().clone()
            after[..., self.sl] = self.host[..., self.sl]
            assert_bits_at(after, self.host, f"{what}: the slab's other channels")


def dev(ops, t):
    return None if t is None else t.to(ops.device)


# ---------------------------------------------------------------------------------------------------------------- dispatch paths
# name -> the dg_last_conv_kernels() mask a launch on that path leaves (include/downgan_hip.h)
PATH_BITS = {"rows_generic": 1, "rows_fast": 2, "halo": 8, "halo_ps_src": 8, "halo_s2_4w": 8, "halo_s2_8w": 8, "halo16": 8,
             "seg_interleaved": 8, "seg_per_image": 8, "stream": 64, "im2col_linear": 16, "im2col_tiled": 16,
             "per_class_generic": 1, "per_class_halo16_fast": 8 | 2, "f8": 32}      # "f8": the MXFP8 halo kernel, tests/conv_f8_ref.py
WGRAD_CODE = {"tap": 1, "im2col": 2, "rows": 3, "wide_s1": 4, "wide_s2": 5, "dense": 6, "f8": 7}


def plan(cv, dtype, kind, ldx, ldy):
    g = _lib.ConvGeom(dtype=_lib.DG_F32 if dtype == "f32" else _lib.DG_BF16, N=cv.N, H=cv.H, W=cv.W, Cin=cv.Cin, Cout=cv.Cout,
                      stride=cv.stride, cin_real=cv.cin_real, pixel_shuffle=int(cv.pixel_shuffle), ldx=ldx, ldy=ldy)
    d = (_lib.GGDesc * 4)()
    n = _lib.lib().dg_conv3x3_plan(C.byref(g), kind, d)
    assert n > 0, n
    return g, [d[i] for i in range(n)]


def _desc_path(d, dtype, bits):
    """gg_launch (csrc/conv_plan.hip) restated for one planned descriptor."""
    epc, es = (4, 4) if dtype == "f32" else (8, 2)
    cch = d.Cred // epc
    step_ok = lambda mult: mult * d.Ws * d.lds * es < (1 << 23)
    unit, same, big = d.sy_mul == 1 and d.sx_mul == 1, d.Hs == d.Hg and d.Ws == d.Wg, d.Hg >= 8 and d.Wg >= 8
    cps_chunks = d.Cred // 4 // epc if d.src_ps else 1
    if unit and not d.src_ps and cch % 8 == 0 and d.Nout > 64 and big and same and step_ok(1):
        return "halo"
    if unit and d.src_ps and cps_chunks % 8 == 0 and cch % 8 == 0 and d.Nout > 64 and big and d.ntaps >= 2 and same and step_ok(4):
        return "halo_ps_src"
    if (d.sy_mul == 2 and d.sx_mul == 2 and not d.src_ps and cch % 16 == 0 and d.Nout > 64 and big and d.Hs == 2 * d.Hg
            and d.Ws == 2 * d.Wg and d.dy_mul == 1 and d.dx_mul == 1 and step_ok(2)):
        return "halo_s2_8w" if dtype == "bf16" and d.Nout % 256 == 0 else "halo_s2_4w"
    if d.Nout <= 16 and unit and not d.src_ps and not d.dst_ps and cch % 8 == 0 and big and d.ntaps >= 2 and same and not bits:
        return "halo16"
    return "rows_fast" if cch % 8 == 0 and (not d.src_ps or cps_chunks % 8 == 0) else "rows_generic"


def conv_path(cv, dtype, kind, ldx, ldy, ep, stream_mode=1):
    """The path dg_conv3x3_fwd (kind 0) / dg_conv3x3_dgrad (kind 1) takes, from the planner's descriptors and the rules of
    csrc/conv_plan.hip, csrc/conv_small.hip and csrc/conv_s2dgrad.hip."""
    _, ds = plan(cv, dtype, kind, ldx, ldy)
    bits = "mask_bits" in ep or "out_bits" in ep
    if kind == 0:
        if 0 < cv.cin_real <= 2 and cv.stride == 1 and not cv.pixel_shuffle:
            return "im2col_tiled" if cv.H % 16 == 0 else "im2col_linear"
        return _desc_path(ds[0], dtype, bits)
    if (stream_mode and dtype == "bf16" and cv.stride == 2 and not cv.pixel_shuffle and cv.Cin == 128 and cv.Cout == 128 and ldx == 128
            and ldy == 128 and not (set(ep) - {"mask_bits", "mask_slope"})):
        return "stream"
    if len(ds) == 1:
        return _desc_path(ds[0], dtype, bits)
    epc = 4 if dtype == "f32" else 8
    d0 = ds[0]
    if not ((d0.Cred // epc) % 8 or d0.Nout <= 64 or d0.Hg < 8 or d0.Wg < 8):          # seg_dgrad_desc
        return "seg_interleaved" if d0.Cred * d0.Nout * 18 <= (2 << 20) else "seg_per_image"
    paths = sorted({_desc_path(d, dtype, bits) for d in ds})
    return {("rows_generic",): "per_class_generic", ("halo16", "rows_fast"): "per_class_halo16_fast"}.get(tuple(paths), "+".join(paths))


def wgrad_path(cv, dtype):
    """dg_conv3x3_wgrad's choice (csrc/wgrad.hip) restated."""
    Wo, Mpix = cv.W // cv.stride, cv.N * (cv.H // cv.stride) * (cv.W // cv.stride)
    if 0 < cv.cin_real <= 2 and cv.stride == 1 and not cv.pixel_shuffle and Wo % 32 == 0:
        return "im2col"
    wide = dtype == "bf16" and cv.Cout >= 128 and cv.Cin >= 128
    rows = cv.stride == 1 and Wo % 32 == 0 and cv.Cout >= 64 and (cv.Cin >= 256 or (cv.Cin >= 64 and Mpix >= (1 << 22)) or wide)
    if rows and wide:
        return "wide_s1"
    if rows:
        return "rows"
    if wide and cv.stride == 2 and Wo % 32 == 0 and not cv.pixel_shuffle:
        return "wide_s2"
    return "tap"


def _expect(case, dtype):
    e = case.expect
    return e[dtype] if isinstance(e, dict) else e


# ---------------------------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    kind: str                      # "fwd", "dgrad", "wgrad", "dense", "linear"
    shape: tuple                   # conv: (N, H, W, Cin, Cout, stride, pixel_shuffle); dense: (N, H, W, n); linear: (B, K, O)
    expect: object                 # path name, or {dtype: path name}
    dtypes: tuple = ("f32", "bf16")
    eps: tuple = ()                # names of EPILOGUES ("" = all the path accepts)
    slab: bool = False
    cin_real: int = 0
    compact: bool = False          # cin_real layers: the source as [N, H, W, 2]
    stream: tuple = (1,)           # settings of dg_set_s2_dgrad_stream to run under
    db: tuple = (True,)            # wgrad: with / without a bias gradient

    def conv(self):
        N, H, W, ci, co, st, ps = self.shape
        return Conv(N, H, W, ci, co, st, bool(ps), cin_real=self.cin_real)


EPILOGUES = ("plain", "bias_act", "bias_r1_r2", "mask", "accumulate", "acc_mask_last", "mask_bits", "out_bits")
EP_F = {"plain": 0, "bias_act": 2, "bias_r1_r2": 2, "mask": 2, "accumulate": 0, "acc_mask_last": 2, "mask_bits": 2, "out_bits": 2}


def case_epilogues(case, dtype):
    """The epilogues of EPILOGUES the case's path accepts: the 1-bit masks need >= 128 output channels in whole 64-channel blocks and
    no pixel shuffle; out_bits a destination written in one piece (not the parity classes of a stride-2 data gradient)."""
    cv = case.conv()
    nout = cv.Cout if case.kind == "fwd" else cv.Cin
    names = case.eps or EPILOGUES
    ok = []
    for n in names:
        if n in ("mask_bits", "out_bits") and (nout < 128 or nout % 64 or (cv.pixel_shuffle and case.kind == "fwd")):
            assert not case.eps, (case.id, n)
            continue
        if n == "out_bits" and case.kind == "dgrad" and cv.stride == 2:
            assert not case.eps, (case.id, n)
            continue
        ok.append(n)
    return ok


def build_epilogue(name, oshape, nout, dtype, gen, ps=False, mag=MAG_ADD):
    """(keyword arguments with host tensors, mask_sign or None).  Scalars are 0.25 / 0.5 exactly.  ``ps``: a pixel-shuffled
    destination, for which the library refuses mask_c0 != 0 (dg_epilogue).  ``mag``: magnitude of the integer addends."""
    kw, sign = {}, None
    if name == "bias_act":
        kw = dict(bias=ints((nout,), mag, gen, torch.float32), act=0.25)
    elif name == "bias_r1_r2":
        kw = dict(bias=ints((nout,), mag, gen, torch.float32), r1=ints(oshape, mag, gen, dtype), s1=0.5,
                  r2=ints(oshape, mag, gen, dtype), s2=0.5)
    elif name == "mask":
        kw = dict(mask=ints(oshape, 2, gen, dtype), mask_slope=0.25)
    elif name == "accumulate":
        kw = dict(accumulate=True)
    elif name == "acc_mask_last":
        kw = dict(accumulate=True, mask=ints(oshape, 2, gen, dtype), mask_slope=0.25, mask_c0=0 if ps else (oshape[-1] // 2) // 16 * 16, mask_last=True)
    elif name == "mask_bits":
        sign = ints(oshape, 2, gen, torch.float32) > 0
        kw = dict(mask_bits=pack_bits(sign), mask_slope=0.25)
    elif name == "out_bits":
        kw = dict(bias=ints((nout,), mag, gen, torch.float32), act=0.25,
                  out_bits=torch.full(tuple(oshape[:-1]) + (oshape[-1] // 64, 4), 0x5a5a, dtype=torch.int16))
    else:
        assert name == "plain", name
    return kw, sign


_conv_data = {}


def conv_data(case, dtype, names=None, positive=False):
    """Integer operands and the float64 accumulator of a forward / data-gradient case for the epilogues ``names`` (default: all the
    case takes), built once; the operands' magnitude follows from the fractional bits those epilogues need.  ``positive``: operands in
    the upper half of their range and weights in [2, 3], all of one sign, so that the sums themselves come close to the budget (signed
    random data stays near its square root)."""
    names = tuple(names or case_epilogues(case, dtype))
    f = max(EP_F[n] for n in names)
    key = (case.id, dtype, f, positive)
    if key not in _conv_data:
        cv = case.conv()
        gen = _gen(sum(map(ord, case.id)) * 2 + (dtype == "bf16"))
        fwd = case.kind == "fwd"
        K = 9 * (cv.cin_real or cv.Cin) if fwd else 9 * cv.Cout
        mag = int_operands(K, MAG_W, dtype, bias=MAG_ADD, residuals=2 * MAG_ADD, preload=MAG_ADD, f=f)
        master = ints((cv.Cout, 9, cv.Cin), MAG_W, gen, torch.float32)
        if cv.cin_real:
            master[..., cv.cin_real:] = 0
        oshape = (cv.N, 2 * cv.Ho, 2 * cv.Wo, cv.Cout // 4) if cv.pixel_shuffle else (cv.N, cv.Ho, cv.Wo, cv.Cout)
        if fwd:
            src = ints((cv.N, cv.H, cv.W, cv.Cin), mag, gen, dtype)
            if cv.cin_real:
                src[..., cv.cin_real:] = 0
            if case.compact:
                src = src[..., :2].contiguous()
            acc, dshape = conv_acc(cv, src, master), oshape
        else:
            src = ints(oshape, mag, gen, dtype)
            acc, dshape = dgrad_acc(cv, src, master), (cv.N, cv.H, cv.W, cv.Cin)
        if positive:
            td = src.dtype
            src = torch.where(src != 0, (src.double().abs() / 2 + mag // 2 + 1).floor().clamp(max=mag), src.double()).to(td)
            master = torch.where(master != 0, 2 + master.abs() % 2, master)
            acc = conv_acc(cv, src, master) if fwd else dgrad_acc(cv, src, master)
            assert float(acc.abs().max()) + 4 * MAG_ADD < (INT_LIMIT >> f)
        pre = ints(dshape, MAG_ADD, gen, dtype)
        _conv_data[key] = (cv, master, src, acc, pre, dshape, gen.get_state())
    return _conv_data[key]


def run_conv_case(ops, case, dtype, only=None, mutate=None, positive=False):
    """Steps (a)-(g) of a forward / data-gradient case for every epilogue it takes (``only``: one of them).  ``mutate(src, master)``
    (CPU mutation check) returns the operands handed to the device instead of the ones the reference was computed from."""
    names = case_epilogues(case, dtype) if only is None else [only]
    cv, master, src, acc, pre, dshape, gstate = conv_data(case, dtype, names, positive)
    fwd = case.kind == "fwd"
    nout = cv.Cout if fwd else cv.Cin
    gen = torch.Generator()
    gen.set_state(gstate)
    src_d, master_d = (src, master) if mutate is None else mutate(src.clone(), master.clone())
    pack = torch.zeros(master.numel(), dtype=TD[dtype], device=ops.device)
    ops.repack(dev(ops, master_d.reshape(-1)), pack, cv.Cout, cv.Cin, 0 if fwd else 1)
    if case.slab:        # the source too is a channel slice of a wider tensor (a dense block's slab): pixel stride above the channel count
        wide = ints(tuple(src_d.shape[:-1]) + (src_d.shape[-1] + 24,), 50, _gen(11), src_d.dtype)
        wide[..., 8:8 + src_d.shape[-1]] = src_d
        src_dev = dev(ops, wide)[..., 8:8 + src_d.shape[-1]]
    else:
        src_dev = dev(ops, src_d)
    hip = ops.name == "hip"
    for name in names:
        kw, sign = build_epilogue(name, dshape, nout, dtype, gen, ps=fwd and cv.pixel_shuffle)
        for mode in case.stream:
            what = f"{case.id} {dtype} {name}" + (f" stream={mode}" if len(case.stream) > 1 else "")
            dst = Dest(ops, pre, slab=case.slab)
            ldsrc, lddst = pix_layout(src_dev)[0], pix_layout(dst.dev)[0]
            ldx, ldy = (ldsrc, lddst) if fwd else (lddst, ldsrc)
            path = conv_path(cv, dtype, 0 if fwd else 1, ldx, ldy, kw, mode)
            want = _expect(case, dtype)
            if case.stream != (1,):
                want = want if mode else "seg_interleaved"
            elif want == "stream" and name not in ("plain", "mask_bits"):
                want = "seg_interleaved"
            assert path == want, f"case guard: {what} would take {path}, the case is there for {want}"
            kwd = {k: (dev(ops, v) if torch.is_tensor(v) else v) for k, v in kw.items()}
            prev = ops.lib.dg_set_s2_dgrad_stream(mode) if hip else None
            try:
                (ops.conv_fwd if fwd else ops.conv_dgrad)(cv, src_dev, pack, dst.dev, **kwd)
                kinds = ops.lib.dg_last_conv_kernels() if hip else None
            finally:
                if hip:
                    ops.lib.dg_set_s2_dgrad_stream(prev)
            if hip:
                assert kinds == PATH_BITS[path], f"{what}: dg_last_conv_kernels() = {kinds}, path {path} leaves {PATH_BITS[path]}"
                if not fwd:
                    g, ds = plan(cv, dtype, 1, ldx, ldy)
                    merged = path.startswith("seg") or path == "stream" or len(ds) == 1
                    assert ops.lib.dg_conv3x3_dgrad_launches(C.byref(g)) == (1 if merged else 4), what
                    e = ops._epilogue(dst.dev, **kwd)
                    assert ops.lib.dg_conv3x3_dgrad_stream_eligible(C.byref(g), C.byref(e)) == int(conv_path(cv, dtype, 1, ldx, ldy, kw, 1) == "stream"), what
            refkw = {k: v for k, v in kw.items() if k not in ("mask_bits", "out_bits")}
            _, stored, bits = (ref_fwd if fwd else ref_dgrad)(cv, None, None, pre, dtype, acc=acc, mask_sign=sign, want_bits="out_bits" in kw, **refkw)
            assert_bits_at(dst.result(), stored, what)
            dst.check(what)
            if bits is not None:
                assert_bits_at(kwd["out_bits"].cpu(), bits, f"{what}: out_bits")


def run_wgrad_case(ops, case, dtype):
    cv = case.conv()
    gen = _gen(sum(map(ord, case.id)) * 2 + (dtype == "bf16"))
    want = _expect(case, dtype)
    assert wgrad_path(cv, dtype) == want, f"case guard: {case.id} {dtype} would take {wgrad_path(cv, dtype)}, the case is there for {want}"
    K = cv.N * cv.Ho * cv.Wo
    mag = int_operands(K, MAG_W, dtype, preload=MAG_ADD)
    x = ints((cv.N, cv.H, cv.W, cv.Cin), mag, gen, dtype)
    if cv.cin_real:
        x[..., cv.cin_real:] = 0
    oshape = (cv.N, 2 * cv.Ho, 2 * cv.Wo, cv.Cout // 4) if cv.pixel_shuffle else (cv.N, cv.Ho, cv.Wo, cv.Cout)
    dy = ints(oshape, MAG_W, gen, dtype)
    dw0, db0 = ints((cv.Cout * 9 * cv.Cin,), MAG_ADD, gen, torch.float32), ints((cv.Cout,), MAG_ADD, gen, torch.float32)
    xs = x[..., :2].contiguous() if case.compact else x
    results = []
    for with_db in case.db:
        what = f"{case.id} {dtype} db={with_db}"
        dw, db = Dest(ops, dw0), Dest(ops, db0)
        ops.conv_wgrad(cv, dev(ops, xs), dev(ops, dy), dw.dev, db=db.dev if with_db else None)
        if ops.name == "hip":
            code = ops.lib.dg_last_wgrad_kernel()
            assert code == WGRAD_CODE[want], f"{what}: dg_last_wgrad_kernel() = {code}, {want} is {WGRAD_CODE[want]}"
        rw, rb = ref_wgrad(cv, x, dy, dw0, db0 if with_db else None)
        assert_bits_at(dw.result().view(cv.Cout, 9, cv.Cin), rw.float().view(cv.Cout, 9, cv.Cin), f"{what}: dw")
        assert torch.equal(rw.float().double(), rw)
        assert_bits_at(db.result(), rb.float() if with_db else db0, f"{what}: db")
        dw.check(what); db.check(what)
        results += [dw.result(), db.result()]
    return results


def run_dense_case(ops, case, dtype):
    """dg_conv3x3_wgrad_dense for n convs of 128 channels on shared slabs; the first conv also through conv_wgrad: equal bits."""
    N, H, W, n = case.shape
    F_ = 128
    gen = _gen(sum(map(ord, case.id)))
    mag = int_operands(N * H * W, MAG_W, dtype, preload=MAG_ADD)
    slab, us = ints((N, H, W, n * F_), mag, gen, dtype), ints((N, H, W, n * F_), MAG_W, gen, dtype)
    cvs = [Conv(N, H, W, (k + 1) * F_, F_) for k in range(n)]
    dws0 = [ints((F_ * 9 * (k + 1) * F_,), MAG_ADD, gen, torch.float32) for k in range(n)]
    dbs0 = [ints((F_,), MAG_ADD, gen, torch.float32) for _ in range(n)]
    dws, dbs = [Dest(ops, t) for t in dws0], [Dest(ops, t) for t in dbs0]
    slab_d, us_d = dev(ops, slab), dev(ops, us)
    ops.conv_wgrad_dense(cvs, slab_d, us_d, [t.dev for t in dws], [t.dev for t in dbs])
    if ops.name == "hip":
        assert ops.lib.dg_last_wgrad_kernel() == WGRAD_CODE[_expect(case, dtype)], (case.id, ops.lib.dg_last_wgrad_kernel())
    for k, c in enumerate(cvs):
        rw, rb = ref_wgrad(c, slab[..., :(k + 1) * F_], us[..., k * F_:(k + 1) * F_], dws0[k], dbs0[k])
        assert_bits_at(dws[k].result().view(F_, 9, c.Cin), rw.float().view(F_, 9, c.Cin), f"{case.id} dw[{k}]")
        assert_bits_at(dbs[k].result(), rb.float(), f"{case.id} db[{k}]")
        dws[k].check(case.id); dbs[k].check(case.id)
    dw1, db1 = Dest(ops, dws0[0]), Dest(ops, dbs0[0])
    ops.conv_wgrad(cvs[0], slab_d[..., :F_], us_d[..., :F_], dw1.dev, db=db1.dev)
    assert_bits(dw1.result(), dws[0].result(), f"{case.id}: conv 1 through conv_wgrad"); assert_bits(db1.result(), dbs[0].result(), f"{case.id}: db 1")


def run_linear_case(ops, case, dtype):
    """Forward, dx (bf16 and fp32 destinations, with and without the mask), dw and dw_wide (accumulate and write) of one (B, K, O);
    ``expect`` = the input-gradient kernel the shape is there for (dg_linear_dx: the wide kernel takes K >= 4096 with B >= 16)."""
    B, K, O = case.shape
    assert _expect(case, dtype) == ("dx_wide" if K >= 4096 and B >= 16 else "dx_narrow"), f"case guard: {case.id}"
    gen = _gen(sum(map(ord, case.id)) * 2 + (dtype == "bf16"))
    x = ints((B, K), int_operands(K, MAG_W, dtype, preload=MAG_ADD), gen, dtype)
    w = ints((O, K), MAG_W, gen, dtype)
    if O % 16 == 0 and K % 32 == 0:      # dg_linear_fwd takes whole 16-row weight groups and whole K-steps; the other shapes are backward-only
        y0 = torch.zeros(B, 128)
        y = Dest(ops, y0)
        ops.linear_fwd(dev(ops, x), dev(ops, w), y.dev)
        assert_bits_at(y.result(), ref_linear_fwd(x, w, y0).float(), f"{case.id} {dtype} fwd"); y.check(case.id)
    # dy: fp32 rows 128 wide of which O are real (integers in the padding too: the kernels must not read them into the product)
    dy = ints((B, 128), int_operands(O, MAG_W, "f32", f=2), gen, torch.float32)
    mask = ints((B, K), 2, gen, dtype)
    for out_dt in ((torch.float32,) if dtype == "f32" else (torch.float32, torch.bfloat16)):
        for m in (None, mask):
            dx = Dest(ops, torch.full((B, K), 3.0, dtype=out_dt))
            ops.linear_dx(dev(ops, dy), dev(ops, w), dx.dev, mask=dev(ops, m), mask_slope=0.25)
            what = f"{case.id} {dtype} dx {out_dt} mask={m is not None}"
            assert_bits_at(dx.result(), ref_linear_dx(dy, w, m, 0.25).to(out_dt), what); dx.check(what)
    dyw = ints((B, 128), int_operands(B, MAG_BF16 if dtype == "bf16" else 2047, "f32", preload=MAG_ADD), gen, torch.float32)
    xw = ints((B, K), MAG_BF16 if dtype == "bf16" else 2047, gen, dtype)
    dw0 = ints((O, K), MAG_ADD, gen, torch.float32)
    if B <= 64:
        dw = Dest(ops, dw0)
        ops.linear_dw(dev(ops, dyw), dev(ops, xw), dw.dev)
        assert_bits_at(dw.result(), ref_linear_dw(dyw, xw, dw0).float(), f"{case.id} {dtype} dw"); dw.check(case.id)
    if B <= 128 and O <= 112:
        for acc in (True, False):
            dw = Dest(ops, dw0 if acc else torch.full((O, K), float("nan")))      # write mode must not read the destination
            ops.linear_dw_wide(dev(ops, dyw)[:, :O], dev(ops, xw), dw.dev, accumulate=acc)
            assert_bits_at(dw.result(), ref_linear_dw_wide(dyw, xw, dw0, acc).float(), f"{case.id} {dtype} dw_wide acc={acc}"); dw.check(case.id)


RUNNERS = {"fwd": run_conv_case, "dgrad": run_conv_case, "wgrad": run_wgrad_case, "dense": run_dense_case, "linear": run_linear_case}


def run_case(ops, case, dtype):
    return RUNNERS[case.kind](ops, case, dtype)


# ---------------------------------------------------------------------------------------------------------------- the table
def _fwd(cid, shape, expect, **kw):
    return Case(cid, "fwd", shape, expect, **kw)


def _dg(cid, shape, expect, **kw):
    return Case(cid, "dgrad", shape, expect, **kw)


def _wg(cid, shape, expect, **kw):
    return Case(cid, "wgrad", shape, expect, **kw)


S2_8W = {"f32": "halo_s2_4w", "bf16": "halo_s2_8w"}
WIDE = ("plain", "mask_bits")
FIRST = "halo-128-128-8x8"       # the case that checks the integer-MFMA assumption; run before anything else

CASES = [
    # halo kernel, stride 1: one tile; ragged in both directions, two images; a partial channel tile; pixel-shuffle store; 2 reduction blocks
    _fwd(FIRST, (1, 8, 8, 128, 128, 1, 0), "halo"),
    _fwd("halo-128-128-24x40-slab", (2, 24, 40, 128, 128, 1, 0), "halo", slab=True),
    _fwd("halo-128-192-24x40", (1, 24, 40, 128, 192, 1, 0), "halo"),
    _fwd("halo-128-512ps-16x24", (1, 16, 24, 128, 512, 1, 1), "halo"),
    _fwd("halo-256-128-16x24", (1, 16, 24, 256, 128, 1, 0), "halo"),
    _dg("halo-dgrad-128-128-24x40", (2, 24, 40, 128, 128, 1, 0), "halo"),
    # ... a pixel-shuffled source: the data gradient of an up-sampling conv
    _dg("halo-ps-src-dgrad-128-256ps-16x24", (1, 16, 24, 128, 256, 1, 1), "halo_ps_src"),
    # stride-2 forward over the parity planes: 4 waves, 8 waves (bf16 with Cout % 256 == 0)
    _fwd("halo-s2-128-128-48x80", (1, 48, 80, 128, 128, 2, 0), "halo_s2_4w"),
    _fwd("halo-s2-128-192-48x80-slab", (1, 48, 80, 128, 192, 2, 0), "halo_s2_4w", slab=True),
    _fwd("halo-s2-128-256-48x80", (1, 48, 80, 128, 256, 2, 0), S2_8W),
    # small-N halo kernel: forward with <= 16 output channels; the data gradient of a 16 -> 192 layer
    _fwd("halo16-128-16-24x40", (2, 24, 40, 128, 16, 1, 0), "halo16"),
    _dg("halo16-dgrad-16-192-16x24-slab", (1, 16, 24, 16, 192, 1, 0), "halo16", slab=True),
    # merged stride-2 data gradient: interleaved class order, per-image order (Cin * Cout * 18 B above 2 MB), one 64-channel reduction block
    _dg("seg-dgrad-256-128-32x48", (2, 32, 48, 256, 128, 2, 0), "seg_interleaved"),
    _dg("seg-dgrad-128-256-32x48-slab", (2, 32, 48, 128, 256, 2, 0), "seg_interleaved", slab=True),
    _dg("seg-dgrad-128-64-32x32", (1, 32, 32, 128, 64, 2, 0), "seg_interleaved"),
    _dg("seg-dgrad-256-512-16x16", (2, 16, 16, 256, 512, 2, 0), "seg_per_image"),
    # four launches per parity class: shapes seg_dgrad_desc refuses (16 outputs; 80 reduction channels are no whole 64-channel blocks)
    _dg("classes-dgrad-16-64-32x32", (1, 32, 32, 16, 64, 2, 0), "per_class_halo16_fast"),
    _dg("classes-dgrad-128-80-32x32", (1, 32, 32, 128, 80, 2, 0), "per_class_generic"),
    # streaming stride-2 data gradient (bf16, 128 -> 128, plain / mask_bits), switch on and off
    _dg("stream-dgrad-34x66", (2, 34, 66, 128, 128, 2, 0), "stream", dtypes=("bf16",), eps=WIDE, stream=(1, 0)),
    _dg("stream-dgrad-16x16", (1, 16, 16, 128, 128, 2, 0), "stream", dtypes=("bf16",), eps=WIDE, stream=(1, 0)),
    # the widest layers
    _fwd("halo-512-1024-16x16", (1, 16, 16, 512, 1024, 1, 0), "halo", eps=WIDE),
    _fwd("halo-s2-1024-1024-16x16", (1, 16, 16, 1024, 1024, 2, 0), S2_8W, eps=WIDE),
    _dg("halo-dgrad-512-1024-16x16", (1, 16, 16, 512, 1024, 1, 0), "halo", eps=WIDE),
    _dg("seg-dgrad-1024-1024-16x16", (1, 16, 16, 1024, 1024, 2, 0), "seg_per_image", eps=WIDE),
    # row-tiled fast kernel: whole 64-channel reduction blocks with <= 64 outputs, or a grid under 8 x 8
    _fwd("rows-fast-128-128-6x10", (3, 6, 10, 128, 128, 1, 0), "rows_fast"),
]
for _ci, _dts in ((64, ("f32", "bf16")), (128, ("bf16",))):
    for _co in (32, 64):
        CASES.append(_fwd(f"rows-fast-{_ci}-{_co}-12x20", (1, 12, 20, _ci, _co, 1, 0), "rows_fast", dtypes=_dts, slab=_co == 32 and _ci == 64))
# row-tiled generic kernel (reduction channels in no whole 64-channel blocks), all four output tile widths, both strides
for _co in (16, 32, 64, 128):
    for _st in (1, 2):
        CASES.append(_fwd(f"rows-generic-16-{_co}-12x20-s{_st}", (1, 12, 20, 16, _co, _st, 0), "rows_generic", slab=_co == 64 and _st == 1))
# im2col forward: 1 and 2 real input channels, padded and compact sources; 24 rows (linear group order), 48 rows (tiled order)
for _cr in (1, 2):
    for _cp in (False, True):
        CASES.append(_fwd(f"im2col-c{_cr}-128-24x32" + ("-compact" if _cp else ""), (1, 24, 32, 16, 128, 1, 0), "im2col_linear", cin_real=_cr, compact=_cp))
        CASES.append(_fwd(f"im2col-c{_cr}-256-48x64" + ("-compact" if _cp else ""), (1, 48, 64, 16, 256, 1, 0), "im2col_tiled", cin_real=_cr, compact=_cp,
                          eps=("plain", "bias_act", "mask", "mask_bits", "out_bits")))

W1 = {"f32": "tap", "bf16": "wide_s1"}
W1R = {"f32": "rows", "bf16": "wide_s1"}
W2 = {"f32": "tap", "bf16": "wide_s2"}
BOTH = (True, False)
CASES += [
    # weight gradient, per-tap kernel
    _wg("wgrad-tap-16-16", (2, 16, 16, 16, 16, 1, 0), "tap", db=BOTH),
    _wg("wgrad-tap-64-32-s2", (1, 12, 20, 64, 32, 2, 0), "tap", db=BOTH),
    _wg("wgrad-tap-80-48-20x12", (1, 20, 12, 80, 48, 1, 0), "tap", db=BOTH),
    _wg("wgrad-tap-16-64ps", (2, 16, 16, 16, 64, 1, 1), "tap", db=(False,)),
    # narrow row-of-taps kernel
    _wg("wgrad-rows-256-64-8x32", (1, 8, 32, 256, 64, 1, 0), "rows", db=BOTH),
    # wide kernel, stride 1 (fused db): one tile pair; ragged channel tiles; pixel-shuffled adjoint
    _wg("wgrad-wide-128-128-8x32", (1, 8, 32, 128, 128, 1, 0), W1, db=BOTH),
    _wg("wgrad-wide-320-192-16x64", (1, 16, 64, 320, 192, 1, 0), W1R, db=BOTH),
    _wg("wgrad-wide-256-256ps-8x32", (1, 8, 32, 256, 256, 1, 1), W1R, db=(False,)),
    # ... 96 tiles per pixel range (> 72): the grouped launch order, 2 splits x 2 units of 48 tiles in 8 unit slots, half of the workgroups padding
    _wg("wgrad-wide-512-1024-8x64", (1, 8, 64, 512, 1024, 1, 0), W1R, db=(True,)),
]
# wide kernel, stride 2: Wo 32 and 64, two images
for _ci, _co in ((128, 128), (320, 192)):
    for _wo in (32, 64):
        CASES.append(_wg(f"wgrad-wide-s2-{_ci}-{_co}-wo{_wo}", (2, 16, 2 * _wo, _ci, _co, 2, 0), W2, db=BOTH))
# im2col kernel: 1 and 2 real input channels, rows of 32 pixels, padded and compact x
for _cr in (1, 2):
    for _cp in (False, True):
        CASES.append(_wg(f"wgrad-im2col-c{_cr}-128-8x32" + ("-compact" if _cp else ""), (2, 8, 32, 16, 128, 1, 0), "im2col", cin_real=_cr, compact=_cp, db=BOTH))
CASES += [
    Case("wgrad-dense-1", "dense", (1, 8, 32, 1), "dense", dtypes=("bf16",)),
    Case("wgrad-dense-3", "dense", (1, 8, 32, 3), "dense", dtypes=("bf16",)),
    Case("linear-2x512x112", "linear", (2, 512, 112), "dx_narrow"),
    Case("linear-33x1024x16", "linear", (33, 1024, 16), "dx_narrow"),
    Case("linear-40x4352x100", "linear", (40, 4352, 100), "dx_wide"),
    Case("linear-96x9608x112", "linear", (96, 256 * 37 + 136, 112), "dx_wide"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
PARAMS = [(c.id, dt) for c in CASES for dt in c.dtypes]
