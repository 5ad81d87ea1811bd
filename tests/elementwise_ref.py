"""Float64 references, comparators and the shared case table of the elementwise / reduction / layout kernel tests
(csrc/elementwise.hip; tests/test_elementwise_gpu.py on the device, tests/test_elementwise_ref_cpu.py on the host).

References.  Every ``ref_*`` restates one contract of include/downgan_hip.h in torch float64 on the CPU.  Tensor inputs are
taken as stored (already rounded to the compute dtype), scalar arguments are rounded to fp32 first (the C ABI takes ``float``);
the arithmetic on those values is float64.  Elementwise references also return ``M``, the per-element sum of the absolute
values of the terms they added.

Per-element comparator (``check_elem``).  |out - ref| <= 4 * 2^-24 * M, plus, for a bf16 output, one rounding to nearest:
2^(floor(log2 max(|ref|, |out|)) - 8), half a bf16 ulp (8 significant bits) in the binade of the larger of the two.  2^-24 is the
unit roundoff of fp32 and no kernel here chains more than four roundings, so both terms are derived, not measured.  Non-finite
values must match in kind and sign; where the reference is zero only the absolute term applies.

Exact comparator (``assert_bits``): equality of the bit patterns, for copies, layout converters, repacks and casts.

Reductions.  ``int_data`` draws small integers (exact in bf16) and asserts that max|value| * terms + |preload| stays below 2^24:
then every partial sum in any order is an integer fp32 holds exactly, the fp32 result must EQUAL the integer sum, and a dropped,
duplicated or misrouted element shows as an integer difference.  Sums of N(0,1) data are held to the project's criterion
(1e-5 of the column's sum of |terms|; rtol 1e-5 for sums of non-negative terms).

Case table.  ``CASES`` lists (id, function, keyword arguments, size); a case function takes (ops, dtype) where ``ops`` is
HipOps on the GPU or EmuOps on the CPU, builds its inputs on the host, runs the op on ``ops.device`` and asserts.  Sizes:
"small" and "view" run on both, "large" (grid-stride loops take a second trip, block caps are reached) on the GPU only.

Size guards.  A case that exists for its size carries ``expect=`` in its keyword arguments; the case function then asserts, from
the shape it is about to run (``guard_trip`` / ``guard_cap``), that the launch takes a second grid-stride trip or reaches its block
cap -- an edit of a shape cannot quietly turn the case back into a single-trip test.

``DG_EW_RATIOS=1`` in the environment makes every comparator print its worst error / bound (observations, never asserted).
"""
from __future__ import annotations

import os

import torch

U = 2.0 ** -24                       # unit roundoff of fp32
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
EW_THREADS = 4096 * 256              # ew_blocks: at most 4096 workgroups of 256 threads, grid-stride over the rest
GUARD = 1024                         # bytes of sentinel behind every device buffer
SENTINEL = 0xA5
INT_LIMIT = 2 ** 24

S_SHAPE = (3, 5, 7, 16)              # small, contiguous
G_SHAPE = (1, 728, 736, 16)          # grid-stride: 535,808 rows
V_SHAPE = (2, 9, 13, 48)             # view: channels [24, 72) of a slab 112 wide
V_SLAB, V_SLAB2 = (112, 24), (80, 16)


def f32(x):
    """A scalar as the C ABI receives it."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def d(t):
    return t.detach().cpu().double()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, dtype, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(TD[dtype] if isinstance(dtype, str) else dtype)


def int_data(shape, lo, hi, gen, dtype, terms, preload=0):
    """Integers in [lo, hi] as (int8 tensor, the same values in ``dtype``).  ``terms`` = how many of them one sum adds,
    ``preload`` = the largest magnitude already in the accumulator."""
    mag = max(abs(lo), abs(hi))
    assert mag <= 64, "integers above 2^8 are not exact in bf16"
    assert mag * terms + preload < INT_LIMIT, f"partial sums reach {mag * terms + preload} >= 2^24: fp32 would round"
    xi = torch.randint(lo, hi + 1, tuple(shape), generator=gen, dtype=torch.int8)
    return xi, xi.to(TD[dtype] if isinstance(dtype, str) else dtype)


def epc(dtype):
    """Elements per 16-byte chunk."""
    return 4 if dtype == "f32" else 8


# ---------------------------------------------------------------------------------------------------------------- comparators
def assert_bits(out, ref, what):
    o, r = bits(out), bits(ref)
    assert o.shape == r.shape and out.dtype == ref.dtype, f"{what}: {tuple(out.shape)} {out.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    if not torch.equal(o, r):
        bad = (o != r).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {o.numel()} elements differ in bits, first at flat index {i}: "
                             f"{float(out.detach().cpu().flatten()[i].float())!r} vs {float(ref.flatten()[i].float())!r}")


def half_ulp_bf16(ref, out):
    """2^(floor(log2 max(|ref|, |out|)) - 8); 0 where the reference is zero (absolute term alone)."""
    mag = torch.maximum(ref.abs(), out.abs())
    _, e = torch.frexp(mag)                          # mag = m * 2^e, m in [0.5, 1): floor(log2 mag) = e - 1
    h = torch.ldexp(torch.ones_like(mag), e - 9)
    return torch.where((ref != 0) & (mag > 0), h, torch.zeros_like(mag))


def elem_bound(ref, out, M, bf16_out):
    b = 4 * U * M
    return b + half_ulp_bf16(ref, out) if bf16_out else b


def _report(family, what, ratio):
    if os.environ.get("DG_EW_RATIOS"):
        print(f"[ew-ratio] {family} | {what} | {ratio:.4f}")


# ---------------------------------------------------------------------------------------------------------------- size guards
def guard_trip(expect, what, *work_items):
    """expect="second_trip": every launch of the case (``work_items`` = its threads' work items, one entry per launch) must be
    larger than the 4096 x 256 threads ew_blocks grants, so the grid-stride loop runs again."""
    assert expect in (None, "second_trip"), expect
    if expect:
        for n in work_items:
            assert n > EW_THREADS, f"size guard: {what} has {n} work items, not more than {EW_THREADS}: one grid-stride trip"


def guard_cap(expect, what, blocks_wanted, cap):
    """expect="cap": the launch wants more workgroups than its cap."""
    assert expect in (None, "cap"), expect
    if expect:
        assert blocks_wanted > cap, f"size guard: {what} wants {blocks_wanted} workgroups, the cap of {cap} is not reached"


def _cdiv(a, b):
    return -(-a // b)


def check_elem(out, ref, M, what, family="elementwise", factor=4):
    """The per-element comparator; ``factor`` is 4 unless a contract names another count of roundings.  Returns the worst
    error / bound."""
    o = d(out)
    assert o.shape == ref.shape == M.shape, f"{what}: {tuple(o.shape)} vs {tuple(ref.shape)} / {tuple(M.shape)}"
    kind = (torch.isnan(ref) == torch.isnan(o)) & (torch.isinf(ref) == torch.isinf(o))
    kind &= ~torch.isinf(ref) | (torch.sign(ref) == torch.sign(o))
    if not bool(kind.all()):
        i = int((~kind).flatten().nonzero()[0])
        raise AssertionError(f"{what}: non-finite mismatch at flat index {i}: got {float(o.flatten()[i])!r}, "
                             f"reference {float(ref.flatten()[i])!r}")
    fin = torch.isfinite(ref)
    zero = torch.zeros_like(ref)
    err = torch.where(fin, (o - ref).abs(), zero)
    bound = torch.where(fin, elem_bound(ref, o, M * (factor / 4.0), out.dtype == torch.bfloat16), zero)
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), zero))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _report(family, what, worst)
    if worst > 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements outside the bound; worst at flat index "
                             f"{i}: got {float(o.flatten()[i])!r}, reference {float(ref.flatten()[i])!r}, error "
                             f"{float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e}")
    return worst


def check_exact_sum(out, ref, what, family="reduction"):
    """fp32 result == integer reference, element for element."""
    o, r = d(out), ref.double()
    assert o.shape == r.shape, f"{what}: {tuple(o.shape)} vs {tuple(r.shape)}"
    assert float(r.abs().max()) < INT_LIMIT, f"{what}: reference total {float(r.abs().max())} >= 2^24"
    if not torch.equal(o, r):
        i = int((o != r).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int((o != r).sum())} of {o.numel()} sums differ; index {i}: got {float(o.flatten()[i])!r}, "
                             f"exact {float(r.flatten()[i])!r} (difference {float((o - r).flatten()[i])!r})")
    _report(family, what + " (exact)", 0.0)


def check_sum(out, ref, scale, what, rel=1e-5, family="reduction"):
    """|out - ref| <= rel * scale, scale = |ref| for sums of non-negative terms, the sum of |terms| otherwise."""
    o, r, s = d(out), ref.double(), scale.double()
    assert o.shape == r.shape == s.shape, what
    err, bound = (o - r).abs(), rel * s
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    _report(family, what, worst)
    assert worst <= 1.0, f"{what}: error {float(err.flatten()[int(ratio.flatten().argmax())]):.3e} is {worst:.3f} x the bound"
    return worst


def same_bits(outs, what):
    for o in outs[1:]:
        assert_bits(o, outs[0], what + ": two runs differ")


# ---------------------------------------------------------------------------------------------------------------- references
def lgrad(y, slope):
    """y > 0 ? 1 : slope -- false for -0, +0 and NaN."""
    y = d(y)
    return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, f32(slope)))


def ref_mask_mul(u, y, slope):
    return d(u) * lgrad(y, slope), d(u).abs()


def ref_axpby(x, a, y=None, b=0.0):
    t1 = f32(a) * d(x)
    t2 = f32(b) * d(y) if y is not None else torch.zeros_like(t1)
    return t1 + t2, t1.abs() + t2.abs()


def ref_interp(real, fake, alpha, swap=False):
    al = d(alpha).view(-1, 1, 1, 1)
    if swap:
        al = 1 - al
    t1, t2 = al * d(real), (1 - al) * d(fake)
    return t1 + t2, t1.abs() + t2.abs()


def ref_scale_rows(g, coef):
    t = d(g) * d(coef).view(-1, 1, 1, 1)
    return t, t.abs()


def ref_l1(a, b, grad_scale=0.0, addend=None):
    """-> (sum |a - b|, gradient, M of the gradient)."""
    diff = d(a) - d(b)
    ad = d(addend) if addend is not None else torch.zeros_like(diff)
    gs = f32(grad_scale)
    return diff.abs().sum(), torch.sign(diff) * gs + ad, gs + ad.abs()


def ref_sqdiff(a, b):
    return ((d(a) - d(b)) ** 2).sum()


def ref_sumsq_rows(g, ss0):
    return d(ss0) + (d(g) ** 2).reshape(g.shape[0], -1).sum(1)


def ref_colsum(dy, db0, drop_row=None, twice_row=None):
    """-> (db0 + column sums, |db0| + column sums of |dy|)."""
    x = d(dy).reshape(-1, dy.shape[-1])
    s = x.sum(0)
    if drop_row is not None:
        s = s - x[drop_row]
    if twice_row is not None:
        s = s + x[twice_row]
    return d(db0) + s, d(db0).abs() + x.abs().sum(0)


def ref_colsum_ps(dy, db0):
    f = dy.shape[-1]
    out, sabs = d(db0).clone(), d(db0).abs()
    for i in range(2):
        for j in range(2):
            sub = d(dy)[:, i::2, j::2, :].reshape(-1, f)
            out[(2 * i + j) * f:(2 * i + j + 1) * f] += sub.sum(0)
            sabs[(2 * i + j) * f:(2 * i + j + 1) * f] += sub.abs().sum(0)
    return out, sabs


def ref_gp_finish(ss, B, B_global, gp_lambda, weight):
    """-> (coef, magnitude the 8 * 2^-24 bound of coef is relative to, scalar).  n = sqrt(ss + 1e-12); coef = k (n - 1) / n with
    k = weight lambda 2 / B_global.  The bound is relative to |coef| itself wherever n - 1 does not cancel (|n - 1| >= 1/2); where it
    does (ss = 1: fp32 gives n = 1 and coef = 0 exactly, float64 about 5e-14) it is relative to the terms added, n and 1:
    M = |k| (n + 1) / n."""
    n = torch.sqrt(d(ss)[:B] + 1e-12)
    k = f32(weight) * f32(gp_lambda) * 2.0 / B_global
    coef = k * (n - 1) / n
    mag = torch.where((n - 1).abs() >= 0.5, coef.abs(), abs(k) * (n + 1) / n)
    return coef, mag, f32(gp_lambda) * ((n - 1) ** 2).sum() / B_global


def ref_sum_strided(inp, n, stride, scale):
    v = d(inp).reshape(-1)[:n * stride:stride]
    return f32(scale) * v.sum(), abs(f32(scale)) * v.abs().sum()


def ref_bias_act(inp, bias, C, act=None, mask=None, mask_slope=1.0):
    v = d(inp)[:, :C].clone()
    M = v.abs()
    if bias is not None:
        v = v + d(bias)[:C]
        M = M + d(bias)[:C].abs()
    if act is not None:
        f = torch.where(v > 0, torch.ones_like(v), torch.full_like(v, f32(act)))
        v, M = v * f, M * f.abs()
    if mask is not None:
        f = lgrad(mask, mask_slope)
        v, M = v * f, M * f.abs()
    return v, M


def ref_adam(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0, use_grad_scale=True, bc2_step=None):
    """torch.optim.Adam on the fp32-rounded hyper-parameters -> dict of (reference, bound) for p, m, v.
    Bounds: 4 * 2^-24 * M for the moments; 8 * 2^-24 * (|p| + lr / bc1 * |m / denom|) for the parameter."""
    lr, b1, b2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
    gg = d(g) * (f32(grad_scale) if use_grad_scale else 1.0)
    m1, m2 = b1 * d(m), (1 - b1) * gg
    v1, v2 = b2 * d(v), (1 - b2) * gg * gg
    mn, vn = m1 + m2, v1 + v2
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** (step if bc2_step is None else bc2_step)
    denom = torch.sqrt(vn) / bc2 ** 0.5 + eps
    upd = (lr / bc1) * (mn / denom)
    return {"p_m_error": (lr / bc1) * 4 * U * (m1.abs() + m2.abs()) / denom,      # the bound of m carried through m / denom
            "p": (d(p) - upd, 8 * U * (d(p).abs() + upd.abs())),
            "m": (mn, 4 * U * (m1.abs() + m2.abs())),
            "v": (vn, 4 * U * (v1.abs() + v2.abs()))}


def check_abs(out, ref, bound, what, family):
    o = d(out)
    err = (o - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    _report(family, what, worst)
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements outside the bound; worst at {i}: got "
                             f"{float(o.flatten()[i])!r}, reference {float(ref.flatten()[i])!r}, bound {float(bound.flatten()[i]):.3e}")
    return worst


def ref_nchw_to_nhwc(src, cpad, tdtype):
    n, c, h, w = src.shape
    out = torch.zeros(n, h, w, cpad, dtype=tdtype)
    out[..., :c] = src.permute(0, 2, 3, 1).to(tdtype)
    return out


def ref_nhwc_to_nchw(src, c):
    return src[..., :c].float().permute(0, 3, 1, 2).contiguous()


def ref_repack(master, cout, cin, kind, tdtype, mirror=True):
    m = master.view(cout, 9, cin)
    if kind == 0:
        return m.reshape(-1).to(tdtype)
    r = m.permute(2, 1, 0)
    if kind == 2 and mirror:
        r = r.flip(1)
    return r.reshape(-1).to(tdtype)


def ref_repack_dense(masters, F_, tdtype):
    """dst_j[ci][tap][(k - j - 1) F + co] = W_k[co][tap][j F + ci], k = j + 1 .. n; the packs concatenated."""
    n, parts = len(masters), []
    for j in range(n):
        dst = torch.zeros(F_, 9, (n - j) * F_)
        for k in range(j + 1, n + 1):
            wk = masters[k - 1].view(F_, 9, k * F_)
            dst[:, :, (k - j - 1) * F_:(k - j) * F_] = wk[:, :, j * F_:(j + 1) * F_].permute(2, 1, 0)
        parts.append(dst.reshape(-1))
    return torch.cat(parts).to(tdtype)


def ref_wgrad_unswap(tmp, dw, cout, cin):
    """dw[co][t][ci] + tmp[ci][8 - t][co]: one fp32 addition per element, so torch's fp32 sum has the same bits."""
    return (dw.view(cout, 9, cin) + tmp.view(cin, 9, cout).flip(1).permute(2, 1, 0)).reshape(-1)


def ref_gather(store, idx, cpad, shift=0):
    i = idx.long()
    if shift:
        i = i[(torch.arange(i.numel()) - shift) % i.numel()]
    out = torch.zeros(i.numel(), store.shape[1], store.shape[2], cpad, dtype=store.dtype)
    out[..., :store.shape[3]] = store[i]
    return out


# ---------------------------------------------------------------------------------------------------------------- device buffers
class Buf:
    """``values`` on ``ops.device`` with a guard of sentinel bytes behind it; with ``slab=(width, lo)`` the values are channels
    [lo, lo + C) of a random slab ``width`` channels wide and ``dev`` is that view."""

    def __init__(self, ops, values, slab=None):
        self.cpu = values.contiguous()
        if slab is None:
            self.host, self.sl = self.cpu, None
        else:
            width, lo = slab
            self.host = randn(tuple(values.shape[:-1]) + (width,), values.dtype, _gen(width * 131 + lo))
            self.sl = slice(lo, lo + values.shape[-1])
            self.host[..., self.sl] = self.cpu
        n = self.host.numel() * self.host.element_size()
        self.raw = torch.full((n + GUARD,), SENTINEL, dtype=torch.uint8, device=ops.device)
        self.full = self.raw[:n].view(self.host.dtype).view(self.host.shape)
        self.full.copy_(self.host)
        self.dev = self.full if slab is None else self.full[..., self.sl]
        self.nbytes = n

    def result(self):
        return self.dev.detach().to("cpu", copy=True).contiguous()       # a copy on the host too: callers keep results across launches

    def check(self, what, written=True):
        """The guard survives, every byte outside the view is unchanged, and so is the view itself unless ``written``."""
        assert bool((self.raw[self.nbytes:] == SENTINEL).all()), f"{what}: the guard behind the buffer was overwritten"
        if self.sl is None and written:
            return
        after = self.full.detach().cpu().clone()
        if written:
            after[..., self.sl] = self.host[..., self.sl]
        assert_bits(after, self.host, f"{what}: bytes outside the written range")


def _place(ops, values, view, which=0):
    return Buf(ops, values, slab=(V_SLAB, V_SLAB2)[which] if view else None)


# ---------------------------------------------------------------------------------------------------------------- cases: elementwise
def _rows(shape):
    return shape[0] * shape[1] * shape[2]


def case_mask_mul(ops, dtype, shape=S_SHAPE, view=False, expect=None):
    guard_trip(expect, "mask_mul", _rows(shape) * (shape[3] // epc(dtype)))
    gen = _gen(101)
    u = _place(ops, randn(shape, dtype, gen), view, 0)
    y = _place(ops, randn(shape, dtype, gen), view, 1)
    ops.mask_mul(u.dev, y.dev, 0.01)
    check_elem(u.result(), *ref_mask_mul(u.cpu, y.cpu, 0.01), "mask_mul")
    u.check("mask_mul u"); y.check("mask_mul y", written=False)


def case_axpby(ops, dtype, shape=S_SHAPE, view=False, with_y=True, in_place=False, expect=None):
    guard_trip(expect, "axpby", _rows(shape) * (shape[3] // epc(dtype)))
    gen = _gen(102)
    x = _place(ops, randn(shape, dtype, gen), view and not in_place, 1)
    y = _place(ops, randn(shape, dtype, gen), view, 1) if with_y else None
    out = x if in_place else _place(ops, randn(shape, dtype, gen), view, 0)
    a, b = 0.2, -1.7
    ops.axpby(out.dev, x.dev, a, y.dev if with_y else None, b if with_y else 0.0)
    check_elem(out.result(), *ref_axpby(x.cpu, a, y.cpu if with_y else None, b), f"axpby y={with_y} in_place={in_place}")
    out.check("axpby out")
    if not in_place:
        x.check("axpby x", written=False)
    if with_y:
        y.check("axpby y", written=False)


def case_gp_interp(ops, dtype, shape=S_SHAPE, expect=None):
    guard_trip(expect, "gp_interp (per image)", shape[1] * shape[2] * shape[3] // epc(dtype))
    gen = _gen(103)
    real, fake = Buf(ops, randn(shape, dtype, gen)), Buf(ops, randn(shape, dtype, gen))
    alpha = torch.rand(shape[0], generator=gen)
    out = Buf(ops, randn(shape, dtype, gen))
    ops.gp_interp(real.dev, fake.dev, alpha.to(ops.device), out.dev)
    check_elem(out.result(), *ref_interp(real.cpu, fake.cpu, alpha), "gp_interp")
    out.check("gp_interp"); real.check("gp_interp real", written=False); fake.check("gp_interp fake", written=False)


def case_scale_rows(ops, dtype, shape=S_SHAPE, expect=None):
    guard_trip(expect, "scale_rows (per image)", shape[1] * shape[2] * shape[3] // epc(dtype))
    gen = _gen(104)
    g = Buf(ops, randn(shape, dtype, gen))
    coef = torch.randn(shape[0], generator=gen)
    out = Buf(ops, randn(shape, dtype, gen))
    ops.scale_rows(g.dev, coef.to(ops.device), out.dev)
    check_elem(out.result(), *ref_scale_rows(g.cpu, coef), "scale_rows")
    out.check("scale_rows"); g.check("scale_rows g", written=False)


def case_layout(ops, dtype, N=2, C=6, H=5, W=7, cpad=16, expect=None):
    guard_trip(expect, "nchw_to_nhwc / nhwc_to_nchw", N * H * W * cpad, N * C * H * W)      # one element per thread
    gen = _gen(105)
    src = torch.randn(N, C, H, W, generator=gen)
    nhwc = Buf(ops, randn((N, H, W, cpad), dtype, gen))          # stale content: the padding channels must be zeroed
    ops.nchw_to_nhwc(src.to(ops.device), nhwc.dev)
    ref = ref_nchw_to_nhwc(src, cpad, TD[dtype])
    assert_bits(nhwc.result(), ref, "nchw_to_nhwc")
    nhwc.check("nchw_to_nhwc")
    back = Buf(ops, torch.randn(N, C, H, W, generator=gen))
    ops.nhwc_to_nchw(nhwc.dev, back.dev)
    assert_bits(back.result(), ref_nhwc_to_nchw(ref, C), "nhwc_to_nchw")
    back.check("nhwc_to_nchw")


def case_nhwc_to_nchw_full(ops, dtype, shape=S_SHAPE, view=False, expect=None):
    """Every channel of the source (C = lds when contiguous, lds > C from a slab slice)."""
    guard_trip(expect, "nhwc_to_nchw", _rows(shape) * shape[3])
    gen = _gen(106)
    src = _place(ops, randn(shape, dtype, gen), view, 0)
    n, h, w, c = shape
    back = Buf(ops, torch.randn(n, c, h, w, generator=gen))
    ops.nhwc_to_nchw(src.dev, back.dev)
    assert_bits(back.result(), ref_nhwc_to_nchw(src.cpu, c), "nhwc_to_nchw")
    back.check("nhwc_to_nchw"); src.check("nhwc_to_nchw src", written=False)


def case_cast(ops, dtype, n=1037, expect=None):
    guard_trip(expect, "cast", n)
    gen = _gen(107)
    src = torch.randn(n, generator=gen)
    dst = Buf(ops, randn((n,), dtype, gen))
    ops.cast(src.to(ops.device), dst.dev)
    assert_bits(dst.result(), src.to(TD[dtype]), "cast")
    dst.check("cast")


def case_compact(ops, dtype, shape=(3, 6, 10, 16), expect=None):
    """gp_interp with real_c / fake_c and scale_rows to [..., 2]: the copies are bit-exact, the compact interpolate has the bits of
    the padded kernel's first two channels, and both obey the per-element bound."""
    # one thread = 16 bytes of compact output: 4 bf16 / 2 fp32 pixels; the padded interpolate: one chunk per thread
    guard_trip(expect, "gp_interp_c2 / scale_rows_c2 / gp_interp (per image)", shape[1] * shape[2] // (epc(dtype) // 2),
               shape[1] * shape[2] * shape[3] // epc(dtype))
    gen = _gen(108)
    B = shape[0]
    c2 = tuple(shape[:3]) + (2,)
    real, fake = Buf(ops, randn(shape, dtype, gen)), Buf(ops, randn(shape, dtype, gen))
    alpha = torch.rand(B, generator=gen)
    xc, rc, fc = (Buf(ops, randn(c2, dtype, gen)) for _ in range(3))
    ops.gp_interp(real.dev, fake.dev, alpha.to(ops.device), xc.dev, rc.dev, fc.dev)
    assert_bits(rc.result(), real.cpu[..., :2].contiguous(), "gp_interp_c2 real_c")
    assert_bits(fc.result(), fake.cpu[..., :2].contiguous(), "gp_interp_c2 fake_c")
    ref, M = ref_interp(real.cpu[..., :2], fake.cpu[..., :2], alpha)
    check_elem(xc.result(), ref, M, "gp_interp_c2")
    full = Buf(ops, randn(shape, dtype, gen))
    ops.gp_interp(real.dev, fake.dev, alpha.to(ops.device), full.dev)
    assert_bits(xc.result(), full.result()[..., :2].contiguous(), "gp_interp_c2 vs the padded kernel")
    xc2 = Buf(ops, randn(c2, dtype, gen))
    ops.gp_interp(real.dev, fake.dev, alpha.to(ops.device), xc2.dev)          # without the copies
    assert_bits(xc2.result(), xc.result(), "gp_interp_c2 without copies")
    coef = torch.randn(B, generator=gen)
    vc = Buf(ops, randn(c2, dtype, gen))
    ops.scale_rows(real.dev, coef.to(ops.device), vc.dev)
    ref, M = ref_scale_rows(real.cpu[..., :2], coef)
    check_elem(vc.result(), ref, M, "scale_rows_c2")
    for b_, name in ((xc, "xhat_c"), (rc, "real_c"), (fc, "fake_c"), (xc2, "xhat_c (no copies)"), (vc, "scale_rows_c2"), (full, "xhat")):
        b_.check(name)
    real.check("real", written=False); fake.check("fake", written=False)


def case_special(ops, dtype):
    """+-0 and NaN in the mask operand; a == b in L1; exact bf16 ties of both parities; a finite fp32 result that rounds to bf16 Inf."""
    td = TD[dtype]
    shape = (1, 1, 2, 8)
    nan, inf = float("nan"), float("inf")
    y = torch.tensor([0.0, -0.0, nan, 1.0, -1.0, 2.0 ** -126, -2.0 ** -126, inf] * 2).view(shape).to(td)
    u = torch.tensor([1.0, -2.0, 3.0, -4.0, 5.0, -6.0, 7.0, -8.0, 0.5, 0.25, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5]).view(shape).to(td)
    ub = Buf(ops, u)
    ops.mask_mul(ub.dev, y.to(ops.device), 0.25)                       # 0.25 u is exact in either dtype: compare bits
    keep = torch.tensor([False, False, False, True, False, True, False, True] * 2).view(shape)
    assert_bits(ub.result(), torch.where(keep, u.float(), u.float() * 0.25).to(td), "mask_mul with +-0 / NaN / +-tiny / Inf masks")
    check_elem(ub.result(), *ref_mask_mul(u, y, 0.25), "mask_mul special")
    # a == b: |a - b| adds nothing and the gradient is the addend (or 0) exactly
    a = randn(shape, dtype, _gen(109))
    add = randn(shape, dtype, _gen(110))
    for addend in (add, None):
        acc, gr = Buf(ops, torch.tensor([3.0])), Buf(ops, randn(shape, dtype, _gen(111)))
        ops.l1(a.to(ops.device), a.clone().to(ops.device), acc.dev, grad=gr.dev, grad_scale=0.37,
               addend=addend.to(ops.device) if addend is not None else None)
        assert_bits(gr.result(), addend if addend is not None else torch.zeros(shape, dtype=td), "l1 gradient at a == b")
        assert_bits(acc.result(), torch.tensor([3.0]), "l1 sum at a == b")
    if dtype != "bf16":
        return
    # fp32 results that are exact bf16 ties: x + y with x = 1 (or 1 + 2^-7) and y = 2^-8 -> the even neighbour
    x = torch.tensor([1.0, 1.0 + 2.0 ** -7, -1.0, -(1.0 + 2.0 ** -7), 1.0, 1.0, 1.0, 1.0]).view(1, 1, 1, 8).to(td)
    t = torch.tensor([2.0 ** -8, 2.0 ** -8, -2.0 ** -8, -2.0 ** -8, 0.0, 0.0, 0.0, 0.0]).view(1, 1, 1, 8).to(td)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6), 1.0, 1.0, 1.0, 1.0]).view(1, 1, 1, 8).to(td)
    out = Buf(ops, torch.zeros(1, 1, 1, 8, dtype=td))
    ops.axpby(out.dev, x.to(ops.device), 1.0, t.to(ops.device), 1.0)
    assert_bits(out.result(), want, "bf16 ties round to even")
    # (1 + 2^-8) * max_bf16 = (2 - 2^-15) * 2^127 is an exact, finite fp32 (FLT_MAX = 3.40282347e38) above the bf16 rounding
    # threshold max_bf16 + half an ulp = (2 - 2^-8) * 2^127 = 3.3961775e38: it rounds to bf16 Inf
    big = torch.tensor([3.3895313892515355e38, -3.3895313892515355e38] * 4).view(1, 1, 1, 8).to(td)
    a_ = 1.00390625                                                   # 1 + 2^-8, exact in fp32
    prod = a_ * big.double()
    assert bool((prod.abs() < 3.4028234663852886e38).all()) and bool((prod.abs() > 3.3961775292304e38).all())
    out = Buf(ops, torch.zeros(1, 1, 1, 8, dtype=td))
    ops.axpby(out.dev, big.to(ops.device), a_)
    assert_bits(out.result(), torch.tensor([inf, -inf] * 4).view(1, 1, 1, 8).to(td), "finite fp32 that rounds to bf16 Inf")


# ---------------------------------------------------------------------------------------------------------------- cases: reductions
def _runs(ops, fn, runs, what):
    outs = [fn() for _ in range(runs)]
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            assert_bits(x, y, what + ": two runs differ")
    return outs[0]


def case_sumsq(ops, dtype, shape=(3, 5, 7, 8), data="int", runs=1, expect=None):
    gen = _gen(120)
    B, per = shape[0], shape[1] * shape[2] * shape[3]
    guard_cap(expect, "sumsq_rows (per image)", _cdiv(per // epc(dtype), 2048), 512)
    if data == "int":
        _, x = int_data(shape, -1, 1, gen, dtype, terms=per, preload=9)
        ss0 = torch.randint(1, 10, (B,), generator=gen).float()
    else:
        x, ss0 = randn(shape, dtype, gen, 1e-3), torch.zeros(B)
    g = Buf(ops, x)

    def run():
        ss = Buf(ops, ss0)
        ops.sumsq_rows(g.dev, ss.dev)
        ss.check("sumsq_rows ss")
        return (ss.result(),)
    (out,) = _runs(ops, run, runs, "sumsq_rows")
    ref = ref_sumsq_rows(x, ss0)
    if data == "int":
        check_exact_sum(out, ref, f"sumsq_rows {shape}")
    else:
        check_sum(out, ref, ref.abs(), f"sumsq_rows {shape} N(0,1)e-3")
    g.check("sumsq_rows g", written=False)


def case_gp_finish(ops, dtype, B=70, B_global=140):
    gen = _gen(121)
    ss = torch.rand(B, generator=gen) * 96 + 4             # n in [2, 10]: (n - 1)^2 is well conditioned
    ss[3], ss[64] = 0.0, 1.0                                # n = 1e-6 (coef finite); n = 1 (coef = 0 within the bound)
    coef, sc = Buf(ops, torch.full((B,), 7.0)), Buf(ops, torch.full((1,), 7.0))
    ops.gp_finish(ss.to(ops.device), B, B_global, 10.0, 0.7, coef.dev, sc.dev)
    cref, cM, sref = ref_gp_finish(ss, B, B_global, 10.0, 0.7)
    assert int((cM == cref.abs()).sum()) == B - 1          # every entry but ss = 1 is held to the relative bound
    assert bool(torch.isfinite(coef.result()).all())
    check_elem(coef.result(), cref, cM, "gp_finish coef", family="gp_finish", factor=8)
    check_sum(sc.result(), sref.view(1), sref.abs().view(1), "gp_finish scalar", rel=(B + 8) * U, family="gp_finish")
    coef.check("coef"); sc.check("scalar")
    # sum_strided: the same 64-lane stride loop
    inp = torch.rand(B, 3, generator=gen) + 0.5
    out = Buf(ops, torch.full((1,), 7.0))
    ops.sum_strided(inp.to(ops.device), B, 3, 1.0 / B, out.dev)
    ref, sabs = ref_sum_strided(inp, B, 3, 1.0 / B)
    check_sum(out.result(), ref.view(1), sabs.view(1), "sum_strided", rel=(B + 8) * U, family="gp_finish")
    out.check("sum_strided")


def case_l1(ops, dtype, shape=S_SHAPE, view=False, data="int", runs=1, sq=False, with_grad=True, expect=None):
    guard_cap(expect, "l1 / sqdiff", _cdiv(_rows(shape) * (shape[3] // epc(dtype)), 2048), 1024)
    gen = _gen(122)
    if data == "int":
        ai = torch.randint(-3, 4, shape, generator=gen, dtype=torch.int8)
        r = torch.randint(0, 4, shape, generator=gen, dtype=torch.int8)
        di = (r == 1).to(torch.int8) - (r == 2).to(torch.int8)          # 0 with p = 1/2, +1 and -1 with p = 1/4 each
        a, b = ai.to(TD[dtype]), (ai - di).to(TD[dtype])
        acc0 = torch.tensor([5.0])
    else:
        a, b, acc0 = randn(shape, dtype, gen), randn(shape, dtype, gen), torch.zeros(1)
    A, Bb = _place(ops, a, view, 0), _place(ops, b, view, 1)
    add = _place(ops, randn(shape, dtype, gen), view, 1) if with_grad and not sq else None

    def run():
        acc = Buf(ops, acc0)
        if sq:
            ops.sqdiff(A.dev, Bb.dev, acc.dev)
            acc.check("sqdiff acc")
            return (acc.result(),)
        gr = _place(ops, randn(shape, dtype, gen), view, 0) if with_grad else None
        ops.l1(A.dev, Bb.dev, acc.dev, grad=gr.dev if gr else None, grad_scale=0.37, addend=add.dev if add else None)
        acc.check("l1 acc")
        if gr:
            gr.check("l1 grad")
        return (acc.result(), gr.result()) if gr else (acc.result(),)
    out = _runs(ops, run, runs, "sqdiff" if sq else "l1")
    name = f"{'sqdiff' if sq else 'l1'} {shape}{' view' if view else ''}"
    if sq:
        total = ref_sqdiff(a, b) + acc0.double()
    else:
        total, gref, gM = ref_l1(a, b, 0.37, add.cpu if add else None)
        total = total + acc0.double()
    if data == "int":            # every term is 0 or 1: no partial sum in any order exceeds the total
        assert float(total) < INT_LIMIT, f"{name}: the exact total {float(total)} is not below 2^24"
        check_exact_sum(out[0], total.view(1), name)
    else:
        check_sum(out[0], total.view(1), total.abs().view(1), name + " N(0,1)")
    if not sq and with_grad:
        check_elem(out[1], gref, gM, name + " gradient")
    A.check(name + " a", written=False); Bb.check(name + " b", written=False)
    if add:
        add.check(name + " addend", written=False)


def _col_data(shape, dtype, gen, data, rows, preload):
    if data == "int":
        return int_data(shape, -4, 4, gen, dtype, terms=rows, preload=preload)[1]
    return randn(shape, dtype, gen)


def _check_cols(out, ref, sabs, data, what):
    if data == "int":
        check_exact_sum(out, ref, what)
    else:
        check_sum(out, ref, sabs, what + " N(0,1)")


def case_colsum(ops, dtype, rows=33, C=16, two_d=False, view=False, data="int", runs=1, data_dtype=None, expect=None):
    """db[c] += column sums of [rows, C]; ``two_d``: a 2-D tensor (``data_dtype`` fp32 whatever the compute dtype); ``view``: the
    V slice (rows = 234, C = 48).  expect="cap": rows / 256 exceeds the 128 workgroups and the last one is ragged."""
    gen = _gen(123)
    shape = V_SHAPE if view else ((rows, C) if two_d else (1, 1, rows, C))
    rows, C = (V_SHAPE[0] * V_SHAPE[1] * V_SHAPE[2], V_SHAPE[3]) if view else (rows, C)
    guard_cap(expect, "colsum", rows // 256, 128)
    if expect:
        assert rows % _cdiv(rows, 128) != 0, f"size guard: colsum of {rows} rows has no ragged last workgroup"
    x = _col_data(shape, data_dtype or dtype, gen, data, rows, 64)
    db0 = torch.randint(-64, 65, (C,), generator=gen).float()
    dy = _place(ops, x, view, 0)

    def run():
        db = Buf(ops, db0)
        ops.colsum(dy.dev, db.dev)
        db.check("colsum db")
        return (db.result(),)
    (out,) = _runs(ops, run, runs, "colsum")
    _check_cols(out, *ref_colsum(x, db0), data, f"colsum [{rows}, {C}]{' view' if view else ''}{' 2-D' if two_d else ''}")
    dy.check("colsum dy", written=False)


def case_colsum_ps(ops, dtype, shape=(2, 10, 14, 24), slab=None, data="int", runs=1, expect=None):
    gen = _gen(124)
    f = shape[-1]
    rows = shape[0] * shape[1] * shape[2] // 4
    guard_cap(expect, "colsum_ps (per sub-position)", rows // 256, 128)
    x = _col_data(shape, dtype, gen, data, rows, 64)
    db0 = torch.randint(-64, 65, (4 * f,), generator=gen).float()
    dy = Buf(ops, x, slab=slab)

    def run():
        db = Buf(ops, db0)
        ops.colsum_ps(dy.dev, db.dev)
        db.check("colsum_ps db")
        return (db.result(),)
    (out,) = _runs(ops, run, runs, "colsum_ps")
    _check_cols(out, *ref_colsum_ps(x, db0), data, f"colsum_ps {shape}{' slab' if slab else ''}")
    dy.check("colsum_ps dy", written=False)


def case_colsum_multi(ops, dtype, shape=(1, 9, 13, 640), nseg=5, data="int", runs=1, expect=None):
    """expect="cap": more workgroups than the 128 a single destination is capped at (the multi pass may use 128 per segment; its
    own cap of 128 * nseg would need rows >= 32768 * nseg)."""
    gen = _gen(125)
    C = shape[-1]
    rows = shape[0] * shape[1] * shape[2]
    guard_cap(expect, "colsum_multi", min(rows // 256, 128 * nseg), 128)
    x = _col_data(shape, dtype, gen, data, rows, 64)
    db0 = torch.randint(-64, 65, (nseg, C // nseg), generator=gen).float()
    dy = Buf(ops, x)

    def run():
        db = Buf(ops, db0)
        ops.colsum_multi(dy.dev, [db.dev[k] for k in range(nseg)])
        db.check("colsum_multi db")
        return (db.result(),)
    (out,) = _runs(ops, run, runs, "colsum_multi")
    if data == "int":            # integer sums without a float64 copy of the (possibly 70 M element) tensor
        x2 = x.reshape(-1, C)
        ref = db0.double().reshape(-1) + sum(x2[i:i + 65536].double().sum(0) for i in range(0, rows, 65536))
        check_exact_sum(out.reshape(-1), ref, f"colsum_multi {shape} / {nseg}")
    else:
        ref, sabs = ref_colsum(x, db0.reshape(-1))
        check_sum(out.reshape(-1), ref, sabs, f"colsum_multi {shape} / {nseg} N(0,1)")
    dy.check("colsum_multi dy", written=False)


def colsum_c256(dtype):
    """The widest column sum: 256 chunks, one row lane per workgroup."""
    return 1024 if dtype == "f32" else 2048


def case_colsum_c256(ops, dtype, data="int", runs=1):
    assert colsum_c256(dtype) // epc(dtype) == 256
    case_colsum(ops, dtype, rows=300, C=colsum_c256(dtype), data=data, runs=runs)


# ---------------------------------------------------------------------------------------------------------------- cases: Adam, packs, feed, head
def case_adam(ops, dtype, n=4 * 1040, grad_scale=1.0, shadow=True, expect=None):
    """Steps 1, 2 and 1000 in sequence on the state the op itself left (the reference restarts from that state at every step, so
    nothing accumulates).  Every step's gradient is a positive multiple of the first one: m and the new gradient then share a sign
    and beta1 m + (1 - beta1) g does not cancel, which the bound on p -- it has no term for a cancelled m -- needs."""
    guard_trip(expect, "adam", n // 4)
    gen = _gen(130)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-2
    g0[::97] = 0.0                                        # g = 0, v = 0: denom = eps, the update is 0 / eps = 0
    p, m, v = Buf(ops, p0), Buf(ops, torch.zeros(n)), Buf(ops, torch.zeros(n))
    sh = Buf(ops, torch.full((n,), 3.0, dtype=torch.bfloat16)) if shadow else None
    hp = (2.5e-4, 0.9, 0.99, 1e-8)
    for step, mult in ((1, 1.0), (2, 0.625), (1000, 1.75)):
        g = Buf(ops, g0 * mult)
        before = (p.result(), m.result(), v.result())
        ops.adam(p.dev, g.dev, m.dev, v.dev, sh.dev if shadow else None, *hp, step, grad_scale=grad_scale)
        ref = ref_adam(*before[:1], g.cpu, *before[1:], *hp, step, grad_scale)
        for name, buf in (("p", p), ("m", m), ("v", v)):
            check_abs(buf.result(), *ref[name], f"adam step {step} grad_scale {grad_scale} {name}", family="adam")
            buf.check("adam " + name)
        zero = (g0 == 0)
        assert_bits(p.result()[zero], before[0][zero], "adam: p where g = 0, v = 0")
        if shadow:
            assert_bits(sh.result(), p.result().to(torch.bfloat16), "adam shadow = RNE bf16 of p")
            sh.check("adam shadow")
        g.check("adam g", written=False)


def case_adam_mixed(ops, dtype, n=4 * 1040, grad_scale=0.5):
    """Independent m and g, the normal training situation: beta1 m + (1 - beta1) g cancels wherever their signs differ.  m and v
    keep the 4 * 2^-24 * M bound, which holds under cancellation; the bound of p gains the term it lacks for it, the bound of m
    carried through the update: lr / bc1 * (4 * 2^-24 * M_m) / denom."""
    gen = _gen(136)
    hp = (2.5e-4, 0.9, 0.99, 1e-8)
    for step in (2, 1000):
        p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 1e-2
        m0, v0 = torch.randn(n, generator=gen) * 1e-2, (torch.randn(n, generator=gen) * 1e-2) ** 2
        assert 0.3 < float(((m0 > 0) != (g0 > 0)).float().mean()) < 0.7
        p, g, m, v = Buf(ops, p0), Buf(ops, g0), Buf(ops, m0), Buf(ops, v0)
        sh = Buf(ops, torch.full((n,), 3.0, dtype=torch.bfloat16))
        ops.adam(p.dev, g.dev, m.dev, v.dev, sh.dev, *hp, step, grad_scale=grad_scale)
        ref = ref_adam(p0, g0, m0, v0, *hp, step, grad_scale)
        check_abs(m.result(), *ref["m"], f"adam mixed signs step {step} m", family="adam")
        check_abs(v.result(), *ref["v"], f"adam mixed signs step {step} v", family="adam")
        check_abs(p.result(), ref["p"][0], ref["p"][1] + ref["p_m_error"], f"adam mixed signs step {step} p", family="adam")
        assert_bits(sh.result(), p.result().to(torch.bfloat16), "adam shadow = RNE bf16 of p")
        for name, buf in (("p", p), ("m", m), ("v", v), ("shadow", sh)):
            buf.check("adam mixed " + name)
        g.check("adam mixed g", written=False)


def case_repack(ops, dtype, cout=48, cin=16, expect=None):
    guard_trip(expect, "repack", cout * 9 * cin)
    gen = _gen(131)
    master = torch.randn(cout * 9 * cin, generator=gen)
    for kind in (0, 1, 2):
        dst = Buf(ops, randn((cout * 9 * cin,), dtype, gen))
        ops.repack(master.to(ops.device), dst.dev, cout, cin, kind)
        assert_bits(dst.result(), ref_repack(master, cout, cin, kind, TD[dtype]), f"repack kind {kind} ({cout}, {cin})")
        dst.check(f"repack kind {kind}")


def case_repack_dense(ops, dtype, F_=8, n=8):
    gen = _gen(132)
    masters = [torch.randn(F_ * 9 * k * F_, generator=gen) for k in range(1, n + 1)]
    dst = Buf(ops, randn((9 * F_ * F_ * n * (n + 1) // 2,), dtype, gen))
    ops.repack_dense([m.to(ops.device) for m in masters], dst.dev, F_)
    assert_bits(dst.result(), ref_repack_dense(masters, F_, TD[dtype]), f"repack_dense F={F_} n={n}")
    dst.check("repack_dense")


def case_wgrad_unswap(ops, dtype, cout=48, cin=16):
    gen = _gen(133)
    tmp, dw0 = torch.randn(cout * 9 * cin, generator=gen), torch.randn(cout * 9 * cin, generator=gen)
    dw = Buf(ops, dw0)
    ops.wgrad_unswap(tmp.to(ops.device), dw.dev, cout, cin)
    assert_bits(dw.result(), ref_wgrad_unswap(tmp, dw0, cout, cin), f"wgrad_unswap ({cout}, {cin})")
    dw.check("wgrad_unswap")


def case_gather(ops, dtype, hw=(8, 12), c_real=3, c_pad=8, idx=(6, 0, 6, 3, 1), nstore=7, expect=None):
    guard_trip(expect, "gather_samples", len(idx) * hw[0] * hw[1] * (c_pad // epc(dtype)))
    gen = _gen(134)
    store = randn((nstore,) + tuple(hw) + (c_real,), dtype, gen)
    assert max(idx) == nstore - 1 and len(set(idx)) < len(idx) and list(idx) != sorted(idx)   # last sample, repeats, unsorted
    i = torch.tensor(idx, dtype=torch.int64)
    dst = Buf(ops, randn((len(idx),) + tuple(hw) + (c_pad,), dtype, gen))
    ops.gather_samples(store.to(ops.device), i.to(ops.device), dst.dev)
    ref = ref_gather(store, i, c_pad)
    assert_bits(dst.result(), ref, f"gather_samples c_real={c_real} c_pad={c_pad}")
    assert bool((bits(dst.result()[..., c_real:]) == 0).all()), "gather_samples: padding channels are +0"
    dst.check("gather_samples")


def case_head(ops, dtype, rows=70, C=112, ldi=128, ldo=120):
    gen = _gen(135)
    inp, bias = torch.randn(rows, ldi, generator=gen), torch.randn(ldi, generator=gen)
    for out_dt in (torch.float32, TD[dtype]):
        msk = Buf(ops, randn((rows, C), out_dt, gen), slab=(ldi, 0))
        for use_bias in (True, False):
            for act in (0.2, None):
                for use_mask in (True, False):
                    out = Buf(ops, randn((rows, C), out_dt, gen), slab=(ldo, 0))
                    ops.bias_act(inp.to(ops.device), bias.to(ops.device) if use_bias else None, out.dev, act=act,
                                 mask=msk.dev if use_mask else None, mask_slope=0.3)
                    ref, M = ref_bias_act(inp, bias if use_bias else None, C, act, msk.cpu if use_mask else None, 0.3)
                    what = f"bias_act {str(out_dt).split('.')[-1]} bias={use_bias} act={act} mask={use_mask}"
                    check_elem(out.result(), ref, M, what, family="head")
                    out.check(what)
        msk.check("bias_act mask", written=False)
    buf0 = torch.randn(rows, 16, generator=gen)
    buf = Buf(ops, buf0)
    ops.fill_col(buf.dev, 5, -0.25)
    want = buf0.clone(); want[:, 5] = -0.25
    assert_bits(buf.result(), want, "fill_col")
    buf.check("fill_col")


# ---------------------------------------------------------------------------------------------------------------- the table
def _c(cid, fn, size, **kw):
    return (cid, fn, kw, size)


CASES = [
    # small, contiguous
    _c("mask_mul-small", case_mask_mul, "small"),
    _c("axpby-small", case_axpby, "small"),
    _c("axpby-no-y-small", case_axpby, "small", with_y=False),
    _c("axpby-in-place-small", case_axpby, "small", in_place=True),
    _c("gp_interp-small", case_gp_interp, "small"),
    _c("scale_rows-small", case_scale_rows, "small"),
    _c("layout-small", case_layout, "small"),
    _c("nhwc_to_nchw-small", case_nhwc_to_nchw_full, "small"),
    _c("cast-small", case_cast, "small"),
    _c("special", case_special, "small"),
    _c("compact-16", case_compact, "small", shape=(3, 6, 10, 16)),
    _c("compact-8", case_compact, "small", shape=(3, 6, 10, 8)),
    _c("sumsq-3x5x7x8", case_sumsq, "small", shape=(3, 5, 7, 8)),
    _c("sumsq-70x2x2x8", case_sumsq, "small", shape=(70, 2, 2, 8)),
    _c("sumsq-normal", case_sumsq, "small", shape=(3, 24, 40, 16), data="normal"),
    _c("gp_finish-70", case_gp_finish, "small"),
    _c("l1-small", case_l1, "small"),
    _c("l1-small-normal", case_l1, "small", data="normal"),
    _c("sqdiff-small", case_l1, "small", sq=True),
    _c("colsum-2d-f32-5x128", case_colsum, "small", rows=5, C=128, two_d=True, data_dtype=torch.float32),
    _c("colsum-234x48", case_colsum, "small", rows=234, C=48),
    _c("colsum-33x16", case_colsum, "small", rows=33, C=16),
    _c("colsum-300xc256", case_colsum_c256, "small"),
    _c("colsum_ps", case_colsum_ps, "small"),
    _c("colsum_ps-slab", case_colsum_ps, "view", slab=(56, 16)),
    _c("colsum_multi-640x5", case_colsum_multi, "small", shape=(1, 9, 13, 640), nseg=5),
    _c("colsum_multi-128x8", case_colsum_multi, "small", shape=(1, 9, 13, 128), nseg=8),
    _c("adam-small", case_adam, "small"),
    _c("adam-small-gs0.5-no-shadow", case_adam, "small", grad_scale=0.5, shadow=False),
    _c("adam-mixed-signs", case_adam_mixed, "small"),
    _c("repack-48x16", case_repack, "small"),
    _c("repack_dense-8x8", case_repack_dense, "small"),
    _c("repack_dense-128x5", case_repack_dense, "small", F_=128, n=5),
    _c("wgrad_unswap-48x16", case_wgrad_unswap, "small"),
    _c("wgrad_unswap-16x128", case_wgrad_unswap, "small", cout=16, cin=128),
    _c("gather-small", case_gather, "small"),
    _c("head", case_head, "small"),
    # views: channels [24, 72) of a slab 112 wide, second operands from a slab 80 wide
    _c("mask_mul-view", case_mask_mul, "view", shape=V_SHAPE, view=True),
    _c("axpby-view", case_axpby, "view", shape=V_SHAPE, view=True),
    _c("l1-view", case_l1, "view", shape=V_SHAPE, view=True),
    _c("l1-view-normal", case_l1, "view", shape=V_SHAPE, view=True, data="normal"),
    _c("sqdiff-view", case_l1, "view", shape=V_SHAPE, view=True, sq=True),
    _c("colsum-view", case_colsum, "view", view=True),
    _c("nhwc_to_nchw-view", case_nhwc_to_nchw_full, "view", shape=V_SHAPE, view=True),
    # large: GPU only; each asserts from its own shape what it is there for (guard_trip / guard_cap)
    _c("mask_mul-G", case_mask_mul, "large", shape=G_SHAPE, expect="second_trip"),
    _c("axpby-G", case_axpby, "large", shape=G_SHAPE, expect="second_trip"),
    _c("axpby-no-y-G", case_axpby, "large", shape=G_SHAPE, with_y=False, expect="second_trip"),
    _c("axpby-in-place-G", case_axpby, "large", shape=G_SHAPE, in_place=True, expect="second_trip"),
    _c("gp_interp-G", case_gp_interp, "large", shape=G_SHAPE, expect="second_trip"),
    _c("scale_rows-G", case_scale_rows, "large", shape=G_SHAPE, expect="second_trip"),
    _c("layout-G", case_layout, "large", N=1, C=2, H=728, W=736, cpad=16, expect="second_trip"),
    _c("nhwc_to_nchw-G", case_nhwc_to_nchw_full, "large", shape=G_SHAPE, expect="second_trip"),
    _c("cast-G", case_cast, "large", n=1300001, expect="second_trip"),
    _c("compact-large", case_compact, "large", shape=(1, 2056, 2048, 8), expect="second_trip"),
    _c("sumsq-large", case_sumsq, "large", shape=(2, 728, 736, 16), expect="cap"),
    _c("l1-large", case_l1, "large", shape=(1, 728, 736, 32), expect="cap"),
    _c("sqdiff-large", case_l1, "large", shape=(1, 728, 736, 32), sq=True, expect="cap"),
    _c("colsum-300001x16", case_colsum, "large", rows=300001, C=16, expect="cap"),
    _c("repack-512x256", case_repack, "large", cout=512, cin=256, expect="second_trip"),
]
for _cr in (2, 3, 6):
    for _cp in (8, 16):
        CASES.append(_c(f"gather-512-c{_cr}-p{_cp}", case_gather, "large", hw=(512, 512), c_real=_cr, c_pad=_cp, expect="second_trip"))
for _gs in (1.0, 0.5):
    for _sh in (True, False):
        CASES.append(_c(f"adam-large-gs{_gs}-shadow{int(_sh)}", case_adam, "large", n=4 * (1048576 + 777), grad_scale=_gs, shadow=_sh,
                        expect="second_trip"))
