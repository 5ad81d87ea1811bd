"""Integer data, float64 references and the shared case table of the EXACT tests of the EOF kernels (csrc/eof.hip): mean, Gram and
projection on v_mfma_f32_32x32x2_f32 with their slice reduce, components with the sign rule, reconstruct.
tests/test_eof_exact_gpu.py runs the table through HipOps("f32") and requires equality of the bit patterns with the references below;
tests/test_eof_exact_cpu.py tests this file (budgets, references against explicit loops, mutation checks, coverage of the table).

Why bits.  Fields are x[t] = mu + d[t] with integer mu in [-64, 64] and integer deviations d in [-m, m], every value an integer
bf16 holds exactly (|x| <= 256); components, coefficients and weights are small integers as well.  Then
  * the centred operand x - mu of the Gram / projection / components is an integer fp32 holds exactly,
  * every fp32 partial sum of an MFMA chain (Gram, projection: one slice of ``slice_len`` pixels, folded every 512 pixels into a
    second fp32 accumulator up to 4 channels) and of an fmaf chain (components: T terms, reconstruct: K terms + mu) is an integer
    below 2^24 IN ANY ORDER -- ``budget`` asserts that per launch from the case's own shape, slice length and data --,
  * the fp64 sum over the slices is exact, and Z, stored as fp32, stays below 2^24 in total,
  * the mean is one IEEE fp64 division of an exact integer sum followed by one rounding to fp32, whatever T is.
There is no fast-math in the build, so every output must EQUAL the float64 reference: a dropped pixel at the end of a slice, a
chunk lost at the 512-pixel fold, a slice boundary off by one chunk, an unmirrored tile, a padding channel or padding column read,
a tie broken to the wrong side or two strides exchanged give another integer (``test_eof_exact_cpu`` shows that each of these
faults changes expected bits of the case that exists for it).  The assumption -- an integer f32 MFMA chain below 2^24 returns that
integer -- is checked first on the device by the smallest Gram case (``FIRST``) in both data kinds.

Data kinds.  "zero-sum": signed deviations whose sum over t is zero at every pixel (negated pairs in an order shuffled per pixel,
plus a triple a, b, -(a + b) when T is odd), so the supplied mu IS the true mean; every Gram case of this kind also runs about an
arbitrary integer offset field (the kernel does not care whether mu is the mean).  "signed": independent deviations (the mean is no
integer).  "one-sign": deviations in the upper quarter of [0, m], so that the sums themselves come close to the budget (signed data
stays near its square root).

Calling the kernels.  HipOps.eof_gram / eof_project choose nslice themselves (64-pixel slices at every small shape), so the runners
call dg_eof_gram / dg_eof_project directly with the case's nslice and a workspace of their own (NaN-filled: a slab that is not
written, e.g. of an empty trailing slice, shows) and then once through the wrapper: equal bits, integer partial sums commute.
Destinations (mu, G, Z, E, amax, out) and the workspace sit between guards (tests/conv_ref.py ``Dest``).

Contract notes.  include/downgan_hip.h asks for zeros in the columns of A beyond K; the kernel never lets them reach E or amax, and
the table pins that by filling them with NaN.  An all-zero row keeps its sign and leaves the key of position 0 (value bits 0).
"""
from __future__ import annotations

import ctypes as ct
import dataclasses
import functools
import math

import numpy as np
import torch

from downgan_amd._lib import check
from downgan_amd.ops import _ptr
from tests.conv_ref import SENTINEL, Dest, assert_bits_at
from tests.elementwise_ref import INT_LIMIT, assert_bits

MAG_MU = 64             # |mu| <= 64
MAG_X = 256             # every field value is an integer bf16 holds exactly
MAG_D = MAG_X - MAG_MU  # deviations at most
OFFSET = 2              # the "offset" variant of a Gram case centres about mu + o, |o| <= OFFSET
MAG_A = 3               # weights A of the components
MAG_E = 31              # components E of projection and reconstruct
MAG_Z = 1 << 16         # ceiling of a coefficient's magnitude where the budget would allow more
PAD_C = 16              # channels of the padded NHWC store
P0 = 37 * 41            # 1517 pixels: ragged against 64, 256 and every chunk width
FORMATS = ("nchw_f32", "nhwc_f32", "nchw_bf16", "nhwc_bf16_pad")
E_LAYOUTS = ("ckp", "kcp", "shared")     # [C, K, P]; the reference's [K, C, P]; one [K, P] for every channel (ld_c = 0)


# ---------------------------------------------------------------------------------------------------------------- data
def zero_sum(rng, T, shape, m):
    """int64 [T, *shape] in [-m, m] whose sum over t is zero everywhere: negated pairs, a triple a, b, -(a + b) when T is odd, in an
    order shuffled per position."""
    n = int(np.prod(shape))
    d = np.zeros((T, n), dtype=np.int64)
    t0 = 0
    if T % 2:
        assert T >= 3
        a, b = rng.integers(-(m // 2), m // 2 + 1, (2, n))
        d[0], d[1], d[2] = a, b, -(a + b)
        t0 = 3
    h = (T - t0) // 2
    v = rng.integers(-m, m + 1, (h, n))
    d[t0:t0 + h], d[t0 + h:] = v, -v
    d = np.take_along_axis(d, np.argsort(rng.random((T, n)), axis=0), axis=0)
    assert not d.sum(0).any() and np.abs(d).max() <= m
    return d.reshape((T,) + tuple(shape))


@functools.lru_cache(maxsize=None)
def fields(seed, T, Cn, P, m, kind):
    """(x [T, C, P], mu [C, P]) int64, x = mu + d."""
    rng = np.random.default_rng(seed)
    mu = rng.integers(-MAG_MU, MAG_MU + 1, (Cn, P))
    assert 1 <= m <= MAG_D
    if kind == "zero-sum":
        d = zero_sum(rng, T, (Cn, P), m)
    elif kind == "signed":
        d = rng.integers(-m, m + 1, (T, Cn, P))
    else:
        assert kind == "one-sign", kind
        d = rng.integers(m - m // 4, m + 1, (T, Cn, P))
    x = mu[None] + d
    assert np.abs(x).max() <= MAG_X
    return x, mu


def ints(seed, shape, mag):
    return np.random.default_rng(seed).integers(-mag, mag + 1, tuple(shape))


def host_store(x, fmt):
    """The host tensor a format holds for x [T, C, P]: NCHW [T, C, P], or the [T, 1, P, c] store (c = C, or PAD_C channels of which
    the padding holds NaN), every value exactly."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    v = t.to(torch.bfloat16 if "bf16" in fmt else torch.float32)
    assert torch.equal(v.double(), t.double()), "a field value is not exact in the format"
    if fmt.startswith("nchw"):
        return v.contiguous()
    T, Cn, P = x.shape
    nh = v.permute(0, 2, 1).reshape(T, 1, P, Cn)
    if fmt.endswith("_pad"):
        pad = torch.full((T, 1, P, PAD_C), float("nan"), dtype=v.dtype)
        pad[..., :Cn] = nh
        return pad
    return nh.contiguous()


def seen(store, fmt, Cn, c0=0):
    """float64 [T, C, P] of the values a kernel reads from ``store`` through the descriptor (channels c0 .. c0 + C of an NHWC store;
    c0 != 0 is the "reads a padding channel" fault)."""
    if fmt.startswith("nchw"):
        return store.double().numpy()
    return store[:, 0, :, c0:c0 + Cn].permute(0, 2, 1).double().numpy()


def stage(ops, x, fmt):
    """(device tensor to keep alive, dg_eof_fields) of x [T, C, P] in ``fmt``."""
    src = host_store(x, fmt).to(ops.device)
    if fmt.startswith("nchw"):
        return src, ops.eof_fields(src)
    T, _, P, c = src.shape
    src = src.contiguous().as_strided((T, 1, P, c), (P * c, P * c, c, 1))    # dense strides spelled out for the size-1 dimensions too
    return src, ops.eof_fields(src, nhwc=True, channels=x.shape[1])


def e_store(E, layout):
    """(host fp32 tensor, ld_k, ld_c) holding the logical components E [C, K, P] in ``layout``."""
    Cn, K, P = E.shape
    t = torch.from_numpy(np.ascontiguousarray(E)).float()
    if layout == "ckp":
        return t.contiguous(), P, K * P
    if layout == "kcp":
        return t.permute(1, 0, 2).contiguous(), Cn * P, P
    assert layout == "shared" and all(np.array_equal(E[0], E[c]) for c in range(Cn))
    return t[0].contiguous(), P, 0


def e_read(store, K, Cn, P, ld_k, ld_c):
    """float64 [C, K, P] a kernel reads from the flat ``store`` at E + k ld_k + c ld_c + p (indices wrap, so that exchanged strides
    -- a fault -- still read something)."""
    flat = store.reshape(-1).double().numpy()
    idx = (np.arange(Cn)[:, None, None] * ld_c + np.arange(K)[None, :, None] * ld_k + np.arange(P)[None, None, :]) % flat.size
    return flat[idx]


# ---------------------------------------------------------------------------------------------------------------- references
def ref_mean(x):
    """float32(float64 sum / T): the sum of integers is exact, the division and the narrowing are IEEE."""
    s = np.asarray(x, dtype=np.float64).sum(0)
    return (s / np.float64(x.shape[0])).astype(np.float32)


def ref_gram(x, mu):
    """float64 [C, T, T]: G[c, i, j] = sum_p (x[i, c, p] - mu[c, p]) (x[j, c, p] - mu[c, p]) about the SUPPLIED mu."""
    d = np.asarray(x, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[None]
    d = d.transpose(1, 0, 2)
    return d @ d.transpose(0, 2, 1)


def ref_project(y, m, E):
    """float64 [B, C, K]: Z[b, c, k] = sum_p (y[b, c, p] - m[c, p]) E[c, k, p]; m may be None."""
    d = np.asarray(y, dtype=np.float64)
    if m is not None:
        d = d - np.asarray(m, dtype=np.float64)[None]
    return (d.transpose(1, 0, 2) @ np.asarray(E, dtype=np.float64).transpose(0, 2, 1)).transpose(1, 0, 2)


def amax_word(value, p):
    """The int64 word dg_eof_components + dg_eof_flip leave for a row whose entry of largest magnitude is ``value`` at ``p``."""
    b = int(np.float32(abs(float(value))).view(np.uint32))
    w = (b << 32) | (0xffffffff - int(p)) | ((1 << 63) if value < 0 else 0)
    return w - (1 << 64) if w >> 63 else w


def ref_components(x, mu, A, tie_highest=False):
    """(E float32 [C, K, P] after the sign rule, amax int64 [C, K]).  E[c, k, p] = sum_t A[c, t, k] (x[t, c, p] - mu[c, p]); the entry
    of largest magnitude of every row, the LOWEST p on ties, becomes positive (``tie_highest``: the fault of taking the highest)."""
    d = np.asarray(x, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[None]
    E = np.asarray(A, dtype=np.float64).transpose(0, 2, 1) @ d.transpose(1, 0, 2)
    E = E + 0.0                                             # integer sums: no negative zero before the flip
    Cn, K, P = E.shape
    a = np.abs(E)
    p = P - 1 - np.argmax(a[..., ::-1], axis=2) if tie_highest else np.argmax(a, axis=2)
    v = np.take_along_axis(E, p[..., None], axis=2)[..., 0]
    words = np.array([[amax_word(v[c, k], p[c, k]) for k in range(K)] for c in range(Cn)], dtype=np.int64)
    E = np.where((v < 0)[..., None], E * -1.0, E)           # a flipped row's zeros become -0.0, as -x does on the device
    return E.astype(np.float32), words


def ref_reconstruct(Z, E, mu):
    """float64 [B, C, P]: out[b, c, p] = sum_k Z[b, c, k] E[c, k, p] (+ mu[c, p]); mu may be None."""
    out = (np.asarray(Z, dtype=np.float64).transpose(1, 0, 2) @ np.asarray(E, dtype=np.float64)).transpose(1, 0, 2)
    return out if mu is None else out + np.asarray(mu, dtype=np.float64)[None]


def f32_exact(v, what):
    r = np.asarray(v).astype(np.float32)
    assert np.array_equal(r.astype(np.float64), np.asarray(v, dtype=np.float64)), f"{what}: the reference is not exact in fp32"
    return r


# ---------------------------------------------------------------------------------------------------------------- budgets
def slice_len(P, nslice):
    """launch_xyt's slice length: ceil(ceil(P / 64) / nslice) * 64 pixels."""
    c64 = -(-P // 64)
    assert 1 <= nslice <= c64, (P, nslice)
    return -(-c64 // nslice) * 64


def kp_of(Cn):
    """Pixels per staged chunk of eof_xyt_kernel<NC>."""
    return 64 if Cn == 1 else 32 if Cn == 2 else 16 if Cn <= 4 else 8


def chain_budget(what, terms, mag_a, mag_b, addend=0):
    """terms * |a| * |b| + addend < 2^24: every fp32 partial sum of the chain, in any order, is an integer fp32 holds."""
    top = int(terms) * int(mag_a) * int(mag_b) + int(addend)
    assert top < INT_LIMIT, f"{what}: partial sums reach {top} >= 2^24: fp32 would round"
    return top


# ---------------------------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    kind: str                 # "mean", "gram", "project", "components", "signrule", "reconstruct"
    T: int                    # fields (mean, gram, components) or batch B (project, reconstruct)
    C: int
    P: int
    K: int = 0
    nslice: int = 0
    fmt: str = "nchw_f32"
    data: str = "zero-sum"
    layout: str = "ckp"
    centred: bool = True      # project: m given; reconstruct: mu given

    @property
    def seed(self):
        return sum((i + 1) * ord(ch) for i, ch in enumerate(self.id))


def _isqrt_budget(sl):
    return math.isqrt((INT_LIMIT - 1) // sl)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Host inputs of a case (numpy int64 / float arrays), built once."""
    k, T, Cn, P, K = case.kind, case.T, case.C, case.P, case.K
    if k == "mean":
        x, _ = fields(case.seed, T, Cn, P, MAG_D, case.data)
        return dict(x=x)
    if k == "gram":
        sl = slice_len(P, case.nslice)
        if case.data == "one-sign":
            x, mu = fields(case.seed, T, Cn, P, min(_isqrt_budget(sl), MAG_D), "one-sign")
            return dict(x=x, mus=(("offset", mu),))
        x, mu = fields(case.seed, T, Cn, P, min(_isqrt_budget(sl) - OFFSET, MAG_D), "zero-sum")
        assert np.array_equal(ref_mean(x), mu.astype(np.float32)), "zero-sum data: mu is the true mean"
        return dict(x=x, mus=(("true-mean", mu), ("offset", mu + ints(case.seed + 1, mu.shape, OFFSET))))
    if k == "project":
        y, mu = fields(case.seed, T, Cn, P, MAG_D, "signed")
        if case.layout == "shared":
            E = np.broadcast_to(ints(case.seed + 2, (1, K, P), MAG_E), (Cn, K, P)).copy()
        else:
            E = ints(case.seed + 2, (Cn, K, P), MAG_E)
        return dict(y=y, m=mu if case.centred else None, E=E)
    if k == "components":
        x, mu = fields(case.seed, T, Cn, P, MAG_D, "signed")
        return dict(x=x, mu=mu, A=ints(case.seed + 3, (Cn, T, K), MAG_A))
    if k == "signrule":
        return signrule_inputs(case)
    assert k == "reconstruct", k
    mz = min((INT_LIMIT - 1 - MAG_MU) // (K * MAG_E), MAG_Z)
    return dict(Z=ints(case.seed + 4, (T, Cn, K), mz), E=ints(case.seed + 5, (Cn, K, P), MAG_E),
                mu=ints(case.seed + 6, (Cn, P), MAG_MU) if case.centred else None)


# constructed rows of the sign rule: (name, ((pixel, sign of the planted entry of largest magnitude), ...), row is flipped).
# Workgroups hold 256 pixels, waves 64: 3 and 300 lie in different workgroups, 10 and 20 in one wave, 130 and 250 in two waves of
# one workgroup, 1516 is the last pixel of the last, partial workgroup (P0 = 1517).
SIGN_ROWS = (("tie-p3-neg-p300-pos", ((3, -1), (300, +1)), True),
             ("tie-p3-pos-p300-neg", ((3, +1), (300, -1)), False),
             ("tie-inside-one-wave", ((10, -1), (20, +1)), True),
             ("tie-across-waves", ((130, +1), (250, -1)), False),
             ("max-in-last-workgroup", ((P0 - 1, -1),), True),
             ("all-zero-row", (), False))
SIGN_MAX = 100


def signrule_inputs(case):
    """T = 5 fields whose deviation rows ARE the constructed rows (A's column k is the unit vector e_k, the sixth column is zero);
    channel 1 takes the same rows through -e_k, the mirror image of every row, so that its flips are the opposite ones."""
    assert (case.T, case.P, case.K) == (5, P0, len(SIGN_ROWS)) and case.C == 2
    rng = np.random.default_rng(case.seed)
    mu = rng.integers(-MAG_MU, MAG_MU + 1, (2, P0))
    d = rng.integers(-(SIGN_MAX - 1), SIGN_MAX, (5, 2, P0))
    for t, (_, plants, _) in enumerate(SIGN_ROWS[:5]):
        for p, s in plants:
            d[t, :, p] = s * SIGN_MAX
    A = np.zeros((2, 5, case.K), dtype=np.int64)
    for k in range(5):
        A[0, k, k], A[1, k, k] = 1, -1
    return dict(x=mu[None] + d, mu=mu, A=A)


def signrule_expected(case):
    """What the constructed rows must give, stated without ``ref_components``: (flipped [C, K] bool, position [C, K])."""
    flip = np.array([[f for _, _, f in SIGN_ROWS], [bool(pl) and not f for _, pl, f in SIGN_ROWS]])
    pos = np.array([[pl[0][0] if pl else 0 for _, pl, _ in SIGN_ROWS]] * 2)
    return flip, pos


def budget(case):
    """Assert the case's integer budget from its own shape, slice length and data; returns the largest sum a chain can reach."""
    inp = inputs(case)
    if case.kind == "mean":
        return int(np.abs(inp["x"]).max()) * case.T              # fp64 sums: no budget to speak of
    if case.kind == "gram":
        sl = slice_len(case.P, case.nslice)
        return max(chain_budget(f"{case.id} {name}", sl, np.abs(inp["x"] - mu[None]).max(), np.abs(inp["x"] - mu[None]).max())
                   for name, mu in inp["mus"])
    if case.kind == "project":
        ma = np.abs(inp["y"] - (0 if inp["m"] is None else inp["m"][None])).max()
        mb = np.abs(inp["E"]).max()
        chain_budget(f"{case.id} slice", slice_len(case.P, case.nslice), ma, mb)
        return chain_budget(f"{case.id} total (Z is fp32)", case.P, ma, mb)
    if case.kind in ("components", "signrule"):
        return chain_budget(case.id, case.T, np.abs(inp["A"]).max(), np.abs(inp["x"] - inp["mu"][None]).max())
    mm = 0 if inp["mu"] is None else np.abs(inp["mu"]).max()
    return chain_budget(case.id, case.K, np.abs(inp["Z"]).max(), np.abs(inp["E"]).max(), mm)


def covers(case):
    """The branches of csrc/eof.hip a case reaches, restated from the kernels' own structure (tests/test_eof_exact_cpu.py asserts
    that the table reaches every one)."""
    tags = {f"kind={case.kind}", f"fmt={case.fmt}"}
    if case.kind in ("gram", "project"):
        Cn, P, ns = case.C, case.P, case.nslice
        sl, kp = slice_len(P, ns), kp_of(Cn)
        two = Cn <= 4
        tags |= {f"NC={Cn}", "chain=two-level" if two else "chain=one-level", f"row-tiles={-(-case.T // 64)}"}
        if kp * Cn < 64:
            tags.add("lane-guard")
        lens = [max(0, min(P, (s + 1) * sl) - s * sl) for s in range(ns)]       # pixels of each slice
        folds = max(-(-n // kp) * kp // 512 for n in lens) if two else 0          # the chunk loop folds at every 512th pixel
        if folds:
            tags |= {"fold", f"folds={folds}"}
        if any(n > 512 and n % kp for n in lens):
            tags.add("ragged-chunk-in-long-slice")
        if any(n == 0 for n in lens):
            tags.add("empty-slice")
        if sl == 64:
            tags.add("64-pixel-slices")
    if case.kind == "project":
        tags |= {f"E={case.layout}", "m=given" if case.centred else "m=None", f"K={case.K}"}
        if "bf16" in case.fmt:
            tags.add("mixed-dtype")
    if case.kind in ("components", "reconstruct", "signrule"):
        tags.add(f"{'components' if case.kind != 'reconstruct' else 'reconstruct'}-KB={-(-case.K // 16) * 16}")
        if case.K % 16:
            tags.add("NaN-padding-columns" if case.kind != "reconstruct" else "K-below-KB")
    if case.kind == "reconstruct":
        tags |= {f"E={case.layout}", "mu=given" if case.centred else "mu=None"}
    if case.kind == "gram" and case.data == "one-sign":
        tags.add("one-sign")
    if case.fmt.endswith("_pad"):
        tags.add("NaN-padding-channels")
    if case.kind == "signrule":
        tags |= {f"sign-row={name}" for name, _, _ in SIGN_ROWS}
    return tags


# ---------------------------------------------------------------------------------------------------------------- runners
def _dest(ops, shape, dtype):
    return Dest(ops, torch.full(tuple(shape), SENTINEL, dtype=dtype))


def _dev(ops, a, dtype=torch.float32):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    assert torch.equal(t.double(), torch.from_numpy(np.ascontiguousarray(a)).double())
    return t.to(ops.device)


def _workspace(ops, floats):
    return Dest(ops, torch.full((int(floats),), float("nan"), dtype=torch.float32))


def run_mean(ops, case):
    x = inputs(case)["x"]
    src, f = stage(ops, x, case.fmt)
    mu = _dest(ops, (case.C, case.P), torch.float32)
    ops.eof_mean(f, mu.dev)
    assert_bits_at(mu.result(), torch.from_numpy(ref_mean(x)), case.id)
    mu.check(case.id)


def gram_explicit(ops, f, mu_d, nslice, G):
    """dg_eof_gram with an explicit nslice and a guarded, NaN-filled workspace of the call's own."""
    nb = -(-f.T // 64)
    ws = _workspace(ops, nslice * (nb * (nb + 1) // 2) * f.C * 4096)
    check(ops.lib.dg_eof_gram(ct.byref(f), _ptr(mu_d), nslice, _ptr(ws.dev), _ptr(G), ops._stream()), "dg_eof_gram")
    torch.cuda.synchronize()
    ws.check("the Gram workspace")


def run_gram(ops, case, wrapper=True):
    inp = inputs(case)
    budget(case)
    x = inp["x"]
    src, f = stage(ops, x, case.fmt)
    for name, mu in inp["mus"]:
        what = f"{case.id} {name}"
        ref = torch.from_numpy(ref_gram(x, mu))
        mu_d = _dev(ops, mu)
        G = _dest(ops, (case.C, case.T, case.T), torch.float64)
        gram_explicit(ops, f, mu_d, case.nslice, G.dev)
        got = G.result()
        assert_bits_at(got, ref, what)
        assert_bits(got, got.transpose(1, 2).contiguous(), f"{what}: the mirror G[c, i, j] == G[c, j, i]")
        G.check(what)
        if wrapper:
            Gw = _dest(ops, (case.C, case.T, case.T), torch.float64)
            ops.eof_gram(f, mu_d, Gw.dev)
            assert_bits_at(Gw.result(), ref, f"{what} through HipOps.eof_gram")
            Gw.check(what)


def project_explicit(ops, f, m_d, E_d, K, ld_k, ld_c, nslice, Z):
    ws = _workspace(ops, nslice * -(-f.T // 64) * f.C * 4096)
    check(ops.lib.dg_eof_project(ct.byref(f), _ptr(m_d), _ptr(E_d), K, ld_k, ld_c, nslice, _ptr(ws.dev), _ptr(Z), ops._stream()),
          "dg_eof_project")
    torch.cuda.synchronize()
    ws.check("the projection workspace")


def run_project(ops, case, wrapper=True):
    inp = inputs(case)
    budget(case)
    y, m, E = inp["y"], inp["m"], inp["E"]
    src, f = stage(ops, y, case.fmt)
    ref = torch.from_numpy(f32_exact(ref_project(y, m, E), case.id))
    store, ld_k, ld_c = e_store(E, case.layout)
    E_d, m_d = store.to(ops.device), _dev(ops, m)
    Z = _dest(ops, (case.T, case.C, case.K), torch.float32)
    project_explicit(ops, f, m_d, E_d, case.K, ld_k, ld_c, case.nslice, Z.dev)
    assert_bits_at(Z.result(), ref, case.id)
    Z.check(case.id)
    if wrapper:
        Zw = _dest(ops, (case.T, case.C, case.K), torch.float32)
        ops.eof_project(f, m_d, E_d, case.K, ld_k, ld_c, Zw.dev)
        assert_bits_at(Zw.result(), ref, f"{case.id} through HipOps.eof_project")
        Zw.check(case.id)


def run_components(ops, case):
    inp = inputs(case)
    budget(case)
    x, mu, A = inp["x"], inp["mu"], inp["A"]
    K, KB = case.K, -(-case.K // 16) * 16
    src, f = stage(ops, x, case.fmt)
    Ap = torch.full((case.C, case.T, KB), float("nan"), dtype=torch.float32)      # padding columns must reach nothing
    Ap[..., :K] = torch.from_numpy(A).float()
    E = _dest(ops, (case.C, K, case.P), torch.float32)
    amax = _dest(ops, (case.C, K), torch.int64)
    ops.eof_components(f, _dev(ops, mu), Ap.to(ops.device), K, E.dev, amax.dev)
    E_ref, words = ref_components(x, mu, A)
    if case.kind == "signrule":
        flip, pos = signrule_expected(case)
        want = np.array([[amax_word((-1 if flip[c, k] else 1) * (SIGN_MAX if SIGN_ROWS[k][1] else 0), pos[c, k])
                          for k in range(K)] for c in range(2)], dtype=np.int64)
        assert np.array_equal(words, want), "the reference disagrees with the constructed rows"
    assert_bits_at(amax.result(), torch.from_numpy(words), f"{case.id}: amax")
    assert_bits_at(E.result(), torch.from_numpy(E_ref), f"{case.id}: E")
    E.check(case.id)
    amax.check(case.id)


def run_reconstruct(ops, case):
    inp = inputs(case)
    budget(case)
    Z, E, mu = inp["Z"], inp["E"], inp["mu"]
    ref = torch.from_numpy(f32_exact(ref_reconstruct(Z, E, mu), case.id))
    store, ld_k, ld_c = e_store(E, case.layout)
    out = _dest(ops, (case.T, case.C, case.P), torch.float32)
    ops.eof_reconstruct(_dev(ops, Z), store.to(ops.device), ld_k, ld_c, case.P, _dev(ops, mu), out.dev)
    assert_bits_at(out.result(), ref, case.id)
    out.check(case.id)


RUNNERS = {"mean": run_mean, "gram": run_gram, "project": run_project, "components": run_components, "signrule": run_components,
           "reconstruct": run_reconstruct}


def run_case(ops, case):
    return RUNNERS[case.kind](ops, case)


# ---------------------------------------------------------------------------------------------------------------- the table
def _gram(T, Cn, P, ns, fmt="nchw_f32", data="zero-sum"):
    cid = f"gram-T{T}-C{Cn}-P{P}-ns{ns}" + ("" if fmt == "nchw_f32" else f"-{fmt}") + ("" if data == "zero-sum" else f"-{data}")
    return Case(cid, "gram", T, Cn, P, nslice=ns, fmt=fmt, data=data)


FIRST = ("gram-T5-C1-P64-ns1", "gram-T5-C1-P64-ns1-one-sign")     # the cases that check the integer-MFMA assumption; run first
CASES = [_gram(5, 1, 64, 1), _gram(5, 1, 64, 1, data="one-sign")]
# one slice of 1536 pixels (the 512-pixel fold fires three times, the last chunk is ragged); 320-pixel slices; 256-pixel slices of
# which the 7th is empty; 64-pixel slices
CASES += [_gram(77, 2, P0, ns) for ns in (1, 5, 7, 24)]
# one tile; a second row tile of one row; three row tiles (six upper tiles)
CASES += [_gram(T, 2, P0, 3) for T in (64, 65, 130)]
# every other channel count: NC = 3, 5, 6, 7 leave lanes of the staging wave idle, NC >= 5 takes the one-level chain
CASES += [_gram(33, Cn, P0, ns) for Cn in (1, 3, 4, 5, 6, 7, 8) for ns in (1, 3)]
# layouts: NCHW fp32, the resident feed's NHWC fp32, the padded bf16 store whose padding channels hold NaN
# (C = 3 and 5 in NCHW fp32 stand in the line above)
CASES += [_gram(33, Cn, P0, 3, fmt=fmt) for Cn in (2, 3, 5) for fmt in ("nchw_f32", "nhwc_f32", "nhwc_bf16_pad")
          if (Cn, fmt) not in ((3, "nchw_f32"), (5, "nchw_f32"))]
# one-sign: each slab stays below 2^24 and the diagonal total lies above it (the slice sum is fp64)
ONE_SIGN = _gram(33, 2, 3000, 2, data="one-sign")
CASES.append(ONE_SIGN)

# mean: a mean that is no integer (T = 5, 77) and one that is exact (T = 64), every format
for _i, (_T, _C) in enumerate((T, Cn) for T in (5, 64, 77) for Cn in (1, 2, 3)):
    for _fmt in (FORMATS[_i % 4], FORMATS[(_i + 2) % 4]):
        CASES.append(Case(f"mean-T{_T}-C{_C}-{_fmt}", "mean", _T, _C, P0, fmt=_fmt, data="signed"))

# projection: every (B, K, C, y format) with the E layout, m and nslice rotating through their values
P_FMTS = ("nchw_f32", "nhwc_f32", "nhwc_bf16_pad")
P_NSLICE = (1, 4, -(-P0 // 64))
for _ib, _B in enumerate((3, 70)):
    for _ik, _K in enumerate((1, 13, 16, 17, 33, 64)):
        for _ic, _C in enumerate((1, 2, 5)):
            for _if, _fmt in enumerate(P_FMTS):
                _lay = E_LAYOUTS[(_ik + _ic + _if) % 3]
                _cen = bool((_ik + _if + _ib + _ic // 2) % 2)
                _ns = P_NSLICE[(_ik + _ib + _if + _ic) % 3]
                CASES.append(Case(f"project-B{_B}-K{_K}-C{_C}-{_fmt}-E{_lay}-m{int(_cen)}-ns{_ns}", "project", _B, _C, P0, K=_K,
                                  nslice=_ns, fmt=_fmt, data="signed", layout=_lay, centred=_cen))

# components: every (T, K, C) with the format rotating; the constructed sign-rule rows in fp32 and in the padded bf16 store
for _it, _T in enumerate((5, 77)):
    for _ik, _K in enumerate((1, 16, 17, 48, 49, 64)):
        for _ic, _C in enumerate((1, 2, 3)):
            _fmt = FORMATS[(_it + _ik + _ic) % 4]
            CASES.append(Case(f"components-T{_T}-K{_K}-C{_C}-{_fmt}", "components", _T, _C, P0, K=_K, fmt=_fmt, data="signed"))
SIGNRULE = [Case(f"signrule-{_fmt}", "signrule", 5, 2, P0, K=len(SIGN_ROWS), fmt=_fmt) for _fmt in ("nchw_f32", "nhwc_bf16_pad")]
CASES += SIGNRULE

# reconstruct: every (K, C, P) with B, the E layout and mu rotating
for _ik, _K in enumerate((1, 16, 17, 48, 49, 64)):
    for _ic, _C in enumerate((1, 2, 5)):
        for _ip, _P in enumerate((255, 256, P0)):
            _B = (1, 5)[(_ik + _ic + _ip) % 2]
            _lay = E_LAYOUTS[(_ik + _ip + _ic // 2) % 2]
            _cen = bool((_ik // 2 + _ic + _ip) % 2)
            CASES.append(Case(f"reconstruct-B{_B}-K{_K}-C{_C}-P{_P}-E{_lay}-mu{int(_cen)}", "reconstruct", _B, _C, _P, K=_K,
                              layout=_lay, centred=_cen))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
assert all(i in BY_ID for i in FIRST)
