"""Fractions skill score without a GPU: spec validation, argument checks that fire before any library call, the ABI surface
and struct layout, the host-side reference of the library (dg_fss_host, dg_fss_bound) against an integer numpy oracle (itself
checked against a brute-force double loop), the known answers of the definition through ``FssResult``, the headroom rules of
``FractionsSkill`` (drain, chunks, limb all-reduce), and the trainer's opt-in hook on the emulated ops (a test-local op class
adds a numpy ``fss`` under the usual make_ops patch), in one process, over 2 gloo ranks, and in the frequency-separation
trainer.  Every comparison of sums is integer equality."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from downgan_amd import _lib, fss, histograms
from downgan_amd.fss import FractionsSkill, FssResult, FssSpec

from .test_gridstats_cpu import _no_library
from .test_histograms_cpu import transform_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------------------------------------------- the definition in numpy
def masks_ref(spec, x):
    """x float32 [T, C, H, W] -> bool [nout, K, T, H, W]: y > thr as an fp32 compare (NaN false, +inf true, equality false)."""
    T, Cn, H, W = x.shape
    y = transform_ref(spec, np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(Cn, -1)).reshape(spec.nout, T, H, W)
    with np.errstate(invalid="ignore"):
        return y[:, None] > spec.thresholds.astype(F32)[:, :, None, None, None]


def counts_ref(m, n):
    """m bool [..., H, W] -> int64 [..., H, W]: the set pixels in the n x n window about each pixel, zero outside the grid, from
    a summed-area table by cumsum in int64."""
    H, W = m.shape[-2:]
    S = np.zeros(m.shape[:-2] + (H + 1, W + 1), dtype=np.int64)
    S[..., 1:, 1:] = m.astype(np.int64).cumsum(axis=-2).cumsum(axis=-1)
    r = n // 2
    h0, h1 = np.clip(np.arange(H) - r, 0, H)[:, None], np.clip(np.arange(H) + r + 1, 0, H)[:, None]
    w0, w1 = np.clip(np.arange(W) - r, 0, W)[None, :], np.clip(np.arange(W) + r + 1, 0, W)[None, :]
    return S[..., h1, w1] - S[..., h0, w1] - S[..., h1, w0] + S[..., h0, w0]


def counts_brute(m, n):
    """The same by the definition's double loop (one H x W mask)."""
    H, W = m.shape
    r = n // 2
    out = np.zeros((H, W), dtype=np.int64)
    for h in range(H):
        for w in range(W):
            out[h, w] = sum(int(m[i, j]) for i in range(h - r, h + r + 1) for j in range(w - r, w + r + 1) if 0 <= i < H and 0 <= j < W)
    return out


def fss_ref(spec, a, b):
    """a, b float32 [T, C, H, W] (the values read) -> (sums [nout, K, S, 3], rates [nout, K, 2], per_field [T, nout, K, S, 3]) as
    arrays of Python integers.  One field adds at most 2^60 here, so the int64 field sums are exact; fields are added as
    Python integers."""
    T = a.shape[0]
    ma, mb = masks_ref(spec, a), masks_ref(spec, b)
    per = np.zeros((T, spec.nout, spec.K, spec.S, 3), dtype=object)
    for s, n in enumerate(spec.scales):
        ca, cb = counts_ref(ma, n), counts_ref(mb, n)
        d = ca - cb
        for e, v in enumerate(((d * d).sum(axis=(-2, -1)), (ca * ca).sum(axis=(-2, -1)), (cb * cb).sum(axis=(-2, -1)))):
            per[:, :, :, s, e] = v.transpose(2, 0, 1).astype(object)
    rates = np.stack([ma.sum(axis=(2, 3, 4)), mb.sum(axis=(2, 3, 4))], axis=-1).astype(object)
    return per.sum(axis=0), rates, per


def ints(a):
    return [int(v) for v in np.asarray(a, dtype=object).reshape(-1)]


def host_sums(spec, a, b):
    """(sums, rates) int64 arrays of the library's host reference over the field pairs of a, b float32 [T, C, H, W]."""
    T, Cn, H, W = a.shape
    sums, rates = np.zeros((spec.nout, spec.K, spec.S, 3), np.int64), np.zeros((spec.nout, spec.K, 2), np.int64)
    s = spec.struct()
    for t in range(T):
        xa, xb = np.ascontiguousarray(a[t], dtype=F32), np.ascontiguousarray(b[t], dtype=F32)
        _lib.check(_lib.lib().dg_fss_host(C.byref(s), xa.ctypes.data, xb.ctypes.data, Cn, H, W, sums.ctypes.data, rates.ctypes.data),
                   "dg_fss_host")
    return sums, rates


def host_result(spec, a, b):
    sums, rates = host_sums(spec, a, b)
    return FssResult(spec, a.shape[2], a.shape[3], sums, rates, a.shape[0])


def test_the_oracle_equals_the_brute_force_definition():
    rng = np.random.default_rng(0)
    for H, W in ((7, 13), (16, 9), (1, 5), (16, 16)):
        m = rng.random((H, W)) < 0.3
        for n in (1, 3, 5, 15, 27, 33):
            np.testing.assert_array_equal(counts_ref(m, n), counts_brute(m, n), err_msg=f"{H} x {W}, n = {n}")
    spec = FssSpec(1, speed=None, thresholds=(0.5,), scales=(1, 3, 7))
    a, b = (rng.random((2, 1, 6, 5)) < 0.4).astype(F32), (rng.random((2, 1, 6, 5)) < 0.4).astype(F32)
    sums, rates, per = fss_ref(spec, a, b)
    for s, n in enumerate(spec.scales):
        ca = np.stack([counts_brute(a[t, 0] > 0.5, n) for t in range(2)])
        cb = np.stack([counts_brute(b[t, 0] > 0.5, n) for t in range(2)])
        assert ints(sums[0, 0, s]) == [int(((ca - cb) ** 2).sum()), int((ca * ca).sum()), int((cb * cb).sum())]
        assert ints(per[1, 0, 0, s]) == [int(((ca[1] - cb[1]) ** 2).sum()), int((ca[1] ** 2).sum()), int((cb[1] ** 2).sum())]
    assert ints(rates) == [int(a.sum()), int(b.sum())]


# ------------------------------------------------------------------------------------------------- spec and argument checks
@pytest.mark.parametrize("kw,match", [
    (dict(C=0), "C <="),
    (dict(C=9), "C <="),
    (dict(C=2.5), "C <="),
    (dict(C=1), "speed"),                                                # the default speed (0, 1) of a 1-channel field
    (dict(C=3, speed=(0, 3)), "speed"),
    (dict(C=2, scale=[1.0]), "scale"),
    (dict(C=2, offset=[0.0, np.nan]), "finite"),
    (dict(C=2, scale=[1e39, 1.0]), "fp32"),
    (dict(C=2, thresholds=()), "1 to 4 thresholds"),
    (dict(C=2, thresholds=(1.0, 2.0, 3.0, 4.0, 5.0)), "1 to 4 thresholds"),
    (dict(C=2, thresholds=[[1.0], [2.0]]), "one list per output"),
    (dict(C=2, thresholds=[[1.0], [2.0], [3.0, 4.0]]), "one length"),
    (dict(C=2, thresholds=(1.0, np.inf)), "finite"),
    (dict(C=2, scales=()), "1 to 8 scales"),
    (dict(C=2, scales=(1, 3, 5, 7, 9, 11, 13, 15, 17)), "1 to 8 scales"),
    (dict(C=2, scales=(1, 4)), "odd"),
    (dict(C=2, scales=(-1, 3)), "odd"),
    (dict(C=2, scales=(1, 4097)), "odd"),
    (dict(C=2, scales=(3, 3)), "increasing"),
    (dict(C=2, scales=(5, 3)), "increasing"),
    (dict(C=2, scales=(1, 3.0)), "integer"),
    (dict(C=2, names=["a", "b"]), "names"),
])
def test_spec_is_checked(monkeypatch, kw, match):
    _no_library(monkeypatch)
    kw = dict(dict(thresholds=(1.0,)), **kw)
    with pytest.raises(ValueError, match=match):
        FssSpec(**kw)


def test_constructors():
    z = FssSpec.zscore(2)
    assert (z.C, z.nout, z.speed, z.K, z.S, z.names) == (2, 3, (0, 1), 2, 8, ["ch0", "ch1", "speed"])
    assert z.thresholds.tolist() == [[1.0, 2.0]] * 3 and z.scales == (1, 3, 5, 9, 17, 33, 65, 129)
    one = FssSpec.zscore(1, thresholds=(0.5,), scales=(1, 4095))
    assert one.speed is None and one.nout == 1 and one.K == 1 and one.scales == (1, 4095)
    stats = {"u10": (0.5, 3.0), "v10": (-0.25, 2.0), "t2m": (280.0, 10.0)}
    p = FssSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [15.0]], scales=(1, 9))
    assert p.speed == (1, 2) and p.names == ["t2m", "u10", "v10", "speed"]
    assert p.scale.tolist() == [10.0, 3.0, 2.0] and p.offset.tolist() == [280.0, 0.5, -0.25]
    assert p.thresholds[:, 0].tolist() == [300.0, 10.0, 10.0, 15.0]
    assert p == FssSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [15.0]], scales=(1, 9))
    assert p != z and p != FssSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [15.0]], scales=(1, 7))
    assert FssSpec(2, thresholds=(0.1,)).thresholds[0, 0] == F32(0.1)            # rounded to fp32
    s = p.struct()
    assert (s.speed_u, s.speed_v, s.nthr, s.nscale) == (1, 2, 1, 2) and list(s.win)[:2] == [1, 9]
    assert s.thr[3][0] == 15.0 and s.scale[2] == 2.0 and s.offset[0] == 280.0
    n = FssSpec(2, speed=None, thresholds=(1.0,)).struct()
    assert (n.speed_u, n.speed_v, n.nthr, n.nscale) == (-1, -1, 1, 8)


@pytest.mark.parametrize("x,kw,err,match", [
    (torch.zeros(2, 3, 8, 8), {}, ValueError, "C = 2"),
    (torch.zeros(2, 9, 8, 8), {}, ValueError, "C <="),
    (torch.zeros(2, 8, 8, 4), {"nhwc": True, "channels": 5}, ValueError, "channels"),
    (torch.zeros(2, 8, 8, 4), {"nhwc": True}, ValueError, "C = 2"),
    (torch.zeros(2, 2, 8, 8, dtype=torch.float64), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 2, 8, 8), np.float32), {}, TypeError, "tensor"),
    (torch.zeros(2, 8, 8), {}, ValueError, "shape"),
    (torch.zeros(0, 2, 8, 8), {}, ValueError, "at least one"),
    (torch.zeros(2, 2, 8, 4), {}, ValueError, "8 x 8 grid"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, x, kw, err, match):
    _no_library(monkeypatch)
    spec = FssSpec.zscore(2)
    good = torch.zeros(2, 2, 8, 8)
    acc = FractionsSkill(spec, 8, 8, device="cpu")
    with pytest.raises(err, match=match):
        acc.add(good, x, nhwc=(False, kw.get("nhwc", False)), channels=kw.get("channels"))
    with pytest.raises(err, match=match):
        acc.add(x, good, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))
    if "grid" not in match:                                               # the one-shot form takes the grid from the fields
        with pytest.raises(err, match=match):
            fss.fss(x, good, spec=spec, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))


def test_accumulator_checks(monkeypatch):
    _no_library(monkeypatch)
    spec = FssSpec.zscore(2)
    x = torch.zeros(2, 2, 8, 8)
    acc = FractionsSkill(spec, 8, 8, device="cpu")
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            acc.add(x, x, n_valid=n)
    with pytest.raises(ValueError, match="differ in length"):
        acc.add(x, torch.zeros(3, 2, 8, 8))
    with pytest.raises(ValueError, match="pair"):
        acc.add(x, x, nhwc=(True, False, True))
    with pytest.raises(TypeError, match="FssSpec"):
        FractionsSkill(histograms.HistSpec.zscore(2), 8, 8, device="cpu")
    with pytest.raises(TypeError, match="FssSpec"):
        fss.fss(x, x, spec=histograms.HistSpec.zscore(2))
    for H, W in ((0, 8), (8, 2049)):
        with pytest.raises(ValueError, match="grid"):
            FractionsSkill(spec, H, W, device="cpu")
    with pytest.raises(ValueError, match="2\\^62"):                      # 2^22 pixels x (2^22)^2
        FractionsSkill(FssSpec.zscore(2, scales=(1, 2049)), 2048, 2048, device="cpu")
    with pytest.raises(ValueError, match="side"):
        FssResult(spec, 8, 8, np.zeros((3, 2, 8, 3), np.int64), np.zeros((3, 2, 2), np.int64), 1).base_rate("both")
    assert acc.fields == 0 and acc._dev_sums.shape == (3, 2, 8, 3) and acc._dev_rates.shape == (3, 2, 2)
    assert acc._dev_sums.dtype == torch.int64 and acc.result().fields == 0


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_fss_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert re.search(r"#define DG_FSS_MAX_THR 4\b", src) and re.search(r"#define DG_FSS_MAX_SCALES 8\b", src)
    assert re.search(r"#define DG_FSS_MAX_SIDE 2048\b", src) and "Fractions skill score (csrc/fss.hip)" in src
    for sym in ("dg_fss_ws_bytes", "dg_fss", "dg_fss_host", "dg_fss_bound"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    assert (_lib.FSS_MAX_THR, _lib.FSS_MAX_SCALES, _lib.FSS_MAX_SIDE) == (fss.THR_MAX, fss.SCALES_MAX, fss.SIDE_MAX) == (4, 8, 2048)
    assert "fss.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()


def test_fss_spec_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.FssSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(dg_fss_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_fss_spec, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("thr_row %zu\\n", sizeof(((dg_fss_spec*)0)->thr[0]));', '  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert int(got["thr_row"]) == 4 * _lib.FSS_MAX_THR


def test_abi_rejects_bad_arguments_without_launching():
    """Every pointer is a made-up address: a call that passed the checks would fault instead of returning a status."""
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    good = FssSpec.zscore(2, scales=(1, 3, 19)).struct()

    def spec(**kw):
        s = FssSpec.zscore(2, scales=(1, 3, 19)).struct()
        for k, v in kw.items():
            if isinstance(v, tuple) and len(v) == 3:
                getattr(s, k)[v[0]][v[1]] = v[2]
            elif isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    ws, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    call = lambda fa, fb, s, H=10, W=10, w=ws, o=out, r=out: lib.dg_fss(fa, fb, H, W, s, w, o, r, None, None)
    g = C.byref(good)
    assert call(f(base=0), f(), g) == -1 and call(f(), f(base=0), g) == -1 and call(None, f(), g) == -1 and call(f(), None, g) == -1
    assert call(f(C=9), f(C=9), g) == -1 and call(f(T=0), f(T=0), g) == -1 and call(f(ld_t=-1), f(), g) == -1
    assert call(f(), f(T=3), g) == -1 and call(f(), f(P=96), g) == -1 and call(f(C=3), f(C=2), g) == -1     # T / C / P differ
    assert call(f(), f(), g, H=10, W=9) == -1 and call(f(), f(), g, H=0, W=10) == -1                          # P != H * W
    assert call(f(P=2049), f(P=2049), g, H=1, W=2049) == -1 and call(f(P=2049), f(P=2049), g, H=2049, W=1) == -1
    assert call(f(), f(), None) == -1
    assert call(f(), f(), g, w=None) == -1 and call(f(), f(), g, o=None) == -1 and call(f(), f(), g, r=None) == -1
    for bad in (dict(nthr=0), dict(nthr=5), dict(nscale=0), dict(nscale=9), dict(speed_u=2), dict(speed_v=-1),
                dict(win=(1, 4)), dict(win=(0, 0)), dict(win=(0, -1)), dict(win=(1, 1)), dict(win=(2, 3)), dict(win=(2, 4097)),
                dict(win=(0, 5)), dict(scale=(1, float("inf"))), dict(offset=(0, float("nan"))),
                dict(thr=(2, 1, float("inf"))), dict(thr=(0, 0, float("nan")))):
        assert call(f(), f(), spec(**bad)) == -1, bad
        assert lib.dg_fss_ws_bytes(f(), 10, 10, spec(**bad)) == 0, bad
    assert call(f(C=1), f(C=1), g) == -1                                 # speed channel 1 of a 1-channel field
    assert call(f(dtype=7), f(), g) == -2 and call(f(), f(dtype=7), g) == -2
    # a scale whose bound is 0 (above 2^62), and T * bound > 2^62
    big = dict(P=2048 * 2048, ld_c=2048 * 2048, ld_t=2 * 2048 * 2048)
    assert call(f(**big), f(**big), spec(win=(2, 2049)), H=2048, W=2048) == -1
    assert lib.dg_fss_ws_bytes(f(**big), 2048, 2048, spec(win=(2, 2049))) == 0
    m = dict(P=1 << 20, ld_c=1 << 20, ld_t=2 << 20)
    assert lib.dg_fss_bound(1024, 1024, 2047) == 1 << 60
    assert call(f(T=5, **m), f(T=5, **m), spec(win=(2, 2047)), H=1024, W=1024) == -1
    assert lib.dg_fss_ws_bytes(f(T=5, **m), 1024, 1024, spec(win=(2, 2047))) == 0
    four = lib.dg_fss_ws_bytes(f(T=4, **m), 1024, 1024, spec(win=(2, 2047)))
    assert four >= 4 * 2 * 3 * 2 * (1 << 20) * 4                          # one uint32 table per (t, series, j, k)
    small = lib.dg_fss_ws_bytes(f(), 10, 10, g)
    assert 4 * 2 * 3 * 2 * 100 * 4 <= small < 1 << 16
    assert lib.dg_fss_ws_bytes(f(C=9), 10, 10, g) == 0 and lib.dg_fss_ws_bytes(f(), 10, 9, g) == 0


def test_bound_is_its_formula():
    lib = _lib.lib()
    for H, W, n in [(7, 13, 1), (7, 13, 5), (7, 13, 27), (16, 9, 15), (1024, 1024, 129), (1024, 1024, 2047), (2048, 2048, 1023),
                    (2048, 1, 4095), (1, 1, 1), (2048, 2048, 1025), (2048, 1024, 1449)]:
        want = H * W * (min(n, H) * min(n, W)) ** 2
        assert fss.bound(H, W, n) == want
        assert lib.dg_fss_bound(H, W, n) == (want if want <= 1 << 62 else 0), (H, W, n)
    assert lib.dg_fss_bound(1024, 1024, 2047) == 1 << 60
    assert lib.dg_fss_bound(2048, 2048, 2049) == 0 and lib.dg_fss_bound(2048, 2048, 1025) == 0     # above 2^62
    assert lib.dg_fss_bound(2048, 2048, 1023) == 2048 * 2048 * 1023 ** 4 > 1 << 61
    for H, W, n in [(0, 5, 1), (5, 0, 1), (2049, 5, 1), (5, 2049, 1), (5, 5, 0), (5, 5, 2), (5, 5, -1), (5, 5, 4097)]:
        assert lib.dg_fss_bound(H, W, n) == 0, (H, W, n)


# ------------------------------------------------------------------------------------------------- the host reference
def special_fields(rng, T, H, W):
    """float32 [T, 2, H, W]: Gaussian values with NaN, +-inf, -0, values equal to a threshold of ``special_spec`` and its fp32
    neighbours, and (3, 4) pairs (speed exactly 5) planted."""
    x = (rng.standard_normal((T, 2, H, W)) * 1.5).astype(F32)
    on = np.array([0.5, 1.0, 5.0], dtype=F32)
    sv = np.concatenate([on, np.nextafter(on, F32(-np.inf)), np.nextafter(on, F32(np.inf)),
                         np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3e38], dtype=F32)])
    flat = x.reshape(T, 2, -1)
    n = flat.shape[2]
    pos = (np.arange(len(sv)) * 7 + 3) % n
    flat[0, 0, pos] = sv
    flat[-1, 1, (pos + 2) % n] = sv[::-1]
    flat[:, 0, n - 1], flat[:, 1, n - 1] = 3.0, 4.0
    return flat.reshape(T, 2, H, W)


def special_spec(scales=(1, 3, 5, 15, 27)):
    return FssSpec(2, thresholds=[[0.5, 1.0], [0.5, 1.0], [5.0, 1.0]], scales=scales)


@pytest.mark.parametrize("H,W", [(7, 13), (16, 9)])
def test_host_reference_equals_the_oracle(H, W):
    rng = np.random.default_rng(H * W)
    a, b = special_fields(rng, 3, H, W), np.roll(special_fields(rng, 3, H, W), 2, axis=3)
    for spec in (special_spec(), FssSpec(2, scale=[3.0, 2.5], offset=[-1.5, 4.0], speed=(1, 0),
                                         thresholds=[[1.5, 0.0], [6.5, 4.0], [6.0, 12.0]], scales=(1, 3, 5, 15, 27))):
        sums, rates, _ = fss_ref(spec, a, b)
        got_s, got_r = host_sums(spec, a, b)
        assert ints(got_s) == ints(sums) and ints(got_r) == ints(rates)
        assert sum(ints(rates)) > 0 and any(v > 0 for v in ints(sums))
    # the speed of a (3, 4) pair equals its threshold 5 and is not counted; +inf is, NaN is not
    one = np.zeros((1, 2, H, W), F32)
    one[0, 0, 0, 0], one[0, 1, 0, 0] = 3.0, 4.0
    one[0, 0, 1, 1], one[0, 0, 2, 2], one[0, 1, 3, 3] = np.inf, np.nan, -0.0
    _, r = host_sums(special_spec(), one, one)
    assert r[:, :, 0].tolist() == [[2, 2], [1, 1], [1, 2]] and np.array_equal(r[:, :, 0], r[:, :, 1])


# ------------------------------------------------------------------------------------------------- known answers
def test_identical_series_score_one_at_every_scale():
    rng = np.random.default_rng(3)
    a = special_fields(rng, 2, 16, 9)
    res = host_result(special_spec(), a, a.copy())
    assert np.all(res.fss() == 1.0) and np.all(res.frequency_bias() == 1.0)
    s = res.sums()
    assert all(int(v) == 0 for v in s[..., 0].reshape(-1)) and ints(s[..., 1]) == ints(s[..., 2])


def test_a_displaced_pixel_scores_one_minus_d_over_n():
    H = W = 48
    spec = FssSpec(1, speed=None, thresholds=(0.5,), scales=(1, 3, 5, 7, 9, 17))
    a, b = np.zeros((1, 1, H, W), F32), np.zeros((1, 1, H, W), F32)
    a[0, 0, 24, 20], b[0, 0, 24, 26] = 1.0, 1.0                          # d = 6, at least 17 / 2 + 6 from every border
    res = host_result(spec, a, b)
    want = [0.0, 0.0, 0.0, 1 / 7, 1 / 3, 11 / 17]
    np.testing.assert_allclose(res.fss()[0, 0], want, rtol=0, atol=1e-15)
    for s, n in enumerate(spec.scales):
        assert ints(res.sums()[0, 0, s]) == [2 * n * n - 2 * n * max(0, n - 6), n * n, n * n]
    assert res.base_rate("real")[0, 0] == res.base_rate("fake")[0, 0] == 1 / (H * W)
    assert res.target()[0, 0] == 0.5 + 0.5 / (H * W) and res.skillful_scale()[0, 0] == 17.0


def test_windows_that_cover_the_grid():
    rng = np.random.default_rng(4)
    H, W, T = 7, 13, 3
    a, b = (rng.random((T, 1, H, W)) < 0.3).astype(F32), (rng.random((T, 1, H, W)) < 0.2).astype(F32)
    spec = FssSpec(1, speed=None, thresholds=(0.5,), scales=(25, 27, 4095))       # n >= 2 max(H, W) - 1
    res = host_result(spec, a, b)
    na, nb = [int(a[t].sum()) for t in range(T)], [int(b[t].sum()) for t in range(T)]
    P = H * W
    want = [sum(P * (x - y) ** 2 for x, y in zip(na, nb)), sum(P * x * x for x in na), sum(P * y * y for y in nb)]
    for s in range(3):
        assert ints(res.sums()[0, 0, s]) == want
    assert ints(res.rates()) == [sum(na), sum(nb)]
    assert res.fss()[0, 0, 0] == 1.0 - want[0] / (want[1] + want[2])


def test_all_ones_against_all_zeros_at_1024_carries_two_to_the_sixty():
    spec = FssSpec(1, speed=None, thresholds=(0.5,), scales=(2047,))
    a, b = np.ones((1, 1, 1024, 1024), F32), np.zeros((1, 1, 1024, 1024), F32)
    res = host_result(spec, a, b)
    assert ints(res.sums()) == [1 << 60, 1 << 60, 0] and ints(res.rates()) == [1 << 20, 0]
    assert res.fss()[0, 0, 0] == 0.0 and res.frequency_bias()[0, 0] == 0.0 and res.base_rate("real")[0, 0] == 1.0


def test_derived_scores_on_hand_made_sums():
    spec = FssSpec(1, speed=None, thresholds=(1.0, 2.0), scales=(1, 3, 5))
    sums = [[[[10, 10, 10], [8, 10, 10], [2, 10, 10]],                   # 0.5, 0.6, 0.9: skilful from n = 3 (target 0.55)
             [[3 << 70, 1 << 70, 2 << 70], [0, 0, 0], [1, 2, 2]]]]       # 0, NaN, 0.75: target 0.5 + 0.8 / 2 = 0.9 never reached
    rates = [[[20, 30], [160, 40]]]
    res = FssResult(spec, 10, 10, sums, rates, 2)
    f = res.fss()
    assert f[0, 0].tolist() == [0.5, 0.6, 0.9] and f[0, 1, 0] == 0.0 and math.isnan(f[0, 1, 1]) and f[0, 1, 2] == 0.75
    assert res.base_rate("real").tolist() == [[0.1, 0.8]] and res.base_rate("fake").tolist() == [[0.15, 0.2]]
    assert res.frequency_bias().tolist() == [[1.5, 0.25]] and res.target().tolist() == [[0.55, 0.9]]
    sk = res.skillful_scale()
    assert sk[0, 0] == 3.0 and math.isnan(sk[0, 1])
    assert ints(res.sums()[0, 1, 0]) == [3 << 70, 1 << 70, 2 << 70] and res.fields == 2
    s = res.summary()
    assert json.loads(json.dumps(s, allow_nan=False)) == s
    assert s["fss"] == [[[0.5, 0.6, 0.9], [0.0, None, 0.75]]] and s["skillful_scale"] == [[3.0, None]]
    assert s["sums"][0][1][0] == [3 << 70, 1 << 70, 2 << 70] and s["rates"] == rates and s["scales"] == [1, 3, 5]
    assert s["channels"] == ["ch0"] and s["fields"] == 2 and s["grid"] == [10, 10] and s["thresholds"] == [[1.0, 2.0]]


def test_all_false_masks_give_nan_and_none():
    spec = FssSpec.zscore(2, thresholds=(50.0,), scales=(1, 5))
    z = np.zeros((2, 2, 7, 13), F32)
    res = host_result(spec, z, z)
    assert np.isnan(res.fss()).all() and np.isnan(res.frequency_bias()).all() and np.isnan(res.skillful_scale()).all()
    assert np.all(res.base_rate("real") == 0) and np.all(res.target() == 0.5)
    s = res.summary()
    json.dumps(s, allow_nan=False)
    assert s["fss"] == [[[None, None]]] * 3 and s["frequency_bias"] == [[None]] * 3 and s["skillful_scale"] == [[None]] * 3


# ------------------------------------------------------------------------------------------------- emulated ops
RECORD = []                  # (real, fake) float32 [T, C, H, W] of every emulated dg_fss call of this process


def fss_emu_ops():
    from oracle.emu_ops import EmuOps

    class FssEmuOps(EmuOps):
        """The emulated ops plus dg_fss's contract in numpy (the oracle above)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            P = t.shape[1] * t.shape[2] if nhwc else t.shape[2] * t.shape[3]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=P)

        def fss_ws_bytes(self, f, H, W, spec):
            return 1

        def fss(self, fa, fb, H, W, s, sums, rates, per_field=None):
            def values(f):
                x = f.t[..., :f.C].permute(0, 3, 1, 2) if f.nhwc else f.t[:, :f.C]
                return x.detach().float().cpu().numpy().copy()
            speed = None if s.speed_u < 0 else (s.speed_u, s.speed_v)
            nout = fa.C + (speed is not None)
            spec = types.SimpleNamespace(nout=nout, K=s.nthr, S=s.nscale, speed=speed, scales=tuple(s.win[:s.nscale]),
                                         scale=np.array(s.scale[:fa.C], F32), offset=np.array(s.offset[:fa.C], F32),
                                         thresholds=np.array([list(s.thr[j])[:s.nthr] for j in range(nout)], F32).reshape(nout, s.nthr))
            a, b = values(fa), values(fb)
            assert a.shape[2:] == (H, W) and fa.T * max(fss.bound(H, W, n) for n in spec.scales) <= 1 << 62
            RECORD.append((a, b))
            S, R, per = fss_ref(spec, a, b)
            sums += torch.from_numpy(S.astype(np.int64))
            rates += torch.from_numpy(R.astype(np.int64))
            if per_field is not None:
                per_field.copy_(torch.from_numpy(per.astype(np.int64)))

    return FssEmuOps("f32")


# ------------------------------------------------------------------------------------------------- headroom
def _pairs(rng, sizes, H=8, W=8):
    out = []
    for n in sizes:
        a = rng.standard_normal((n, 2, H, W)).astype(F32)
        out.append((torch.from_numpy(a), torch.from_numpy(np.roll(a, 1, axis=3) + 0.3 * rng.standard_normal(a.shape).astype(F32))))
    return out


def test_draining_and_chunking_leave_the_totals_unchanged(monkeypatch):
    rng = np.random.default_rng(6)
    spec = FssSpec.zscore(2, thresholds=(0.0, 1.0), scales=(1, 3, 15))
    batches = _pairs(rng, (2, 2, 6, 2, 2, 1))
    ops = fss_emu_ops()

    def run():
        acc = FractionsSkill(spec, 8, 8, device="cpu", ops=ops)
        calls = len(RECORD)
        for a, b in batches:
            acc.add(a, b)
        return acc, acc.result(), [r[0].shape[0] for r in RECORD[calls:]]
    acc, plain, sizes = run()
    assert sizes == [2, 2, 6, 2, 2, 1] and acc.drains == 1               # one call per batch, drained once by result()
    mb = fss.bound(8, 8, 15)
    assert acc._max_bound == mb == 64 * 64 * 64
    monkeypatch.setattr(fss, "DRAIN_LIMIT", 4 * mb)                      # room for four fields on the device
    acc2, low, sizes2 = run()
    assert sizes2 == [2, 2, 4, 2, 2, 2, 1]                               # the batch of 6 is cut into 4 + 2
    assert acc2.drains >= 4                                              # ... and at least every second add drains first
    assert ints(low.sums()) == ints(plain.sums()) and ints(low.rates()) == ints(plain.rates()) and low.fields == plain.fields == 15
    a, b = torch.cat([p[0] for p in batches]), torch.cat([p[1] for p in batches])
    S, R, _ = fss_ref(spec, a.numpy(), b.numpy())
    assert ints(plain.sums()) == ints(S) and ints(plain.rates()) == ints(R)
    monkeypatch.setattr(fss, "DRAIN_LIMIT", 1)                           # below one field's bound: one field per call
    acc3, one, sizes3 = run()
    assert sizes3 == [1] * 15 and ints(one.sums()) == ints(plain.sums())
    # n_valid: the padding fields are not read
    monkeypatch.setattr(fss, "DRAIN_LIMIT", 1 << 62)
    acc4 = FractionsSkill(spec, 8, 8, device="cpu", ops=ops)
    junk = torch.full((3, 2, 8, 8), 9.0)
    for a_, b_ in batches:
        acc4.add(torch.cat([a_, junk[:2]]), torch.cat([b_, -junk[:2]]), n_valid=a_.shape[0])
    assert ints(acc4.result().sums()) == ints(plain.sums()) and acc4.fields == 15


def test_workspace_cap_cuts_a_batch_into_chunks(monkeypatch):
    rng = np.random.default_rng(7)
    spec = FssSpec.zscore(2, thresholds=(0.5,), scales=(1, 5))
    (a, b), = _pairs(rng, (7,))
    ops = fss_emu_ops()
    monkeypatch.setattr(ops, "fss_ws_bytes", lambda f, H, W, s: 100 * f.T)
    monkeypatch.setattr(fss, "WS_CAP", 350)                              # three fields per call
    n0 = len(RECORD)
    got = FractionsSkill(spec, 8, 8, device="cpu", ops=ops).add(a, b).result()
    assert [r[0].shape[0] for r in RECORD[n0:]] == [3, 3, 1]
    S, R, _ = fss_ref(spec, a.numpy(), b.numpy())
    assert ints(got.sums()) == ints(S) and ints(got.rates()) == ints(R)


def test_limb_all_reduce_round_trips_large_integers():
    vals = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 70) + 12345, (3 << 100) + (1 << 64) - 1, (1 << 128) - 1]
    t = fss.to_limbs(vals)
    assert t.dtype == torch.int64 and tuple(t.shape) == (len(vals), fss.LIMBS) and int(t.max()) < 1 << 32
    assert fss.from_limbs(t) == vals
    assert fss.from_limbs(t * 3) == [3 * v for v in vals]               # limbs grown past 32 bits by a sum still recombine
    for bad in ([-1], [1 << 128]):
        with pytest.raises(ValueError, match="limb"):
            fss.to_limbs(bad)

    class Three:                                                         # three ranks holding the same values
        world_size = 3

        def allreduce_sum_(self, flat):
            flat.mul_(3)
    assert fss.allreduce_ints(Three(), vals) == [3 * v for v in vals]
    assert fss.allreduce_ints(None, vals) == vals


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def _trainer(log_fss, dist=None, fs=False):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.GAN.wasserstein_fs import WassersteinGANFS
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = (WassersteinGANFS if fs else WassersteinGAN)(G, C_, dist=dist)
    if log_fss is not None:
        tr.log_fss = log_fss
    return tr


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: fss_emu_ops())
    setattr_(losses, "_ops", {})
    setattr_(histograms, "_ops", {})


def _loaders(lo=0, step=1, batch=2):
    from downgan_amd import synthetic
    from downgan_amd.GAN.dataloader import NetCDFSR
    coarse, fine = synthetic.tiles(6, 2, 16, seed=11)
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b][lo::step].copy()), torch.from_numpy(fine[a:b][lo::step].copy()))
    dl = torch.utils.data.DataLoader(ds(0, 2), batch_size=batch)
    tl = torch.utils.data.DataLoader(ds(2, 6), batch_size=batch)
    return dl, tl


def _run_epoch(log_fss, dist=None, lo=0, step=1, batch=2, fs=False):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(log_fss, dist, fs)
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr


def _one_shot(records, spec):
    a, b = np.concatenate([r[0] for r in records]), np.concatenate([r[1] for r in records])
    return fss.fss(torch.from_numpy(a), torch.from_numpy(b), spec=spec, ops=fss_emu_ops()), a, b


def test_log_fss_off_leaves_the_summary_unchanged(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_fss is False and WassersteinGAN.fss_spec is None and WassersteinGAN.fss_results is None
    n0 = len(RECORD)
    bare = _run_epoch(None).metrics_log[0]                                # the attribute never touched
    t_off = _run_epoch(False)
    off = t_off.metrics_log[0]
    assert t_off.fss_results is None and len(RECORD) == n0 and "fss" not in off
    assert list(off) == list(bare) and json.dumps(off, sort_keys=True) == json.dumps(bare, sort_keys=True)
    tr = _run_epoch(True)
    recs = RECORD[n0:]
    on = dict(tr.metrics_log[0])
    d = on.pop("fss")
    assert json.dumps(on, sort_keys=True) == json.dumps(off, sort_keys=True)    # the hook adds a key and changes nothing else
    assert json.loads(json.dumps(d, allow_nan=False)) == d
    assert set(d) == {"train", "test"} == set(tr.fss_results)
    assert [r[0].shape[0] for r in recs] == [2, 2, 2]                     # one train batch, two test batches, one call each
    spec = FssSpec.zscore(2)
    for part, rec, n in (("train", recs[:1], 2), ("test", recs[1:], 4)):
        once, a, b = _one_shot(rec, spec)
        assert d[part] == once.summary() == tr.fss_results[part].summary()
        assert d[part]["fields"] == n and d[part]["channels"] == ["ch0", "ch1", "speed"] and d[part]["grid"] == [128, 128]
        S, R, _ = fss_ref(spec, a, b)
        assert ints(tr.fss_results[part].sums()) == ints(S) and ints(tr.fss_results[part].rates()) == ints(R)
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    np.testing.assert_array_equal(np.concatenate([r[0] for r in recs[1:]]), fine[2:6])     # the real side is the test set
    assert tr.fss_results["test"].fss().shape == (3, 2, 8)


def test_log_fss_without_log_metrics(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    monkeypatch.setattr(WassersteinGAN, "log_metrics", False)
    n0 = len(RECORD)
    tr = _run_epoch(True)
    s = tr.metrics_log[0]
    assert "train" not in s and s["fss"]["train"]["fields"] == 2 and s["fss"]["test"]["fields"] == 4
    assert s["fss"]["test"] == _one_shot(RECORD[n0 + 1:], FssSpec.zscore(2))[0].summary()


def test_frequency_separation_trainer_reports_fss(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    n0 = len(RECORD)
    tr = _run_epoch(True, fs=True)
    s = tr.metrics_log[0]
    assert s["fss"]["train"]["fields"] == 2 and s["fss"]["test"]["fields"] == 4
    assert s["fss"]["test"] == _one_shot(RECORD[n0 + 1:], FssSpec.zscore(2))[0].summary()


def test_a_custom_spec_reaches_the_hook(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    spec = FssSpec(2, speed=None, thresholds=(0.5,), scales=(1, 7))
    monkeypatch.setattr(WassersteinGAN, "fss_spec", spec)
    s = _run_epoch(True).metrics_log[0]["fss"]["test"]
    assert s["channels"] == ["ch0", "ch1"] and s["scales"] == [1, 7] and np.array(s["fss"]).shape == (2, 1, 2)


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import downgan_amd.config.hyperparams as hp
    _patch(setattr)
    hp.batch_size, hp.lr = 1, 0.0
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    tr = _run_epoch(True, dist=d, lo=rank, step=world, batch=1)
    res = {k: (ints(v.sums()), ints(v.rates()), v.fields) for k, v in tr.fss_results.items()}
    big = fss.allreduce_ints(d, [(1 << 70) + rank, 5], "cpu")
    torch.save({"summary": tr.metrics_log[0]["fss"], "res": res, "big": big}, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_sums(monkeypatch):
    """lr = 0 keeps G identical in both runs, so the generated fields are the same and only the reduction is tested."""
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(hp, "lr", 0.0)
    torch.set_num_threads(4)
    tr = _run_epoch(True)
    ref = tr.fss_results
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["summary"] == r1["summary"] and r0["big"] == r1["big"] == [(2 << 70) + 1, 10]
    for part in ("train", "test"):
        assert r0["summary"][part] == tr.metrics_log[0]["fss"][part]
        for r in (r0, r1):
            assert r["res"][part] == (ints(ref[part].sums()), ints(ref[part].rates()), ref[part].fields)
