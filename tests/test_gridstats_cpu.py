"""Per-gridpoint statistics without a GPU: spec validation, argument checks that fire before any library call, the ABI surface
and struct layout, the slice rule, the host-side derivations of ``GridMaps`` from hand-made sums against two-pass numpy, and the
trainer's opt-in hook on the emulated ops (a test-local op class adds a numpy ``gridstats`` under the usual make_ops patch), in
one process, over 2 gloo ranks, and in the frequency-separation trainer."""
import ctypes as C
import json
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

from downgan_amd import _lib, gridstats, histograms
from downgan_amd.gridstats import GridMaps, GridSpec, GridStats

from .test_histograms_cpu import transform_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
LD = np.longdouble


# ------------------------------------------------------------------------------------------------- the definition in numpy
def grid_ref(spec, a, b=None):
    """The definition over a (and b) float32 [C, T, P], the values the kernel reads: (sums longdouble [nout, NS, P], mags
    longdouble [nout, NS, P] = the sums of the |terms|, extrema float32 [nout, NE, P], counts int32 [nout, NC, P]); the row
    layout of include/downgan_hip.h.  Transform in numpy float32 (transform_ref), sums in longdouble."""
    Cn, T, P = a.shape
    nout, K = spec.nout, spec.K
    piv = spec.pivot.astype(LD)[:, None, None]

    def side(x):
        y = transform_ref(spec, x.reshape(Cn, -1)).reshape(nout, T, P)
        fin = np.isfinite(y)
        u = np.where(fin, y.astype(LD) - piv, LD(0))
        S = [(u ** k).sum(axis=1) for k in (1, 2, 3, 4)]
        M = [(np.abs(u) ** k).sum(axis=1) for k in (1, 2, 3, 4)]
        mn = np.where(fin, y, F32(np.inf)).min(axis=1).astype(F32)
        mx = np.where(fin, y, F32(-np.inf)).max(axis=1).astype(F32)
        with np.errstate(invalid="ignore"):
            E = [(y > spec.thresholds[:, k][:, None, None]).sum(axis=1).astype(np.int32) for k in range(K)]
        return y, fin, u, S, M, [mn, mx], fin.sum(axis=1).astype(np.int32), E

    ya, fa, ua, Sa, Ma, ea, na, Ea = side(a)
    if b is None:
        return np.stack(Sa, 1), np.stack(Ma, 1), np.stack(ea, 1), np.stack([na] + Ea, 1)
    yb, fb, ub, Sb, Mb, eb, nb, Eb = side(b)
    both = fa & fb
    with np.errstate(invalid="ignore"):
        d = np.where(both, yb.astype(LD) - ya.astype(LD), LD(0))
    x = ua * ub
    pair = [d.sum(axis=1), np.abs(d).sum(axis=1), (d * d).sum(axis=1), x.sum(axis=1)]
    pmag = [np.abs(d).sum(axis=1), np.abs(d).sum(axis=1), (d * d).sum(axis=1), np.abs(x).sum(axis=1)]
    return (np.stack(Sa + Sb + pair, 1), np.stack(Ma + Mb + pmag, 1), np.stack(ea + eb, 1),
            np.stack([na, nb, both.sum(axis=1).astype(np.int32)] + Ea + Eb, 1))


def sum_bound(mags, T_total):
    """The issue's bound on every fp64 sum: (T + 8) 2^-52 sum |term| -- twice the first-order bound of a length-T fp64 sum
    with at most 4 roundings per term; the factor 2 covers the reference's own rounding."""
    return (T_total + 8) * LD(2.0) ** -52 * mags


def maps_of(spec, H, W, a, b=None, fields=None):
    """A GridMaps built from the numpy definition (CPU tensors); a, b float32 [C, T, H*W]."""
    s, _, e, c = grid_ref(spec, a, b)
    return GridMaps(spec, H, W, b is not None, torch.from_numpy(s.astype(np.float64)), torch.from_numpy(e), torch.from_numpy(c),
                    a.shape[1] if fields is None else fields)


# ------------------------------------------------------------------------------------------------- spec and argument checks
def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("library or device touched before the arguments were checked")
    from downgan_amd import backend
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(backend, "make_ops", boom)
    monkeypatch.setattr(histograms, "_ops", {})


@pytest.mark.parametrize("kw,match", [
    (dict(C=0), "C <="),
    (dict(C=9), "C <="),
    (dict(C=2.5), "C <="),
    (dict(C=1), "speed"),                                                # the default speed (0, 1) of a 1-channel field
    (dict(C=3, speed=(0, 3)), "speed"),
    (dict(C=2, scale=[1.0]), "scale"),
    (dict(C=2, offset=[0.0, np.nan]), "finite"),
    (dict(C=2, scale=[1e39, 1.0]), "fp32"),
    (dict(C=2, pivot=[0.0, 0.0]), "pivot"),
    (dict(C=2, pivot=[0.0, 0.0, np.inf]), "finite"),
    (dict(C=2, thresholds=(1.0, 2.0, 3.0, 4.0, 5.0)), "at most"),
    (dict(C=2, thresholds=[[1.0], [2.0]]), "one list per output"),
    (dict(C=2, thresholds=[[1.0], [2.0], [3.0, 4.0]]), "one length"),
    (dict(C=2, thresholds=(1.0, np.inf)), "finite"),
    (dict(C=2, names=["a", "b"]), "names"),
])
def test_spec_is_checked(monkeypatch, kw, match):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=match):
        GridSpec(**kw)


def test_constructors():
    z = GridSpec.zscore(2)
    assert (z.C, z.nout, z.speed, z.K, z.names) == (2, 3, (0, 1), 2, ["ch0", "ch1", "speed"])
    assert z.thresholds.tolist() == [[2.0, 3.0]] * 3 and z.pivot.tolist() == [0.0, 0.0, 0.0]
    one = GridSpec.zscore(1, thresholds=())
    assert one.speed is None and one.nout == 1 and one.K == 0
    stats = {"u10": (0.5, 3.0), "v10": (-0.25, 2.0), "t2m": (280.0, 10.0)}
    p = GridSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [15.0]])
    assert p.speed == (1, 2) and p.names == ["t2m", "u10", "v10", "speed"]
    assert p.scale.tolist() == [10.0, 3.0, 2.0] and p.offset.tolist() == [280.0, 0.5, -0.25]
    assert p.pivot.tolist() == [280.0, 0.5, -0.25, 0.0] and p.thresholds[:, 0].tolist() == [300.0, 10.0, 10.0, 15.0]
    assert p == GridSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [15.0]]) and p != z
    assert GridSpec(2, thresholds=(0.1,)).thresholds.dtype == np.float32
    assert GridSpec(2, thresholds=(0.1,)).thresholds[0, 0] == F32(0.1)          # rounded to fp32
    s = p.struct()
    assert (s.speed_u, s.speed_v, s.nthr) == (1, 2, 1) and s.thr[3][0] == 15.0 and s.pivot[0] == 280.0 and s.scale[2] == 2.0
    n = GridSpec(2, speed=None).struct()
    assert (n.speed_u, n.speed_v, n.nthr) == (-1, -1, 0)


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
    spec = GridSpec.zscore(2)
    good = torch.zeros(2, 2, 8, 8)
    single = GridStats(spec, 8, 8, paired=False, device="cpu")
    with pytest.raises(err, match=match):
        single.add(x, **kw)
    pair = GridStats(spec, 8, 8, paired=True, device="cpu")
    with pytest.raises(err, match=match):
        pair.add(good, x, nhwc=(False, kw.get("nhwc", False)), channels=kw.get("channels"))
    with pytest.raises(err, match=match):
        pair.add(x, good, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))
    if "grid" not in match:                                               # the one-shot form takes the grid from the fields
        with pytest.raises(err, match=match):
            gridstats.gridstats(x, spec=spec, **kw)
        with pytest.raises(err, match=match):
            gridstats.gridstats(good, x, spec=spec, nhwc=(False, kw.get("nhwc", False)), channels=kw.get("channels"))


def test_accumulator_checks(monkeypatch):
    _no_library(monkeypatch)
    spec = GridSpec.zscore(2)
    x = torch.zeros(2, 2, 8, 8)
    pair, single = GridStats(spec, 8, 8, device="cpu"), GridStats(spec, 8, 8, paired=False, device="cpu")
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            pair.add(x, x, n_valid=n)
    with pytest.raises(ValueError, match="paired"):
        pair.add(x)
    with pytest.raises(ValueError, match="one series"):
        single.add(x, x)
    with pytest.raises(ValueError, match="differ in length"):
        pair.add(x, torch.zeros(3, 2, 8, 8))
    with pytest.raises(TypeError, match="GridSpec"):
        GridStats(histograms.HistSpec.zscore(2), 8, 8, device="cpu")
    with pytest.raises(TypeError, match="GridSpec"):
        gridstats.gridstats(x, spec=histograms.HistSpec.zscore(2))
    with pytest.raises(ValueError, match="grid"):
        GridStats(spec, 0, 8, device="cpu")
    with pytest.raises(ValueError, match="side"):
        GridMaps(spec, 8, 8, False, None, None, None, 1).count("fake")
    pair._added = 2 ** 31 - 2                                            # the int32 counters: the total must stay below 2^31
    with pytest.raises(ValueError, match="2\\^31"):
        pair.add(x, x)
    assert pair.fields == 0 and pair._sums.shape == (3, 12, 64) and pair._cnt.shape == (3, 7, 64) and pair._cnt.dtype == torch.int32
    assert single._sums.shape == (3, 4, 64) and single._ext.shape == (3, 2, 64) and single._cnt.shape == (3, 3, 64)
    e = pair._ext
    assert torch.isposinf(e[:, 0::2]).all() and torch.isneginf(e[:, 1::2]).all()


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_gridstats_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert re.search(r"#define DG_GRID_MAX_THR 4\b", src) and "Per-gridpoint statistics (csrc/gridstats.hip)" in src
    for sym in ("dg_gridstats_ws_bytes", "dg_gridstats_slices", "dg_gridstats"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    assert _lib.GRID_MAX_THR == gridstats.THR_MAX == 4
    assert "gridstats.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()


def test_grid_spec_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.GridSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(dg_grid_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_grid_spec, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("thr_row %zu\\n", sizeof(((dg_grid_spec*)0)->thr[0]));', '  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert int(got["thr_row"]) == 4 * _lib.GRID_MAX_THR


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=64, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    good = GridSpec.zscore(2).struct()

    def spec(**kw):
        s = GridSpec.zscore(2).struct()
        for k, v in kw.items():
            if isinstance(v, tuple) and len(v) == 3:
                getattr(s, k)[v[0]][v[1]] = v[2]
            elif isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    ws, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    call = lambda fa, fb, s, w=ws, o=out: lib.dg_gridstats(fa, fb, s, w, o, o, o, None)
    assert lib.dg_gridstats_slices(64, 100) > 1                          # so that a NULL workspace is an error below
    assert call(f(base=0), None, C.byref(good)) == -1
    assert call(f(C=9), None, C.byref(good)) == -1
    assert call(f(T=0), None, C.byref(good)) == -1
    assert call(f(P=0), None, C.byref(good)) == -1
    assert call(f(ld_t=-1), None, C.byref(good)) == -1
    assert call(f(), None, C.byref(good), None) == -1
    assert call(f(), None, C.byref(good), ws, None) == -1
    assert call(f(), None, None) == -1
    assert call(f(), None, spec(nthr=5)) == -1 and call(f(), None, spec(nthr=-1)) == -1
    assert call(f(), None, spec(speed_u=2)) == -1 and call(f(), None, spec(speed_v=-1)) == -1
    assert call(f(), None, spec(scale=(1, float("inf")))) == -1 and call(f(), None, spec(offset=(0, float("nan")))) == -1
    assert call(f(), None, spec(pivot=(2, float("nan")))) == -1
    assert call(f(), None, spec(thr=(2, 1, float("inf")))) == -1
    assert call(f(C=1), None, C.byref(good)) == -1                       # speed channel 1 of a 1-channel field
    assert call(f(), f(T=63), C.byref(good)) == -1 and call(f(), f(P=96), C.byref(good)) == -1
    assert call(f(), f(base=0), C.byref(good)) == -1
    assert call(f(C=3), f(C=2), C.byref(good)) == -1
    assert call(f(dtype=7), None, C.byref(good)) == -2
    assert call(f(), f(dtype=7), C.byref(good)) == -2
    assert lib.dg_gridstats_ws_bytes(f(C=9), 0, C.byref(good)) == 0 and lib.dg_gridstats_ws_bytes(f(), 1, spec(nthr=9)) == 0
    one = lib.dg_gridstats_ws_bytes(f(), 0, C.byref(good))
    two = lib.dg_gridstats_ws_bytes(f(), 1, C.byref(good))
    S = lib.dg_gridstats_slices(64, 100)
    assert one >= S * 3 * 100 * (4 * 8 + 2 * 4 + 3 * 4) and two >= S * 3 * 100 * (12 * 8 + 4 * 4 + 7 * 4) and two < 1 << 20
    assert 0 < lib.dg_gridstats_ws_bytes(f(T=3), 1, C.byref(good)) <= 4096     # one slice: no partial state


def test_the_slice_rule_is_the_documented_function_of_T_and_P():
    lib = _lib.lib()

    def rule(T, P):
        nb = -(-P // 256)
        return 1 if nb >= 1024 else max(1, min(-(-1024 // nb), T // 16))
    for T, P in [(40, 4096), (300, 256), (3, 37000), (1, 91), (4096, 128 * 128), (32, 1 << 20), (24, 64), (15, 64), (16, 64),
                 (32, 1), (100000, 255 * 1024), (100000, 256 * 1024 - 255), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1)]:
        got = lib.dg_gridstats_slices(T, P)
        assert got == rule(T, P) == lib.dg_gridstats_slices(T, P) and got >= 1, (T, P, got)
    assert lib.dg_gridstats_slices(40, 4096) == 2 and lib.dg_gridstats_slices(300, 256) == 18
    assert lib.dg_gridstats_slices(3, 37000) == 1 and lib.dg_gridstats_slices(4096, 128 * 128) == 16
    assert lib.dg_gridstats_slices(0, 5) == 0 and lib.dg_gridstats_slices(5, 0) == 0


# ------------------------------------------------------------------------------------------------- derived maps
def _gauss_pair(T=4096, H=4, W=5, seed=0):
    """Gaussian data with |mean - pivot| <= std in every channel and pixel, fake correlated with real."""
    rng = np.random.default_rng(seed)
    P = H * W
    std = rng.uniform(0.5, 3.0, (2, 1, P))
    mean = rng.uniform(-1.0, 1.0, (2, 1, P)) * std
    a = (mean + std * rng.standard_normal((2, T, P))).astype(F32)
    b = (0.7 * a + 0.5 * std * rng.standard_normal((2, T, P)) + 0.1).astype(F32)
    return a, b


def test_maps_against_two_pass_numpy():
    H, W = 4, 5
    a, b = _gauss_pair(H=H, W=W)
    spec = GridSpec(2, scale=[1.5, 0.5], offset=[0.25, -1.0], pivot=[0.0, -1.0, 2.0], thresholds=[[1.0, 4.0], [-1.0, 0.0], [2.0, 5.0]])
    m = maps_of(spec, H, W, a, b)
    ya = transform_ref(spec, a.reshape(2, -1)).reshape(3, -1, H, W).astype(np.float64)
    yb = transform_ref(spec, b.reshape(2, -1)).reshape(3, -1, H, W).astype(np.float64)
    T = ya.shape[1]
    for side, y in (("real", ya), ("fake", yb)):
        mu = y.mean(axis=1)
        c = y - mu[:, None]
        var = (c * c).mean(axis=1)
        np.testing.assert_array_equal(m.count(side), np.full((3, H, W), T))
        np.testing.assert_allclose(m.mean(side), mu, rtol=1e-10, atol=0)
        np.testing.assert_allclose(m.variance(side), var, rtol=1e-10, atol=0)
        np.testing.assert_allclose(m.variance(side, ddof=1), var * T / (T - 1), rtol=1e-10, atol=0)
        np.testing.assert_allclose(m.std(side), np.sqrt(var), rtol=1e-10, atol=0)
        np.testing.assert_allclose(m.skewness(side), (c ** 3).mean(axis=1) / var ** 1.5, rtol=0, atol=1e-10)
        np.testing.assert_allclose(m.kurtosis(side), (c ** 4).mean(axis=1) / var ** 2 - 3, rtol=0, atol=1e-10)
        np.testing.assert_array_equal(m.min(side), y.min(axis=1))
        np.testing.assert_array_equal(m.max(side), y.max(axis=1))
        ex = m.exceedance(side)
        assert ex.shape == (3, 2, H, W)
        for k in range(2):
            np.testing.assert_array_equal(ex[:, k], (y > spec.thresholds[:, k].astype(np.float64)[:, None, None, None]).mean(axis=1))
    d = yb - ya
    np.testing.assert_allclose(m.bias(), d.mean(axis=1), rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(m.mae(), np.abs(d).mean(axis=1), rtol=1e-10, atol=0)
    np.testing.assert_allclose(m.rmse(), np.sqrt((d * d).mean(axis=1)), rtol=1e-10, atol=0)
    ca, cb = ya - ya.mean(axis=1)[:, None], yb - yb.mean(axis=1)[:, None]
    corr = (ca * cb).mean(axis=1) / np.sqrt((ca * ca).mean(axis=1) * (cb * cb).mean(axis=1))
    np.testing.assert_allclose(m.correlation(), corr, rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.std_ratio(), yb.std(axis=1) / ya.std(axis=1), rtol=1e-10, atol=0)
    assert m.nonfinite("real").tolist() == [0, 0, 0]


def test_nan_rules_of_the_correlation_and_of_empty_pixels():
    H, W = 2, 3
    a, b = _gauss_pair(T=64, H=H, W=W, seed=1)
    a[0, 5, 0] = np.nan                                   # pixel 0, channel 0: one real value missing -> n_ab != n_fake
    b[1, 7, 1] = np.inf                                   # pixel 1, channel 1: one generated value missing
    a[0, :, 2] = 1.5                                      # pixel 2, channel 0: constant real series -> variance 0
    a[:, :, 3] = np.nan                                   # pixel 3: no valid real value at all
    spec = GridSpec.zscore(2)
    m = maps_of(spec, H, W, a, b)
    r = m.correlation().reshape(3, -1)
    assert np.isnan(r[0, 0]) and np.isnan(r[2, 0]) and np.isfinite(r[1, 0])       # the speed inherits the NaN
    assert np.isnan(r[1, 1]) and np.isnan(r[2, 1]) and np.isfinite(r[0, 1])
    assert np.isnan(r[0, 2]) and np.isfinite(r[1, 2])
    assert np.isnan(r[:, 3]).all() and np.isfinite(r[:, 4:]).all()
    assert m.count("real").reshape(3, -1)[:, 3].tolist() == [0, 0, 0] and m.count_pairs().reshape(3, -1)[0, 0] == 63
    for f in (m.mean, m.std, m.min, m.max, m.skewness):
        assert np.isnan(f("real").reshape(3, -1)[:, 3]).all()
    assert np.isnan(m.bias().reshape(3, -1)[:, 3]).all() and np.isnan(m.std_ratio().reshape(3, -1)[0, 2])
    assert m.nonfinite("real").tolist() == [65, 64, 65] and m.nonfinite("fake").tolist() == [0, 1, 1]
    assert m.exceedance("fake").reshape(3, 2, -1)[1, :, 1].min() >= 1 / 64       # +inf exceeds every threshold
    s = m.summary()
    json.dumps(s, allow_nan=False)
    with pytest.raises(ValueError, match="pair"):
        maps_of(spec, H, W, a).bias()


def test_summary_is_json_serialisable_and_save_round_trips(tmp_path):
    H, W = 4, 5
    a, b = _gauss_pair(T=256, H=H, W=W, seed=2)
    spec = GridSpec.zscore(2)
    m = maps_of(spec, H, W, a, b)
    s = m.summary()
    assert json.loads(json.dumps(s, allow_nan=False)) == s
    assert s["channels"] == ["ch0", "ch1", "speed"] and s["fields"] == 256 and s["grid"] == [H, W]
    for k in ("bias_mean", "abs_bias_mean", "mae_mean", "rmse_rms", "corr_mean", "corr_min", "pattern_corr_mean",
              "pattern_corr_std"):
        assert len(s[k]) == 3 and all(isinstance(v, float) for v in s[k]), k
    assert np.array(s["exceed_max_abs_diff"]).shape == (3, 2) and s["nonfinite"] == {"real": [0, 0, 0], "fake": [0, 0, 0]}
    np.testing.assert_allclose(s["bias_mean"], m.bias().reshape(3, -1).mean(axis=1), rtol=1e-12)
    np.testing.assert_allclose(s["rmse_rms"], np.sqrt((m.rmse() ** 2).reshape(3, -1).mean(axis=1)), rtol=1e-12)
    np.testing.assert_allclose(s["corr_min"], m.correlation().reshape(3, -1).min(axis=1), rtol=1e-12)
    want = [np.corrcoef(m.mean("real")[j].ravel(), m.mean("fake")[j].ravel())[0, 1] for j in range(3)]
    np.testing.assert_allclose(s["pattern_corr_mean"], want, rtol=1e-9)
    names = m.save(str(tmp_path / "maps"))
    assert "summary.json" in names and {"real_mean.npy", "fake_std.npy", "bias.npy", "correlation.npy", "real_exceedance.npy"} <= set(names)
    assert json.load(open(tmp_path / "maps" / "summary.json")) == s
    for k, v in m.maps().items():
        np.testing.assert_array_equal(np.load(tmp_path / "maps" / (k + ".npy")), v)
    one = maps_of(spec, H, W, a)
    json.dumps(one.summary(), allow_nan=False)
    assert set(one.maps()) == {f"real_{k}" for k in ("count", "mean", "std", "skewness", "kurtosis", "min", "max", "exceedance")}


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def grid_emu_ops():
    from oracle.emu_ops import EmuOps

    class GridEmuOps(EmuOps):
        """The emulated ops plus dg_gridstats's contract in numpy (float32 transform, sums rounded to float64)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            P = t.shape[1] * t.shape[2] if nhwc else t.shape[2] * t.shape[3]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=P)

        def gridstats_ws_bytes(self, f, paired, spec):
            return 1

        def gridstats(self, fa, fb, s, sums, extrema, counts):
            def values(f):
                x = f.t[..., :f.C].permute(3, 0, 1, 2) if f.nhwc else f.t[:, :f.C].permute(1, 0, 2, 3)
                return x.detach().float().cpu().numpy().reshape(f.C, f.T, -1)
            speed = None if s.speed_u < 0 else (s.speed_u, s.speed_v)
            nout = fa.C + (speed is not None)
            spec = types.SimpleNamespace(nout=nout, K=s.nthr, speed=speed, scale=np.array(s.scale[:fa.C], F32),
                                         offset=np.array(s.offset[:fa.C], F32), pivot=np.array(s.pivot[:nout], F32),
                                         thresholds=np.array([list(s.thr[j])[:s.nthr] for j in range(nout)], F32).reshape(nout, s.nthr))
            S, _, e, c = grid_ref(spec, values(fa), None if fb is None else values(fb))
            sums += torch.from_numpy(S.astype(np.float64))
            counts += torch.from_numpy(c)
            e = torch.from_numpy(e)
            extrema[:, 0::2] = torch.minimum(extrema[:, 0::2], e[:, 0::2])
            extrema[:, 1::2] = torch.maximum(extrema[:, 1::2], e[:, 1::2])

    return GridEmuOps("f32")


def _trainer(log_maps, dist=None, fs=False, map_dir=None):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.GAN.wasserstein_fs import WassersteinGANFS
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = (WassersteinGANFS if fs else WassersteinGAN)(G, C_, dist=dist)
    tr.log_maps = log_maps
    tr.map_dir = map_dir
    return tr


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: grid_emu_ops())
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


def _run_epoch(log_maps, dist=None, lo=0, step=1, batch=2, fs=False, map_dir=None):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(log_maps, dist, fs, map_dir)
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr


def test_log_maps_off_leaves_the_summary_unchanged(monkeypatch, tmp_path):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_maps is False and WassersteinGAN.map_spec is None and WassersteinGAN.map_dir is None
    assert WassersteinGAN.map_results is None
    t_off = _run_epoch(False)
    off = t_off.metrics_log[0]
    assert t_off.map_results is None
    tr = _run_epoch(True, map_dir=str(tmp_path / "maps"))
    on = dict(tr.metrics_log[0])
    assert "maps" not in off
    d = on.pop("maps")
    assert json.dumps(on, sort_keys=True) == json.dumps(off, sort_keys=True)    # the hook adds a key and changes nothing else
    json.dumps(d, allow_nan=False)
    assert set(d) == {"train", "test"} == set(tr.map_results)
    for part, n in (("train", 2), ("test", 4)):
        assert d[part]["fields"] == n == tr.map_results[part].fields and d[part]["channels"] == ["ch0", "ch1", "speed"]
        assert d[part] == tr.map_results[part].summary()
        assert os.path.exists(tmp_path / "maps" / "0" / part / "summary.json")
        assert np.load(tmp_path / "maps" / "0" / part / "bias.npy").shape == (3, 128, 128)
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    spec = GridSpec.zscore(2)
    a = np.ascontiguousarray(fine[2:6].transpose(1, 0, 2, 3)).reshape(2, 4, -1)
    S, _, e, c = grid_ref(spec, a)
    got_s, got_e, got_c = tr.map_results["test"].host()
    np.testing.assert_array_equal(got_c[:, 0], c[:, 0])                         # the real side of the pair is the test set
    np.testing.assert_array_equal(got_c[:, 3:5], c[:, 1:3])
    np.testing.assert_array_equal(got_e[:, 0:2], e)
    np.testing.assert_allclose(got_s[:, 0:4], S.astype(np.float64), rtol=1e-12, atol=1e-12)

def test_log_maps_without_log_metrics(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    monkeypatch.setattr(WassersteinGAN, "log_metrics", False)
    s = _run_epoch(True).metrics_log[0]
    assert "train" not in s and s["maps"]["train"]["fields"] == 2 and s["maps"]["test"]["fields"] == 4


def test_frequency_separation_trainer_reports_maps(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    s = _run_epoch(True, fs=True).metrics_log[0]
    assert s["maps"]["train"]["fields"] == 2 and s["maps"]["test"]["fields"] == 4


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import downgan_amd.config.hyperparams as hp
    _patch(setattr)
    hp.batch_size, hp.lr = 1, 0.0
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    tr = _run_epoch(True, dist=d, lo=rank, step=world, batch=1)
    res = {k: v.host() for k, v in tr.map_results.items()}
    torch.save({"summary": tr.metrics_log[0]["maps"], "maps": res}, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_maps(monkeypatch):
    """lr = 0 keeps G identical in both runs, so the generated fields are the same and only the reduction is tested."""
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(hp, "lr", 0.0)
    torch.set_num_threads(4)
    tr = _run_epoch(True)
    ref = tr.map_results
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["summary"] == r1["summary"]
    for part in ("train", "test"):
        assert r0["summary"][part]["fields"] == ref[part].fields
        for r in (r0, r1):
            s, e, c = r["maps"][part]
            rs, re_, rc = ref[part].host()
            np.testing.assert_array_equal(c, rc)
            np.testing.assert_array_equal(e, re_)
            np.testing.assert_allclose(s, rs, rtol=1e-12, atol=0)
