"""Intensity-scale verification without a GPU: the integer numpy oracle (iscale_ref) against a brute-force Haar decomposition with
explicit father and mother components, the library's host reference (dg_iscale_host, dg_iscale_bound, dg_iscale_levels) against
the oracle and against closed forms, the derived scores of ``IscaleResult`` on hand-made sums, special values, spec and argument
checks that fire before any library call, the ABI surface and struct layout, the headroom rules of ``IntensityScale`` (drain,
chunks, limb all-reduce over 2 gloo ranks) on emulated ops (a test-local op class adds a numpy ``iscale``), and the trainer's
opt-in hook: off by default, appended last, one accumulator per part.  Every comparison of sums is integer equality."""
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

from downgan_amd import _lib, histograms, iscale
from downgan_amd.iscale import IntensityScale, IscaleResult, IscaleSpec

from .iscale_ref import F32, block_sums, ints, iscale_ref, log_side
from .test_gridstats_cpu import _no_library
from .test_trainer_hooks_cpu import FEED, KEYS, _loaders, _run, _stub, _trainer
from .test_trainer_hooks_cpu import log  # noqa: F401  (the fixture that stubs the twelve other accumulators)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, 1), (5, 3), (16, 16), (64, 64), (65, 33), (128, 128), (72, 200)]


def host_sums(spec, a, b):
    """int64 sums of the library's host reference over the field pairs of a, b float32 [T, C, H, W]."""
    T, Cn, H, W = a.shape
    sums = np.zeros((spec.nout, spec.K, log_side(H, W) + 1, 3), np.int64)
    s = spec.struct()
    for t in range(T):
        xa, xb = np.ascontiguousarray(a[t], dtype=F32), np.ascontiguousarray(b[t], dtype=F32)
        _lib.check(_lib.lib().dg_iscale_host(C.byref(s), xa.ctypes.data, xb.ctypes.data, Cn, H, W, sums.ctypes.data), "dg_iscale_host")
    return sums


def host_result(spec, a, b):
    return IscaleResult(spec, a.shape[2], a.shape[3], host_sums(spec, a, b), a.shape[0])


def one_channel(thr=0.5):
    return IscaleSpec(1, speed=None, thresholds=(thr,))


# ------------------------------------------------------------------------------------------------- the oracle
def haar_components(x, n):
    """x float64 [2^n, 2^n] -> the energies (sums of squares over the pixels) of its n mother components, finest first, and of
    the father component, by the explicit decomposition: F_l = the block means of side 2^l spread back over their blocks,
    mother l = F_(l-1) - F_l, father = F_n."""
    S = 1 << n
    fathers = []
    for l in range(n + 1):
        b = 1 << l
        means = x.reshape(S // b, b, S // b, b).mean(axis=(1, 3))
        fathers.append(np.kron(means, np.ones((b, b))))
    assert np.array_equal(fathers[0], x)
    parts = [fathers[l - 1] - fathers[l] for l in range(1, n + 1)] + [fathers[n]]
    assert np.allclose(sum(parts), x, rtol=0, atol=1e-12)
    for i in range(len(parts)):                                           # the components are orthogonal
        for j in range(i):
            assert abs((parts[i] * parts[j]).sum()) < 1e-9
    return [float((p * p).sum()) for p in parts]


@pytest.mark.parametrize("N", [8, 16])
def test_the_oracle_equals_a_brute_force_haar_decomposition(N):
    rng = np.random.default_rng(N)
    n = log_side(N, N)
    a, b = (rng.random((1, 1, N, N)) < 0.4).astype(F32), (rng.random((1, 1, N, N)) < 0.3).astype(F32)
    spec = one_channel()
    sums, per = iscale_ref(spec, a, b)
    assert ints(per[0]) == ints(sums)
    res = IscaleResult(spec, N, N, sums, 1)
    comp = res.components()[0, 0]                                          # [n + 1, 3]
    ia, ib = a[0, 0].astype(np.float64), b[0, 0].astype(np.float64)
    for e, x in enumerate((ib - ia, ia, ib)):
        np.testing.assert_allclose(comp[:, e], haar_components(x, n), rtol=0, atol=1e-9)
    assert comp[:, 0].sum() == int(sums[0, 0, 0, 0]) == int((ia != ib).sum())           # D_0: the disagreeing pixels
    assert int(sums[0, 0, 0, 1]) == int(ia.sum()) and int(sums[0, 0, 0, 2]) == int(ib.sum())
    np.testing.assert_allclose(res.mse()[0, 0], comp[:, 0] / (N * N), rtol=1e-15)
    np.testing.assert_allclose(res.mse()[0, 0].sum(), ((ib - ia) ** 2).mean(), rtol=1e-14)
    assert res.scales_px == tuple(1 << l for l in range(n)) + (N,) and res.levels == n + 1


def test_the_oracle_pads_a_ragged_grid_with_zeros():
    rng = np.random.default_rng(2)
    m = rng.random((2, 5, 3)) < 0.5
    for l in range(4):
        got = block_sums(m, 3, l)
        b = 1 << l
        for t in range(2):
            for y in range(8 // b):
                for x in range(8 // b):
                    want = sum(int(m[t, h, w]) for h in range(y * b, (y + 1) * b) for w in range(x * b, (x + 1) * b) if h < 5 and w < 3)
                    assert got[t, y, x] == want


# ------------------------------------------------------------------------------------------------- the host reference
def gauss_pair(rng, T, Cn, H, W):
    a = rng.standard_normal((T, Cn, H, W)).astype(F32)
    return a, (np.roll(a, 1, axis=3) + 0.5 * rng.standard_normal(a.shape)).astype(F32)


@pytest.mark.parametrize("grid", GRIDS)
def test_host_reference_equals_the_oracle(grid):
    H, W = grid
    rng = np.random.default_rng(H * W)
    for Cn, spec in ((1, IscaleSpec(1, speed=None, thresholds=(-0.5, 0.7))),
                     (2, IscaleSpec(2, scale=[3.0, 2.5], offset=[-1.5, 4.0], speed=(1, 0), thresholds=[[1.5, 0.0], [6.5, 4.0], [6.0, 12.0]]))):
        a, b = gauss_pair(rng, 2, Cn, H, W)
        want, _ = iscale_ref(spec, a, b)
        got = host_sums(spec, a, b)
        assert got.shape == (spec.nout, spec.K, log_side(H, W) + 1, 3) and ints(got) == ints(want)
        assert H * W < 16 or (all(v > 0 for v in ints(want[0, :, 0])) and any(v > 0 for v in ints(want[-1, :, 0])))   # not degenerate


def test_one_aligned_block_against_an_empty_field():
    N, n = 32, 5
    for m, (y, x) in ((0, (7, 9)), (1, (6, 10)), (2, (4, 28)), (3, (24, 8)), (5, (0, 0))):
        a, b = np.zeros((1, 1, N, N), F32), np.zeros((1, 1, N, N), F32)
        a[0, 0, y:y + (1 << m), x:x + (1 << m)] = 1.0
        s = host_sums(one_channel(), a, b)[0, 0]
        for l in range(n + 1):
            want = 4 ** (m + l) if l <= m else 16 ** m
            assert s[l].tolist() == [want, want, 0], (m, l)


def test_a_checkerboard_against_an_empty_field():
    N, n = 16, 4
    P = N * N
    a = ((np.add.outer(np.arange(N), np.arange(N)) % 2) == 0).astype(F32)[None, None]
    res = host_result(one_channel(), a, np.zeros_like(a))
    s = res.sums()[0, 0]
    assert ints(s[0]) == [P // 2, P // 2, 0]
    for l in range(1, n + 1):
        assert ints(s[l]) == [P * 4 ** l // 4, P * 4 ** l // 4, 0]
    # all the energy of the pattern sits in component 1 (features of 1 px); the father component carries the mean 1/2
    assert res.components()[0, 0, :, 1].tolist() == [P / 4, 0.0, 0.0, 0.0, P / 4]
    assert res.energy("real")[0, 0].tolist() == [0.25, 0.0, 0.0, 0.0, 0.25] and res.base_rates("real")[0, 0] == 0.5
    assert res.energy_rel_diff()[0, 0, 0] == -1.0 and math.isnan(res.energy_rel_diff()[0, 0, 1])
    assert res.worst_scale()[0, 0] == 1.0


def test_identical_series():
    rng = np.random.default_rng(3)
    a, _ = gauss_pair(rng, 2, 2, 16, 9)
    res = host_result(IscaleSpec.zscore(2, thresholds=(0.0, 0.5)), a, a.copy())
    s = res.sums()
    assert all(int(v) == 0 for v in s[..., 0].reshape(-1)) and ints(s[..., 1]) == ints(s[..., 2]) and min(ints(s[..., 0, 1])) > 0
    assert np.all(res.skill() == 1.0) and np.all(res.energy_rel_diff() == 0.0) and np.all(res.frequency_bias() == 1.0)
    assert np.all(res.mse() == 0.0)


def test_all_false_masks_give_nan_and_none():
    spec = IscaleSpec.zscore(2, thresholds=(50.0,))
    z = np.zeros((2, 2, 7, 13), F32)
    res = host_result(spec, z, z)
    assert np.isnan(res.skill()).all() and np.isnan(res.energy_rel_diff()).all() and np.isnan(res.frequency_bias()).all()
    assert np.isnan(res.worst_scale()).all() and np.all(res.base_rates("fake") == 0) and np.all(res.mse_random() == 0)
    s = res.summary()
    json.dumps(s, allow_nan=False)
    assert s["skill"] == [[[None] * 5]] * 3 and s["frequency_bias"] == [[None]] * 3 and s["worst_scale"] == [[None]] * 3
    assert s["energy_rel_diff"] == [[[None] * 5]] * 3 and s["mse"] == [[[0.0] * 5]] * 3


def test_all_ones_against_all_zeros_at_2048_carries_two_to_the_forty_four():
    N, n = 2048, 11
    a, b = np.ones((1, 1, N, N), F32), np.zeros((1, 1, N, N), F32)
    res = host_result(one_channel(), a, b)
    assert ints(res.sums()) == [v for l in range(n + 1) for v in (4 ** (n + l), 4 ** (n + l), 0)]
    assert int(res.sums()[0, 0, n, 0]) == 1 << 44 == iscale.bound(N, N)
    c = res.components()[0, 0, :, 0]
    assert c[:n].tolist() == [0.0] * n and c[n] == N * N                  # a constant field: the father component alone
    assert res.mse_random()[0, 0] == 1.0 and res.skill()[0, 0].tolist() == [1.0] * n + [1.0 - (n + 1)]


def test_derived_scores_on_hand_made_sums():
    spec = IscaleSpec(1, speed=None, thresholds=(1.0, 2.0))
    # a 2 x 2 grid, one field pair: one pixel each, in different places; then sums far beyond int64
    sums = [[[[2, 1, 1], [0, 1, 1]],
             [[3 << 70, 2 << 70, 1 << 70], [1 << 70, 4 << 70, 1 << 70]]]]
    res = IscaleResult(spec, 2, 2, sums, 1)
    assert res.n == 1 and res.padded_pixels == 4 and res.scales_px == (1, 2)
    assert res.components()[0, 0].tolist() == [[2.0, 0.75, 0.75], [0.0, 0.25, 0.25]]
    assert res.mse()[0, 0].tolist() == [0.5, 0.0] and res.mse_random()[0, 0] == 0.375
    assert res.energy("real")[0, 0].tolist() == [0.1875, 0.0625] and res.base_rates("real")[0, 0] == 0.25
    sk = res.skill()[0, 0]
    assert sk.tolist() == [-5 / 3, 1.0]                                # 1 - 2 * (1/2) / (3/8), rounded once
    assert sk.mean() == pytest.approx(1 - 0.5 / 0.375, rel=1e-15)        # mean_l SS_l = 1 - MSE / MSE_random
    assert res.worst_scale()[0, 0] == 1.0 and res.energy_rel_diff()[0, 0].tolist() == [0.0, 0.0]
    assert res.frequency_bias().tolist() == [[1.0, 0.5]]
    assert ints(res.sums()[0, 1, 0]) == [3 << 70, 2 << 70, 1 << 70] and res.fields == 1
    s = res.summary()
    assert json.loads(json.dumps(s, allow_nan=False)) == s
    assert s["sums"] == sums and s["scales_px"] == [1, 2] and s["levels"] == 2 and s["grid"] == [2, 2] and s["fields"] == 1
    assert s["skill"][0][0] == sk.tolist() and s["channels"] == ["ch0"] and s["thresholds"] == [[1.0, 2.0]]
    # the identity on a random pair: sum_l SS_l = (n + 1) (1 - MSE / MSE_random), and the components sum to the level-0 sums
    rng = np.random.default_rng(9)
    a, b = gauss_pair(rng, 3, 2, 20, 37)
    zs = IscaleSpec.zscore(2)
    r = host_result(zs, a, b)
    mse = np.array([[int(v) for v in row] for row in r.sums()[:, :, 0, 0]], dtype=np.float64) / r.padded_pixels
    np.testing.assert_allclose(r.skill().mean(axis=2), 1 - mse / r.mse_random(), rtol=1e-12)
    np.testing.assert_allclose(r.components().sum(axis=2), r.sums()[:, :, 0].astype(np.float64), rtol=1e-12)
    assert r.padded_pixels == 3 * 64 * 64
    want_random = r.base_rates("fake") * (1 - r.base_rates("real")) + r.base_rates("real") * (1 - r.base_rates("fake"))
    np.testing.assert_allclose(r.mse_random(), want_random, rtol=1e-12)
    with pytest.raises(ValueError, match="side"):
        r.energy("both")


def test_special_values():
    """NaN is false, +inf true, -inf false (its speed is +inf: true), equality with the threshold false (the speed of a (3, 4)
    pair is exactly 5)."""
    spec = IscaleSpec(2, thresholds=[[0.5, 1.0], [0.5, 1.0], [5.0, 1.0]])
    one = np.zeros((1, 2, 7, 13), F32)
    one[0, 0, 0, 0], one[0, 1, 0, 0] = 3.0, 4.0
    one[0, 0, 1, 1], one[0, 0, 2, 2], one[0, 1, 3, 3], one[0, 1, 4, 4] = np.inf, np.nan, -0.0, -np.inf
    one[0, 0, 5, 5], one[0, 0, 5, 6], one[0, 0, 5, 7] = 0.5, np.nextafter(F32(0.5), F32(1)), np.nextafter(F32(0.5), F32(0))
    s = host_sums(spec, one, one)
    assert s[:, :, 0, 1].tolist() == [[3, 2], [1, 1], [2, 3]] and np.array_equal(s[..., 1], s[..., 2]) and not s[..., 0].any()
    want, _ = iscale_ref(spec, one, one)
    assert ints(s) == ints(want)


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
    (dict(C=2, names=["a", "b"]), "names"),
])
def test_spec_is_checked(monkeypatch, kw, match):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=match):
        IscaleSpec(**kw)


def test_constructors():
    z = IscaleSpec.zscore(2)
    assert (z.C, z.nout, z.speed, z.K, z.names) == (2, 3, (0, 1), 2, ["ch0", "ch1", "speed"])
    assert z.thresholds.tolist() == [[1.0, 2.0]] * 3 and iscale.DEFAULT_THRESHOLDS == (1.0, 2.0)
    one = IscaleSpec.zscore(1, thresholds=(0.5,))
    assert one.speed is None and one.nout == 1 and one.K == 1
    stats = {"u10": (0.5, 3.0), "v10": (-0.25, 2.0), "t2m": (280.0, 10.0)}
    p = IscaleSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [15.0]])
    assert p.speed == (1, 2) and p.names == ["t2m", "u10", "v10", "speed"]
    assert p.scale.tolist() == [10.0, 3.0, 2.0] and p.offset.tolist() == [280.0, 0.5, -0.25]
    assert p == IscaleSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [15.0]]) and p != z
    assert p != IscaleSpec.physical(stats, ["t2m", "u10", "v10"], thresholds=[[300.0], [10.0], [10.0], [16.0]])
    assert IscaleSpec(2, thresholds=(0.1,)).thresholds[0, 0] == F32(0.1)          # rounded to fp32
    s = p.struct()
    assert (s.speed_u, s.speed_v, s.nthr) == (1, 2, 1) and s.thr[3][0] == 15.0 and s.scale[2] == 2.0 and s.offset[0] == 280.0
    n = IscaleSpec(2, speed=None).struct()
    assert (n.speed_u, n.speed_v, n.nthr) == (-1, -1, 2)


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
    spec = IscaleSpec.zscore(2)
    good = torch.zeros(2, 2, 8, 8)
    acc = IntensityScale(spec, 8, 8, device="cpu")
    with pytest.raises(err, match=match):
        acc.add(good, x, nhwc=(False, kw.get("nhwc", False)), channels=kw.get("channels"))
    with pytest.raises(err, match=match):
        acc.add(x, good, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))
    if "grid" not in match:                                               # the one-shot form takes the grid from the fields
        with pytest.raises(err, match=match):
            iscale.intensity_scale(x, good, spec=spec, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))


def test_accumulator_checks(monkeypatch):
    _no_library(monkeypatch)
    spec = IscaleSpec.zscore(2)
    x = torch.zeros(2, 2, 8, 8)
    acc = IntensityScale(spec, 8, 8, device="cpu")
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            acc.add(x, x, n_valid=n)
    with pytest.raises(ValueError, match="differ in length"):
        acc.add(x, torch.zeros(3, 2, 8, 8))
    with pytest.raises(ValueError, match="pair"):
        acc.add(x, x, nhwc=(True, False, True))
    with pytest.raises(TypeError, match="IscaleSpec"):
        IntensityScale(histograms.HistSpec.zscore(2), 8, 8, device="cpu")
    with pytest.raises(TypeError, match="IscaleSpec"):
        iscale.intensity_scale(x, x, spec=histograms.HistSpec.zscore(2))
    for H, W in ((0, 8), (8, 2049)):
        with pytest.raises(ValueError, match="grid"):
            IntensityScale(spec, H, W, device="cpu")
    assert acc.fields == 0 and acc._dev_sums.shape == (3, 2, 4, 3) and acc._dev_sums.dtype == torch.int64
    assert acc.result().fields == 0 and IntensityScale(spec, 65, 33, device="cpu")._dev_sums.shape == (3, 2, 8, 3)


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_iscale_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert re.search(r"#define DG_ISCALE_MAX_THR 4\b", src) and re.search(r"#define DG_ISCALE_MAX_LEVELS 12\b", src)
    assert re.search(r"#define DG_ISCALE_MAX_SIDE 2048\b", src) and "Intensity-scale verification (csrc/iscale.hip)" in src
    for sym in ("dg_iscale_levels", "dg_iscale_bound", "dg_iscale_ws_bytes", "dg_iscale", "dg_iscale_host"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    assert (_lib.ISCALE_MAX_THR, _lib.ISCALE_MAX_LEVELS, _lib.ISCALE_MAX_SIDE) == (iscale.THR_MAX, iscale.LEVELS_MAX, iscale.SIDE_MAX) == (4, 12, 2048)
    assert "iscale.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()


def test_iscale_spec_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.IscaleSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(dg_iscale_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_iscale_spec, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("thr_row %zu\\n", sizeof(((dg_iscale_spec*)0)->thr[0]));', '  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert int(got["thr_row"]) == 4 * _lib.ISCALE_MAX_THR


def test_abi_rejects_bad_arguments_without_launching():
    """Every pointer is a made-up address: a call that passed the checks would fault instead of returning a status."""
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    good = IscaleSpec.zscore(2).struct()

    def spec(**kw):
        s = IscaleSpec.zscore(2).struct()
        for k, v in kw.items():
            if isinstance(v, tuple) and len(v) == 3:
                getattr(s, k)[v[0]][v[1]] = v[2]
            elif isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    ws, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    call = lambda fa, fb, s, H=10, W=10, w=ws, o=out: lib.dg_iscale(fa, fb, H, W, s, w, o, None, None)
    g = C.byref(good)
    assert call(f(base=0), f(), g) == -1 and call(f(), f(base=0), g) == -1 and call(None, f(), g) == -1 and call(f(), None, g) == -1
    assert call(f(C=9), f(C=9), g) == -1 and call(f(T=0), f(T=0), g) == -1 and call(f(ld_t=-1), f(), g) == -1
    assert call(f(), f(T=3), g) == -1 and call(f(), f(P=96), g) == -1 and call(f(C=3), f(C=2), g) == -1     # T / C / P differ
    assert call(f(), f(), g, H=10, W=9) == -1 and call(f(), f(), g, H=0, W=10) == -1                          # P != H * W
    assert call(f(P=2049), f(P=2049), g, H=1, W=2049) == -1 and call(f(P=2049), f(P=2049), g, H=2049, W=1) == -1
    assert call(f(), f(), None) == -1
    assert call(f(), f(), g, w=None) == -1 and call(f(), f(), g, o=None) == -1
    for bad in (dict(nthr=0), dict(nthr=5), dict(speed_u=2), dict(speed_v=-1), dict(scale=(1, float("inf"))),
                dict(offset=(0, float("nan"))), dict(thr=(2, 1, float("inf"))), dict(thr=(0, 0, float("nan")))):
        assert call(f(), f(), spec(**bad)) == -1, bad
        assert lib.dg_iscale_ws_bytes(f(), 10, 10, spec(**bad)) == 0, bad
    assert call(f(C=1), f(C=1), g) == -1                                 # speed channel 1 of a 1-channel field
    assert call(f(dtype=7), f(), g) == -2 and call(f(), f(dtype=7), g) == -2
    # T * bound > 2^62: 2^18 fields of 2048 x 2048 are the most one call takes
    big = dict(P=2048 * 2048, ld_c=0, ld_t=0)
    assert lib.dg_iscale_ws_bytes(f(T=1 << 18, **big), 2048, 2048, g) > 0
    assert call(f(T=(1 << 18) + 1, **big), f(T=(1 << 18) + 1, **big), g, H=2048, W=2048) == -1
    assert lib.dg_iscale_ws_bytes(f(T=(1 << 18) + 1, **big), 2048, 2048, g) == 0
    # the workspace: per-field slots and one 4-byte total per (t, j, k, tile) -- nothing per pixel
    m = dict(P=1 << 20, ld_c=1 << 20, ld_t=2 << 20)
    four = lib.dg_iscale_ws_bytes(f(T=4, **m), 1024, 1024, g)
    assert 4 * 6 * (11 * 3 * 8 + 256 * 4) <= four <= 4 * 6 * (11 * 3 * 8 + 256 * 4) + 512 < (1 << 20) // 8
    assert 0 < lib.dg_iscale_ws_bytes(f(), 10, 10, g) <= 4 * 6 * (5 * 3 * 8 + 4) + 512
    assert lib.dg_iscale_ws_bytes(f(C=9), 10, 10, g) == 0 and lib.dg_iscale_ws_bytes(f(), 10, 9, g) == 0


def test_bound_and_levels_are_their_formulas():
    lib = _lib.lib()
    for H, W in [(1, 1), (1, 2), (2, 1), (3, 3), (5, 3), (16, 16), (17, 16), (64, 64), (65, 33), (128, 128), (72, 200), (1024, 1024),
                 (1025, 7), (2048, 2048), (1, 2048), (2047, 2)]:
        n = next(k for k in range(12) if 2 ** k >= max(H, W))
        assert iscale.log_side(H, W) == n and lib.dg_iscale_levels(H, W) == n + 1 <= _lib.ISCALE_MAX_LEVELS
        assert lib.dg_iscale_bound(H, W) == iscale.bound(H, W) == 16 ** n
    assert lib.dg_iscale_bound(2048, 2048) == 1 << 44 and lib.dg_iscale_levels(2048, 2048) == 12
    for H, W in [(0, 5), (5, 0), (2049, 5), (5, 2049), (-1, 4)]:
        assert lib.dg_iscale_bound(H, W) == 0 and lib.dg_iscale_levels(H, W) == 0, (H, W)


# ------------------------------------------------------------------------------------------------- emulated ops
RECORD = []                  # (real, fake) float32 [T, C, H, W] of every emulated dg_iscale call of this process


def iscale_emu_ops():
    from oracle.emu_ops import EmuOps

    class IscaleEmuOps(EmuOps):
        """The emulated ops plus dg_iscale's contract in numpy (the oracle)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            P = t.shape[1] * t.shape[2] if nhwc else t.shape[2] * t.shape[3]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=P)

        def iscale_ws_bytes(self, f, H, W, spec):
            return 1

        def iscale(self, fa, fb, H, W, s, sums, per_field=None):
            def values(f):
                x = f.t[..., :f.C].permute(0, 3, 1, 2) if f.nhwc else f.t[:, :f.C]
                return x.detach().float().cpu().numpy().copy()
            speed = None if s.speed_u < 0 else (s.speed_u, s.speed_v)
            nout = fa.C + (speed is not None)
            spec = types.SimpleNamespace(nout=nout, K=s.nthr, speed=speed, scale=np.array(s.scale[:fa.C], F32),
                                         offset=np.array(s.offset[:fa.C], F32),
                                         thresholds=np.array([list(s.thr[j])[:s.nthr] for j in range(nout)], F32).reshape(nout, s.nthr))
            a, b = values(fa), values(fb)
            assert a.shape[2:] == (H, W) and fa.T * iscale.bound(H, W) <= 1 << 62
            RECORD.append((a, b))
            S, per = iscale_ref(spec, a, b)
            sums += torch.from_numpy(S.astype(np.int64))
            if per_field is not None:
                per_field.copy_(torch.from_numpy(per.astype(np.int64)))

    return IscaleEmuOps("f32")


def _pairs(rng, sizes, H=8, W=8):
    out = []
    for n in sizes:
        a = rng.standard_normal((n, 2, H, W)).astype(F32)
        out.append((torch.from_numpy(a), torch.from_numpy(np.roll(a, 1, axis=3) + 0.3 * rng.standard_normal(a.shape).astype(F32))))
    return out


def test_draining_and_chunking_leave_the_totals_unchanged(monkeypatch):
    rng = np.random.default_rng(6)
    spec = IscaleSpec.zscore(2, thresholds=(0.0, 1.0))
    batches = _pairs(rng, (2, 2, 6, 2, 2, 1))
    ops = iscale_emu_ops()

    def run():
        acc = IntensityScale(spec, 8, 8, device="cpu", ops=ops)
        calls = len(RECORD)
        for a, b in batches:
            acc.add(a, b)
        return acc, acc.result(), [r[0].shape[0] for r in RECORD[calls:]]
    acc, plain, sizes = run()
    assert sizes == [2, 2, 6, 2, 2, 1] and acc.drains == 1               # one call per batch, drained once by result()
    mb = iscale.bound(8, 8)
    assert acc._bound == mb == 16 ** 3
    monkeypatch.setattr(iscale, "DRAIN_LIMIT", 4 * mb)                   # room for four fields on the device
    acc2, low, sizes2 = run()
    assert sizes2 == [2, 2, 4, 2, 2, 2, 1]                               # the batch of 6 is cut into 4 + 2
    assert acc2.drains >= 4                                              # ... and at least every second add drains first
    assert ints(low.sums()) == ints(plain.sums()) and low.fields == plain.fields == 15
    a, b = torch.cat([p[0] for p in batches]), torch.cat([p[1] for p in batches])
    S, _ = iscale_ref(spec, a.numpy(), b.numpy())
    assert ints(plain.sums()) == ints(S)
    monkeypatch.setattr(iscale, "DRAIN_LIMIT", 1)                        # below one field's bound: one field per call
    acc3, one, sizes3 = run()
    assert sizes3 == [1] * 15 and ints(one.sums()) == ints(plain.sums())
    # the workspace cap cuts a batch as well
    monkeypatch.setattr(iscale, "DRAIN_LIMIT", 1 << 62)
    monkeypatch.setattr(ops, "iscale_ws_bytes", lambda f, H, W, s: 100 * f.T)
    monkeypatch.setattr(iscale, "WS_CAP", 350)                           # three fields per call
    acc5, capped, sizes5 = run()
    assert sizes5 == [2, 2, 3, 3, 2, 2, 1] and ints(capped.sums()) == ints(plain.sums())
    # n_valid: the padding fields are not read
    acc4 = IntensityScale(spec, 8, 8, device="cpu", ops=ops)
    junk = torch.full((3, 2, 8, 8), 9.0)
    for a_, b_ in batches:
        acc4.add(torch.cat([a_, junk[:2]]), torch.cat([b_, -junk[:2]]), n_valid=a_.shape[0])
    assert ints(acc4.result().sums()) == ints(plain.sums()) and acc4.fields == 15
    # the one-shot form, in NHWC with padded channels on one side
    nh = torch.full((15, 8, 8, 5), float("nan"))
    nh[..., :2] = b.permute(0, 2, 3, 1)
    once = iscale.intensity_scale(a, nh, spec=spec, nhwc=(False, True), channels=2, ops=ops)
    assert ints(once.sums()) == ints(plain.sums()) and once.summary() == plain.summary()


def _rank_pairs(rank, world):
    rng = np.random.default_rng(21)
    (a, b), = _pairs(rng, (6,), H=12, W=20)
    return a[rank::world], b[rank::world]


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    a, b = _rank_pairs(rank, world)
    acc = IntensityScale(IscaleSpec.zscore(2, thresholds=(0.0, 1.0)), 12, 20, device="cpu", ops=iscale_emu_ops())
    acc._sums[0] += (1 << 70) + rank                                     # a total beyond int64 survives the limb all-reduce
    res = acc.add(a, b).reduce_(d).result()
    torch.save({"sums": ints(res.sums()), "fields": res.fields, "summary": res.summary()}, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_sums():
    a, b = _rank_pairs(0, 1)
    spec = IscaleSpec.zscore(2, thresholds=(0.0, 1.0))
    ref = iscale.intensity_scale(a, b, spec=spec, ops=iscale_emu_ops())
    want = ints(ref.sums())
    assert want == ints(iscale_ref(spec, a.numpy(), b.numpy())[0])
    want[0] += (2 << 70) + 1
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0 == r1 and r0["sums"] == want and r0["fields"] == 6


# ------------------------------------------------------------------------------------------------- the trainer's hook
@pytest.fixture
def ilog(log, monkeypatch):  # noqa: F811
    """The recording stubs of test_trainer_hooks_cpu, and one more for the thirteenth accumulator."""
    monkeypatch.setattr(iscale, "IntensityScale", _stub(log, "IntensityScale"))
    return log


def test_the_hook_is_off_by_default_and_changes_nothing(ilog):
    from downgan_amd.engine import METRIC_SINKS
    from downgan_amd.GAN.wasserstein import HOOKS, WassersteinGAN
    assert WassersteinGAN.log_intensity_scale is False and WassersteinGAN.intensity_scale_spec is None
    assert WassersteinGAN.intensity_scale_results is None
    assert METRIC_SINKS[-1] == ("intensity_scale", False) and [n for n, _ in METRIC_SINKS[:-1]] == sorted({k for k, _, _ in FEED}, key=[k for k, _, _ in FEED].index)
    assert [h.key for h in HOOKS] == list(KEYS) + ["intensity_scale"] and HOOKS[-1].flag == "log_intensity_scale"
    bare = _trainer(None)
    _run(bare)
    off = _trainer(None, log_intensity_scale=False)
    _run(off)
    assert ilog.made == [] and len(ilog.passes) == 6                      # the constructor log stays empty
    assert all(p["adds"] == [] and p["kw"].get("intensity_scale") is None for p in ilog.passes)
    a, b = bare.metrics_log[0], off.metrics_log[0]
    assert list(a) == list(b) == ["epoch", "train", "test", "test_batches"]
    assert json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True) and off.intensity_scale_results is None


@pytest.mark.parametrize("fs", [False, True])
@pytest.mark.parametrize("log_metrics", [True, False])
def test_the_hook_on_its_own(ilog, fs, log_metrics):
    from downgan_amd.GAN.wasserstein_fs import WassersteinGANFS
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    if fs:
        tr = WassersteinGANFS(Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2))
    else:
        tr = _trainer(None)
    tr.log_intensity_scale, tr.log_metrics = True, log_metrics
    tl = _run(tr)
    assert tl.walks == 1
    made = ilog.of("IntensityScale")
    assert len(ilog.made) == len(made) == 2                               # one accumulator per part, nothing else
    for _, _, args, kw in made:
        assert args == (IscaleSpec.zscore(2), 128, 128) and kw == {"device": torch.device("cpu")}
    assert len(ilog.passes) == 3
    for p, acc in zip(ilog.passes, (made[0][1], made[1][1], made[1][1])):
        assert [k for k, v in p["kw"].items() if v is not None] == ["intensity_scale"] and p["kw"]["intensity_scale"] is acc
        (stub, tensors, kw), = p["adds"]
        assert stub is acc and tensors[0] is p["fine"] and tensors[1] is p["engine"].G.fake and len(tensors) == 2
        assert kw == {"n_valid": 2, "nhwc": True, "channels": 2}
    s = tr.metrics_log[0]
    assert list(s) == (["epoch", "train", "test", "test_batches"] if log_metrics else ["epoch"]) + ["intensity_scale"]
    assert list(s["intensity_scale"]) == ["train", "test"] == list(tr.intensity_scale_results)
    for part, (_, acc, _, _) in zip(("train", "test"), made):
        assert tr.intensity_scale_results[part] is acc.res
        assert s["intensity_scale"][part] == {"stub": "IntensityScale", "serial": acc.serial, "args": []}
    assert [(a.name, d) for a, d in ilog.reduced] == [("IntensityScale", None)] * 2 and ilog.saved == []


def test_with_every_hook_on_it_is_fed_after_distances_and_reported_last(ilog):
    from .test_trainer_hooks_cpu import FLAGS
    spec = IscaleSpec(2, speed=None, thresholds=(0.5,))
    tr = _trainer(True, log_intensity_scale=True, intensity_scale_spec=spec)
    _run(tr)
    assert all(a[0] is spec for _, _, a, _ in ilog.of("IntensityScale")) and len(ilog.of("IntensityScale")) == 2
    assert len(ilog.made) == 27 + 2
    for p, part in zip(ilog.passes, ("train", "test", "test")):
        names = [a[0].name for a in p["adds"]]
        assert names[-2:] == ["Distances", "IntensityScale"] and names.count("IntensityScale") == 1
        assert len(names) == (15 if part == "test" else 14)
        assert list(p["kw"])[-1] == "intensity_scale"
        fine, fake = p["adds"][-1][1]
        assert fine is p["fine"] and fake is p["engine"].G.fake
    s = tr.metrics_log[0]
    assert list(s) == ["epoch", "train", "test", "test_batches"] + list(KEYS) + ["intensity_scale"]
    assert set(tr.intensity_scale_results) == {"train", "test"}
    # the results stay while the flag is off, and are replaced when it is on again
    kept = tr.intensity_scale_results
    for f in FLAGS + ("log_intensity_scale",):
        setattr(tr, f, False)
    dl, tl = _loaders()
    tr._train_epoch(dl, tl, epoch=1)
    assert list(tr.metrics_log[1]) == ["epoch", "train", "test", "test_batches"] and tr.intensity_scale_results is kept


def test_the_hook_with_numbers_on_the_emulated_ops(monkeypatch):
    """The real accumulator under the trainer, the ops method emulated in numpy: the summary is that of the pairs it was fed."""
    import downgan_amd.config.hyperparams as hp
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    monkeypatch.setattr(backend, "make_ops", lambda dtype, device: iscale_emu_ops())
    monkeypatch.setattr(losses, "_ops", {})
    monkeypatch.setattr(histograms, "_ops", {})
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    n0 = len(RECORD)
    tr = _trainer(None, log_intensity_scale=True)
    _run(tr)
    recs = RECORD[n0:]
    assert [r[0].shape for r in recs] == [(2, 2, 128, 128)] * 3           # one train batch, two test batches, one call each
    d = tr.metrics_log[0]["intensity_scale"]
    assert json.loads(json.dumps(d, allow_nan=False)) == d and list(tr.metrics_log[0])[-1] == "intensity_scale"
    spec = IscaleSpec.zscore(2)
    for part, rec, n in (("train", recs[:1], 2), ("test", recs[1:], 4)):
        a, b = np.concatenate([r[0] for r in rec]), np.concatenate([r[1] for r in rec])
        S, _ = iscale_ref(spec, a, b)
        got = tr.intensity_scale_results[part]
        assert ints(got.sums()) == ints(S) and got.fields == n and d[part] == got.summary()
        assert d[part]["levels"] == 8 and d[part]["scales_px"] == [1, 2, 4, 8, 16, 32, 64, 128] and d[part]["grid"] == [128, 128]
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    np.testing.assert_array_equal(np.concatenate([r[0] for r in recs[1:]]), fine[2:6])     # the real side is the test set


def test_importing_the_trainer_does_not_import_the_module():
    import sys
    code = "import sys, downgan_amd.GAN.wasserstein, downgan_amd.engine\nprint('downgan_amd.iscale' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, capture_output=True, text=True).stdout
    assert out.strip() == "False"
