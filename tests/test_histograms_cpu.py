"""Value histograms without a GPU: the library's host bin rule against numpy float32 on adversarial values, argument checks
that fire before any library call, the ABI surface and struct layout, known answers of the derived statistics (quantiles, W1,
KS, exceedance), and the trainer's opt-in hook on the emulated ops (a test-local op class adds a numpy ``hist`` under the usual
make_ops patch), in one process, over 2 gloo ranks, and in the frequency-separation trainer."""
import ctypes as C
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

from downgan_amd import _lib, histograms
from downgan_amd.histograms import HistSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------------------------------------------- the definition in numpy
def transform_ref(spec, x):
    """x float32 [C, n] -> the nout output values float32 [nout, n] (affine, then the speed of the pair)."""
    x = np.asarray(x, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (x * spec.scale[:, None]).astype(F32)
        y = (y + spec.offset[:, None]).astype(F32)
        outs = list(y)
        if spec.speed is not None:
            u, v = y[spec.speed[0]], y[spec.speed[1]]
            outs.append(np.sqrt((u * u).astype(F32) + (v * v).astype(F32)).astype(F32))
    return np.stack(outs)


def bins_ref(spec, x):
    """int64 [nout, n]: 0 underflow, 1 .. bins interior, bins + 1 overflow, bins + 2 NaN (numpy float32, the contract)."""
    y = transform_ref(spec, x)
    out = np.empty(y.shape, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(spec.nout):
            t = ((y[j] - spec.lo[j]).astype(F32) * spec.inv_w[j]).astype(F32)
            inner = np.where((t >= 0) & (t < spec.bins), t, 0).astype(np.int64) + 1
            out[j] = np.where(np.isnan(t), spec.bins + 2, np.where(t < 0, 0, np.where(t >= spec.bins, spec.bins + 1, inner)))
    return out


def hist_ref(spec, x):
    """counts int64 [nout, bins + 3], moments float64 [nout, 2], extrema float32 [nout, 2] of x float32 [C, n]."""
    y, b = transform_ref(spec, x), bins_ref(spec, x)
    counts = np.stack([np.bincount(b[j], minlength=spec.bins + 3) for j in range(spec.nout)])
    mom = np.zeros((spec.nout, 2))
    ext = np.array([[np.inf, -np.inf]] * spec.nout, dtype=F32)
    for j in range(spec.nout):
        f = y[j][np.isfinite(y[j])].astype(np.float64)
        mom[j] = f.sum(), (f * f).sum()
        if f.size:
            ext[j] = f.min(), f.max()
    return counts, mom, ext


def edge_values(lo, w, k):
    """lo + k w and its two fp32 neighbours, for every k."""
    e = (F32(lo) + np.arange(k + 1, dtype=np.float64) * w).astype(F32)
    return np.concatenate([e, np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf))])


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(F32).max, -np.finfo(F32).max, np.finfo(F32).tiny,
                    -np.finfo(F32).tiny, 1e-45, -1e-45, 3e-39, -3e-39, np.nextafter(F32(0), F32(1)) * 7], dtype=F32)


# ------------------------------------------------------------------------------------------------- the host bin rule
def test_exact_edges_and_their_neighbours():
    spec = HistSpec(2048, [-8.0], [8.0], speed=None)
    assert spec.inv_w[0] == 128.0
    x = np.concatenate([edge_values(-8.0, 1 / 128, 2048), SPECIAL])[None]
    got = histograms.host_bins(spec, x)
    np.testing.assert_array_equal(got, bins_ref(spec, x))
    e = (F32(-8.0) + np.arange(2048, dtype=np.float64) / 128).astype(F32)
    np.testing.assert_array_equal(histograms.host_bins(spec, e[None])[0], np.arange(1, 2049))     # each edge opens its bin


def test_unrepresentable_inverse_width():
    spec = HistSpec(1000, [-1.0, 0.5], [2.0, 3.5], speed=None)
    assert float(spec.inv_w[0]) != 1000 / 3
    x = np.stack([np.concatenate([edge_values(-1.0, 3 / 1000, 1000), SPECIAL]),
                  np.concatenate([edge_values(0.5, 3 / 1000, 1000), SPECIAL])])
    np.testing.assert_array_equal(histograms.host_bins(spec, x), bins_ref(spec, x))


def test_zero_subnormals_infinities_nan_and_scaled_overflow():
    spec = HistSpec(16, [0.0, 0.0, 0.0], [1e-37, 1.0, 2.0], scale=[1.0, 2.0], offset=[0.0, -0.0])
    tiny = np.array([0.0, -0.0, 1e-45, 2e-45, 1e-40, 1e-38, -1e-45, -1e-40], dtype=F32)
    x = np.concatenate([tiny, SPECIAL])
    x = np.stack([x, x[::-1].copy()])
    got = histograms.host_bins(spec, x)
    np.testing.assert_array_equal(got, bins_ref(spec, x))
    fmax = histograms.host_bins(spec, np.array([[1.0], [np.finfo(F32).max]], dtype=F32))
    assert fmax[1, 0] == spec.bins + 1                                   # FLT_MAX * 2 = inf: overflow, not NaN
    assert got[0, 1] == got[0, 0] == 1                                   # -0 is +0
    assert (got[:, np.isnan(x[0])][0] == spec.bins + 2).all()


def test_random_values_with_affine_and_speed():
    rng = np.random.default_rng(3)
    spec = HistSpec(257, [-5.0, -3.0, -1.0, 0.0], [5.0, 3.0, 4.0, 9.0], scale=[1.7, 0.3, 2.5], offset=[0.1, -0.2, 3.0],
                    speed=(2, 0))
    x = (rng.standard_normal((3, 50000)) * 3).astype(F32)
    np.testing.assert_array_equal(histograms.host_bins(spec, x), bins_ref(spec, x))


# ------------------------------------------------------------------------------------------------- argument checks
def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("library or device touched before the arguments were checked")
    from downgan_amd import backend
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(backend, "make_ops", boom)
    monkeypatch.setattr(histograms, "_ops", {})


@pytest.mark.parametrize("kw,match", [
    (dict(bins=0, lo=[0.0], hi=[1.0], speed=None), "bins"),
    (dict(bins=4097, lo=[0.0], hi=[1.0], speed=None), "bins"),
    (dict(bins=2.5, lo=[0.0], hi=[1.0], speed=None), "bins"),
    (dict(bins=8, lo=[1.0], hi=[1.0], speed=None), "lo < hi"),
    (dict(bins=8, lo=[0.0], hi=[np.inf], speed=None), "finite"),
    (dict(bins=8, lo=[np.nan], hi=[1.0], speed=None), "finite"),
    (dict(bins=8, lo=[-1e39], hi=[1.0], speed=None), "fp32"),
    (dict(bins=8, lo=[0.0, 0.0], hi=[1.0], speed=None), "one value per output"),
    (dict(bins=8, lo=[0.0, 0.0], hi=[1.0, 1.0]), "speed"),                   # C = 1 and the default speed (0, 1)
    (dict(bins=8, lo=[0.0] * 3, hi=[1.0] * 3, speed=(0, 2)), "speed"),
    (dict(bins=8, lo=[0.0] * 10, hi=[1.0] * 10), "C <="),
    (dict(bins=8, lo=[0.0] * 3, hi=[1.0] * 3, scale=[1.0]), "scale"),
    (dict(bins=4096, lo=[0.0], hi=[1e-42], speed=None), "bin width"),
    (dict(bins=8, lo=[0.0], hi=[1.0], speed=None, names=["a", "b"]), "names"),
])
def test_spec_is_checked(monkeypatch, kw, match):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=match):
        HistSpec(**kw)


@pytest.mark.parametrize("x,kw,err,match", [
    (torch.zeros(2, 3, 8, 8), {}, ValueError, "C = 2"),
    (torch.zeros(2, 9, 8, 8), {}, ValueError, "C <="),
    (torch.zeros(2, 8, 8, 4), {"nhwc": True, "channels": 5}, ValueError, "channels"),
    (torch.zeros(2, 8, 8, 4), {"nhwc": True}, ValueError, "C = 2"),
    (torch.zeros(2, 2, 8, 8, dtype=torch.float64), {}, TypeError, "fp32 or bf16"),
    (torch.zeros(2, 2, 8, 8, dtype=torch.float16), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 2, 8, 8), np.float32), {}, TypeError, "tensor"),
    (torch.zeros(2, 8, 8), {}, ValueError, "shape"),
    (torch.zeros(0, 2, 8, 8), {}, ValueError, "at least one"),
    (torch.zeros(2, 2, 0, 8), {}, ValueError, "at least one"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, x, kw, err, match):
    _no_library(monkeypatch)
    spec = HistSpec.zscore(2)
    with pytest.raises(err, match=match):
        histograms.histogram(x, spec, **kw)
    acc = histograms.ValueHistogram(spec, device="cpu")
    with pytest.raises(err, match=match):
        acc.add(x, **kw)
    with pytest.raises(TypeError, match="HistSpec"):
        histograms.histogram(torch.zeros(1, 2, 4, 4), None)


def test_accumulator_checks_n_valid(monkeypatch):
    _no_library(monkeypatch)
    acc = histograms.ValueHistogram(HistSpec.zscore(2), device="cpu")
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            acc.add(torch.zeros(2, 2, 8, 8), n_valid=n)
    with pytest.raises(TypeError):
        histograms.ValueHistogram([0.0, 1.0], device="cpu")


def test_constructors():
    z = HistSpec.zscore(2)
    assert (z.bins, z.C, z.nout, z.speed, z.names) == (2048, 2, 3, (0, 1), ["ch0", "ch1", "speed"])
    assert z.lo.tolist() == [-10.0, -10.0, 0.0] and z.hi[2] == F32(10 * np.sqrt(2))
    one = HistSpec.zscore(1)
    assert one.speed is None and one.nout == 1
    stats = {"u10": (0.5, 3.0), "v10": (-0.25, 2.0), "t2m": (280.0, 10.0)}
    p = HistSpec.physical(stats, ["t2m", "u10", "v10"], -40.0, 40.0, bins=800)
    assert p.speed == (1, 2) and p.names == ["t2m", "u10", "v10", "speed"]
    assert p.scale.tolist() == [10.0, 3.0, 2.0] and p.offset.tolist() == [280.0, 0.5, -0.25]
    assert p.hi[3] == F32(40 * np.sqrt(2)) and p.lo[3] == 0.0
    np.testing.assert_allclose(p.edges()[0, [0, -1]], [-40.0, 40.0])
    assert p == HistSpec.physical(stats, ["t2m", "u10", "v10"], -40.0, 40.0, bins=800) and p != z


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_hist_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert re.search(r"#define DG_HIST_MAX_BINS 4096\b", src) and re.search(r"#define DG_HIST_MAX_OUT \(DG_EOF_MAX_C \+ 1\)", src)
    for sym in ("dg_hist_ws_bytes", "dg_hist", "dg_hist_host_bins"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    assert _lib.HIST_MAX_BINS == histograms.BINS_MAX == 4096 and _lib.HIST_MAX_OUT == 9


def test_hist_spec_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.HistSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(dg_hist_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_hist_spec, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    good = HistSpec.zscore(2).struct()

    def spec(**kw):
        s = HistSpec.zscore(2).struct()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    ws, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    call = lambda fx, s, w=ws: lib.dg_hist(fx, s, w, out, out, out, None)
    assert call(f(base=0), C.byref(good)) == -1
    assert call(f(C=9), C.byref(good)) == -1
    assert call(f(T=0), C.byref(good)) == -1
    assert call(f(P=0), C.byref(good)) == -1
    assert call(f(), C.byref(good), None) == -1
    assert call(f(), spec(nbins=0)) == -1 and call(f(), spec(nbins=4097)) == -1
    assert call(f(), spec(speed_u=2)) == -1 and call(f(), spec(speed_v=-1)) == -1
    assert call(f(), spec(inv_w=(2, 0.0))) == -1 and call(f(), spec(inv_w=(0, float("inf")))) == -1
    assert call(f(), spec(lo=(1, float("nan")))) == -1
    assert call(f(C=1), C.byref(good)) == -1                             # speed channel 1 of a 1-channel field
    assert call(f(dtype=7), C.byref(good)) == -2
    assert lib.dg_hist_ws_bytes(f(C=9), C.byref(good)) == 0 and lib.dg_hist_ws_bytes(f(), spec(nbins=0)) == 0
    assert 0 < lib.dg_hist_ws_bytes(f(), C.byref(good)) <= 1 << 20
    x = np.zeros((2, 4), F32)
    b = np.zeros((3, 4), np.int32)
    assert lib.dg_hist_host_bins(spec(nbins=0), x.ctypes.data, 2, 4, b.ctypes.data) == -1
    assert lib.dg_hist_host_bins(C.byref(good), None, 2, 4, b.ctypes.data) == -1


# ------------------------------------------------------------------------------------------------- derived statistics
def make_hist(spec, x, fields=1):
    """A Histogram of the values x float32 [C, n] built from the numpy definition (CPU tensors)."""
    counts, mom, ext = hist_ref(spec, x)
    return histograms.Histogram(spec, torch.from_numpy(counts), torch.from_numpy(mom), torch.from_numpy(ext), fields)


def test_wasserstein_of_a_shift_by_k_bins():
    spec = HistSpec(64, [-4.0], [4.0], speed=None)
    w = spec.width()[0]
    rng = np.random.default_rng(1)
    a = (-4.0 + (rng.integers(0, 40, 5000) + 0.5) * w).astype(F32)[None]
    for k in (1, 3, 17):
        b = (a + F32(k * w)).astype(F32)
        ha, hb = make_hist(spec, a), make_hist(spec, b)
        np.testing.assert_array_equal(hb.host()[0][0, 1 + k:-2], ha.host()[0][0, 1:-2 - k])
        np.testing.assert_allclose(histograms.wasserstein1(ha, hb), [k * w], rtol=1e-12)
        np.testing.assert_allclose(histograms.wasserstein1(hb, ha), [k * w], rtol=1e-12)
    assert histograms.wasserstein1(ha, ha).tolist() == [0.0]


def test_wasserstein_of_bin_centred_samples_is_the_sorted_difference():
    spec = HistSpec(128, [-2.0, 0.0], [2.0, 8.0], speed=None)
    w = spec.width()
    rng = np.random.default_rng(2)
    idx = lambda n, hi: rng.integers(0, hi, (2, n))
    cen = lambda i: (spec.lo[:, None].astype(np.float64) + (i + 0.5) * w[:, None]).astype(F32)
    a, b = cen(idx(3000, 128)), cen(idx(3000, 100))
    got = histograms.wasserstein1(make_hist(spec, a), make_hist(spec, b))
    want = [np.mean(np.abs(np.sort(a[j].astype(np.float64)) - np.sort(b[j].astype(np.float64)))) for j in range(2)]
    np.testing.assert_allclose(got, want, rtol=1e-9)


def test_ks_distance():
    spec = HistSpec(32, [0.0], [1.0], speed=None)
    a = np.full((1, 100), 0.1, F32)
    b = np.full((1, 70), 0.9, F32)
    assert histograms.ks_distance(make_hist(spec, a), make_hist(spec, b)).tolist() == [1.0]
    c = np.concatenate([a, np.full((1, 100), 0.9, F32)], axis=1)
    np.testing.assert_allclose(histograms.ks_distance(make_hist(spec, a), make_hist(spec, c)), [0.5], rtol=1e-12)
    with pytest.raises(ValueError, match="share"):
        histograms.ks_distance(make_hist(spec, a), make_hist(HistSpec(31, [0.0], [1.0], speed=None), a))


def test_quantiles_moments_and_range():
    spec = HistSpec(400, [-4.0, -4.0, 0.0], [4.0, 4.0, 6.0])
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 20000)).astype(F32)
    x[0, :30] = [9.0] * 10 + [-7.5] * 10 + [np.nan] * 10
    h = make_hist(spec, x)
    y = transform_ref(spec, x)
    fin = [yj[np.isfinite(yj)].astype(np.float64) for yj in y]
    q = np.array([0.0, 1e-4, 0.01, 0.1, 0.5, 0.9, 0.99, 0.9999, 1.0])
    got = h.quantile(q)
    assert got.shape == (3, len(q))
    for j in range(3):
        assert got[j, 0] == fin[j].min() and got[j, -1] == fin[j].max()
        want = np.quantile(fin[j], q, method="inverted_cdf")
        inside = (want >= spec.lo[j]) & (want < spec.hi[j])
        assert np.all(np.abs(got[j] - want)[inside] <= spec.width()[j] * (1 + 1e-6)), (j, got[j], want)
    assert h.quantile(0.5).shape == (3,)
    np.testing.assert_allclose(h.mean(), [f.mean() for f in fin], rtol=1e-12)
    np.testing.assert_allclose(h.std(), [f.std() for f in fin], rtol=1e-9)
    assert h.min().tolist() == [f.min() for f in fin] and h.max().tolist() == [f.max() for f in fin]
    assert h.nan().tolist() == [10, 0, 10]
    assert h.out_of_range()[0].tolist() == [10 + int((x[0, 30:] < -4).sum()), 10 + int((x[0, 30:] >= 4).sum())]
    assert h.finite().tolist() == [len(f) for f in fin]
    with pytest.raises(ValueError, match="quantile"):
        h.quantile(1.5)


def test_exceedance_of_a_distribution_against_itself():
    spec = HistSpec.zscore(2, bins=2048, lim=6.0)
    rng = np.random.default_rng(5)
    h = make_hist(spec, rng.standard_normal((2, 400000)).astype(F32))
    qs = (0.9, 0.99, 0.999, 0.9999)
    got = histograms.exceedance(h, h, qs)
    assert got.shape == (3, 4)
    np.testing.assert_allclose(got, np.broadcast_to(1 - np.array(qs), (3, 4)), rtol=1e-6, atol=1e-12)
    wide = make_hist(spec, 2 * rng.standard_normal((2, 400000)).astype(F32))
    assert np.all(histograms.exceedance(h, wide, qs) > 1 - np.array(qs))          # a wider fake exceeds the real tails


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def hist_emu_ops():
    from oracle.emu_ops import EmuOps

    class HistEmuOps(EmuOps):
        """The emulated ops plus dg_hist's contract in numpy (float32 bin rule, float64 moments)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=t.shape[1] * t.shape[2])

        def hist_ws_bytes(self, f, spec):
            return 1

        def hist(self, f, s, counts, moments, extrema):
            x = f.t[..., :f.C].permute(3, 0, 1, 2) if f.nhwc else f.t[:, :f.C].permute(1, 0, 2, 3)
            x = x.detach().float().cpu().numpy().reshape(f.C, -1)
            speed = None if s.speed_u < 0 else (s.speed_u, s.speed_v)
            nout = f.C + (speed is not None)
            spec = types.SimpleNamespace(bins=s.nbins, nout=nout, speed=speed, lo=np.array(s.lo[:nout], F32),
                                         inv_w=np.array(s.inv_w[:nout], F32), scale=np.array(s.scale[:f.C], F32),
                                         offset=np.array(s.offset[:f.C], F32))
            c, m, e = hist_ref(spec, x)
            counts += torch.from_numpy(c)
            moments += torch.from_numpy(m)
            extrema[:, 0] = torch.minimum(extrema[:, 0], torch.from_numpy(e[:, 0]))
            extrema[:, 1] = torch.maximum(extrema[:, 1], torch.from_numpy(e[:, 1]))

    return HistEmuOps("f32")


def _trainer(log_distributions, dist=None, fs=False):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.GAN.wasserstein_fs import WassersteinGANFS
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = (WassersteinGANFS if fs else WassersteinGAN)(G, C_, dist=dist)
    tr.log_distributions = log_distributions
    return tr


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: hist_emu_ops())
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


def _run_epoch(log_distributions, dist=None, lo=0, step=1, batch=2, fs=False):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(log_distributions, dist, fs)
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr


SIDE_KEYS = {"quantiles", "mean", "std", "min", "max", "out_of_range", "nan"}


def test_log_distributions_off_leaves_the_summary_unchanged(monkeypatch):
    import json

    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_distributions is False and WassersteinGAN.distribution_spec is None
    off = _run_epoch(False).metrics_log[0]
    tr = _run_epoch(True)
    on = dict(tr.metrics_log[0])
    assert "distributions" not in off
    d = on.pop("distributions")
    assert on == off                                      # the hook adds a key and changes nothing else
    json.dumps(d)
    assert set(d) == {"train", "test"}
    for part, n in (("train", 2), ("test", 4)):
        p = d[part]
        assert {"channels", "fields", "q", "exceed_q", "real", "fake", "w1", "ks", "exceed_fake"} <= set(p)
        assert p["fields"] == n and p["channels"] == ["ch0", "ch1", "speed"]
        for side in ("real", "fake"):
            assert SIDE_KEYS <= set(p[side])
            assert np.array(p[side]["quantiles"]).shape == (3, len(p["q"]))
        assert len(p["w1"]) == len(p["ks"]) == 3 and np.array(p["exceed_fake"]).shape == (3, len(p["exceed_q"]))
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    spec = HistSpec.zscore(2)
    x = np.ascontiguousarray(fine[2:6].transpose(1, 0, 2, 3)).reshape(2, -1)
    counts, mom, ext = hist_ref(spec, x)
    real, fake = tr.distribution_results["test"]
    np.testing.assert_array_equal(real.host()[0], counts)
    np.testing.assert_array_equal(real.host()[2], ext)
    np.testing.assert_allclose(real.host()[1], mom, rtol=1e-12)
    np.testing.assert_allclose(d["test"]["real"]["mean"], real.mean(), rtol=1e-12)
    np.testing.assert_allclose(d["test"]["w1"], histograms.wasserstein1(real, fake), rtol=1e-12)


def test_log_distributions_without_log_metrics(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    monkeypatch.setattr(WassersteinGAN, "log_metrics", False)
    s = _run_epoch(True).metrics_log[0]
    assert "train" not in s and s["distributions"]["train"]["fields"] == 2 and s["distributions"]["test"]["fields"] == 4


def test_frequency_separation_trainer_reports_distributions(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    s = _run_epoch(True, fs=True).metrics_log[0]
    assert s["distributions"]["train"]["fields"] == 2 and s["distributions"]["test"]["fields"] == 4


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import downgan_amd.config.hyperparams as hp
    _patch(setattr)
    hp.batch_size, hp.lr = 1, 0.0
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    tr = _run_epoch(True, dist=d, lo=rank, step=world, batch=1)
    res = {k: [h.host() for h in v] for k, v in tr.distribution_results.items()}
    torch.save({"summary": tr.metrics_log[0]["distributions"], "hists": res}, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def _close(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _close(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], str):
        assert a == b, path
    else:
        np.testing.assert_allclose(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), rtol=1e-9, atol=0, err_msg=path)


def test_two_gloo_ranks_give_the_single_process_histograms(monkeypatch):
    """lr = 0 keeps G identical in both runs, so the generated fields are the same and only the reduction is tested."""
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(hp, "lr", 0.0)
    torch.set_num_threads(4)
    tr = _run_epoch(True)
    ref, ref_h = tr.metrics_log[0]["distributions"], tr.distribution_results
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["summary"] == r1["summary"]
    for part in ("train", "test"):
        assert r0["summary"][part]["fields"] == ref[part]["fields"]
        for side in range(2):
            c, m, e = r0["hists"][part][side]
            rc, rm, re_ = ref_h[part][side].host()
            np.testing.assert_array_equal(c, rc)
            np.testing.assert_array_equal(e, re_)
            np.testing.assert_allclose(m, rm, rtol=1e-9, atol=0)
        _close(r0["summary"][part], ref[part], part)
