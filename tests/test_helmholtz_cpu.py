"""Helmholtz spectra without a GPU: the float64 definition and the identities that pin it (Nyquist rule, exchange of the pair,
sign of the row direction, pure flows from potentials), the half-spectrum evaluation the kernel uses against the full-spectrum
definition, argument checks that fire before any library call, the ABI surface, the host helpers on hand-made arrays, and the
trainer's opt-in hook on the emulated ops (a test-local op class adds numpy ``helmholtz`` / ``helmholtz_cross`` under the usual
make_ops patch), in one process and over 2 gloo ranks."""
import ctypes as C
import os
import re
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from downgan_amd import _lib, spectra

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the float64 definition
def ring_index(N):
    f = np.fft.fftfreq(N) * N
    return np.floor(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2) + 0.5).astype(int)


def _ring_means(planes, N):
    """planes [..., N, N] -> [..., N/2 + 1] ring means (corners dropped)."""
    K = N // 2 + 1
    k = ring_index(N).ravel()
    cnt = np.bincount(k)[:K]
    flat = planes.reshape(-1, N * N)
    out = np.stack([np.bincount(k, weights=p)[:K] / cnt for p in flat])
    return out.reshape(planes.shape[:-2] + (K,))


def _parts(u, v, scale, fft2):
    N = u.shape[-1]
    U = scale[0] * fft2(np.asarray(u, dtype=np.float64))
    V = scale[1] * fft2(np.asarray(v, dtype=np.float64))
    f = np.fft.fftfreq(N) * N
    kx, ky = f[None, :], f[:, None]                       # kx along the LAST axis (W), ky along axis -2 (H)
    k2 = kx ** 2 + ky ** 2
    g = np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2)) / (2.0 * N * N)
    return U, V, kx * V - ky * U, kx * U + ky * V, g


def helm_ref(u, v, scale=(1.0, 1.0), fft2=np.fft.fft2):
    """The definition, float64: u, v [..., N, N] -> [..., 3, N/2 + 1] (ke, rot, div)."""
    N = u.shape[-1]
    U, V, R, D, g = _parts(u, v, scale, fft2)
    ke = (np.abs(U) ** 2 + np.abs(V) ** 2) / (2.0 * N * N)
    return np.stack([_ring_means(p, N) for p in (ke, np.abs(R) ** 2 * g, np.abs(D) ** 2 * g)], axis=-2)


def helm_cross_ref(ua, va, ub, vb, scale=(1.0, 1.0), fft2=np.fft.fft2):
    """[..., 8, N/2 + 1]: ke, rot, div of a, of b, co_rot, co_div."""
    N = ua.shape[-1]
    _, _, Ra, Da, g = _parts(ua, va, scale, fft2)
    _, _, Rb, Db, _ = _parts(ub, vb, scale, fft2)
    co = [_ring_means(np.real(x * np.conj(y)) * g, N) for x, y in ((Ra, Rb), (Da, Db))]
    return np.concatenate([helm_ref(ua, va, scale, fft2), helm_ref(ub, vb, scale, fft2), np.stack(co, axis=-2)], axis=-2)


def potential_flows(rng, T, N, slope):
    """(rotational, divergent) flows [T, 2, N, N] whose ring kinetic energy falls as k^-slope: psi, chi are power-law Gaussian
    fields with the Nyquist rows and columns zeroed in Fourier space, differentiated spectrally: (u, v) = (-d psi / dH,
    d psi / dW) and (d chi / dW, d chi / dH)."""
    f = np.fft.fftfreq(N) * N
    kx, ky = f[None, :], f[:, None]
    r = np.sqrt(kx ** 2 + ky ** 2)
    r[0, 0] = 1.0
    flows = []
    for which in ("rot", "div"):
        P = np.fft.fft2(rng.standard_normal((T, N, N))) * r ** (-(slope + 2) / 2)
        P[:, N // 2, :] = 0.0
        P[:, :, N // 2] = 0.0
        if which == "rot":
            uh, vh = -1j * ky * P, 1j * kx * P
        else:
            uh, vh = 1j * kx * P, 1j * ky * P
        flows.append(np.stack([np.real(np.fft.ifft2(uh)), np.real(np.fft.ifft2(vh))], axis=1))
    return flows


def offset(x):
    """The constants 1/N and -2/N on u and v: ring 0 is well conditioned."""
    N = x.shape[-1]
    y = x.copy()
    y[:, 0] += 1.0 / N
    y[:, 1] -= 2.0 / N
    return y


def plane_wave(N, p, q, au, av, phase=0.7):
    """(u, v) = (au, av) cos(2 pi (p col + q row) / N + phase)."""
    h = np.arange(N)
    c = np.cos(2 * np.pi * ((p * h[None, :] + q * h[:, None]) % N) / N + phase)
    return au * c, av * c


def half_spectrum_model(u, v, scale=(1.0, 1.0)):
    """What the column kernel evaluates, in float64: the half spectrum kx = 0 .. N/2, Hermitian weights, the Nyquist rule."""
    N = u.shape[-1]
    K = N // 2 + 1
    U = scale[0] * np.fft.fft2(u)[:, :K]
    V = scale[1] * np.fft.fft2(v)[:, :K]
    kx = np.arange(K, dtype=np.float64)[None, :]
    vv = np.arange(N)
    ky = np.where(vv <= N // 2, vv, vv - N).astype(np.float64)[:, None]
    k2 = kx ** 2 + ky ** 2
    w = np.where((kx == 0) | (kx == N // 2), 1.0, 2.0)
    gk = w / (2.0 * N * N)
    g = np.where(k2 == 0, 0.0, gk / np.where(k2 == 0, 1.0, k2))
    nyq = (kx == N // 2) | (vv[:, None] == N // 2)
    D, R = kx * U + ky * V, kx * V - ky * U
    au, av = np.abs(U) ** 2, np.abs(V) ** 2
    div = np.where(nyq, kx ** 2 * au + ky ** 2 * av, np.abs(D) ** 2) * g
    rot = np.where(nyq, kx ** 2 * av + ky ** 2 * au, np.abs(R) ** 2) * g
    ke = (au + av) * gk
    ring = np.floor(np.sqrt(k2) + 0.5).astype(int).ravel()
    cnt = np.bincount(ring_index(N).ravel())[:K]
    return np.stack([np.bincount(ring, weights=p.ravel())[:K] / cnt for p in (ke, rot, div)])


def test_reference_identities_of_pure_and_mixed_flows():
    rng = np.random.default_rng(7)
    for N, slope in ((16, 0), (32, 2), (64, 3)):
        rot, div = potential_flows(rng, 2, N, slope)
        for flow, foreign in ((rot, 2), (div, 1)):
            s = helm_ref(flow[:, 0], flow[:, 1])
            assert (s[:, foreign] <= 1e-12 * s[:, 0]).all(), (N, slope, foreign)       # a pure flow has no foreign part
            x = offset(flow)
            s = helm_ref(x[:, 0], x[:, 1])
            assert (s[:, 1:, 0] == 0).all() and (s[:, 0, 0] > 0).all()                 # ring 0: the mean has neither part
            np.testing.assert_allclose(s[:, 1, 1:] + s[:, 2, 1:], s[:, 0, 1:], rtol=1e-12)
            assert (s[:, foreign, 1:] <= 1e-12 * s[:, 0, 1:]).all()
        mix = offset(rot + 0.3 * div)
        s = helm_ref(mix[:, 0], mix[:, 1])
        s_r, s_d = helm_ref(rot[:, 0], rot[:, 1]), helm_ref(div[:, 0], div[:, 1])
        np.testing.assert_allclose(s[:, 1, 1:], s_r[:, 1, 1:], rtol=1e-9)             # the parts do not mix
        np.testing.assert_allclose(s[:, 2, 1:], 0.09 * s_d[:, 2, 1:], rtol=1e-9)


def test_reference_conventions_exchange_and_row_direction():
    rng = np.random.default_rng(8)
    N = 32
    x = rng.standard_normal((3, 2, N, N))
    s = helm_ref(x[:, 0], x[:, 1])
    # a field whose first channel points along H is the same call with the pair exchanged: transposing the grid swaps the roles
    xt = np.swapaxes(x, -1, -2)
    np.testing.assert_allclose(helm_ref(xt[:, 1], xt[:, 0]), s, rtol=1e-10, atol=1e-13)
    # rows that run the other way are the same call with sv negated
    xf = x[:, :, ::-1, :]
    np.testing.assert_allclose(helm_ref(xf[:, 0], xf[:, 1], scale=(1.0, -1.0)), s, rtol=1e-10, atol=1e-13)
    assert np.abs(helm_ref(xf[:, 0], xf[:, 1]) - s)[:, 1:].max() > 1e-3 * s[:, 0].max()      # and it matters
    # the split is not invariant under per-channel scaling; the scale argument is the pre-scaled call
    np.testing.assert_allclose(helm_ref(x[:, 0], x[:, 1], scale=(2.0, -3.0)), helm_ref(2.0 * x[:, 0], -3.0 * x[:, 1]), rtol=1e-12)
    rot, _ = potential_flows(rng, 2, N, 2)
    t = helm_ref(rot[:, 0], rot[:, 1], scale=(2.0, 1.0))
    assert (t[:, 2, 2:] > 0.01 * t[:, 0, 2:]).all()         # a purely rotational flow, wrongly scaled, shows a divergent part
    # the paired planes: co of (a, a) is a's own, the co-planes sum to half the component co-spectra, Cauchy-Schwarz
    y = 0.5 * x + rng.standard_normal(x.shape)
    c = helm_cross_ref(x[:, 0], x[:, 1], y[:, 0], y[:, 1], scale=(2.0, -3.0))
    aa = helm_cross_ref(x[:, 0], x[:, 1], x[:, 0], x[:, 1])
    np.testing.assert_allclose(aa[:, 6:8], aa[:, 1:3], rtol=1e-12)
    N2 = N * N
    co = lambda a, b: _ring_means(np.real(np.fft.fft2(a) * np.conj(np.fft.fft2(b))) / N2, N)
    want = 0.5 * (4.0 * co(x[:, 0], y[:, 0]) + 9.0 * co(x[:, 1], y[:, 1]))
    np.testing.assert_allclose((c[:, 6] + c[:, 7])[:, 1:], want[:, 1:], rtol=1e-9, atol=1e-12)
    assert (np.abs(c[:, 6]) <= np.sqrt(c[:, 1] * c[:, 4]) * (1 + 1e-12)).all()
    assert (np.abs(c[:, 7]) <= np.sqrt(c[:, 2] * c[:, 5]) * (1 + 1e-12)).all()


def test_nyquist_rule_in_float64():
    """A wave (2, 16) at N = 32 with (u, v) = (1, 1) cos: rot = div = ke / 2 (doubling one member of the pair would give 0.75 /
    1.25 of it), and the half-spectrum evaluation with the no-cross-term rule equals the full-spectrum definition."""
    N = 32
    cnt = np.bincount(ring_index(N).ravel())
    for p, q in ((2, N // 2), (N // 2, 3)):
        k0 = int(np.floor(np.sqrt(p * p + q * q) + 0.5))
        for au, av in ((1.0, 1.0), (float(p), float(q)), (-float(q), float(p))):
            s = helm_ref(*plane_wave(N, p, q, au, av))
            norm = s[:, k0] * 4 * cnt[k0] / N ** 2
            k2 = p * p + q * q
            want = (au * au + av * av, (p * p * av * av + q * q * au * au) / k2, (p * p * au * au + q * q * av * av) / k2)
            np.testing.assert_allclose(norm, want, rtol=1e-12, err_msg=str((p, q, au, av)))
            np.testing.assert_allclose(half_spectrum_model(*plane_wave(N, p, q, au, av)), s, rtol=1e-10, atol=1e-18 * N ** 4)
    s = helm_ref(*plane_wave(N, 2, 16, 1.0, 1.0))
    np.testing.assert_allclose(s[1, 16], 0.5 * s[0, 16], rtol=1e-12)
    np.testing.assert_allclose(s[2, 16], 0.5 * s[0, 16], rtol=1e-12)
    rng = np.random.default_rng(9)
    for n in (16, 32):
        x = rng.standard_normal((2, n, n))
        np.testing.assert_allclose(half_spectrum_model(x[0], x[1], (2.0, -3.0)), helm_ref(x[0], x[1], (2.0, -3.0)), rtol=1e-10)


def test_plane_wave_known_answers_in_float64():
    """planes * 4 count[k0] / N^2 = (au^2 + av^2, (p av - q au)^2 / (p^2 + q^2), (p au + q av)^2 / (p^2 + q^2)) off the
    Nyquist lines; the GPU test uses these."""
    N = 32
    cnt = np.bincount(ring_index(N).ravel())
    for p, q in ((1, 0), (5, 3), (15, 1), (3, -7)):
        k0 = int(np.floor(np.sqrt(p * p + q * q) + 0.5))
        for au, av in ((float(p), float(q)), (-float(q), float(p)), (1.0, 1.0)):
            s = helm_ref(*plane_wave(N, p, q, au, av))
            k2 = p * p + q * q
            want = [au * au + av * av, (p * av - q * au) ** 2 / k2, (p * au + q * av) ** 2 / k2]
            np.testing.assert_allclose(s[:, k0] * 4 * cnt[k0] / N ** 2, want, rtol=0, atol=1e-12 * want[0])
            assert np.abs(np.delete(s, k0, axis=1)).max() <= 1e-15 * N * N * want[0]


# ------------------------------------------------------------------------------------------------------- argument checks
def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("library or device touched before the arguments were checked")
    from downgan_amd import backend
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(backend, "make_ops", boom)
    monkeypatch.setattr(spectra, "_ops", {})


Z = torch.zeros
OK = Z(2, 2, 16, 16)
inf, nan = float("inf"), float("nan")


@pytest.mark.parametrize("a,b,kw,err,match", [
    (OK, Z(3, 2, 16, 16), {}, ValueError, "paired"),                                   # T
    (OK, Z(2, 3, 16, 16), {}, ValueError, "paired"),                                   # C
    (OK, Z(2, 2, 32, 32), {}, ValueError, "paired"),                                   # N
    (OK, Z(2, 16, 16, 4), {"nhwc_b": True}, ValueError, "paired"),                     # C through the other layout
    (OK, OK, {"pair": (0, 2)}, ValueError, "pair"),                                    # out of range
    (OK, OK, {"pair": (-1, 0)}, ValueError, "pair"),
    (OK, OK, {"pair": (1, 1)}, ValueError, "pair"),                                    # equal
    (OK, OK, {"pair": (0,)}, ValueError, "pair"),
    (OK, OK, {"pair": (0.0, 1.0)}, ValueError, "pair"),
    (Z(2, 1, 16, 16), Z(2, 1, 16, 16), {}, ValueError, "C >= 2"),
    (Z(2, 16, 16, 1), Z(2, 16, 16, 1), {"nhwc": True}, ValueError, "C >= 2"),
    (Z(2, 2, 96, 96), Z(2, 2, 96, 96), {}, ValueError, "power of two"),
    (Z(2, 2, 8, 8), Z(2, 2, 8, 8), {}, ValueError, "power of two"),
    (Z(2, 2, 64, 128), Z(2, 2, 64, 128), {}, ValueError, "square"),
    (Z(2, 9, 16, 16), Z(2, 9, 16, 16), {}, ValueError, "C <="),
    (Z(2, 2, 16, 16, dtype=torch.float64), OK, {}, TypeError, "fp32 or bf16"),
    (OK, Z(2, 2, 16, 16, dtype=torch.float16), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 2, 16, 16), np.float32), OK, {}, TypeError, "tensor"),
    (Z(2, 16, 16), Z(2, 16, 16), {}, ValueError, "shape"),
    (OK, OK, {"scale": (0.0, 1.0)}, ValueError, "scale"),
    (OK, OK, {"scale": (1.0, -0.0)}, ValueError, "scale"),
    (OK, OK, {"scale": (inf, 1.0)}, ValueError, "scale"),
    (OK, OK, {"scale": (1.0, nan)}, ValueError, "scale"),
    (OK, OK, {"scale": (1.0,)}, ValueError, "scale"),
    (OK, OK, {"scale": 2.0}, ValueError, "scale"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, a, b, kw, err, match):
    _no_library(monkeypatch)
    for per_field in (False, True):
        with pytest.raises(err, match=match):
            spectra.helmholtz_cross(a, b, per_field=per_field, **kw)
    same = isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype
    if same and "nhwc_b" not in kw:                       # the one-sided call has the same checks of its one side
        with pytest.raises(err, match=match):
            spectra.helmholtz_rapsd(a, **kw)
        with pytest.raises(err, match=match):
            spectra.helmholtz_rapsd(a, per_field=True, **kw)
    with pytest.raises((ValueError, TypeError)):
        acc_kw = {k: kw.pop(k) for k in ("pair", "scale") if k in kw}
        spectra.HelmholtzSpectrum(16, device="cpu", **acc_kw).add(a, b, **kw)


def test_accumulator_checks_its_shape(monkeypatch):
    _no_library(monkeypatch)
    for N in (96, 8, 4096):
        with pytest.raises(ValueError):
            spectra.HelmholtzSpectrum(N, device="cpu")
    for bad in ((0, 0), (0, 8), (-1, 1)):
        with pytest.raises(ValueError, match="pair"):
            spectra.HelmholtzSpectrum(16, pair=bad, device="cpu")
    with pytest.raises(ValueError, match="scale"):
        spectra.HelmholtzSpectrum(16, scale=(0.0, 1.0), device="cpu")
    acc = spectra.HelmholtzSpectrum(16, device="cpu")
    assert acc.sums.shape == (8, 9) and acc.count == 0 and acc.pair == (0, 1) and acc.scale == (1.0, 1.0)
    assert spectra.HelmholtzSpectrum(16, scale=(2.0, 3.0), rows_up=False, device="cpu").scale == (2.0, -3.0)
    with pytest.raises(ValueError, match="HelmholtzSpectrum"):
        acc.add(torch.zeros(2, 2, 32, 32), torch.zeros(2, 2, 32, 32))
    with pytest.raises(ValueError, match="pair"):
        spectra.HelmholtzSpectrum(16, pair=(0, 2), device="cpu").add(OK, OK)
    with pytest.raises(ValueError, match="n_valid"):
        acc.add(OK, OK, n_valid=3)
    with pytest.raises(ValueError, match="n_valid"):
        acc.add(OK, OK, n_valid=0)
    with pytest.raises(ValueError, match="no field"):
        acc.mean()


def test_header_declares_and_library_exports_the_helmholtz_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert "Helmholtz spectra" in src
    for sym in ("dg_helmholtz_ws_bytes", "dg_helmholtz", "dg_helmholtz_cross_ws_bytes", "dg_helmholtz_cross"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    lib = _lib.lib()
    assert lib.dg_helmholtz_ws_bytes.restype is C.c_size_t and lib.dg_helmholtz_cross_ws_bytes.restype is C.c_size_t
    assert len(lib.dg_helmholtz.argtypes) == 9 and len(lib.dg_helmholtz_cross.argtypes) == 10
    from downgan_amd.ops import HipOps
    for name in ("helmholtz_ws_bytes", "helmholtz", "helmholtz_cross_ws_bytes", "helmholtz_cross"):
        assert callable(getattr(HipOps, name)), name


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=128 * 128, ld_t=2 * 128 * 128, ld_c=128 * 128, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    sc = lambda a=1.0, b=1.0: (C.c_float * 2)(a, b)
    ws = C.c_void_p(0x2000)
    one, two = lib.dg_helmholtz, lib.dg_helmholtz_cross
    assert one(f(), 0, 1, sc(), 96, ws, None, None, None) == -1                  # not a power of two
    assert one(f(), 0, 1, sc(), 64, ws, None, None, None) == -1                  # P != N * N
    assert one(f(), 0, 0, sc(), 128, ws, None, None, None) == -1                 # cu == cv
    assert one(f(), 0, 2, sc(), 128, ws, None, None, None) == -1                 # cv >= C
    assert one(f(), -1, 1, sc(), 128, ws, None, None, None) == -1
    assert one(f(C=1), 0, 1, sc(), 128, ws, None, None, None) == -1
    assert one(f(C=9), 0, 1, sc(), 128, ws, None, None, None) == -1
    assert one(f(base=0), 0, 1, sc(), 128, ws, None, None, None) == -1
    assert one(None, 0, 1, sc(), 128, ws, None, None, None) == -1
    assert one(f(), 0, 1, sc(), 128, None, None, None, None) == -1
    assert one(f(), 0, 1, None, 128, ws, None, None, None) == -1
    assert one(f(), 0, 1, sc(0.0, 1.0), 128, ws, None, None, None) == -1
    assert one(f(), 0, 1, sc(1.0, float("nan")), 128, ws, None, None, None) == -1
    assert one(f(), 0, 1, sc(float("inf"), 1.0), 128, ws, None, None, None) == -1
    assert one(f(dtype=7), 0, 1, sc(), 128, ws, None, None, None) == -2
    assert two(f(), f(T=5), 0, 1, sc(), 128, ws, None, None, None) == -1         # a mismatched pair
    assert two(f(), f(C=3), 0, 1, sc(), 128, ws, None, None, None) == -1
    assert two(f(), f(P=64 * 64), 0, 1, sc(), 128, ws, None, None, None) == -1
    assert two(f(), None, 0, 1, sc(), 128, ws, None, None, None) == -1
    assert two(None, f(), 0, 1, sc(), 128, ws, None, None, None) == -1
    assert two(f(), f(), 1, 1, sc(), 128, ws, None, None, None) == -1
    assert two(f(), f(), 0, 1, sc(1.0, 0.0), 128, ws, None, None, None) == -1
    assert two(f(), f(), 0, 1, sc(), 128, None, None, None, None) == -1
    assert two(f(dtype=7), f(), 0, 1, sc(), 128, ws, None, None, None) == -2
    assert two(f(dtype=_lib.DG_BF16), f(dtype=7), 0, 1, sc(), 128, ws, None, None, None) == -2
    assert two(f(dtype=7), f(T=5), 0, 1, sc(), 128, ws, None, None, None) == -1  # the shape is checked first
    w1, w2 = lib.dg_helmholtz_ws_bytes, lib.dg_helmholtz_cross_ws_bytes
    for w in (w1, w2):
        assert w(4, 96) == 0 and w(0, 128) == 0 and w(4, 8) == 0 and w(4, 4096) == 0
    spec = 32 * 513 * 1024 * 8                                                   # one component's half spectra of 32 fields
    assert w1(32, 1024) == lib.dg_cross_rapsd_ws_bytes(32, 1, 1024)              # the same bytes as cross spectra of one channel
    small = lib.dg_rapsd_ws_bytes(32, 1, 1024) - spec                            # dg_rapsd's partials: one set per plane at most
    assert 2 * spec < w1(32, 1024) <= 2 * spec + 3 * small and 4 * spec < w2(32, 1024) <= 4 * spec + 8 * small
    assert w2(32, 1024) > spectra.WS_CAP > w2(16, 1024)                          # 32 pairs at N = 1024 go as 16 + 16


# ---------------------------------------------------------------------------------------------------------- host helpers
def _hand_made():
    s = np.zeros((8, 4))
    s[0] = [9.0, 4.0, 2.0, 1.0]          # ke_a
    s[1] = [0.0, 3.0, 1.0, 0.0]          # rot_a
    s[2] = [0.0, 1.0, 1.0, 1.0]          # div_a
    s[3] = [4.0, 4.0, 8.0, 1.0]          # ke_b
    s[4] = [0.0, 3.0, 4.0, 0.0]          # rot_b
    s[5] = [0.0, 1.0, 4.0, 1.0]          # div_b
    s[6] = [0.0, 3.0, -1.0, 0.0]         # co_rot
    s[7] = [0.0, 0.5, 2.0, -1.0]         # co_div
    return s


def test_divergent_fraction_and_coherence_values():
    s = _hand_made()
    fr = spectra.divergent_fraction(s)
    assert fr.shape == (2, 4) and fr.dtype == np.float64
    assert np.isnan(fr[:, 0]).all()                                               # ring 0
    np.testing.assert_allclose(fr[0, 1:], [0.25, 0.5, 1.0], rtol=1e-15)
    np.testing.assert_allclose(fr[1, 1:], [0.25, 0.5, 1.0], rtol=1e-15)
    one = spectra.divergent_fraction(s[:3])
    assert one.shape == (4,)
    np.testing.assert_array_equal(one, fr[0])
    z = np.ones((3, 4))
    z[1:, 2] = 0.0
    assert np.isnan(spectra.divergent_fraction(z)[[0, 2]]).all()                  # rot + div = 0: NaN, no warning
    coh = spectra.helmholtz_coherence(s)
    assert coh.shape == (2, 4)
    assert np.isnan(coh[:, 0]).all() and np.isnan(coh[0, 3])
    np.testing.assert_allclose(coh[0, 1:3], [1.0, -0.5], rtol=1e-15)
    np.testing.assert_allclose(coh[1, 1:], [0.5, 1.0, -1.0], rtol=1e-15)
    assert spectra.effective_resolution(coh[0]) == 1 and spectra.effective_resolution(coh[1]) == 2
    assert spectra.effective_resolution(coh).tolist() == [1, 2]
    stack = np.stack([s, s])
    np.testing.assert_array_equal(spectra.helmholtz_coherence(stack)[1], coh)
    np.testing.assert_array_equal(spectra.divergent_fraction(stack)[1], fr)
    for v in (s.tolist(), torch.from_numpy(s)):
        np.testing.assert_array_equal(spectra.helmholtz_coherence(v), coh)
        np.testing.assert_array_equal(spectra.divergent_fraction(v), fr)
    for bad in (np.zeros(5), np.zeros((2, 5)), np.zeros((4, 5))):
        with pytest.raises(ValueError, match="3, K"):
            spectra.divergent_fraction(bad)
    with pytest.raises(ValueError, match="8, K"):
        spectra.helmholtz_coherence(s[:3])


def test_spectral_slope():
    k = np.arange(65, dtype=np.float64)
    k[0] = 1.0
    p = np.stack([7.0 * k ** -3.0, 0.1 * k ** (-5.0 / 3.0), np.ones(65)])
    np.testing.assert_allclose(spectra.spectral_slope(p, 2, 40), [-3.0, -5.0 / 3.0, 0.0], rtol=1e-12, atol=1e-13)
    assert isinstance(spectra.spectral_slope(p[0], 1, 64), float)
    np.testing.assert_allclose(spectra.spectral_slope(torch.from_numpy(p[1]), 4, 16), -5.0 / 3.0, rtol=1e-12)
    q = p.copy()
    q[0, 10] = 0.0
    out = spectra.spectral_slope(q, 2, 40)
    assert np.isnan(out[0]) and out[1] == pytest.approx(-5.0 / 3.0)
    # a broken power law: the band decides
    b = np.where(k < 16, k ** -3.0, 16.0 ** -3.0 * (k / 16.0) ** -1.0)
    assert spectra.spectral_slope(b, 2, 15) == pytest.approx(-3.0) and spectra.spectral_slope(b, 16, 64) == pytest.approx(-1.0)
    for kmin, kmax in ((0, 10), (5, 5), (6, 5), (1, 65), (1.0, 8)):
        with pytest.raises(ValueError, match="spectral_slope"):
            spectra.spectral_slope(p, kmin, kmax)


# ------------------------------------------------------------------------------------------------- emulated ops, trainer
def helmholtz_emu_ops():
    from oracle.emu_ops import EmuOps

    class HelmholtzEmuOps(EmuOps):
        """The emulated ops plus dg_helmholtz's and dg_helmholtz_cross's contract in numpy (float64 definition)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn)

        @staticmethod
        def _seen(f):
            return (f.t[..., :f.C].permute(0, 3, 1, 2) if f.nhwc else f.t).detach().double().cpu().numpy()

        def helmholtz_ws_bytes(self, T, N):
            return int(_lib.lib().dg_helmholtz_ws_bytes(T, N))

        def helmholtz_cross_ws_bytes(self, T, N):
            return int(_lib.lib().dg_helmholtz_cross_ws_bytes(T, N))

        @staticmethod
        def _out(pf, per_field, sum):
            if per_field is not None:
                per_field.copy_(torch.from_numpy(pf))
            if sum is not None:
                sum.copy_(torch.from_numpy(pf.sum(0)))

        def helmholtz(self, f, cu, cv, scale, N, per_field=None, sum=None):
            x = self._seen(f)
            assert x.shape == (f.T, f.C, N, N)
            self._out(helm_ref(x[:, cu], x[:, cv], scale), per_field, sum)

        def helmholtz_cross(self, fa, fb, cu, cv, scale, N, per_field=None, sum=None):
            a, b = self._seen(fa), self._seen(fb)
            assert a.shape == b.shape == (fa.T, fa.C, N, N)
            self._out(helm_cross_ref(a[:, cu], a[:, cv], b[:, cu], b[:, cv], scale), per_field, sum)

    return HelmholtzEmuOps("f32")


def test_api_and_accumulator_on_emulated_ops():
    """Bookkeeping without a device: pair, scale, rows_up, layouts, n_valid, chunk sums, mean."""
    rng = np.random.default_rng(3)
    a64 = rng.standard_normal((5, 3, 16, 16))
    b64 = 0.5 * a64 + rng.standard_normal((5, 3, 16, 16))
    a, b = torch.from_numpy(a64.astype(np.float32)), torch.from_numpy(b64.astype(np.float32))
    ad, bd = a.double().numpy(), b.double().numpy()
    ops = helmholtz_emu_ops()
    got = spectra.helmholtz_rapsd(a, ops=ops)
    assert got.shape == (3, 9) and got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), helm_ref(ad[:, 0], ad[:, 1]).mean(0), rtol=1e-12, atol=1e-13)
    pf = spectra.helmholtz_rapsd(a, pair=(2, 0), scale=(2.0, 3.0), rows_up=False, per_field=True, ops=ops)
    assert pf.shape == (5, 3, 9)
    np.testing.assert_allclose(pf.numpy(), helm_ref(ad[:, 2], ad[:, 0], (2.0, -3.0)), rtol=1e-12, atol=1e-13)
    nhwc = a.permute(0, 2, 3, 1).contiguous()
    np.testing.assert_array_equal(spectra.helmholtz_rapsd(nhwc, nhwc=True, ops=ops).numpy(), got.numpy())
    np.testing.assert_array_equal(spectra.helmholtz_rapsd(nhwc, nhwc=True, channels=2, ops=ops).numpy(), got.numpy())
    ref = helm_cross_ref(ad[:, 0], ad[:, 1], bd[:, 0], bd[:, 1])
    c = spectra.helmholtz_cross(a, b.permute(0, 2, 3, 1).contiguous(), nhwc_b=True, ops=ops)
    assert c.shape == (8, 9)
    np.testing.assert_allclose(c.numpy(), ref.mean(0), rtol=1e-12, atol=1e-13)
    assert spectra.helmholtz_cross(a, b, per_field=True, ops=ops).shape == (5, 8, 9)
    acc = spectra.HelmholtzSpectrum(16, device="cpu", ops=ops)
    acc.add(a[:2], b[:2]).add(a[2:], b[2:], n_valid=2)
    assert acc.count == 4
    np.testing.assert_allclose(acc.mean().numpy(), ref[:4].mean(0), rtol=1e-12, atol=1e-13)
    coh = spectra.helmholtz_coherence(acc.mean())
    assert np.nanmax(np.abs(coh)) <= 1 + 1e-12


KEYS = set(spectra.HELM_CROSS_PLANES) | {"div_frac_real", "div_frac_fake", "coh_rot", "coh_div", "k_eff_rot", "k_eff_div",
                                         "wavelength_px_rot", "wavelength_px_div", "fields"}


def _trainer(on, dist=None, npred=2):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, npred, num_res_blocks=1), Critic(16, 128, npred)
    tr = WassersteinGAN(G, C_, dist=dist)
    tr.log_helmholtz = on
    return tr


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: helmholtz_emu_ops())
    setattr_(losses, "_ops", {})
    setattr_(spectra, "_ops", {})


def _loaders(lo=0, step=1, batch=2):
    from downgan_amd import synthetic
    from downgan_amd.GAN.dataloader import NetCDFSR
    coarse, fine = synthetic.tiles(6, 2, 16, seed=11)
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b][lo::step].copy()), torch.from_numpy(fine[a:b][lo::step].copy()))
    return torch.utils.data.DataLoader(ds(0, 2), batch_size=batch), torch.utils.data.DataLoader(ds(2, 6), batch_size=batch)


def _run_epoch(on, dist=None, lo=0, step=1, batch=2, **attrs):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(on, dist)
    for k, v in attrs.items():
        setattr(tr, k, v)
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr.metrics_log[0]


def test_log_helmholtz_off_leaves_the_summary_unchanged(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN as W
    assert W.log_helmholtz is False and W.helmholtz_pair == (0, 1) and W.helmholtz_scale is None
    assert W.helmholtz_rows_up is True and W.helmholtz_threshold == 0.5
    off = _run_epoch(False)
    on = _run_epoch(True, helmholtz_scale=(2.0, 3.0), helmholtz_rows_up=False)
    assert "helmholtz" not in off
    hz = on.pop("helmholtz")
    assert on == off                                      # the hook adds a key and changes nothing else
    assert set(hz) == {"train", "test"}
    K = 65
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    for part, n, sl in (("train", 2, slice(0, 2)), ("test", 4, slice(2, 6))):
        d = hz[part]
        assert set(d) == KEYS and d["fields"] == n
        for key in KEYS - {"k_eff_rot", "k_eff_div", "wavelength_px_rot", "wavelength_px_div", "fields"}:
            assert np.array(d[key]).shape == (K,), key
        s = np.stack([d[name] for name in spectra.HELM_CROSS_PLANES])
        frac, coh = spectra.divergent_fraction(s), spectra.helmholtz_coherence(s)
        np.testing.assert_array_equal(d["div_frac_real"], frac[0])
        np.testing.assert_array_equal(d["div_frac_fake"], frac[1])
        np.testing.assert_array_equal(d["coh_rot"], coh[0])
        np.testing.assert_array_equal(d["coh_div"], coh[1])
        for i, what in enumerate(("rot", "div")):
            k = d["k_eff_" + what]
            assert isinstance(k, int) and k == spectra.effective_resolution(coh[i], 0.5)
            assert d["wavelength_px_" + what] == (128 / k if k else np.inf)
        assert np.nanmax(np.abs(coh)) <= 1 + 1e-12        # Cauchy-Schwarz on every ring
        np.testing.assert_allclose(s[1, 1:] + s[2, 1:], s[0, 1:], rtol=1e-12)
        real = helm_ref(fine[sl, 0], fine[sl, 1], (2.0, -3.0)).mean(0)
        np.testing.assert_allclose(s[:3], real, rtol=1e-12, atol=1e-300)


def test_threshold_and_pair_are_used(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    d = _run_epoch(True, helmholtz_threshold=-2.0, helmholtz_pair=(1, 0))["helmholtz"]["test"]
    assert d["k_eff_rot"] == d["k_eff_div"] == 64 and d["wavelength_px_rot"] == d["wavelength_px_div"] == 2.0
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    np.testing.assert_allclose(d["rot_real"], helm_ref(fine[2:6, 1], fine[2:6, 0]).mean(0)[1], rtol=1e-12, atol=1e-300)


def test_trainer_refuses_a_scalar_field_and_a_bad_pair(monkeypatch):
    _patch(monkeypatch.setattr)
    from downgan_amd import synthetic
    from downgan_amd.GAN.dataloader import NetCDFSR
    tr = _trainer(True, npred=1)
    coarse, fine = synthetic.tiles(2, 2, 16, seed=11)
    dl = torch.utils.data.DataLoader(NetCDFSR(torch.from_numpy(coarse), torch.from_numpy(fine[:, :1].copy())), batch_size=2)
    with pytest.raises(ValueError, match="n_predictands >= 2"):
        tr.train(dl, None, epochs=1)
    assert tr.num_steps == 0                              # raised at the start of the epoch, before any step
    tr = _trainer(True)
    tr.helmholtz_pair = (0, 2)
    with pytest.raises(ValueError, match="pair"):
        tr.train(_loaders()[0], None, epochs=1)
    tr = _trainer(True)
    tr.helmholtz_scale = (0.0, 1.0)
    with pytest.raises(ValueError, match="scale"):
        tr.train(_loaders()[0], None, epochs=1)


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import downgan_amd.config.hyperparams as hp
    _patch(setattr)
    hp.batch_size, hp.lr = 1, 0.0
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    summary = _run_epoch(True, dist=d, lo=rank, step=world, batch=1)
    torch.save(summary, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_spectra(monkeypatch):
    """lr = 0 keeps G identical in both runs, so the generated fields are the same and only the reduction is tested."""
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(hp, "lr", 0.0)
    torch.set_num_threads(4)
    ref = _run_epoch(True)["helmholtz"]
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"))["helmholtz"] for r in range(2))
    for part in ("train", "test"):
        assert r0[part]["fields"] == r1[part]["fields"] == ref[part]["fields"]
        for key in ("k_eff_rot", "k_eff_div", "wavelength_px_rot", "wavelength_px_div"):
            assert r0[part][key] == r1[part][key] == ref[part][key], (part, key)
        for key in spectra.HELM_CROSS_PLANES + ("div_frac_real", "div_frac_fake", "coh_rot", "coh_div"):
            np.testing.assert_array_equal(r0[part][key], r1[part][key], err_msg=f"{part} {key}")
            np.testing.assert_allclose(r0[part][key], ref[part][key], rtol=1e-9, atol=1e-300, err_msg=f"{part} {key}")
