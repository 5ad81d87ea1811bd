"""Cross spectra without a GPU: argument checks that fire before any library call, the ABI surface, the host helpers
(coherence, error spectra, effective resolution) on hand-made arrays, and the trainer's opt-in hook on the emulated ops (a
test-local op class adds a numpy ``cross_rapsd`` under the usual make_ops patch), in one process and over 2 gloo ranks."""
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


def ring_index(N):
    f = np.fft.fftfreq(N) * N
    return np.floor(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2) + 0.5).astype(int)


def cross_ref(a, b):
    """The definition, float64: a, b [N, N] -> [3, N/2 + 1]."""
    N = a.shape[0]
    A, B = np.fft.fft2(np.asarray(a, dtype=np.float64)), np.fft.fft2(np.asarray(b, dtype=np.float64))
    k = ring_index(N).ravel()
    cnt = np.bincount(k)[:N // 2 + 1]
    planes = (np.abs(A) ** 2, np.abs(B) ** 2, np.real(A * np.conj(B)))
    return np.stack([np.bincount(k, weights=p.ravel() / (N * N))[:N // 2 + 1] / cnt for p in planes])


def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("library or device touched before the arguments were checked")
    from downgan_amd import backend
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(backend, "make_ops", boom)
    monkeypatch.setattr(spectra, "_ops", {})


Z = torch.zeros
OK = Z(2, 2, 16, 16)


@pytest.mark.parametrize("a,b,kw,err,match", [
    (OK, Z(3, 2, 16, 16), {}, ValueError, "paired"),                                   # T
    (OK, Z(2, 1, 16, 16), {}, ValueError, "paired"),                                   # C
    (OK, Z(2, 2, 32, 32), {}, ValueError, "paired"),                                   # N
    (OK, Z(2, 16, 16, 4), {"nhwc_b": True}, ValueError, "paired"),                     # C through the other layout
    (Z(2, 16, 16, 2), OK, {"nhwc": True}, ValueError, "shape|square|paired|power"),    # nhwc_b defaults to nhwc
    (Z(2, 1, 96, 96), Z(2, 1, 96, 96), {}, ValueError, "power of two"),
    (OK, Z(2, 2, 96, 96), {}, ValueError, "power of two"),
    (Z(2, 1, 8, 8), Z(2, 1, 8, 8), {}, ValueError, "power of two"),
    (Z(2, 1, 64, 128), Z(2, 1, 64, 128), {}, ValueError, "square"),
    (OK, Z(2, 2, 16, 32), {}, ValueError, "square"),
    (Z(2, 9, 16, 16), Z(2, 9, 16, 16), {}, ValueError, "C <="),
    (Z(2, 16, 16, 16), Z(2, 16, 16, 16), {"nhwc": True}, ValueError, "C <="),
    (Z(2, 16, 16, 4), Z(2, 16, 16, 4), {"nhwc": True, "channels": 5}, ValueError, "channels"),
    (Z(2, 2, 16, 16, dtype=torch.float64), OK, {}, TypeError, "fp32 or bf16"),
    (OK, Z(2, 2, 16, 16, dtype=torch.float64), {}, TypeError, "fp32 or bf16"),
    (OK, Z(2, 2, 16, 16, dtype=torch.float16), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 2, 16, 16), np.float32), OK, {}, TypeError, "tensor"),
    (OK, np.zeros((2, 2, 16, 16), np.float32), {}, TypeError, "tensor"),
    (OK, [[0.0]], {}, TypeError, "tensor"),
    (Z(2, 16, 16), Z(2, 16, 16), {}, ValueError, "shape"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, a, b, kw, err, match):
    _no_library(monkeypatch)
    with pytest.raises(err, match=match):
        spectra.cross_rapsd(a, b, **kw)
    with pytest.raises(err, match=match):
        spectra.cross_rapsd(a, b, per_field=True, **kw)
    acc = spectra.CrossSpectrum(2, 16, device="cpu")
    with pytest.raises((ValueError, TypeError)):
        acc.add(a, b, **kw)


def test_accumulator_checks_its_shape(monkeypatch):
    _no_library(monkeypatch)
    for C_, N in ((9, 128), (0, 128), (2, 96), (2, 4096)):
        with pytest.raises(ValueError):
            spectra.CrossSpectrum(C_, N, device="cpu")
    acc = spectra.CrossSpectrum(2, 16, device="cpu")
    assert acc.sums.shape == (2, 3, 9) and acc.count == 0
    with pytest.raises(ValueError, match="CrossSpectrum"):
        acc.add(torch.zeros(2, 2, 32, 32), torch.zeros(2, 2, 32, 32))
    with pytest.raises(ValueError, match="CrossSpectrum"):
        acc.add(torch.zeros(2, 1, 16, 16), torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError, match="paired"):
        acc.add(torch.zeros(2, 2, 16, 16), torch.zeros(3, 2, 16, 16))
    with pytest.raises(ValueError, match="n_valid"):
        acc.add(torch.zeros(2, 2, 16, 16), torch.zeros(2, 2, 16, 16), n_valid=3)
    with pytest.raises(ValueError, match="n_valid"):
        acc.add(torch.zeros(2, 2, 16, 16), torch.zeros(2, 2, 16, 16), n_valid=0)
    with pytest.raises(ValueError, match="no field"):
        acc.mean()
    with pytest.raises(ValueError, match="no field"):
        acc.coherence()


def test_header_declares_and_library_exports_the_cross_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert "Cross spectra" in src
    for sym in ("dg_cross_rapsd_ws_bytes", "dg_cross_rapsd"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    assert _lib.lib().dg_cross_rapsd_ws_bytes.restype is C.c_size_t


def test_abi_rejects_bad_arguments_without_launching():
    """The workspace of the benchmarked shape (32 pairs of 2 x 1024^2) holds the two sides' half spectra, 2 x 64 x 513 x
    1024 x 8 B = 537.9 MB: 1.0 MB MORE than WS_CAP (512 MiB), so no workspace of that shape can lie under the cap and
    ``cross_rapsd`` splits such a batch in two calls.  Checked instead: the workspace is the two buffers plus at most three times
    dg_rapsd's partials (one set per plane), and half the batch fits under the cap with room to spare."""
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=128 * 128, ld_t=2 * 128 * 128, ld_c=128 * 128, ld_p=1)
    mk = lambda **kw: _lib.EofFields(**dict(ok, **kw))
    f = lambda **kw: C.byref(mk(**kw))
    ws = C.c_void_p(0x2000)
    cross = lib.dg_cross_rapsd
    assert cross(f(), f(), 96, ws, None, None, None) == -1                # not a power of two
    assert cross(f(P=96 * 96), f(P=96 * 96), 96, ws, None, None, None) == -1
    assert cross(f(P=4096 * 4096), f(P=4096 * 4096), 4096, ws, None, None, None) == -1
    assert cross(f(), f(), 64, ws, None, None, None) == -1                # P != N * N
    assert cross(f(C=9), f(C=9), 128, ws, None, None, None) == -1
    assert cross(f(base=0), f(), 128, ws, None, None, None) == -1
    assert cross(f(), f(base=0), 128, ws, None, None, None) == -1
    assert cross(f(), f(), 128, None, None, None, None) == -1
    assert cross(f(), None, 128, ws, None, None, None) == -1              # a null side
    assert cross(None, f(), 128, ws, None, None, None) == -1
    assert cross(f(), f(T=5), 128, ws, None, None, None) == -1            # a mismatched pair
    assert cross(f(), f(C=1), 128, ws, None, None, None) == -1
    assert cross(f(), f(P=64 * 64), 128, ws, None, None, None) == -1
    assert cross(f(P=64 * 64), f(), 128, ws, None, None, None) == -1
    assert cross(f(), f(ld_p=-1), 128, ws, None, None, None) == -1
    assert cross(f(dtype=7), f(), 128, ws, None, None, None) == -2
    assert cross(f(), f(dtype=7), 128, ws, None, None, None) == -2
    assert cross(f(dtype=_lib.DG_BF16), f(dtype=7), 128, ws, None, None, None) == -2
    assert cross(f(dtype=7), f(T=5), 128, ws, None, None, None) == -1     # the shape is checked first, as in dg_rapsd
    wsb = lib.dg_cross_rapsd_ws_bytes
    assert wsb(4, 2, 96) == 0 and wsb(0, 2, 128) == 0 and wsb(4, 9, 128) == 0 and wsb(4, 0, 128) == 0
    assert wsb(4, 2, 8) == 0 and wsb(4, 2, 4096) == 0
    spec = 64 * 513 * 1024 * 8                                            # one side's half spectra of 32 x 2 fields
    b32 = wsb(32, 2, 1024)
    assert 2 * spec < b32 <= 2 * spec + 3 * (lib.dg_rapsd_ws_bytes(32, 2, 1024) - spec)   # two buffers + three planes of partials
    assert 2 * spec > spectra.WS_CAP                                      # why the whole batch cannot fit (see the docstring)
    assert wsb(16, 2, 1024) < 0.6 * spectra.WS_CAP and wsb(1, 2, 2048) < spectra.WS_CAP
    assert wsb(1, 2, 1024) >= 4 * 513 * 1024 * 8


# ---------------------------------------------------------------------------------------------------------- host helpers
def _hand_made():
    s = np.zeros((2, 3, 5))
    s[0] = [[4.0, 4.0, 1.0, 9.0, 0.0], [1.0, 9.0, 4.0, 1.0, 2.0], [2.0, 3.0, -1.0, 0.0, 0.0]]
    s[1] = [[1.0, 2.0, 2.0, 2.0, 2.0], [1.0, 2.0, 8.0, 2.0, 0.5], [1.0, 2.0, 4.0, -2.0, 0.25]]
    return s


def test_coherence_and_error_spectra_values():
    s = _hand_made()
    coh = spectra.coherence(s)
    assert coh.shape == (2, 5) and coh.dtype == np.float64
    np.testing.assert_allclose(coh[0, :4], [1.0, 0.5, -0.5, 0.0], rtol=1e-15)
    assert np.isnan(coh[0, 4])                                            # s0 = 0: the denominator vanishes
    np.testing.assert_allclose(coh[1], [1.0, 1.0, 1.0, -1.0, 0.25], rtol=1e-15)
    err = spectra.error_spectrum(s)
    np.testing.assert_allclose(err, [[1.0, 7.0, 7.0, 10.0, 2.0], [0.0, 0.0, 2.0, 8.0, 2.0]], rtol=1e-15)
    rel = spectra.relative_error_spectrum(s)
    np.testing.assert_allclose(rel[0, :4], [0.25, 1.75, 7.0, 10.0 / 9.0], rtol=1e-15)
    assert np.isinf(rel[0, 4])
    np.testing.assert_allclose(rel[1], [0.0, 0.0, 1.0, 4.0, 1.0], rtol=1e-15)
    z = np.zeros((3, 4))
    assert np.isnan(spectra.coherence(z)).all() and spectra.coherence(z).shape == (4,)
    for bad in (np.zeros(5), np.zeros((2, 5)), np.zeros((2, 2, 5))):
        with pytest.raises(ValueError, match="3, K"):
            spectra.coherence(bad)
    # one field's [3, K] and a per-field [T, C, 3, K] stack go through unchanged
    np.testing.assert_array_equal(spectra.coherence(s[1]), coh[1])
    np.testing.assert_array_equal(spectra.error_spectrum(np.stack([s, s]))[1], err)


def test_effective_resolution_edge_cases():
    nan = float("nan")
    N = 16                                                                # K = 9, k = 0 .. 8
    coh = np.array([
        [0.0, 0.4, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9],                    # fails at k = 1 -> 0 (ring 0 is ignored anyway)
        [-5.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.5, 0.5, 0.5],                   # never fails -> N/2 (>= keeps 0.5; ring 0 ignored)
        [1.0, 0.9, 0.8, 0.3, 0.9, 0.9, 0.9, 0.9, 0.9],                    # a dip then recovery stops at the dip -> 2
        [1.0, 0.9, 0.9, 0.9, 0.9, nan, 0.9, 0.9, 0.9],                    # a NaN ring stops -> 4
        [1.0, nan, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9],                    # NaN at k = 1 -> 0
        [nan, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.49999, 0.9],                # NaN in ring 0 does not matter -> 6
    ])
    k = spectra.effective_resolution(coh)
    assert k.dtype == np.int64 and k.tolist() == [0, N // 2, 2, 4, 0, 6]
    assert spectra.effective_resolution(coh, threshold=0.75).tolist() == [0, 2, 2, 4, 0, 6]
    assert spectra.effective_resolution(coh, threshold=-10.0).tolist() == [8, 8, 8, 4, 0, 8]
    assert spectra.effective_resolution(coh[2]) == 2 and isinstance(spectra.effective_resolution(coh[2]), int)
    assert spectra.effective_resolution(np.stack([coh, coh])).shape == (2, 6)
    w = spectra.wavelength_px(k, N)
    assert w.tolist() == [np.inf, 2.0, 8.0, 4.0, np.inf, 16.0 / 6.0]
    assert spectra.wavelength_px(0, N) == np.inf and spectra.wavelength_px(4, 128) == 32.0
    with pytest.raises(ValueError):
        spectra.effective_resolution(np.array([1.0]))


def test_helpers_take_lists_arrays_and_tensors():
    s = _hand_made()
    for fn in (spectra.coherence, spectra.error_spectrum, spectra.relative_error_spectrum):
        want = fn(s)
        for v in (s.tolist(), torch.from_numpy(s), torch.from_numpy(s).float()):
            np.testing.assert_array_equal(fn(v), want, err_msg=fn.__name__)
    coh = spectra.coherence(s)
    want = spectra.effective_resolution(coh)
    assert want.tolist() == [1, 2]                                        # rings 1..: .5 | -.5 ... and 1, 1 | -1 ...
    for v in (coh.tolist(), torch.from_numpy(coh)):
        np.testing.assert_array_equal(spectra.effective_resolution(v), want)
    assert spectra.wavelength_px(want.tolist(), 8).tolist() == spectra.wavelength_px(want, 8).tolist() == [8.0, 4.0]


def test_accumulator_on_emulated_ops():
    """CrossSpectrum's bookkeeping (sums, count, n_valid, mean, coherence) with the numpy ops: no device involved."""
    rng = np.random.default_rng(3)
    a = torch.from_numpy(rng.standard_normal((5, 2, 16, 16)).astype(np.float32))
    b = torch.from_numpy((0.5 * a.numpy() + rng.standard_normal((5, 2, 16, 16))).astype(np.float32))
    ops = coherence_emu_ops()
    acc = spectra.CrossSpectrum(2, 16, device="cpu", ops=ops)
    acc.add(a[:2], b[:2]).add(a[2:], b[2:].permute(0, 2, 3, 1).contiguous(), n_valid=2, nhwc_b=True)
    assert acc.count == 4
    ref = np.mean([[cross_ref(a[t, c].numpy(), b[t, c].numpy()) for c in range(2)] for t in range(4)], axis=0)
    np.testing.assert_allclose(acc.mean().numpy(), ref, rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(acc.coherence(), spectra.coherence(acc.mean()))
    got = spectra.cross_rapsd(a, b, ops=ops)
    assert got.shape == (2, 3, 9) and got.dtype == torch.float64
    pf = spectra.cross_rapsd(a, b, per_field=True, ops=ops)
    assert pf.shape == (5, 2, 3, 9)
    np.testing.assert_allclose(pf.mean(0).numpy(), got.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(spectra.error_spectrum(pf[0, 1]), cross_ref((a.double() - b.double())[0, 1].numpy(), a[0, 1].numpy())[0], rtol=1e-9)


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def coherence_emu_ops():
    from oracle.emu_ops import EmuOps

    class CoherenceEmuOps(EmuOps):
        """The emulated ops plus dg_cross_rapsd's contract in numpy (float64 definition)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn)

        def cross_rapsd_ws_bytes(self, T, Cn, N):
            return int(_lib.lib().dg_cross_rapsd_ws_bytes(T, Cn, N))

        def cross_rapsd(self, fa, fb, N, per_field=None, sum=None):
            seen = lambda f: (f.t[..., :f.C].permute(0, 3, 1, 2) if f.nhwc else f.t).detach().double().cpu().numpy()
            a, b = seen(fa), seen(fb)
            assert a.shape == b.shape == (fa.T, fa.C, N, N)
            pf = np.array([[cross_ref(a[t, c], b[t, c]) for c in range(fa.C)] for t in range(fa.T)])
            if per_field is not None:
                per_field.copy_(torch.from_numpy(pf))
            if sum is not None:
                sum.copy_(torch.from_numpy(pf.sum(0)))

    return CoherenceEmuOps("f32")


KEYS = {"real", "fake", "co", "coherence", "rel_error", "k_eff", "wavelength_px", "fields"}


def _trainer(log_coherence, dist=None):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = WassersteinGAN(G, C_, dist=dist)
    tr.log_coherence = log_coherence
    return tr


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: coherence_emu_ops())
    setattr_(losses, "_ops", {})
    setattr_(spectra, "_ops", {})


def _loaders(lo=0, step=1, batch=2):
    from downgan_amd import synthetic
    from downgan_amd.GAN.dataloader import NetCDFSR
    coarse, fine = synthetic.tiles(6, 2, 16, seed=11)
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b][lo::step].copy()), torch.from_numpy(fine[a:b][lo::step].copy()))
    dl = torch.utils.data.DataLoader(ds(0, 2), batch_size=batch)
    tl = torch.utils.data.DataLoader(ds(2, 6), batch_size=batch)
    return dl, tl


def _run_epoch(log_coherence, dist=None, lo=0, step=1, batch=2):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(log_coherence, dist)
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr.metrics_log[0]


def test_log_coherence_off_leaves_the_summary_unchanged(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_coherence is False and WassersteinGAN.coherence_threshold == 0.5
    off = _run_epoch(False)
    on = _run_epoch(True)
    assert "coherence" not in off
    co = on.pop("coherence")
    assert on == off                                      # the hook adds a key and changes nothing else
    assert set(co) == {"train", "test"}
    K = 65
    for part, n in (("train", 2), ("test", 4)):
        d = co[part]
        assert set(d) == KEYS and d["fields"] == n
        for key in ("real", "fake", "co", "coherence", "rel_error"):
            assert np.array(d[key]).shape == (2, K), key
        assert len(d["k_eff"]) == len(d["wavelength_px"]) == 2 and all(isinstance(k, int) for k in d["k_eff"])
        s = np.stack([d["real"], d["fake"], d["co"]], axis=1)
        np.testing.assert_allclose(d["coherence"], spectra.coherence(s), rtol=1e-12)
        np.testing.assert_allclose(d["rel_error"], spectra.relative_error_spectrum(s), rtol=1e-12)
        assert d["k_eff"] == spectra.effective_resolution(d["coherence"], 0.5).tolist()
        assert d["wavelength_px"] == [128 / k if k else np.inf for k in d["k_eff"]]
        assert np.nanmax(np.abs(d["coherence"])) <= 1 + 1e-12             # Cauchy-Schwarz on every ring
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    real_test = np.mean([[cross_ref(fine[t, c], fine[t, c])[0] for c in range(2)] for t in range(2, 6)], axis=0)
    np.testing.assert_allclose(co["test"]["real"], real_test, rtol=1e-12)
    real_train = np.mean([[cross_ref(fine[t, c], fine[t, c])[0] for c in range(2)] for t in range(0, 2)], axis=0)
    np.testing.assert_allclose(co["train"]["real"], real_train, rtol=1e-12)


def test_coherence_threshold_is_used(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    torch.manual_seed(0)
    tr = _trainer(True)
    tr.coherence_threshold = -2.0                         # every finite ring passes
    dl, tl = _loaders()
    tr.train(dl, tl, epochs=1)
    d = tr.metrics_log[0]["coherence"]["test"]
    assert d["k_eff"] == [64, 64] and d["wavelength_px"] == [2.0, 2.0]


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


def test_two_gloo_ranks_give_the_single_process_coherence(monkeypatch):
    """lr = 0 keeps G identical in both runs, so the generated fields are the same and only the reduction is tested."""
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(hp, "lr", 0.0)
    torch.set_num_threads(4)
    ref = _run_epoch(True)["coherence"]
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"))["coherence"] for r in range(2))
    assert r0 == r1
    for part in ("train", "test"):
        assert r0[part]["fields"] == ref[part]["fields"]
        assert r0[part]["k_eff"] == ref[part]["k_eff"] and r0[part]["wavelength_px"] == ref[part]["wavelength_px"]
        for key in ("real", "fake", "co", "coherence", "rel_error"):
            np.testing.assert_allclose(r0[part][key], ref[part][key], rtol=1e-9, atol=0, err_msg=f"{part} {key}")
