"""Radially averaged power spectra without a GPU: the ring counts of the C ABI against the definition, argument checks that
fire before any library call, the ABI surface, the log-spectral distance, and the trainer's opt-in hook on the emulated ops
(a test-local op class adds a numpy ``rapsd`` under the usual make_ops patch), in one process and over 2 gloo ranks."""
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
NS = [16, 32, 64, 128, 256, 512, 1024, 2048]


def ring_index(N):
    f = np.fft.fftfreq(N) * N
    return np.floor(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2) + 0.5).astype(int)


def rapsd_ref(x):
    """The definition, float64: x [N, N] -> [N/2 + 1]."""
    N = x.shape[0]
    P = np.abs(np.fft.fft2(np.asarray(x, dtype=np.float64))) ** 2 / (N * N)
    k = ring_index(N)
    return np.array([P[k == i].mean() for i in range(N // 2 + 1)])


@pytest.mark.parametrize("N", NS)
def test_ring_counts_match_the_definition(N):
    k = ring_index(N)
    got = spectra.ring_counts(N)
    np.testing.assert_array_equal(got, np.bincount(k.ravel())[:N // 2 + 1])
    assert got.sum() == int((k <= N // 2).sum()) < N * N
    np.testing.assert_array_equal(spectra.wavenumbers(N), np.arange(N // 2 + 1))


def test_ring_boundary_pairs_land_in_ring_k():
    """u^2 + v^2 = k^2 + k sits 1/(8k) inside ring k's outer edge; counted there, not in ring k + 1."""
    N = 2048
    k = ring_index(N)
    f = (np.fft.fftfreq(N) * N).astype(np.int64)
    r2 = f[:, None] ** 2 + f[None, :] ** 2
    kk = np.floor(np.sqrt(r2)).astype(np.int64)
    edge = (r2 == kk * kk + kk) & (kk <= N // 2)
    assert edge.sum() > 0
    np.testing.assert_array_equal(k[edge], kk[edge])


def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("library or device touched before the arguments were checked")
    from downgan_amd import backend
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(backend, "make_ops", boom)
    monkeypatch.setattr(spectra, "_ops", {})


@pytest.mark.parametrize("x,kw,err,match", [
    (torch.zeros(2, 1, 96, 96), {}, ValueError, "power of two"),
    (torch.zeros(2, 1, 8, 8), {}, ValueError, "power of two"),
    (torch.zeros(1, 1, 4096, 4096, dtype=torch.bfloat16), {}, ValueError, "power of two"),
    (torch.zeros(2, 1, 64, 128), {}, ValueError, "square"),
    (torch.zeros(2, 9, 16, 16), {}, ValueError, "C <="),
    (torch.zeros(2, 16, 16, 16), {"nhwc": True}, ValueError, "C <="),
    (torch.zeros(2, 16, 16, 4), {"nhwc": True, "channels": 5}, ValueError, "channels"),
    (torch.zeros(2, 1, 16, 16, dtype=torch.float64), {}, TypeError, "fp32 or bf16"),
    (torch.zeros(2, 1, 16, 16, dtype=torch.float16), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 1, 16, 16), np.float32), {}, TypeError, "tensor"),
    (torch.zeros(1, 16, 16), {}, ValueError, "shape"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, x, kw, err, match):
    _no_library(monkeypatch)
    with pytest.raises(err, match=match):
        spectra.rapsd(x, **kw)
    acc = spectra.RadialSpectrum(1, 16, device="cpu")
    with pytest.raises((ValueError, TypeError)):
        acc.add(x, **kw)


def test_accumulator_checks_its_shape(monkeypatch):
    _no_library(monkeypatch)
    for C_, N in ((9, 128), (0, 128), (2, 96), (2, 4096)):
        with pytest.raises(ValueError):
            spectra.RadialSpectrum(C_, N, device="cpu")
    acc = spectra.RadialSpectrum(2, 16, device="cpu")
    with pytest.raises(ValueError, match="RadialSpectrum"):
        acc.add(torch.zeros(2, 2, 32, 32))
    with pytest.raises(ValueError, match="n_valid"):
        acc.add(torch.zeros(2, 2, 16, 16), n_valid=3)
    with pytest.raises(ValueError, match="no field"):
        acc.mean()


def test_header_declares_and_library_exports_the_rapsd_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert re.search(r"#define DG_RAPSD_MAX_N 2048\b", src)
    for sym in ("dg_rapsd_ws_bytes", "dg_rapsd", "dg_rapsd_ring_counts"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    assert _lib.RAPSD_MAX_N == spectra.N_MAX == 2048


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=128 * 128, ld_t=2 * 128 * 128, ld_c=128 * 128, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    ws = C.c_void_p(0x2000)
    assert lib.dg_rapsd(f(), 96, ws, None, None, None) == -1              # not a power of two
    assert lib.dg_rapsd(f(P=96 * 96), 96, ws, None, None, None) == -1
    assert lib.dg_rapsd(f(P=4096 * 4096), 4096, ws, None, None, None) == -1
    assert lib.dg_rapsd(f(), 64, ws, None, None, None) == -1              # P != N * N
    assert lib.dg_rapsd(f(C=9), 128, ws, None, None, None) == -1
    assert lib.dg_rapsd(f(base=0), 128, ws, None, None, None) == -1
    assert lib.dg_rapsd(f(), 128, None, None, None, None) == -1
    assert lib.dg_rapsd(f(dtype=7), 128, ws, None, None, None) == -2
    counts = (C.c_int64 * 65)()
    assert lib.dg_rapsd_ring_counts(96, counts) == -1 and lib.dg_rapsd_ring_counts(128, None) == -1
    assert lib.dg_rapsd_ws_bytes(4, 2, 96) == 0 and lib.dg_rapsd_ws_bytes(0, 2, 128) == 0 and lib.dg_rapsd_ws_bytes(4, 9, 128) == 0
    b1, b64 = lib.dg_rapsd_ws_bytes(1, 2, 1024), lib.dg_rapsd_ws_bytes(32, 2, 1024)
    assert 64 * 513 * 1024 * 8 < b64 < spectra.WS_CAP and b1 >= 2 * 513 * 1024 * 8
    assert lib.dg_rapsd_ws_bytes(1, 1, 2048) < spectra.WS_CAP


def test_log_spectral_distance():
    p = np.array([[1.0, 2.0, 4.0, 8.0], [1.0, 1.0, 1.0, 1.0]])
    q = p * np.array([[1.0, 10.0, 10.0, 10.0], [5.0, 0.1, 1.0, 10.0]])
    got = spectra.log_spectral_distance(p, q)
    np.testing.assert_allclose(got, [10.0, np.sqrt(200.0 / 3)], rtol=1e-12)
    assert spectra.log_spectral_distance(p[0], q[0], kmin=0) == pytest.approx(np.sqrt(300.0 / 4), rel=1e-12)
    assert spectra.log_spectral_distance(torch.tensor(p), torch.tensor(p)).tolist() == [0.0, 0.0]
    q = p * (1 + 1e-9)                                    # lists are read as float64
    np.testing.assert_allclose(spectra.log_spectral_distance(p.tolist(), q.tolist()), spectra.log_spectral_distance(p, q), rtol=1e-12)


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def spectra_emu_ops():
    from oracle.emu_ops import EmuOps

    class SpectraEmuOps(EmuOps):
        """The emulated ops plus dg_rapsd's contract in numpy (float64 definition)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn)

        def rapsd_ws_bytes(self, T, Cn, N):
            return int(_lib.lib().dg_rapsd_ws_bytes(T, Cn, N))

        def rapsd(self, f, N, per_field=None, sum=None):
            x = f.t[..., :f.C].permute(0, 3, 1, 2) if f.nhwc else f.t
            x = x.detach().double().cpu().numpy()
            pf = np.array([[rapsd_ref(x[t, c]) for c in range(f.C)] for t in range(f.T)])
            if per_field is not None:
                per_field.copy_(torch.from_numpy(pf))
            if sum is not None:
                sum.copy_(torch.from_numpy(pf.sum(0)))

    return SpectraEmuOps("f32")


def _trainer(log_spectra, dist=None):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = WassersteinGAN(G, C_, dist=dist)
    tr.log_spectra = log_spectra
    return tr


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: spectra_emu_ops())
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


def _run_epoch(log_spectra, dist=None, lo=0, step=1, batch=2):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(log_spectra, dist)
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr.metrics_log[0]


def test_log_spectra_off_leaves_the_summary_unchanged(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_spectra is False
    off = _run_epoch(False)
    on = _run_epoch(True)
    assert "spectra" not in off
    sp = on.pop("spectra")
    assert on == off                                      # the hook adds a key and changes nothing else
    assert set(sp) == {"train", "test"}
    for part, n in (("train", 2), ("test", 4)):
        d = sp[part]
        assert set(d) == {"real", "fake", "lsd", "fields"} and d["fields"] == n
        assert np.array(d["real"]).shape == np.array(d["fake"]).shape == (2, 65) and len(d["lsd"]) == 2
        np.testing.assert_allclose(d["lsd"], spectra.log_spectral_distance(np.array(d["real"]), np.array(d["fake"])), rtol=1e-12)
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    real_test = np.mean([[rapsd_ref(fine[t, c]) for c in range(2)] for t in range(2, 6)], axis=0)
    np.testing.assert_allclose(sp["test"]["real"], real_test, rtol=1e-12)


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
    ref = _run_epoch(True)["spectra"]
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"))["spectra"] for r in range(2))
    assert r0 == r1
    for part in ("train", "test"):
        assert r0[part]["fields"] == ref[part]["fields"]
        for key in ("real", "fake", "lsd"):
            np.testing.assert_allclose(r0[part][key], ref[part][key], rtol=1e-9, atol=0, err_msg=f"{part} {key}")
