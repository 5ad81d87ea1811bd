"""dg_rapsd on the MI355X (csrc/spectra.hip), frequency by frequency (tests/spectra_rings_ref.py): every frequency of a 16 x 16,
32 x 32 and 64 x 64 field as a field of its own, all fields of an N in one call, and one frequency on every ring at N = 128, 512
and 2048.  The bounds are the project's own (tests/test_spectra_gpu.py): single cosines to 1e-5 on the ring that holds the power
and 1e-7 N^2 on every other ring, multi-frequency fields to 1e-4 per ring against float64."""
import numpy as np
import pytest
import torch

from downgan_amd import spectra
from tests import spectra_rings_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RAPSD_PTS = 2048          # complex points per workgroup of the row and column passes (csrc/spectra.hip)


def _column_plan(F, N):
    """rapsd_ws restated: (S slices per field, line batches per slice)."""
    K, nfft = N // 2 + 1, RAPSD_PTS // N
    nb = -(-K // nfft)
    s = min(max(-(-2048 // F), 1), nb)
    return s, -(-nb // s)


@pytest.mark.parametrize("N", [16, 32, 64])
def test_every_frequency_lands_in_its_ring(N):
    x = torch.from_numpy(S.exhaustive(N)).to(DEV)
    F = x.shape[0]
    assert F == N * (N // 2 + 1)
    ops = spectra._default_ops(torch.device(DEV))
    assert spectra._chunk(ops, F, 1, N) == F                       # one library call
    s, batches = _column_plan(F, N)
    assert (s, batches) == ((1, 2) if N == 64 else (1, 1))        # N = 64: the multi-batch loop of one column workgroup
    got = spectra.rapsd(x, per_field=True)[:, 0].cpu().numpy()
    counts = spectra.ring_counts(N)
    want, k0 = S.exhaustive_expected(N, counts)
    a, b = S.exhaustive_freqs(N)
    on = want > 0
    assert on.sum() == (k0 <= N // 2).sum() and (on.sum(1) <= 1).all()
    rel = np.abs(got[on] / want[on] - 1)
    off = np.abs(np.where(on, 0.0, got))
    print(f"[rings] N={N}: {F} fields, worst relative error on the ring {rel.max():.3e}, worst power elsewhere {off.max():.3e} "
          f"(bound {1e-7 * N * N:.3e})")
    f = int(np.argmax(np.abs(got / np.where(on, want, 1.0) - 1) * on))
    assert rel.max() <= 1e-5, (int(a[f]), int(b[f]), int(k0[f]), got[f, min(k0[f], N // 2)], want[f].max())
    f, k = np.unravel_index(int(np.argmax(off)), off.shape)
    assert off.max() <= 1e-7 * N * N, (int(a[f]), int(b[f]), int(k0[f]), int(k), got[f, k])


def _check_one_per_ring(name, t, kw, values, N, counts):
    ref = S.rapsd_ref(values, counts)
    got = spectra.rapsd(t, per_field=True, **kw).cpu().numpy()
    assert got.shape == ref.shape
    rel = np.abs(got / ref - 1)
    print(f"[rings] N={N} {name}: worst ratio error per field {rel.reshape(-1, rel.shape[-1]).max(1)}")
    i = np.unravel_index(int(np.argmax(rel)), rel.shape)
    assert rel.max() <= 1e-4, (name, i, got[i], ref[i])


@pytest.mark.parametrize("N", [128, 512, 2048])
def test_one_frequency_on_every_ring(N):
    x32 = torch.from_numpy(S.one_per_ring(N).astype(np.float32))[:, None]           # [4, 1, N, N]
    _check_one_per_ring("nchw_f32", x32.to(DEV), {}, x32.double().numpy(), N, spectra.ring_counts(N))


def test_one_frequency_on_every_ring_in_every_layout():
    N, C = 128, 2
    counts = spectra.ring_counts(N)
    x32 = torch.from_numpy(S.one_per_ring(N).astype(np.float32)).reshape(2, C, N, N)
    pad = torch.full((2, N, N, 16), float("nan"), dtype=torch.bfloat16)            # padding channels must not be read
    pad[..., :C] = x32.permute(0, 2, 3, 1).to(torch.bfloat16)
    _check_one_per_ring("nchw_f32", x32.to(DEV), {}, x32.double().numpy(), N, counts)
    _check_one_per_ring("nhwc_f32", x32.permute(0, 2, 3, 1).contiguous().to(DEV), {"nhwc": True}, x32.double().numpy(), N, counts)
    _check_one_per_ring("nhwc_bf16_padded", pad.to(DEV), {"nhwc": True, "channels": C},
                        pad[..., :C].permute(0, 3, 1, 2).double().numpy(), N, counts)
