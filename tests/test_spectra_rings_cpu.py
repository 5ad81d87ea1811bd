"""The references of the every-frequency RAPSD tests (tests/spectra_rings_ref.py) without a GPU: the integer ring rule against the
definition and the library's ring counts, the analytic spectra of the exhaustive and of the one-per-ring fields against the
float64 definition on the fp32 values the kernel sees, and what the chosen frequencies are there for (edges, Nyquist, mirror)."""
import numpy as np
import pytest

from downgan_amd import spectra
from tests import spectra_rings_ref as S


@pytest.mark.parametrize("N", [16, 32, 64, 128, 512, 2048])
def test_ring_rule_matches_the_definition_and_the_counts(N):
    f = np.fft.fftfreq(N) * N
    k_def = np.floor(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2) + 0.5).astype(np.int64)
    k = S.ring_map(N)
    assert np.array_equal(k, k_def)
    r2 = (f[:, None] ** 2 + f[None, :] ** 2).astype(np.int64)
    assert ((k * k - k + 1 <= r2) | (k == 0)).all() and (r2 <= k * k + k).all()
    assert np.array_equal(np.bincount(k.ravel())[:N // 2 + 1], spectra.ring_counts(N))


@pytest.mark.parametrize("N", [16, 32, 64])
def test_exhaustive_expectation_is_the_float64_spectrum(N):
    counts = spectra.ring_counts(N)
    x = S.exhaustive(N)
    want, k0 = S.exhaustive_expected(N, counts)
    a, b = S.exhaustive_freqs(N)
    assert x.shape == (N * (N // 2 + 1), 1, N, N) and x.dtype == np.float32
    h = np.arange(N)
    for f in (1, N // 2 + 3, x.shape[0] - 2):                     # the integer-reduced argument against the plain one
        plain = np.cos(2 * np.pi * (a[f] * h[:, None] + b[f] * h[None, :]) / N + S.PHI)
        assert np.abs(x[f, 0] - plain).max() <= 1e-6
    ref = S.rapsd_ref(x[:, 0], counts)
    on = want > 0
    assert np.abs(ref[on] / want[on] - 1).max() <= 1e-6            # fp32 rounding of the samples
    assert np.abs(np.where(on, 0.0, ref)).max() <= 1e-9 * N * N
    # what the set contains: every frequency of the half plane, the four self-conjugate ones, corners that must leave nothing
    assert len({(int(p), int(q)) for p, q in zip(a, b)}) == a.size
    corner = k0 > N // 2
    assert corner.any() and not want[corner].any()
    sc = np.isin(a, (0, N // 2)) & np.isin(b, (0, N // 2))
    assert sc.sum() == 4 and (sc & ~corner).sum() == 3
    for f in np.nonzero(sc & ~corner)[0]:
        assert want[f, k0[f]] == pytest.approx(N * N * np.cos(S.PHI) ** 2 / counts[k0[f]], rel=1e-15)
    assert ((a == N // 2) & ~corner).sum() > 1 and ((b == N // 2) & ~corner).sum() > 1      # Nyquist row and column, inside the disc
    assert (a > N // 2).any()                                      # negative row frequencies


@pytest.mark.parametrize("N", [128, 512, 2048])
def test_one_per_ring_points(N):
    pts = S.ring_points(N)
    h = N // 2
    ks = np.arange(1, h + 1)
    for f in range(4):
        a, b = np.array(pts[f]).T
        assert np.array_equal(S.ring_of(a, b, N), ks)
        assert ((0 <= b) & (b <= h) & (np.abs(a) <= h)).all()
    r2 = [np.array(p)[:, 0].astype(np.int64) ** 2 + np.array(p)[:, 1].astype(np.int64) ** 2 for p in pts]
    # field 1 sits on the inner edge wherever a lattice point does, field 2 on the outer edge likewise; both occur
    assert (r2[0] <= r2[1]).all()
    assert (r2[0] == ks * ks - ks + 1).sum() > h // 8 and (r2[1] == ks * ks + ks).sum() > h // 16
    fa, fb = np.meshgrid(np.arange(-h, h + 1), np.arange(0, h + 1), indexing="ij")
    kk = S.ring_of(fa, fb, N)
    q = fa.astype(np.int64) ** 2 + fb.astype(np.int64) ** 2
    for k in (1, 2, h // 2, h - 1, h):
        assert r2[0][k - 1] == q[kk == k].min() and r2[1][k - 1] == q[kk == k].max()
    assert pts[2][h - 1][1] == h and 0 < pts[2][h - 1][0] < h      # the Nyquist column, on the only ring that reaches it
    assert pts[2][:h - 1] == pts[0][:h - 1]
    assert all(p[0] == -q_[0] and p[1] == q_[1] for p, q_ in zip(pts[3], pts[1])) and min(p[0] for p in pts[3]) < 0


@pytest.mark.parametrize("N", [128, 512])
def test_one_per_ring_reference_equals_the_analytic_ring_sums(N):
    counts = spectra.ring_counts(N)
    x = S.one_per_ring(N)
    want = S.one_per_ring_expected(N, counts)
    ref64 = S.rapsd_ref(x, counts)
    assert np.abs(ref64 / want - 1).max() <= 1e-10
    ref32 = S.rapsd_ref(x.astype(np.float32), counts)              # the values the kernel sees
    assert np.abs(ref32 / want - 1).max() <= 1e-5
