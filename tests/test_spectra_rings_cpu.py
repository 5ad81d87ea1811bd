"""The references of the every-frequency RAPSD tests (tests/spectra_rings_ref.py) without a GPU: the integer ring rule against the
definition and the library's ring counts, the analytic spectra of the exhaustive and of the one-per-ring fields against the
float64 definition on the fp32 values the kernel sees, and what the chosen frequencies are there for (edges, Nyquist, mirror).
For the cross and Helmholtz spectra: the analytic answers of the exhaustive pairs against the full-spectrum definition, the
half-spectrum evaluation with its Nyquist rule against that definition at every frequency, a mutation check (every planted
single-frequency fault must make the GPU test's comparator fail), and the one-per-ring pairs with their fp32-FFT proxy."""
import functools

import numpy as np
import pytest
import torch

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


# ------------------------------------------------------------------------------------- cross spectra and Helmholtz spectra
def _flat(cross):
    """[F, 2, 3, K] -> [F, 6, K]: the comparator takes one plane axis."""
    return cross.reshape(cross.shape[0], 6, cross.shape[-1])


@functools.lru_cache(maxsize=None)
def _exhaustive_case(N):
    counts = spectra.ring_counts(N)
    A, B = (x.astype(np.float64) for x in S.exhaustive_pair(N))     # the fp32 samples
    return counts, A, B, S.helm_cross_ref(A, B, counts), S.cross_ref(A, B, counts)


@pytest.mark.parametrize("N", [16, 32, 64])
def test_exhaustive_pair_expectation_is_the_float64_definition(N):
    counts, A, B, ref_h, ref_c = _exhaustive_case(N)
    F = N * (N // 2 + 1)
    A32, B32 = S.exhaustive_pair(N)
    assert A32.shape == B32.shape == (F, 2, N, N) and A32.dtype == B32.dtype == np.float32
    assert np.array_equal(A32[:, 0:1], S.exhaustive(N)) and np.array_equal(A32[:, 1], 0.5 * A32[:, 0])
    a, b = S.exhaustive_freqs(N)
    _, _, delta, _, cb = S.exhaustive_pair_amps(N)
    h = np.arange(N)
    for f in (1, N // 2 + 3, F - 2):                               # the integer-reduced argument against the plain one
        plain = np.cos(2 * np.pi * (a[f] * h[:, None] + b[f] * h[None, :]) / N + S.PHI + delta[f])
        assert np.abs(B32[f] - cb[f][:, None, None] * plain).max() <= 1e-6
    want_h, want_c, k0 = S.exhaustive_pair_expected(N, counts)
    e_h, amp_h, e_c, amp_c = S.exhaustive_pair_envelopes(N, counts)
    for name, ref, want, E, amp in (("helm", ref_h, want_h, e_h, amp_h), ("cross", _flat(ref_c), _flat(want_c),
                                                                          e_c.reshape(F, 6), amp_c.reshape(F, 6))):
        on, off = S.exhaustive_errors(ref, want, k0, E, amp, N)
        inside = k0 <= N // 2
        elsewhere = np.abs(ref - want).copy()
        elsewhere[np.nonzero(inside)[0], :, k0[inside]] = 0.0
        print(f"[rings-pair] N={N} {name}: float64 definition on the fp32 samples against the analytic answer: on the ring "
              f"{on.max():.3e} of E, elsewhere {elsewhere.max() / (N * N):.3e} N^2")
        assert on.max() <= 1e-6, (name, on.max())
        assert elsewhere.max() <= 1e-9 * N * N, (name, elsewhere.max())
        assert not want[~inside].any()
    # the one-sided reference is planes 0-2 of the paired one, and (b, a) exchanges the sides
    ba = S.helm_cross_ref(B[:40], A[:40], counts)
    assert np.array_equal(ba[:, 0:3], ref_h[:40, 3:6]) and np.array_equal(ba[:, 3:6], ref_h[:40, 0:3])


@pytest.mark.parametrize("N", [16, 32, 64])
def test_exhaustive_pair_contains_what_the_kernels_branch_on(N):
    counts = spectra.ring_counts(N)
    a, b = S.exhaustive_freqs(N)
    want_h, want_c, k0 = S.exhaustive_pair_expected(N, counts)
    _, _, delta, _, _ = S.exhaustive_pair_amps(N)
    h = N // 2
    inside = k0 <= h
    assert ((a > h) & inside & (b > 0)).sum() > N                  # negative row frequencies: the v - N branch of helm_geom
    assert ((b == 0) & (a != 0) & inside).sum() == N - 1            # the line u = 0 with ky != 0 (weight 1, kx = 0)
    assert ((a == h) & inside).sum() > 1 and ((b == h) & inside).sum() > 1         # Nyquist row and column, inside the disc
    sc = np.isin(a, (0, h)) & np.isin(b, (0, h))
    assert sc.sum() == 4 and (sc & inside).sum() == 3
    assert (~inside).any() and not want_h[~inside].any() and not want_c[~inside].any()
    r2 = S.signed(a, N).astype(np.int64) ** 2 + b.astype(np.int64) ** 2
    assert (r2[inside] == (k0 * k0 - k0 + 1)[inside]).sum() >= 4 and (r2[inside] == (k0 * k0 + k0)[inside]).sum() >= 4      # ring edges
    f = np.nonzero(inside)[0]
    on = want_h[f, :, k0[f]]                                        # [n, 8]
    neg_rot, neg_div = int((on[:, 6] < 0).sum()), int((on[:, 7] < 0).sum())
    print(f"[rings-pair] N={N}: {f.size} frequencies inside the disc, co_rot < 0 at {neg_rot}, co_div < 0 at {neg_div}")
    assert 3 * neg_rot > f.size and 3 * neg_div > f.size
    assert (on[:, [0, 3]] > 0).all() and (on[:, [1, 2, 4, 5]] >= 0).all()
    assert (want_c[f, :, 2, k0[f]] < 0).sum() > f.size // 3
    assert np.abs(np.cos(delta[inside])).min() >= 0.2


@pytest.mark.parametrize("N", [16, 32, 64])
def test_half_spectrum_evaluation_equals_the_full_spectrum_definition(N):
    """The Nyquist rule, the Hermitian weights and the partner rule against the definition at every frequency.  Measure: ring
    SUMS (mean x count) against the side's total over all frequencies, sum of (u^2 + v^2) / 2 over the samples by Parseval (the
    co-planes: the geometric mean of the sides; cross planes: the sums of squares), which is the ring's own ke wherever a wave
    lies inside the disc and still a scale for the corner waves, whose rings are all empty."""
    counts, A, B, ref_h, ref_c = _exhaustive_case(N)
    got_h, got_c = S.half_spectrum_eval(A, B, counts)
    ta, tb = 0.5 * (A ** 2).sum((1, 2, 3)), 0.5 * (B ** 2).sum((1, 2, 3))
    den_h = np.stack([ta] * 3 + [tb] * 3 + [np.sqrt(ta * tb)] * 2, axis=1)[:, :, None]
    pa, pb = (A ** 2).sum((2, 3)), (B ** 2).sum((2, 3))
    den_c = np.stack([pa, pb, np.sqrt(pa * pb)], axis=2)[..., None]
    e_h = (np.abs(got_h - ref_h) * counts / den_h).max()
    e_c = (np.abs(got_c - ref_c) * counts / den_c).max()
    print(f"[rings-pair] N={N}: half-spectrum evaluation against the definition, Helmholtz {e_h:.3e}, cross {e_c:.3e}")
    assert e_h <= 1e-12 and e_c <= 1e-12, (e_h, e_c)


def _faults(N, counts):
    """One planted fault of each kind with the frequency it is planted at, chosen from the expectation."""
    a, b = S.exhaustive_freqs(N)
    want_h, _, k0 = S.exhaustive_pair_expected(N, counts)
    h = N // 2
    r2 = S.signed(a, N).astype(np.int64) ** 2 + b.astype(np.int64) ** 2
    edge = np.nonzero((r2 == k0 * k0 + k0) & (k0 < h) & (b > 0) & (b < h) & (a > 0) & (a < h))[0]
    f = np.nonzero(k0 <= h)[0]
    co = np.zeros((a.size, 2))
    co[f] = want_h[f, 6:8, k0[f]]
    neg = np.nonzero((co[:, 0] < 0) & (b > 0) & (b < h) & (a > 0) & (a < h))[0]
    assert edge.size and neg.size
    e, n = int(edge[0]), int(neg[0])
    return [("ring", int(b[e]), int(a[e])),
            ("weight", 0, 5),
            ("ky", 3, N - 5),
            ("partner", 2, h),
            ("cross", 2, h), ("cross", h, 3), ("cross", h, N - 3),
            ("swap", 5, 3),
            ("abs", int(b[n]), int(a[n]))]


def test_the_comparator_catches_every_planted_single_frequency_fault():
    N = 32
    counts, A, B, _, _ = _exhaustive_case(N)
    F = A.shape[0]
    want_h, want_c, k0 = S.exhaustive_pair_expected(N, counts)
    e_h, amp_h, e_c, amp_c = S.exhaustive_pair_envelopes(N, counts)

    def compare(fault):
        got_h, got_c = S.half_spectrum_eval(A, B, counts, fault=fault)
        S.check_exhaustive(f"helm {fault}", got_h, want_h, k0, e_h, amp_h, N)
        S.check_exhaustive(f"cross {fault}", _flat(got_c), _flat(want_c), k0, e_c.reshape(F, 6), amp_c.reshape(F, 6), N)

    compare(None)                                                  # the faultless evaluation passes
    faults = _faults(N, counts)
    assert {k for k, _, _ in faults} == {"ring", "weight", "ky", "partner", "cross", "swap", "abs"}
    for fault in faults:
        with pytest.raises(AssertionError) as info:
            compare(fault)
        # and the comparator names the frequency the fault sits at
        _, u, v = fault
        named = info.value.args[0][2]
        assert (named[0] % N, named[1]) in ((v, u), ((N - v) % N, u)), (fault, named)


FFT32 = lambda x: torch.fft.fft2(torch.from_numpy(x).float()).numpy()
PAIR_TOL = 1e-4           # the bound of the one-per-ring GPU test (the project's bound for multi-frequency fields)


@pytest.mark.parametrize("N", [128, 512])
def test_one_per_ring_pair_reference_and_its_fp32_proxy(N):
    counts = spectra.ring_counts(N)
    A, B = S.one_per_ring_pair(N)
    assert A.shape == B.shape == (4, 2, N, N) and A.dtype == np.float64
    assert np.array_equal(A[:, 0], S.one_per_ring(N)) and np.array_equal(A[:, 1], 0.5 * A[:, 0])
    np.testing.assert_allclose(B.mean((2, 3)), np.tile([0.5 * S.CONST, -S.CONST], (4, 1)), atol=1e-12)
    A32, B32 = A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)
    ref64, ref32 = S.helm_cross_ref(A, B, counts), S.helm_cross_ref(A32, B32, counts)
    rounding = max(S.helm_measure(ref32, ref64))
    # what the fields are: side b never far below side a, negative co-planes on about half of the rings
    assert (ref64[:, 3] >= 0.0999 * ref64[:, 0]).all()
    negative = ((ref64[:, 6, 1:] < 0) | (ref64[:, 7, 1:] < 0)).mean()
    # each ring holds one wave, whose ke is N^2 / 4 (xu^2 + xv^2) / count
    ks = np.arange(1, N // 2 + 1)
    np.testing.assert_allclose(ref64[:, 0, 1:] * counts[1:], np.tile(N * N / 4 * 1.25, (4, N // 2)), rtol=1e-10)
    np.testing.assert_allclose(ref64[:, 3, 1:] * counts[1:], np.tile(N * N / 4 * ((0.75 - 0.5 * (ks % 3)) ** 2 + (1.25 - 0.5 * (ks % 4)) ** 2),
                                                                     (4, 1)), rtol=1e-10)
    proxy = max(S.helm_measure(S.helm_cross_ref(A32, B32, counts, fft2=FFT32), ref32))
    cref = S.cross_ref(A32, B32, counts)
    crounding = max(S.cross_measure(S.cross_ref(A, B, counts), cref))
    cproxy = max(S.cross_measure(S.cross_ref(A32, B32, counts, fft2=FFT32), cref))
    print(f"[rings-pair] N={N} one per ring: fp32 sample rounding {rounding:.3e} (Helmholtz), {crounding:.3e} (cross); fp32 FFT on "
          f"the CPU against float64 on the same samples {proxy:.3e} (Helmholtz), {cproxy:.3e} (cross), bound {PAIR_TOL:.0e}; "
          f"rings with a negative co-plane {negative:.2f}")
    assert rounding <= 1e-5 and crounding <= 1e-5
    assert negative > 1 / 3
    assert proxy <= PAIR_TOL and cproxy <= PAIR_TOL
    half_h, half_c = S.half_spectrum_eval(A32[:2], B32[:2], counts) if N == 128 else (ref32[:2], cref[:2])
    assert max(S.helm_measure(half_h, ref32[:2])) <= 1e-12 and max(S.cross_measure(half_c, cref[:2])) <= 1e-12
