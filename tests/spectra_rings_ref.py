"""Fields, ring rule and float64 references of the every-frequency tests of dg_rapsd (csrc/spectra.hip):
tests/test_spectra_rings_gpu.py on the device, tests/test_spectra_rings_cpu.py for the references themselves.

The goal is that EVERY frequency lands in its ring with its weight.  Ring means of broadband fields cannot show that: a ring at
N = 1024 holds thousands of frequencies, so one misplaced boundary frequency, a wrong Hermitian weight on one line or a wrong
N - v partner at v = 0 or v = N/2 moves a mean by about 1 / count.  Here each frequency carries a ring's power alone.

Ring rule, in integers: frequency (a, b) (row, column; signed, a in (-N/2, N/2], N/2 standing for -N/2) lies in ring k with
k^2 - k + 1 <= a^2 + b^2 <= k^2 + k (k = 0: the origin); rings k > N/2 (the corners) are dropped.

``exhaustive(N)``: one field per (a, b), a = 0 .. N-1 (as FFT row indices), b = 0 .. N/2: cos(2 pi (a h + b w) / N + PHI).  All
power lies in ring k0 of the rule: N^2 / (2 count[k0]), N^2 cos^2(PHI) / count[k0] at the four self-conjugate frequencies,
nothing anywhere when k0 > N/2.

``one_per_ring(N)``: four fields, each the sum of one unit cosine per ring k = 1 .. N/2 (phases spread) plus a constant; the
cosine of ring k sits at (1) the lattice point of smallest r^2, (2) of largest r^2 (the ring's outer edge), (3) a point on the
Nyquist column b = N/2 where the ring has one (ring N/2 only), else as (1), (4) the point of (2) mirrored to a negative row
frequency.  Synthesised in float64 by an inverse FFT of the Hermitian spectrum.
"""
from __future__ import annotations

import functools

import numpy as np

PHI = 0.3               # phase of the exhaustive cosines: not 0, so that real and imaginary parts both carry signal
CONST = 0.5             # the constant of the one-per-ring fields (ring 0)


def signed(a, N):
    """FFT index -> signed frequency in (-N/2, N/2] (the magnitude is all the ring rule needs)."""
    a = np.asarray(a) % N
    return np.where(a > N // 2, a - N, a)


def ring_of(a, b, N):
    """Ring index of the frequencies (a, b) (FFT indices or signed), by the integer rule; > N/2 for the corners."""
    fa, fb = signed(a, N).astype(np.int64), signed(b, N).astype(np.int64)
    r2 = fa * fa + fb * fb
    k = np.floor(np.sqrt(r2.astype(np.float64))).astype(np.int64)
    k = np.where(k * k > r2, k - 1, k)
    k = np.where((k + 1) * (k + 1) <= r2, k + 1, k)
    return np.where(r2 > k * k + k, k + 1, k)


def ring_map(N):
    i = np.arange(N)
    return ring_of(i[:, None], i[None, :], N)


def rapsd_ref(x, counts):
    """float64 definition with the integer ring rule, x [..., N, N] -> [..., N/2 + 1]; ``counts``: the divisors (ring_counts)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[-1]
    K = N // 2 + 1
    k = ring_map(N).ravel()
    keep = k < K
    flat = (np.abs(np.fft.fft2(x)) ** 2 / (N * N)).reshape(-1, N * N)
    sums = np.stack([np.bincount(k[keep], weights=row[keep], minlength=K) for row in flat])
    return (sums / np.asarray(counts, dtype=np.float64)).reshape(x.shape[:-2] + (K,))


# ---------------------------------------------------------------------------------------------------------------- exhaustive
def exhaustive_freqs(N):
    a, b = np.meshgrid(np.arange(N), np.arange(N // 2 + 1), indexing="ij")
    return a.ravel(), b.ravel()


@functools.lru_cache(maxsize=None)
def exhaustive(N):
    """float32 [N (N/2 + 1), 1, N, N]: field f = cos(2 pi (a_f h + b_f w) / N + PHI).  The argument is reduced in integers."""
    a, b = exhaustive_freqs(N)
    table = np.cos(2 * np.pi * np.arange(N) / N + PHI)
    h = np.arange(N)
    idx = (a[:, None, None] * h[None, :, None] + b[:, None, None] * h[None, None, :]) % N
    return table[idx].astype(np.float32)[:, None]


def exhaustive_expected(N, counts):
    """float64 [F, N/2 + 1]: the analytic spectra of ``exhaustive(N)``, and k0 [F] (> N/2: a corner, nothing anywhere)."""
    a, b = exhaustive_freqs(N)
    k0 = ring_of(a, b, N)
    selfconj = np.isin(a, (0, N // 2)) & np.isin(b, (0, N // 2))
    power = np.where(selfconj, N * N * np.cos(PHI) ** 2, N * N / 2.0)
    want = np.zeros((a.size, N // 2 + 1))
    inside = k0 <= N // 2
    f = np.nonzero(inside)[0]
    want[f, k0[f]] = power[f] / np.asarray(counts, dtype=np.float64)[k0[f]]
    return want, k0


# ---------------------------------------------------------------------------------------------------------------- one per ring
@functools.lru_cache(maxsize=None)
def ring_points(N):
    """[4][N/2] (a signed, b) of the cosine of ring k = 1 .. N/2 in each of the four fields, enumerated in integers over the half
    plane b = 0 .. N/2, |a| <= N/2."""
    h = N // 2
    a, b = np.meshgrid(np.arange(0, h + 1), np.arange(0, h + 1), indexing="ij")
    a, b = a.ravel(), b.ravel()
    ok = ~((np.isin(a, (0, h))) & (np.isin(b, (0, h))))          # no self-conjugate point: every cosine has power N^2 / 2
    a, b = a[ok], b[ok]
    r2 = a.astype(np.int64) ** 2 + b.astype(np.int64) ** 2
    k = ring_of(a, b, N)
    pts = [[], [], [], []]
    order = np.lexsort((a, r2, k))                               # by ring, then r^2, then a
    a, b, r2, k = a[order], b[order], r2[order], k[order]
    start = np.searchsorted(k, np.arange(1, h + 2))
    for kk in range(1, h + 1):
        lo, hi = start[kk - 1], start[kk]
        assert hi > lo, (N, kk)
        first, last = (int(a[lo]), int(b[lo])), (int(a[hi - 1]), int(b[hi - 1]))
        assert r2[lo] >= kk * kk - kk + 1 and r2[hi - 1] <= kk * kk + kk
        nyq = [(int(a[i]), int(b[i])) for i in range(lo, hi) if b[i] == h and 0 < a[i] < h]
        pts[0].append(first)
        pts[1].append(last)
        pts[2].append(nyq[0] if nyq else first)
        pts[3].append((-last[0], last[1]))
    return pts


def phase(k):
    return (0.3 + 0.7 * k) % (2 * np.pi)


@functools.lru_cache(maxsize=None)
def one_per_ring(N):
    """float64 [4, N, N]: CONST + sum over k = 1 .. N/2 of cos(2 pi (a_k h + b_k w) / N + phase(k))."""
    out = np.empty((4, N, N))
    for f, pts in enumerate(ring_points(N)):
        X = np.zeros((N, N), dtype=np.complex128)
        X[0, 0] = N * N * CONST
        for kk, (a, b) in enumerate(pts, start=1):
            z = 0.5 * N * N * np.exp(1j * phase(kk))
            X[a % N, b % N] += z
            X[-a % N, -b % N] += np.conj(z)
        x = np.fft.ifft2(X)
        assert np.abs(x.imag).max() <= 1e-9
        out[f] = x.real
    return out


def one_per_ring_expected(N, counts):
    """float64 [N/2 + 1]: the analytic ring means of every field of ``one_per_ring(N)``: CONST^2 N^2 in ring 0, N^2 / 2 over the
    ring's count elsewhere."""
    want = N * N / 2.0 / np.asarray(counts, dtype=np.float64)
    want[0] = CONST * CONST * N * N
    return want
