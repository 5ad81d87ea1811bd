"""Fields, ring rule and float64 references of the every-frequency tests of the four column kernels of csrc/spectra.hip:
dg_rapsd (tests/test_spectra_rings_gpu.py), dg_cross_rapsd, dg_helmholtz and dg_helmholtz_cross
(tests/test_spectra_rings_pair_gpu.py) on the device, tests/test_spectra_rings_cpu.py for the references themselves.

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

The paired kernels (cross spectra, Helmholtz spectra) add to the ring walk a geometry per point (signed ky, k2, the Nyquist
flag) and the Nyquist rule, a second formula at every point with u = N/2 or v = N/2.  ``cross_ref`` / ``helm_cross_ref`` are the
FULL-SPECTRUM definitions of include/downgan_hip.h and know nothing of half spectra; ``half_spectrum_eval`` restates what the
kernels do (and can be told to do it wrong at one frequency: the mutation check).

``exhaustive_pair(N)``: two vector fields (u, v) per (a, b), side a = (1, 0.5) cos(.. + PHI), side b = (bu, bv) cos(.. + PHI +
delta) with amplitudes and delta that depend on (a, b).  (1, 0.5) tells kx from ky, ky from -ky and u from v; delta and the
signs of (bu, bv) make the co-planes negative at half of the frequencies.  ``exhaustive_pair_expected`` is the analytic answer.

``one_per_ring_pair(N)``: the four fields of ``one_per_ring`` as side a = (1, 0.5) f; side b has on ring k the amplitudes
(0.75 - 0.5 (k mod 3), 1.25 - 0.5 (k mod 4)), a phase 2 pi (k mod 7) / 7 ahead of a's, and the constants (0.5, -1) CONST.
"""
from __future__ import annotations

import functools
import math

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


# ------------------------------------------------------------------------------------- full-spectrum definitions of the pairs
@functools.lru_cache(maxsize=4)
def _ring_flat(N):
    k = ring_map(N).ravel()
    keep = k <= N // 2
    return keep, k[keep]


def _ring_means(planes, counts):
    """[..., N, N] -> [..., N/2 + 1]: sums over the rings of the integer rule (corners dropped), divided by ``counts``."""
    N = planes.shape[-1]
    K = N // 2 + 1
    keep, k = _ring_flat(N)
    flat = planes.reshape(-1, N * N)
    sums = np.stack([np.bincount(k, weights=row[keep], minlength=K) for row in flat])
    return (sums / np.asarray(counts, dtype=np.float64)).reshape(planes.shape[:-2] + (K,))


def _fft2_64(x, fft2):
    return np.asarray(fft2(np.asarray(x, dtype=np.float64))).astype(np.complex128)


def _chunks(T, N):
    step = max(1, (1 << 20) // (N * N))                           # at most 2^20 points per component at a time
    return [(t0, min(T, t0 + step)) for t0 in range(0, T, step)]


def cross_ref(a, b, counts, fft2=np.fft.fft2):
    """The definition ("Cross spectra"), float64: a, b [..., N, N] -> [..., 3, N/2 + 1], ring means of |A|^2 / N^2, |B|^2 / N^2 and
    Re(A conj B) / N^2 over the full spectrum.  Another ``fft2`` (an fp32 one) shows what its precision alone costs."""
    a, b = np.asarray(a), np.asarray(b)
    N = a.shape[-1]
    fa, fb = a.reshape(-1, N, N), b.reshape(-1, N, N)
    out = np.empty((fa.shape[0], 3, N // 2 + 1))
    for t0, t1 in _chunks(fa.shape[0], N):
        A, B = _fft2_64(fa[t0:t1], fft2), _fft2_64(fb[t0:t1], fft2)
        planes = np.stack([np.abs(A) ** 2, np.abs(B) ** 2, np.real(A * np.conj(B))], axis=1) / (N * N)
        out[t0:t1] = _ring_means(planes, counts)
    return out.reshape(a.shape[:-2] + (3, N // 2 + 1))


def helm_cross_ref(a, b, counts, scale=(1.0, 1.0), fft2=np.fft.fft2):
    """The definition ("Helmholtz spectra"), float64: a, b [..., 2, N, N] (u, v) -> [..., 8, N/2 + 1], ring means of ke, rot, div
    of a, of b, co_rot, co_div over the FULL spectrum: kx = fftfreq along W, ky along H, no Nyquist shortcut.  Planes 0-2 are the
    one-sided definition."""
    a, b = np.asarray(a), np.asarray(b)
    N = a.shape[-1]
    f = np.fft.fftfreq(N) * N
    kx, ky = f[None, :], f[:, None]
    k2 = kx ** 2 + ky ** 2
    g = np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2)) / (2.0 * N * N)
    fa, fb = a.reshape(-1, 2, N, N), b.reshape(-1, 2, N, N)
    out = np.empty((fa.shape[0], 8, N // 2 + 1))
    for t0, t1 in _chunks(fa.shape[0], N):
        planes, RD = [], []
        for x in (fa, fb):
            U, V = scale[0] * _fft2_64(x[t0:t1, 0], fft2), scale[1] * _fft2_64(x[t0:t1, 1], fft2)
            R, D = kx * V - ky * U, kx * U + ky * V
            RD.append((R, D))
            planes += [(np.abs(U) ** 2 + np.abs(V) ** 2) / (2.0 * N * N), np.abs(R) ** 2 * g, np.abs(D) ** 2 * g]
        planes += [np.real(RD[0][0] * np.conj(RD[1][0])) * g, np.real(RD[0][1] * np.conj(RD[1][1])) * g]
        out[t0:t1] = _ring_means(np.stack(planes, axis=1), counts)
    return out.reshape(a.shape[:-3] + (8, N // 2 + 1))


def helm_measure(got, ref):
    """max over fields and rings of |got - ref| / ke_ref per plane ([..., 3, K] or [..., 8, K]; the co-planes against
    sqrt(ke_a ke_b)): the measure of tests/test_helmholtz_gpu.py's check_planes."""
    ka = ref[..., 0:1, :]
    den = [ka] * 3
    if ref.shape[-2] == 8:
        kb = ref[..., 3:4, :]
        den += [kb] * 3 + [np.sqrt(ka * kb)] * 2
    den = np.concatenate(den, axis=-2)
    assert (den > 0).all()
    err = np.abs(got - ref) / den
    return [float(err[..., p, :].max()) for p in range(ref.shape[-2])]


def cross_measure(got, ref):
    """(planes 0, 1 relative, plane 2 against sqrt(Paa Pbb)): the measure of tests/test_coherence_gpu.py."""
    e01 = np.abs(got[..., :2, :] / ref[..., :2, :] - 1).max()
    e2 = (np.abs(got[..., 2, :] - ref[..., 2, :]) / np.sqrt(ref[..., 0, :] * ref[..., 1, :])).max()
    return float(e01), float(e2)


# ----------------------------------------------------------------------------------------------------------- exhaustive pairs
def exhaustive_pair_amps(N, scale=(1.0, 1.0), pair=(0, 1)):
    """(xa [F, 2], xb [F, 2], delta [F], ca [F, 2], cb [F, 2]): the amplitudes (xu, xv) each side's Helmholtz planes see, i.e.
    channels ``pair`` times ``scale``, side b's phase lead, and the amplitudes of the stored channels."""
    a, b = exhaustive_freqs(N)
    ca = np.stack([np.ones(a.size), np.full(a.size, 0.5)], axis=1)
    cb = np.stack([0.75 - 0.5 * ((a + 2 * b) % 3), 1.25 - 0.5 * ((2 * a + b) % 4)], axis=1)
    delta = 2 * np.pi * ((3 * a + 5 * b) % 7) / 7
    seen = lambda c: np.stack([scale[0] * c[:, pair[0]], scale[1] * c[:, pair[1]]], axis=1)
    return seen(ca), seen(cb), delta, ca, cb


@functools.lru_cache(maxsize=None)
def exhaustive_pair(N):
    """(A, B) float32 [N (N/2 + 1), 2, N, N] each, one pair per frequency of ``exhaustive_freqs``: side a = (1, 0.5) c with c the
    field of ``exhaustive``, side b = (bu, bv) cos(same argument + PHI + delta).  Arguments reduced in integers."""
    a, b = exhaustive_freqs(N)
    _, _, delta, ca, cb = exhaustive_pair_amps(N)
    m, h = np.arange(N), np.arange(N)
    idx = (a[:, None, None] * h[None, :, None] + b[:, None, None] * h[None, None, :]) % N
    c = np.cos(2 * np.pi * m / N + PHI)[idx]
    table = np.cos(2 * np.pi * m[None, :] / N + PHI + delta[:, None])
    cp = table[np.arange(a.size)[:, None, None], idx]
    A = (ca[:, :, None, None] * c[:, None]).astype(np.float32)
    B = (cb[:, :, None, None] * cp[:, None]).astype(np.float32)
    return A, B


def _exhaustive_geometry(N):
    a, b = exhaustive_freqs(N)
    selfc = np.isin(a, (0, N // 2)) & np.isin(b, (0, N // 2))
    nyq = (a == N // 2) | (b == N // 2)
    return a, b, ring_of(a, b, N), selfc, nyq


def exhaustive_pair_expected(N, counts, scale=(1.0, 1.0), pair=(0, 1)):
    """(helm float64 [F, 8, K], cross float64 [F, 2, 3, K], k0 [F]): the analytic spectra of ``exhaustive_pair(N)`` as
    helmholtz_cross(A, B, scale=, pair=) and cross_rapsd(A, B) define them.  Everything lies on ring k0; k0 > N/2 (a corner):
    nothing anywhere.  With W(px, py) = N^2 / 4 cos(px - py), at self-conjugate points N^2 / 2 cos(PHI + px) cos(PHI + py):
    ke = (xu yu + xv yv) W, rot = W (kx xv - ky xu)(kx yv - ky yu) / k2, div = W (kx xu + ky xv)(kx yu + ky yv) / k2, on the
    Nyquist row and column (where the frequency and its fftfreq alias (-N/2) share the power) without the cross terms."""
    a, b, k0, selfc, nyq = _exhaustive_geometry(N)
    counts = np.asarray(counts, dtype=np.float64)
    xa, xb, delta, ca, cb = exhaustive_pair_amps(N, scale, pair)
    ky, kx = signed(a, N).astype(np.float64), b.astype(np.float64)
    k2 = kx * kx + ky * ky
    ik2 = np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2))

    def W(px, py):
        return np.where(selfc, N * N / 2.0 * np.cos(PHI + px) * np.cos(PHI + py), N * N / 4.0 * np.cos(px - py))

    def planes(x, y, w):
        (xu, xv), (yu, yv) = x.T, y.T
        rot = np.where(nyq, kx * kx * xv * yv + ky * ky * xu * yu, (kx * xv - ky * xu) * (kx * yv - ky * yu))
        div = np.where(nyq, kx * kx * xu * yu + ky * ky * xv * yv, (kx * xu + ky * xv) * (kx * yu + ky * yv))
        return [(xu * yu + xv * yv) * w, w * rot * ik2, w * div * ik2]

    zero = np.zeros_like(delta)
    vals = np.stack(planes(xa, xa, W(zero, zero)) + planes(xb, xb, W(delta, delta)) + planes(xa, xb, W(zero, delta))[1:], axis=1)
    cvals = np.stack([2 * W(zero, zero)[:, None] * ca ** 2, 2 * W(delta, delta)[:, None] * cb ** 2,
                      2 * W(zero, delta)[:, None] * ca * cb], axis=2)                       # [F, 2, 3]
    K = N // 2 + 1
    f = np.nonzero(k0 < K)[0]
    helm, cross = np.zeros((a.size, 8, K)), np.zeros((a.size, 2, 3, K))
    helm[f, :, k0[f]] = vals[f] / counts[k0[f], None]
    cross[f, :, :, k0[f]] = cvals[f] / counts[k0[f], None, None]
    return helm, cross, k0


def exhaustive_pair_envelopes(N, counts, scale=(1.0, 1.0), pair=(0, 1)):
    """The scales of the comparator, none of which depends on a phase: (E_helm [F, 8], amp_helm [F, 8], E_cross [F, 2, 3],
    amp_cross [F, 2, 3]).  amp: xu^2 + xv^2 of the plane's side (co-planes: the geometric mean of the sides), for the cross
    planes the channel's amplitude squared (plane 2: |xa xb|).  E, on ring k0: N^2 / 4 amp / count (N^2 / 2 at self-conjugate
    points) for the Helmholtz planes, N^2 / 2 amp / count for the cross planes; 1 for the corners, which have no ring."""
    a, b, k0, selfc, _ = _exhaustive_geometry(N)
    xa, xb, _, ca, cb = exhaustive_pair_amps(N, scale, pair)
    sa, sb = (xa ** 2).sum(1), (xb ** 2).sum(1)
    amp_h = np.stack([sa] * 3 + [sb] * 3 + [np.sqrt(sa * sb)] * 2, axis=1)
    amp_c = np.stack([ca ** 2, cb ** 2, np.abs(ca * cb)], axis=2)
    inside = k0 <= N // 2
    cnt = np.asarray(counts, dtype=np.float64)[np.where(inside, k0, 0)]
    e_h = np.where(inside[:, None], np.where(selfc, N * N / 2.0, N * N / 4.0)[:, None] * amp_h / cnt[:, None], 1.0)
    e_c = np.where(inside[:, None, None], N * N / 2.0 * amp_c / cnt[:, None, None], 1.0)
    return e_h, amp_h, e_c, amp_c


ON_TOL = 1e-5             # |got - want| <= ON_TOL * E on the ring that holds the wave (the project's bound for single waves)
OFF_TOL = 1e-7            # |got| <= OFF_TOL * N^2 * amp on every other ring


def exhaustive_errors(got, want, k0, E, amp, N):
    """got, want [F, P, K], E, amp [F, P] -> (on [F, P]: |got - want| / E on ring k0, 0 for the corners; off [F, P]: the largest
    |got| / (N^2 amp) over every other ring, for the corners over every ring)."""
    F, P, K = got.shape
    inside = k0 < K
    f = np.arange(F)
    on = np.where(inside[:, None], np.abs(got - want)[f, :, np.where(inside, k0, 0)] / E, 0.0)
    other = np.ones((F, K), dtype=bool)
    other[f[inside], k0[inside]] = False
    off = np.where(other[:, None, :], np.abs(got), 0.0).max(-1) / (N * N * amp)
    return on, off


def check_exhaustive(name, got, want, k0, E, amp, N):
    """The comparator of the exhaustive tests: every frequency, every plane, both bounds; the worst frequency is named as
    (a, b, k0, plane).  -> (worst on-ring value, worst off-ring value)."""
    a, b = exhaustive_freqs(N)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.shape[:2] == E.shape == amp.shape, (name, got.shape, want.shape, E.shape)
    assert np.isfinite(got).all(), name
    on, off = exhaustive_errors(got, want, k0, E, amp, N)
    print(f"[rings-pair] N={N} {name}: {got.shape[0]} frequencies x {got.shape[1]} planes, worst |got - want| / E on the ring "
          f"{on.max():.3e} (bound {ON_TOL:.0e}), worst |got| / (N^2 amp) elsewhere {off.max():.3e} (bound {OFF_TOL:.0e})")
    f, p = np.unravel_index(int(np.argmax(on)), on.shape)
    kk = min(int(k0[f]), N // 2)
    assert on.max() <= ON_TOL, (name, "on ring", (int(a[f]), int(b[f]), int(k0[f]), int(p)), got[f, p, kk], want[f, p, kk], on.max())
    f, p = np.unravel_index(int(np.argmax(off)), off.shape)
    assert off.max() <= OFF_TOL, (name, "off ring", (int(a[f]), int(b[f]), int(k0[f]), int(p)), np.abs(got[f, p]).max(), off.max())
    return float(on.max()), float(off.max())


# ------------------------------------------------------------------------------------------------------- one per ring, paired
@functools.lru_cache(maxsize=None)
def one_per_ring_pair(N, fields=(0, 1, 2, 3)):
    """(A, B) float64 [len(fields), 2, N, N] on the lattice points of ``ring_points``: A = (1, 0.5) one_per_ring(N); B has on
    ring k the amplitudes (0.75 - 0.5 (k mod 3), 1.25 - 0.5 (k mod 4)), the phase phase(k) + 2 pi (k mod 7) / 7 and the constants
    (0.5, -1) CONST."""
    f = one_per_ring(N)[list(fields)]
    A = np.stack([f, 0.5 * f], axis=1)
    B = np.empty_like(A)
    ks = np.arange(1, N // 2 + 1)
    amps = (0.75 - 0.5 * (ks % 3), 1.25 - 0.5 * (ks % 4))
    lead = 2 * np.pi * (ks % 7) / 7
    for i, fi in enumerate(fields):
        for c, const in enumerate((0.5 * CONST, -1.0 * CONST)):
            X = np.zeros((N, N), dtype=np.complex128)
            X[0, 0] = N * N * const
            for kk, (a, b) in enumerate(ring_points(N)[fi], start=1):
                z = 0.5 * N * N * amps[c][kk - 1] * np.exp(1j * (phase(kk) + lead[kk - 1]))
                X[a % N, b % N] += z
                X[-a % N, -b % N] += np.conj(z)
            x = np.fft.ifft2(X)
            assert np.abs(x.imag).max() <= 1e-9
            B[i, c] = x.real
    return A, B


# --------------------------------------------------------------------------------------------- what the kernels do, restated
def ring_span(u, k, N):
    """(vmin, vmax): the |v| of ring k on line u, in integers (csrc/spectra.hip's ring_span); empty when vmin > vmax."""
    hi = k * k + k - u * u
    if hi < 0:
        return 1, 0
    lo = max((0 if k == 0 else k * k - k + 1) - u * u, 0)
    vmin = math.isqrt(lo)
    return vmin + (vmin * vmin < lo), min(math.isqrt(hi), N // 2)


def half_spectrum_eval(A, B, counts, fault=None, scale=(1.0, 1.0)):
    """(helm [..., 8, K], cross [..., 2, 3, K]) of A, B [..., 2, N, N] the way the column kernels evaluate them, in float64:
    lines u = 0 .. N/2 of the half spectrum (u along W), the Hermitian weight (1 on u = 0 and u = N/2, else 2), per point
    kx = u, ky = v or v - N, g = weight / (2 N^2 k2) (0 at k2 = 0), the NYQUIST RULE (no cross term where u = N/2 or v = N/2),
    then per line and ring the walk v = vmin .. vmax of ``ring_span`` with the partner N - v unless v is 0 or N/2.

    ``fault`` = (kind, u, v) plants one single-frequency error at point (u, v) of the half spectrum:
      "ring"     the point is summed into the next ring (an off-by-one vmax at the ring's outer edge)
      "weight"   twice the weight (2 instead of 1 on line u = 0)
      "ky"       ky = N - v instead of v - N (not negated, v > N/2)
      "partner"  the partner N - v taken although v = N/2: the point counts twice
      "cross"    the general formula, cross term included, at a Nyquist point
      "swap"     co_rot and co_div exchanged
      "abs"      co_rot and co_div lose their sign"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    N = A.shape[-1]
    K = N // 2 + 1
    kind, fu, fv = fault if fault is not None else (None, None, None)
    u, v = np.arange(K)[None, :], np.arange(N)[:, None]
    kx, ky = np.broadcast_to(u, (N, K)).astype(np.float64), np.broadcast_to(np.where(v <= N // 2, v, v - N), (N, K)).astype(np.float64)
    nyq = np.broadcast_to((u == N // 2) | (v == N // 2), (N, K)).copy()
    w = np.broadcast_to(np.where((u == 0) | (u == N // 2), 1.0, 2.0), (N, K)).copy()
    if kind == "ky":
        ky[fv, fu] = N - fv
    if kind == "cross":
        nyq[fv, fu] = False
    if kind == "weight":
        w[fv, fu] *= 2.0
    k2 = kx * kx + ky * ky
    g = w * np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2)) / (2.0 * N * N)
    M = np.zeros((K, N, K))                                         # times point (v, u) is added to ring k
    for uu in range(K):
        for k in range(K):
            vmin, vmax = ring_span(uu, k, N)
            for vv in range(vmin, vmax + 1):
                M[k, vv, uu] += 1
                if vv != 0 and vv != N // 2:
                    M[k, N - vv, uu] += 1
    if kind == "ring":
        k = int(np.argmax(M[:, fv, fu]))
        assert M[k, fv, fu] == 1 and k + 1 < K
        M[k, fv, fu], M[k + 1, fv, fu] = 0, 1
    if kind == "partner":
        assert fv == N // 2 and M[:, fv, fu].sum() == 1
        M[:, fv, fu] *= 2

    def dot(x, y):
        return np.real(x * np.conj(y))

    def products(Ua, Va, Ub, Vb):
        rot = np.where(nyq, kx * kx * dot(Va, Vb) + ky * ky * dot(Ua, Ub), dot(kx * Va - ky * Ua, kx * Vb - ky * Ub))
        div = np.where(nyq, kx * kx * dot(Ua, Ub) + ky * ky * dot(Va, Vb), dot(kx * Ua + ky * Va, kx * Ub + ky * Vb))
        return [rot * g, div * g]

    SA, SB = np.fft.rfft2(A), np.fft.rfft2(B)                       # [..., 2, v, u]
    sides = [(scale[0] * S[..., 0, :, :], scale[1] * S[..., 1, :, :]) for S in (SA, SB)]
    planes = []
    for U, V in sides:
        planes += [(dot(U, U) + dot(V, V)) * w / (2.0 * N * N)] + products(U, V, U, V)
    co = products(*sides[0], *sides[1])
    if kind == "swap":
        co[0][..., fv, fu], co[1][..., fv, fu] = co[1][..., fv, fu].copy(), co[0][..., fv, fu].copy()
    if kind == "abs":
        co = [c.copy() for c in co]
        for c in co:
            c[..., fv, fu] = np.abs(c[..., fv, fu])
    helm = np.einsum("...pvu,kvu->...pk", np.stack(planes + co, axis=-3), M) / np.asarray(counts, dtype=np.float64)
    cplanes = np.stack([dot(SA, SA), dot(SB, SB), dot(SA, SB)], axis=-3) * w / (N * N)       # [..., 2, 3, v, u]
    cross = np.einsum("...pvu,kvu->...pk", cplanes, M) / np.asarray(counts, dtype=np.float64)
    return helm, cross
