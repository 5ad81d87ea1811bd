"""Radially averaged power spectra (RAPSD) of real and generated fields, computed on the GPU (csrc/spectra.hip).

The per-scale diagnostic of a downscaling generator: does it put the right amount of variance at the small scales the coarse
input lacks?  For one square field x (N x N, N a power of two, 16 <= N <= 2048):

    P = |fft2(x)|^2 / N^2,  f = fftfreq(N) * N (signed integer frequencies),  r^2 = f_u^2 + f_v^2
    ring k: (2k - 1)^2 <= 4 r^2 < (2k + 1)^2  (= floor(r + 1/2), evaluated exactly in integers),  k = 0 .. N/2
    S[k] = mean of P over ring k   (the corners, k > N/2, are dropped; no windowing, no mean removal)

``rapsd`` reads NCHW tensors, the resident feed's ``[n, H, W, c]`` store and the generator's padded NHWC output in place
(fp32 or bf16).  ``RadialSpectrum`` accumulates the spectra of many batches on the device (and over data-parallel ranks);
the trainer's opt-in hook (``WassersteinGAN.log_spectra``) keeps one for the real and one for the generated fields.  Every
reduction runs in a fixed order: two calls on the same data are bit-identical.

The RAPSD is phase-blind: a generator can match it perfectly while every small-scale phase is unrelated to the truth.
``cross_rapsd`` takes the PAIRED fields a, b (A = fft2(a), B = fft2(b)) and returns three ring means per wavenumber,

    plane 0 = |A|^2 / N^2,  plane 1 = |B|^2 / N^2,  plane 2 = Re(A conj B) / N^2   (planes 0, 1: bit-equal to ``rapsd``)

from which follow the ``coherence`` s2 / sqrt(s0 s1), the ``error_spectrum`` s0 + s1 - 2 s2 (the ring power of a - b) and the
``effective_resolution``: the last wavenumber down to which the coherence stays above a threshold, i.e. the scale below which
the generated field is only plausible texture.  ``CrossSpectrum`` is the accumulator (``WassersteinGAN.log_coherence``).

All of the above look at one channel at a time.  ``helmholtz_rapsd`` takes the wind as a vector: the kinetic energy per wavenumber
and its split into a rotational (vortical) and a divergent part, which depends on the phase relation between the two components'
spectra; ``helmholtz_cross`` adds, for the paired real and generated winds, the co-spectra of each part, from which follow
``helmholtz_coherence`` and an ``effective_resolution`` per part -- down to which scale the generator reproduces the real vortical
flow, and down to which the divergent one -- next to ``divergent_fraction`` and ``spectral_slope``.  ``HelmholtzSpectrum`` is the
accumulator (``WassersteinGAN.log_helmholtz``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fields import default_ops, descriptor as _descriptor, n_valid as _n_valid, pair as _paired, series

N_MIN, N_MAX = 16, _lib.RAPSD_MAX_N
C_MAX = _lib.EOF_MAX_C
WS_CAP = 512 << 20           # bytes of dg_rapsd workspace at most: longer series are split into chunks of fields

_ops = {}                    # device -> op backend of the module-level calls


def _default_ops(device):
    return default_ops(_ops, device)


def check_n(N):
    """ValueError unless N is a power of two in [N_MIN, N_MAX]."""
    if not (isinstance(N, (int, np.integer)) and N_MIN <= N <= N_MAX and (N & (N - 1)) == 0):
        raise ValueError(f"RAPSD needs square N x N fields with N a power of two, {N_MIN} <= N <= {N_MAX} (got N = {N})")


def wavenumbers(N):
    """The ring index k = 0 .. N/2 of each bin (cycles per field side)."""
    check_n(N)
    return np.arange(N // 2 + 1)


def ring_counts(N):
    """int64 [N/2 + 1]: number of frequency pairs in each ring, as the kernels count them (dg_rapsd_ring_counts)."""
    check_n(N)
    out = np.zeros(N // 2 + 1, dtype=np.int64)
    _lib.check(_lib.lib().dg_rapsd_ring_counts(int(N), out.ctypes.data_as(C.POINTER(C.c_int64))), "dg_rapsd_ring_counts")
    return out


def _fields(x, channels, nhwc):
    """Validate without touching a device -> the ``fields.Series`` (tensor, nhwc, C, T, N, N)."""
    s = series(x, channels, nhwc, "RAPSD")
    if s.H != s.W:
        raise ValueError(f"RAPSD needs square fields (got {s.H} x {s.W})")
    check_n(s.H)
    return s


def _chunk(o, T, Cn, N):
    """Most fields per dg_rapsd call with a workspace of at most WS_CAP bytes (at least one)."""
    tc = min(T, max(1, WS_CAP // max(1, o.rapsd_ws_bytes(1, Cn, N))))
    while tc > 1 and o.rapsd_ws_bytes(tc, Cn, N) > WS_CAP:
        tc -= 1
    return tc


def _sum_into(o, x, nhwc, Cn, T, N, total):
    """total [C, K] fp64 (device) += sum over the T fields of their spectra; chunk sums added in order."""
    tc = _chunk(o, T, Cn, N)
    part = torch.empty_like(total)
    for t0 in range(0, T, tc):
        xs, f = _descriptor(o, x[t0:t0 + tc], nhwc, Cn)
        o.rapsd(f, N, sum=part)
        total += part


def rapsd(x, channels=None, nhwc=False, per_field=False, ops=None):
    """Radially averaged power spectra of a series of square fields on the GPU.

    x: device tensor [T, C, N, N] (fp32 / bf16), or with ``nhwc`` a dense-pixel [T, N, N, c_pad] store of which the leading
    ``channels`` are read (the generator's padded output; default: all), or a ``dataloader.NativeBatch``.
    Returns float64 [C, N/2 + 1], the mean over T, or [T, C, N/2 + 1] with ``per_field``."""
    x, nhwc, Cn, T, N = _fields(x, channels, nhwc)[:5]
    o = ops if ops is not None else _default_ops(x.device)
    K = N // 2 + 1
    if per_field:
        out = torch.empty(T, Cn, K, dtype=torch.float64, device=x.device)
        tc = _chunk(o, T, Cn, N)
        for t0 in range(0, T, tc):
            xs, f = _descriptor(o, x[t0:t0 + tc], nhwc, Cn)
            o.rapsd(f, N, per_field=out[t0:t0 + tc])
        return out
    total = torch.zeros(Cn, K, dtype=torch.float64, device=x.device)
    _sum_into(o, x, nhwc, Cn, T, N, total)
    return total / T


def log_spectral_distance(p_ref, p, kmin=1):
    """sqrt(mean over k >= kmin of (10 log10(p / p_ref))^2) per channel: [C, K] -> numpy [C] ([K] -> a float)."""
    host = lambda v: v.detach().cpu().double().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)
    a, b = host(p_ref), host(p)
    if a.shape != b.shape or a.shape[-1] <= kmin:
        raise ValueError(f"log_spectral_distance: shapes {a.shape} / {b.shape} with kmin = {kmin}")
    d = 10.0 * np.log10(b[..., kmin:] / a[..., kmin:])
    out = np.sqrt(np.mean(d * d, axis=-1))
    return float(out) if out.ndim == 0 else out


def _pair(a, b, channels, nhwc, nhwc_b):
    """Validate both sides and their agreement without touching a device -> ((a, nhwc_a), (b, nhwc_b), C, T, N)."""
    a, b = _fields(a, channels, nhwc), _fields(b, channels, nhwc if nhwc_b is None else nhwc_b)
    _paired(a, b, ("a", "b"))
    return a[:2], b[:2], a.C, a.T, a.H


def _cross_chunk(o, T, Cn, N):
    """Pairs per dg_cross_rapsd call: the fewest calls whose workspace stays within WS_CAP bytes (at least one pair a call),
    then the T pairs spread evenly over them (32 go as 16 + 16, not 31 + 1)."""
    tc = min(T, max(1, WS_CAP // max(1, o.cross_rapsd_ws_bytes(1, Cn, N))))
    while tc > 1 and o.cross_rapsd_ws_bytes(tc, Cn, N) > WS_CAP:
        tc -= 1
    calls = -(-T // tc)
    return -(-T // calls)


def _cross_sum_into(o, a, b, Cn, T, N, total):
    """total [C, 3, K] fp64 (device) += sum over the T pairs of their cross spectra; chunk sums added in order."""
    (a, na), (b, nb) = a, b
    tc = _cross_chunk(o, T, Cn, N)
    part = torch.empty_like(total)
    for t0 in range(0, T, tc):
        xa, fa = _descriptor(o, a[t0:t0 + tc], na, Cn)
        xb, fb = _descriptor(o, b[t0:t0 + tc], nb, Cn)
        o.cross_rapsd(fa, fb, N, sum=part)
        total += part


def cross_rapsd(a, b, channels=None, nhwc=False, nhwc_b=None, per_field=False, ops=None):
    """Radially averaged cross spectra of a series of paired square fields on the GPU.

    a, b: as ``rapsd``'s x, with the same T, C and N; the layouts (``nhwc`` for a, ``nhwc_b`` for b, default: as a) and the
    dtypes are independent (the trainer's real side is the staged NHWC store, its generated side the padded bf16 output).
    Returns float64 [C, 3, N/2 + 1], the mean over T of the planes |A|^2 / N^2, |B|^2 / N^2 and Re(A conj B) / N^2, or
    [T, C, 3, N/2 + 1] with ``per_field``.  Per library call planes 0 and 1 equal ``dg_rapsd`` of
    a and of b bit for bit, and so do they here whenever ``rapsd`` splits the series into the same calls (always when both fit
    one call); where they split differently the slice sums run in another order and the two agree to fp64 rounding.
    Cross-channel coherence (u against v of one field) needs nothing extra: ``cross_rapsd(x[:, :1], x[:, 1:2])``."""
    sa, sb, Cn, T, N = _pair(a, b, channels, nhwc, nhwc_b)
    dev = sa[0].device
    o = ops if ops is not None else _default_ops(dev)
    K = N // 2 + 1
    if per_field:
        out = torch.empty(T, Cn, 3, K, dtype=torch.float64, device=dev)
        tc = _cross_chunk(o, T, Cn, N)
        for t0 in range(0, T, tc):
            xa, fa = _descriptor(o, sa[0][t0:t0 + tc], sa[1], Cn)
            xb, fb = _descriptor(o, sb[0][t0:t0 + tc], sb[1], Cn)
            o.cross_rapsd(fa, fb, N, per_field=out[t0:t0 + tc])
        return out
    total = torch.zeros(Cn, 3, K, dtype=torch.float64, device=dev)
    _cross_sum_into(o, sa, sb, Cn, T, N, total)
    return total / T


def _host(v):
    return v.detach().cpu().double().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64)


def _planes(s):
    s = _host(s)
    if s.ndim < 2 or s.shape[-2] != 3:
        raise ValueError(f"cross spectra are [..., 3, K] (got shape {s.shape})")
    return s[..., 0, :], s[..., 1, :], s[..., 2, :]


def coherence(s):
    """s2 / sqrt(s0 s1) per wavenumber: cross spectra [..., 3, K] -> numpy float64 [..., K]; NaN where the denominator is 0."""
    s0, s1, s2 = _planes(s)
    den = np.sqrt(s0 * s1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, np.nan, s2 / den)


def error_spectrum(s):
    """s0 + s1 - 2 s2, the ring power of a - b: [..., 3, K] -> numpy float64 [..., K]."""
    s0, s1, s2 = _planes(s)
    return s0 + s1 - 2.0 * s2


def relative_error_spectrum(s):
    """error_spectrum / s0 (the error's power relative to side a's, 2 for unrelated fields of equal power): [..., K]."""
    s0, _, _ = _planes(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        return error_spectrum(s) / s0


def effective_resolution(coh, threshold=0.5):
    """The largest k in 1 .. N/2 with coh[..., j] >= threshold for every 1 <= j <= k (0 when ring 1 fails; a NaN ring fails;
    ring 0, the mean, is ignored): coherence [..., K] -> numpy int64 [...] ([K] -> an int)."""
    c = _host(coh)
    if c.ndim < 1 or c.shape[-1] < 2:
        raise ValueError(f"effective_resolution: coherence is [..., K] with K >= 2 (got shape {c.shape})")
    with np.errstate(invalid="ignore"):
        ok = c[..., 1:] >= threshold                          # NaN compares false
    k = np.logical_and.accumulate(ok, axis=-1).sum(axis=-1).astype(np.int64)
    return int(k) if k.ndim == 0 else k


def wavelength_px(k_eff, N):
    """N / k_eff, the wavelength in grid points of wavenumber k_eff; inf for k_eff = 0."""
    k = np.asarray(k_eff, dtype=np.float64)
    with np.errstate(divide="ignore"):
        out = np.where(k == 0, np.inf, N / np.where(k == 0, 1.0, k))
    return float(out) if out.ndim == 0 else out


class CrossSpectrum:
    """Running mean of the cross spectra of paired C-channel N x N fields: fp64 sums [C, 3, K] and the pair count stay on the
    device (one buffer, so ``reduce_`` is one all-reduce under data parallelism)."""

    def __init__(self, C, N, device="cuda:0", ops=None):
        check_n(N)
        if not 1 <= C <= C_MAX:
            raise ValueError(f"cross spectra take 1 <= C <= {C_MAX} channels (got C = {C})")
        self.C, self.N, self.K = int(C), int(N), N // 2 + 1
        self.device = torch.device(device)
        self._ops = ops
        self._acc = torch.zeros(self.C * 3 * self.K + 1, dtype=torch.float64, device=self.device)

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def sums(self):
        return self._acc[:-1].view(self.C, 3, self.K)

    @property
    def count(self):
        """Number of pairs (per channel) added so far."""
        return int(round(float(self._acc[-1].item())))

    def add(self, a, b, n_valid=None, nhwc=False, nhwc_b=None, channels=None):
        """Add the cross spectra of the first ``n_valid`` (default: all) pairs of a batch (layouts as ``cross_rapsd``)."""
        sa, sb, Cn, T, N = _pair(a, b, channels, nhwc, nhwc_b)
        if (Cn, N) != (self.C, self.N):
            raise ValueError(f"CrossSpectrum({self.C}, {self.N}) given {Cn} channels of {N} x {N}")
        n = _n_valid(n_valid, T)
        _cross_sum_into(self.ops, (sa[0][:n], sa[1]), (sb[0][:n], sb[1]), Cn, n, N, self.sums)
        self._acc[-1] += n
        return self

    def mean(self):
        """float64 [C, 3, K]: the mean cross spectra of every pair added (and, after ``reduce_``, of every rank)."""
        if self.count == 0:
            raise ValueError("CrossSpectrum.mean: no field was added")
        return self.sums / self._acc[-1]

    def coherence(self):
        """numpy float64 [C, K]: the coherence of the mean cross spectra."""
        return coherence(self.mean())

    def reduce_(self, dist):
        """Sum the sums and counts over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place."""
        if dist is not None and dist.world_size > 1:
            dist.allreduce_sum_(self._acc)
        return self


class RadialSpectrum:
    """Running mean of the spectra of C-channel N x N fields: fp64 sums [C, K] and the field count stay on the device
    (one buffer, so ``reduce_`` is one all-reduce under data parallelism)."""

    def __init__(self, C, N, device="cuda:0", ops=None):
        check_n(N)
        if not 1 <= C <= C_MAX:
            raise ValueError(f"RAPSD takes 1 <= C <= {C_MAX} channels (got C = {C})")
        self.C, self.N, self.K = int(C), int(N), N // 2 + 1
        self.device = torch.device(device)
        self._ops = ops
        self._acc = torch.zeros(self.C * self.K + 1, dtype=torch.float64, device=self.device)

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def sums(self):
        return self._acc[:-1].view(self.C, self.K)

    @property
    def count(self):
        """Number of fields (per channel) added so far."""
        return int(round(float(self._acc[-1].item())))

    def add(self, fields, n_valid=None, nhwc=False, channels=None):
        """Add the spectra of the first ``n_valid`` (default: all) fields of a batch (layouts as ``rapsd``)."""
        x, nhwc, Cn, T, N = _fields(fields, channels, nhwc)[:5]
        if (Cn, N) != (self.C, self.N):
            raise ValueError(f"RadialSpectrum({self.C}, {self.N}) given {Cn} channels of {N} x {N}")
        n = _n_valid(n_valid, T)
        _sum_into(self.ops, x[:n], nhwc, Cn, n, N, self.sums)
        self._acc[-1] += n
        return self

    def mean(self):
        """float64 [C, K]: the mean spectrum of every field added (and, after ``reduce_``, of every rank)."""
        if self.count == 0:
            raise ValueError("RadialSpectrum.mean: no field was added")
        return self.sums / self._acc[-1]

    def reduce_(self, dist):
        """Sum the sums and counts over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place."""
        if dist is not None and dist.world_size > 1:
            dist.allreduce_sum_(self._acc)
        return self


# ---------------------------------------------------------------------------------------------------- Helmholtz spectra
HELM_PLANES = ("ke", "rot", "div")
HELM_CROSS_PLANES = ("ke_real", "rot_real", "div_real", "ke_fake", "rot_fake", "div_fake", "co_rot", "co_div")


def _helm_pair(pair, Cn=None):
    """ValueError unless ``pair`` is two distinct channel indices (below Cn when given) -> (cu, cv)."""
    try:
        cu, cv = pair
        ok = all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) for c in (cu, cv))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"Helmholtz spectra take pair = (channel of u, channel of v), two integers (got {pair!r})")
    top = C_MAX if Cn is None else Cn
    if cu == cv or not (0 <= cu < top and 0 <= cv < top):
        raise ValueError(f"Helmholtz spectra need a pair of two different channels in [0, {top}) (got pair = {tuple(pair)})")
    return int(cu), int(cv)


def _helm_scale(scale, rows_up):
    """ValueError unless ``scale`` is None or two finite non-zero numbers -> (su, sv), sv negated for rows that run downward."""
    if scale is None:
        su, sv = 1.0, 1.0
    else:
        try:
            su, sv = (float(v) for v in scale)
        except (TypeError, ValueError):
            raise ValueError(f"Helmholtz spectra take scale = (scale of u, scale of v) (got {scale!r})") from None
        if not (np.isfinite(su) and np.isfinite(sv) and su != 0.0 and sv != 0.0):
            raise ValueError(f"Helmholtz spectra need finite non-zero scales (got scale = {(su, sv)})")
    return su, sv if rows_up else -sv


def _helm_fields(x, channels, nhwc, pair):
    x, nhwc, Cn, T, N = _fields(x, channels, nhwc)[:5]
    if Cn < 2:
        raise ValueError(f"Helmholtz spectra need a vector field: C >= 2 channels (got C = {Cn})")
    return x, nhwc, Cn, T, N, _helm_pair(pair, Cn)


def _helm_chunk(o, T, N, paired):
    """Fields (pairs) per library call: the fewest calls whose workspace stays within WS_CAP bytes, the T spread evenly over
    them (as ``_cross_chunk``)."""
    nbytes = o.helmholtz_cross_ws_bytes if paired else o.helmholtz_ws_bytes
    tc = min(T, max(1, WS_CAP // max(1, nbytes(1, N))))
    while tc > 1 and nbytes(tc, N) > WS_CAP:
        tc -= 1
    calls = -(-T // tc)
    return -(-T // calls)


def _helm_run(o, a, b, Cn, T, N, cu, cv, sc, total=None, per_field=None):
    """One-sided (b None) or paired call over the T fields in chunks: ``total`` [NP, K] += the chunk sums in order, or
    ``per_field`` [T, NP, K] filled."""
    tc = _helm_chunk(o, T, N, b is not None)
    part = None if total is None else torch.empty_like(total)
    for t0 in range(0, T, tc):
        kw = {"sum": part} if per_field is None else {"per_field": per_field[t0:t0 + tc]}
        xa, fa = _descriptor(o, a[0][t0:t0 + tc], a[1], Cn)
        if b is None:
            o.helmholtz(fa, cu, cv, sc, N, **kw)
        else:
            xb, fb = _descriptor(o, b[0][t0:t0 + tc], b[1], Cn)
            o.helmholtz_cross(fa, fb, cu, cv, sc, N, **kw)
        if total is not None:
            total += part


def helmholtz_rapsd(x, pair=(0, 1), scale=None, rows_up=True, channels=None, nhwc=False, per_field=False, ops=None):
    """Helmholtz decomposition of the kinetic energy spectrum of a series of square vector fields on the GPU.

    x: as ``rapsd``'s, with C >= 2 channels; ``pair`` = (channel of u, channel of v).  u points along increasing column index
    (the last axis) and v along increasing row index; ``rows_up=False`` says that the rows run the other way (v points toward
    decreasing row index, e.g. a northward v on rows stored north to south) and negates v's scale.  A field whose first wind
    component points along the rows is the same call with the pair exchanged.  With U = su fft2(u), V = sv fft2(v), the signed
    integer wavenumbers kx (along W), ky (along H) and k2 = kx^2 + ky^2:

        ke = (|U|^2 + |V|^2) / (2 N^2),  div = |kx U + ky V|^2 / (2 k2 N^2),  rot = |kx V - ky U|^2 / (2 k2 N^2)

    (rot = div = 0 at k2 = 0), averaged over ``rapsd``'s rings: rot + div = ke on every ring k >= 1.
    ``scale`` = (su, sv), None = (1, 1).  UNLIKE every scalar spectrum here the decomposition is NOT invariant under per-channel
    scaling: on z-scored channels the split is only meaningful with ``scale = (std_u, std_v)``, the standard deviations the
    channels were divided by, so that both components are in the same physical unit again.
    Returns float64 [3, N/2 + 1] (planes ke, rot, div), the mean over T, or [T, 3, N/2 + 1] with ``per_field``."""
    sc = _helm_scale(scale, rows_up)
    x, nhwc, Cn, T, N, (cu, cv) = _helm_fields(x, channels, nhwc, pair)
    o = ops if ops is not None else _default_ops(x.device)
    K = N // 2 + 1
    if per_field:
        out = torch.empty(T, 3, K, dtype=torch.float64, device=x.device)
        _helm_run(o, (x, nhwc), None, Cn, T, N, cu, cv, sc, per_field=out)
        return out
    total = torch.zeros(3, K, dtype=torch.float64, device=x.device)
    _helm_run(o, (x, nhwc), None, Cn, T, N, cu, cv, sc, total=total)
    return total / T


def _helm_sides(a, b, pair, nhwc, nhwc_b, channels=None):
    sa, sb, Cn, T, N = _pair(a, b, channels, nhwc, nhwc_b)
    if Cn < 2:
        raise ValueError(f"Helmholtz spectra need a vector field: C >= 2 channels (got C = {Cn})")
    return sa, sb, Cn, T, N, _helm_pair(pair, Cn)


def helmholtz_cross(a, b, pair=(0, 1), scale=None, rows_up=True, nhwc=False, nhwc_b=None, per_field=False, ops=None,
                    channels=None):
    """Helmholtz spectra of the PAIRED vector fields a (real) and b (generated) and the co-spectra of their rotational and of
    their divergent parts (``pair``, ``scale``, ``rows_up`` as ``helmholtz_rapsd``, layouts and ``channels`` as ``cross_rapsd``:
    of a padded NHWC store only the leading ``channels`` count, and the pair lies among them).

    Returns float64 [8, N/2 + 1], the mean over T of the planes ke_a, rot_a, div_a, ke_b, rot_b, div_b, co_rot, co_div, or
    [T, 8, N/2 + 1] with ``per_field``; co_rot = Re(Ra conj Rb) / (2 k2 N^2) with R = kx V - ky U of each side, co_div likewise
    with D = kx U + ky V, so |co_x| <= sqrt(x_a x_b) on every ring and co_rot + co_div = (co_u + co_v) / 2 of ``cross_rapsd`` on
    the scaled channels.  Per library call planes 0-5 equal ``helmholtz_rapsd`` of a and of b bit for bit."""
    sc = _helm_scale(scale, rows_up)
    sa, sb, Cn, T, N, (cu, cv) = _helm_sides(a, b, pair, nhwc, nhwc_b, channels)
    dev = sa[0].device
    o = ops if ops is not None else _default_ops(dev)
    K = N // 2 + 1
    if per_field:
        out = torch.empty(T, 8, K, dtype=torch.float64, device=dev)
        _helm_run(o, sa, sb, Cn, T, N, cu, cv, sc, per_field=out)
        return out
    total = torch.zeros(8, K, dtype=torch.float64, device=dev)
    _helm_run(o, sa, sb, Cn, T, N, cu, cv, sc, total=total)
    return total / T


def _helm_planes(s):
    s = _host(s)
    if s.ndim < 2 or s.shape[-2] not in (3, 8):
        raise ValueError(f"Helmholtz spectra are [..., 3, K] or [..., 8, K] (got shape {s.shape})")
    return s


def divergent_fraction(s):
    """div / (rot + div) per wavenumber, NaN on ring 0 (and wherever both vanish): Helmholtz spectra [..., 3, K] -> numpy
    float64 [..., K]; paired spectra [..., 8, K] -> [..., 2, K], side a then side b."""
    s = _helm_planes(s)
    if s.shape[-2] == 8:
        return np.stack([divergent_fraction(s[..., 0:3, :]), divergent_fraction(s[..., 3:6, :])], axis=-2)
    rot, div = s[..., 1, :], s[..., 2, :]
    den = rot + div
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(den == 0, np.nan, div / den)
    out[..., 0] = np.nan
    return out


def helmholtz_coherence(s):
    """co_rot / sqrt(rot_a rot_b) and co_div / sqrt(div_a div_b) per wavenumber: paired Helmholtz spectra [..., 8, K] -> numpy
    float64 [..., 2, K] (rot, div); NaN where a denominator is 0 (ring 0).  ``effective_resolution`` takes each row."""
    s = _helm_planes(s)
    if s.shape[-2] != 8:
        raise ValueError(f"helmholtz_coherence takes paired spectra [..., 8, K] (got shape {s.shape})")
    rows = []
    for pa, pb, pc in ((1, 4, 6), (2, 5, 7)):
        den = np.sqrt(s[..., pa, :] * s[..., pb, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            rows.append(np.where(den == 0, np.nan, s[..., pc, :] / den))
    return np.stack(rows, axis=-2)


def spectral_slope(p, kmin, kmax):
    """Least-squares slope of log p against log k over the rings kmin <= k <= kmax (1 <= kmin < kmax <= K - 1): spectra
    [..., K] -> numpy float64 [...] ([K] -> a float); -3 for p ~ k^-3.  NaN where a ring of the band is not positive."""
    p = _host(p)
    if p.ndim < 1 or not (isinstance(kmin, (int, np.integer)) and isinstance(kmax, (int, np.integer))
                          and 1 <= kmin < kmax <= p.shape[-1] - 1):
        raise ValueError(f"spectral_slope: a band 1 <= kmin < kmax <= K - 1 of spectra [..., K] (got kmin = {kmin}, kmax = {kmax}, "
                         f"shape {p.shape})")
    x = np.log(np.arange(kmin, kmax + 1, dtype=np.float64))
    x = x - x.mean()
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.log(np.where(p[..., kmin:kmax + 1] > 0, p[..., kmin:kmax + 1], np.nan))
    out = (y * x).sum(axis=-1) / (x * x).sum()
    return float(out) if out.ndim == 0 else out


class HelmholtzSpectrum:
    """Running mean of the paired Helmholtz spectra of N x N vector fields (``helmholtz_cross``): fp64 sums [8, K] and the pair
    count stay on the device (one buffer, so ``reduce_`` is one all-reduce under data parallelism)."""

    def __init__(self, N, pair=(0, 1), scale=None, rows_up=True, device="cuda:0", ops=None):
        check_n(N)
        self.pair = _helm_pair(pair)
        self.scale = _helm_scale(scale, rows_up)
        self.N, self.K = int(N), N // 2 + 1
        self.device = torch.device(device)
        self._ops = ops
        self._acc = torch.zeros(8 * self.K + 1, dtype=torch.float64, device=self.device)

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def sums(self):
        return self._acc[:-1].view(8, self.K)

    @property
    def count(self):
        """Number of pairs added so far."""
        return int(round(float(self._acc[-1].item())))

    def add(self, a, b, n_valid=None, nhwc=False, nhwc_b=None, channels=None):
        """Add the spectra of the first ``n_valid`` (default: all) pairs of a batch (layouts as ``cross_rapsd``)."""
        sa, sb, Cn, T, N, (cu, cv) = _helm_sides(a, b, self.pair, nhwc, nhwc_b, channels)
        if N != self.N:
            raise ValueError(f"HelmholtzSpectrum({self.N}) given fields of {N} x {N}")
        n = _n_valid(n_valid, T)
        _helm_run(self.ops, (sa[0][:n], sa[1]), (sb[0][:n], sb[1]), Cn, n, N, cu, cv, self.scale, total=self.sums)
        self._acc[-1] += n
        return self

    def mean(self):
        """float64 [8, K]: the mean spectra of every pair added (and, after ``reduce_``, of every rank)."""
        if self.count == 0:
            raise ValueError("HelmholtzSpectrum.mean: no field was added")
        return self.sums / self._acc[-1]

    def reduce_(self, dist):
        """Sum the sums and counts over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place."""
        if dist is not None and dist.world_size > 1:
            dist.allreduce_sum_(self._acc)
        return self
