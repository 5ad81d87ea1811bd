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
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, backend

N_MIN, N_MAX = 16, _lib.RAPSD_MAX_N
C_MAX = _lib.EOF_MAX_C
WS_CAP = 512 << 20           # bytes of dg_rapsd workspace at most: longer series are split into chunks of fields

_ops = {}                    # device -> op backend of the module-level calls


def _default_ops(device):
    key = str(device)
    if key not in _ops:
        _ops[key] = backend.make_ops("f32", device)
    return _ops[key]


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
    """Validate without touching a device -> (tensor, nhwc, C, T, N)."""
    if hasattr(x, "nhwc") and hasattr(x, "channels"):          # dataloader.NativeBatch
        x, nhwc, channels = x.nhwc, True, x.channels if channels is None else channels
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"RAPSD takes a tensor or a NativeBatch (got {type(x).__name__})")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"RAPSD reads fp32 or bf16 fields (got {x.dtype})")
    if x.dim() != 4:
        raise ValueError(f"RAPSD takes [T, C, N, N] (or [T, N, N, c] with nhwc=True) fields (got shape {tuple(x.shape)})")
    if nhwc:
        T, H, W, cp = x.shape
        Cn = cp if channels is None else int(channels)
        if not 1 <= Cn <= cp:
            raise ValueError(f"channels = {Cn} but the NHWC store holds {cp}")
    else:
        T, cx, H, W = x.shape
        Cn = cx if channels is None else int(channels)
        if not 1 <= Cn <= cx:
            raise ValueError(f"channels = {Cn} but the tensor holds {cx}")
    if H != W:
        raise ValueError(f"RAPSD needs square fields (got {H} x {W})")
    check_n(int(H))
    if not 1 <= Cn <= C_MAX:
        raise ValueError(f"RAPSD takes 1 <= C <= {C_MAX} channels (got C = {Cn})")
    if T < 1:
        raise ValueError("RAPSD needs at least one field")
    return x, nhwc, Cn, int(T), int(H)


def _descriptor(o, x, nhwc, Cn):
    if nhwc:
        if not (x.stride(3) == 1 and x.stride(2) == x.shape[3] and x.stride(1) == x.shape[2] * x.shape[3]):
            x = x.contiguous()
        return x, o.eof_fields(x, nhwc=True, channels=Cn)
    x = x[:, :Cn]
    if not (x.stride(3) == 1 and x.stride(2) == x.shape[3] and x.stride(1) == x.shape[2] * x.shape[3]):
        x = x.contiguous()
    return x, o.eof_fields(x)


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
    x, nhwc, Cn, T, N = _fields(x, channels, nhwc)
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
    a, na, Ca, Ta, Na = _fields(a, channels, nhwc)
    b, nb, Cb, Tb, Nb = _fields(b, channels, nhwc if nhwc_b is None else nhwc_b)
    if (Ta, Ca, Na) != (Tb, Cb, Nb):
        raise ValueError(f"cross spectra need paired fields: a has T, C, N = {Ta}, {Ca}, {Na} and b has {Tb}, {Cb}, {Nb}")
    if a.device != b.device:
        raise ValueError(f"cross spectra need both sides on one device (got {a.device} and {b.device})")
    return (a, na), (b, nb), Ca, Ta, Na


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
        n = T if n_valid is None else int(n_valid)
        if not 1 <= n <= T:
            raise ValueError(f"n_valid = {n} of a batch of {T}")
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
        x, nhwc, Cn, T, N = _fields(fields, channels, nhwc)
        if (Cn, N) != (self.C, self.N):
            raise ValueError(f"RadialSpectrum({self.C}, {self.N}) given {Cn} channels of {N} x {N}")
        n = T if n_valid is None else int(n_valid)
        if not 1 <= n <= T:
            raise ValueError(f"n_valid = {n} of a batch of {T}")
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
