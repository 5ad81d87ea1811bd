"""Histograms and quantiles of real and generated fields, computed on the GPU (csrc/histogram.hip).

The distribution check of a downscaling generator: do the generated values follow the distribution of the real ones, in the
tails too (a GAN can match the mean error and the spectrum and still clip or invent strong winds)?  For output channel j of a
``HistSpec`` (``bins`` interior bins on [lo_j, hi_j), inv_w_j = fp32(bins / (hi_j - lo_j)) rounded once from float64):

    y_c = fp32(fp32(x_c * scale_c) + offset_c)                 physical units (default scale 1, offset 0: y = x)
    s   = sqrt_rn(fp32(fp32(y_u * y_u) + fp32(y_v * y_v)))      the speed of the pair ``speed`` = (u, v), appended last
    t   = fp32(fp32(y - lo_j) * inv_w_j)                        NaN -> NaN count; t < 0 -> underflow; t >= bins -> overflow;
                                                                otherwise interior bin int(t)

Every step is one correctly rounded fp32 operation, so numpy float32 arithmetic reproduces the counts exactly.  ``histogram``
reads NCHW tensors, the resident feed's ``[n, H, W, c]`` store and the generator's padded NHWC output in place (fp32 or bf16);
``ValueHistogram`` accumulates many batches on the device (and over data-parallel ranks); the trainer's opt-in hook
(``WassersteinGAN.log_distributions``) keeps one for the real and one for the generated fields.  Quantiles, the 1-D Wasserstein
distance, the Kolmogorov-Smirnov distance and tail exceedances are derived on the host in float64 from the counts, with the
bin-width error that binning implies.  Two calls on the same data are bit-identical (no float atomics, fixed-order sums).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from .fields import agree, default_ops, descriptor as _descriptor, n_valid as _n_valid, series

BINS_MAX = _lib.HIST_MAX_BINS
C_MAX = _lib.EOF_MAX_C

_ops = {}                    # device -> op backend of the module-level calls


def _default_ops(device):
    return default_ops(_ops, device)


def _f32(v, what):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"histogram {what} must be finite (got {a.tolist()})")
    with np.errstate(over="ignore"):
        b = a.astype(np.float32)
    if not np.all(np.isfinite(b)):
        raise ValueError(f"histogram {what} must be finite in fp32 (got {a.tolist()})")
    return b


class HistSpec:
    """Bins and units of the histograms of C input channels (+ the speed of a pair of them, appended as the last output).

    bins: interior bins per output channel (1 .. BINS_MAX); lo, hi: one value per output channel (nout = C + 1 with a speed
    channel, else C), rounded to fp32, lo < hi; scale, offset: per input channel (default 1, 0); speed: the input channels
    (u, v) of the speed channel, or None; names: one per output channel."""

    def __init__(self, bins, lo, hi, scale=None, offset=None, speed=(0, 1), names=None):
        if not (isinstance(bins, (int, np.integer)) and 1 <= bins <= BINS_MAX):
            raise ValueError(f"histogram bins must be an integer in [1, {BINS_MAX}] (got {bins!r})")
        self.bins = int(bins)
        self.lo, self.hi = _f32(lo, "lo"), _f32(hi, "hi")
        nout = len(self.lo)
        if len(self.hi) != nout or nout < 1:
            raise ValueError(f"histogram lo and hi need one value per output channel (got {len(self.lo)} and {len(self.hi)})")
        if not np.all(self.lo < self.hi):
            raise ValueError(f"histogram needs lo < hi in every channel (got lo = {self.lo.tolist()}, hi = {self.hi.tolist()})")
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        self.C = nout - (self.speed is not None)
        self.nout = nout
        if not 1 <= self.C <= C_MAX:
            raise ValueError(f"histogram takes 1 <= C <= {C_MAX} input channels (got C = {self.C} from {nout} output channels)")
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"histogram speed channels {speed} out of range for C = {self.C} input channels")
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"histogram scale and offset need one value per input channel (C = {self.C})")
        inv_w = self.bins / (self.hi.astype(np.float64) - self.lo.astype(np.float64))
        with np.errstate(over="ignore", under="ignore"):
            self.inv_w = inv_w.astype(np.float32)
        if not np.all(np.isfinite(self.inv_w) & (self.inv_w > 0)):
            raise ValueError(f"histogram bin width out of fp32 range: bins / (hi - lo) = {inv_w.tolist()}")
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != nout:
            raise ValueError(f"histogram names need one entry per output channel ({nout})")

    @classmethod
    def zscore(cls, C, bins=2048, lim=10.0):
        """Standardised fields: components on [-lim, lim], the speed of channels (0, 1) (when C >= 2) on [0, lim * sqrt 2]."""
        speed = (0, 1) if C >= 2 else None
        lo = [-lim] * C + ([0.0] if speed else [])
        hi = [lim] * C + ([lim * math.sqrt(2.0)] if speed else [])
        return cls(bins, lo, hi, speed=speed)

    @classmethod
    def physical(cls, stats, order, lo, hi, bins=2048, speed=("u10", "v10")):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, binned in
        physical units (y = x * std + mean).  lo, hi: one value per output channel, or scalars for the components (the speed
        then spans [0, max(|lo|, |hi|) * sqrt 2]).  speed: the names of the (u, v) pair, or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        if np.ndim(lo) == 0 and np.ndim(hi) == 0:
            top = max(abs(float(lo)), abs(float(hi))) * math.sqrt(2.0)
            lo = [float(lo)] * len(order) + ([0.0] if sp else [])
            hi = [float(hi)] * len(order) + ([top] if sp else [])
        names = order + (["speed"] if sp else [])
        return cls(bins, lo, hi, scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp, names=names)

    def width(self):
        """float64 [nout]: the nominal bin width (hi - lo) / bins."""
        return (self.hi.astype(np.float64) - self.lo.astype(np.float64)) / self.bins

    def edges(self):
        """float64 [nout, bins + 1]: lo + k * width."""
        return self.lo.astype(np.float64)[:, None] + np.arange(self.bins + 1)[None, :] * self.width()[:, None]

    def struct(self):
        """The dg_hist_spec of this spec (no library call)."""
        s = _lib.HistSpec()
        s.nbins = self.bins
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        for j in range(self.nout):
            s.lo[j], s.inv_w[j] = float(self.lo[j]), float(self.inv_w[j])
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        return s

    def __eq__(self, other):
        return (isinstance(other, HistSpec) and self.bins == other.bins and self.speed == other.speed
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("lo", "hi", "scale", "offset")))

    __hash__ = None


def host_bins(spec, x):
    """int32 [nout, n]: the bin of each value of x (fp32 [C, n], planar) under ``spec``, computed by the library on the host
    (dg_hist_host_bins: 0 underflow, 1 .. bins interior, bins + 1 overflow, bins + 2 NaN)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[0] != spec.C:
        raise ValueError(f"host_bins takes [C = {spec.C}, n] values (got shape {x.shape})")
    out = np.empty((spec.nout, x.shape[1]), dtype=np.int32)
    s = spec.struct()
    _lib.check(_lib.lib().dg_hist_host_bins(ctypes.byref(s), x.ctypes.data, spec.C, x.shape[1], out.ctypes.data),
               "dg_hist_host_bins")
    return out


def _fields(x, channels, nhwc):
    """Validate without touching a device -> (tensor, nhwc, C, T).  Kept under this name, as ``_descriptor`` and ``_default_ops``
    are, for the GPU tests and tools that call the kernels directly."""
    return series(x, channels, nhwc, "histogram")[:4]


def _check_spec(spec, s):
    if not isinstance(spec, HistSpec):
        raise TypeError(f"histogram takes a HistSpec (got {type(spec).__name__})")
    agree(s, spec, "given")


class Histogram:
    """Histograms of nout channels under one HistSpec: device counts int64 [nout, bins + 3] (underflow, bins, overflow, NaN),
    moments fp64 [nout, 2] (sum, sum of squares of the finite values), extrema fp32 [nout, 2] (min, max of the finite values),
    and the number of fields.  The statistics are computed on the host in float64."""

    def __init__(self, spec, counts, moments, extrema, fields):
        self.spec, self.counts, self.moments, self.extrema, self.fields = spec, counts, moments, extrema, int(fields)
        self._h = None

    def host(self):
        """(counts int64, moments float64, extrema float32) as numpy arrays (copied once)."""
        if self._h is None:
            self._h = tuple(t.detach().cpu().numpy().copy() for t in (self.counts, self.moments, self.extrema))
        return self._h

    def edges(self):
        return self.spec.edges()

    def finite(self):
        """int64 [nout]: the number of finite values."""
        return self.host()[0][:, :-1].sum(axis=1)

    def nan(self):
        return self.host()[0][:, -1].copy()

    def out_of_range(self):
        """int64 [nout, 2]: the finite values below lo and at or above hi (the underflow and overflow bins)."""
        c = self.host()[0]
        return np.stack([c[:, 0], c[:, -2]], axis=1)

    def min(self):
        return self.host()[2][:, 0].astype(np.float64)

    def max(self):
        return self.host()[2][:, 1].astype(np.float64)

    def mean(self):
        n = self.finite().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.host()[1][:, 0] / n

    def std(self):
        """Population standard deviation of the finite values."""
        n = self.finite().astype(np.float64)
        m = self.host()[1]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = m[:, 0] / n
            return np.sqrt(np.maximum(m[:, 1] / n - mean * mean, 0.0))

    def _spans(self, j):
        """left, right [bins + 2] of the finite bins of channel j: [min, lo], interior [lo + (b-1) w, lo + b w], [hi, max]."""
        e = self.edges()[j]
        lo, hi = float(self.spec.lo[j]), float(self.spec.hi[j])
        mn, mx = self.min()[j], self.max()[j]
        left = np.concatenate([[min(mn, lo)], e[:-1], [hi]])
        right = np.concatenate([[lo], e[1:], [max(mx, hi)]])
        return left, right

    def quantile(self, q):
        """float64 [nout, len(q)] ([nout] for a scalar q): the first bin (underflow, interior, overflow) whose cumulative count
        reaches q * n, interpolated linearly inside it; q = 0 gives min and q = 1 max.  Error: one bin width inside [lo, hi)."""
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
        if np.any((qs < 0) | (qs > 1)) or np.any(np.isnan(qs)):
            raise ValueError(f"quantile levels must lie in [0, 1] (got {qs.tolist()})")
        c = self.host()[0]
        out = np.full((self.spec.nout, len(qs)), np.nan)
        for j in range(self.spec.nout):
            cnt = c[j, :-1].astype(np.float64)
            n = cnt.sum()
            if n == 0:
                continue
            cum = np.cumsum(cnt)
            left, right = self._spans(j)
            for k, qk in enumerate(qs):
                if qk == 0:
                    out[j, k] = self.min()[j]
                elif qk == 1:
                    out[j, k] = self.max()[j]
                else:
                    m = qk * n
                    i = int(np.searchsorted(cum, m, side="left"))
                    prev = cum[i - 1] if i > 0 else 0.0
                    out[j, k] = left[i] + (m - prev) / cnt[i] * (right[i] - left[i])
        return out[:, 0] if np.ndim(q) == 0 else out

    def cdf(self, x):
        """float64 [nout]: the fraction of finite values <= x[j] (x: one value per channel, or a scalar), with the same
        linear interpolation inside a bin as ``quantile``."""
        xs = np.broadcast_to(np.asarray(x, dtype=np.float64), (self.spec.nout,))
        c = self.host()[0]
        out = np.full(self.spec.nout, np.nan)
        for j in range(self.spec.nout):
            cnt = c[j, :-1].astype(np.float64)
            n = cnt.sum()
            if n == 0:
                continue
            left, right = self._spans(j)
            span = right - left
            with np.errstate(invalid="ignore", divide="ignore"):
                frac = np.where(span > 0, np.clip((xs[j] - left) / np.where(span > 0, span, 1.0), 0.0, 1.0),
                                (xs[j] >= right).astype(np.float64))
            out[j] = float((cnt * frac).sum() / n)
        return out


def histogram(x, spec, channels=None, nhwc=False, ops=None):
    """Histograms of a series of fields on the GPU under ``spec``.

    x: device tensor [T, C, H, W] (fp32 / bf16), or with ``nhwc`` a dense-pixel [T, H, W, c_pad] store of which the leading
    ``channels`` are read (the generator's padded output; default: all), or a ``dataloader.NativeBatch``.  Returns a
    ``Histogram`` over every value of the T fields."""
    s = series(x, channels, nhwc, "histogram")
    _check_spec(spec, s)
    return ValueHistogram(spec, s.x.device, ops=ops).add(s.x, nhwc=s.nhwc, channels=s.C).result()


def _pair(a, b):
    if not (isinstance(a, Histogram) and isinstance(b, Histogram)):
        raise TypeError("expected two Histogram objects")
    if a.spec != b.spec:
        raise ValueError("the two histograms must share one HistSpec")
    return a.host()[0][:, :-1].astype(np.float64), b.host()[0][:, :-1].astype(np.float64)


def _cdfs(a, b):
    ca, cb = _pair(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.cumsum(ca, axis=1) / ca.sum(axis=1, keepdims=True), np.cumsum(cb, axis=1) / cb.sum(axis=1, keepdims=True)


def wasserstein1(a, b):
    """float64 [nout]: the 1-D Wasserstein distance of the two binned distributions, the underflow mass at lo, interior bin
    b at lo + (b - 1/2) w, the overflow mass at hi: sum_i |F_a(i) - F_b(i)| (x_{i+1} - x_i)."""
    Fa, Fb = _cdfs(a, b)
    w = a.spec.width()
    gaps = np.concatenate([np.full((a.spec.nout, 1), 0.5), np.ones((a.spec.nout, a.spec.bins - 1)),
                           np.full((a.spec.nout, 1), 0.5)], axis=1) * w[:, None]
    return (np.abs(Fa[:, :-1] - Fb[:, :-1]) * gaps).sum(axis=1)


def ks_distance(a, b):
    """float64 [nout]: max_i |F_a(i) - F_b(i)| on the binned support."""
    Fa, Fb = _cdfs(a, b)
    return np.abs(Fa - Fb).max(axis=1)


def exceedance(real, fake, qs=(0.99, 0.999, 0.9999)):
    """float64 [nout, len(qs)]: the fraction of the generated values above the real q-quantile tau_q (read from the fake
    histogram with the within-bin interpolation of ``quantile``); close to 1 - q when the tails match."""
    _pair(real, fake)
    tau = real.quantile(np.asarray(qs, dtype=np.float64))
    return np.stack([1.0 - fake.cdf(tau[:, k]) for k in range(tau.shape[1])], axis=1)


class ValueHistogram:
    """Running histograms of the fields added so far: counts (+ the field count), moments and extrema stay on the device
    (``reduce_`` is one int64 and one fp64 all-reduce plus the min / max of the extrema under data parallelism)."""

    def __init__(self, spec, device="cuda:0", ops=None):
        if not isinstance(spec, HistSpec):
            raise TypeError(f"ValueHistogram takes a HistSpec (got {type(spec).__name__})")
        self.spec = spec
        self.device = torch.device(device)
        self._ops = ops
        nb = spec.nout * (spec.bins + 3)
        self._cnt = torch.zeros(nb + 1, dtype=torch.int64, device=self.device)       # the last entry: fields added
        self._mom = torch.zeros(spec.nout, 2, dtype=torch.float64, device=self.device)
        self._ext = torch.tensor([[math.inf, -math.inf]] * spec.nout, dtype=torch.float32).to(self.device)
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def counts(self):
        return self._cnt[:-1].view(self.spec.nout, self.spec.bins + 3)

    @property
    def fields(self):
        return int(self._cnt[-1].item())

    def add(self, fields, n_valid=None, nhwc=False, channels=None):
        """Add every value of the first ``n_valid`` (default: all) fields of a batch (layouts as ``histogram``)."""
        s = series(fields, channels, nhwc, "histogram")
        _check_spec(self.spec, s)
        n = _n_valid(n_valid, s.T)
        if self._struct is None:
            self._struct = self.spec.struct()
        xs, f = _descriptor(self.ops, s.x[:n], s.nhwc, s.C)
        self.ops.hist(f, self._struct, self.counts, self._mom, self._ext)
        self._cnt[-1] += n
        return self

    def reduce_(self, dist):
        """Sum the counts and moments and take the extrema over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist),
        once, in place."""
        if dist is not None and dist.world_size > 1:
            dist.allreduce_sum_(self._cnt)
            dist.allreduce_sum_(self._mom.view(-1))
            dist.minmax_(self._ext.view(1, -1), self.spec.nout)
        return self

    def result(self):
        """The ``Histogram`` of every value added (and, after ``reduce_``, of every rank)."""
        return Histogram(self.spec, self.counts.clone(), self._mom.clone(), self._ext.clone(), self.fields)
