"""Increment histograms of real and generated fields on the GPU (csrc/increments.hip): structure functions and intermittency.

A generated field can have the right spectrum (``spectra``) and the right value distribution (``histograms``) and still be too
smooth in its fronts and gust lines: the distribution of the velocity differences over a short distance then has Gaussian tails
where the real one is heavy-tailed.  The tools for this are the distributions of the spatial increments per separation r,

    direction 0 (along w):  d = fp32(y[t, h, w + r] - y[t, h, w])      0 <= w < W - r
    direction 1 (along h):  d = fp32(y[t, h + r, w] - y[t, h, w])      0 <= h < H - r

of the output values y of ``histograms`` (y_c = fp32(fp32(x_c * scale_c) + offset_c), the speed of the pair ``speed`` appended
last), one correctly rounded fp32 subtraction each, without wrap-around; a lag >= the extent contributes nothing.  Per series
(real, generated), output channel, direction and lag the kernel keeps the histogram of d under the 1-D bin rule of ``histograms``
(``nbins`` interior bins on [-range, range), inv_w = fp32(nbins / (2 range)) rounded once from float64; index 0 underflow,
1 .. nbins interior, nbins + 1 overflow, nbins + 2 NaN), the number of finite d and, over the finite d in float64, the sums of
u, |u|, u^2, u^3, |u|^3, u^4.  The counts are exact and all three outputs are bit-identical between two calls (integer LDS and
global atomics, fixed-order fp64 sums).  From them follow on the host the structure functions S_p(r) = <|d|^p>, the flatness
S_4 / S_2^2 (3 for a Gaussian, growing towards small r in real wind), the skewness <d^3> / S_2^(3/2), the scaling exponents, the
longitudinal and transverse structure functions of the (u, v) pair, and per lag the W1 and KS distances between the real and the
generated increment distributions.  S_2 is the only one of these the spectrum already determines.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib, fields
from .fss import allreduce_ints
from .histograms import C_MAX, Histogram, HistSpec, _f32, ks_distance, wasserstein1

LAGS_MAX = _lib.INCR_MAX_LAGS
LAG_MAX = _lib.INCR_MAX_LAG
BINS_MAX = _lib.INCR_MAX_BINS
SIDE_MAX = _lib.INCR_MAX_SIDE
DEFAULT_LAGS = (1, 2, 4, 8, 16, 32, 64, 128)
SERIES = ("real", "fake")

_ops = {}                    # device -> op backend of the module-level calls


def _default_ops(device):
    return fields.default_ops(_ops, device)


def _int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


class IncrementSpec:
    """Lags, bins and units of the increment histograms of C input channels (+ the speed of a pair of them, appended last).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None; lags: 1 ..
    LAGS_MAX strictly increasing separations in pixels, each in [1, LAG_MAX]; nbins: interior bins of every table (1 .. BINS_MAX);
    ranges: the half-width of the binned interval [-range, range) per (output channel, lag) -- a scalar, one value per lag, or an
    [nout, nlag] array; names: one per output channel."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), lags=DEFAULT_LAGS, nbins=128, ranges=8.0, names=None):
        if not (_int(C) and 1 <= C <= C_MAX):
            raise ValueError(f"increment histograms take 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"increment speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"increment scale and offset need one value per input channel (C = {self.C})")
        lags = list(lags)
        if not 1 <= len(lags) <= LAGS_MAX:
            raise ValueError(f"an IncrementSpec holds 1 .. {LAGS_MAX} lags (got {len(lags)})")
        if not all(_int(r) and 1 <= r <= LAG_MAX for r in lags):
            raise ValueError(f"increment lags must be integers in [1, {LAG_MAX}] (got {lags})")
        if any(b <= a for a, b in zip(lags, lags[1:])):
            raise ValueError(f"increment lags must be strictly increasing (got {lags})")
        self.lags = tuple(int(r) for r in lags)
        if not (_int(nbins) and 1 <= nbins <= BINS_MAX):
            raise ValueError(f"increment nbins must be an integer in [1, {BINS_MAX}] (got {nbins!r})")
        self.nbins = int(nbins)
        r = np.asarray(ranges, dtype=np.float64)
        if r.ndim > 2 or (r.ndim == 1 and r.shape != (self.nlag,)) or (r.ndim == 2 and r.shape != (self.nout, self.nlag)):
            raise ValueError(f"increment ranges are a scalar, one value per lag ({self.nlag}) or an [nout = {self.nout}, nlag = "
                             f"{self.nlag}] array (got shape {r.shape})")
        r = np.broadcast_to(r, (self.nout, self.nlag))
        self.ranges = _f32(r, "ranges").reshape(self.nout, self.nlag)
        if not np.all(self.ranges > 0):
            raise ValueError(f"increment ranges must be > 0 (got {self.ranges.tolist()})")
        self.lo = -self.ranges
        inv_w = self.nbins / (2.0 * self.ranges.astype(np.float64))
        with np.errstate(over="ignore", under="ignore"):
            self.inv_w = inv_w.astype(np.float32)
        if not np.all(np.isfinite(self.inv_w) & (self.inv_w > 0)):
            raise ValueError(f"increment bin width out of fp32 range: nbins / (2 range) = {inv_w.tolist()}")
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"increment names need one entry per output channel ({self.nout})")

    @property
    def nlag(self):
        return len(self.lags)

    @staticmethod
    def lag_ranges(lim, lags):
        """The default half-widths: ``lim`` from lag 64 on, shrinking as (r / 64)^(1/3) below it (the Kolmogorov scaling of an
        increment's spread), so that the bins follow the narrowing of the distribution towards small separations."""
        return [float(lim) * min(1.0, (r / 64.0) ** (1.0 / 3.0)) for r in lags]

    @classmethod
    def zscore(cls, C, lags=DEFAULT_LAGS, nbins=128, lim=8.0):
        """Standardised fields: the speed of channels (0, 1) when C >= 2, half-widths ``lag_ranges(lim, lags)``."""
        return cls(C, speed=(0, 1) if C >= 2 else None, lags=lags, nbins=nbins, ranges=cls.lag_ranges(lim, lags))

    @classmethod
    def physical(cls, stats, order, lim, lags=DEFAULT_LAGS, nbins=128, speed=("u10", "v10")):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, the
        increments binned in physical units (y = x * std + mean) with half-widths ``lag_ranges(lim, lags)``.  speed: the names
        of the (u, v) pair, or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        return cls(len(order), scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp, lags=lags,
                   nbins=nbins, ranges=cls.lag_ranges(lim, lags), names=order + (["speed"] if sp else []))

    def width(self):
        """float64 [nout, nlag]: the nominal bin width 2 range / nbins."""
        return 2.0 * self.ranges.astype(np.float64) / self.nbins

    def centres(self, j, l):
        """float64 [nbins]: the centres of the interior bins of output channel j at lag index l."""
        return float(self.lo[j, l]) + (np.arange(self.nbins) + 0.5) * self.width()[j, l]

    def struct(self):
        """The dg_incr_spec of this spec (no library call)."""
        s = _lib.IncrSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nlag, s.nbins = self.nlag, self.nbins
        for l, r in enumerate(self.lags):
            s.lag[l] = r
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            for l in range(self.nlag):
                s.lo[j][l], s.inv_w[j][l] = float(self.lo[j, l]), float(self.inv_w[j, l])
        return s

    def __eq__(self, other):
        return (isinstance(other, IncrementSpec) and self.C == other.C and self.speed == other.speed and self.lags == other.lags
                and self.nbins == other.nbins
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("ranges", "scale", "offset")))

    __hash__ = None


def host_increments(spec, x):
    """(counts int64 [nout, 2, nlag, nbins + 3], finite int64 [nout, 2, nlag], moments float64 [nout, 2, nlag, 6]) of one series
    of fields x (fp32 [T, C, H, W]) computed by the library on the host (dg_incr_host: the code the kernel runs)."""
    if not isinstance(spec, IncrementSpec):
        raise TypeError(f"host_increments takes an IncrementSpec (got {type(spec).__name__})")
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 4 or x.shape[1] != spec.C:
        raise ValueError(f"host_increments takes [T, C = {spec.C}, H, W] fields (got shape {x.shape})")
    T, _, H, W = x.shape
    counts = np.zeros((spec.nout, 2, spec.nlag, spec.nbins + 3), dtype=np.int64)
    finite = np.zeros((spec.nout, 2, spec.nlag), dtype=np.int64)
    moments = np.zeros((spec.nout, 2, spec.nlag, 6), dtype=np.float64)
    s = spec.struct()
    for t in range(T):
        _lib.check(_lib.lib().dg_incr_host(ctypes.byref(s), x[t].ctypes.data, spec.C, H, W, counts.ctypes.data, finite.ctypes.data,
                                           moments.ctypes.data), "dg_incr_host")
    return counts, finite, moments


def _jsonable(a):
    """Nested lists of an array, None where the value is not finite."""
    if isinstance(a, np.ndarray):
        return [_jsonable(v) for v in a]
    v = float(a)
    return v if math.isfinite(v) else None


def _ratio(num, den):
    """num / den, NaN where den is not > 0 or either is NaN."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


class IncrementResult:
    """The tables of an IncrementSpec over nser series (1: real only; 2: real, generated) of H x W fields, as numpy arrays:
    counts int64 [nser, nout, 2, nlag, nbins + 3], finite int64 [nser, nout, 2, nlag], moments float64 [nser, nout, 2, nlag, 6]
    (sums of u, |u|, u^2, u^3, |u|^3, u^4 over the finite increments).  Every statistic is derived on the host in float64 and
    is NaN where it is undefined (no finite increment: a lag >= the extent; a zero S_2: a constant field); ``summary`` reports
    those as None."""

    def __init__(self, spec, counts, finite, moments, fields, H, W):
        self.spec, self.fields, self.H, self.W = spec, int(fields), int(H), int(W)
        self.counts = np.asarray(counts, dtype=np.int64)
        self.finite = np.asarray(finite, dtype=np.int64)
        self.moments = np.asarray(moments, dtype=np.float64)
        self.nser = self.counts.shape[0]
        shape = (self.nser, spec.nout, 2, spec.nlag)
        if self.counts.shape != shape + (spec.nbins + 3,) or self.finite.shape != shape or self.moments.shape != shape + (6,):
            raise ValueError(f"increment tables of shape {self.counts.shape}, {self.finite.shape}, {self.moments.shape} do not fit "
                             f"the spec ({shape})")

    # ---- addressing
    def _series(self, s):
        i = SERIES.index(s) if s in SERIES else s
        if not (_int(i) and 0 <= i < self.nser):
            raise IndexError(f"series {s!r} of {self.nser} ({SERIES[:self.nser]})")
        return int(i)

    def _channel(self, c):
        if isinstance(c, str):
            if c not in self.spec.names:
                raise KeyError(f"no channel named {c!r} (channels: {self.spec.names})")
            return self.spec.names.index(c)
        if not 0 <= int(c) < self.spec.nout:
            raise IndexError(f"channel {c} of {self.spec.nout}")
        return int(c)

    def _lag(self, r):
        if r not in self.spec.lags:
            raise KeyError(f"lag {r!r} is not one of {self.spec.lags}")
        return self.spec.lags.index(r)

    @staticmethod
    def _direction(d):
        if d not in (0, 1):
            raise IndexError(f"direction is 0 (along w) or 1 (along h) (got {d!r})")
        return int(d)

    def pdf(self, series, channel, direction, lag):
        """(centres, density), float64 [nbins] each: the density of the increments of ``channel`` at separation ``lag`` (a value
        of spec.lags) in ``direction`` over the interior bins, normalised by the number of non-NaN increments and the bin width
        (NaN without any).  At lag 1 this is the gradient distribution."""
        s, j, d, l = self._series(series), self._channel(channel), self._direction(direction), self._lag(lag)
        c = self.counts[s, j, d, l]
        n = float(c[:-1].sum())
        return self.spec.centres(j, l), _ratio(c[1:-2].astype(np.float64), n * self.spec.width()[j, l])

    # ---- structure functions
    def structure(self, p):
        """float64 [nser, nout, 2, nlag]: S_p = sum |u|^p / finite, p = 1 .. 4."""
        if p not in (1, 2, 3, 4):
            raise ValueError(f"structure functions are kept for p = 1 .. 4 (got {p!r})")
        return _ratio(self.moments[..., {1: 1, 2: 2, 3: 4, 4: 5}[p]], self.finite)

    def skewness(self):
        """float64 [nser, nout, 2, nlag]: <u^3> / S_2^(3/2)."""
        return _ratio(_ratio(self.moments[..., 3], self.finite), self.structure(2) ** 1.5)

    def flatness(self):
        """float64 [nser, nout, 2, nlag]: S_4 / S_2^2 (3 for a Gaussian)."""
        return _ratio(self.structure(4), self.structure(2) ** 2)

    def flatness_ratio(self):
        """float64 [nout, 2, nlag]: the flatness of the generated over that of the real increments (< 1: too smooth)."""
        self._two()
        f = self.flatness()
        return _ratio(f[1], f[0])

    def _pooled(self, p, pairs):
        if self.spec.speed is None:
            raise ValueError("longitudinal and transverse structure functions need the (u, v) pair of spec.speed")
        if p not in (1, 2, 3, 4):
            raise ValueError(f"structure functions are kept for p = 1 .. 4 (got {p!r})")
        k = {1: 1, 2: 2, 3: 4, 4: 5}[p]
        num = sum(self.moments[:, j, d, :, k] for j, d in pairs)
        den = sum(self.finite[:, j, d, :] for j, d in pairs)
        return _ratio(num, den)

    def longitudinal(self, p):
        """float64 [nser, nlag]: S_p of the increments along the separation -- u along w pooled with v along h (the sums and the
        counts are pooled, not the ratios)."""
        u, v = self.spec.speed if self.spec.speed is not None else (0, 0)
        return self._pooled(p, ((u, 0), (v, 1)))

    def transverse(self, p):
        """float64 [nser, nlag]: S_p of the increments across the separation -- u along h pooled with v along w."""
        u, v = self.spec.speed if self.spec.speed is not None else (0, 0)
        return self._pooled(p, ((u, 1), (v, 0)))

    def exponents(self, p, lags=None):
        """float64 [nser, nout, 2]: the least-squares slope of log S_p on log r over ``lags`` (default: all of the spec), using
        the lags at which S_p is finite and > 0; NaN with fewer than two of them."""
        ls = self.spec.lags if lags is None else tuple(lags)
        idx = [self._lag(r) for r in ls]
        S = self.structure(p)[..., idx]
        x = np.log(np.asarray(ls, dtype=np.float64))
        out = np.full(S.shape[:-1], np.nan)
        for i in np.ndindex(*out.shape):
            ok = np.isfinite(S[i]) & (S[i] > 0)
            if ok.sum() >= 2:
                xs, ys = x[ok], np.log(S[i][ok])
                xm = xs - xs.mean()
                out[i] = float((xm * (ys - ys.mean())).sum() / (xm * xm).sum())
        return out

    # ---- real against generated
    def _two(self):
        if self.nser != 2:
            raise ValueError("this statistic compares the real and the generated series, but only one series was added")

    def _distance(self, fn):
        self._two()
        sp = self.spec
        out = np.full((sp.nout, 2, sp.nlag), np.nan)
        z2, ze = torch.zeros(1, 2, dtype=torch.float64), torch.zeros(1, 2)
        for j, d, l in np.ndindex(*out.shape):
            hs = HistSpec(sp.nbins, [float(sp.lo[j, l])], [float(sp.ranges[j, l])], speed=None)
            a, b = (Histogram(hs, torch.from_numpy(self.counts[s, j, d, l][None].copy()), z2, ze, self.fields) for s in (0, 1))
            out[j, d, l] = fn(a, b)[0]
        return out

    def w1(self):
        """float64 [nout, 2, nlag]: the 1-D Wasserstein distance of the real and the generated binned increment distributions
        (``histograms.wasserstein1``); NaN where either has no non-NaN increment."""
        return self._distance(wasserstein1)

    def ks(self):
        """float64 [nout, 2, nlag]: their Kolmogorov-Smirnov distance (``histograms.ks_distance``)."""
        return self._distance(ks_distance)

    def summary(self):
        """A JSON-serialisable dict (None where undefined)."""
        sp = self.spec
        out = {"channels": list(sp.names), "lags": list(sp.lags), "fields": self.fields, "grid": [self.H, self.W],
               "nbins": sp.nbins, "series": list(SERIES[:self.nser])}
        S = {p: self.structure(p) for p in (1, 2, 3, 4)}
        sk, fl, z2 = self.skewness(), self.flatness(), self.exponents(2)
        for s in range(self.nser):
            d = {"finite": self.finite[s].tolist(), "nan": self.counts[s, ..., -1].tolist(),
                 "out_of_range": (self.counts[s, ..., 0] + self.counts[s, ..., -2]).tolist(),
                 "structure": {str(p): _jsonable(S[p][s]) for p in S}, "skewness": _jsonable(sk[s]), "flatness": _jsonable(fl[s]),
                 "exponent_2": _jsonable(z2[s])}
            if sp.speed is not None:
                for name, fn in (("longitudinal", self.longitudinal), ("transverse", self.transverse)):
                    s2, s4 = fn(2)[s], fn(4)[s]
                    d[name] = {"S2": _jsonable(s2), "flatness": _jsonable(_ratio(s4, s2 ** 2))}
            out[SERIES[s]] = d
        if self.nser == 2:
            out["w1"], out["ks"] = _jsonable(self.w1()), _jsonable(self.ks())
            out["flatness_ratio"] = _jsonable(self.flatness_ratio())
        return out


class Increments:
    """Running increment histograms of the fields added so far: counts, finite and moments stay on the device (two series'
    worth; a run without generated fields uses the first half).  Every ``add`` of one accumulator takes the same grid and either
    always or never a generated series."""

    def __init__(self, spec, device="cuda:0", ops=None):
        if not isinstance(spec, IncrementSpec):
            raise TypeError(f"Increments takes an IncrementSpec (got {type(spec).__name__})")
        self.spec = spec
        self.device = torch.device(device)
        self._ops = ops
        rows = (2, spec.nout, 2, spec.nlag)
        self._cnt = torch.zeros(*rows, spec.nbins + 3, dtype=torch.int64, device=self.device)
        self._fin = torch.zeros(*rows, dtype=torch.int64, device=self.device)
        self._mom = torch.zeros(*rows, 6, dtype=torch.float64, device=self.device)
        self.fields = 0
        self.nser = None
        self.grid = None
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    def add(self, real, fake=None, n_valid=None, nhwc=False, channels=None):
        """Add the increments of the first ``n_valid`` (default: all) fields of a batch: the real series alone, or the pair
        (real, generated).  Layouts as ``histograms.histogram`` ([T, C, H, W] fp32 / bf16; with ``nhwc`` a [T, H, W, c_pad]
        store of which the leading ``channels`` are read; a ``NativeBatch``); the two series may differ in layout and dtype:
        pass ``nhwc`` as a (real, fake) pair then."""
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "increment histograms", self.spec)
        nser, grid = 1 if b is None else 2, (a.H, a.W)
        if not all(1 <= v <= SIDE_MAX for v in grid):
            raise ValueError(f"increment histograms take grids of 1 <= H, W <= {SIDE_MAX} (got {grid[0]} x {grid[1]})")
        if self.nser not in (None, nser):
            raise ValueError(f"this accumulator holds {self.nser} series per add (got {nser})")
        if self.grid not in (None, grid):
            raise ValueError(f"this accumulator holds {self.grid[0]} x {self.grid[1]} fields (got {grid[0]} x {grid[1]})")
        self.nser, self.grid = nser, grid
        if self._struct is None:
            self._struct = self.spec.struct()
        o, (H, W) = self.ops, grid
        # one call for the whole batch: dg_incr's workspace is a fixed number of per-workgroup slots, whatever the field count
        ka, fa = fields.descriptor(o, a.x[:n], a.nhwc, a.C)
        kb, fb = fields.descriptor(o, b.x[:n], b.nhwc, b.C) if b is not None else (None, None)
        o.incr(fa, fb, H, W, self._struct, self._cnt[:nser], self._fin[:nser], self._mom[:nser])
        self.fields += n
        return self

    def reduce_(self, dist):
        """Sum over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place: the counts, ``finite`` and the
        field count exactly (``fss.allreduce_ints``), the moments in fp64."""
        if dist is not None and dist.world_size > 1:
            dev = self.device if getattr(dist, "backend", "gloo") == "nccl" else "cpu"
            nc, nf = self._cnt.numel(), self._fin.numel()
            vals = allreduce_ints(dist, self._cnt.reshape(-1).cpu().tolist() + self._fin.reshape(-1).cpu().tolist() + [self.fields], dev)
            self._cnt.copy_(torch.tensor(vals[:nc], dtype=torch.int64).reshape(self._cnt.shape))
            self._fin.copy_(torch.tensor(vals[nc:nc + nf], dtype=torch.int64).reshape(self._fin.shape))
            self.fields = vals[-1]
            dist.allreduce_sum_(self._mom.view(-1))
        return self

    def result(self):
        """The ``IncrementResult`` of every field added (and, after ``reduce_``, of every rank)."""
        ns = self.nser or 1
        H, W = self.grid or (0, 0)
        return IncrementResult(self.spec, self._cnt[:ns].cpu().numpy().copy(), self._fin[:ns].cpu().numpy().copy(),
                               self._mom[:ns].cpu().numpy().copy(), self.fields, H, W)


def increments(real, fake=None, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """Increment histograms of a series of fields (or of the pair real, generated) on the GPU -> ``IncrementResult``.  spec None:
    ``IncrementSpec.zscore`` of the fields' channels; the other arguments as ``Increments.add``."""
    if spec is not None and not isinstance(spec, IncrementSpec):
        raise TypeError(f"increments takes an IncrementSpec (got {type(spec).__name__})")
    Cn, _, _, device = fields.one_shot(real, nhwc, channels, "increment histograms")
    if spec is None:
        spec = IncrementSpec.zscore(Cn)
    return Increments(spec, device, ops=ops).add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
