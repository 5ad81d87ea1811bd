"""Temporal diagnostics of real and generated series on the GPU (csrc/temporal.hip): spells, ramps, lag autocorrelation.

Every other diagnostic of this package treats the fields of a series as an unordered sample (``gridstats``' "temporal correlation"
is the correlation of real against generated over the sample axis).  A generator that downscales frame by frame can have the right
marginals and spectra and still flicker from frame to frame; this module looks along the time axis of ONE series.  The fields
must be added in time order.  For output channel j of a ``TemporalSpec`` (the output values y of ``histograms``: y_c =
fp32(fp32(x_c * scale_c) + offset_c), the speed of the pair ``speed`` appended last) the device keeps, per series:

    spells    per threshold k and pixel: a spell is a maximal run of consecutive times with y > thr (``below[k]`` False) or
              y < thr (True); NaN and equality fail.  The pooled duration histogram (durations >= ndur in the last row), and per
              pixel the number of completed spells, their total time and the longest run.  A run still open after the last
              field is in no histogram row (right-censored: ``TemporalResult.censored``); a run that starts at time 0 is counted
              like any other although its true start is unknown (left-censored).
    ramps     per lag tau: the histogram of d = fp32(y[t] - y[t - tau]) under the 1-D bin rule of ``histograms`` on
              [-range, range), pooled over the pixels -- the time-axis twin of ``increments``.
    persistence  per pixel and lag, in float64 in t order: n, sum y, sum y^2 over the finite y and m, sum y[t] y[t - tau],
              sum (y[t] + y[t - tau]) over the pairs of finite values, from which follows the lag autocorrelation.

The state between calls (the open run of every pixel and its last max(lags) values) lives on the device, so the result does not
depend on how the series was cut into ``add`` calls, on layout or on dtype, down to the bits of the float64 sums; two runs on the
same data are bit-identical (integer atomics only, every float64 sum has one owner and a fixed order).
"""
from __future__ import annotations

import ctypes
import json
import math
import os

import numpy as np
import torch

from . import _lib, fields
from .gridstats import SIDES, _side
from .histograms import C_MAX, Histogram, HistSpec, _default_ops, _f32, ks_distance, wasserstein1
from .increments import _int, _jsonable, _ratio

THR_MAX = _lib.TEMPORAL_MAX_THR
DUR_MAX = _lib.TEMPORAL_MAX_DUR
LAGS_MAX = _lib.TEMPORAL_MAX_LAGS
LAG_MAX = _lib.TEMPORAL_MAX_LAG
BINS_MAX = _lib.TEMPORAL_MAX_BINS
DEFAULT_LAGS = (1, 2, 3, 6)
T_MAX = 2 ** 31


class TemporalSpec:
    """Thresholds, lags, bins and units of the temporal diagnostics of C input channels (+ the speed of a pair of them, appended
    last).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None;
    thresholds: 0 .. THR_MAX values per output channel -- one list per output channel, or one list of numbers for all -- rounded
    to fp32; below: per threshold, False: the spell is y > thr (storm), True: y < thr (drought) (one flag for all, or one per
    threshold); ndur: rows of the duration histogram (1 .. DUR_MAX; the last row takes every longer spell); lags: 0 .. LAGS_MAX
    strictly increasing lead times in fields, each in [1, LAG_MAX]; nbins: interior bins of every ramp table (1 .. BINS_MAX);
    ranges: the half-width of the binned interval [-range, range) per (output channel, lag) -- a scalar, one value per lag, or
    an [nout, nlag] array; names: one per output channel.  At least one threshold or one lag."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), thresholds=(), below=False, ndur=64, lags=DEFAULT_LAGS,
                 nbins=128, ranges=8.0, names=None):
        if not (_int(C) and 1 <= C <= C_MAX):
            raise ValueError(f"temporal diagnostics take 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"temporal speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"temporal scale and offset need one value per input channel (C = {self.C})")
        thr = list(thresholds)
        if all(np.ndim(t) == 0 for t in thr):
            thr = [thr] * self.nout                                  # one list for every channel
        if len(thr) != self.nout or len({len(t) for t in thr}) != 1:
            raise ValueError(f"temporal thresholds need one list per output channel ({self.nout}), all of one length")
        self.nthr = len(thr[0])
        if self.nthr > THR_MAX:
            raise ValueError(f"temporal diagnostics take at most {THR_MAX} thresholds per channel (got {self.nthr})")
        self.thresholds = (np.stack([_f32(t, "thresholds") for t in thr]) if self.nthr else np.zeros((self.nout, 0), np.float32))
        bl = [bool(below)] * self.nthr if np.ndim(below) == 0 else [bool(b) for b in below]
        if len(bl) != self.nthr:
            raise ValueError(f"temporal below needs one flag per threshold ({self.nthr}; got {len(bl)})")
        self.below = tuple(bl)
        if not (_int(ndur) and 1 <= ndur <= DUR_MAX):
            raise ValueError(f"temporal ndur must be an integer in [1, {DUR_MAX}] (got {ndur!r})")
        self.ndur = int(ndur)
        lags = list(lags)
        if len(lags) > LAGS_MAX:
            raise ValueError(f"a TemporalSpec holds at most {LAGS_MAX} lags (got {len(lags)})")
        if not all(_int(r) and 1 <= r <= LAG_MAX for r in lags):
            raise ValueError(f"temporal lags must be integers in [1, {LAG_MAX}] (got {lags})")
        if any(b <= a for a, b in zip(lags, lags[1:])):
            raise ValueError(f"temporal lags must be strictly increasing (got {lags})")
        self.lags = tuple(int(r) for r in lags)
        if self.nthr == 0 and self.nlag == 0:
            raise ValueError("a TemporalSpec needs at least one threshold or one lag")
        if not (_int(nbins) and 1 <= nbins <= BINS_MAX):
            raise ValueError(f"temporal nbins must be an integer in [1, {BINS_MAX}] (got {nbins!r})")
        self.nbins = int(nbins)
        r = np.asarray(ranges, dtype=np.float64)
        if r.ndim > 2 or (r.ndim == 1 and r.shape != (self.nlag,)) or (r.ndim == 2 and r.shape != (self.nout, self.nlag)):
            raise ValueError(f"temporal ranges are a scalar, one value per lag ({self.nlag}) or an [nout = {self.nout}, nlag = "
                             f"{self.nlag}] array (got shape {r.shape})")
        r = np.broadcast_to(r, (self.nout, self.nlag))
        self.ranges = _f32(r, "ranges").reshape(self.nout, self.nlag)
        if not np.all(self.ranges > 0):
            raise ValueError(f"temporal ranges must be > 0 (got {self.ranges.tolist()})")
        self.lo = -self.ranges
        inv_w = self.nbins / (2.0 * self.ranges.astype(np.float64))
        with np.errstate(over="ignore", under="ignore"):
            self.inv_w = inv_w.astype(np.float32)
        if not np.all(np.isfinite(self.inv_w) & (self.inv_w > 0)):
            raise ValueError(f"temporal bin width out of fp32 range: nbins / (2 range) = {inv_w.tolist()}")
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"temporal names need one entry per output channel ({self.nout})")

    @property
    def nlag(self):
        return len(self.lags)

    @property
    def R(self):
        """The largest lag: the number of past values kept per pixel (0 without lags)."""
        return self.lags[-1] if self.lags else 0

    @classmethod
    def zscore(cls, C, lags=DEFAULT_LAGS, ndur=64, nbins=128, lim=8.0):
        """Standardised fields: spells above +1, +2 and below -1, -2 on the components; with C >= 2 the speed of channels
        (0, 1) with spells above 1.5, 2.5 (storm) and below 0.5, 0.25 (wind drought); ramps on the symmetric range
        [-lim, lim)."""
        speed = (0, 1) if C >= 2 else None
        thr = [[1.0, 2.0, -1.0, -2.0]] * C + ([[1.5, 2.5, 0.5, 0.25]] if speed else [])
        return cls(C, speed=speed, thresholds=thr, below=(False, False, True, True), ndur=ndur, lags=lags, nbins=nbins, ranges=lim)

    def width(self):
        """float64 [nout, nlag]: the nominal ramp bin width 2 range / nbins."""
        return 2.0 * self.ranges.astype(np.float64) / self.nbins

    def struct(self):
        """The dg_temporal_spec of this spec (no library call)."""
        s = _lib.TemporalSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nthr, s.ndur, s.nlag, s.nbins = self.nthr, self.ndur, self.nlag, self.nbins
        for k, b in enumerate(self.below):
            s.below[k] = int(b)
        for l, r in enumerate(self.lags):
            s.lag[l] = r
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            for k in range(self.nthr):
                s.thr[j][k] = float(self.thresholds[j, k])
            for l in range(self.nlag):
                s.lo[j][l], s.inv_w[j][l] = float(self.lo[j, l]), float(self.inv_w[j, l])
        return s

    def shapes(self, S, P):
        """{name: (shape, numpy dtype)} of the seven device arrays of S series on P pixels, in the order of the C ABI."""
        o, K, L = self.nout, self.nthr, self.nlag
        return {"open": ((S, o, K, P), np.int32), "tail": ((S, o, self.R, P), np.float32), "spells": ((S, o, K, self.ndur), np.int64),
                "spellmap": ((S, o, K, 3, P), np.int32), "ramps": ((S, o, L, self.nbins + 3), np.int64),
                "acsum": ((S, o, 2 + 2 * L, P), np.float64), "accnt": ((S, o, 1 + L, P), np.int32)}

    def __eq__(self, other):
        return (isinstance(other, TemporalSpec) and self.C == other.C and self.speed == other.speed and self.lags == other.lags
                and self.below == other.below and self.ndur == other.ndur and self.nbins == other.nbins
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("thresholds", "ranges", "scale", "offset")))

    __hash__ = None


ARRAYS = ("open", "tail", "spells", "spellmap", "ramps", "acsum", "accnt")


def _check_spec(spec):
    if not isinstance(spec, TemporalSpec):
        raise TypeError(f"temporal diagnostics take a TemporalSpec (got {type(spec).__name__})")


def _check_time(t0, n):
    if t0 < 0 or t0 + n >= T_MAX:
        raise ValueError(f"a temporal series holds fewer than 2^31 fields: t0 = {t0} plus {n} fields is out of range")


def host_temporal(spec, x, t0=0, state=None):
    """{name: numpy array} of one series (the seven arrays of ``TemporalSpec.shapes`` without the series dimension) after
    adding x (fp32 [T, C, P], in time order) as the times t0 .. t0 + T - 1 to ``state`` (the dict of an earlier call, updated in
    place and returned; None: zeros), computed by the library on the host (dg_temporal_host, plain C++: the definition the
    kernel is tested against)."""
    _check_spec(spec)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3 or x.shape[1] != spec.C or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"host_temporal takes [T, C = {spec.C}, P] values (got shape {x.shape})")
    T, _, P = x.shape
    t0 = int(t0)
    _check_time(t0, T)
    if state is None:
        state = {k: np.zeros(shape[1:], dtype=dt) for k, (shape, dt) in spec.shapes(1, P).items()}
    for k, (shape, dt) in spec.shapes(1, P).items():
        if state[k].shape != shape[1:] or state[k].dtype != dt or not state[k].flags.c_contiguous:
            raise ValueError(f"host_temporal state {k!r} must be a contiguous {np.dtype(dt).name} array of shape {shape[1:]}")
    s = spec.struct()
    ptr = lambda a: a.ctypes.data if a.size else None
    _lib.check(_lib.lib().dg_temporal_host(ctypes.byref(s), x.ctypes.data, spec.C, T, P, t0, *[ptr(state[k]) for k in ARRAYS]),
               "dg_temporal_host")
    return state


def _bin_durations(runs, ndur):
    """int64 [..., ndur]: the open runs int32 [..., P] binned like spells (run r > 0 into row min(r, ndur) - 1), with torch
    where the runs live."""
    rows = (runs.clamp(max=ndur) - 1).to(torch.int64)
    on = (runs > 0).to(torch.int64)
    out = torch.zeros(runs.shape[:-1] + (ndur,), dtype=torch.int64, device=runs.device)
    if runs.numel():
        out.scatter_add_(-1, rows.clamp(min=0), on)
    return out


def _finite_mean(a):
    """The mean of the finite values over the last two axes (NaN where there is none)."""
    f = a.reshape(a.shape[:-2] + (-1,))
    ok = np.isfinite(f)
    return _ratio(np.where(ok, f, 0.0).sum(axis=-1), ok.sum(axis=-1))


class TemporalResult:
    """The temporal diagnostics of a TemporalSpec over S series (1: real only; 2: real, generated) of ``fields`` H x W fields, as
    numpy arrays (the integers and float64 sums of the device, see ``TemporalSpec.shapes``; ``censored`` int64
    [S, nout, nthr, ndur]: the runs still open after the last field, binned like ``spells``).  ``side`` is "real" (the only series
    when not paired) or "fake".  Every statistic is derived on the host in float64 and is NaN where undefined; ``summary``
    reports those as None."""

    def __init__(self, spec, H, W, paired, fields, spells, censored, spellmap, ramps, acsum, accnt):
        _check_spec(spec)
        self.spec, self.H, self.W, self.paired, self.fields = spec, int(H), int(W), bool(paired), int(fields)
        self.spells, self.cens = np.asarray(spells, dtype=np.int64), np.asarray(censored, dtype=np.int64)
        self.spellmap, self.ramps = np.asarray(spellmap, dtype=np.int32), np.asarray(ramps, dtype=np.int64)
        self.acsum, self.accnt = np.asarray(acsum, dtype=np.float64), np.asarray(accnt, dtype=np.int32)
        shapes = spec.shapes(self.S, self.H * self.W)
        for k, a in (("spells", self.spells), ("spells", self.cens), ("spellmap", self.spellmap), ("ramps", self.ramps),
                     ("acsum", self.acsum), ("accnt", self.accnt)):
            if a.shape != shapes[k][0]:
                raise ValueError(f"temporal array {k!r} of shape {a.shape} does not fit the spec ({shapes[k][0]})")

    @classmethod
    def from_state(cls, spec, H, W, fields, real, fake=None):
        """The result of one or two per-series array dicts as ``host_temporal`` returns them."""
        st = [real] if fake is None else [real, fake]
        arr = {k: np.stack([s[k] for s in st]) for k in ARRAYS}
        cens = _bin_durations(torch.from_numpy(arr["open"]), spec.ndur).numpy()
        return cls(spec, H, W, fake is not None, fields, arr["spells"], cens, arr["spellmap"], arr["ramps"], arr["acsum"], arr["accnt"])

    @property
    def S(self):
        return 2 if self.paired else 1

    def _map(self, a):
        a = np.asarray(a, dtype=np.float64)
        return a.reshape(a.shape[:-1] + (self.H, self.W))

    def _need_pair(self):
        if not self.paired:
            raise ValueError("this statistic compares the real and the generated series: Temporal(paired=True)")

    # ---- spells
    def spell_counts(self, side="real"):
        """int64 [nout, nthr, ndur]: completed spells by duration 1 .. ndur (the last row: ndur and longer), pooled over pixels."""
        return self.spells[_side(side, self.paired)].copy()

    def censored(self, side="real"):
        """int64 [nout, nthr, ndur]: the runs still open after the last field, by their length so far (not in spell_counts)."""
        return self.cens[_side(side, self.paired)].copy()

    def mean_duration(self, side="real"):
        """float64 [nout, nthr]: the mean length of the completed spells (exact: total time / count, not from the histogram)."""
        m = self.spellmap[_side(side, self.paired)].astype(np.int64)
        return _ratio(m[:, :, 1].sum(axis=-1), m[:, :, 0].sum(axis=-1))

    def duration_quantile(self, q, side="real"):
        """float64 [nout, nthr, Q] ([nout, nthr] for a scalar q): the smallest duration d with #{spells <= d} >= ceil(q n), 0 < q
        <= 1 (ndur stands for "ndur or longer"); NaN without completed spells."""
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1)
        if not np.all((qs > 0) & (qs <= 1)):
            raise ValueError(f"duration quantile levels must lie in (0, 1] (got {qs.tolist()})")
        c = self.spell_counts(side)
        cum, n = np.cumsum(c, axis=-1), c.sum(axis=-1)
        out = np.full(c.shape[:2] + (len(qs),), np.nan)
        for k, qk in enumerate(qs):
            target = np.maximum(np.ceil(qk * n.astype(np.float64)), 1.0)
            d = 1 + (cum < target[..., None]).sum(axis=-1)
            out[..., k] = np.where(n > 0, d, np.nan)
        return out[..., 0] if np.ndim(q) == 0 else out

    def duration_survival(self, side="real"):
        """float64 [nout, nthr, ndur]: the fraction of completed spells that last at least d = 1 .. ndur (NaN without any)."""
        c = self.spell_counts(side)
        at_least = np.cumsum(c[..., ::-1], axis=-1)[..., ::-1]
        return _ratio(at_least, np.broadcast_to(c.sum(axis=-1, keepdims=True), c.shape))

    def spell_frequency(self, side="real"):
        """float64 [nout, nthr, H, W]: completed spells per field added."""
        m = self.spellmap[_side(side, self.paired)]
        return self._map(_ratio(m[:, :, 0], np.full(m[:, :, 0].shape, self.fields)))

    def mean_spell_map(self, side="real"):
        """float64 [nout, nthr, H, W]: the mean length of a pixel's completed spells (NaN where it has none)."""
        m = self.spellmap[_side(side, self.paired)]
        return self._map(_ratio(m[:, :, 1], m[:, :, 0]))

    def longest_spell_map(self, side="real"):
        """float64 [nout, nthr, H, W]: the longest run of a pixel, open runs included."""
        return self._map(self.spellmap[_side(side, self.paired)][:, :, 2])

    # ---- ramps
    def ramp_hist(self, side="real"):
        """int64 [nout, nlag, nbins + 3]: the ramp counts with the rows of ``histograms.Histogram`` (underflow, bins, overflow,
        NaN); ``ramp_histogram`` wraps one of them."""
        return self.ramps[_side(side, self.paired)].copy()

    def ramp_histogram(self, channel, lag, side="real"):
        """The ``histograms.Histogram`` (one output channel; no moments or extrema) of the ramps of output channel ``channel``
        (index or name) at ``lag`` (a value of spec.lags): ``quantile`` inside [-range, range), ``wasserstein1`` and
        ``ks_distance`` apply."""
        sp = self.spec
        j = sp.names.index(channel) if isinstance(channel, str) else int(channel)
        if lag not in sp.lags:
            raise KeyError(f"lag {lag!r} is not one of {sp.lags}")
        l = sp.lags.index(lag)
        hs = HistSpec(sp.nbins, [float(sp.lo[j, l])], [float(sp.ranges[j, l])], speed=None, names=[sp.names[j]])
        c = torch.from_numpy(self.ramps[_side(side, self.paired), j, l][None].copy())
        ext = torch.tensor([[float(sp.lo[j, l]), float(sp.ranges[j, l])]])
        return Histogram(hs, c, torch.zeros(1, 2, dtype=torch.float64), ext, self.fields)

    def _ramp_distance(self, fn):
        self._need_pair()
        sp = self.spec
        out = np.full((sp.nout, sp.nlag), np.nan)
        for j, l in np.ndindex(*out.shape):
            out[j, l] = fn(self.ramp_histogram(j, sp.lags[l], "real"), self.ramp_histogram(j, sp.lags[l], "fake"))[0]
        return out

    def ramp_w1(self):
        """float64 [nout, nlag]: the 1-D Wasserstein distance of the real and the generated ramp distributions."""
        return self._ramp_distance(wasserstein1)

    def ramp_ks(self):
        """float64 [nout, nlag]: their Kolmogorov-Smirnov distance."""
        return self._ramp_distance(ks_distance)

    # ---- persistence
    def autocorrelation(self, side="real"):
        """float64 [nout, nlag, H, W]: r_tau = (c / m - mu e / m + mu^2) / (s2 / n - mu^2) with mu = s1 / n (the lagged
        covariance about the mean of all finite values over their variance); NaN where m = 0 or the variance is not > 0."""
        s = _side(side, self.paired)
        L = self.spec.nlag
        n = self.accnt[s, :, 0].astype(np.float64)[:, None]
        m = self.accnt[s, :, 1:].astype(np.float64)
        s1, s2 = self.acsum[s, :, 0][:, None], self.acsum[s, :, 1][:, None]
        c, e = self.acsum[s, :, 2:2 + 2 * L:2], self.acsum[s, :, 3:3 + 2 * L:2]
        with np.errstate(divide="ignore", invalid="ignore"):
            mu = s1 / n
            var = s2 / n - mu * mu
            r = (c / m - mu * e / m + mu * mu) / var
        return self._map(np.where((m > 0) & (var > 0), r, np.nan))

    def autocorrelation_bias(self):
        """Generated minus real autocorrelation (a flickering generator: negative at lag 1)."""
        self._need_pair()
        return self.autocorrelation("fake") - self.autocorrelation("real")

    def decorrelation_time(self, level=1.0 / math.e, side="real"):
        """float64 [nout, H, W]: the lead time, in fields, at which the autocorrelation first falls to ``level``, interpolated
        linearly between the given lags (r = 1 at lag 0); NaN when it never does within the lags, or where r is NaN first."""
        r = self.autocorrelation(side)
        out = np.full(r.shape[:1] + r.shape[2:], np.nan)
        done = np.zeros(out.shape, dtype=bool)
        prev_r, prev_t = np.ones(out.shape), 0.0
        for l, tau in enumerate(self.spec.lags):
            cur = r[:, l]
            bad = np.isnan(cur) & ~done
            hit = (cur <= level) & ~done
            with np.errstate(divide="ignore", invalid="ignore"):
                t = prev_t + (prev_r - level) / (prev_r - cur) * (tau - prev_t)
            out = np.where(hit, t, out)
            done |= hit | bad
            prev_r, prev_t = cur, float(tau)
        return out

    # ---- everything
    def maps(self):
        """{name: array} of every per-pixel map this result holds."""
        out = {}
        for side in SIDES[:self.S]:
            if self.spec.nthr:
                out[f"{side}_spell_frequency"] = self.spell_frequency(side)
                out[f"{side}_mean_spell"] = self.mean_spell_map(side)
                out[f"{side}_longest_spell"] = self.longest_spell_map(side)
            if self.spec.nlag:
                out[f"{side}_autocorrelation"] = self.autocorrelation(side)
                out[f"{side}_decorrelation_time"] = self.decorrelation_time(side=side)
        if self.paired and self.spec.nlag:
            out["autocorrelation_bias"] = self.autocorrelation_bias()
        return out

    def summary(self, q=(0.5, 0.9, 0.99)):
        """A JSON-serialisable dict (None where undefined); lists run over the output channels first."""
        sp = self.spec
        mean = lambda a: _jsonable(_finite_mean(a))
        out = {"channels": list(sp.names), "fields": self.fields, "grid": [self.H, self.W], "series": list(SIDES[:self.S]),
               "thresholds": sp.thresholds.astype(np.float64).tolist(), "below": list(sp.below), "ndur": sp.ndur,
               "lags": list(sp.lags), "nbins": sp.nbins, "q": [float(v) for v in q]}
        for side in SIDES[:self.S]:
            d = {}
            if sp.nthr:
                d["spells"] = self.spell_counts(side).sum(axis=-1).tolist()
                d["censored"] = self.censored(side).sum(axis=-1).tolist()
                d["mean_duration"] = _jsonable(self.mean_duration(side))
                d["duration_quantiles"] = _jsonable(self.duration_quantile(list(q), side))
                d["longest"] = self.spellmap[_side(side, self.paired)][:, :, 2].max(axis=-1).tolist()
            if sp.nlag:
                c = self.ramp_hist(side)
                d["ramp_nan"] = c[..., -1].tolist()
                d["ramp_out_of_range"] = (c[..., 0] + c[..., -2]).tolist()
                d["autocorrelation_mean"] = mean(self.autocorrelation(side))
                d["decorrelation_time_mean"] = mean(self.decorrelation_time(side=side))
            out[side] = d
        if self.paired and sp.nlag:
            out["ramp_w1"], out["ramp_ks"] = _jsonable(self.ramp_w1()), _jsonable(self.ramp_ks())
            out["autocorrelation_bias_mean"] = mean(self.autocorrelation_bias())
        return out

    def save(self, directory):
        """One ``<name>.npy`` per map and per pooled table (``<side>_spells``, ``<side>_censored``, ``<side>_ramps``) plus
        ``summary.json`` under ``directory`` (created); returns the file names."""
        os.makedirs(directory, exist_ok=True)
        arrays = dict(self.maps())
        for side in SIDES[:self.S]:
            if self.spec.nthr:
                arrays[f"{side}_spells"], arrays[f"{side}_censored"] = self.spell_counts(side), self.censored(side)
            if self.spec.nlag:
                arrays[f"{side}_ramps"] = self.ramp_hist(side)
        names = []
        for k, a in arrays.items():
            np.save(os.path.join(directory, k + ".npy"), a)
            names.append(k + ".npy")
        with open(os.path.join(directory, "summary.json"), "w") as f:
            json.dump(self.summary(), f, indent=1)
        return names + ["summary.json"]


class Temporal:
    """Running temporal diagnostics of the series added so far on an H x W grid.  The fields of every ``add`` continue the
    series where the last one ended (``fields`` counts them on the host: no sync in ``add``), so the caller feeds batches in time
    order and without gaps; how the series is cut into batches does not change any output bit.

    There is no ``reduce_``: a time series cannot be summed over data-parallel ranks that hold interleaved samples -- the spells
    and lagged products of the whole series are not functions of those of its sub-series.  Evaluate on one rank.

    ``nbytes``: the device arrays, dominated by the per-pixel state: S * nout * P * (4 nthr + 4 R + 12 nthr + 8 (2 + 2 nlag) +
    4 (1 + nlag)) bytes."""

    def __init__(self, spec, H, W, paired=True, device="cuda:0", ops=None):
        _check_spec(spec)
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"Temporal needs a grid of 1 <= H * W < 2^31 pixels (got {H} x {W})")
        self.spec, self.H, self.W, self.paired = spec, H, W, bool(paired)
        self.device = torch.device(device)
        self._ops = ops
        tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32,
               np.dtype(np.float64): torch.float64}
        self.arrays = {k: torch.zeros(shape, dtype=tdt[np.dtype(dt)], device=self.device)
                       for k, (shape, dt) in spec.shapes(2 if self.paired else 1, H * W).items()}
        self.fields = 0                                              # = t0 of the next add
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def nbytes(self):
        return sum(a.numel() * a.element_size() for a in self.arrays.values())

    def add(self, real, fake=None, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) fields of a batch as the next times of the series: ``real`` alone, or the
        pair (real, fake) when this accumulator is paired.  Layouts as ``gridhist.GridHist.add`` ([T, C, H, W]; with ``nhwc`` a
        [T, H, W, c_pad] store of which the leading ``channels`` are read; a ``NativeBatch``); the two series may differ in
        layout and dtype: pass ``nhwc`` as a pair (real, fake) then."""
        if self.paired != (fake is not None):
            raise ValueError("a paired Temporal takes (real, fake)" if self.paired else "this Temporal takes one series (paired=False)")
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "temporal diagnostics", self.spec, "Temporal", (self.H, self.W))
        _check_time(self.fields, n)
        if self._struct is None:
            self._struct = self.spec.struct()
        ka, fa = fields.descriptor(self.ops, a.x[:n], a.nhwc, a.C)
        kb, fb = fields.descriptor(self.ops, b.x[:n], b.nhwc, b.C) if self.paired else (None, None)
        self.ops.temporal(fa, fb, self._struct, self.fields, *[self.arrays[k] for k in ARRAYS])
        self.fields += n
        return self

    def result(self):
        """The ``TemporalResult`` of every field added."""
        A = self.arrays
        cens = _bin_durations(A["open"], self.spec.ndur)
        host = lambda t: t.detach().cpu().numpy().copy()
        return TemporalResult(self.spec, self.H, self.W, self.paired, self.fields, host(A["spells"]), host(cens), host(A["spellmap"]),
                              host(A["ramps"]), host(A["acsum"]), host(A["accnt"]))


def temporal(real, fake=None, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """Temporal diagnostics of one series of fields in time order, or of a (real, fake) pair, on the GPU -> ``TemporalResult``.
    spec None: ``TemporalSpec.zscore`` of the fields' channels; the other arguments as ``Temporal.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "temporal diagnostics")
    if spec is None:
        spec = TemporalSpec.zscore(Cn)
    _check_spec(spec)
    acc = Temporal(spec, H, W, paired=fake is not None, device=device, ops=ops)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
