"""Per-gridpoint statistics maps of real and generated fields, computed on the GPU (csrc/gridstats.hip).

Where on the grid is a downscaling generator wrong?  The EOF, spectrum and histogram diagnostics pool over space; this one
reduces over the fields t and keeps the pixel p.  For output channel j of a ``GridSpec`` (the transform of ``histograms``,
the same device code):

    y_c = fp32(fp32(x_c * scale_c) + offset_c)                 physical units (default scale 1, offset 0: y = x)
    s   = sqrt_rn(fp32(fp32(y_u * y_u) + fp32(y_v * y_v)))      the speed of the pair ``speed`` = (u, v), appended last
    u   = float64(y) - float64(pivot_j)                         valid <=> y finite

the device keeps, per series and pixel, n, sum u .. sum u^4 (fp64), min, max (fp32) and the counts of y > threshold; for a
(real, generated) pair also n_ab, sum d, sum |d|, sum d^2 (d = y_fake - y_real) and sum u_real u_fake over the fields where
both are valid.  ``GridStats`` accumulates batches on the device (and over data-parallel ranks), the trainer's opt-in hook
(``WassersteinGAN.log_maps``) keeps one per part, and ``GridMaps`` derives the maps every downscaling paper shows -- mean,
standard deviation, skewness, kurtosis, extremes, exceedance frequencies, bias, MAE, RMSE, temporal correlation -- on the host in
float64.  Counts and extrema are exact; two calls on the same data are bit-identical (no atomics, t-ordered sums).
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from . import _lib, fields
from .histograms import C_MAX, _default_ops, _f32

THR_MAX = _lib.GRID_MAX_THR
SIDES = ("real", "fake")


class GridSpec:
    """Units, pivots and thresholds of the per-gridpoint statistics of C input channels (+ the speed of a pair of them,
    appended as the last output).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None; pivot:
    per output channel, the value the power sums are taken about (default: ``offset`` for the components, 0 for the speed;
    a pivot near the mean keeps the moments well conditioned); thresholds: up to THR_MAX values per output channel -- one
    list per output channel, or one list of numbers for all -- rounded to fp32; names: one per output channel."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), pivot=None, thresholds=(), names=None):
        if not (isinstance(C, (int, np.integer)) and 1 <= C <= C_MAX):
            raise ValueError(f"gridstats takes 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"gridstats speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"gridstats scale and offset need one value per input channel (C = {self.C})")
        if pivot is None:
            pivot = list(self.offset) + ([0.0] if self.speed is not None else [])
        self.pivot = _f32(pivot, "pivot")
        if len(self.pivot) != self.nout:
            raise ValueError(f"gridstats pivot needs one value per output channel ({self.nout})")
        thr = list(thresholds)
        if all(np.ndim(t) == 0 for t in thr):
            thr = [thr] * self.nout                                  # one list for every channel
        if len(thr) != self.nout or len({len(t) for t in thr}) != 1:
            raise ValueError(f"gridstats thresholds need one list per output channel ({self.nout}), all of one length")
        K = len(thr[0])
        if K > THR_MAX:
            raise ValueError(f"gridstats takes at most {THR_MAX} thresholds per channel (got {K})")
        self.thresholds = (np.stack([_f32(t, "thresholds") for t in thr]) if K else np.zeros((self.nout, 0), np.float32))
        self.K = K
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"gridstats names need one entry per output channel ({self.nout})")

    @classmethod
    def zscore(cls, C, thresholds=(2.0, 3.0)):
        """Standardised fields: pivot 0, the speed of channels (0, 1) when C >= 2, the same thresholds in every channel."""
        return cls(C, speed=(0, 1) if C >= 2 else None, thresholds=thresholds)

    @classmethod
    def physical(cls, stats, order, thresholds=(), speed=("u10", "v10")):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, evaluated
        in physical units (y = x * std + mean, pivot = mean).  thresholds: as the constructor's, in physical units; speed: the
        names of the (u, v) pair, or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        names = order + (["speed"] if sp else [])
        return cls(len(order), scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp,
                   thresholds=thresholds, names=names)

    def struct(self):
        """The dg_grid_spec of this spec (no library call)."""
        s = _lib.GridSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nthr = self.K
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            s.pivot[j] = float(self.pivot[j])
            for k in range(self.K):
                s.thr[j][k] = float(self.thresholds[j, k])
        return s

    def __eq__(self, other):
        return (isinstance(other, GridSpec) and self.C == other.C and self.speed == other.speed
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("scale", "offset", "pivot", "thresholds")))

    __hash__ = None


def rows(paired, K):
    """(sums, extrema, counts) rows per output channel of the device arrays (include/downgan_hip.h)."""
    return (12, 4, 3 + 2 * K) if paired else (4, 2, 1 + K)


def _side(side, paired):
    s = {"real": 0, "fake": 1, 0: 0, 1: 1}.get(side)
    if s is None or (s == 1 and not paired):
        raise ValueError(f"side must be 'real'{' or ' + repr('fake') if paired else ''} (got {side!r})")
    return s


def _jsonable(a):
    a = np.asarray(a, dtype=np.float64)
    return [None if not math.isfinite(v) else float(v) for v in a.reshape(-1)] if a.ndim == 1 else [_jsonable(r) for r in a]


def _pattern_corr(a, b):
    """Per channel: the Pearson correlation over the pixels where both maps are finite."""
    out = np.full(a.shape[0], np.nan)
    for j in range(a.shape[0]):
        m = np.isfinite(a[j]) & np.isfinite(b[j])
        if m.sum() >= 2:
            x, y = a[j][m] - a[j][m].mean(), b[j][m] - b[j][m].mean()
            d = math.sqrt(float((x * x).sum()) * float((y * y).sum()))
            out[j] = float((x * y).sum()) / d if d > 0 else np.nan
    return out


class GridMaps:
    """The accumulated per-pixel sums of one GridSpec on an H x W grid: device (or CPU) tensors sums fp64 [nout, 4 | 12, P],
    extrema fp32 [nout, 2 | 4, P], counts int32 [nout, 1 + K | 3 + 2 K, P] and the number of fields.  Every map is derived on
    the host in float64, shape [nout, H, W]; ``side`` is "real" (the only series when not paired) or "fake"."""

    def __init__(self, spec, H, W, paired, sums, extrema, counts, fields):
        self.spec, self.H, self.W, self.paired, self.fields = spec, int(H), int(W), bool(paired), int(fields)
        self.sums, self.extrema, self.counts = sums, extrema, counts
        self._h = None

    def host(self):
        """(sums float64 [nout, NS, P], extrema float32 [nout, NE, P], counts int32 [nout, NC, P]) as numpy arrays (copied
        once)."""
        if self._h is None:
            P, n = self.H * self.W, self.spec.nout
            self._h = tuple(t.detach().cpu().numpy().copy().reshape(n, -1, P) for t in (self.sums, self.extrema, self.counts))
        return self._h

    def _map(self, a):
        return np.asarray(a, dtype=np.float64).reshape(a.shape[:-1] + (self.H, self.W))

    def _S(self, side):
        s = _side(side, self.paired)
        return [self._map(self.host()[0][:, 4 * s + k]) for k in range(4)]

    def count(self, side="real"):
        """Valid (finite) values per pixel."""
        s = _side(side, self.paired)
        return self._map(self.host()[2][:, s])

    def _central(self, side):
        """n, m1 (about the pivot) and the central moments m2, m3, m4 (NaN where n = 0)."""
        n = self.count(side)
        S1, S2, S3, S4 = self._S(side)
        with np.errstate(invalid="ignore", divide="ignore"):
            a1, a2, a3, a4 = S1 / n, S2 / n, S3 / n, S4 / n
            m2 = np.maximum(a2 - a1 * a1, 0.0)
            m3 = a3 - 3 * a1 * a2 + 2 * a1 ** 3
            m4 = a4 - 4 * a1 * a3 + 6 * a1 * a1 * a2 - 3 * a1 ** 4
        return n, a1, m2, m3, m4

    def mean(self, side="real"):
        return self._central(side)[1] + self.spec.pivot.astype(np.float64)[:, None, None]

    def variance(self, side="real", ddof=0):
        n, _, m2, _, _ = self._central(side)
        with np.errstate(invalid="ignore", divide="ignore"):
            return m2 if ddof == 0 else np.where(n > ddof, m2 * n / (n - ddof), np.nan)

    def std(self, side="real", ddof=0):
        return np.sqrt(self.variance(side, ddof))

    def skewness(self, side="real"):
        _, _, m2, m3, _ = self._central(side)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(m2 > 0, m3 / m2 ** 1.5, np.nan)

    def kurtosis(self, side="real"):
        """Excess kurtosis m4 / m2^2 - 3."""
        _, _, m2, _, m4 = self._central(side)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(m2 > 0, m4 / (m2 * m2) - 3.0, np.nan)

    def _ext(self, side, which):
        s = _side(side, self.paired)
        e = self._map(self.host()[1][:, 2 * s + which])
        return np.where(self.count(side) > 0, e, np.nan)

    def min(self, side="real"):
        return self._ext(side, 0)

    def max(self, side="real"):
        return self._ext(side, 1)

    def exceedance(self, side="real"):
        """float64 [nout, K, H, W]: the fraction of ALL fields with y > threshold (a NaN never exceeds, +inf always does)."""
        s, K = _side(side, self.paired), self.spec.K
        e0 = (3 + s * K) if self.paired else 1
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._map(self.host()[2][:, e0:e0 + K]) / float(self.fields)

    def _need_pair(self):
        if not self.paired:
            raise ValueError("bias, MAE, RMSE and correlation need a (real, fake) pair: GridStats(paired=True)")

    def count_pairs(self):
        self._need_pair()
        return self._map(self.host()[2][:, 2])

    def _paired(self, row):
        self._need_pair()
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._map(self.host()[0][:, row]) / self.count_pairs()

    def bias(self):
        """mean of y_fake - y_real over the fields where both are valid."""
        return self._paired(8)

    def mae(self):
        return self._paired(9)

    def rmse(self):
        return np.sqrt(self._paired(10))

    def correlation(self):
        """Temporal Pearson correlation per pixel; NaN where the pair count differs from either side's count (the one-sided
        moments then cover other fields than the cross sum) and where a variance is 0."""
        na, a1, va, _, _ = self._central("real")
        nb, b1, vb, _, _ = self._central("fake")
        nab = self.count_pairs()
        with np.errstate(invalid="ignore", divide="ignore"):
            cov = self._map(self.host()[0][:, 11]) / nab - a1 * b1
            r = cov / np.sqrt(va * vb)
        return np.where((nab == na) & (nab == nb) & (va > 0) & (vb > 0), r, np.nan)

    def std_ratio(self):
        """std_fake / std_real (NaN where the real field is constant)."""
        self._need_pair()
        sa, sb = self.std("real"), self.std("fake")
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(sa > 0, sb / sa, np.nan)

    def nonfinite(self, side="real"):
        """int [nout]: the NaN / inf values seen."""
        return (self.fields * self.H * self.W - self.count(side).reshape(self.spec.nout, -1).sum(axis=1)).astype(np.int64)

    def maps(self):
        """{name: array} of every map this result holds."""
        out = {}
        for side in SIDES[:2 if self.paired else 1]:
            for k in ("count", "mean", "std", "skewness", "kurtosis", "min", "max", "exceedance"):
                out[f"{side}_{k}"] = getattr(self, k)(side)
        if self.paired:
            for k in ("bias", "mae", "rmse", "correlation", "std_ratio"):
                out[k] = getattr(self, k)()
        return out

    def summary(self):
        """A JSON-serialisable dict, one entry per output channel in every list (None where undefined)."""
        dom = lambda a: np.array([np.nanmean(r) if np.isfinite(r).any() else np.nan for r in a.reshape(a.shape[0], -1)])
        s = {"channels": list(self.spec.names), "fields": self.fields, "grid": [self.H, self.W],
             "thresholds": _jsonable(self.spec.thresholds),
             "nonfinite": {side: [int(v) for v in self.nonfinite(side)] for side in SIDES[:2 if self.paired else 1]}}
        for side in SIDES[:2 if self.paired else 1]:
            s[f"{side}_mean"] = _jsonable(dom(self.mean(side)))
            s[f"{side}_std"] = _jsonable(dom(self.std(side)))
        if self.paired:
            bias, corr = self.bias(), self.correlation()
            with np.errstate(invalid="ignore"):
                s["bias_mean"] = _jsonable(dom(bias))
                s["abs_bias_mean"] = _jsonable(dom(np.abs(bias)))
                s["mae_mean"] = _jsonable(dom(self.mae()))
                s["rmse_rms"] = _jsonable(np.sqrt(dom(self.rmse() ** 2)))
                s["corr_mean"] = _jsonable(dom(corr))
                s["corr_min"] = _jsonable(np.array([np.nanmin(r) if np.isfinite(r).any() else np.nan
                                                    for r in corr.reshape(corr.shape[0], -1)]))
                s["pattern_corr_mean"] = _jsonable(_pattern_corr(self.mean("real"), self.mean("fake")))
                s["pattern_corr_std"] = _jsonable(_pattern_corr(self.std("real"), self.std("fake")))
                d = np.abs(self.exceedance("fake") - self.exceedance("real")).reshape(self.spec.nout, self.spec.K, -1)
                s["exceed_max_abs_diff"] = _jsonable(d.max(axis=2)) if self.spec.K else [[] for _ in range(self.spec.nout)]
        return s

    def save(self, directory):
        """One ``<name>.npy`` per map plus ``summary.json`` under ``directory`` (created); returns the file names."""
        os.makedirs(directory, exist_ok=True)
        names = []
        for k, a in self.maps().items():
            np.save(os.path.join(directory, k + ".npy"), a)
            names.append(k + ".npy")
        with open(os.path.join(directory, "summary.json"), "w") as f:
            json.dump(self.summary(), f, indent=1)
        return names + ["summary.json"]


class GridStats:
    """Running per-pixel statistics of the fields added so far on an H x W grid; everything stays on the device (``reduce_``:
    one fp64 and one int32 all-reduce plus the min / max of the extrema under data parallelism)."""

    def __init__(self, spec, H, W, paired=True, device="cuda:0", ops=None):
        if not isinstance(spec, GridSpec):
            raise TypeError(f"GridStats takes a GridSpec (got {type(spec).__name__})")
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"GridStats needs a grid of 1 <= H * W < 2^31 pixels (got {H} x {W})")
        self.spec, self.H, self.W, self.paired = spec, H, W, bool(paired)
        self.device = torch.device(device)
        self._ops = ops
        P, (ns, ne, nc) = H * W, rows(self.paired, spec.K)
        self._sums = torch.zeros(spec.nout, ns, P, dtype=torch.float64, device=self.device)
        ext = torch.empty(spec.nout, ne // 2, 2, P, dtype=torch.float32)
        ext[:, :, 0], ext[:, :, 1] = math.inf, -math.inf
        self._ext = ext.view(spec.nout, ne, P).to(self.device)
        self._cnt = torch.zeros(spec.nout, nc, P, dtype=torch.int32, device=self.device)
        self._nf = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._added = 0                                              # this rank's fields (host mirror: no sync in add)
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def fields(self):
        return int(self._nf.item())

    def add(self, real, fake=None, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) fields of a batch: ``real`` alone, or the pair (real, fake) when this
        accumulator is paired.  Layouts as ``histograms.histogram`` ([T, C, H, W]; with ``nhwc`` a [T, H, W, c_pad] store of
        which the leading ``channels`` are read; a ``NativeBatch``); the two series may differ in layout and dtype: pass
        ``nhwc`` as a pair (real, fake) then."""
        if self.paired != (fake is not None):
            raise ValueError("a paired GridStats takes (real, fake)" if self.paired else "this GridStats takes one series (paired=False)")
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "gridstats", self.spec, "GridStats", (self.H, self.W))
        if self._added + n >= 2 ** 31:
            raise ValueError(f"GridStats counts in int32: {self._added} + {n} fields would reach 2^31")
        if self._struct is None:
            self._struct = self.spec.struct()
        ka, fa = fields.descriptor(self.ops, a.x[:n], a.nhwc, a.C)
        kb, fb = fields.descriptor(self.ops, b.x[:n], b.nhwc, b.C) if self.paired else (None, None)
        self.ops.gridstats(fa, fb, self._struct, self._sums, self._ext, self._cnt)
        self._nf += n
        self._added += n
        return self

    def reduce_(self, dist):
        """Sum the sums and counts and take the extrema over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist),
        once, in place."""
        if dist is not None and dist.world_size > 1:
            dist.allreduce_sum_(self._nf)
            if self.fields >= 2 ** 31:
                raise ValueError(f"GridStats counts in int32: the ranks hold {self.fields} fields together (>= 2^31)")
            dist.allreduce_sum_(self._sums.view(-1))
            dist.allreduce_sum_(self._cnt.view(-1))
            n, ne, P = self._ext.shape
            mm = self._ext.view(n, ne // 2, 2, P).permute(0, 1, 3, 2).contiguous()     # (min, max) pairs, as Dist.minmax_ takes
            dist.minmax_(mm.view(1, -1), mm.numel() // 2)
            self._ext.view(n, ne // 2, 2, P).copy_(mm.permute(0, 1, 3, 2))
        return self

    def result(self):
        """The ``GridMaps`` of every field added (and, after ``reduce_``, of every rank)."""
        return GridMaps(self.spec, self.H, self.W, self.paired, self._sums.clone(), self._ext.clone(), self._cnt.clone(), self.fields)


def gridstats(real, fake=None, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """Per-gridpoint statistics of one series of fields, or of a (real, fake) pair, on the GPU -> ``GridMaps``.  spec None:
    ``GridSpec.zscore`` of the fields' channels; the other arguments as ``GridStats.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "gridstats")
    if spec is None:
        spec = GridSpec.zscore(Cn)
    if not isinstance(spec, GridSpec):
        raise TypeError(f"gridstats takes a GridSpec (got {type(spec).__name__})")
    acc = GridStats(spec, H, W, paired=fake is not None, device=device, ops=ops)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
