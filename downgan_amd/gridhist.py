"""Per-gridpoint histograms of real and generated fields, computed on the GPU (csrc/gridhist.hip).

What is the distribution AT a gridpoint?  ``histograms`` pools over space and time and ``gridstats`` keeps four moments and at
most four threshold counts per pixel; neither gives the map every downscaling evaluation opens with: the local 95th / 98th /
99th percentile of wind speed, real against generated, and with it the VALUE-style indices ("P98 bias", the local QQ line, the
local Kolmogorov-Smirnov and Wasserstein distances).  For output channel j of a ``histograms.HistSpec`` (its transform, speed
channel, lo / hi / bins, at most BINS_MAX bins) the device keeps

    counts int32 [nout, S, bins + 3, P]      S = 1: one series; S = 2: (real, generated); the pixel index fastest
    counts[j, s, r, p] = the number of added fields whose output channel j at pixel p fell in row r

with the rows of ``histograms``: 0 underflow, 1 .. bins interior, bins + 1 overflow, bins + 2 NaN, the same device code bit for
bit.  The table is per pixel, so it takes nout * S * (bins + 3) * P * 4 bytes: 1.6 GB for nout = 3, S = 2, bins = 64 on a
1024 x 1024 grid, 26 MB on 128 x 128 (``GridHist.nbytes``).  Counts are exact and do not depend on how the fields were chunked
into calls, on layout or on dtype (bf16 inputs are the values the kernel reads); two calls on the same data are bit-identical
(integer atomics only).  ``GridHist`` accumulates batches on the device (and over data-parallel ranks), the trainer's opt-in hook
(``WassersteinGAN.log_quantile_maps``) keeps one per part, and ``GridHistMaps`` derives the maps: a second kernel scans the table
on the device into integer quantile ranks and the integer W1 / KS sums, and only those maps come to the host, where float64
finishes them.  The tables are also the input of empirical quantile mapping (``downgan_amd.qmap``: ``QuantileMap.fit`` of a paired result).
"""
from __future__ import annotations

import ctypes
import json
import os

import numpy as np
import torch

from . import _lib, fields
from .gridstats import SIDES, _jsonable, _side
from .histograms import HistSpec, _default_ops

BINS_MAX = _lib.GRIDHIST_MAX_BINS
Q_MAX = _lib.GRIDHIST_MAX_Q
FIELDS_MAX = 2 ** 26             # 2 (bins + 1) n^2 must stay below 2^63 in the integer W1 sum


def _check_spec(spec):
    if not isinstance(spec, HistSpec):
        raise TypeError(f"GridHist takes a histograms.HistSpec (got {type(spec).__name__})")
    if spec.bins > BINS_MAX:
        raise ValueError(f"per-gridpoint histograms take at most {BINS_MAX} bins: the table is per pixel (got bins = {spec.bins})")


def _levels(q):
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1)
    if not 1 <= len(qs) <= Q_MAX:
        raise ValueError(f"between 1 and {Q_MAX} quantile levels per scan (got {len(qs)})")
    if not np.all((qs > 0) & (qs < 1)):                              # false for NaN
        raise ValueError(f"quantile levels must lie in (0, 1) (got {qs.tolist()})")
    return qs


def _planar(spec, x, what):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3 or x.shape[1] != spec.C or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"host_table takes [T, C = {spec.C}, P] values (got shape {x.shape} for {what})")
    return x


def host_table(spec, xa, xb=None):
    """int32 [nout, S, bins + 3, P]: the table of xa (and xb) float32 [T, C, P], computed by the library on the host
    (dg_gridhist_host, plain C++: the definition the kernels are tested against)."""
    _check_spec(spec)
    xa = _planar(spec, xa, "xa")
    if xb is not None:
        xb = _planar(spec, xb, "xb")
        if xb.shape != xa.shape:
            raise ValueError(f"host_table needs two series of one shape (got {xa.shape} and {xb.shape})")
    T, _, P = xa.shape
    out = np.zeros((spec.nout, 2 if xb is not None else 1, spec.bins + 3, P), dtype=np.int32)
    s = spec.struct()
    _lib.check(_lib.lib().dg_gridhist_host(ctypes.byref(s), xa.ctypes.data, xb.ctypes.data if xb is not None else None, spec.C,
                                           T, P, out.ctypes.data), "dg_gridhist_host")
    return out


def _scan_shapes(counts, q):
    qs = _levels(q)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if counts.ndim != 4 or counts.shape[1] not in (1, 2) or not 1 <= counts.shape[2] - 3 <= BINS_MAX or counts.shape[3] < 1:
        raise ValueError(f"a table is int32 [nout, 1 | 2, bins + 3, P] with bins <= {BINS_MAX} (got shape {counts.shape})")
    return counts, qs


def host_scan(counts, q):
    """(ranks int32 [nout, S, Q, 3, P], dist int64 [nout, 2, P] or None for S = 1) of a table int32 [nout, S, bins + 3, P] for
    the levels q, computed by the library on the host (dg_gridhist_scan_host)."""
    counts, qs = _scan_shapes(counts, q)
    nout, S, nb3, P = counts.shape
    ranks = np.empty((nout, S, len(qs), 3, P), dtype=np.int32)
    dist = np.empty((nout, 2, P), dtype=np.int64) if S == 2 else None
    qa = (ctypes.c_double * len(qs))(*qs.tolist())
    _lib.check(_lib.lib().dg_gridhist_scan_host(counts.ctypes.data, nout, S, nb3 - 3, P, qa, len(qs), ranks.ctypes.data,
                                                dist.ctypes.data if dist is not None else None), "dg_gridhist_scan_host")
    return ranks, dist


class GridHistMaps:
    """The accumulated per-pixel histograms of one HistSpec on an H x W grid: the device (or CPU) table int32
    [nout, S, bins + 3, P] and the number of fields.  Every map is float64 [nout, (Q,) H, W]; ``side`` is "real" (the only series
    when not paired) or "fake".  The scans run where the table lives: on the device through ``ops`` (dg_gridhist_scan), for a
    CPU table through the library's host reference; only integer maps [.., Q, 3, P] and [.., 2, P] and per-pixel row sums come
    to the host, never the table -- except through ``table()``."""

    def __init__(self, spec, H, W, paired, counts, fields, ops=None):
        _check_spec(spec)
        self.spec, self.H, self.W, self.paired, self.fields = spec, int(H), int(W), bool(paired), int(fields)
        self.counts, self._ops = counts, ops
        self._scans, self._rows = {}, {}

    @property
    def S(self):
        return 2 if self.paired else 1

    def table(self):
        """int32 numpy [nout, S, bins + 3, P]: the whole table on the host (as large as the table: see the module docstring)."""
        return self.counts.detach().cpu().numpy().copy()

    def _map(self, a):
        a = np.asarray(a, dtype=np.float64)
        return a.reshape(a.shape[:-1] + (self.H, self.W))

    def _rowsum(self, key, lo, hi):
        """int64 numpy [nout, S, P]: the sum of the rows lo .. hi - 1 per pixel (reduced where the table lives)."""
        if key not in self._rows:
            self._rows[key] = self.counts[:, :, lo:hi].sum(dim=2, dtype=torch.int64).cpu().numpy()
        return self._rows[key]

    def _finite(self):
        return self._rowsum("finite", 0, self.spec.bins + 2)

    def count(self, side="real"):
        """Finite values per pixel."""
        return self._map(self._finite()[:, _side(side, self.paired)])

    def nan(self, side="real"):
        """NaN values per pixel."""
        b = self.spec.bins
        return self._map(self._rowsum("nan", b + 2, b + 3)[:, _side(side, self.paired)])

    def out_of_range(self, side="real"):
        """The fraction of a pixel's finite values in the underflow plus overflow rows (NaN where it has none)."""
        s, b = _side(side, self.paired), self.spec.bins
        out = self._rowsum("under", 0, 1)[:, s] + self._rowsum("over", b + 1, b + 2)[:, s]
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._map(out / self._finite()[:, s].astype(np.float64))

    def scan(self, q=(0.5,)):
        """(ranks int32 [nout, S, Q, 3, P], dist int64 [nout, 2, P] or None) of the levels q as numpy arrays: one pass of the
        scan kernel over the table (cached per q)."""
        qs = _levels(q)
        key = tuple(qs.tolist())
        if key not in self._scans:
            c = self.counts
            if c.is_cuda or self._ops is not None:
                o = self._ops if self._ops is not None else _default_ops(c.device)
                nout, S, _, P = c.shape
                ranks = torch.empty(nout, S, len(qs), 3, P, dtype=torch.int32, device=c.device)
                dist = torch.empty(nout, 2, P, dtype=torch.int64, device=c.device) if S == 2 else None
                o.gridhist_scan(c, key, ranks, dist)
                self._scans[key] = (ranks.cpu().numpy(), dist.cpu().numpy() if dist is not None else None)
            else:
                self._scans[key] = host_scan(c.numpy(), qs)
        return self._scans[key]

    def quantile(self, q, side="real"):
        """float64 [nout, Q, H, W] ([nout, H, W] for a scalar q): lo + (b - 1) w + (q n - below) / counts[b] * w in the
        interior row b that holds the ceil(q n)-th smallest value (the interior formula of ``Histogram.quantile``); ``lo`` in
        the underflow row and ``hi`` in the overflow row (flagged by ``out_of_range``); NaN where the pixel has no finite
        value.  Error: one bin width inside [lo, hi)."""
        s = _side(side, self.paired)
        qs = _levels(q)
        r = self.scan(qs)[0][:, s].astype(np.float64)                # [nout, Q, 3, P]
        b, below, cnt = r[:, :, 0], r[:, :, 1], r[:, :, 2]
        n = self._finite()[:, s].astype(np.float64)[:, None, :]
        lo, hi, w = (v.astype(np.float64)[:, None, None] for v in (self.spec.lo, self.spec.hi, self.spec.width()))
        with np.errstate(invalid="ignore", divide="ignore"):
            inner = lo + (b - 1) * w + (qs[None, :, None] * n - below) / cnt * w
        out = np.where(b < 0, np.nan, np.where(b == 0, lo, np.where(b > self.spec.bins, hi, inner)))
        out = self._map(out)
        return out[:, 0] if np.ndim(q) == 0 else out

    def _need_pair(self):
        if not self.paired:
            raise ValueError("quantile bias, W1 and KS need a (real, fake) pair: GridHist(paired=True)")

    def quantile_bias(self, q):
        """Generated minus real quantile."""
        self._need_pair()
        return self.quantile(q, "fake") - self.quantile(q, "real")

    def _dist(self, row):
        self._need_pair()
        d = self.scan(next(iter(self._scans), (0.5,)))[1][:, row].astype(np.float64)
        n = self._finite().astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(d < 0, np.nan, d / (n[:, 0] * n[:, 1]))

    def w1(self):
        """The 1-D Wasserstein distance of the two binned distributions of each pixel (the convention of
        ``histograms.wasserstein1``: underflow mass at lo, interior bin at its centre, overflow at hi); NaN where a side has
        no finite value."""
        return self._map(self._dist(0) * (self.spec.width() / 2)[:, None])

    def ks(self):
        """max_r |F_real(r) - F_fake(r)| on the binned support of each pixel (``histograms.ks_distance``)."""
        return self._map(self._dist(1))

    def pooled(self, side="real"):
        """The ``histograms.Histogram``-compatible counts int64 numpy [nout, bins + 3] summed over the pixels: what
        ``histograms.histogram`` counts on the same data."""
        s = _side(side, self.paired)
        return self.counts[:, s].sum(dim=2, dtype=torch.int64).cpu().numpy()

    def maps(self, q=(0.5, 0.95, 0.99)):
        """{name: array} of every map this result holds at the levels q."""
        out = {}
        for side in SIDES[:self.S]:
            out[f"{side}_count"], out[f"{side}_nan"] = self.count(side), self.nan(side)
            out[f"{side}_out_of_range"] = self.out_of_range(side)
            out[f"{side}_quantile"] = self.quantile(list(q), side)
        if self.paired:
            out["quantile_bias"], out["w1"], out["ks"] = self.quantile_bias(list(q)), self.w1(), self.ks()
        return out

    def summary(self, q=(0.5, 0.95, 0.99)):
        """A JSON-serialisable dict, one entry per output channel in every list (None where undefined)."""
        qs = _levels(q)
        flat = lambda a: a.reshape(a.shape[0], -1)
        stat = lambda a, f: np.array([f(r[np.isfinite(r)]) if np.isfinite(r).any() else np.nan for r in flat(a)])
        s = {"channels": list(self.spec.names), "fields": self.fields, "grid": [self.H, self.W], "bins": self.spec.bins,
             "q": qs.tolist(), "nbytes": int(self.counts.numel()) * 4,
             "nan": {side: [int(v) for v in flat(self.nan(side)).sum(axis=1)] for side in SIDES[:self.S]},
             "out_of_range_max": {side: _jsonable(stat(self.out_of_range(side), np.max)) for side in SIDES[:self.S]}}
        for side in SIDES[:self.S]:
            qm = self.quantile(qs, side)
            s[f"{side}_quantile_mean"] = [_jsonable(stat(qm[:, k], np.mean)) for k in range(len(qs))]
        if self.paired:
            bias = np.abs(self.quantile_bias(qs))
            s["abs_quantile_bias_mean"] = [_jsonable(stat(bias[:, k], np.mean)) for k in range(len(qs))]
            s["abs_quantile_bias_max"] = [_jsonable(stat(bias[:, k], np.max)) for k in range(len(qs))]
            for name, m in (("w1", self.w1()), ("ks", self.ks())):
                s[f"{name}_mean"], s[f"{name}_max"] = _jsonable(stat(m, np.mean)), _jsonable(stat(m, np.max))
                worst = [int(np.nanargmax(r)) if np.isfinite(r).any() else None for r in flat(m)]
                s[f"{name}_worst_pixel"] = [None if p is None else [p // self.W, p % self.W] for p in worst]
        return s

    def save(self, directory, q=(0.5, 0.95, 0.99)):
        """One ``<name>.npy`` per map plus ``summary.json`` under ``directory`` (created); returns the file names."""
        os.makedirs(directory, exist_ok=True)
        names = []
        for k, a in self.maps(q).items():
            np.save(os.path.join(directory, k + ".npy"), a)
            names.append(k + ".npy")
        with open(os.path.join(directory, "summary.json"), "w") as f:
            json.dump(self.summary(q), f, indent=1)
        return names + ["summary.json"]


class GridHist:
    """Running per-pixel histograms of the fields added so far on an H x W grid; the table stays on the device (``reduce_``:
    one int32 all-reduce of the table plus the field count under data parallelism).  ``nbytes``: the size of the table,
    nout * S * (bins + 3) * H * W * 4 (1.6 GB for nout = 3, S = 2, bins = 64 on 1024 x 1024; 26 MB on 128 x 128)."""

    def __init__(self, spec, H, W, paired=True, device="cuda:0", ops=None):
        _check_spec(spec)
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"GridHist needs a grid of 1 <= H * W < 2^31 pixels (got {H} x {W})")
        self.spec, self.H, self.W, self.paired = spec, H, W, bool(paired)
        self.device = torch.device(device)
        self._ops = ops
        n = spec.nout * (2 if self.paired else 1) * (spec.bins + 3) * H * W
        self._buf = torch.zeros(n + 1, dtype=torch.int32, device=self.device)        # the last entry: fields added
        self._added = 0                                              # this rank's fields (host mirror: no sync in add)
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def counts(self):
        return self._buf[:-1].view(self.spec.nout, 2 if self.paired else 1, self.spec.bins + 3, self.H * self.W)

    @property
    def fields(self):
        return int(self._buf[-1].item())

    @property
    def nbytes(self):
        return (self._buf.numel() - 1) * 4

    def add(self, real, fake=None, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) fields of a batch: ``real`` alone, or the pair (real, fake) when this
        accumulator is paired.  Layouts as ``gridstats.GridStats.add`` ([T, C, H, W]; with ``nhwc`` a [T, H, W, c_pad] store
        of which the leading ``channels`` are read; a ``NativeBatch``); the two series may differ in layout and dtype: pass
        ``nhwc`` as a pair (real, fake) then."""
        if self.paired != (fake is not None):
            raise ValueError("a paired GridHist takes (real, fake)" if self.paired else "this GridHist takes one series (paired=False)")
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "gridhist", self.spec, "GridHist", (self.H, self.W))
        if self._added + n >= FIELDS_MAX:
            raise ValueError(f"GridHist holds fewer than 2^26 fields: {self._added} + {n} would reach 2^26, where the scan's int64 sum "
                             "2 (bins + 1) n^2 reaches 2^63 (the table itself counts in int32)")
        if self._struct is None:
            self._struct = self.spec.struct()
        ka, fa = fields.descriptor(self.ops, a.x[:n], a.nhwc, a.C)
        kb, fb = fields.descriptor(self.ops, b.x[:n], b.nhwc, b.C) if self.paired else (None, None)
        self.ops.gridhist(fa, fb, self._struct, self.counts)
        self._buf[-1] += n
        self._added += n
        return self

    def reduce_(self, dist):
        """Sum the table and the field count over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in
        place: one int32 all-reduce."""
        if dist is not None and dist.world_size > 1:
            dist.allreduce_sum_(self._buf)
            if self.fields >= FIELDS_MAX or self.fields < 0:
                raise ValueError(f"GridHist holds fewer than 2^26 fields: the ranks hold {self.fields} together, which would reach 2^26, "
                                 "where the scan's int64 sum 2 (bins + 1) n^2 reaches 2^63 (the table itself counts in int32)")
        return self

    def result(self):
        """The ``GridHistMaps`` of every field added (and, after ``reduce_``, of every rank)."""
        return GridHistMaps(self.spec, self.H, self.W, self.paired, self.counts.clone(), self.fields, ops=self._ops)


def gridhist(real, fake=None, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """Per-gridpoint histograms of one series of fields, or of a (real, fake) pair, on the GPU -> ``GridHistMaps``.  spec None:
    ``HistSpec.zscore(C, bins=64, lim=6.0)`` of the fields' channels; the other arguments as ``GridHist.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "gridhist")
    if spec is None:
        spec = HistSpec.zscore(Cn, bins=64, lim=6.0)
    _check_spec(spec)
    acc = GridHist(spec, H, W, paired=fake is not None, device=device, ops=ops)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
