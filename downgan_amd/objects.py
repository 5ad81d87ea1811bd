"""Object-based verification of real against generated fields, computed on the GPU (csrc/objects.hip).

Every other diagnostic of this package treats a field as a bag of pixels or of Fourier modes.  This one knows that the pixels
above a storm threshold form things: a gust front, a lee jet and a convective cell are single features, each with an area, a
mass, a peak and a place.  For output channel j of an ``ObjectSpec`` (the transform of ``histograms`` / ``fss``, the same device
code) and threshold k, an OBJECT is a connected component (connectivity 4 or 8) of the mask y > thr[j][k]; the device labels
all planes of a batch by lock-free union-find and returns one exact integer record per object:

    [plane, root, area, overlap, mass, sum_qh, sum_qw, qmax, h0, h1, w0, w1]            (include/downgan_hip.h)

with q = clamp(rint(y / quantum), 0, 2^24 - 1) the fixed-point intensity of a pixel, mass = sum q, and overlap the number of the
object's pixels that are also above the threshold on the other side.  ``Objects`` pools the records of every batch on the host at
once -- object counts, area and mass distributions in log2 bins, the largest object, fields without any object, matched objects
-- as exact integers, sums them exactly over data-parallel ranks, and the trainer's opt-in hook (``WassersteinGAN.log_objects``)
keeps one per part.  ``ObjectsResult`` forms objects per field, mean areas, the per-object POD / FAR / CSI and the SAL score.

SAL (structure, amplitude, location; Wernli et al. 2008) is computed in its THRESHOLDED variant: every term, the amplitude A
included, comes from the objects above the threshold only (the original A uses the domain mean of the whole field).  The objects
counted are those with area >= min_area and mass > 0.  With R_n the mass of object n, R = sum R_n, the centre of mass
xbar = (sum sum_qh, sum sum_qw) / R, x_n = (sum_qh_n, sum_qw_n) / R_n, the scaled volume V = sum R_n (R_n / qmax_n) / R, the spread
r = sum R_n |x_n - xbar| / R and d = hypot(H - 1, W - 1), for a = real and b = generated:

    A = (R_b - R_a) / ((R_a + R_b) / 2)        S = (V_b - V_a) / ((V_a + V_b) / 2)
    L1 = |xbar_b - xbar_a| / d                 L2 = 2 |r_b - r_a| / d                 L = L1 + L2

per field pair and (j, k), in float64.  A pair is defined only when both sides have R > 0; the others are counted by kind.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib, fields
from .fss import allreduce_ints
from .gridstats import _jsonable
from .histograms import C_MAX, _default_ops, _f32

THR_MAX, SIDE_MAX, COLS = _lib.OBJ_MAX_THR, _lib.OBJ_MAX_SIDE, _lib.OBJ_COLS
WS_CAP = 512 << 20           # bytes of dg_objects workspace at most: a batch is cut into chunks of fields (at least one)
SLOT_LIMIT = 1 << 31         # T 2 nout nthr ceil(P / 2) of one call stays below this (the library rejects more)
AREA_BINS = 23               # floor(log2(area)) of an area <= 2^22
MASS_BINS = 47               # row 0: mass == 0; row 1 + floor(log2(mass)) of a mass < 2^46
SIDES = ("real", "fake")
PLANE, ROOT, AREA, OVERLAP, MASS, SUM_QH, SUM_QW, QMAX, H0, H1, W0, W1 = range(12)
SAL_TERMS = ("S", "A", "L1", "L2")
UNDEFINED = ("real_only", "fake_only", "neither")


class ObjectSpec:
    """Units, thresholds, connectivity and intensity quantum of the exceedance objects of C input channels (+ the speed of a pair
    of them, appended as the last output).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None;
    thresholds: 1 .. THR_MAX values per output channel -- one list per output channel, or one list of numbers for all --
    rounded to fp32; connectivity: 4 (edge neighbours) or 8 (corner neighbours too); quantum: the intensity step, q =
    rint(y / quantum) (the device multiplies by fp32(1 / quantum)); min_area: objects below it are dropped from every pooled
    statistic; names: one per output channel."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), thresholds=(), connectivity=8, quantum=2.0 ** -10, min_area=1,
                 names=None):
        if not (isinstance(C, (int, np.integer)) and 1 <= C <= C_MAX):
            raise ValueError(f"objects takes 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"objects speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"objects scale and offset need one value per input channel (C = {self.C})")
        thr = list(thresholds)
        if all(np.ndim(t) == 0 for t in thr):
            thr = [thr] * self.nout                                  # one list for every channel
        if len(thr) != self.nout or len({len(t) for t in thr}) != 1:
            raise ValueError(f"objects thresholds need one list per output channel ({self.nout}), all of one length")
        K = len(thr[0])
        if not 1 <= K <= THR_MAX:
            raise ValueError(f"objects takes 1 to {THR_MAX} thresholds per channel (got {K})")
        self.thresholds = np.stack([_f32(t, "thresholds") for t in thr])
        self.K = K
        if connectivity not in (4, 8):
            raise ValueError(f"objects connectivity is 4 or 8 (got {connectivity!r})")
        self.connectivity = int(connectivity)
        if not (isinstance(quantum, (int, float, np.integer, np.floating)) and math.isfinite(quantum) and quantum > 0):
            raise ValueError(f"objects quantum must be a finite positive number (got {quantum!r})")
        with np.errstate(over="ignore"):
            inv = np.float32(1.0 / float(quantum))
        if not (np.isfinite(inv) and inv > 0):
            raise ValueError(f"objects quantum must have a finite positive inverse in fp32 (got {quantum!r})")
        self.quantum, self.inv_quantum = float(quantum), inv
        if not (isinstance(min_area, (int, np.integer)) and min_area >= 1):
            raise ValueError(f"objects min_area must be an integer >= 1 (got {min_area!r})")
        self.min_area = int(min_area)
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"objects names need one entry per output channel ({self.nout})")

    @classmethod
    def zscore(cls, C, thresholds=(1.0, 2.0), connectivity=8, quantum=2.0 ** -10, min_area=1):
        """Standardised fields: the speed of channels (0, 1) when C >= 2, the same thresholds in every channel."""
        return cls(C, speed=(0, 1) if C >= 2 else None, thresholds=thresholds, connectivity=connectivity, quantum=quantum,
                   min_area=min_area)

    @classmethod
    def physical(cls, stats, order, thresholds, connectivity=8, quantum=2.0 ** -10, min_area=1, speed=("u10", "v10")):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, evaluated
        in physical units (y = x * std + mean).  thresholds and quantum: in physical units; speed: the names of the (u, v) pair,
        or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        names = order + (["speed"] if sp else [])
        return cls(len(order), scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp,
                   thresholds=thresholds, connectivity=connectivity, quantum=quantum, min_area=min_area, names=names)

    def struct(self):
        """The dg_objects_spec of this spec (no library call)."""
        s = _lib.ObjectsSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nthr, s.connectivity, s.inv_quantum = self.K, self.connectivity, float(self.inv_quantum)
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            for k in range(self.K):
                s.thr[j][k] = float(self.thresholds[j, k])
        return s

    def __eq__(self, other):
        return (isinstance(other, ObjectSpec) and self.C == other.C and self.speed == other.speed
                and (self.connectivity, self.min_area, float(self.inv_quantum)) == (other.connectivity, other.min_area, float(other.inv_quantum))
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("scale", "offset", "thresholds")))

    __hash__ = None


def _host_table(s, C, a, b=None, capacity=None):
    """host_objects for a dg_objects_spec ``s`` of C input channels."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[0] != C:
        raise ValueError(f"host_objects takes [C = {C}, H, W] values (got shape {a.shape})")
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32)
        if b.shape != a.shape:
            raise ValueError(f"host_objects needs both fields of one shape (got {a.shape} and {b.shape})")
    _, H, W = a.shape
    nout = C + (1 if s.speed_u >= 0 else 0)
    count = np.zeros(1, np.int64)
    per_plane = np.zeros((2, nout, max(1, min(s.nthr, THR_MAX))), np.int64)
    run = lambda table, cap: _lib.check(_lib.lib().dg_objects_host(
        ctypes.byref(s), a.ctypes.data, None if b is None else b.ctypes.data, C, H, W, table.ctypes.data if cap else None, cap,
        count.ctypes.data, per_plane.ctypes.data), "dg_objects_host")
    if capacity is None:
        run(np.zeros((0, COLS), np.int64), 0)
        capacity = int(count[0])
    table = np.zeros((int(capacity), COLS), np.int64)
    run(table, int(capacity))
    return table[:min(int(count[0]), int(capacity))], int(count[0]), per_plane


def host_objects(spec, a, b=None, capacity=None):
    """(table int64 [min(count, capacity), 12] sorted by (plane, root), count, per_plane int64 [2, nout, K]) of one field ``a``
    (fp32 [C, H, W]) or one field pair, computed by the library on the host (dg_objects_host, a plain flood fill: the definition
    the kernels are tested against).  capacity None: as many rows as there are objects."""
    return _host_table(spec.struct(), spec.C, a, b, capacity)


class HostOps:
    """The operations ``Objects`` needs, served by the library's host reference (dg_objects_host) on CPU tensors: an explicit
    reference path for tests, tools and machines without a GPU, never chosen by default."""

    device = torch.device("cpu")

    class _Fields:
        def __init__(self, x):
            self.x = x
            self.T, self.C, self.P = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]

    def eof_fields(self, x, nhwc=False, channels=None):
        x = x.detach().to(torch.float32)
        x = x[..., :channels].permute(0, 3, 1, 2) if nhwc else x
        return self._Fields(np.ascontiguousarray(x.numpy()))

    def objects_ws_bytes(self, f, H, W, spec):
        return 256 + 8 * f.T * 2 * (f.C + (spec.speed_u >= 0)) * spec.nthr * f.P

    def objects(self, fa, fb, H, W, spec, capacity=None):
        njk2 = 2 * (fa.C + (spec.speed_u >= 0)) * spec.nthr
        tables, planes = [], []
        for t in range(fa.T):
            tab, _, pp = _host_table(spec, fa.C, fa.x[t], None if fb is None else fb.x[t])
            tab = tab.copy()
            tab[:, PLANE] += t * njk2
            tables.append(tab)
            planes.append(pp.reshape(-1))
        return torch.from_numpy(np.concatenate(tables)), torch.from_numpy(np.concatenate(planes)), 1


def _log2_bin(v):
    """floor(log2(v)) of positive int64 values, exact (the exponent of the float64, exact below 2^53)."""
    return np.frexp(v.astype(np.float64))[1] - 1


def sal_terms(cols, nplanes):
    """(R, V, xh, xw, r) float64 [nplanes] of the records ``cols`` (int64 [12, n], one row per column of the table, mass > 0)
    grouped by plane: total mass, scaled volume, centre of mass and spread of every plane (V, xh, xw, r NaN where R = 0)."""
    plane = cols[PLANE]
    m, qh, qw = (cols[i].astype(np.float64) for i in (MASS, SUM_QH, SUM_QW))
    R = np.bincount(plane, weights=m, minlength=nplanes)
    sh = np.bincount(plane, weights=qh, minlength=nplanes)
    sw = np.bincount(plane, weights=qw, minlength=nplanes)
    with np.errstate(invalid="ignore", divide="ignore"):
        V = np.bincount(plane, weights=m * (m / cols[QMAX].astype(np.float64)), minlength=nplanes) / R
        xh, xw = sh / R, sw / R
        dist = np.hypot(qh / m - xh[plane], qw / m - xw[plane])
        r = np.bincount(plane, weights=m * dist, minlength=nplanes) / R
    return R, V, xh, xw, r


class ObjectsResult:
    """The pooled object statistics of one ObjectSpec on an H x W grid over ``fields`` fields (field pairs when paired): exact
    integers per (side, output channel, threshold) and the SAL terms of every defined pair."""

    def __init__(self, spec, H, W, paired, fields, tables, sal, undefined, sal_pairs, records=None):
        self.spec, self.H, self.W, self.paired, self.fields = spec, int(H), int(W), bool(paired), int(fields)
        self._t = {k: np.array(v, dtype=np.int64) for k, v in tables.items()}
        self._sal = np.array(sal, dtype=np.float64)                  # [nout, K, 9]: sums of S A L1 L2 L |S| |A| |L|, pairs
        self._undefined = np.array(undefined, dtype=np.int64)        # [nout, K, 3]
        self._pairs = sal_pairs                                      # float64 [pairs, nout, K, 4], NaN where undefined (this rank's)
        self.records = records                                       # with keep_records: int64 [n, 13]: the field, then the record with plane = (side nout + j) K + k

    def counts(self):
        """int64 [sides, nout, K]: the number of objects."""
        return self._t["count"].copy()

    def objects_per_field(self):
        """float64 [sides, nout, K]: objects per field."""
        return self._t["count"] / self.fields if self.fields else np.full(self._t["count"].shape, np.nan)

    def area_histogram(self):
        """(count, area) int64 [sides, nout, K, 23]: the objects and their total area per floor(log2(area)) bin."""
        return self._t["area_count"].copy(), self._t["area_sum"].copy()

    def mass_histogram(self):
        """int64 [sides, nout, K, 47]: the objects per mass bin; column 0 is mass == 0, column 1 + floor(log2(mass)) the rest."""
        return self._t["mass_count"].copy()

    def mean_area(self):
        """float64 [sides, nout, K]: pixels per object (NaN without objects)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._t["area_sum"].sum(-1) / self._t["count"]

    def max_area(self):
        return self._t["max_area"].copy()

    def empty_fields(self):
        """int64 [sides, nout, K]: fields with no object."""
        return self._t["empty"].copy()

    def matched(self):
        """int64 [sides, nout, K]: objects that share a pixel with the other side's mask (zeros when unpaired)."""
        return self._t["matched"].copy()

    def _score(self, num, den):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(den > 0, num / np.where(den > 0, den, 1), np.nan)

    def _need_pair(self, what):
        if not self.paired:
            raise ValueError(f"{what} needs real and generated fields (this accumulator was fed one series)")

    def pod(self):
        """float64 [nout, K]: matched real objects / real objects (probability of detection; NaN without real objects)."""
        self._need_pair("pod")
        return self._score(self._t["matched"][0], self._t["count"][0])

    def far(self):
        """float64 [nout, K]: unmatched generated objects / generated objects (false-alarm ratio)."""
        self._need_pair("far")
        return self._score(self._t["count"][1] - self._t["matched"][1], self._t["count"][1])

    def csi(self):
        """float64 [nout, K]: hits / (hits + misses + false alarms) with hits = matched real, misses = unmatched real, false
        alarms = unmatched generated objects."""
        self._need_pair("csi")
        hits = self._t["matched"][0]
        return self._score(hits, self._t["count"][0] + self._t["count"][1] - self._t["matched"][1])

    def sal(self):
        """{"S", "A", "L1", "L2", "L", "abs_S", "abs_A", "abs_L": float64 [nout, K] means over the defined pairs (NaN without
        one), "pairs": int64 [nout, K]}."""
        self._need_pair("sal")
        n = self._sal[..., 8]
        out = {k: self._score(self._sal[..., i], n) for i, k in enumerate(("S", "A", "L1", "L2", "L", "abs_S", "abs_A", "abs_L"))}
        out["pairs"] = n.astype(np.int64)
        return out

    def sal_undefined(self):
        """int64 [nout, K, 3]: the pairs without a SAL -- objects on the real side only, on the generated side only, on neither."""
        self._need_pair("sal_undefined")
        return self._undefined.copy()

    def sal_pairs(self):
        """{"S", "A", "L1", "L2": float64 [pairs, nout, K]} of every pair this process added, in the order added (NaN where
        undefined; not gathered over ranks)."""
        self._need_pair("sal_pairs")
        return {k: self._pairs[..., i].copy() for i, k in enumerate(SAL_TERMS)}

    def summary(self):
        """A JSON-serialisable dict (None where undefined); the exact integers are kept as integers."""
        ints = lambda a: np.asarray(a).tolist()
        sides = SIDES[:2 if self.paired else 1]
        d = {"channels": list(self.spec.names), "fields": self.fields, "grid": [self.H, self.W],
             "thresholds": _jsonable(self.spec.thresholds), "connectivity": self.spec.connectivity, "quantum": self.spec.quantum,
             "min_area": self.spec.min_area}
        for name, key in (("count", "count"), ("area_count", "area_count"), ("area_sum", "area_sum"), ("mass_count", "mass_count"),
                          ("max_area", "max_area"), ("empty_fields", "empty"), ("matched", "matched")):
            d[name] = {s: ints(self._t[key][i]) for i, s in enumerate(sides)}
        d["objects_per_field"] = {s: _jsonable(self.objects_per_field()[i]) for i, s in enumerate(sides)}
        d["mean_area"] = {s: _jsonable(self.mean_area()[i]) for i, s in enumerate(sides)}
        if self.paired:
            d["pod"], d["far"], d["csi"] = _jsonable(self.pod()), _jsonable(self.far()), _jsonable(self.csi())
            sal = self.sal()
            d["sal"] = {k: (ints(v) if k == "pairs" else _jsonable(v)) for k, v in sal.items()}
            d["sal_undefined"] = {k: ints(self._undefined[..., i]) for i, k in enumerate(UNDEFINED)}
        return d


class Objects:
    """Running object statistics of the fields (paired: the (real, generated) field pairs) added so far on an H x W grid.  The
    device returns the records of a chunk of fields; they are pooled on the host at once and dropped, unless ``keep_records``."""

    TABLES = (("count", ()), ("area_count", (AREA_BINS,)), ("area_sum", (AREA_BINS,)), ("mass_count", (MASS_BINS,)), ("max_area", ()),
              ("empty", ()), ("matched", ()))

    def __init__(self, spec, H, W, paired=True, device=None, ops=None, keep_records=False):
        if not isinstance(spec, ObjectSpec):
            raise TypeError(f"Objects takes an ObjectSpec (got {type(spec).__name__})")
        H, W = int(H), int(W)
        if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
            raise ValueError(f"Objects needs a grid of 1 <= H, W <= {SIDE_MAX} (got {H} x {W})")
        self.spec, self.H, self.W, self.paired = spec, H, W, bool(paired)
        self.device = torch.device(ops.device if ops is not None and device is None else "cuda:0" if device is None else device)
        self._ops = ops
        self.keep_records = bool(keep_records)
        ns = 2 if self.paired else 1
        self._t = {k: np.zeros((ns, spec.nout, spec.K) + tail, np.int64) for k, tail in self.TABLES}
        self._sal = np.zeros((spec.nout, spec.K, 9), np.float64)
        self._undefined = np.zeros((spec.nout, spec.K, 3), np.int64)
        self._pairs = []
        self._records = []
        self.fields = 0
        self.calls = 0                                               # dg_objects calls, repeats after a table growth included
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    def _pool(self, rec, m):
        """Pool the sorted records int64 [n, 12] of a chunk of ``m`` fields."""
        sp, ns = self.spec, 2 if self.paired else 1
        nout, K = sp.nout, sp.K
        if self.keep_records:
            kept = np.concatenate([(rec[:, :1] // (2 * nout * K)) + self.fields, rec], axis=1)
            kept[:, 1] %= 2 * nout * K                               # the plane without the field: (side nout + j) K + k
            self._records.append(kept)
        if sp.min_area > 1:
            rec = rec[rec[:, AREA] >= sp.min_area]
        c = np.ascontiguousarray(rec.T)                              # one contiguous row per column of the table
        plane, area, mass = c[PLANE], c[AREA], c[MASS]
        sjk = plane % (2 * nout * K)                                 # (side, j, k)
        n3 = 2 * nout * K
        tab = lambda v: v.reshape((2, nout, K) + v.shape[1:])[:ns]
        t = self._t
        t["count"] += tab(np.bincount(sjk, minlength=n3))
        ab = sjk * AREA_BINS + _log2_bin(area)
        t["area_count"] += tab(np.bincount(ab, minlength=n3 * AREA_BINS).reshape(n3, AREA_BINS))
        # float64 weights are exact here: a bin's total area stays below the pixels of the chunk, far below 2^53
        asum = np.bincount(ab, weights=area.astype(np.float64), minlength=n3 * AREA_BINS).astype(np.int64)
        t["area_sum"] += tab(asum.reshape(n3, AREA_BINS))
        mb = np.where(mass > 0, 1 + _log2_bin(np.maximum(mass, 1)), 0)
        t["mass_count"] += tab(np.bincount(sjk * MASS_BINS + mb, minlength=n3 * MASS_BINS).reshape(n3, MASS_BINS))
        big = np.array([area[sjk == g].max(initial=0) for g in range(n3)], np.int64)
        t["max_area"] = np.maximum(t["max_area"], tab(big))
        per_plane = np.bincount(plane, minlength=m * n3).reshape(m, n3)
        t["empty"] += tab((per_plane == 0).sum(0))
        t["matched"] += tab(np.bincount(sjk[c[OVERLAP] > 0], minlength=n3))
        if not self.paired:
            return
        heavy = c if mass.all() else np.ascontiguousarray(c[:, mass > 0])
        R, V, xh, xw, r = (v.reshape(m, 2, nout, K) for v in sal_terms(heavy, m * n3))
        both = (R[:, 0] > 0) & (R[:, 1] > 0)
        d = math.hypot(self.H - 1, self.W - 1)
        pairs = np.full((m, nout, K, 4), np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            pairs[..., 0] = (V[:, 1] - V[:, 0]) / (0.5 * (V[:, 0] + V[:, 1]))
            pairs[..., 1] = (R[:, 1] - R[:, 0]) / (0.5 * (R[:, 0] + R[:, 1]))
            pairs[..., 2] = np.hypot(xh[:, 1] - xh[:, 0], xw[:, 1] - xw[:, 0]) / d if d > 0 else 0.0
            pairs[..., 3] = 2.0 * np.abs(r[:, 1] - r[:, 0]) / d if d > 0 else 0.0
        pairs[~both] = np.nan
        self._pairs.append(pairs)
        z = np.where(both[..., None], pairs, 0.0)
        L = z[..., 2] + z[..., 3]
        for i, v in enumerate((z[..., 0], z[..., 1], z[..., 2], z[..., 3], L, np.abs(z[..., 0]), np.abs(z[..., 1]), np.abs(L), both)):
            self._sal[..., i] += v.sum(0)
        has = R > 0
        for i, v in enumerate((has[:, 0] & ~has[:, 1], ~has[:, 0] & has[:, 1], ~has[:, 0] & ~has[:, 1])):
            self._undefined[..., i] += v.sum(0)

    def add(self, real, fake=None, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) fields / field pairs of a batch.  Layouts as ``fss.FractionsSkill.add``
        ([T, C, H, W]; with ``nhwc`` a [T, H, W, c_pad] store of which the leading ``channels`` are read; a ``NativeBatch``);
        the two series may differ in layout and dtype: pass ``nhwc`` as a pair (real, fake) then.  Every dg_objects call ends
        with one synchronising copy of its object count; a table that was too small is grown and the call repeated."""
        if (fake is not None) != self.paired:
            raise ValueError("a paired Objects takes (real, fake), an unpaired one real alone")
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "objects", self.spec, "Objects", (self.H, self.W))
        if self._struct is None:
            self._struct = self.spec.struct()
        o = self.ops
        _, f1 = fields.descriptor(o, a.x[:1], a.nhwc, a.C)
        per_field = max(1, o.objects_ws_bytes(f1, self.H, self.W, self._struct))
        most = 2 * self.spec.nout * self.spec.K * ((self.H * self.W + 1) // 2)       # objects of one field at most
        tc = max(1, min(n, WS_CAP // per_field, (SLOT_LIMIT - 1) // most))
        for t0 in range(0, n, tc):
            m = min(tc, n - t0)
            ka, fa = fields.descriptor(o, a.x[t0:t0 + m], a.nhwc, a.C)
            fb = None
            if self.paired:
                kb, fb = fields.descriptor(o, b.x[t0:t0 + m], b.nhwc, b.C)
            table, _, calls = o.objects(fa, fb, self.H, self.W, self._struct)
            self.calls += calls
            self._pool(table.cpu().numpy(), m)
            self.fields += m
        return self

    def reduce_(self, dist):
        """Sum the pooled tables over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place: the integer
        tables exactly (fss.allreduce_ints; the largest area by a max), the SAL sums and pair counts with one ordinary float64
        all-reduce.  Those float sums agree from run to run at one world size, but not across world sizes (the order of the
        additions differs).  ``sal_pairs`` and kept records stay this rank's."""
        if dist is not None and dist.world_size > 1:
            dev = self.device if getattr(dist, "backend", "gloo") == "nccl" else "cpu"
            keys = [k for k, _ in self.TABLES if k != "max_area"]
            flat = np.concatenate([self._t[k].reshape(-1) for k in keys] + [self._undefined.reshape(-1), [self.fields]])
            vals = np.array(allreduce_ints(dist, flat.tolist(), dev), dtype=np.int64)
            off = 0
            for k in keys:
                n = self._t[k].size
                self._t[k] = vals[off:off + n].reshape(self._t[k].shape)
                off += n
            self._undefined = vals[off:off + self._undefined.size].reshape(self._undefined.shape)
            self.fields = int(vals[-1])
            big = self._t["max_area"].reshape(-1)                    # <= 2^22: exact in float64
            mm = torch.from_numpy(np.stack([big, big], axis=1).astype(np.float64).reshape(1, -1)).to(dev)
            dist.minmax_(mm, big.size)
            self._t["max_area"] = mm.cpu().numpy().reshape(-1, 2)[:, 1].astype(np.int64).reshape(self._t["max_area"].shape)
            s = torch.from_numpy(self._sal.reshape(-1).copy()).to(dev)
            dist.allreduce_sum_(s)
            self._sal = s.cpu().numpy().reshape(self._sal.shape)
        return self

    def result(self):
        """The ``ObjectsResult`` of everything added (and, after ``reduce_``, of every rank)."""
        sp = self.spec
        pairs = np.concatenate(self._pairs) if self._pairs else np.zeros((0, sp.nout, sp.K, 4))
        records = (np.concatenate(self._records) if self._records else np.zeros((0, COLS + 1), np.int64)) if self.keep_records else None
        return ObjectsResult(sp, self.H, self.W, self.paired, self.fields, self._t, self._sal, self._undefined, pairs, records)


def objects(real, fake=None, spec=None, n_valid=None, nhwc=False, channels=None, ops=None, keep_records=False):
    """Object statistics of a series of fields, or of a (real, generated) pair of series, on the GPU -> ``ObjectsResult``.  spec
    None: ``ObjectSpec.zscore`` of the fields' channels; the other arguments as ``Objects.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "objects")
    if spec is None:
        spec = ObjectSpec.zscore(Cn)
    if not isinstance(spec, ObjectSpec):
        raise TypeError(f"objects takes an ObjectSpec (got {type(spec).__name__})")
    acc = Objects(spec, H, W, paired=fake is not None, device=device, ops=ops, keep_records=keep_records)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
