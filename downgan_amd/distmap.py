"""Distance-map verification of real against generated fields, computed on the GPU (csrc/distmap.hip).

How far from a real exceedance does the generator put its exceedances, in pixels?  ``fss`` tells at which window size the
fractions agree, SAL's L compares centres of mass (a generator that scatters gust cells symmetrically round the true front gets
L = 0); the distance measures of binary fields give the displacement itself.  For output channel j of a ``DistSpec`` (the
transform of ``histograms`` / ``fss`` / ``objects``, the same device code) and threshold k, A is the mask y > thr[j][k] of the real
field and B that of the generated one; the device computes the exact squared Euclidean distance transform d2 of both masks
(``distance_transform`` returns it on its own) and one exact integer record per field pair:

    [n_a, n_b, n_ab, sum_dq_b2a, sum_d2_b2a, max_d2_b2a, sum_dq_a2b, sum_d2_a2b, max_d2_a2b, bad1, bad2]   (include/downgan_hip.h)

with dq = floor(1024 sqrt(d2)) the fixed-point distance, b2a the pixels of B measured against A (generated -> real: the false
alarm distance), a2b the pixels of A against B (the miss distance), and bad1 / bad2 the sums of |w_A - w_B| and (w_A - w_B)^2
over all pixels, w = min(dq, 1024 cutoff): Baddeley's Delta with p = 1, 2 and the cutoff transform, defined also when a side is
empty.  Next to the records the device counts the pixels of either side by ring = ceil(distance to the other side): the ring
table, whose CDF says "90 % of the generated storm pixels lie within 3 px of a real one".  ``Distances`` pools the records on the
host as Python integers, sums them exactly over data-parallel ranks, and the trainer's opt-in hook
(``WassersteinGAN.log_distances``) keeps one per part.  ``DistanceResult`` forms the mean error distances, the Hausdorff distance,
Baddeley's Delta and the displacement quantiles (the pooled partial Hausdorff distance).
"""
from __future__ import annotations

import ctypes
import json
import math
import os

import numpy as np
import torch

from . import _lib, fields
from .fss import allreduce_ints
from .gridstats import _jsonable
from .histograms import C_MAX, _default_ops, _f32

THR_MAX, SIDE_MAX, RINGS_MAX, CUTOFF_MAX, COLS, FAR = (_lib.DIST_MAX_THR, _lib.DIST_MAX_SIDE, _lib.DIST_MAX_RINGS,
                                                       _lib.DIST_MAX_CUTOFF, _lib.DIST_COLS, _lib.DIST_FAR)
WS_CAP = 512 << 20           # bytes of dg_distmap workspace (and d2 output) at most: a batch is cut into chunks of fields (at least one)
N_A, N_B, N_AB, SUM_DQ_B2A, SUM_D2_B2A, MAX_D2_B2A, SUM_DQ_A2B, SUM_D2_A2B, MAX_D2_A2B, BAD1, BAD2 = range(11)
KINDS = ("both", "real_only", "fake_only", "neither")
DIRECTIONS = ("fake_to_real", "real_to_fake")
# the pooled sums of one (j, k): the pairs by kind, then over the pairs of kind "both" the pixels and distance sums of either
# direction, then over all pairs the Baddeley sums and the pixel counts
POOLED = KINDS + ("n_b_both", "sum_dq_b2a", "sum_d2_b2a", "n_a_both", "sum_dq_a2b", "sum_d2_a2b", "bad1", "bad2", "n_a", "n_b", "n_ab")


class DistSpec:
    """Units, thresholds, Baddeley cutoff and ring count of the distance maps of C input channels (+ the speed of a pair of them,
    appended as the last output).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None;
    thresholds: 1 .. THR_MAX values per output channel -- one list per output channel, or one list of numbers for all --
    rounded to fp32; cutoff: the cap of Baddeley's distance transform in pixels (1 .. CUTOFF_MAX); nring: the rings of the
    ring table (1 .. RINGS_MAX; farther pixels share one bin); names: one per output channel."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), thresholds=(), cutoff=32, nring=64, names=None):
        if not (isinstance(C, (int, np.integer)) and 1 <= C <= C_MAX):
            raise ValueError(f"distmap takes 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"distmap speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"distmap scale and offset need one value per input channel (C = {self.C})")
        thr = list(thresholds)
        if all(np.ndim(t) == 0 for t in thr):
            thr = [thr] * self.nout                                  # one list for every channel
        if len(thr) != self.nout or len({len(t) for t in thr}) != 1:
            raise ValueError(f"distmap thresholds need one list per output channel ({self.nout}), all of one length")
        K = len(thr[0])
        if not 1 <= K <= THR_MAX:
            raise ValueError(f"distmap takes 1 to {THR_MAX} thresholds per channel (got {K})")
        self.thresholds = np.stack([_f32(t, "thresholds") for t in thr])
        self.K = K
        if not (isinstance(cutoff, (int, np.integer)) and 1 <= cutoff <= CUTOFF_MAX):
            raise ValueError(f"distmap cutoff must be an integer in [1, {CUTOFF_MAX}] pixels (got {cutoff!r})")
        self.cutoff = int(cutoff)
        if not (isinstance(nring, (int, np.integer)) and 1 <= nring <= RINGS_MAX):
            raise ValueError(f"distmap nring must be an integer in [1, {RINGS_MAX}] (got {nring!r})")
        self.nring = int(nring)
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"distmap names need one entry per output channel ({self.nout})")

    @classmethod
    def zscore(cls, C, thresholds=(1.0, 2.0), cutoff=32, nring=64):
        """Standardised fields: the speed of channels (0, 1) when C >= 2, the same thresholds in every channel."""
        return cls(C, speed=(0, 1) if C >= 2 else None, thresholds=thresholds, cutoff=cutoff, nring=nring)

    @classmethod
    def physical(cls, stats, order, thresholds, cutoff=32, nring=64, speed=("u10", "v10")):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, evaluated
        in physical units (y = x * std + mean).  thresholds: in physical units; speed: the names of the (u, v) pair, or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        names = order + (["speed"] if sp else [])
        return cls(len(order), scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp,
                   thresholds=thresholds, cutoff=cutoff, nring=nring, names=names)

    def struct(self):
        """The dg_distmap_spec of this spec (no library call)."""
        s = _lib.DistmapSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nthr, s.nring, s.cutoff = self.K, self.nring, self.cutoff
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            for k in range(self.K):
                s.thr[j][k] = float(self.thresholds[j, k])
        return s

    def __eq__(self, other):
        return (isinstance(other, DistSpec) and self.C == other.C and self.speed == other.speed
                and (self.cutoff, self.nring) == (other.cutoff, other.nring)
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("scale", "offset", "thresholds")))

    __hash__ = None


def host_scalars(d2, cutoff=CUTOFF_MAX):
    """(ring, dq, w) of one squared distance 0 <= d2 <= FAR by the library's integer definitions (host side)."""
    ring, dq, w = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.lib().dg_distmap_host_scalars(int(d2), int(cutoff), ctypes.addressof(ring), ctypes.addressof(dq),
                                                  ctypes.addressof(w)), "dg_distmap_host_scalars")
    return ring.value, dq.value, w.value


def _host_call(s, C, a, b=None):
    """host_distmap for a dg_distmap_spec ``s`` of C input channels."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 3 or a.shape[0] != C:
        raise ValueError(f"host_distmap takes [C = {C}, H, W] values (got shape {a.shape})")
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32)
        if b.shape != a.shape:
            raise ValueError(f"host_distmap needs both fields of one shape (got {a.shape} and {b.shape})")
    _, H, W = a.shape
    nout, K = C + (1 if s.speed_u >= 0 else 0), max(1, min(s.nthr, THR_MAX))
    d2 = np.zeros((2, nout, K, H, W), np.int32)
    if b is None:
        _lib.check(_lib.lib().dg_distmap_host(ctypes.byref(s), a.ctypes.data, None, C, H, W, None, None, d2.ctypes.data),
                   "dg_distmap_host")
        return d2[0]
    records = np.zeros((nout, K, COLS), np.int64)
    rings = np.zeros((nout, K, 2, max(1, min(s.nring, RINGS_MAX)) + 2), np.int64)
    _lib.check(_lib.lib().dg_distmap_host(ctypes.byref(s), a.ctypes.data, b.ctypes.data, C, H, W, records.ctypes.data,
                                          rings.ctypes.data, d2.ctypes.data), "dg_distmap_host")
    return records, rings, d2


def host_distmap(spec, a, b=None):
    """The library's host reference (dg_distmap_host: the definition the kernels are tested against) on one field ``a`` (fp32
    [C, H, W]) -> d2 int32 [nout, K, H, W]; on one field pair -> (records int64 [nout, K, 11], rings int64 [nout, K, 2,
    nring + 2], d2 int32 [2, nout, K, H, W])."""
    return _host_call(spec.struct(), spec.C, a, b)


class HostOps:
    """The operations ``Distances`` and ``distance_transform`` need, served by the library's host reference (dg_distmap_host) on
    CPU tensors: an explicit reference path for tests, tools and machines without a GPU, never chosen by default."""

    device = torch.device("cpu")

    class _Fields:
        def __init__(self, x):
            self.x = x
            self.T, self.C, self.P = x.shape[0], x.shape[1], x.shape[2] * x.shape[3]

    def eof_fields(self, x, nhwc=False, channels=None):
        x = x.detach().to(torch.float32)
        x = x[..., :channels].permute(0, 3, 1, 2) if nhwc else x
        return self._Fields(np.ascontiguousarray(x.numpy()))

    def distmap_ws_bytes(self, f, H, W, spec):
        return 2 * f.T * 2 * (f.C + (spec.speed_u >= 0)) * spec.nthr * f.P

    def distmap(self, fa, fb, H, W, spec, records=None, rings=None, d2=None):
        for t in range(fa.T):
            if fb is None:
                d2[t, 0] = torch.from_numpy(_host_call(spec, fa.C, fa.x[t]).reshape(d2.shape[2:]))
                continue
            rec, ring, d = _host_call(spec, fa.C, fa.x[t], fb.x[t])
            if records is not None:
                records[t] = torch.from_numpy(rec)
            if rings is not None:
                rings += torch.from_numpy(ring)
            if d2 is not None:
                d2[t] = torch.from_numpy(d.reshape(d2.shape[1:]))


def distance_transform(x, spec=None, nhwc=False, channels=None, ops=None):
    """The exact squared Euclidean distance transform of the exceedance masks of a series of fields, on the GPU -> int32 tensor
    [T, nout, K, H, W]: d2 = the squared distance in pixels to the nearest pixel with y > thr[j][k] (0 on the mask; FAR = 2^30
    everywhere where a field has none).  spec None: ``DistSpec.zscore`` of the fields' channels; layouts as ``Distances.add``."""
    x, x_nhwc, Cn, T, H, W = sx = fields.series(x, channels, nhwc, "distmap")
    if spec is None:
        spec = DistSpec.zscore(Cn)
    if not isinstance(spec, DistSpec):
        raise TypeError(f"distance_transform takes a DistSpec (got {type(spec).__name__})")
    fields.agree(sx, spec, "given")
    if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
        raise ValueError(f"distmap needs a grid of 1 <= H, W <= {SIDE_MAX} (got {H} x {W})")
    o = ops if ops is not None else _default_ops(x.device)
    s = spec.struct()
    _, f1 = fields.descriptor(o, x[:1], x_nhwc, Cn)
    per_field = max(1, o.distmap_ws_bytes(f1, H, W, s)) + 8 * spec.nout * spec.K * H * W
    tc = max(1, min(T, WS_CAP // per_field))
    out = torch.empty(T, spec.nout, spec.K, H, W, dtype=torch.int32, device=o.device)
    for t0 in range(0, T, tc):
        m = min(tc, T - t0)
        kx, fx = fields.descriptor(o, x[t0:t0 + m], x_nhwc, Cn)
        d2 = torch.empty(m, 2, spec.nout, spec.K, H * W, dtype=torch.int32, device=o.device)   # the side-1 planes stay unwritten
        o.distmap(fx, None, H, W, s, d2=d2)
        out[t0:t0 + m] = d2[:, 0].view(m, spec.nout, spec.K, H, W)
    return out


def _ratio(num, den):
    """float64 array of the Python integers num / den, NaN where den == 0."""
    return np.array([[n / d if d else math.nan for n, d in zip(rn, rd)] for rn, rd in zip(num, den)], dtype=np.float64)


class DistanceResult:
    """The pooled distance measures of one DistSpec on an H x W grid over ``fields`` field pairs, per (output channel,
    threshold), formed from exact integers."""

    def __init__(self, spec, H, W, fields, sums, rings, hmax, hsum, records=None):
        self.spec, self.H, self.W, self.fields = spec, int(H), int(W), int(fields)
        self._s = {k: [[int(v) for v in row] for row in sums[k]] for k in POOLED}      # Python integers [nout][K]
        self._rings = np.array(rings, dtype=np.int64)                # [nout, K, 2, nring + 2]
        self._hmax = np.array(hmax, dtype=np.int64)                  # [nout, K]: the largest max_d2 of either direction
        self._hsum = np.array(hsum, dtype=np.float64)                # [nout, K]: the sum over the pairs of their Hausdorff distance
        self.records = records                                       # with keep_records: int64 [fields, nout, K, 11] (this rank's)

    def pairs(self):
        """{"both", "real_only", "fake_only", "neither": int64 [nout, K]}: the field pairs by the sides that hold a pixel."""
        return {k: np.array(self._s[k], dtype=np.int64) for k in KINDS}

    def pixels(self):
        """{"real", "fake", "both": Python integers [nout][K]}: the pixels in A, in B and in both, over all pairs."""
        return {"real": self._s["n_a"], "fake": self._s["n_b"], "both": self._s["n_ab"]}

    def med_fake_to_real(self):
        """float64 [nout, K]: the mean distance in px from a generated exceedance pixel to the nearest real one, pooled over the
        pairs where both sides hold a pixel (NaN without one): how far off the false alarms are."""
        return _ratio(self._s["sum_dq_b2a"], self._s["n_b_both"]) / 1024.0

    def med_real_to_fake(self):
        """float64 [nout, K]: the mean distance in px from a real exceedance pixel to the nearest generated one: the misses."""
        return _ratio(self._s["sum_dq_a2b"], self._s["n_a_both"]) / 1024.0

    def med(self):
        """float64 [nout, K]: the symmetric mean error distance, the larger of the two directions."""
        return np.fmax(self.med_fake_to_real(), self.med_real_to_fake())

    def hausdorff(self):
        """{"mean", "max": float64 [nout, K]}: over the pairs of kind "both", sqrt(max(max_d2_b2a, max_d2_a2b)) in px."""
        both = np.array(self._s["both"], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(both > 0, self._hsum / np.where(both > 0, both, 1), np.nan)
        return {"mean": mean, "max": np.where(both > 0, np.sqrt(self._hmax.astype(np.float64)), np.nan)}

    def baddeley1(self):
        """float64 [nout, K]: the mean over all pairs and pixels of |w_A - w_B| in px (Baddeley's Delta with p = 1)."""
        n = self.fields * self.H * self.W
        return _ratio(self._s["bad1"], [[n] * self.spec.K] * self.spec.nout) / 1024.0

    def baddeley2(self):
        """float64 [nout, K]: sqrt of the mean over all pairs and pixels of (w_A - w_B)^2, in px (p = 2)."""
        n = self.fields * self.H * self.W
        return np.sqrt(_ratio(self._s["bad2"], [[n] * self.spec.K] * self.spec.nout)) / 1024.0

    def rings(self):
        """int64 [nout, K, 2, nring + 2]: the ring table (direction 0: generated pixels by their distance to the real mask)."""
        return self._rings.copy()

    def ring_cdf(self, direction):
        """float64 [nout, K, nring]: the share of the matched pixels of one direction ("fake_to_real" / 0, "real_to_fake" / 1)
        within r = 0 .. nring - 1 px of the other side (matched: the other side holds a pixel; NaN without one)."""
        r = self._rings[:, :, _direction(direction)]
        total = r[..., :self.spec.nring + 1].sum(-1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(total > 0, np.cumsum(r[..., :self.spec.nring], -1) / np.where(total > 0, total, 1), np.nan)

    def displacement_quantile(self, q, direction):
        """[nout][K] of the smallest r whose ring CDF reaches q (an int; None past nring - 1 or without matched pixels): the
        pooled partial Hausdorff distance of one direction, rounded up to whole pixels."""
        if not 0.0 < q <= 1.0:
            raise ValueError(f"displacement_quantile takes 0 < q <= 1 (got {q!r})")
        r = self._rings[:, :, _direction(direction)]
        out = []
        for j in range(self.spec.nout):
            row = []
            for k in range(self.spec.K):
                total, cum, found = int(r[j, k, :self.spec.nring + 1].sum()), 0, None
                for i in range(self.spec.nring):
                    cum += int(r[j, k, i])
                    if total and cum >= q * total:
                        found = i
                        break
                row.append(found)
            out.append(row)
        return out

    def summary(self, q=(0.5, 0.9, 0.99)):
        """A JSON-serialisable dict (None where undefined); the exact integers are kept as integers."""
        h = self.hausdorff()
        d = {"channels": list(self.spec.names), "fields": self.fields, "grid": [self.H, self.W],
             "thresholds": _jsonable(self.spec.thresholds), "cutoff": self.spec.cutoff, "nring": self.spec.nring,
             "pairs": {k: self._s[k] for k in KINDS}, "pixels": self.pixels(),
             "med_fake_to_real": _jsonable(self.med_fake_to_real()), "med_real_to_fake": _jsonable(self.med_real_to_fake()),
             "med": _jsonable(self.med()), "hausdorff": {k: _jsonable(v) for k, v in h.items()},
             "baddeley1": _jsonable(self.baddeley1()), "baddeley2": _jsonable(self.baddeley2()),
             "sums": {k: self._s[k] for k in POOLED[4:]}, "rings": self._rings.tolist(),
             "displacement_quantile": {name: {str(v): self.displacement_quantile(v, i) for v in q} for i, name in enumerate(DIRECTIONS)}}
        return d

    def save(self, directory, q=(0.5, 0.9, 0.99)):
        """``rings.npy``, ``ring_cdf_<direction>.npy`` and ``summary.json`` under ``directory`` (created); returns the file names."""
        os.makedirs(directory, exist_ok=True)
        arrays = {"rings": self._rings}
        for name in DIRECTIONS:
            arrays[f"ring_cdf_{name}"] = self.ring_cdf(name)
        names = []
        for k, a in arrays.items():
            np.save(os.path.join(directory, k + ".npy"), a)
            names.append(k + ".npy")
        with open(os.path.join(directory, "summary.json"), "w") as f:
            json.dump(self.summary(q), f, indent=1)
        return names + ["summary.json"]


def _direction(direction):
    if direction in (0, 1):
        return int(direction)
    if direction in DIRECTIONS:
        return DIRECTIONS.index(direction)
    raise ValueError(f"direction is one of {DIRECTIONS} or 0 / 1 (got {direction!r})")


class Distances:
    """Running distance measures of the (real, generated) field pairs added so far on an H x W grid.  The device returns the
    records of a chunk of fields, pooled on the host at once as Python integers and dropped, unless ``keep_records``; the ring
    table accumulates on the device."""

    def __init__(self, spec, H, W, device=None, ops=None, keep_records=False):
        if not isinstance(spec, DistSpec):
            raise TypeError(f"Distances takes a DistSpec (got {type(spec).__name__})")
        H, W = int(H), int(W)
        if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
            raise ValueError(f"Distances needs a grid of 1 <= H, W <= {SIDE_MAX} (got {H} x {W})")
        self.spec, self.H, self.W = spec, H, W
        self.device = torch.device(ops.device if ops is not None and device is None else "cuda:0" if device is None else device)
        self._ops = ops
        self.keep_records = bool(keep_records)
        self._s = {k: [[0] * spec.K for _ in range(spec.nout)] for k in POOLED}
        self._hmax = np.zeros((spec.nout, spec.K), np.int64)
        self._hsum = np.zeros((spec.nout, spec.K), np.float64)
        self._rings = None                                           # int64 [nout, K, 2, nring + 2] on the device, made on first use
        self._records = []
        self.fields = 0
        self.calls = 0
        self.ws_cap = WS_CAP
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    def _pool(self, rec):
        """Pool the records int64 [m, nout, K, 11] of a chunk of fields: Python integers throughout (bad2 alone reaches 2^60
        per record)."""
        if self.keep_records:
            self._records.append(rec.copy())
        na, nb = rec[..., N_A] > 0, rec[..., N_B] > 0
        kind = {"both": na & nb, "real_only": na & ~nb, "fake_only": ~na & nb, "neither": ~na & ~nb}
        both = kind["both"]
        total = lambda col, where=None: (rec[..., col] if where is None else np.where(where, rec[..., col], 0)).astype(object).sum(0)
        add = {k: v.astype(object).sum(0) for k, v in kind.items()}
        add.update(n_b_both=total(N_B, both), sum_dq_b2a=total(SUM_DQ_B2A, both), sum_d2_b2a=total(SUM_D2_B2A, both),
                   n_a_both=total(N_A, both), sum_dq_a2b=total(SUM_DQ_A2B, both), sum_d2_a2b=total(SUM_D2_A2B, both),
                   bad1=total(BAD1), bad2=total(BAD2), n_a=total(N_A), n_b=total(N_B), n_ab=total(N_AB))
        for key, v in add.items():
            for j in range(self.spec.nout):
                for k in range(self.spec.K):
                    self._s[key][j][k] += int(v[j, k])
        h2 = np.where(both, np.maximum(rec[..., MAX_D2_B2A], rec[..., MAX_D2_A2B]), 0)     # below 2^24: its sqrt is exact to 1 ulp
        self._hmax = np.maximum(self._hmax, h2.max(0))
        self._hsum += np.sqrt(h2.astype(np.float64)).sum(0)

    def add(self, real, fake, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) field pairs of a batch.  Layouts as ``fss.FractionsSkill.add`` ([T, C, H, W];
        with ``nhwc`` a [T, H, W, c_pad] store of which the leading ``channels`` are read; a ``NativeBatch``); the two series may
        differ in layout and dtype: pass ``nhwc`` as a pair (real, fake) then.  Every dg_distmap call ends with one
        synchronising copy of its records."""
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "distmap", self.spec, "Distances", (self.H, self.W))
        if self._struct is None:
            self._struct = self.spec.struct()
        o, sp = self.ops, self.spec
        if self._rings is None:
            self._rings = torch.zeros(sp.nout, sp.K, 2, sp.nring + 2, dtype=torch.int64, device=o.device)
        _, f1 = fields.descriptor(o, a.x[:1], a.nhwc, a.C)
        per_field = max(1, o.distmap_ws_bytes(f1, self.H, self.W, self._struct))
        tc = max(1, min(n, self.ws_cap // per_field))
        for t0 in range(0, n, tc):
            m = min(tc, n - t0)
            ka, fa = fields.descriptor(o, a.x[t0:t0 + m], a.nhwc, a.C)
            kb, fb = fields.descriptor(o, b.x[t0:t0 + m], b.nhwc, b.C)
            records = torch.empty(m, sp.nout, sp.K, COLS, dtype=torch.int64, device=o.device)
            o.distmap(fa, fb, self.H, self.W, self._struct, records=records, rings=self._rings)
            self.calls += 1
            self._pool(records.cpu().numpy())
            self.fields += m
        return self

    def _ring_table(self):
        sp = self.spec
        return np.zeros((sp.nout, sp.K, 2, sp.nring + 2), np.int64) if self._rings is None else self._rings.cpu().numpy()

    def reduce_(self, dist):
        """Sum the pooled integers and the ring table over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in
        place and exactly: fss.allreduce_ints carries every total as 32-bit limbs, so the pooled bad2 (2^60 per record) cannot
        overflow; the largest Hausdorff distance by a max; the sum of the per-pair Hausdorff distances with one ordinary float64
        all-reduce (equal from run to run at one world size).  Kept records stay this rank's."""
        if dist is not None and dist.world_size > 1:
            dev = self.device if getattr(dist, "backend", "gloo") == "nccl" else "cpu"
            sp = self.spec
            rings = self._ring_table()
            flat = [v for key in POOLED for row in self._s[key] for v in row] + [int(v) for v in rings.reshape(-1)] + [self.fields]
            vals = allreduce_ints(dist, flat, dev)
            off = 0
            for key in POOLED:
                for j in range(sp.nout):
                    self._s[key][j] = vals[off:off + sp.K]
                    off += sp.K
            self._rings = torch.tensor(vals[off:off + rings.size], dtype=torch.int64).reshape(rings.shape).to(self.device)
            self.fields = int(vals[-1])
            big = self._hmax.reshape(-1)                             # <= 2^24: exact in float64
            mm = torch.from_numpy(np.stack([big, big], axis=1).astype(np.float64).reshape(1, -1)).to(dev)
            dist.minmax_(mm, big.size)
            self._hmax = mm.cpu().numpy().reshape(-1, 2)[:, 1].astype(np.int64).reshape(self._hmax.shape)
            s = torch.from_numpy(self._hsum.reshape(-1).copy()).to(dev)
            dist.allreduce_sum_(s)
            self._hsum = s.cpu().numpy().reshape(self._hsum.shape)
        return self

    def result(self):
        """The ``DistanceResult`` of everything added (and, after ``reduce_``, of every rank)."""
        sp = self.spec
        records = None
        if self.keep_records:
            records = np.concatenate(self._records) if self._records else np.zeros((0, sp.nout, sp.K, COLS), np.int64)
        return DistanceResult(sp, self.H, self.W, self.fields, self._s, self._ring_table(), self._hmax, self._hsum, records)


def distances(real, fake, spec=None, n_valid=None, nhwc=False, channels=None, ops=None, keep_records=False):
    """Distance measures of a (real, generated) pair of series, on the GPU -> ``DistanceResult``.  spec None:
    ``DistSpec.zscore`` of the fields' channels; the other arguments as ``Distances.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "distmap")
    if spec is None:
        spec = DistSpec.zscore(Cn)
    if not isinstance(spec, DistSpec):
        raise TypeError(f"distances takes a DistSpec (got {type(spec).__name__})")
    acc = Distances(spec, H, W, device=device, ops=ops, keep_records=keep_records)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
