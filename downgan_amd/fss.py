"""Fractions skill score (FSS, Roberts & Lean 2008) of real against generated fields, computed on the GPU (csrc/fss.hip).

A generator that puts a gust front in the right place but a few pixels off is punished twice by MAE / RMSE and by the
per-gridpoint maps, and spectra and histograms cannot see the displacement at all.  The FSS asks instead: at which neighbourhood
size does the generated field put threshold exceedances where the real field has them?  For output channel j of an ``FssSpec``
(the transform of ``histograms`` / ``gridstats``, the same device code), threshold k and window side n (odd):

    I_a[t,p] = (y_a > thr[j][k])                                 fp32 compare: NaN false, +inf true, equality false; I_b likewise
    c_a[t,h,w] = number of set I_a in rows h-r .. h+r, columns w-r .. w+r, r = (n-1)/2, zero outside the grid; c_b likewise
    D = sum (c_a - c_b)^2,  A = sum c_a^2,  B = sum c_b^2          exact integers over all fields and pixels
    FSS = 1 - D / (A + B)                                        NaN when A + B = 0

The device works in integers only (summed-area tables, 64-bit squares, integer atomics): the sums are exact and two calls on the
same data are bit-identical.  ``FractionsSkill`` accumulates batches in device int64 accumulators in front of host totals kept
as Python integers (drained before the accumulators could pass 2^62), sums them exactly over data-parallel ranks, and the
trainer's opt-in hook (``WassersteinGAN.log_fss``) keeps one per part.  ``FssResult`` forms the score, the base rates, the
frequency bias, the "useful" level 0.5 + f0 / 2 and the smallest skilful scale on the host.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, fields
from .gridstats import _jsonable
from .histograms import C_MAX, _default_ops, _f32

THR_MAX, SCALES_MAX, SIDE_MAX = _lib.FSS_MAX_THR, _lib.FSS_MAX_SCALES, _lib.FSS_MAX_SIDE
WS_CAP = 512 << 20           # bytes of dg_fss workspace at most: a batch is cut into chunks of fields (at least one)
CALL_LIMIT = 1 << 62         # the most T * max dg_fss_bound of one dg_fss call (the library rejects more)
DRAIN_LIMIT = 1 << 62        # the device accumulators are drained to the host totals before they could pass this
LIMBS = 4                    # 32-bit limbs of the exact all-reduce: totals below 2^128
DEFAULT_SCALES = (1, 3, 5, 9, 17, 33, 65, 129)
SIDES = ("real", "fake")


def bound(H, W, win):
    """dg_fss_bound in Python integers: H W (min(win, H) min(win, W))^2, the most one field adds to D, A or B."""
    return H * W * (min(win, H) * min(win, W)) ** 2


def score(D, A, B):
    """1 - D / (A + B) from the exact integers (NaN when A + B = 0)."""
    return 1.0 - int(D) / (int(A) + int(B)) if int(A) + int(B) > 0 else math.nan


class FssSpec:
    """Units, thresholds and window sides of the fractions skill score of C input channels (+ the speed of a pair of them,
    appended as the last output).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None;
    thresholds: 1 .. THR_MAX values per output channel -- one list per output channel, or one list of numbers for all --
    rounded to fp32; scales: 1 .. SCALES_MAX odd window sides, strictly increasing, at most 2 SIDE_MAX - 1; names: one per
    output channel."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), thresholds=(), scales=DEFAULT_SCALES, names=None):
        if not (isinstance(C, (int, np.integer)) and 1 <= C <= C_MAX):
            raise ValueError(f"fss takes 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"fss speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"fss scale and offset need one value per input channel (C = {self.C})")
        thr = list(thresholds)
        if all(np.ndim(t) == 0 for t in thr):
            thr = [thr] * self.nout                                  # one list for every channel
        if len(thr) != self.nout or len({len(t) for t in thr}) != 1:
            raise ValueError(f"fss thresholds need one list per output channel ({self.nout}), all of one length")
        K = len(thr[0])
        if not 1 <= K <= THR_MAX:
            raise ValueError(f"fss takes 1 to {THR_MAX} thresholds per channel (got {K})")
        self.thresholds = np.stack([_f32(t, "thresholds") for t in thr])
        self.K = K
        sc = list(scales)
        if not all(isinstance(n, (int, np.integer)) for n in sc):
            raise ValueError(f"fss scales are integer window sides (got {sc!r})")
        if not 1 <= len(sc) <= SCALES_MAX:
            raise ValueError(f"fss takes 1 to {SCALES_MAX} scales (got {len(sc)})")
        if not all(n % 2 == 1 and 1 <= n <= 2 * SIDE_MAX - 1 for n in sc):
            raise ValueError(f"fss window sides must be odd and in [1, {2 * SIDE_MAX - 1}] (got {sc})")
        if any(b <= a for a, b in zip(sc, sc[1:])):
            raise ValueError(f"fss window sides must be strictly increasing (got {sc})")
        self.scales = tuple(int(n) for n in sc)
        self.S = len(self.scales)
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"fss names need one entry per output channel ({self.nout})")

    @classmethod
    def zscore(cls, C, thresholds=(1.0, 2.0), scales=DEFAULT_SCALES):
        """Standardised fields: the speed of channels (0, 1) when C >= 2, the same thresholds in every channel."""
        return cls(C, speed=(0, 1) if C >= 2 else None, thresholds=thresholds, scales=scales)

    @classmethod
    def physical(cls, stats, order, thresholds, scales=DEFAULT_SCALES, speed=("u10", "v10")):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, evaluated
        in physical units (y = x * std + mean).  thresholds: as the constructor's, in physical units; speed: the names of the
        (u, v) pair, or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        names = order + (["speed"] if sp else [])
        return cls(len(order), scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp,
                   thresholds=thresholds, scales=scales, names=names)

    def struct(self):
        """The dg_fss_spec of this spec (no library call)."""
        s = _lib.FssSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nthr, s.nscale = self.K, self.S
        for i, n in enumerate(self.scales):
            s.win[i] = n
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            for k in range(self.K):
                s.thr[j][k] = float(self.thresholds[j, k])
        return s

    def __eq__(self, other):
        return (isinstance(other, FssSpec) and self.C == other.C and self.speed == other.speed and self.scales == other.scales
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("scale", "offset", "thresholds")))

    __hash__ = None


def _side(side):
    s = {"real": 0, "fake": 1, 0: 0, 1: 1}.get(side)
    if s is None:
        raise ValueError(f"side must be 'real' or 'fake' (got {side!r})")
    return s


class FssResult:
    """The exact sums of one FssSpec on an H x W grid over ``fields`` field pairs: D, A, B per (output channel, threshold,
    scale) and the mask counts N_a, N_b per (output channel, threshold), as Python integers."""

    def __init__(self, spec, H, W, sums, rates, fields):
        self.spec, self.H, self.W, self.fields = spec, int(H), int(W), int(fields)
        self._sums = np.empty((spec.nout, spec.K, spec.S, 3), dtype=object)
        self._sums.reshape(-1)[:] = [int(v) for v in np.asarray(sums, dtype=object).reshape(-1)]
        self._rates = np.empty((spec.nout, spec.K, 2), dtype=object)
        self._rates.reshape(-1)[:] = [int(v) for v in np.asarray(rates, dtype=object).reshape(-1)]

    def sums(self):
        """Python-int array [nout, K, S, 3]: D, A, B."""
        return self._sums.copy()

    def rates(self):
        """Python-int array [nout, K, 2]: N_a (real), N_b (generated)."""
        return self._rates.copy()

    def fss(self):
        """float64 [nout, K, S]: 1 - D / (A + B), NaN where no window of either series holds an exceedance."""
        s = self._sums
        out = np.empty(s.shape[:3], dtype=np.float64)
        for i in np.ndindex(*out.shape):
            out[i] = score(*s[i])
        return out

    def base_rate(self, side="real"):
        """float64 [nout, K]: the fraction of all pixels of all fields above the threshold."""
        n = self.fields * self.H * self.W
        r = self._rates[:, :, _side(side)]
        return np.array([[int(v) / n if n else math.nan for v in row] for row in r], dtype=np.float64).reshape(r.shape)

    def frequency_bias(self):
        """float64 [nout, K]: N_b / N_a (NaN when the real series never exceeds the threshold)."""
        r = self._rates
        return np.array([[int(b) / int(a) if int(a) else math.nan for a, b in row] for row in r], dtype=np.float64).reshape(r.shape[:2])

    def target(self):
        """float64 [nout, K]: 0.5 + base_rate("real") / 2, the usual level above which a scale counts as skilful."""
        return 0.5 + self.base_rate("real") / 2

    def skillful_scale(self):
        """float64 [nout, K]: the smallest window side with FSS >= target, NaN when there is none."""
        f, t = self.fss(), self.target()
        out = np.full(t.shape, np.nan)
        for j, k in np.ndindex(*t.shape):
            for s, n in enumerate(self.spec.scales):
                if f[j, k, s] >= t[j, k]:                            # a NaN score or target never passes
                    out[j, k] = float(n)
                    break
        return out

    def summary(self):
        """A JSON-serialisable dict (None where undefined); the exact integers are kept as integers."""
        return {"channels": list(self.spec.names), "fields": self.fields, "grid": [self.H, self.W],
                "thresholds": _jsonable(self.spec.thresholds), "scales": list(self.spec.scales),
                "fss": [_jsonable(a) for a in self.fss()],
                "base_rate": {side: _jsonable(self.base_rate(side)) for side in SIDES},
                "frequency_bias": _jsonable(self.frequency_bias()), "target": _jsonable(self.target()),
                "skillful_scale": _jsonable(self.skillful_scale()),
                "sums": [[[[int(v) for v in s] for s in k] for k in j] for j in self._sums],
                "rates": [[[int(v) for v in k] for k in j] for j in self._rates]}


def to_limbs(values, device="cpu"):
    """int64 [len(values), LIMBS]: the non-negative Python integers ``values`` (< 2^(32 LIMBS)) as 32-bit limbs, lowest first."""
    vals = [int(v) for v in values]
    if any(v < 0 or v >> (32 * LIMBS) for v in vals):
        raise ValueError(f"the limb all-reduce carries integers in [0, 2^{32 * LIMBS})")
    return torch.tensor([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(LIMBS)] for v in vals], dtype=torch.int64).reshape(-1, LIMBS).to(device)


def from_limbs(t):
    """The Python integers of a limb tensor (every limb may have grown past 32 bits by summation)."""
    return [sum(int(l) << (32 * i) for i, l in enumerate(row)) for row in t.cpu().tolist()]


def allreduce_ints(dist, values, device="cpu"):
    """The exact sums of the Python integers ``values`` over the ranks of ``dist``: split into 32-bit limbs in an int64 tensor
    (a limb sum stays below 2^63 for fewer than 2^31 ranks), one all-reduce, recombined."""
    if dist is None or dist.world_size <= 1:
        return [int(v) for v in values]
    t = to_limbs(values, device)
    dist.allreduce_sum_(t.view(-1))
    return from_limbs(t)


class FractionsSkill:
    """Running FSS sums of the (real, generated) field pairs added so far on an H x W grid: device int64 accumulators in
    front of host totals kept as Python integers."""

    def __init__(self, spec, H, W, device=None, ops=None):
        if not isinstance(spec, FssSpec):
            raise TypeError(f"FractionsSkill takes an FssSpec (got {type(spec).__name__})")
        H, W = int(H), int(W)
        if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
            raise ValueError(f"FractionsSkill needs a grid of 1 <= H, W <= {SIDE_MAX} (got {H} x {W})")
        self._max_bound = max(bound(H, W, n) for n in spec.scales)
        if self._max_bound > CALL_LIMIT:
            raise ValueError(f"one {H} x {W} field at window side {spec.scales[-1]} can add {self._max_bound} > 2^62 to a sum: "
                             "beyond the int64 device path")
        self.spec, self.H, self.W = spec, H, W
        self.device = torch.device("cuda:0" if device is None else device)
        self._ops = ops
        self._dev_sums = torch.zeros(spec.nout, spec.K, spec.S, 3, dtype=torch.int64, device=self.device)
        self._dev_rates = torch.zeros(spec.nout, spec.K, 2, dtype=torch.int64, device=self.device)
        self._dev_bound = 0                                          # the most a device sum can hold now (host mirror: no sync)
        self._sums = [0] * self._dev_sums.numel()                    # host totals
        self._rates = [0] * self._dev_rates.numel()
        self.fields = 0
        self.drains = 0
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    def _drain(self):
        """Move the device accumulators into the host totals (one synchronising copy) and zero them."""
        for host, dev in ((self._sums, self._dev_sums), (self._rates, self._dev_rates)):
            for i, v in enumerate(dev.reshape(-1).cpu().tolist()):
                host[i] += v
            dev.zero_()
        self._dev_bound = 0
        self.drains += 1

    def add(self, real, fake, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) field pairs of a batch.  Layouts as ``histograms.histogram`` ([T, C, H, W];
        with ``nhwc`` a [T, H, W, c_pad] store of which the leading ``channels`` are read; a ``NativeBatch``); the two series
        may differ in layout and dtype: pass ``nhwc`` as a pair (real, fake) then."""
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "fss", self.spec, "FractionsSkill", (self.H, self.W))
        if self._struct is None:
            self._struct = self.spec.struct()
        o, mb = self.ops, self._max_bound
        limit = min(DRAIN_LIMIT, CALL_LIMIT)
        _, f1 = fields.descriptor(o, a.x[:1], a.nhwc, a.C)
        per_field = max(1, o.fss_ws_bytes(f1, self.H, self.W, self._struct))
        tc = max(1, min(n, WS_CAP // per_field, limit // mb))         # fields per call: workspace cap and per-call headroom
        for t0 in range(0, n, tc):
            m = min(tc, n - t0)
            if self._dev_bound and self._dev_bound + m * mb > limit:
                self._drain()
            ka, fa = fields.descriptor(o, a.x[t0:t0 + m], a.nhwc, a.C)
            kb, fb = fields.descriptor(o, b.x[t0:t0 + m], b.nhwc, b.C)
            o.fss(fa, fb, self.H, self.W, self._struct, self._dev_sums, self._dev_rates)
            self._dev_bound += m * mb
        self.fields += n
        return self

    def reduce_(self, dist):
        """Sum the totals exactly over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place."""
        if dist is not None and dist.world_size > 1:
            self._drain()
            dev = self.device if getattr(dist, "backend", "gloo") == "nccl" else "cpu"
            vals = allreduce_ints(dist, self._sums + self._rates + [self.fields], dev)
            ns = len(self._sums)
            self._sums, self._rates, self.fields = vals[:ns], vals[ns:-1], vals[-1]
        return self

    def result(self):
        """The ``FssResult`` of every pair added (and, after ``reduce_``, of every rank)."""
        if self._dev_bound:
            self._drain()
        return FssResult(self.spec, self.H, self.W, list(self._sums), list(self._rates), self.fields)


def fss(real, fake, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """Fractions skill score of a (real, generated) pair of series of fields on the GPU -> ``FssResult``.  spec None:
    ``FssSpec.zscore`` of the fields' channels; the other arguments as ``FractionsSkill.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "fss")
    if spec is None:
        spec = FssSpec.zscore(Cn)
    if not isinstance(spec, FssSpec):
        raise TypeError(f"fss takes an FssSpec (got {type(spec).__name__})")
    acc = FractionsSkill(spec, H, W, device=device, ops=ops)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
