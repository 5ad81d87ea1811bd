"""Intensity-scale verification (Casati, Ross & Stephenson 2004; the energies of Casati 2010) of real against generated
fields, computed on the GPU (csrc/iscale.hip).

The fractions skill score says from which window size the generator is skilful; it cannot say whether the error at 8 px is a
displacement of 8-px features or noise at 1 px that the window averages away.  The intensity-scale score splits the error of the
thresholded fields into orthogonal 2-D Haar components, one per dyadic scale, so that the mean squared error adds up over the
scales.  For output channel j of an ``IscaleSpec`` (the transform of ``fss`` / ``histograms``, the same device code) and
threshold k, with n the smallest integer with 2^n >= max(H, W) and the masks zero outside the grid, on the 2^n x 2^n square
anchored at pixel (0, 0):

    I_a[t,p] = (y_a > thr[j][k])                                 fp32 compare: NaN false, +inf true, equality false; I_b likewise
    S_l(X, block) = sum of X over an aligned block of side 2^l,  l = 0 .. n
    D_l = sum (S_l(I_b) - S_l(I_a))^2,  A_l = sum S_l(I_a)^2,  B_l = sum S_l(I_b)^2     exact integers over all fields and blocks

and on the host, from Python integers, with E = D, A or B and N = fields * 4^n padded pixels:

    component l = 1 .. n (mother wavelet, features of side 2^(l-1)):  E_(l-1) / 4^(l-1) - E_l / 4^l
    component n + 1 (father, the mean of the square):                 E_n / 4^n             they sum to E_0
    MSE_l = the D component / N,  En_l(a), En_l(b) = the A, B components / N,  r_a = A_0 / N,  r_b = B_0 / N
    MSE_random = r_b (1 - r_a) + r_a (1 - r_b)
    SS_l = 1 - (n + 1) MSE_l / MSE_random                         NaN when MSE_random = 0
    energy relative difference = (En_l(b) - En_l(a)) / (En_l(b) + En_l(a))      NaN when the denominator is 0

The device works in integers only (wave ballots, popcounts, packed adds, integer atomics) and keeps nothing per pixel: the sums
are exact and two calls on the same data are bit-identical.  ``IntensityScale`` accumulates batches in device int64 accumulators
in front of host totals kept as Python integers (drained before the accumulators could pass 2^62), sums them exactly over
data-parallel ranks, and the trainer's opt-in hook (``WassersteinGAN.log_intensity_scale``) keeps one per part.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib, fields
from .fss import allreduce_ints
from .gridstats import _jsonable
from .histograms import C_MAX, _default_ops, _f32

THR_MAX, LEVELS_MAX, SIDE_MAX = _lib.ISCALE_MAX_THR, _lib.ISCALE_MAX_LEVELS, _lib.ISCALE_MAX_SIDE
WS_CAP = 512 << 20           # bytes of dg_iscale workspace at most: a batch is cut into chunks of fields (at least one)
CALL_LIMIT = 1 << 62         # the most T * dg_iscale_bound of one dg_iscale call (the library rejects more)
DRAIN_LIMIT = 1 << 62        # the device accumulators are drained to the host totals before they could pass this
DEFAULT_THRESHOLDS = (1.0, 2.0)
SIDES = ("real", "fake")


def log_side(H, W):
    """n, the smallest integer with 2^n >= max(H, W): the levels are 0 .. n (dg_iscale_levels = n + 1)."""
    return (max(int(H), int(W)) - 1).bit_length()


def bound(H, W):
    """dg_iscale_bound in Python integers: 16^n, the most one field adds to any of D_l, A_l, B_l."""
    return 16 ** log_side(H, W)


class IscaleSpec:
    """Units and thresholds of the intensity-scale verification of C input channels (+ the speed of a pair of them, appended as
    the last output).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None;
    thresholds: 1 .. THR_MAX values per output channel -- one list per output channel, or one list of numbers for all --
    rounded to fp32; names: one per output channel.  The scales are not chosen: they are the dyadic ones of the grid."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), thresholds=DEFAULT_THRESHOLDS, names=None):
        if not (isinstance(C, (int, np.integer)) and 1 <= C <= C_MAX):
            raise ValueError(f"iscale takes 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"iscale speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"iscale scale and offset need one value per input channel (C = {self.C})")
        thr = list(thresholds)
        if all(np.ndim(t) == 0 for t in thr):
            thr = [thr] * self.nout                                  # one list for every channel
        if len(thr) != self.nout or len({len(t) for t in thr}) != 1:
            raise ValueError(f"iscale thresholds need one list per output channel ({self.nout}), all of one length")
        K = len(thr[0])
        if not 1 <= K <= THR_MAX:
            raise ValueError(f"iscale takes 1 to {THR_MAX} thresholds per channel (got {K})")
        self.thresholds = np.stack([_f32(t, "thresholds") for t in thr])
        self.K = K
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"iscale names need one entry per output channel ({self.nout})")

    @classmethod
    def zscore(cls, C, thresholds=DEFAULT_THRESHOLDS):
        """Standardised fields: the speed of channels (0, 1) when C >= 2, the same thresholds in every channel."""
        return cls(C, speed=(0, 1) if C >= 2 else None, thresholds=thresholds)

    @classmethod
    def physical(cls, stats, order, thresholds, speed=("u10", "v10")):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, evaluated
        in physical units (y = x * std + mean).  thresholds: as the constructor's, in physical units; speed: the names of the
        (u, v) pair, or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        names = order + (["speed"] if sp else [])
        return cls(len(order), scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp,
                   thresholds=thresholds, names=names)

    def struct(self):
        """The dg_iscale_spec of this spec (no library call)."""
        s = _lib.IscaleSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nthr = self.K
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            for k in range(self.K):
                s.thr[j][k] = float(self.thresholds[j, k])
        return s

    def __eq__(self, other):
        return (isinstance(other, IscaleSpec) and self.C == other.C and self.speed == other.speed
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("scale", "offset", "thresholds")))

    __hash__ = None


def _side(side):
    s = {"real": 0, "fake": 1, 0: 0, 1: 1}.get(side)
    if s is None:
        raise ValueError(f"side must be 'real' or 'fake' (got {side!r})")
    return s


def _float(q):
    """A Fraction (or None: undefined) as the nearest float64 (NaN)."""
    return math.nan if q is None else q.numerator / q.denominator


class IscaleResult:
    """The exact sums of one IscaleSpec on an H x W grid over ``fields`` field pairs: D_l, A_l, B_l per (output channel,
    threshold, level l = 0 .. n) as Python integers, and what is formed from them.  The n + 1 components are the Haar (mother)
    components of the features of side ``scales_px[:n]`` = 1, 2, .. 2^(n-1) px and, last, the father component (the mean over
    the 2^n square, ``scales_px[n]`` = 2^n)."""

    def __init__(self, spec, H, W, sums, fields):
        self.spec, self.H, self.W, self.fields = spec, int(H), int(W), int(fields)
        self.n = log_side(H, W)
        self.levels = self.n + 1
        self.scales_px = tuple(1 << l for l in range(self.n)) + (1 << self.n,)
        self._sums = np.empty((spec.nout, spec.K, self.levels, 3), dtype=object)
        self._sums.reshape(-1)[:] = [int(v) for v in np.asarray(sums, dtype=object).reshape(-1)]

    @property
    def padded_pixels(self):
        """N = fields * 4^n."""
        return self.fields * 4 ** self.n

    def sums(self):
        """Python-int array [nout, K, n + 1, 3]: D_l, A_l, B_l."""
        return self._sums.copy()

    def _components(self, j, k, e):
        """The n + 1 components of term e (0 D, 1 A, 2 B) as exact Fractions."""
        E = [int(v) for v in self._sums[j, k, :, e]]
        return [Fraction(E[l - 1], 4 ** (l - 1)) - Fraction(E[l], 4 ** l) for l in range(1, self.levels)] + [Fraction(E[self.n], 4 ** self.n)]

    def _per_component(self, f):
        """float64 [nout, K, n + 1] of f(j, k) -> n + 1 Fractions (None: undefined)."""
        out = np.empty((self.spec.nout, self.spec.K, self.levels), dtype=np.float64)
        for j, k in np.ndindex(self.spec.nout, self.spec.K):
            out[j, k] = [_float(q) for q in f(j, k)]
        return out

    def components(self):
        """float64 [nout, K, n + 1, 3]: the Haar components of D, A and B (each the nearest double of the exact value); over
        the components they sum to D_0, A_0 = N_a and B_0 = N_b."""
        return np.stack([self._per_component(lambda j, k: self._components(j, k, e)) for e in range(3)], axis=-1)

    def mse(self):
        """float64 [nout, K, n + 1]: MSE_l, the D component over the padded pixels; their sum is the MSE of the binary fields."""
        N = self.padded_pixels
        return self._per_component(lambda j, k: [q / N if N else None for q in self._components(j, k, 0)])

    def energy(self, side="real"):
        """float64 [nout, K, n + 1]: En_l of the real (A) or generated (B) masks; their sum is the base rate."""
        N, e = self.padded_pixels, 1 + _side(side)
        return self._per_component(lambda j, k: [q / N if N else None for q in self._components(j, k, e)])

    def base_rates(self, side="real"):
        """float64 [nout, K]: r = N_a / N (or N_b / N), the fraction of the padded pixels above the threshold."""
        N, e = self.padded_pixels, 1 + _side(side)
        return np.array([[int(self._sums[j, k, 0, e]) / N if N else math.nan for k in range(self.spec.K)]
                         for j in range(self.spec.nout)], dtype=np.float64).reshape(self.spec.nout, self.spec.K)

    def frequency_bias(self):
        """float64 [nout, K]: N_b / N_a (NaN when the real series never exceeds the threshold)."""
        s = self._sums
        return np.array([[int(s[j, k, 0, 2]) / int(s[j, k, 0, 1]) if int(s[j, k, 0, 1]) else math.nan for k in range(self.spec.K)]
                         for j in range(self.spec.nout)], dtype=np.float64).reshape(self.spec.nout, self.spec.K)

    def _mse_random(self, j, k):
        """r_b (1 - r_a) + r_a (1 - r_b) as an exact Fraction (None without a field)."""
        N = self.padded_pixels
        if not N:
            return None
        na, nb = int(self._sums[j, k, 0, 1]), int(self._sums[j, k, 0, 2])
        return Fraction(nb * (N - na) + na * (N - nb), N * N)

    def mse_random(self):
        """float64 [nout, K]: the MSE of a random forecast with the two base rates."""
        return np.array([[_float(self._mse_random(j, k)) for k in range(self.spec.K)] for j in range(self.spec.nout)],
                        dtype=np.float64).reshape(self.spec.nout, self.spec.K)

    def skill(self):
        """float64 [nout, K, n + 1]: SS_l = 1 - (n + 1) MSE_l / MSE_random (NaN when MSE_random = 0); the mean over the
        components is 1 - MSE / MSE_random."""
        N = self.padded_pixels

        def f(j, k):
            r = self._mse_random(j, k)
            if not r:
                return [None] * self.levels
            return [1 - self.levels * q / N / r for q in self._components(j, k, 0)]
        return self._per_component(f)

    def energy_rel_diff(self):
        """float64 [nout, K, n + 1]: (En_l(b) - En_l(a)) / (En_l(b) + En_l(a)), NaN where both vanish; positive where the
        generator has too much structure at that scale."""
        def f(j, k):
            a, b = self._components(j, k, 1), self._components(j, k, 2)
            return [(y - x) / (y + x) if y + x else None for x, y in zip(a, b)]
        return self._per_component(f)

    def worst_scale(self):
        """float64 [nout, K]: ``scales_px`` of the component with the lowest skill (the first of equals), NaN when the skill is
        undefined."""
        s = self.skill()
        out = np.full(s.shape[:2], np.nan)
        for j, k in np.ndindex(*out.shape):
            if not np.isnan(s[j, k]).any():
                out[j, k] = float(self.scales_px[int(np.argmin(s[j, k]))])
        return out

    def summary(self):
        """A JSON-serialisable dict (None where undefined); the exact integers are kept as integers."""
        return {"channels": list(self.spec.names), "fields": self.fields, "grid": [self.H, self.W], "levels": self.levels,
                "thresholds": _jsonable(self.spec.thresholds), "scales_px": list(self.scales_px),
                "skill": [_jsonable(a) for a in self.skill()], "mse": [_jsonable(a) for a in self.mse()],
                "mse_random": _jsonable(self.mse_random()),
                "energy": {side: [_jsonable(a) for a in self.energy(side)] for side in SIDES},
                "energy_rel_diff": [_jsonable(a) for a in self.energy_rel_diff()],
                "base_rate": {side: _jsonable(self.base_rates(side)) for side in SIDES},
                "frequency_bias": _jsonable(self.frequency_bias()), "worst_scale": _jsonable(self.worst_scale()),
                "sums": [[[[int(v) for v in s] for s in k] for k in j] for j in self._sums]}


class IntensityScale:
    """Running intensity-scale sums of the (real, generated) field pairs added so far on an H x W grid: device int64
    accumulators in front of host totals kept as Python integers."""

    def __init__(self, spec, H, W, device=None, ops=None):
        if not isinstance(spec, IscaleSpec):
            raise TypeError(f"IntensityScale takes an IscaleSpec (got {type(spec).__name__})")
        H, W = int(H), int(W)
        if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
            raise ValueError(f"IntensityScale needs a grid of 1 <= H, W <= {SIDE_MAX} (got {H} x {W})")
        self.spec, self.H, self.W = spec, H, W
        self.levels = log_side(H, W) + 1
        self._bound = bound(H, W)
        self.device = torch.device("cuda:0" if device is None else device)
        self._ops = ops
        self._dev_sums = torch.zeros(spec.nout, spec.K, self.levels, 3, dtype=torch.int64, device=self.device)
        self._dev_bound = 0                                          # the most a device sum can hold now (host mirror: no sync)
        self._sums = [0] * self._dev_sums.numel()                    # host totals
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
        for i, v in enumerate(self._dev_sums.reshape(-1).cpu().tolist()):
            self._sums[i] += v
        self._dev_sums.zero_()
        self._dev_bound = 0
        self.drains += 1

    def add(self, real, fake, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) field pairs of a batch.  Layouts as ``histograms.histogram`` ([T, C, H, W];
        with ``nhwc`` a [T, H, W, c_pad] store of which the leading ``channels`` are read; a ``NativeBatch``); the two series
        may differ in layout and dtype: pass ``nhwc`` as a pair (real, fake) then."""
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "iscale", self.spec, "IntensityScale", (self.H, self.W))
        if self._struct is None:
            self._struct = self.spec.struct()
        o, mb = self.ops, self._bound
        limit = min(DRAIN_LIMIT, CALL_LIMIT)
        _, f1 = fields.descriptor(o, a.x[:1], a.nhwc, a.C)
        per_field = max(1, o.iscale_ws_bytes(f1, self.H, self.W, self._struct))
        tc = max(1, min(n, WS_CAP // per_field, limit // mb))         # fields per call: workspace cap and per-call headroom
        for t0 in range(0, n, tc):
            m = min(tc, n - t0)
            if self._dev_bound and self._dev_bound + m * mb > limit:
                self._drain()
            ka, fa = fields.descriptor(o, a.x[t0:t0 + m], a.nhwc, a.C)
            kb, fb = fields.descriptor(o, b.x[t0:t0 + m], b.nhwc, b.C)
            o.iscale(fa, fb, self.H, self.W, self._struct, self._dev_sums)
            self._dev_bound += m * mb
        self.fields += n
        return self

    def reduce_(self, dist):
        """Sum the totals exactly over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place."""
        if dist is not None and dist.world_size > 1:
            self._drain()
            dev = self.device if getattr(dist, "backend", "gloo") == "nccl" else "cpu"
            vals = allreduce_ints(dist, self._sums + [self.fields], dev)
            self._sums, self.fields = vals[:-1], vals[-1]
        return self

    def result(self):
        """The ``IscaleResult`` of every pair added (and, after ``reduce_``, of every rank)."""
        if self._dev_bound:
            self._drain()
        return IscaleResult(self.spec, self.H, self.W, list(self._sums), self.fields)


def intensity_scale(real, fake, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """Intensity-scale verification of a (real, generated) pair of series of fields on the GPU -> ``IscaleResult``.  spec None:
    ``IscaleSpec.zscore`` of the fields' channels; the other arguments as ``IntensityScale.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "iscale")
    if spec is None:
        spec = IscaleSpec.zscore(Cn)
    if not isinstance(spec, IscaleSpec):
        raise TypeError(f"intensity_scale takes an IscaleSpec (got {type(spec).__name__})")
    acc = IntensityScale(spec, H, W, device=device, ops=ops)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()
