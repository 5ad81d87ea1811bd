"""Field-deformation verification (the displacement and amplitude score of Keil & Craig 2007, 2009) of real against generated
fields, computed on the GPU (csrc/deform.hip).

Neighbourhood (``fss``), scale-separation (``iscale``) and feature (``objects``, ``distmap``) scores cannot say by which vector, at
which place, the generated field has to be moved to lie on the real one, nor how much error is left once it has been moved.  A
pyramidal image matcher answers that with a displacement field, and the error splits into a displacement and an amplitude part.
For output channel j of a ``DeformSpec`` (the transform of ``fss`` / ``iscale``, the same device code):

    q = the 8-bit code of y:  b = hist_bin(y, lo[j], inv_step[j], 254) in fp32;  q = b for 1 .. 254, 255 for the overflow code,
        0 for underflow and NaN.  lo is the threshold below which the field counts as empty.  Integers from here on.
    P_0 = q,  P_l = the SUMS of the 2 x 2 blocks of P_(l-1) (zeros beyond the grid), l = 1 .. F = levels
    "target X, source Y" (direction 0: X real, Y generated; direction 1 the other way round), for l = F .. 0, at every pixel p:
        init[p] = 2 d_(l+1)[p >> 1]  (0 at l = F),   Y'[x] = Y_l[x + init[x]]          everything reads 0 outside the level's grid
        cost(p, s) = sum over w in [-2, 2]^2 of (X_l[p + w] - Y'[p + w + s])^2,   s in [-2, 2]^2
        s* = the least cost; of equal costs the first in the order sorted by (sy^2 + sx^2, sy, sx): the zero shift wins every tie
        d_l[p] = s* + init[p + s*]                                                     M[p] = Y_0[p + d_0[p]] is the morphed field
    |d_0| components <= D = 2 (2^(F+1) - 1)

and the exact integer sums per (channel, direction) over all fields: the table ``disp`` of the vectors d_0[p] over the pixels with
X_0[p] > 0, n_target = #{X_0 > 0}, n_either = #{X_0 > 0 or M > 0}, sse_morphed = sum (X_0 - M)^2, sse_raw = sum (X_0 - Y_0)^2,
energy = sum X_0^2.  ``DeformResult`` forms the scores from them in Python integers.  ``Deformation`` accumulates batches in
device int64 accumulators in front of host totals kept as Python integers (drained before the accumulators could pass 2^62) and
sums them exactly over data-parallel ranks: the accumulator protocol of the trainer's diagnostics, so a trainer hook is one table
row away (there is none yet).  ``displacement_field`` returns d_0 itself, for plotting the vectors.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, fields
from .fss import allreduce_ints
from .gridstats import _jsonable
from .histograms import C_MAX, _default_ops, _f32

LEVELS_MAX, SIDE_MAX, NSCALARS = _lib.DEFORM_MAX_LEVELS, _lib.DEFORM_MAX_SIDE, _lib.DEFORM_SCALARS
WS_CAP = 512 << 20           # bytes of dg_deform workspace at most: a batch is cut into chunks of fields (at least one)
CALL_LIMIT = 1 << 62         # the most T * dg_deform_bound of one call (the library rejects more)
PIXEL_LIMIT = 1 << 31        # the most T * H * W of one call (the library rejects more)
DRAIN_LIMIT = 1 << 62        # the device accumulators are drained to the host totals before they could pass this
DEFAULT_LO, DEFAULT_STEP, DEFAULT_LEVELS = 0.5, 1.0 / 64.0, 3
SCALARS = ("n_target", "n_either", "sse_morphed", "sse_raw", "energy")
DIRECTIONS = ("real", "fake")      # the target of direction 0 and 1


def max_displacement(levels):
    """D = 2 (2^(F+1) - 1): the most a component of d_0 can be."""
    return 2 * ((2 << int(levels)) - 1)


def bound(H, W):
    """dg_deform_bound in Python integers: 255^2 H W, the most one field adds to any sum."""
    return 255 * 255 * int(H) * int(W)


class DeformSpec:
    """Units, quantiser and pyramid depth of the field-deformation verification of C input channels (+ the speed of a pair of
    them, appended as the last output).

    scale, offset: per input channel (default 1, 0); speed: the input channels (u, v) of the speed channel, or None; lo: per
    output channel (or one number), the value below which the field counts as empty; step: per output channel (or one number),
    the width of one of the 254 inner codes (the codes saturate at lo + 254 step); both rounded to fp32, the kernel uses
    inv_step = fp32(1 / step); levels: F, 1 .. LEVELS_MAX; names: one per output channel."""

    def __init__(self, C, scale=None, offset=None, speed=(0, 1), lo=DEFAULT_LO, step=DEFAULT_STEP, levels=DEFAULT_LEVELS, names=None):
        if not (isinstance(C, (int, np.integer)) and 1 <= C <= C_MAX):
            raise ValueError(f"deform takes 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"deform speed channels {speed} out of range for C = {self.C} input channels")
        self.nout = self.C + (self.speed is not None)
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"deform scale and offset need one value per input channel (C = {self.C})")
        self.lo = _f32(np.full(self.nout, lo) if np.ndim(lo) == 0 else lo, "lo")
        st = _f32(np.full(self.nout, step) if np.ndim(step) == 0 else step, "step")
        if len(self.lo) != self.nout or len(st) != self.nout:
            raise ValueError(f"deform lo and step need one value per output channel ({self.nout})")
        if not np.all(st > 0):
            raise ValueError(f"deform step must be > 0 (got {st.tolist()})")
        with np.errstate(over="ignore"):
            self.inv_step = (np.float32(1.0) / st).astype(np.float32)
        if not np.all(np.isfinite(self.inv_step) & (self.inv_step > 0)):
            raise ValueError(f"deform step {st.tolist()} has no finite positive fp32 inverse")
        if not (isinstance(levels, (int, np.integer)) and 1 <= levels <= LEVELS_MAX):
            raise ValueError(f"deform takes 1 <= levels <= {LEVELS_MAX} (got {levels!r})")
        self.levels = int(levels)
        self.D = max_displacement(self.levels)
        if names is None:
            names = [f"ch{c}" for c in range(self.C)] + (["speed"] if self.speed is not None else [])
        self.names = [str(n) for n in names]
        if len(self.names) != self.nout:
            raise ValueError(f"deform names need one entry per output channel ({self.nout})")

    @classmethod
    def zscore(cls, C, lo=DEFAULT_LO, step=DEFAULT_STEP, levels=DEFAULT_LEVELS):
        """Standardised fields: the speed of channels (0, 1) when C >= 2, the same quantiser in every channel."""
        return cls(C, speed=(0, 1) if C >= 2 else None, lo=lo, step=step, levels=levels)

    @classmethod
    def physical(cls, stats, order, lo, step, speed=("u10", "v10"), levels=DEFAULT_LEVELS):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, evaluated
        in physical units (y = x * std + mean).  lo, step: as the constructor's, in physical units; speed: the names of the
        (u, v) pair, or None."""
        order = list(order)
        sp = None if speed is None else (order.index(speed[0]), order.index(speed[1]))
        names = order + (["speed"] if sp else [])
        return cls(len(order), scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order], speed=sp, lo=lo, step=step,
                   levels=levels, names=names)

    def struct(self):
        """The dg_deform_spec of this spec (no library call)."""
        s = _lib.DeformSpec()
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.levels = self.levels
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for j in range(self.nout):
            s.lo[j], s.inv_step[j] = float(self.lo[j]), float(self.inv_step[j])
        return s

    def __eq__(self, other):
        return (isinstance(other, DeformSpec) and self.C == other.C and self.speed == other.speed and self.levels == other.levels
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("scale", "offset", "lo", "inv_step")))

    __hash__ = None


def _ratio(num, den):
    """num / den as a float, NaN when den is 0 (num a float or a Python integer)."""
    return num / den if den else math.nan


class DeformResult:
    """The exact sums of one DeformSpec on an H x W grid over ``fields`` field pairs, as Python integers: ``disp``
    [nout, 2, 2 D + 1, 2 D + 1] and the scalars [nout, 2, 5] (``SCALARS``), and what is formed from them.  Direction 0 moves the
    generated field onto the real one (the target is real), direction 1 the real field onto the generated one.  Every score is
    float64 [nout, 2] unless stated otherwise, NaN where its denominator is 0."""

    def __init__(self, spec, H, W, disp, scalars, fields):
        self.spec, self.H, self.W, self.fields = spec, int(H), int(W), int(fields)
        self.D, self.side = spec.D, 2 * spec.D + 1
        self._disp = np.empty((spec.nout, 2, self.side, self.side), dtype=object)
        self._disp.reshape(-1)[:] = [int(v) for v in np.asarray(disp, dtype=object).reshape(-1)]
        self._scalars = np.empty((spec.nout, 2, NSCALARS), dtype=object)
        self._scalars.reshape(-1)[:] = [int(v) for v in np.asarray(scalars, dtype=object).reshape(-1)]
        ax = np.arange(-self.D, self.D + 1)
        self._dy, self._dx = np.meshgrid(ax, ax, indexing="ij")
        self._r2 = self._dy * self._dy + self._dx * self._dx

    def sums(self):
        """(disp, scalars): Python-int arrays [nout, 2, 2 D + 1, 2 D + 1] and [nout, 2, 5]."""
        return self._disp.copy(), self._scalars.copy()

    def scalar(self, name):
        """Python-int array [nout, 2] of one of ``SCALARS``."""
        return self._scalars[..., SCALARS.index(name)].copy()

    def _each(self, f, shape=()):
        out = np.full((self.spec.nout, 2) + shape, np.nan, dtype=np.float64)
        for j, d in np.ndindex(self.spec.nout, 2):
            out[j, d] = f(self._disp[j, d], [int(v) for v in self._scalars[j, d]])
        return out

    def rose(self):
        """The displacement table [nout, 2, 2 D + 1, 2 D + 1] (index dy + D, dx + D): int64, or Python integers beyond it."""
        big = any(int(v) >= 1 << 63 for v in self._disp.reshape(-1))
        return self._disp.copy() if big else self._disp.astype(np.int64)

    def _weighted(self, table, w):
        """sum table * w with the counts as Python integers and w float64 (exact where w is integral and small)."""
        return math.fsum(int(c) * float(x) for c, x in zip(table.reshape(-1), w.reshape(-1)) if c)

    def dis(self):
        """The mean length of the displacement vectors over the target's non-empty pixels, in pixels."""
        r = np.sqrt(self._r2.astype(np.float64))
        return self._each(lambda t, s: _ratio(self._weighted(t, r), s[0]))

    def mean_vector(self):
        """float64 [nout, 2, 2]: the mean (dy, dx), the systematic shift."""
        def f(t, s):
            sy = sum(int(c) * int(y) for c, y in zip(t.reshape(-1), self._dy.reshape(-1)) if c)
            sx = sum(int(c) * int(x) for c, x in zip(t.reshape(-1), self._dx.reshape(-1)) if c)
            return [_ratio(sy, s[0]), _ratio(sx, s[0])]
        return self._each(f, (2,))

    def modal_vector(self):
        """float64 [nout, 2, 2]: the most frequent (dy, dx); of equal counts the shortest, then the first in (dy, dx) order."""
        def f(t, s):
            if not s[0]:
                return [math.nan, math.nan]
            flat = t.reshape(-1)
            best = max(range(flat.size), key=lambda i: (int(flat[i]), -int(self._r2.reshape(-1)[i]), -i))
            return [float(self._dy.reshape(-1)[best]), float(self._dx.reshape(-1)[best])]
        return self._each(f, (2,))

    def displacement_quantile(self, q):
        """The smallest length |d| with at least the fraction ``q`` of the target's non-empty pixels at or below it."""
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError(f"a quantile is between 0 and 1 (got {q!r})")
        order = np.argsort(self._r2.reshape(-1), kind="stable")

        def f(t, s):
            if not s[0]:
                return math.nan
            flat, cum = t.reshape(-1), 0
            for i in order:
                cum += int(flat[i])
                if cum and cum >= float(q) * s[0]:
                    return math.sqrt(float(self._r2.reshape(-1)[i]))
            return math.sqrt(float(self._r2.max()))
        return self._each(f)

    def _inv_step(self, j):
        return float(self.spec.inv_step[j])

    def _rms(self, num_index, den_index):
        out = np.full((self.spec.nout, 2), np.nan)
        for j, d in np.ndindex(self.spec.nout, 2):
            s = [int(v) for v in self._scalars[j, d]]
            if s[den_index]:
                out[j, d] = math.sqrt(s[num_index] / s[den_index]) / self._inv_step(j)
        return out

    def amp(self):
        """sqrt(sse_morphed / n_either) / inv_step: the RMS error left after the morphing, in the field's units."""
        return self._rms(2, 1)

    def amp_raw(self):
        """sqrt(sse_raw / n_either) / inv_step: the same before the morphing."""
        return self._rms(3, 1)

    def explained(self):
        """1 - sse_morphed / sse_raw: the part of the squared error that the displacement explains."""
        return self._each(lambda t, s: 1.0 - s[2] / s[3] if s[3] else math.nan)

    def _combined(self, per_direction, weight_index):
        out = np.full(self.spec.nout, np.nan)
        for j in range(self.spec.nout):
            n = [int(self._scalars[j, d, weight_index]) for d in range(2)]
            if n[0] + n[1]:
                out[j] = sum(n[d] * per_direction[j, d] for d in range(2) if n[d]) / (n[0] + n[1])
        return out

    def dis_combined(self):
        """float64 [nout]: DIS = (n_0 dis_0 + n_1 dis_1) / (n_0 + n_1) with the n_target weights."""
        return self._combined(self.dis(), 0)

    def amp_combined(self):
        """float64 [nout]: AMP = (n_0 amp_0 + n_1 amp_1) / (n_0 + n_1) with the n_either weights."""
        return self._combined(self.amp(), 1)

    def i0(self):
        """float64 [nout]: the RMS of the real field over its non-empty pixels, sqrt(energy_0 / n_target_0) / inv_step."""
        out = np.full(self.spec.nout, np.nan)
        for j in range(self.spec.nout):
            n, e = int(self._scalars[j, 0, 0]), int(self._scalars[j, 0, 4])
            if n:
                out[j] = math.sqrt(e / n) / self._inv_step(j)
        return out

    def das(self, d_max=None, i0=None):
        """float64 [nout]: DAS = DIS / d_max + AMP / I0; d_max defaults to D, I0 to ``i0()``; NaN where a denominator is 0."""
        d_max = float(self.D) if d_max is None else float(d_max)
        i0 = self.i0() if i0 is None else np.broadcast_to(np.asarray(i0, dtype=np.float64), (self.spec.nout,))
        dis, amp = self.dis_combined(), self.amp_combined()
        out = np.full(self.spec.nout, np.nan)
        for j in range(self.spec.nout):
            if d_max and i0[j] and not math.isnan(i0[j]):
                out[j] = dis[j] / d_max + amp[j] / i0[j]
        return out

    def summary(self):
        """A JSON-serialisable dict (None where undefined); the exact integers are kept as integers.  The displacement table
        is given sparsely: [dy, dx, count] of its non-zero bins."""
        rose = [[[[int(y), int(x), int(t[y + self.D, x + self.D])] for y, x in zip(self._dy.reshape(-1), self._dx.reshape(-1))
                  if t[y + self.D, x + self.D]] for t in per_j] for per_j in self._disp]
        return {"channels": list(self.spec.names), "fields": self.fields, "grid": [self.H, self.W], "levels": self.spec.levels,
                "max_displacement": self.D, "directions": list(DIRECTIONS),
                "lo": _jsonable(self.spec.lo), "inv_step": _jsonable(self.spec.inv_step),
                "dis": _jsonable(self.dis()), "amp": _jsonable(self.amp()), "amp_raw": _jsonable(self.amp_raw()),
                "explained": _jsonable(self.explained()), "mean_vector": [_jsonable(a) for a in self.mean_vector()],
                "modal_vector": [_jsonable(a) for a in self.modal_vector()],
                "median_displacement": _jsonable(self.displacement_quantile(0.5)),
                "dis_combined": _jsonable(self.dis_combined()), "amp_combined": _jsonable(self.amp_combined()),
                "i0": _jsonable(self.i0()), "das": _jsonable(self.das()),
                "scalars": {name: [[int(v) for v in row] for row in self._scalars[..., i]] for i, name in enumerate(SCALARS)},
                "rose": rose}


def _grid(H, W, owner):
    H, W = int(H), int(W)
    if not (1 <= H <= SIDE_MAX and 1 <= W <= SIDE_MAX):
        raise ValueError(f"{owner} needs a grid of 1 <= H, W <= {SIDE_MAX} (got {H} x {W})")
    return H, W


def _chunk(o, a, n, H, W, struct, limit):
    """Fields per call: the workspace cap, the pixel limit and the per-call headroom (at least one)."""
    _, f1 = fields.descriptor(o, a.x[:1], a.nhwc, a.C)
    per_field = max(1, o.deform_ws_bytes(f1, H, W, struct))
    return max(1, min(n, WS_CAP // per_field, PIXEL_LIMIT // (H * W), limit // bound(H, W)))


class Deformation:
    """Running field-deformation sums of the (real, generated) field pairs added so far on an H x W grid: device int64
    accumulators in front of host totals kept as Python integers."""

    def __init__(self, spec, H, W, device=None, ops=None):
        if not isinstance(spec, DeformSpec):
            raise TypeError(f"Deformation takes a DeformSpec (got {type(spec).__name__})")
        self.H, self.W = _grid(H, W, "Deformation")
        self.spec = spec
        self._bound = bound(self.H, self.W)
        self.device = torch.device("cuda:0" if device is None else device)
        self._ops = ops
        side = 2 * spec.D + 1
        self._dev_disp = torch.zeros(spec.nout, 2, side * side, dtype=torch.int64, device=self.device)
        self._dev_scalars = torch.zeros(spec.nout, 2, NSCALARS, dtype=torch.int64, device=self.device)
        self._dev_bound = 0                                          # the most a device sum can hold now (host mirror: no sync)
        self._disp = [0] * self._dev_disp.numel()                    # host totals
        self._scalars = [0] * self._dev_scalars.numel()
        self.fields = 0
        self.drains = 0
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    def _drain(self):
        """Move the device accumulators into the host totals (one synchronising copy each) and zero them."""
        for dev, host in ((self._dev_disp, self._disp), (self._dev_scalars, self._scalars)):
            for i, v in enumerate(dev.reshape(-1).cpu().tolist()):
                host[i] += v
            dev.zero_()
        self._dev_bound = 0
        self.drains += 1

    def add(self, real, fake, n_valid=None, nhwc=False, channels=None):
        """Add the first ``n_valid`` (default: all) field pairs of a batch.  Layouts as ``histograms.histogram`` ([T, C, H, W];
        with ``nhwc`` a [T, H, W, c_pad] store of which the leading ``channels`` are read; a ``NativeBatch``); the two series
        may differ in layout and dtype: pass ``nhwc`` as a pair (real, fake) then."""
        a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "deform", self.spec, "Deformation", (self.H, self.W))
        if self._struct is None:
            self._struct = self.spec.struct()
        o, mb = self.ops, self._bound
        limit = min(DRAIN_LIMIT, CALL_LIMIT)
        tc = _chunk(o, a, n, self.H, self.W, self._struct, limit)
        for t0 in range(0, n, tc):
            m = min(tc, n - t0)
            if self._dev_bound and self._dev_bound + m * mb > limit:
                self._drain()
            ka, fa = fields.descriptor(o, a.x[t0:t0 + m], a.nhwc, a.C)
            kb, fb = fields.descriptor(o, b.x[t0:t0 + m], b.nhwc, b.C)
            o.deform(fa, fb, self.H, self.W, self._struct, self._dev_disp, self._dev_scalars)
            self._dev_bound += m * mb
        self.fields += n
        return self

    def reduce_(self, dist):
        """Sum the totals exactly over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place."""
        if dist is not None and dist.world_size > 1:
            self._drain()
            dev = self.device if getattr(dist, "backend", "gloo") == "nccl" else "cpu"
            vals = allreduce_ints(dist, self._disp + self._scalars + [self.fields], dev)
            nd = len(self._disp)
            self._disp, self._scalars, self.fields = vals[:nd], vals[nd:-1], vals[-1]
        return self

    def result(self):
        """The ``DeformResult`` of every pair added (and, after ``reduce_``, of every rank)."""
        if self._dev_bound:
            self._drain()
        return DeformResult(self.spec, self.H, self.W, list(self._disp), list(self._scalars), self.fields)


def _spec_of(spec, Cn, what):
    if spec is None:
        spec = DeformSpec.zscore(Cn)
    if not isinstance(spec, DeformSpec):
        raise TypeError(f"{what} takes a DeformSpec (got {type(spec).__name__})")
    return spec


def deformation(real, fake, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """Field-deformation verification of a (real, generated) pair of series of fields on the GPU -> ``DeformResult``.  spec None:
    ``DeformSpec.zscore`` of the fields' channels; the other arguments as ``Deformation.add``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "deform")
    acc = Deformation(_spec_of(spec, Cn, "deformation"), H, W, device=device, ops=ops)
    return acc.add(real, fake, n_valid=n_valid, nhwc=nhwc, channels=channels).result()


def displacement_field(real, fake, spec=None, n_valid=None, nhwc=False, channels=None, ops=None, morphed=False):
    """The displacement fields d_0 of a (real, generated) pair of series -> int16 tensor [n, nout, 2, 2, H, W] on the fields'
    device: direction (0: the generated field moved onto the real one, 1: the other way round), then (dy, dx); the source pixel
    of target pixel (h, w) is (h + dy, w + dx).  With ``morphed`` also the moved quantised source, uint8 [n, nout, 2, H, W]
    -> (field, morphed).  The other arguments as ``deformation``."""
    Cn, H, W, device = fields.one_shot(real, nhwc, channels, "deform")
    spec = _spec_of(spec, Cn, "displacement_field")
    H, W = _grid(H, W, "displacement_field")
    a, b, n = fields.batch(real, fake, nhwc, channels, n_valid, "deform", spec, "displacement_field", (H, W))
    o = _default_ops(torch.device(device)) if ops is None else ops
    struct = spec.struct()
    out = torch.empty(n, spec.nout, 2, 2, H, W, dtype=torch.int16, device=a.x.device)
    mor = torch.empty(n, spec.nout, 2, H, W, dtype=torch.uint8, device=a.x.device) if morphed else None
    tc = _chunk(o, a, n, H, W, struct, CALL_LIMIT)
    for t0 in range(0, n, tc):
        m = min(tc, n - t0)
        ka, fa = fields.descriptor(o, a.x[t0:t0 + m], a.nhwc, a.C)
        kb, fb = fields.descriptor(o, b.x[t0:t0 + m], b.nhwc, b.C)
        o.deform_field(fa, fb, H, W, struct, out[t0:t0 + m], None if mor is None else mor[t0:t0 + m])
    return (out, mor) if morphed else out
