"""Joint (2-D) histograms of real and generated fields on the GPU (csrc/joint.hip): wind roses and real-vs-generated densities.

The one-quantity diagnostics (``histograms``, ``gridstats``) cannot say whether the generator reproduces the wind rose (the
joint distribution of direction and speed: the marginals of u, v and the speed can all match while the prevailing wind is
turned by 30 degrees), nor what it produces GIVEN the real value (conditional bias and spread, how much of the truth survives).
Both are 2-D histograms over the same fields.

Two series of fields of equal T, C, P: ``a`` (the real fields, or the only series) and optionally ``b`` (the generated ones).
One transform serves both, every step one correctly rounded fp32 operation (the code of ``histograms``):

    y_c = fp32(fp32(x_c * scale_c) + offset_c)
    s   = sqrt_rn(fp32(fp32(y_u * y_u) + fp32(y_v * y_v)))      the speed of the pair ``speed`` = (u, v)

An AXIS is (source a | b, channel, bins, lo, hi).  Channel 0 .. C-1 is a component, "speed" the speed, "direction" the
direction.  Component and speed axes use the 1-D bin rule of ``histograms`` (inv_w = fp32(bins / (hi - lo)) rounded once from
float64; t = fp32(fp32(y - lo) * inv_w)): index 0 underflow, 1 .. bins interior, bins + 1 overflow, bins + 2 NaN.

The DIRECTION axis has bins = nsec sectors in the meteorological convention: the direction the wind comes FROM, clockwise from
north, sector 0 centred on north.  nsec is a multiple of 4 in 4 .. 72, shared by all direction axes of a spec; K = nsec / 4;
``calm`` is an fp32 value, finite and >= 0; t_k = fp32(tan(k pi / (4 K))), k = 1 .. K-1, rounded once from float64.  atan2 is not
correctly rounded, so the rule uses compares of single rounded products, in this order:

    1. y_u or y_v NaN -> index nsec + 2
    2. not (s > calm) -> index 0 (calm); index nsec + 1 is never used
    3. x = -y_u, y = -y_v, ax = |x|, ay = |y|, swap = ax > ay
    4. m = swap ? ay : ax,  M = swap ? ax : ay
    5. j = #{k in 1 .. K-1 : m >= fp32(M * t_k)}
    6. q = swap ? 2K - 1 - j : j
    7. half sector h = q if x >= 0 and y > 0;  4K - 1 - q if x > 0 and y <= 0;  4K + q if x <= 0 and y < 0;
       8K - 1 - q if x < 0 and y >= 0
    8. sector = ((h + 1) >> 1) mod nsec, index = 1 + sector

A PAIR is two axes (X, Y); its table is int64 [bins_x + 3, bins_y + 3], row-major, X first, at most CELLS_MAX cells; a spec holds
at most PAIRS_MAX pairs.  Because every axis uses the 1-D rule, the marginals of a table equal the ``histograms`` counts of the
same axis exactly.  Counts are exact and two calls are bit-identical (integer LDS and global atomics only); the statistics are
derived on the host in float64 from the counts alone, with the bin-width error each docstring states.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib, fields
from .histograms import C_MAX, _f32

PAIRS_MAX = _lib.HIST2D_MAX_PAIRS
CELLS_MAX = _lib.HIST2D_MAX_CELLS
SECTORS_MAX = _lib.HIST2D_MAX_SECTORS

_ops = {}                    # device -> op backend of the module-level calls


def _default_ops(device):
    return fields.default_ops(_ops, device)


class Axis:
    """One axis of a pair: ``source`` "a" / "b" (or 0 / 1), ``channel`` an int (a component), "speed" or "direction", ``bins``
    interior bins on [lo, hi) (a direction axis: bins = nsec sectors, no lo / hi)."""

    def __init__(self, source, channel, bins, lo=None, hi=None):
        if source not in ("a", "b", 0, 1):
            raise ValueError(f"axis source must be 'a' / 'b' or 0 / 1 (got {source!r})")
        self.source = int({"a": 0, "b": 1}.get(source, source))
        if not (channel in ("speed", "direction") or (isinstance(channel, (int, np.integer)) and not isinstance(channel, bool)
                                                       and channel >= 0)):
            raise ValueError(f"axis channel must be a channel index >= 0, 'speed' or 'direction' (got {channel!r})")
        self.channel = channel if isinstance(channel, str) else int(channel)
        if not (isinstance(bins, (int, np.integer)) and 1 <= bins <= CELLS_MAX):
            raise ValueError(f"axis bins must be an integer >= 1 (got {bins!r})")
        self.bins = int(bins)
        if self.channel == "direction":
            if lo is not None or hi is not None:
                raise ValueError(f"a direction axis takes no lo / hi (got lo = {lo!r}, hi = {hi!r})")
            if self.bins % 4 or not 4 <= self.bins <= SECTORS_MAX:
                raise ValueError(f"direction sectors must be a multiple of 4 in [4, {SECTORS_MAX}] (got {self.bins})")
            self.lo = self.hi = self.inv_w = None
        else:
            if lo is None or hi is None:
                raise ValueError(f"axis {self.channel!r} needs lo and hi")
            self.lo, self.hi = _f32(lo, "lo")[0], _f32(hi, "hi")[0]
            if not self.lo < self.hi:
                raise ValueError(f"axis needs lo < hi (got lo = {float(self.lo)}, hi = {float(self.hi)})")
            inv_w = self.bins / (float(self.hi) - float(self.lo))
            with np.errstate(over="ignore", under="ignore"):
                self.inv_w = np.float32(inv_w)
            if not (np.isfinite(self.inv_w) and self.inv_w > 0):
                raise ValueError(f"axis bin width out of fp32 range: bins / (hi - lo) = {inv_w}")

    @property
    def is_direction(self):
        return self.channel == "direction"

    def width(self):
        """The nominal bin width (hi - lo) / bins; a direction axis: the sector width in degrees."""
        return 360.0 / self.bins if self.is_direction else (float(self.hi) - float(self.lo)) / self.bins

    def centres(self):
        """float64 [bins]: the centres of the interior bins; a direction axis: the sector centres in degrees (0 = north,
        90 = east)."""
        if self.is_direction:
            return np.arange(self.bins) * self.width()
        return float(self.lo) + (np.arange(self.bins) + 0.5) * self.width()

    def _key(self):
        return (self.source, self.channel, self.bins, None if self.lo is None else float(self.lo),
                None if self.hi is None else float(self.hi))

    def __eq__(self, other):
        return isinstance(other, Axis) and self._key() == other._key()

    __hash__ = None

    def __repr__(self):
        return f"Axis{self._key()}"


class JointSpec:
    """The pairs, units and direction rule of the joint histograms of C input channels.

    pairs: 1 .. PAIRS_MAX (X, Y) tuples of ``Axis``; scale, offset: per input channel (default 1, 0), one transform for both
    series; speed: the input channels (u, v) of the speed and the direction, or None (then no axis may use them); calm: the
    speed up to which the wind has no direction (fp32, finite, >= 0); names: one per pair."""

    def __init__(self, pairs, C, scale=None, offset=None, speed=(0, 1), calm=0.0, names=None):
        if not (isinstance(C, (int, np.integer)) and 1 <= C <= C_MAX):
            raise ValueError(f"joint histograms take 1 <= C <= {C_MAX} input channels (got C = {C!r})")
        self.C = int(C)
        self.speed = None if speed is None else tuple(int(s) for s in speed)
        if self.speed is not None and (len(self.speed) != 2 or not all(0 <= s < self.C for s in self.speed)):
            raise ValueError(f"joint speed channels {speed} out of range for C = {self.C} input channels")
        self.scale = _f32(np.ones(self.C) if scale is None else scale, "scale")
        self.offset = _f32(np.zeros(self.C) if offset is None else offset, "offset")
        if len(self.scale) != self.C or len(self.offset) != self.C:
            raise ValueError(f"joint scale and offset need one value per input channel (C = {self.C})")
        self.calm = _f32(calm, "calm")[0]
        if not self.calm >= 0:
            raise ValueError(f"joint calm threshold must be >= 0 (got {float(self.calm)})")
        pairs = [tuple(p) for p in pairs]
        if not 1 <= len(pairs) <= PAIRS_MAX:
            raise ValueError(f"a JointSpec holds 1 .. {PAIRS_MAX} pairs (got {len(pairs)})")
        self.nsec = 0
        for i, p in enumerate(pairs):
            if len(p) != 2 or not all(isinstance(ax, Axis) for ax in p):
                raise TypeError(f"pair {i} must be two Axis objects (got {p!r})")
            for ax in p:
                if isinstance(ax.channel, int) and ax.channel >= self.C:
                    raise ValueError(f"pair {i}: channel {ax.channel} does not exist (C = {self.C})")
                if isinstance(ax.channel, str) and self.speed is None:
                    raise ValueError(f"pair {i}: a {ax.channel} axis needs a speed pair (speed = None)")
                if ax.is_direction:
                    if self.nsec and ax.bins != self.nsec:
                        raise ValueError(f"pair {i}: all direction axes share one sector count (got {ax.bins} and {self.nsec})")
                    self.nsec = ax.bins
            cells = (p[0].bins + 3) * (p[1].bins + 3)
            if cells > CELLS_MAX:
                raise ValueError(f"pair {i}: ({p[0].bins} + 3) x ({p[1].bins} + 3) = {cells} cells exceed {CELLS_MAX}")
        self.pairs = pairs
        K = self.nsec // 4
        self.tan_k = np.zeros(SECTORS_MAX // 4, dtype=np.float32)          # tan_k[k], k = 1 .. K-1; entry 0 is not read
        for k in range(1, K):
            self.tan_k[k] = np.float32(math.tan(k * math.pi / (4 * K)))
        if names is None:
            names = [f"pair{i}" for i in range(len(pairs))]
        self.names = [str(n) for n in names]
        if len(self.names) != len(pairs):
            raise ValueError(f"joint names need one entry per pair ({len(pairs)})")

    @property
    def npairs(self):
        return len(self.pairs)

    @property
    def uses_b(self):
        return any(ax.source == 1 for p in self.pairs for ax in p)

    @classmethod
    def zscore(cls, C, bins=96, lim=6.0, nsec=36, speed_bins=64):
        """Standardised fields.  C >= 2: the roses (direction x speed) of a and of b, the (u, v) densities of a and of b, then
        the real-vs-generated densities (a_j, b_j) of every component and of the speed -- dropped from the end beyond PAIRS_MAX
        pairs.  Components on [-lim, lim], the speed of channels (0, 1) on [0, lim * sqrt 2].  C = 1: the (a_0, b_0) density."""
        comp = lambda src, c: Axis(src, c, bins, -lim, lim)
        if C < 2:
            return cls([(comp("a", 0), comp("b", 0))], C, speed=None, names=["ch0"])
        spd = lambda src: Axis(src, "speed", speed_bins, 0.0, lim * math.sqrt(2.0))
        pairs = [(Axis("a", "direction", nsec), spd("a")), (Axis("b", "direction", nsec), spd("b")),
                 (comp("a", 0), comp("a", 1)), (comp("b", 0), comp("b", 1))]
        names = ["rose_real", "rose_fake", "uv_real", "uv_fake"]
        pairs += [(comp("a", c), comp("b", c)) for c in range(C)] + [(spd("a"), spd("b"))]
        names += [f"ch{c}" for c in range(C)] + ["speed"]
        return cls(pairs[:PAIRS_MAX], C, speed=(0, 1), names=names[:PAIRS_MAX])

    @classmethod
    def physical(cls, stats, order, lo, hi, bins=96, nsec=36, speed_bins=64, speed=("u10", "v10"), calm=0.5):
        """Fields standardised with ``stats`` ({name: (mean, std)}, GAN/preprocess.field_stats) in channel ``order``, binned in
        physical units (y = x * std + mean): the pairs of ``zscore`` with the components on [lo, hi] (scalars), the speed on
        [0, max(|lo|, |hi|) * sqrt 2] and winds up to ``calm`` (physical units) without a direction.  speed: the names of the
        (u, v) pair, or None (then only the real-vs-generated densities of the components)."""
        order = list(order)
        C = len(order)
        comp = lambda src, c: Axis(src, c, bins, float(lo), float(hi))
        kw = dict(scale=[stats[n][1] for n in order], offset=[stats[n][0] for n in order])
        if speed is None:
            return cls([(comp("a", c), comp("b", c)) for c in range(C)][:PAIRS_MAX], C, speed=None, names=order[:PAIRS_MAX], **kw)
        u, v = order.index(speed[0]), order.index(speed[1])
        top = max(abs(float(lo)), abs(float(hi))) * math.sqrt(2.0)
        spd = lambda src: Axis(src, "speed", speed_bins, 0.0, top)
        pairs = [(Axis("a", "direction", nsec), spd("a")), (Axis("b", "direction", nsec), spd("b")),
                 (comp("a", u), comp("a", v)), (comp("b", u), comp("b", v))]
        names = ["rose_real", "rose_fake", "uv_real", "uv_fake"]
        pairs += [(comp("a", c), comp("b", c)) for c in range(C)] + [(spd("a"), spd("b"))]
        names += order + ["speed"]
        return cls(pairs[:PAIRS_MAX], C, speed=(u, v), calm=calm, names=names[:PAIRS_MAX], **kw)

    def table_shapes(self):
        """[(bins_x + 3, bins_y + 3)] per pair."""
        return [(p[0].bins + 3, p[1].bins + 3) for p in self.pairs]

    def offsets(self):
        """int [npairs + 1]: the first cell of every pair's table in the concatenated counts, then their total."""
        return [0] + np.cumsum([a * b for a, b in self.table_shapes()]).tolist()

    def _chan(self, ax):
        return self.C if ax.channel == "speed" else self.C + 1 if ax.channel == "direction" else ax.channel

    def struct(self):
        """The dg_hist2d_spec of this spec (no library call)."""
        s = _lib.Hist2dSpec()
        s.npairs = self.npairs
        s.speed_u, s.speed_v = self.speed if self.speed is not None else (-1, -1)
        s.nsec = self.nsec
        s.calm = float(self.calm)
        for k in range(len(self.tan_k)):
            s.tan_k[k] = float(self.tan_k[k])
        for c in range(self.C):
            s.scale[c], s.offset[c] = float(self.scale[c]), float(self.offset[c])
        for i, p in enumerate(self.pairs):
            for e, ax in enumerate(p):
                d = s.ax[i][e]
                d.src, d.chan, d.nbins = ax.source, self._chan(ax), ax.bins
                d.lo, d.inv_w = (0.0, 1.0) if ax.is_direction else (float(ax.lo), float(ax.inv_w))
        return s

    def __eq__(self, other):
        return (isinstance(other, JointSpec) and self.C == other.C and self.speed == other.speed and self.pairs == other.pairs
                and float(self.calm) == float(other.calm)
                and all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("scale", "offset")))

    __hash__ = None


def host_bins(spec, xa, xb=None):
    """int32 [npairs, 2, n]: the X and the Y index of each point of xa (and xb; fp32 [C, n], planar) under every pair of
    ``spec``, computed by the library on the host (dg_hist2d_host_bins: the code the kernel runs)."""
    if not isinstance(spec, JointSpec):
        raise TypeError(f"host_bins takes a JointSpec (got {type(spec).__name__})")
    xa = np.ascontiguousarray(xa, dtype=np.float32)
    if xa.ndim != 2 or xa.shape[0] != spec.C:
        raise ValueError(f"host_bins takes [C = {spec.C}, n] values (got shape {xa.shape})")
    if xb is not None:
        xb = np.ascontiguousarray(xb, dtype=np.float32)
        if xb.shape != xa.shape:
            raise ValueError(f"host_bins: the two series differ in shape ({xa.shape} and {xb.shape})")
    elif spec.uses_b:
        raise ValueError("host_bins: the spec has an axis of series b but xb is None")
    out = np.empty((spec.npairs, 2, xa.shape[1]), dtype=np.int32)
    s = spec.struct()
    _lib.check(_lib.lib().dg_hist2d_host_bins(ctypes.byref(s), xa.ctypes.data, None if xb is None else xb.ctypes.data, spec.C,
                                              xa.shape[1], out.ctypes.data), "dg_hist2d_host_bins")
    return out


def _norm(t):
    n = t.sum()
    return t / n if n > 0 else np.full(t.shape, np.nan)


def _tv(p, q):
    return 0.5 * float(np.abs(p - q).sum())


def _js(p, q):
    m = 0.5 * (p + q)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = lambda a: float(np.where(a > 0, a * np.log(a / m), 0.0).sum())
        return 0.5 * kl(p) + 0.5 * kl(q)


class Joint:
    """The tables of a JointSpec: ``counts`` int64, the [bins_x + 3, bins_y + 3] tables concatenated in pair order (a device or
    host tensor), and the number of fields.  Pairs are addressed by index or by name.  The statistics are computed on the host in
    float64 from the counts alone; "finite cells" are those outside the NaN row and column (under- and overflow included),
    "interior" the bins 1 .. bins of an axis."""

    def __init__(self, spec, counts, fields):
        self.spec, self.counts, self.fields = spec, counts, int(fields)
        self._h = None

    def host(self):
        """The concatenated counts as one int64 numpy array (copied once)."""
        if self._h is None:
            self._h = self.counts.detach().cpu().numpy().copy()
        return self._h

    def index(self, p):
        if isinstance(p, str):
            if p not in self.spec.names:
                raise KeyError(f"no pair named {p!r} (pairs: {self.spec.names})")
            return self.spec.names.index(p)
        if not 0 <= int(p) < self.spec.npairs:
            raise IndexError(f"pair {p} of {self.spec.npairs}")
        return int(p)

    def table(self, p):
        """int64 [bins_x + 3, bins_y + 3] of pair p."""
        i = self.index(p)
        o = self.spec.offsets()
        return self.host()[o[i]:o[i + 1]].reshape(self.spec.table_shapes()[i])

    def marginals(self, p):
        """(int64 [bins_x + 3], int64 [bins_y + 3]): the 1-D counts of the X and of the Y axis of pair p -- for a component or
        speed axis exactly the ``histograms`` counts of that channel under the same bins."""
        t = self.table(p)
        return t.sum(axis=1), t.sum(axis=0)

    def _interior(self, p):
        i = self.index(p)
        X, Y = self.spec.pairs[i]
        return X, Y, self.table(i)[1:X.bins + 1, 1:Y.bins + 1].astype(np.float64)

    def conditional_mean(self, p):
        """float64 [bins_x]: the mean of Y given that X falls into each interior X bin, over the interior Y bins, every count
        placed at its bin centre (NaN for an empty row).  Error: at most half a Y bin width."""
        X, Y, t = self._interior(p)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (t * Y.centres()[None, :]).sum(axis=1) / t.sum(axis=1)

    def conditional_std(self, p):
        """float64 [bins_x]: the population standard deviation of Y per interior X bin, counts at the Y bin centres.  Error: the
        variance carries the within-bin variance w_y^2 / 12 at most (no Sheppard correction is applied)."""
        X, Y, t = self._interior(p)
        m = self.conditional_mean(p)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = Y.centres()[None, :] - m[:, None]
            return np.sqrt((t * d * d).sum(axis=1) / t.sum(axis=1))

    def conditional_quantile(self, p, q):
        """float64 [bins_x, len(q)] ([bins_x] for a scalar q): per interior X bin the first interior Y bin whose cumulative
        count reaches q * n, interpolated linearly inside it, as ``Histogram.quantile`` (NaN for an empty row).  Error: one Y
        bin width."""
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
        if np.any((qs < 0) | (qs > 1)) or np.any(np.isnan(qs)):
            raise ValueError(f"quantile levels must lie in [0, 1] (got {qs.tolist()})")
        X, Y, t = self._interior(p)
        w = Y.width()
        left = Y.centres() - 0.5 * w
        out = np.full((X.bins, len(qs)), np.nan)
        for r in range(X.bins):
            n = t[r].sum()
            if n == 0:
                continue
            cum = np.cumsum(t[r])
            for k, qk in enumerate(qs):
                m = qk * n
                i = min(int(np.searchsorted(cum, m, side="left")), Y.bins - 1)
                while t[r, i] == 0:                     # q = 0: the first occupied bin
                    i += 1
                prev = cum[i - 1] if i > 0 else 0.0
                out[r, k] = left[i] + (m - prev) / t[r, i] * w
        return out[:, 0] if np.ndim(q) == 0 else out

    def conditional_bias(self, p):
        """float64 [bins_x]: conditional_mean minus the X bin centre -- for a real-vs-generated pair (X real, Y generated) how
        far the generator is off given the real value.  Error: half an X plus half a Y bin width."""
        X, Y, _ = self._interior(p)
        if X.is_direction or Y.is_direction:
            raise ValueError("conditional_bias is defined for component and speed axes")
        return self.conditional_mean(p) - X.centres()

    def mutual_information(self, p):
        """The mutual information of the binned X and Y in nats over the finite cells.  Error: binning can only lose
        information (the value is a lower bound of the continuous MI up to the O(cells / n) small-sample bias upwards)."""
        P = _norm(self.table(p)[:-1, :-1].astype(np.float64))
        px, py = P.sum(axis=1, keepdims=True), P.sum(axis=0, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.where(P > 0, P * np.log(P / (px * py)), 0.0).sum())

    def _dir_axis(self, p):
        i = self.index(p)
        for e, ax in enumerate(self.spec.pairs[i]):
            if ax.is_direction:
                return i, e
        raise ValueError(f"pair {self.spec.names[i]!r} has no direction axis")

    def rose(self, p):
        """(calm, freq): of a (direction, speed) pair the fraction of the finite points that are calm and the frequencies
        float64 [nsec, speed bins] of the others (fractions of the finite points; calm + freq.sum() = 1 when no speed falls
        outside its axis).  Error: none in the counts; a point within one fp32 rounding of a sector boundary may sit in the
        neighbouring sector."""
        i, e = self._dir_axis(p)
        if e != 0 or self.spec.pairs[i][1].is_direction:
            raise ValueError("rose takes a pair with the direction on X and a speed or component on Y")
        t = self.table(i)[:-1, :-1].astype(np.float64)
        n = t.sum()
        if n == 0:
            return math.nan, np.full((t.shape[0] - 2, t.shape[1] - 2), np.nan)
        return float(t[0].sum() / n), t[1:-1, 1:-1] / n

    def direction_frequencies(self, p):
        """float64 [nsec]: the fraction of the finite points whose wind comes from each sector (the calm fraction is the rest)."""
        i, e = self._dir_axis(p)
        t = self.table(i)[:-1, :-1].astype(np.float64)
        m = t.sum(axis=1 - e)
        return m[1:-1] / m.sum() if m.sum() > 0 else np.full(len(m) - 2, np.nan)

    def _two(self, p, q, other):
        a, b = self.table(p), (self if other is None else other).table(q)
        if a.shape != b.shape:
            raise ValueError(f"the two tables differ in shape ({a.shape} and {b.shape})")
        return _norm(a[:-1, :-1].astype(np.float64)), _norm(b[:-1, :-1].astype(np.float64))

    def tv_distance(self, p, q, other=None):
        """The total-variation distance 1/2 sum |P - Q| of the finite cells of table p and table q (of ``other``, default this
        Joint), each normalised: 0 for identical, 1 for disjoint tables.  Error: differences inside a cell are not seen."""
        return _tv(*self._two(p, q, other))

    def js_divergence(self, p, q, other=None):
        """The Jensen-Shannon divergence in nats (<= ln 2) of the same two normalised tables.  Error: as tv_distance."""
        return _js(*self._two(p, q, other))

    def summary(self, q=(0.05, 0.5, 0.95, 0.99)):
        """JSON-serialisable: pair names, field count, and -- for the pairs the spec holds -- the calm fractions of the real and
        generated roses, the direction and rose TV distances, the (u, v) JS divergence, and per real-vs-generated pair the
        mutual information and the conditional bias at the X bins holding the real q-quantiles."""
        sp = self.spec
        roses, uv, rf = {}, {}, []
        for i, (X, Y) in enumerate(sp.pairs):
            if X.is_direction and Y.channel == "speed" and X.source == Y.source:
                roses.setdefault(X.source, i)
            elif sp.speed is not None and X.source == Y.source and (X.channel, Y.channel) == sp.speed:
                uv.setdefault(X.source, i)
            elif (X.source, Y.source) == (0, 1) and X.channel == Y.channel and not X.is_direction:
                rf.append(i)
        out = {"pairs": list(sp.names), "fields": self.fields, "q": list(q), "calm": None, "direction_tv": None, "rose_tv": None,
               "uv_js": None, "real_vs_generated": {}}
        if 0 in roses and 1 in roses:
            a, b = roses[0], roses[1]
            out["calm"] = {"real": self.rose(a)[0], "fake": self.rose(b)[0]}
            da = np.concatenate([[out["calm"]["real"]], self.direction_frequencies(a)])
            db = np.concatenate([[out["calm"]["fake"]], self.direction_frequencies(b)])
            out["direction_tv"] = _tv(da, db)
            out["rose_tv"] = self.tv_distance(a, b)
        if 0 in uv and 1 in uv:
            out["uv_js"] = self.js_divergence(uv[0], uv[1])
        for i in rf:
            X = sp.pairs[i][0]
            mx = self.table(i)[1:X.bins + 1, :-1].sum(axis=1).astype(np.float64)
            bias = self.conditional_bias(i)
            at = []
            if mx.sum() > 0:
                cum = np.cumsum(mx)
                at = [float(bias[min(int(np.searchsorted(cum, qk * cum[-1], side="left")), X.bins - 1)]) for qk in q]
            out["real_vs_generated"][sp.names[i]] = {"mutual_information": self.mutual_information(i), "bias_at_q": at}
        return out


def _batch(spec, a, b, n_valid, nhwc, channels):
    """Validate without touching a device -> (a Series, b Series | None, n)."""
    a, b, n = fields.batch(a, b, nhwc, channels, n_valid, "joint histograms", spec, sides=("a", "b"))
    if b is None and spec.uses_b:
        raise ValueError("the JointSpec has an axis of series b but b is None")
    return a, b, n


class ValueJoint:
    """Running joint histograms of the fields added so far: the tables (+ the field count) stay on the device as one int64
    tensor (``reduce_`` is one int64 all-reduce under data parallelism)."""

    def __init__(self, spec, device="cuda:0", ops=None):
        if not isinstance(spec, JointSpec):
            raise TypeError(f"ValueJoint takes a JointSpec (got {type(spec).__name__})")
        self.spec = spec
        self.device = torch.device(device)
        self._ops = ops
        self._cnt = torch.zeros(spec.offsets()[-1] + 1, dtype=torch.int64, device=self.device)   # the last entry: fields added
        self._struct = None

    @property
    def ops(self):
        if self._ops is None:
            self._ops = _default_ops(self.device)
        return self._ops

    @property
    def counts(self):
        return self._cnt[:-1]

    @property
    def fields(self):
        return int(self._cnt[-1].item())

    def add(self, a, b=None, n_valid=None, nhwc=False, channels=None):
        """Add every value of the first ``n_valid`` (default: all) fields of a batch: series ``a`` alone, or the pair (a, b).
        Layouts as ``histograms.histogram`` ([T, C, H, W] fp32 / bf16; with ``nhwc`` a [T, H, W, c_pad] store of which the
        leading ``channels`` are read; a ``NativeBatch``); the two series may differ in layout and dtype: pass ``nhwc`` as an
        (a, b) pair then."""
        a, b, n = _batch(self.spec, a, b, n_valid, nhwc, channels)
        if self._struct is None:
            self._struct = self.spec.struct()
        o = self.ops
        xa, fa = fields.descriptor(o, a.x[:n], a.nhwc, a.C)
        xb, fb = fields.descriptor(o, b.x[:n], b.nhwc, b.C) if b is not None else (None, None)
        o.hist2d(fa, fb, self._struct, self.counts)
        self._cnt[-1] += n
        return self

    def reduce_(self, dist):
        """Sum the tables and the field count over the data-parallel ranks of ``dist`` (downgan_amd.dist.Dist), once, in place."""
        if dist is not None and dist.world_size > 1:
            dist.allreduce_sum_(self._cnt)
        return self

    def result(self):
        """The ``Joint`` of every value added (and, after ``reduce_``, of every rank)."""
        return Joint(self.spec, self.counts.clone(), self.fields)


def joint_histogram(a, spec, b=None, channels=None, nhwc=False, ops=None):
    """Joint histograms of a series of fields (or of the pair a = real, b = generated) on the GPU under ``spec`` -> ``Joint``.
    The arguments as ``ValueJoint.add``."""
    if not isinstance(spec, JointSpec):
        raise TypeError(f"joint histograms take a JointSpec (got {type(spec).__name__})")
    device = _batch(spec, a, b, None, nhwc, channels)[0].x.device
    return ValueJoint(spec, device, ops=ops).add(a, b, nhwc=nhwc, channels=channels).result()
