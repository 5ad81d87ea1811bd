"""Empirical quantile mapping: the per-gridpoint bias correction of generated fields, fitted and applied on the GPU
(csrc/qmap.hip).

``gridhist`` says where and how the generated distribution at a gridpoint is wrong; this module acts on it.  Empirical quantile
mapping (EQM) sends a generated value y at pixel p to the real value of the same local rank, y' = F_real^-1(F_gen(y)): the
bias-correction half of BCSD and the "GAN + QM" baseline of downscaling studies.  It needs no accumulator of its own: the
calibration statistics are the exact paired table int32 [nout, 2, bins + 3, P] a ``gridhist.GridHist`` keeps.  ``QuantileMap.fit``
turns that table into one piecewise-linear transfer function per pixel and output channel,

    nodes float32 [nout, bins + 3, P]     rows 0 .. bins: where the bin edge lo + k w of the generated values goes;
                                          row bins + 1: d_lo = nodes[0] - lo;  row bins + 2: d_hi = nodes[bins] - hi

and ``apply`` sends every value of a series of fields through the transfer function of its pixel: linear between the two nodes
of its bin, the constant shift d_lo / d_hi beyond the calibrated range, NaN for NaN.  Where the real CDF is flat at a target
its inverse is an interval, and the node takes the point of it nearest to the edge itself: the least correction, and equal
real and generated histograms give the identity exactly.  A pixel without finite values on either side keeps the identity
(``valid`` is False there).  The definition (include/downgan_hip.h "Empirical quantile mapping") is integer arithmetic and
single correctly rounded operations, so the device and the library's host reference agree bit for bit, two calls are
bit-identical, and the result does not depend on layout, dtype (bf16 inputs are the values the kernel reads) or on how the fields
were chunked into calls.  The values mapped are the spec's OUTPUT values (after its affine transform; the speed as its own
channel): the result is float32 [T, nout, H, W] in those units.  EQM is fitted once, on a calibration part of the data, and
applied to what the generator makes afterwards: ``Generator.generate(coarse, qmap=m)``.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, fields
from . import gridhist as _gh
from .gridhist import BINS_MAX, GridHist, GridHistMaps, _check_spec
from .histograms import HistSpec, _default_ops


def _table(counts):
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    if counts.ndim != 4 or counts.shape[1] != 2 or not 1 <= counts.shape[2] - 3 <= BINS_MAX or counts.shape[3] < 1:
        raise ValueError(f"quantile mapping needs a (real, fake) pair: a table int32 [nout, 2, bins + 3, P] with bins <= {BINS_MAX} "
                         f"(got shape {counts.shape})")
    return counts


def host_fit(counts, lo, width):
    """float32 numpy [nout, bins + 3, P]: the transfer nodes of a paired table int32 [nout, 2, bins + 3, P] with the bin origins
    ``lo`` and widths ``width`` (one per output channel), computed by the library on the host (dg_qmap_fit_host, plain C++: the
    definition the kernel is tested against)."""
    counts = _table(counts)
    nout, _, nb3, P = counts.shape
    lo = np.ascontiguousarray(lo, dtype=np.float32).reshape(-1)
    width = np.ascontiguousarray(width, dtype=np.float64).reshape(-1)
    if len(lo) != nout or len(width) != nout:
        raise ValueError(f"host_fit needs one lo and one width per output channel ({nout}; got {len(lo)} and {len(width)})")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(width) & (width > 0))):
        raise ValueError(f"host_fit needs finite lo and finite width > 0 (got {lo.tolist()} and {width.tolist()})")
    nodes = np.empty((nout, nb3, P), dtype=np.float32)
    _lib.check(_lib.lib().dg_qmap_fit_host(counts.ctypes.data, nout, nb3 - 3, P, lo.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           width.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nodes.ctypes.data), "dg_qmap_fit_host")
    return nodes


def host_apply(spec, x, nodes):
    """float32 numpy [T, nout, P]: the values x float32 [T, C, P] through the transfer nodes float32 [nout, bins + 3, P] under
    ``spec``, computed by the library on the host (dg_qmap_apply_host)."""
    _check_spec(spec)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3 or x.shape[1] != spec.C or x.shape[0] < 1 or x.shape[2] < 1:
        raise ValueError(f"host_apply takes [T, C = {spec.C}, P] values (got shape {x.shape})")
    T, _, P = x.shape
    nodes = np.ascontiguousarray(nodes, dtype=np.float32)
    if nodes.shape != (spec.nout, spec.bins + 3, P):
        raise ValueError(f"host_apply takes nodes [nout = {spec.nout}, bins + 3 = {spec.bins + 3}, P = {P}] (got shape {nodes.shape})")
    out = np.empty((T, spec.nout, P), dtype=np.float32)
    s = spec.struct()
    _lib.check(_lib.lib().dg_qmap_apply_host(ctypes.byref(s), x.ctypes.data, spec.C, T, P, nodes.ctypes.data, out.ctypes.data),
               "dg_qmap_apply_host")
    return out


class QuantileMap:
    """The fitted transfer functions of one HistSpec on an H x W grid: ``nodes`` float32 [nout, bins + 3, P] where the table
    lived, ``valid`` bool [nout, H, W] (both sides had finite values; elsewhere the map is the identity) and ``fields``, the
    number of calibration fields."""

    def __init__(self, spec, H, W, nodes, valid, fields, ops=None):
        _check_spec(spec)
        self.spec, self.H, self.W, self.fields = spec, int(H), int(W), int(fields)
        if tuple(nodes.shape) != (spec.nout, spec.bins + 3, self.H * self.W) or nodes.dtype != torch.float32:
            raise ValueError(f"nodes are float32 [nout = {spec.nout}, bins + 3 = {spec.bins + 3}, P = {self.H * self.W}] "
                             f"(got {nodes.dtype} {tuple(nodes.shape)})")
        if not (isinstance(valid, torch.Tensor) and valid.dtype == torch.bool and tuple(valid.shape) == (spec.nout, self.H, self.W)):
            raise ValueError(f"valid is a bool tensor [nout = {spec.nout}, H = {self.H}, W = {self.W}] "
                             f"(got {type(valid).__name__ if not isinstance(valid, torch.Tensor) else (valid.dtype, tuple(valid.shape))})")
        self.nodes, self.valid, self._ops = nodes.contiguous(), valid, ops
        self._struct = None
        self._moved = {}

    @classmethod
    def fit(cls, maps, ops=None):
        """Fit on a paired ``GridHistMaps`` (or a paired ``GridHist``, whose ``result()`` is used): side "real" is the target,
        side "fake" the source.  A device table is fitted on the device through ``ops`` (dg_qmap_fit), a CPU table through the
        library's host reference."""
        if isinstance(maps, GridHist):
            maps = maps.result()
        if not isinstance(maps, GridHistMaps):
            raise TypeError(f"QuantileMap.fit takes a paired GridHistMaps or GridHist (got {type(maps).__name__})")
        _check_spec(maps.spec)
        if not maps.paired:
            raise ValueError("quantile mapping needs a (real, fake) pair: GridHist(paired=True)")
        spec, c = maps.spec, maps.counts
        ops = ops if ops is not None else maps._ops
        fin = maps._finite()                                         # int64 numpy [nout, 2, P], reduced where the table lives
        valid = torch.from_numpy(((fin[:, 0] > 0) & (fin[:, 1] > 0)).reshape(spec.nout, maps.H, maps.W)).to(c.device)
        if c.is_cuda:
            o = ops if ops is not None else _default_ops(c.device)
            nodes = torch.empty(spec.nout, spec.bins + 3, maps.H * maps.W, dtype=torch.float32, device=c.device)
            o.qmap_fit(c.contiguous(), spec.lo, spec.width(), nodes)
        else:
            nodes = torch.from_numpy(host_fit(c.numpy(), spec.lo, spec.width()))
        return cls(spec, maps.H, maps.W, nodes, valid, maps.fields, ops=ops)

    def _nodes_on(self, device):
        if self.nodes.device == device:
            return self.nodes
        key = str(device)
        if key not in self._moved:
            self._moved[key] = self.nodes.to(device)
        return self._moved[key]

    def apply(self, x, n_valid=None, nhwc=False, channels=None, out=None):
        """Map the first ``n_valid`` (default: all) fields of a batch -> float32 [n, nout, H, W] on the batch's device, in the
        spec's output units.  Layouts as ``gridhist.GridHist.add`` ([T, C, H, W]; with ``nhwc`` a [T, H, W, c_pad] store of which
        the leading ``channels`` are read; a ``NativeBatch``; fp32 or bf16).  ``out``: a contiguous float32 [>= n, nout, H, W]
        tensor on that device whose first n fields are overwritten (the rest is left as it is)."""
        a, _, n = fields.batch(x, None, nhwc, channels, n_valid, "qmap", self.spec, "QuantileMap", (self.H, self.W),
                               sides=("given", "given"))
        shape = (self.spec.nout, self.H, self.W)
        if out is None:
            out = torch.empty((n,) + shape, dtype=torch.float32, device=a.x.device)
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 4
                  and tuple(out.shape[1:]) == shape and out.shape[0] >= n and out.device == a.x.device):
            raise ValueError(f"out is a contiguous float32 [>= {n}, {shape[0]}, {shape[1]}, {shape[2]}] tensor on {a.x.device}")
        nodes = self._nodes_on(a.x.device)
        if a.x.is_cuda:                                               # a CPU batch: the library's host reference
            o = self._ops if self._ops is not None else _default_ops(a.x.device)
            if self._struct is None:
                self._struct = self.spec.struct()
            kept, f = fields.descriptor(o, a.x[:n], a.nhwc, a.C)
            o.qmap_apply(f, self._struct, nodes, out[:n])
        else:
            v = a.x[:n, ..., :a.C].permute(0, 3, 1, 2) if a.nhwc else a.x[:n, :a.C]
            planar = v.float().reshape(n, a.C, -1).contiguous().numpy()
            out[:n] = torch.from_numpy(host_apply(self.spec, planar, nodes.numpy())).view((n,) + shape)
        return out[:n]

    def transfer(self):
        """(edges float64 [nout, bins + 1], nodes float64 [nout, bins + 1, H, W]): the local QQ line of every pixel, the bin
        edges of the generated values against where they are mapped."""
        b = self.spec.bins
        n = self.nodes[:, :b + 1].detach().cpu().numpy().astype(np.float64)
        return self.spec.edges(), n.reshape(self.spec.nout, b + 1, self.H, self.W)

    def save(self, path):
        """One ``.npz`` with the nodes and every field of the spec; ``load`` gives the same map bit for bit."""
        s = self.spec
        with open(path, "wb") as f:
            np.savez(f, nodes=self.nodes.detach().cpu().numpy(), valid=self.valid.detach().cpu().numpy(),
                     grid=np.array([self.H, self.W, self.fields], dtype=np.int64), bins=np.int64(s.bins), lo=s.lo, hi=s.hi,
                     scale=s.scale, offset=s.offset, speed=np.array(s.speed if s.speed is not None else [], dtype=np.int64),
                     names=np.array(s.names))
        return path

    @classmethod
    def load(cls, path, device="cpu", ops=None):
        with np.load(path) as z:
            speed = tuple(int(v) for v in z["speed"]) or None
            spec = HistSpec(int(z["bins"]), z["lo"], z["hi"], scale=z["scale"], offset=z["offset"], speed=speed,
                            names=[str(n) for n in z["names"]])
            H, W, n = (int(v) for v in z["grid"])
            nodes, valid = torch.from_numpy(z["nodes"]).to(device), torch.from_numpy(z["valid"]).to(device)
        return cls(spec, H, W, nodes, valid, n, ops=ops)


def quantile_map(real, fake, spec=None, n_valid=None, nhwc=False, channels=None, ops=None):
    """``gridhist.gridhist(real, fake, spec)`` and then ``QuantileMap.fit``: the map that sends the distribution of ``fake`` at
    every gridpoint to that of ``real``.  spec None: ``HistSpec.zscore(C, bins=64, lim=6.0)``, the default of ``gridhist``; the
    other arguments as ``GridHist.add``."""
    if spec is not None:
        _check_spec(spec)
    if fake is None:
        raise ValueError("quantile mapping needs a (real, fake) pair: GridHist(paired=True)")
    return QuantileMap.fit(_gh.gridhist(real, fake, spec=spec, n_valid=n_valid, nhwc=nhwc, channels=channels, ops=ops), ops=ops)
