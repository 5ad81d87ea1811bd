"""How every diagnostic takes a series of fields: the argument rules between a caller's batch and ``ops.eof_fields``.

A series is a tensor [T, C, H, W] (fp32 / bf16), with ``nhwc`` a dense-pixel [T, H, W, c_pad] store of which the leading
``channels`` are read (the generator's padded output), or a ``dataloader.NativeBatch``.  Everything up to ``descriptor`` checks
without touching a device or the library; ``batch`` is the order within one ``add``, and the owner's own limits follow it.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _lib, backend

C_MAX = _lib.EOF_MAX_C


class Series(NamedTuple):
    """One validated series: the tensor, its layout flag, the channels read, the fields, the grid."""
    x: torch.Tensor
    nhwc: bool
    C: int
    T: int
    H: int
    W: int


def default_ops(cache, device):
    """The op backend of ``device`` in ``cache`` (a module's own ``_ops``), made on first use."""
    key = str(device)
    if key not in cache:
        cache[key] = backend.make_ops("f32", device)
    return cache[key]


SIDES = ("real", "fake")      # what the two series of a pair are called in the messages; joint calls them ("a", "b")


def flags(nhwc, sides=SIDES):
    """``nhwc`` as one flag for both series, or one flag each -> (first, second)."""
    fl = tuple(nhwc) if isinstance(nhwc, (tuple, list)) else (nhwc, nhwc)
    if len(fl) != 2:
        raise ValueError(f"nhwc is one flag or a ({sides[0]}, {sides[1]}) pair (got {nhwc!r})")
    return fl


def series(x, channels, nhwc, noun):
    """Validate one series for the diagnostic called ``noun`` in the messages -> ``Series``."""
    if hasattr(x, "nhwc") and hasattr(x, "channels"):          # dataloader.NativeBatch
        x, nhwc, channels = x.nhwc, True, x.channels if channels is None else channels
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{noun} takes a tensor or a NativeBatch (got {type(x).__name__})")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{noun} reads fp32 or bf16 fields (got {x.dtype})")
    if x.dim() != 4:
        raise ValueError(f"{noun} takes [T, C, H, W] (or [T, H, W, c] with nhwc=True) fields (got shape {tuple(x.shape)})")
    T, held, H, W = (x.shape[i] for i in ((0, 3, 1, 2) if nhwc else (0, 1, 2, 3)))
    Cn = held if channels is None else int(channels)
    if not 1 <= Cn <= held:
        raise ValueError(f"channels = {Cn} but the {'NHWC store' if nhwc else 'tensor'} holds {held}")
    if not 1 <= Cn <= C_MAX:
        raise ValueError(f"{noun} takes 1 <= C <= {C_MAX} channels (got C = {Cn} of shape {tuple(x.shape)})")
    if T < 1 or H * W < 1:
        raise ValueError(f"{noun} needs at least one field of at least one pixel (got shape {tuple(x.shape)})")
    if H * W >= 2 ** 31 or T >= 2 ** 31:
        raise ValueError(f"{noun} takes fewer than 2^31 fields of fewer than 2^31 pixels (got shape {tuple(x.shape)})")
    return Series(x, bool(nhwc), Cn, int(T), int(H), int(W))


def agree(s, spec, what, owner=None, grid=None):
    """The ``what`` ("real", "fake", "given") series against its owner: the channels of ``spec`` and, where the owner was
    made for one, its ``grid``."""
    if s.C != spec.C:
        raise ValueError(f"the {type(spec).__name__} describes C = {spec.C} input channels but the {what} fields hold {s.C}")
    if grid is not None and (s.H, s.W) != tuple(grid):
        raise ValueError(f"{owner} was made for a {grid[0]} x {grid[1]} grid but the {what} fields are {s.H} x {s.W}")


def pair(a, b, sides=SIDES):
    """Two series that are added together: one length, one channel count, one grid, one device."""
    for what, va, vb in (("length", a.T, b.T), ("channels", a.C, b.C), ("grid", (a.H, a.W), (b.H, b.W))):
        if va != vb:
            raise ValueError(f"the paired {sides[0]} and {sides[1]} series differ in {what} ({va} and {vb})")
    if a.x.device != b.x.device:
        raise ValueError(f"the paired {sides[0]} and {sides[1]} series live on different devices ({a.x.device} and {b.x.device})")


def n_valid(n, T):
    """How many leading fields of a T-field batch to add: ``n``, or all of them (None)."""
    n = T if n is None else int(n)
    if not 1 <= n <= T:
        raise ValueError(f"n_valid = {n} of a batch of {T}")
    return n


def descriptor(o, x, nhwc, C):
    """(tensor, ``o.eof_fields`` of it): a dense batch is described in place (an NCHW one as its ``[:, :C]`` view), any other
    is copied first.  The tensor is what the descriptor points into: keep it until the kernel has been launched."""
    if not nhwc:
        x = x[:, :C]
    if not (x.stride(3) == 1 and x.stride(2) == x.shape[3] and x.stride(1) == x.shape[2] * x.shape[3]):
        x = x.contiguous()
    return x, (o.eof_fields(x, nhwc=True, channels=C) if nhwc else o.eof_fields(x))


def batch(real, fake, nhwc, channels, n, noun, spec, owner=None, grid=None, sides=SIDES):
    """Every check of one ``add`` (``fake`` None: of one series), in order -> (real Series, fake Series | None, fields to add)."""
    fl = flags(nhwc, sides)
    a = series(real, channels, fl[0], noun)
    b = None if fake is None else series(fake, channels, fl[1], noun)
    agree(a, spec, sides[0], owner, grid)
    if b is not None:
        agree(b, spec, sides[1], owner, grid)
        pair(a, b, sides)
    return a, b, n_valid(n, a.T)


def one_shot(real, nhwc, channels, noun, sides=SIDES):
    """What a one-shot function needs to make its accumulator -> (C, H, W, device) of the first series."""
    s = series(real, channels, flags(nhwc, sides)[0], noun)
    return s.C, s.H, s.W, s.x.device
