"""The definition of the field-deformation sums in numpy, shared by test_deform_cpu and test_deform_gpu: the quantiser in numpy
float32, everything after it in int64, the 25 shifts and the 5 x 5 window as shifted views of zero-padded arrays, the tie rule as
the order of a loop with a strict <, totals as Python integers.  Shares no code with the library."""
import numpy as np

from .test_histograms_cpu import transform_ref

F32 = np.float32
ORDER = sorted(((sy, sx) for sy in range(-2, 3) for sx in range(-2, 3)), key=lambda s: (s[0] * s[0] + s[1] * s[1], s[0], s[1]))
NSCALARS = 5


def ints(a):
    return [int(v) for v in np.asarray(a, dtype=object).reshape(-1)]


def max_disp(F):
    return 2 * (2 ** (F + 1) - 1)


def quantise_ref(spec, x):
    """x float32 [T, C, H, W] -> q int64 [T, nout, H, W] in 0 .. 255."""
    T, Cn, H, W = x.shape
    y = transform_ref(spec, np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(Cn, -1)).reshape(spec.nout, T, H, W)
    q = np.empty(y.shape, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(spec.nout):
            t = ((y[j] - F32(spec.lo[j])).astype(F32) * F32(spec.inv_step[j])).astype(F32)
            inner = np.where((t >= 0) & (t < 254), t, 0).astype(np.int64) + 1
            q[j] = np.where(np.isnan(t), 0, np.where(t < 0, 0, np.where(t >= 254, 255, inner)))
    return q.transpose(1, 0, 2, 3)


def pyramid_ref(q, F):
    """q int64 [..., H, W] -> [P_0 .. P_F]: sums of 2 x 2 blocks, zeros beyond the grid."""
    out = [q]
    for _ in range(F):
        p = out[-1]
        h, w = p.shape[-2:]
        e = np.zeros(p.shape[:-2] + (h + h % 2, w + w % 2), dtype=np.int64)
        e[..., :h, :w] = p
        out.append(e[..., 0::2, 0::2] + e[..., 0::2, 1::2] + e[..., 1::2, 0::2] + e[..., 1::2, 1::2])
    return out


def gather0(a, yy, xx):
    """a [N, h, w] read at the index arrays yy, xx [N, h', w'], 0 outside."""
    h, w = a.shape[-2:]
    ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
    n = np.arange(a.shape[0])[:, None, None]
    return np.where(ok, a[n, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0)


def match_ref(X, Y, F):
    """Pyramids X (target), Y (source), each a list of int64 [N, h_l, w_l] -> d_0 as (dy, dx) int64 [N, H, W]."""
    dy = dx = None
    for l in range(F, -1, -1):
        N, h, w = X[l].shape
        gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        gy, gx = np.broadcast_to(gy, (N, h, w)), np.broadcast_to(gx, (N, h, w))
        if dy is None:
            iy = ix = np.zeros((N, h, w), dtype=np.int64)
        else:
            iy, ix = (2 * np.repeat(np.repeat(d, 2, axis=1), 2, axis=2)[:, :h, :w] for d in (dy, dx))
        yp = gather0(Y[l], gy + iy, gx + ix)
        xpad = np.pad(X[l], ((0, 0), (2, 2), (2, 2)))
        ypad = np.pad(yp, ((0, 0), (4, 4), (4, 4)))
        best = by = bx = None
        for sy, sx in ORDER:
            e = xpad - ypad[:, 2 + sy:2 + sy + h + 4, 2 + sx:2 + sx + w + 4]          # over the grid and a margin of 2
            e = e * e
            cost = sum(e[:, wy:wy + h, wx:wx + w] for wy in range(5) for wx in range(5))
            if best is None:
                best, by, bx = cost, np.full((N, h, w), sy), np.full((N, h, w), sx)
            else:
                m = cost < best
                best, by, bx = np.where(m, cost, best), np.where(m, sy, by), np.where(m, sx, bx)
        dy, dx = by + gather0(iy, gy + by, gx + bx), bx + gather0(ix, gy + by, gx + bx)
    return dy, dx


def deform_ref(spec, a, b):
    """a, b float32 [T, C, H, W] (the values read) -> (disp [nout, 2, 2 D + 1, 2 D + 1] and scalars [nout, 2, 5] as arrays of
    Python integers, field int16 [T, nout, 2, 2, H, W], morphed uint8 [T, nout, 2, H, W])."""
    T, _, H, W = a.shape
    F, D = spec.levels, max_disp(spec.levels)
    side = 2 * D + 1
    qa, qb = (quantise_ref(spec, x).reshape(T * spec.nout, H, W) for x in (a, b))
    pa, pb = pyramid_ref(qa, F), pyramid_ref(qb, F)
    disp = np.zeros((spec.nout, 2, side, side), dtype=object)
    scal = np.zeros((spec.nout, 2, NSCALARS), dtype=object)
    field = np.zeros((T, spec.nout, 2, 2, H, W), dtype=np.int16)
    morphed = np.zeros((T, spec.nout, 2, H, W), dtype=np.uint8)
    gy, gx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for d, (X, Y) in enumerate(((pa, pb), (pb, pa))):
        dy, dx = match_ref(X, Y, F)
        assert np.abs(dy).max() <= D and np.abs(dx).max() <= D
        m = gather0(Y[0], gy + dy, gx + dx)
        shape = (T, spec.nout, H, W)
        x0, y0, m, dy, dx = (v.reshape(shape) for v in (X[0], Y[0], m, dy, dx))
        field[:, :, d, 0], field[:, :, d, 1], morphed[:, :, d] = dy, dx, m
        for j in range(spec.nout):
            on = x0[:, j] > 0
            np.add.at(disp[j, d], (dy[:, j][on] + D, dx[:, j][on] + D), 1)
            scal[j, d] = [int(on.sum()), int((on | (m[:, j] > 0)).sum()), int(((x0[:, j] - m[:, j]) ** 2).sum()),
                          int(((x0[:, j] - y0[:, j]) ** 2).sum()), int((x0[:, j] ** 2).sum())]
    return disp, scal, field, morphed
