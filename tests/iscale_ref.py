"""The definition of the intensity-scale sums in numpy, shared by test_iscale_cpu and test_iscale_gpu: the exceedance masks as
fp32 compares, zero-padded to the 2^n x 2^n square anchored at pixel (0, 0), block sums by reshape, totals as Python integers."""
import numpy as np

from .test_histograms_cpu import transform_ref

F32 = np.float32


def log_side(H, W):
    n = 0
    while (1 << n) < max(H, W):
        n += 1
    return n


def masks_ref(spec, x):
    """x float32 [T, C, H, W] -> bool [nout, K, T, H, W]: y > thr as an fp32 compare (NaN false, +inf true, equality false)."""
    T, Cn, H, W = x.shape
    y = transform_ref(spec, np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(Cn, -1)).reshape(spec.nout, T, H, W)
    with np.errstate(invalid="ignore"):
        return y[:, None] > spec.thresholds.astype(F32)[:, :, None, None, None]


def block_sums(m, n, l):
    """m bool [..., H, W] -> int64 [..., 2^(n-l), 2^(n-l)]: the sums over the aligned blocks of side 2^l of the padded square."""
    H, W = m.shape[-2:]
    S, b, nb = 1 << n, 1 << l, 1 << (n - l)
    p = np.zeros(m.shape[:-2] + (S, S), dtype=np.int64)
    p[..., :H, :W] = m
    return p.reshape(m.shape[:-2] + (nb, b, nb, b)).sum(axis=(-3, -1))


def iscale_ref(spec, a, b):
    """a, b float32 [T, C, H, W] (the values read) -> (sums [nout, K, n + 1, 3], per_field [T, nout, K, n + 1, 3]) as arrays of
    Python integers: D_l, A_l, B_l.  One field adds at most 2^44, so the int64 field sums are exact; fields are added as Python
    integers."""
    T, _, H, W = a.shape
    n = log_side(H, W)
    ma, mb = masks_ref(spec, a), masks_ref(spec, b)
    per = np.zeros((T, spec.nout, spec.K, n + 1, 3), dtype=object)
    for l in range(n + 1):
        sa, sb = block_sums(ma, n, l), block_sums(mb, n, l)
        d = sb - sa
        for e, v in enumerate(((d * d).sum(axis=(-2, -1)), (sa * sa).sum(axis=(-2, -1)), (sb * sb).sum(axis=(-2, -1)))):
            per[:, :, :, l, e] = v.transpose(2, 0, 1).astype(object)
    return per.sum(axis=0), per


def ints(a):
    return [int(v) for v in np.asarray(a, dtype=object).reshape(-1)]
