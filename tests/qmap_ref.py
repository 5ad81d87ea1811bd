"""The definition of empirical quantile mapping (include/downgan_hip.h "Empirical quantile mapping") restated in numpy, with
every rounding step explicit: int64 products, one np.float64 division and addition per node position, one np.float64 multiply
and add and one rounding to np.float32 per node, three np.float32 operations per mapped value.  Written from the definition,
not from the C++; the tests compare the library's host references and the kernels with it bit for bit.  Also the hand-made
tables both test files use."""
import numpy as np

from .test_histograms_cpu import F32, transform_ref

F64 = np.float64
QNAN = np.uint32(0x7fc00000)


def fit_pixel(a, b, nbins, lo, w):
    """float32 [nbins + 3]: the nodes of one pixel from its generated column a and real column b (int, [nbins + 3])."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    ng, nr = int(a[:nbins + 2].sum()), int(b[:nbins + 2].sum())
    k = np.arange(nbins + 1)
    if ng == 0 or nr == 0:
        pos = k.astype(F64)
    else:
        X = np.cumsum(a[:nbins + 1]) * nr                            # int64: below 2^52 for fewer than 2^26 fields
        Bp = np.cumsum(b[:nbins + 1]) * ng
        top = np.searchsorted(Bp, X, side="right") - 1               # max{s : B'_s <= X}, -1 when there is none
        over, under = X > Bp[nbins], X <= Bp[0]
        s = np.clip(np.searchsorted(Bp, X, side="left"), 1, nbins)   # the smallest s in 1 .. nbins with B'_s >= X
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = (X - Bp[s - 1]).astype(F64) / (b[s] * ng).astype(F64)
        plo = (s - 1).astype(F64) + frac
        phi = np.maximum(plo, top.astype(F64))
        plo = np.where(over, F64(nbins), np.where(under, F64(0), plo))
        phi = np.where(over, F64(nbins), np.where(under, np.maximum(top, 0).astype(F64), phi))
        pos = np.minimum(np.maximum(k.astype(F64), plo), phi)
    out = np.empty(nbins + 3, dtype=F32)
    out[:nbins + 1] = (F64(F32(lo)) + pos * F64(w)).astype(F32)
    out[nbins + 1] = F32(out[0] - F32(lo))
    out[nbins + 2] = F32(out[nbins] - F32(F64(F32(lo)) + F64(nbins) * F64(w)))
    return out


def fit_ref(counts, lo, width):
    """float32 [nout, nbins + 3, P] of a table int32 [nout, 2, nbins + 3, P] (side 0 real, side 1 generated)."""
    nout, _, nb3, P = counts.shape
    out = np.empty((nout, nb3, P), dtype=F32)
    for j in range(nout):
        for p in range(P):
            out[j, :, p] = fit_pixel(counts[j, 1, :, p], counts[j, 0, :, p], nb3 - 3, lo[j], width[j])
    return out


def apply_values(y, lo, inv_w, nbins, nodes):
    """float32 like y: the output values y float32 [..., P] of one channel through nodes float32 [nbins + 3, P]."""
    y = np.asarray(y, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = ((y - F32(lo)).astype(F32) * F32(inv_w)).astype(F32)
        inner = (t >= 0) & (t < nbins)
        k = np.where(inner, t, 0).astype(np.int64)
        p = np.broadcast_to(np.arange(y.shape[-1]), y.shape)
        n0, n1 = nodes[k, p], nodes[k + 1, p]
        f = (t - k.astype(F32)).astype(F32)
        dm = (n1 - n0).astype(F32)
        mid = (n0 + (f * dm).astype(F32)).astype(F32)
        low = (y + nodes[nbins + 1][p]).astype(F32)
        high = (y + nodes[nbins + 2][p]).astype(F32)
    out = np.where(inner, mid, np.where(t < 0, low, high)).astype(F32)
    bits = out.view(np.uint32).copy()
    bits[np.isnan(t)] = QNAN
    return bits.view(F32)


def apply_ref(spec, x, nodes):
    """float32 [T, nout, P]: x float32 [T, C, P] (the values the kernel reads) under ``spec`` through nodes [nout, bins + 3, P]."""
    T, Cn, P = x.shape
    y = transform_ref(spec, np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(Cn, -1)).reshape(spec.nout, T, P)
    return np.stack([apply_values(y[j], spec.lo[j], spec.inv_w[j], spec.bins, nodes[j]) for j in range(spec.nout)], axis=1)


def assert_order_preserving(y, out, rows, nan, lo, hi, nbins, what):
    """y, out float32 [T, P], rows int [T, P], nan bool [T, P]: per pixel, sorted by y, the mapped values do not decrease.
    Among values of one row this holds EXACTLY: d, t, f, f dm and n_k + f dm (or y + d_lo / y + d_hi) are each a non-decreasing
    function of the step before, dm >= 0.  Between two rows it holds to rounding only, as for any fp32 interpolation.  With
    u = 2^-24 (u |x| <= ulp(x)), R = hi - lo and v the two values:
      the later value is at least its row's lower node n (f >= 0, so fp32(n + m) >= n), or, in the underflow row, it is the
      earlier one's case below;
      the earlier value of bin k is at most fp32(n_k + fp32(n_{k+1} - n_k)) <= n_{k+1} + u |dm| + u |v|, and of the underflow
      row (y < lo exactly, the sign of y - lo survives both roundings) at most fp32(lo + fp32(n_0 - lo)) <= n_0 + u |d_lo| + u |v|:
      an inversion of at most 2 ulp of M = max(|lo|, |hi|, R, |v|) between rows below the overflow row;
      a y of the overflow row has fp32(fp32(y - lo) inv_w) >= nbins, three roundings (inv_w is a rounded quotient itself), so
      y >= hi - 3 u R, and y + d_hi >= n_nbins - 3 u R - u |d_hi| - u |v|: with the earlier value's n_nbins + u |dm| + u |v| (or
      the underflow row's u |d_lo|) an inversion of at most 3 + 1 + 1 + 1 + 1 + 1 = 8 ulp of M where the later row is the overflow."""
    T, P = y.shape
    M = max(abs(float(lo)), abs(float(hi)), float(hi) - float(lo))
    for p in range(P):
        ok = ~nan[:, p]
        order = np.argsort(y[ok, p], kind="stable")
        o, r = out[ok, p][order].astype(F64), rows[ok, p][order]
        with np.errstate(invalid="ignore", over="ignore"):
            big = np.maximum(np.maximum(np.abs(o[1:]), np.abs(o[:-1])), M)
            ulp = np.spacing(np.where(np.isfinite(big), big, 0).astype(F32)).astype(F64)
            tol = np.where(r[1:] == r[:-1], 0.0, np.where(r[1:] == nbins + 1, 8.0, 2.0) * ulp)
            assert np.all(o[1:] >= np.where(np.isfinite(o[:-1]), o[:-1] - tol, o[:-1])), (what, p, o, r)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


# ------------------------------------------------------------------------------------------------- tables
PATTERNS = 12


def hand_table(P, bins, rng, nout=2):
    """int32 [nout, 2, bins + 3, P] (side 0 real, side 1 generated): pixel p carries pattern p % 12 -- 0: empty on both sides;
    1: the real side empty; 2: the generated side empty; 3: all mass in the underflow rows; 4: all in the overflow rows; 5: all in
    the NaN rows (no finite value); 6: a single non-empty bin on the real side against a spread generated side; 7: the reverse;
    8: a == b with empty bins inside; 9: n = 2^26 - 1 in one bin of the generated side against a spread-out real side (the int64
    products near 2^52); 10: the reverse; 11: random with gaps.  The NaN row holds junk except where the pattern says: it must
    not count."""
    c = np.zeros((nout, 2, bins + 3, P), dtype=np.int64)
    fin = bins + 2
    for p in range(P):
        for j in range(nout):
            real, gen = c[j, 0, :, p], c[j, 1, :, p]
            k = p % PATTERNS
            spread = lambda n: np.floor(rng.dirichlet(np.ones(fin)) * n).astype(np.int64)
            if k in (1, 2):
                (gen if k == 1 else real)[:fin] = rng.integers(0, 6, fin)
                (gen if k == 1 else real)[1] += 1
            elif k == 3:
                real[0], gen[0] = 5 + j, 9
            elif k == 4:
                real[bins + 1], gen[bins + 1] = 3, 4 + j
            elif k == 5:
                real[bins + 2], gen[bins + 2] = 7, 8
            elif k in (6, 7):
                one, many = (real, gen) if k == 6 else (gen, real)
                one[1 + (p + j) % bins] = 11
                many[:fin] = rng.integers(0, 9, fin)
                many[bins] += 1
            elif k == 8:
                col = rng.integers(0, 50, fin) * rng.integers(0, 2, fin)
                col[1 + p % bins] += 3
                real[:fin] = gen[:fin] = col
            elif k in (9, 10):
                one, many = (gen, real) if k == 9 else (real, gen)
                one[1 + (p + j) % bins] = 2 ** 26 - 1
                many[:fin] = spread(2 ** 26 - 1 - 100 * j)
                many[1] += 1
            elif k == 11:
                real[:fin] = rng.integers(0, 1000, fin) * rng.integers(0, 2, fin)
                gen[:fin] = rng.integers(0, 1000, fin) * rng.integers(0, 2, fin)
                real[1] += 1
                gen[bins] += 1
            if k != 5:
                real[bins + 2], gen[bins + 2] = rng.integers(0, 50, 2)
    assert c.max() < 2 ** 26 and c[:, :, :fin].sum(axis=2).max() < 2 ** 26
    return c.astype(np.int32)


def random_table(P, bins, rng, nout=2):
    """Sparse random counts: about half the rows of a pixel are empty, so flat stretches of both CDFs are common."""
    c = rng.integers(0, 40, (nout, 2, bins + 3, P)) * rng.integers(0, 2, (nout, 2, bins + 3, P))
    return c.astype(np.int32)


def spec_axes(bins, nout=2):
    """(lo float32 [nout], width float64 [nout]) of bins on [-6, 6] and, for the further channels, on [0, 7.5 + j]."""
    lo = np.array([-6.0] + [0.0] * (nout - 1), dtype=F32)
    hi = np.array([6.0] + [7.5 + j for j in range(1, nout)], dtype=F32)
    return lo, (hi.astype(F64) - lo.astype(F64)) / bins
