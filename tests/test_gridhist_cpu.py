"""Per-gridpoint histograms without a GPU: spec and argument checks that fire before any library call, the ABI surface, the two
host references (dg_gridhist_host, dg_gridhist_scan_host) against numpy, the host-side derivations of ``GridHistMaps`` from
hand-made tables against ``histograms``, and the trainer's opt-in hook on the emulated ops (a test-local op class adds a numpy
``gridhist`` / ``gridhist_scan`` under the usual make_ops patch), in one process, over 2 gloo ranks, and in the
frequency-separation trainer."""
import ctypes as C
import json
import os
import re
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from downgan_amd import _lib, gridhist, histograms
from downgan_amd.gridhist import GridHist, GridHistMaps
from downgan_amd.histograms import HistSpec, Histogram

from .test_gridstats_cpu import _no_library
from .test_histograms_cpu import F32, bins_ref, transform_ref  # noqa: F401  (transform_ref: the definition bins_ref bins)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q16 = [0.5, 0.25, float(np.nextafter(0.25, 0.0)), float(np.nextafter(0.25, 1.0)), 1e-300, 0.01, 0.05, 0.1, 0.3, 0.75, 0.9, 0.95,
       0.98, 0.99, 0.999, float(np.nextafter(1.0, 0.0))]
Q3 = [0.5, 0.95, 0.99]


# ------------------------------------------------------------------------------------------------- the definitions in numpy
def specs():
    """bins = 1; bins = 64 with an affine transform and the speed (width 1/4 in every channel: speed 5 is an edge); bins = 256
    without the speed."""
    return [("one_bin", HistSpec(1, [-1.0, -1.0], [1.0, 1.0], speed=None)),
            ("affine_speed", HistSpec(64, [-8.0, -8.0, 0.0], [8.0, 8.0, 16.0], scale=[2.0, 0.5], offset=[-1.0, 0.25])),
            ("fine", HistSpec(256, [-4.0, -4.0], [4.0, 4.0], speed=None))]


def table_ref(spec, a, b=None):
    """int32 [nout, S, bins + 3, P] of a (and b) float32 [C, T, P], the values the kernel reads: per-pixel np.bincount of the
    rows of the numpy float32 definition (test_histograms_cpu.transform_ref + the bin rule)."""
    out = []
    for x in (a,) if b is None else (a, b):
        Cn, T, P = x.shape
        rows = bins_ref(spec, x.reshape(Cn, -1)).reshape(spec.nout, T, P)
        out.append(np.stack([np.stack([np.bincount(rows[j, :, p], minlength=spec.bins + 3) for p in range(P)], axis=1)
                             for j in range(spec.nout)]))
    return np.stack(out, axis=1).astype(np.int32)


def scan_ref(counts, q):
    """(ranks int32 [nout, S, Q, 3, P], dist int64 [nout, 2, P] or None) of the header's definition: int64 cumulative sums,
    np.ceil of the float64 product, Python-int cross products."""
    c = np.asarray(counts).astype(np.int64)
    nout, S, nb3, P = c.shape
    bins = nb3 - 3
    fin = c[:, :, :bins + 2]
    cum = np.cumsum(fin, axis=2)
    n = cum[:, :, -1]
    ranks = np.empty((nout, S, len(q), 3, P), dtype=np.int32)
    for k, qk in enumerate(q):
        target = np.ceil(np.float64(qk) * n.astype(np.float64)).astype(np.int64)
        b = np.minimum((cum < target[:, :, None]).sum(axis=2), bins + 1)          # the first row whose cumulative count >= k
        at = np.take_along_axis(fin, b[:, :, None], axis=2)[:, :, 0]
        below = np.take_along_axis(cum, b[:, :, None], axis=2)[:, :, 0] - at
        ranks[:, :, k, 0] = np.where(n > 0, b, -1)
        ranks[:, :, k, 1] = np.where(n > 0, below, 0)
        ranks[:, :, k, 2] = np.where(n > 0, at, 0)
    if S == 1:
        return ranks, None
    A, B = cum[:, 0].astype(object), cum[:, 1].astype(object)                     # Python ints: no overflow to reason about
    na, nb = n[:, 0].astype(object)[:, None], n[:, 1].astype(object)[:, None]
    d = np.abs(A * nb - B * na)
    g = np.full(bins + 1, 2, dtype=object)
    g[0] = g[bins] = 1
    d0 = (d[:, :bins + 1] * g[None, :, None]).sum(axis=1)
    d1 = d.max(axis=1)
    none = (n[:, 0] == 0) | (n[:, 1] == 0)
    return ranks, np.stack([np.where(none, -1, d0), np.where(none, -1, d1)], axis=1).astype(np.int64)


def special_values(spec):
    """float32 inputs that land on every bin edge of the spec's input channels, their two fp32 neighbours (the planted
    ``special_values`` idea of test_gridstats_gpu), +-0, denormals, +-inf, NaN and +-FLT_MAX."""
    f = np.finfo(F32)
    vals = []
    for c in range(spec.C):
        edges = spec.edges()[c]
        on = ((edges - float(spec.offset[c])) / float(spec.scale[c])).astype(F32)
        vals += [on, np.nextafter(on, F32(-np.inf)), np.nextafter(on, F32(np.inf))]
    vals.append(np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, f.tiny, -f.tiny, np.inf, -np.inf, np.nan, f.max, -f.max],
                         dtype=F32))
    return np.concatenate(vals)


def data(rng, spec, T, H, W, shift=0):
    """float32 [T, 2, H, W]: Gaussian values with the special values planted at known (t, p) of both channels, pairs whose
    outputs are (3, 4) (speed exactly 5: an edge of the speed channel), and one pixel that is never finite."""
    x = (rng.standard_normal((T, 2, H, W)) * 2).astype(F32)
    flat = x.transpose(1, 0, 2, 3).reshape(2, -1)                    # a copy: [C, T*P]
    sv = special_values(spec)
    n = flat.shape[1]
    pos = (np.arange(len(sv)) * 7919 + 13 + shift) % n
    flat[0, pos] = sv
    flat[1, (pos + 5) % n] = sv[::-1]
    u, v = ((np.array([3.0, 4.0]) - spec.offset.astype(np.float64)) / spec.scale.astype(np.float64)).astype(F32)
    flat[0, (pos[:4] + 11) % n], flat[1, (pos[:4] + 11) % n] = u, v
    x = flat.reshape(2, T, H, W).transpose(1, 0, 2, 3).copy()
    if H * W > 20:
        x[:, 0, H - 1, W - 1] = np.nan                               # no finite value at all in channel 0 (and the speed)
    return x


def cube(x):
    """[T, C, H, W] -> [C, T, P]."""
    return np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(x.shape[1], x.shape[0], -1)


def hand_table(P, bins, rng, nout=2):
    """int32 [nout, 2, bins + 3, P]: pixel p carries pattern p % 9 -- 0: no finite value on the real side only; 1: all mass in
    one interior row; 2: all in underflow; 3: all in overflow; 4: na != nb; 5: n = 4, one per row where there is room (q n an
    exact integer at q = 0.5, 0.25); 6: n = 8 (q n one ulp either side of 2 at the neighbours of 0.25); 7: counts near the
    2^26 limit; 8: random.  The NaN row holds junk everywhere: it must not count."""
    c = np.zeros((nout, 2, bins + 3, P), dtype=np.int64)
    for p in range(P):
        for j in range(nout):
            for s in range(2):
                k, col = p % 9, c[j, s, :, p]
                if k == 0:
                    col[:bins + 2] = 0 if s == 0 else rng.integers(0, 5, bins + 2)
                    col[1] += s
                elif k == 1:
                    col[1 + (p + j + s) % bins] = 7 + s
                elif k == 2:
                    col[0] = 5 + j
                elif k == 3:
                    col[bins + 1] = 3 + s
                elif k == 4:
                    col[:bins + 2] = rng.integers(0, 9 + 20 * s, bins + 2)
                    col[bins] += 1
                elif k == 5:
                    for i in range(4):
                        col[(i * (1 + s) + j) % (bins + 2)] += 1
                elif k == 6:
                    for i in range(8):
                        col[(i * (2 - s) + j) % (bins + 2)] += 1
                elif k == 7:
                    w = rng.integers(1, 100, bins + 2).astype(np.float64)
                    col[:bins + 2] = np.floor(w / w.sum() * (2 ** 26 - 1 - 200 * s)).astype(np.int64)
                else:
                    col[:bins + 2] = rng.integers(0, 1000, bins + 2) * rng.integers(0, 2, bins + 2)
                    col[1] += 1
                col[bins + 2] = rng.integers(0, 50)
    assert c.max() < 2 ** 26 and c[:, :, :bins + 2].sum(axis=2).max() < 2 ** 26
    return c.astype(np.int32)


def hand_tables(P):
    rng = np.random.default_rng(1000 + P)
    return [("bins1", hand_table(P, 1, rng)), ("bins8", hand_table(P, 8, rng, nout=3)), ("bins64", hand_table(P, 64, rng, nout=1))]


# ------------------------------------------------------------------------------------------------- spec and argument checks
def test_spec_and_levels_are_checked(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="at most 256 bins"):
        GridHist(HistSpec(257, [-1.0, -1.0], [1.0, 1.0], speed=None), 8, 8, device="cpu")
    with pytest.raises(ValueError, match="at most 256 bins"):
        gridhist.gridhist(torch.zeros(2, 2, 8, 8), spec=HistSpec.zscore(2))          # the default 2048 bins of zscore
    with pytest.raises(ValueError, match="at most 256 bins"):
        gridhist.host_table(HistSpec.zscore(2), np.zeros((1, 2, 4), F32))
    with pytest.raises(TypeError, match="HistSpec"):
        GridHist(object(), 8, 8, device="cpu")
    with pytest.raises(ValueError, match="grid"):
        GridHist(HistSpec.zscore(2, bins=64), 0, 8, device="cpu")
    assert gridhist.BINS_MAX == 256 and gridhist.Q_MAX == 16 and gridhist.FIELDS_MAX == 2 ** 26
    GridHist(HistSpec.zscore(2, bins=256), 2, 2, device="cpu")
    m = GridHistMaps(HistSpec.zscore(2, bins=4), 1, 2, True, torch.zeros(3, 2, 7, 2, dtype=torch.int32), 0)
    for bad in ([0.0], [1.0], [0.5, -0.1], [0.5, 1.5], [float("nan")], [], [0.5] * 17):
        with pytest.raises(ValueError, match="levels"):
            m.quantile(bad)
        with pytest.raises(ValueError, match="levels"):
            m.summary(bad)
        with pytest.raises(ValueError, match="levels"):
            gridhist.host_scan(np.zeros((1, 1, 4, 2), np.int32), bad)
    with pytest.raises(ValueError, match="side"):
        GridHistMaps(HistSpec.zscore(2, bins=4), 1, 2, False, torch.zeros(3, 1, 7, 2, dtype=torch.int32), 0).count("fake")
    with pytest.raises(ValueError, match="pair"):
        GridHistMaps(HistSpec.zscore(2, bins=4), 1, 2, False, torch.zeros(3, 1, 7, 2, dtype=torch.int32), 0).w1()
    with pytest.raises(ValueError, match="table is int32"):
        gridhist.host_scan(np.zeros((1, 3, 4, 2), np.int32), [0.5])


@pytest.mark.parametrize("x,kw,err,match", [
    (torch.zeros(2, 3, 8, 8), {}, ValueError, "C = 2"),
    (torch.zeros(2, 9, 8, 8), {}, ValueError, "C <="),
    (torch.zeros(2, 8, 8, 4), {"nhwc": True, "channels": 5}, ValueError, "channels"),
    (torch.zeros(2, 8, 8, 4), {"nhwc": True}, ValueError, "C = 2"),
    (torch.zeros(2, 2, 8, 8, dtype=torch.float64), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 2, 8, 8), np.float32), {}, TypeError, "tensor"),
    (torch.zeros(2, 8, 8), {}, ValueError, "shape"),
    (torch.zeros(0, 2, 8, 8), {}, ValueError, "at least one"),
    (torch.zeros(2, 2, 8, 4), {}, ValueError, "8 x 8 grid"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, x, kw, err, match):
    _no_library(monkeypatch)
    spec = HistSpec.zscore(2, bins=64, lim=6.0)
    good = torch.zeros(2, 2, 8, 8)
    single = GridHist(spec, 8, 8, paired=False, device="cpu")
    with pytest.raises(err, match=match):
        single.add(x, **kw)
    pair = GridHist(spec, 8, 8, paired=True, device="cpu")
    with pytest.raises(err, match=match):
        pair.add(good, x, nhwc=(False, kw.get("nhwc", False)), channels=kw.get("channels"))
    with pytest.raises(err, match=match):
        pair.add(x, good, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))
    if "grid" not in match:                                               # the one-shot form takes the grid from the fields
        with pytest.raises(err, match=match):
            gridhist.gridhist(x, spec=spec, **kw)


def test_accumulator_checks(monkeypatch):
    _no_library(monkeypatch)
    spec = HistSpec.zscore(2, bins=64, lim=6.0)
    x = torch.zeros(2, 2, 8, 8)
    pair, single = GridHist(spec, 8, 8, device="cpu"), GridHist(spec, 8, 8, paired=False, device="cpu")
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            pair.add(x, x, n_valid=n)
    with pytest.raises(ValueError, match="paired"):
        pair.add(x)
    with pytest.raises(ValueError, match="one series"):
        single.add(x, x)
    with pytest.raises(ValueError, match="differ in length"):
        pair.add(x, torch.zeros(3, 2, 8, 8))
    with pytest.raises(ValueError, match="nhwc"):
        pair.add(x, x, nhwc=(True, False, True))
    pair._added = 2 ** 26 - 2                                            # the int64 W1 sum: the total must stay below 2^26
    with pytest.raises(ValueError, match="would reach 2\\^26.*counts in int32"):
        pair.add(x, x)
    pair._added = 2 ** 26 - 3
    with pytest.raises(AssertionError, match="library or device touched"):      # one field fewer passes every check
        pair.add(x, x)
    assert pair.fields == 0 and pair.counts.shape == (3, 2, 67, 64) and pair.counts.dtype == torch.int32
    assert single.counts.shape == (3, 1, 67, 64) and pair.nbytes == 3 * 2 * 67 * 64 * 4 and single.nbytes == 3 * 67 * 64 * 4
    assert GridHist(spec, 1024, 1024, device="meta").nbytes == 3 * 2 * 67 * 1024 * 1024 * 4        # the docstring's 1.6 GB

    class TwoRanks:                                                      # the limit holds again after the reduction
        world_size = 2

        @staticmethod
        def allreduce_sum_(t):
            t *= 2
    full = GridHist(spec, 2, 2, device="cpu")
    full._buf[-1] = 2 ** 25
    with pytest.raises(ValueError, match="would reach 2\\^26.*counts in int32"):
        full.reduce_(TwoRanks())
    ok = GridHist(spec, 2, 2, device="cpu")
    ok._buf[-1] = 2 ** 25 - 1
    assert ok.reduce_(TwoRanks()).fields == 2 ** 26 - 2


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_gridhist_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert "Per-gridpoint histograms (csrc/gridhist.hip)" in src
    assert re.search(r"#define DG_GRIDHIST_MAX_BINS 256\b", src) and re.search(r"#define DG_GRIDHIST_MAX_Q 16\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"const dg_eof_fields*": C.POINTER(_lib.EofFields), "const dg_hist_spec*": C.POINTER(_lib.HistSpec), "int": C.c_int,
             "const double*": C.POINTER(C.c_double)}
    for sym in ("dg_gridhist_ws_bytes", "dg_gridhist", "dg_gridhist_scan", "dg_gridhist_host", "dg_gridhist_scan_host"):
        m = re.search(rf"\b(size_t|int) {sym}\s*\(([^)]*)\)", code)
        assert m, sym
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
        args = [" ".join(a.split()[:-1]) for a in m.group(2).replace("\n", " ").split(",")]
        want = [ctype.get(a, C.c_void_p) for a in args]                 # every other pointer is passed as void*
        assert _lib._PROTOS[sym] == want, (sym, args)
        assert getattr(_lib.lib(), sym).restype == (C.c_size_t if m.group(1) == "size_t" else C.c_int)
    assert _lib.GRIDHIST_MAX_BINS == gridhist.BINS_MAX == 256 and _lib.GRIDHIST_MAX_Q == gridhist.Q_MAX == 16
    assert "gridhist.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=64, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    good = HistSpec.zscore(2, bins=64).struct()

    def spec(**kw):
        s = HistSpec.zscore(2, bins=64).struct()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    out = C.c_void_p(0x3000)
    call = lambda fa, fb, s, o=out: lib.dg_gridhist(fa, fb, s, None, o, None)
    assert call(f(base=0), None, C.byref(good)) == -1 and call(f(C=9), None, C.byref(good)) == -1
    assert call(f(T=0), None, C.byref(good)) == -1 and call(f(P=0), None, C.byref(good)) == -1
    assert call(f(), None, C.byref(good), None) == -1 and call(f(), None, None) == -1
    assert call(f(), None, spec(nbins=257)) == -1 and call(f(), None, spec(nbins=0)) == -1
    assert call(f(), None, spec(speed_u=2)) == -1 and call(f(), None, spec(inv_w=(1, 0.0))) == -1
    assert call(f(), None, spec(lo=(2, float("nan")))) == -1 and call(f(), None, spec(scale=(1, float("inf")))) == -1
    assert call(f(C=1), None, C.byref(good)) == -1                       # speed channel 1 of a 1-channel field
    assert call(f(), f(T=63), C.byref(good)) == -1 and call(f(), f(P=96), C.byref(good)) == -1
    assert call(f(), f(base=0), C.byref(good)) == -1 and call(f(C=3), f(C=2), C.byref(good)) == -1
    assert call(f(dtype=7), None, C.byref(good)) == -2 and call(f(), f(dtype=7), C.byref(good)) == -2
    assert lib.dg_gridhist_ws_bytes(f(), 1, spec(nbins=257)) == 0 and lib.dg_gridhist_ws_bytes(f(C=9), 0, C.byref(good)) == 0
    assert 0 < lib.dg_gridhist_ws_bytes(f(), 1, C.byref(good)) <= 4096   # no partial tables
    q = (C.c_double * 17)(*([0.5] * 17))
    p = C.c_void_p(0x1000)
    scan = lambda **kw: lib.dg_gridhist_scan(*[dict(dict(counts=p, nout=3, S=2, nbins=64, P=100, q=q, Q=3, ranks=p, dist=p, stream=None),
                                                    **kw)[k] for k in ("counts", "nout", "S", "nbins", "P", "q", "Q", "ranks", "dist", "stream")])
    for kw in (dict(counts=None), dict(ranks=None), dict(dist=None), dict(q=None), dict(nout=0), dict(nout=10), dict(S=0), dict(S=3),
               dict(nbins=0), dict(nbins=257), dict(P=0), dict(Q=0), dict(Q=17), dict(q=(C.c_double * 3)(0.5, 1.0, 0.2)),
               dict(q=(C.c_double * 3)(0.5, 0.0, 0.2)), dict(q=(C.c_double * 3)(0.5, float("nan"), 0.2))):
        assert scan(**kw) == -1, kw
    assert lib.dg_gridhist_host(None, p, None, 2, 1, 1, p) == -1 and lib.dg_gridhist_host(C.byref(good), None, None, 2, 1, 1, p) == -1
    assert lib.dg_gridhist_scan_host(p, 3, 2, 64, 100, q, 17, p, p) == -1 and lib.dg_gridhist_scan_host(p, 3, 2, 64, 100, q, 3, p, None) == -1


# ------------------------------------------------------------------------------------------------- the host references
@pytest.mark.parametrize("name,spec", specs())
def test_host_table_against_numpy(name, spec):
    T, H, W = 7, 16, 16
    rng = np.random.default_rng(3)
    assert len(special_values(spec)) <= T * H * W                    # every planted value has a cell of its own
    xa, xb = data(rng, spec, T, H, W), data(rng, spec, T, H, W, shift=3)
    a, b = cube(xa), cube(xb)
    want = table_ref(spec, a, b)
    got = gridhist.host_table(spec, xa.reshape(T, 2, -1), xb.reshape(T, 2, -1))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(gridhist.host_table(spec, xa.reshape(T, 2, -1)), table_ref(spec, a))
    assert got.dtype == np.int32 and got.shape == (spec.nout, 2, spec.bins + 3, H * W)
    np.testing.assert_array_equal(got.sum(axis=2), np.full((spec.nout, 2, H * W), T))           # every field lands in one row
    assert got[0, 0, :spec.bins + 2, H * W - 1].sum() == 0 and got[0, 0, spec.bins + 2, H * W - 1] == T   # the never-finite pixel
    assert got[:, :, 0].sum() > 0 and got[:, :, spec.bins + 1].sum() > 0 and got[:, :, spec.bins + 2].sum() > 0
    if spec.speed is not None:                                       # the (3, 4) pairs: speed exactly 5 opens row 1 + 5 / w
        pos = (np.arange(4) * 7919 + 13 + 11) % (T * H * W)
        rows = bins_ref(spec, a.reshape(2, -1))[2, pos]
        assert np.all(rows == 1 + 20)
    # chunks add up, and pooled over the pixels the table is the value histogram's
    two = gridhist.host_table(spec, xa[:2].reshape(2, 2, -1), xb[:2].reshape(2, 2, -1)) + \
        gridhist.host_table(spec, xa[2:].reshape(T - 2, 2, -1), xb[2:].reshape(T - 2, 2, -1))
    np.testing.assert_array_equal(two, want)
    pooled = np.stack([np.bincount(r, minlength=spec.bins + 3) for r in bins_ref(spec, a.reshape(2, -1))])
    np.testing.assert_array_equal(got[:, 0].sum(axis=2), pooled)


@pytest.mark.parametrize("P", [1, 5, 64])
@pytest.mark.parametrize("q", [[0.5], Q3, Q16], ids=["Q1", "Q3", "Q16"])
def test_host_scan_against_numpy(P, q):
    for name, c in hand_tables(P):
        ranks, dist = gridhist.host_scan(c, q)
        want_r, want_d = scan_ref(c, q)
        np.testing.assert_array_equal(ranks, want_r, err_msg=name)
        np.testing.assert_array_equal(dist, want_d, err_msg=name)
        one_r, one_d = gridhist.host_scan(c[:, 1:], q)               # S = 1: no dist
        assert one_d is None
        np.testing.assert_array_equal(one_r, want_r[:, 1:], err_msg=name)


def test_host_scan_edge_cases_by_hand():
    bins = 8
    c = hand_table(9, bins, np.random.default_rng(0), nout=1)
    q = [0.5, 0.25, float(np.nextafter(0.25, 0.0)), float(np.nextafter(0.25, 1.0))]
    ranks, dist = gridhist.host_scan(c, q)
    assert ranks[0, 0, :, :, 0].tolist() == [[-1, 0, 0]] * 4 and ranks[0, 1, 0, 0, 0] >= 0           # n = 0 on the real side only
    assert dist[0, :, 0].tolist() == [-1, -1]
    assert ranks[0, 0, 0, :, 1].tolist() == [2, 0, 7] and ranks[0, 1, 0, :, 1].tolist() == [3, 0, 8]  # one interior row
    assert ranks[0, 0, :, 0, 2].tolist() == [0] * 4 and ranks[0, 0, :, 0, 3].tolist() == [bins + 1] * 4  # under / overflow only
    assert dist[0, :, 2].tolist() == [0, 0] and dist[0, :, 3].tolist() == [0, 0]
    # pattern 5, real side: one value in each of rows 0 .. 3; q n = 2 exactly -> the second value (row 1), not the third
    assert ranks[0, 0, 0, :, 5].tolist() == [1, 1, 1] and ranks[0, 0, 1, :, 5].tolist() == [0, 0, 1]
    # pattern 6, generated side: one value in each of rows 0 .. 7; q n = 2 - ulp -> k = 2 (row 1); 2 + ulp -> k = 3 (row 2)
    assert 8 * q[2] < 2 < 8 * q[3]
    assert ranks[0, 1, 1, :, 6].tolist() == [1, 1, 1] and ranks[0, 1, 2, :, 6].tolist() == [1, 1, 1]
    assert ranks[0, 1, 3, :, 6].tolist() == [2, 2, 1]
    # real side of pattern 6: two values in each of rows 0, 2, 4 and one in rows 6, 8
    assert ranks[0, 0, 1, :, 6].tolist() == [0, 0, 2] and ranks[0, 0, 3, :, 6].tolist() == [2, 2, 2]
    na, nb = c[0, 0, :bins + 2, 7].sum(), c[0, 1, :bins + 2, 7].sum()
    assert na > 2 ** 26 - 200 and dist[0, 0, 7] > 0 and dist[0, 1, 7] <= int(na) * int(nb)            # no int64 wrap near the limit


# ------------------------------------------------------------------------------------------------- GridHistMaps on the host
def pixel_hist(spec, col, fields):
    """The histograms.Histogram of one pixel's column int [nout, bins + 3] (extrema lo / hi: no value outside the range)."""
    ext = torch.from_numpy(np.stack([spec.lo, spec.hi], axis=1).copy())
    return Histogram(spec, torch.from_numpy(col.astype(np.int64)), torch.zeros(spec.nout, 2, dtype=torch.float64), ext, fields)


def test_maps_against_the_pooled_histogram_functions(tmp_path):
    """quantile, w1 and ks of a pixel whose values all lie in [lo, hi) equal Histogram.quantile, wasserstein1 and ks_distance of
    that pixel's column to 1e-12: both sides are a handful of float64 operations on the same integers, and W1 differs only in
    the order of a sum of at most 257 terms."""
    H, W, T = 4, 5, 40
    spec = HistSpec(32, [-3.0, 0.0, 0.0], [3.0, 6.0, 9.0], scale=[1.0, 2.0], offset=[0.0, 3.0])
    rng = np.random.default_rng(2)
    xa = rng.standard_normal((T, 2, H * W)).astype(F32).clip(-1.4, 1.4)              # every output inside its range
    xb = (rng.standard_normal((T, 2, H * W)) * 0.7 + 0.3).astype(F32).clip(-1.4, 1.4)
    xa[:, :, 3], xb[:, :, 3] = 5.0, -5.0                             # pixel 3: everything out of range (not compared below)
    xb[::2, 0, 7] = np.nan                                           # pixel 7: na != nb in channel 0 and the speed
    xa[:, 1, 11] = np.nan                                            # pixel 11: no finite real value in channel 1 and the speed
    t = gridhist.host_table(spec, xa, xb)
    m = GridHistMaps(spec, H, W, True, torch.from_numpy(t), T)
    q = [0.05, 0.5, 0.95, 0.99]
    quant = {s: m.quantile(q, s).reshape(3, len(q), -1) for s in ("real", "fake")}
    w1, ks = m.w1().reshape(3, -1), m.ks().reshape(3, -1)
    inside = (m.out_of_range("real").reshape(3, -1) == 0) & (m.out_of_range("fake").reshape(3, -1) == 0)
    assert inside.sum() >= 3 * (H * W - 3)
    for p in range(H * W):
        ha, hb = pixel_hist(spec, t[:, 0, :, p], T), pixel_hist(spec, t[:, 1, :, p], T)
        qa, qb, w, k = ha.quantile(q), hb.quantile(q), histograms.wasserstein1(ha, hb), histograms.ks_distance(ha, hb)
        for j in range(3):
            if inside[j, p]:
                np.testing.assert_allclose(quant["real"][j, :, p], qa[j], rtol=1e-12, atol=0)
                np.testing.assert_allclose(quant["fake"][j, :, p], qb[j], rtol=1e-12, atol=0)
                np.testing.assert_allclose(w1[j, p], w[j], rtol=1e-12, atol=0)
                np.testing.assert_allclose(ks[j, p], k[j], rtol=1e-12, atol=0)
    assert np.all(m.quantile(0.5, "real")[:, 0, 3] == spec.hi) and np.all(m.quantile(0.5, "fake")[:2, 0, 3] == spec.lo[:2])
    assert np.all(m.out_of_range("real")[:, 0, 3] == 1.0) and m.quantile(0.5).shape == (3, H, W)
    assert np.isnan(m.quantile(0.5, "real")[1, 2, 1]) and np.isnan(w1[1, 11]) and np.isnan(ks[2, 11]) and np.isnan(m.out_of_range()[1, 2, 1])
    assert m.count("fake")[0, 1, 2] == T // 2 and m.nan("fake")[0, 1, 2] == T // 2 and m.count("real")[0, 1, 2] == T
    np.testing.assert_array_equal(m.quantile_bias(q), m.quantile(q, "fake") - m.quantile(q, "real"))
    for s, side in enumerate(("real", "fake")):
        np.testing.assert_array_equal(m.pooled(side), t[:, s].astype(np.int64).sum(axis=2))
    np.testing.assert_array_equal(m.table(), t)
    s = m.summary(q)
    assert json.loads(json.dumps(s, allow_nan=False)) == s
    assert s["channels"] == ["ch0", "ch1", "speed"] and s["fields"] == T and s["grid"] == [H, W] and s["q"] == q
    assert s["nbytes"] == t.size * 4 and s["nan"]["fake"][0] == T // 2 and s["nan"]["real"][1] == T
    for j in range(3):
        np.testing.assert_allclose(s["w1_mean"][j], np.nanmean(w1[j]), rtol=1e-12)
        np.testing.assert_allclose(s["ks_max"][j], np.nanmax(ks[j]), rtol=1e-12)
        assert s["ks_worst_pixel"][j] == [int(np.nanargmax(ks[j])) // W, int(np.nanargmax(ks[j])) % W]
        bias = np.abs(m.quantile_bias(q)).reshape(3, len(q), -1)
        np.testing.assert_allclose(s["abs_quantile_bias_max"][2][j], np.nanmax(bias[j, 2]), rtol=1e-12)
        np.testing.assert_allclose(s["abs_quantile_bias_mean"][1][j], np.nanmean(bias[j, 1]), rtol=1e-12)
    names = m.save(str(tmp_path / "q"), q)
    assert set(names) == {"summary.json", "quantile_bias.npy", "w1.npy", "ks.npy"} | {
        f"{sd}_{k}.npy" for sd in ("real", "fake") for k in ("count", "nan", "out_of_range", "quantile")}
    assert json.load(open(tmp_path / "q" / "summary.json")) == s
    for k, v in m.maps(q).items():
        np.testing.assert_array_equal(np.load(tmp_path / "q" / (k + ".npy")), v)
    one = GridHistMaps(spec, H, W, False, torch.from_numpy(t[:, :1].copy()), T)
    json.dumps(one.summary(), allow_nan=False)
    assert set(one.maps()) == {f"real_{k}" for k in ("count", "nan", "out_of_range", "quantile")}
    np.testing.assert_array_equal(one.quantile(q), m.quantile(q, "real"))


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def hist_emu_ops():
    from oracle.emu_ops import EmuOps

    class GridHistEmuOps(EmuOps):
        """The emulated ops plus dg_gridhist's and dg_gridhist_scan's contracts in numpy."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            P = t.shape[1] * t.shape[2] if nhwc else t.shape[2] * t.shape[3]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=P)

        def gridhist_ws_bytes(self, f, paired, spec):
            return 1

        def gridhist(self, fa, fb, s, counts):
            def values(f):
                x = f.t[..., :f.C].permute(3, 0, 1, 2) if f.nhwc else f.t[:, :f.C].permute(1, 0, 2, 3)
                return x.detach().float().cpu().numpy().reshape(f.C, f.T, -1)
            speed = None if s.speed_u < 0 else (s.speed_u, s.speed_v)
            nout = fa.C + (speed is not None)
            spec = types.SimpleNamespace(nout=nout, bins=s.nbins, speed=speed, scale=np.array(s.scale[:fa.C], F32),
                                         offset=np.array(s.offset[:fa.C], F32), lo=np.array(s.lo[:nout], F32),
                                         inv_w=np.array(s.inv_w[:nout], F32))
            counts += torch.from_numpy(table_ref(spec, values(fa), None if fb is None else values(fb)))

        def gridhist_scan(self, counts, q, ranks, dist=None):
            r, d = scan_ref(counts.numpy(), list(q))
            ranks.copy_(torch.from_numpy(r))
            if dist is not None:
                dist.copy_(torch.from_numpy(d))

    return GridHistEmuOps("f32")


def _trainer(on, dist=None, fs=False, qdir=None):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.GAN.wasserstein_fs import WassersteinGANFS
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = (WassersteinGANFS if fs else WassersteinGAN)(G, C_, dist=dist)
    tr.log_quantile_maps = on
    tr.quantile_map_dir = qdir
    return tr


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: hist_emu_ops())
    setattr_(losses, "_ops", {})
    setattr_(histograms, "_ops", {})


def _loaders(lo=0, step=1, batch=2):
    from downgan_amd import synthetic
    from downgan_amd.GAN.dataloader import NetCDFSR
    coarse, fine = synthetic.tiles(6, 2, 16, seed=11)
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b][lo::step].copy()), torch.from_numpy(fine[a:b][lo::step].copy()))
    dl = torch.utils.data.DataLoader(ds(0, 2), batch_size=batch)
    tl = torch.utils.data.DataLoader(ds(2, 6), batch_size=batch)
    return dl, tl


def _run_epoch(on, dist=None, lo=0, step=1, batch=2, fs=False, qdir=None):
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    tr = _trainer(on, dist, fs, qdir)
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr


def test_hook_off_leaves_the_summary_and_the_calls_unchanged(monkeypatch, tmp_path):
    import downgan_amd.config.hyperparams as hp
    from downgan_amd.engine import TrainEngine
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    assert WassersteinGAN.log_quantile_maps is False and WassersteinGAN.quantile_map_spec is None
    assert WassersteinGAN.quantile_map_q == (0.5, 0.95, 0.99) and WassersteinGAN.quantile_map_dir is None
    assert WassersteinGAN.quantile_map_results is None
    seen = []
    real_pass = TrainEngine.metrics_pass

    def spy(self, *a, **kw):
        seen.append(set(kw))
        return real_pass(self, *a, **kw)
    monkeypatch.setattr(TrainEngine, "metrics_pass", spy)
    t_off = _run_epoch(False)
    off = t_off.metrics_log[0]
    assert "quantile_maps" not in off and t_off.quantile_map_results is None
    assert seen and not any("hist_maps" in kw for kw in seen)        # the new keyword is handed down only when the hook is on
    del seen[:]
    tr = _run_epoch(True, qdir=str(tmp_path / "q"))
    assert seen and all("hist_maps" in kw for kw in seen)
    on = dict(tr.metrics_log[0])
    d = on.pop("quantile_maps")
    assert json.dumps(on, sort_keys=True) == json.dumps(off, sort_keys=True)    # the hook adds a key and changes nothing else
    json.dumps(d, allow_nan=False)
    assert set(d) == {"train", "test"} == set(tr.quantile_map_results)
    for part, n in (("train", 2), ("test", 4)):
        res = tr.quantile_map_results[part]
        assert d[part]["fields"] == n == res.fields and d[part]["channels"] == ["ch0", "ch1", "speed"]
        assert d[part]["bins"] == 64 and d[part]["q"] == [0.5, 0.95, 0.99] and d[part] == res.summary((0.5, 0.95, 0.99))
        assert os.path.exists(tmp_path / "q" / "0" / part / "summary.json")
        assert np.load(tmp_path / "q" / "0" / part / "quantile_bias.npy").shape == (3, 3, 128, 128)
        assert np.load(tmp_path / "q" / "0" / part / "w1.npy").shape == (3, 128, 128)
    from downgan_amd import synthetic
    _, fine = synthetic.tiles(6, 2, 16, seed=11)
    spec = HistSpec.zscore(2, bins=64, lim=6.0)
    got = tr.quantile_map_results["test"].table()
    np.testing.assert_array_equal(got[:, 0], table_ref(spec, cube(fine[2:6]))[:, 0])    # the real side of the pair is the test set
    np.testing.assert_array_equal(got[:, 0], gridhist.host_table(spec, fine[2:6].reshape(4, 2, -1))[:, 0])
    np.testing.assert_array_equal(got.sum(axis=2), np.full((3, 2, 128 * 128), 4))


def test_hook_without_log_metrics(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    monkeypatch.setattr(WassersteinGAN, "log_metrics", False)
    s = _run_epoch(True).metrics_log[0]
    assert "train" not in s and s["quantile_maps"]["train"]["fields"] == 2 and s["quantile_maps"]["test"]["fields"] == 4


def test_frequency_separation_trainer_reports_quantile_maps(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    s = _run_epoch(True, fs=True).metrics_log[0]
    assert s["quantile_maps"]["train"]["fields"] == 2 and s["quantile_maps"]["test"]["fields"] == 4


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import downgan_amd.config.hyperparams as hp
    _patch(setattr)
    hp.batch_size, hp.lr = 1, 0.0
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    tr = _run_epoch(True, dist=d, lo=rank, step=world, batch=1)
    res = {k: v.table() for k, v in tr.quantile_map_results.items()}
    torch.save({"summary": tr.metrics_log[0]["quantile_maps"], "tables": res}, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_table(monkeypatch):
    """lr = 0 keeps G identical in both runs, so the generated fields are the same and only the reduction is tested: the
    reduced table equals the single-process table of the concatenated data."""
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(hp, "lr", 0.0)
    torch.set_num_threads(4)
    tr = _run_epoch(True)
    ref = tr.quantile_map_results
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["summary"] == r1["summary"]
    for part in ("train", "test"):
        assert r0["summary"][part]["fields"] == ref[part].fields
        assert r0["summary"][part] == tr.metrics_log[0]["quantile_maps"][part]
        for r in (r0, r1):
            np.testing.assert_array_equal(r["tables"][part], ref[part].table())
