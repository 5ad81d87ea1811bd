"""Empirical quantile mapping without a GPU: the two host references (dg_qmap_fit_host, dg_qmap_apply_host) against the numpy
restatement of the definition (tests/qmap_ref.py) bit for bit, the properties of the map, what the method buys on a planted
bias, argument checks that fire before any library call, the ABI surface, the save / load round trip and
``Generator.generate`` on the emulated ops."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from downgan_amd import _lib, gridhist, qmap
from downgan_amd.gridhist import GridHist, GridHistMaps
from downgan_amd.histograms import HistSpec
from downgan_amd.qmap import QuantileMap

from . import qmap_ref as R
from .test_gridhist_cpu import data, specs
from .test_gridstats_cpu import _no_library
from .test_histograms_cpu import F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tables(P, bins, nout=2):
    rng = np.random.default_rng(100 * bins + P)
    return [("hand", R.hand_table(P, bins, rng, nout)), ("random", R.random_table(P, bins, rng, nout))]


def check_nodes(nodes, counts, lo, width, name):
    """The properties every fitted table has: monotone nodes, the two shift rows, the identity where a == b or a side is empty."""
    nout, nb3, P = nodes.shape
    bins = nb3 - 3
    assert np.all(np.diff(nodes[:, :bins + 1].astype(np.float64), axis=1) >= 0), name
    hi = (lo.astype(np.float64)[:, None] + bins * width[:, None]).astype(F32)
    np.testing.assert_array_equal(nodes[:, bins + 1], (nodes[:, 0] - lo[:, None]).astype(F32), err_msg=name)
    np.testing.assert_array_equal(nodes[:, bins + 2], (nodes[:, bins] - hi).astype(F32), err_msg=name)
    ident = (lo.astype(np.float64)[:, None] + np.arange(bins + 1)[None, :] * width[:, None]).astype(F32)     # fp32(lo + k w)
    fin = counts[:, :, :bins + 2].astype(np.int64)
    same = np.all(fin[:, 0] == fin[:, 1], axis=1) | (fin[:, 0].sum(axis=1) == 0) | (fin[:, 1].sum(axis=1) == 0)     # [nout, P]
    for j, p in zip(*np.nonzero(same)):
        np.testing.assert_array_equal(nodes[j, :bins + 1, p], ident[j], err_msg=f"{name} identity at {j}, {p}")
        assert nodes[j, bins + 1, p] == 0 and nodes[j, bins + 2, p] == 0, (name, j, p)
    return int(same.sum())


# ------------------------------------------------------------------------------------------------- the host references
@pytest.mark.parametrize("P", [1, 5, 67])
@pytest.mark.parametrize("bins", [1, 2, 64, 256])
def test_host_fit_equals_the_numpy_definition(bins, P):
    lo, width = R.spec_axes(bins)
    for name, c in tables(P, bins):
        got = qmap.host_fit(c, lo, width)
        assert got.dtype == np.float32 and got.shape == (2, bins + 3, P)
        np.testing.assert_array_equal(R.bits(got), R.bits(R.fit_ref(c, lo, width)), err_msg=name)
        assert np.all(np.isfinite(got))
        n_ident = check_nodes(got, c, lo, width, name)
        if name == "hand":
            assert n_ident >= 2 * min(P, 3)                          # patterns 0 .. 2 (and 5, 8) are identities
    both = c.copy()
    both[:, 1] = both[:, 0]                                          # a == b everywhere, empty bins included
    assert check_nodes(qmap.host_fit(both, lo, width), both, lo, width, "a == b") == 2 * P


def test_host_fit_by_hand():
    """Four bins on [0, 4]: a generated sample shifted one bin up is mapped one bin down, and flat stretches of the real CDF take
    the point nearest to the edge."""
    lo, w = np.array([0.0], F32), np.array([1.0])
    c = np.zeros((1, 2, 7, 3), np.int32)
    c[0, 0, :, 0] = [0, 4, 4, 0, 0, 0, 9]                            # real: bins 0, 1
    c[0, 1, :, 0] = [0, 0, 4, 4, 0, 0, 1]                            # generated: bins 1, 2
    c[0, 0, :, 1] = [2, 0, 0, 4, 0, 2, 0]                            # real: under, bin 2, over
    c[0, 1, :, 1] = [0, 2, 2, 2, 2, 0, 0]                            # generated: uniform
    c[0, 0, :, 2] = [0, 0, 0, 0, 8, 0, 0]                            # real: all in the last bin
    c[0, 1, :, 2] = [0, 8, 0, 0, 0, 0, 0]                            # generated: all in the first
    n = qmap.host_fit(c, lo, w)[0]
    # pixel 0: G = 0, 0, 4, 8, 8 of 8; the real CDF is 0 on [.., 0], 4 at 1, 8 on [2, 4]: edges 3 and 4 lie in that last interval
    assert n[:5, 0].tolist() == [0.0, 0.0, 1.0, 3.0, 4.0] and n[5:, 0].tolist() == [0.0, 0.0]
    # pixel 1: X = 0, 16, 32, 48, 64 against B' = 16, 16, 16, 48, 48 (overflow mass above): 0 -> below the underflow mass -> 0;
    # 16 -> [0, 2] -> 1; 32 -> half way through bin 2 -> 2.5; 48 -> [3, 4] -> 3; 64 > B'_4 -> 4
    assert n[:5, 1].tolist() == [0.0, 1.0, 2.5, 3.0, 4.0] and n[5:, 1].tolist() == [0.0, 0.0]
    # pixel 2: X = 0 -> 0 (nearest point of [.., 3]), then 64 = B'_4 reached at pos 4 exactly
    assert n[:5, 2].tolist() == [0.0, 4.0, 4.0, 4.0, 4.0] and n[5:, 2].tolist() == [0.0, 0.0]
    np.testing.assert_array_equal(R.bits(n), R.bits(R.fit_ref(c, lo, w)[0]))


def special(spec, nodes, T, H, W, seed):
    """float32 [T, C, P]: the planted data of test_gridhist_cpu (every edge and its fp32 neighbours, +-0, denormals, +-inf, NaN,
    +-FLT_MAX, a never-finite pixel)."""
    return data(np.random.default_rng(seed), spec, T, H, W).reshape(T, 2, H * W)


@pytest.mark.parametrize("name,spec", specs())
def test_host_apply_equals_the_numpy_definition(name, spec):
    T, H, W = 7, 16, 16
    P = H * W
    x = special(spec, None, T, H, W, 5)
    rng = np.random.default_rng(7)
    with np.errstate(over="ignore"):                                 # 1.25 FLT_MAX
        other = special(spec, None, T, H, W, 6) * F32(1.25)
    fitted = qmap.host_fit(gridhist.host_table(spec, x, other), spec.lo, spec.width())
    hand = qmap.host_fit(R.hand_table(P, spec.bins, rng, spec.nout), spec.lo, spec.width())
    for what, nodes in (("fitted", fitted), ("hand", hand)):
        got = qmap.host_apply(spec, x, nodes)
        assert got.dtype == np.float32 and got.shape == (T, spec.nout, P)
        np.testing.assert_array_equal(R.bits(got), R.bits(R.apply_ref(spec, x, nodes)), err_msg=what)
        y = R.transform_ref(spec, np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(2, -1)).reshape(spec.nout, T, P)
        for j in range(spec.nout):
            yj, oj = y[j], got[:, j]
            nan = np.isnan(yj)
            assert nan.any() and np.all(oj[nan].view(np.uint32) == 0x7fc00000) and not np.isnan(oj[~nan]).any()
            assert np.all(oj[yj == np.inf] == np.inf) and np.all(oj[yj == -np.inf] == -np.inf)
            with np.errstate(over="ignore", invalid="ignore"):
                t = ((yj - spec.lo[j]).astype(F32) * spec.inv_w[j]).astype(F32)
                low, high = t < 0, t >= spec.bins
                assert (low.any() or j == spec.C) and high.any()                    # a speed is never below lo = 0
                d_lo, d_hi = np.broadcast_to(nodes[j, spec.bins + 1], yj.shape), np.broadcast_to(nodes[j, spec.bins + 2], yj.shape)
                np.testing.assert_array_equal(oj[low], (yj[low] + d_lo[low]).astype(F32))
                np.testing.assert_array_equal(oj[high], (yj[high] + d_hi[high]).astype(F32))
            rows = np.where(low, 0, np.where(high, spec.bins + 1, 1 + np.where(low | high | nan, 0, t).astype(np.int64)))
            R.assert_order_preserving(yj, oj, rows, nan, spec.lo[j], spec.hi[j], spec.bins, (what, j))


def test_identity_map_returns_the_value_to_four_ulp():
    """Under the identity nodes fp32(lo + k w) an in-range y comes back as n_k + f (n_{k+1} - n_k): three roundings at the scale of
    the range, so within 4 ulp of max(|lo|, |hi|)."""
    for bins in (1, 64, 256):
        spec = HistSpec(bins, [-6.0], [6.0], speed=None)
        P = 4096
        rng = np.random.default_rng(bins)
        edges = spec.edges()[0].astype(F32)
        y = np.concatenate([rng.uniform(-6, 6, P - 3 * len(edges) % P).astype(F32), edges, np.nextafter(edges, F32(-9)),
                            np.nextafter(edges, F32(9))])
        y = y[(y >= -6) & (y < 6)]
        nodes = qmap.host_fit(np.zeros((1, 2, bins + 3, len(y)), np.int32), spec.lo, spec.width())      # nothing to calibrate on
        out = qmap.host_apply(spec, y.reshape(1, 1, -1), nodes)[0, 0]
        err = np.abs(out.astype(np.float64) - y.astype(np.float64)).max()
        print(f"bins {bins}: identity error {err / np.spacing(F32(6.0)):.2f} ulp of 6")
        assert err <= 4 * np.spacing(F32(6.0))


@pytest.mark.parametrize("seed", [1, 2])
def test_mapping_removes_a_planted_bias(seed):
    """real = g = mu_p + sigma_p z against gen = 0.4 + 1.3 g' (g' an independent sample of g; at every fourth pixel g is skewed to
    sign(g) |g|^1.5, so that some values leave the range): after mapping gen through the map fitted on
    (real, gen), the sample W1 (mean absolute difference of the sorted samples) per pixel is at most half a bin width and at most
    the W1 before, on the pixels where neither side has an out-of-range count -- which must be at least 3/4 of them (how many are is a
    property of the drawn data alone, not of the map: seeds 1 and 2 are the first two whose table has that many; 0 has 15)."""
    P, T = 24, 400
    spec = HistSpec(64, [-6.0], [6.0], speed=None)
    rng = np.random.default_rng(seed)
    mu, sigma = 0.5 * rng.standard_normal(P), rng.uniform(0.5, 1.5, P)
    skew = lambda g: np.where(np.arange(P) % 4 == 0, np.sign(g) * np.abs(g) ** 1.5, g)
    real = skew(mu + sigma * rng.standard_normal((T, P))).astype(F32).reshape(T, 1, P)
    gen = (0.4 + 1.3 * skew(mu + sigma * rng.standard_normal((T, P)))).astype(F32).reshape(T, 1, P)
    table = gridhist.host_table(spec, real, gen)
    m = QuantileMap.fit(GridHistMaps(spec, 1, P, True, torch.from_numpy(table), T))
    assert m.valid.all() and m.fields == T and m.nodes.shape == (1, 67, P)
    out = m.apply(torch.from_numpy(gen).view(T, 1, 1, P)).numpy().reshape(T, P)
    np.testing.assert_array_equal(R.bits(out), R.bits(qmap.host_apply(spec, gen, m.nodes.numpy())[:, 0]))
    inside = (table[0, :, 0] == 0).all(axis=0) & (table[0, :, 65] == 0).all(axis=0)
    w1 = lambda a, b: np.abs(np.sort(a.astype(np.float64), axis=0) - np.sort(b.astype(np.float64), axis=0)).mean(axis=0)
    before, after = w1(gen[:, 0], real[:, 0]), w1(out, real[:, 0])
    w = spec.width()[0]
    print(f"{inside.sum()} of {P} pixels inside; W1 before {before[inside].min():.3f} .. {before[inside].max():.3f}, "
          f"after {after[inside].min():.4f} .. {after[inside].max():.4f} (w = {w})")
    assert inside.sum() >= 3 * P // 4
    assert np.all(after[inside] <= 0.5 * w) and np.all(after[inside] <= before[inside])


# ------------------------------------------------------------------------------------------------- argument checks
def test_arguments_are_checked_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    spec = HistSpec(64, [-6.0, -6.0], [6.0, 6.0], speed=None)
    nodes = lambda s, P: torch.zeros(s.nout, s.bins + 3, P)
    with pytest.raises(TypeError, match="takes a histograms.HistSpec"):
        QuantileMap(object(), 8, 8, nodes(spec, 64), None, 0)
    with pytest.raises(TypeError, match="takes a histograms.HistSpec"):
        qmap.quantile_map(torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8), spec="zscore")
    with pytest.raises(TypeError, match="takes a histograms.HistSpec"):
        qmap.host_apply(None, np.zeros((1, 2, 4), F32), np.zeros((2, 67, 4), F32))
    with pytest.raises(ValueError, match="at most 256 bins"):
        big = HistSpec.zscore(2)                                     # the default 2048 bins of zscore
        QuantileMap(big, 8, 8, nodes(big, 64), None, 0)
    with pytest.raises(ValueError, match="at most 256 bins"):
        qmap.quantile_map(torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8), spec=HistSpec.zscore(2))
    with pytest.raises(ValueError, match="pair"):
        QuantileMap.fit(GridHistMaps(spec, 2, 2, False, torch.zeros(2, 1, 67, 4, dtype=torch.int32), 0))
    with pytest.raises(ValueError, match="pair"):
        QuantileMap.fit(GridHist(spec, 2, 2, paired=False, device="cpu"))
    with pytest.raises(ValueError, match="pair"):
        qmap.quantile_map(torch.zeros(2, 2, 8, 8), None, spec=spec)
    with pytest.raises(ValueError, match="pair"):
        qmap.host_fit(np.zeros((2, 1, 67, 4), np.int32), spec.lo, spec.width())
    with pytest.raises(TypeError, match="GridHistMaps or GridHist"):
        QuantileMap.fit(torch.zeros(2, 2, 67, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="nodes are float32"):
        QuantileMap(spec, 8, 8, nodes(spec, 63), None, 0)
    for bad in (None, torch.ones(2, 8, 8), torch.ones(2, 64, dtype=torch.bool), torch.ones(3, 8, 8, dtype=torch.bool)):
        with pytest.raises(ValueError, match="valid is a bool tensor"):
            QuantileMap(spec, 8, 8, nodes(spec, 64), bad, 0)
    m = QuantileMap(spec, 8, 8, nodes(spec, 64), torch.ones(2, 8, 8, dtype=torch.bool), 0)
    x = torch.zeros(2, 2, 8, 8)
    for bad, kw, err, match in ((torch.zeros(2, 2, 8, 4), {}, ValueError, "8 x 8 grid"),
                                (torch.zeros(2, 3, 8, 8), {}, ValueError, "C = 2"),
                                (torch.zeros(2, 8, 8, 4), {"nhwc": True}, ValueError, "C = 2"),
                                (torch.zeros(2, 8, 8, 4), {"nhwc": True, "channels": 5}, ValueError, "channels"),
                                (torch.zeros(2, 2, 8, 8, dtype=torch.float64), {}, TypeError, "fp32 or bf16"),
                                (np.zeros((2, 2, 8, 8), F32), {}, TypeError, "tensor"),
                                (torch.zeros(2, 8, 8), {}, ValueError, "shape"),
                                (torch.zeros(0, 2, 8, 8), {}, ValueError, "at least one")):
        with pytest.raises(err, match=match):
            m.apply(bad, **kw)
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            m.apply(x, n_valid=n)
    for out in (torch.zeros(1, 2, 8, 8), torch.zeros(2, 2, 8, 8, dtype=torch.float64), torch.zeros(2, 2, 8, 9)[..., :8],
                torch.zeros(2, 3, 8, 8)):
        with pytest.raises(ValueError, match="out is a contiguous float32"):
            m.apply(x, out=out)
    with pytest.raises(AssertionError, match="library or device touched"):                # every check passed
        m.apply(x, out=torch.zeros(3, 2, 8, 8))
    from downgan_amd.networks.generator import Generator
    G = Generator(16, 128, 2, 2, num_res_blocks=1, device="cpu")
    coarse = torch.zeros(2, 2, 16, 16)
    speedy = HistSpec.zscore(2, bins=64, lim=6.0)
    with pytest.raises(ValueError, match="no speed channel"):
        G.generate(coarse, qmap=QuantileMap(speedy, 128, 128, nodes(speedy, 128 * 128), torch.ones(3, 128, 128, dtype=torch.bool), 0))
    one = HistSpec(64, [-6.0], [6.0], speed=None)
    with pytest.raises(ValueError, match="C = 2 input channels"):
        G.generate(coarse, qmap=QuantileMap(one, 128, 128, nodes(one, 128 * 128), torch.ones(1, 128, 128, dtype=torch.bool), 0))
    with pytest.raises(TypeError, match="QuantileMap"):
        G.generate(coarse, qmap=spec)


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_qmap_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert "Empirical quantile mapping (csrc/qmap.hip)" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"const dg_eof_fields*": C.POINTER(_lib.EofFields), "const dg_hist_spec*": C.POINTER(_lib.HistSpec), "int": C.c_int,
             "const double*": C.POINTER(C.c_double), "const float* lo": C.POINTER(C.c_float)}
    for sym in ("dg_qmap_fit", "dg_qmap_apply", "dg_qmap_fit_host", "dg_qmap_apply_host"):
        m = re.search(rf"\bint {sym}\s*\(([^)]*)\)", code)
        assert m, sym
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
        decl = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        want = [ctype.get(a, ctype.get(" ".join(a.split()[:-1]), C.c_void_p)) for a in decl]     # every other pointer goes as void*
        assert _lib._PROTOS[sym] == want, (sym, decl)
        assert getattr(_lib.lib(), sym).restype == C.c_int
    assert "qmap.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()
    assert "not applied here" not in gridhist.__doc__ and "qmap" in gridhist.__doc__


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    p = C.c_void_p(0x1000)
    lo, w = (C.c_float * 9)(*([-6.0] * 9)), (C.c_double * 9)(*([0.1875] * 9))
    fit_args = ("counts", "nout", "nbins", "P", "lo", "width", "nodes")
    good = dict(counts=p, nout=3, nbins=64, P=100, lo=lo, width=w, nodes=p)
    bad = (dict(counts=None), dict(nodes=None), dict(lo=None), dict(width=None), dict(nout=0), dict(nout=10), dict(nbins=0),
           dict(nbins=257), dict(P=0), dict(P=-4), dict(lo=(C.c_float * 3)(0.0, float("nan"), 0.0)),
           dict(lo=(C.c_float * 3)(0.0, float("inf"), 0.0)), dict(width=(C.c_double * 3)(1.0, 0.0, 1.0)),
           dict(width=(C.c_double * 3)(1.0, -1.0, 1.0)), dict(width=(C.c_double * 3)(1.0, float("nan"), 1.0)),
           dict(width=(C.c_double * 3)(1.0, float("inf"), 1.0)))
    for kw in bad:
        a = [dict(good, **kw)[k] for k in fit_args]
        assert lib.dg_qmap_fit(*a, None) == -1, kw
        assert lib.dg_qmap_fit_host(*a) == -1, kw
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=64, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))

    def spec(**kw):
        s = HistSpec.zscore(2, bins=64).struct()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    call = lambda fx, s, nodes=p, out=p: lib.dg_qmap_apply(fx, s, nodes, out, None)
    assert call(None, spec()) == -1 and call(f(), None) == -1 and call(f(), spec(), None) == -1 and call(f(), spec(), p, None) == -1
    assert call(f(base=0), spec()) == -1 and call(f(C=9), spec()) == -1 and call(f(T=0), spec()) == -1 and call(f(P=0), spec()) == -1
    assert call(f(), spec(nbins=257)) == -1 and call(f(), spec(nbins=0)) == -1 and call(f(), spec(speed_u=2)) == -1
    assert call(f(), spec(inv_w=(1, 0.0))) == -1 and call(f(), spec(lo=(2, float("nan")))) == -1
    assert call(f(), spec(scale=(1, float("inf")))) == -1 and call(f(C=1), spec()) == -1
    assert call(f(dtype=7), spec()) == -2
    host = lambda s=spec(), x=p, Cn=2, T=1, P=1, nodes=p, out=p: lib.dg_qmap_apply_host(s, x, Cn, T, P, nodes, out)
    assert host(s=None) == -1 and host(x=None) == -1 and host(nodes=None) == -1 and host(out=None) == -1
    assert host(Cn=9) == -1 and host(Cn=1) == -1 and host(T=0) == -1 and host(P=0) == -1 and host(s=spec(nbins=257)) == -1


# ------------------------------------------------------------------------------------------------- the module
def test_fit_transfer_and_save_load_round_trip(tmp_path):
    T, H, W = 9, 6, 7
    spec = HistSpec(32, [-8.0, -8.0, 0.0], [8.0, 8.0, 16.0], scale=[2.0, 0.5], offset=[-1.0, 0.25], names=["u", "v", "speed"])
    rng = np.random.default_rng(4)
    real, fake = (torch.from_numpy(rng.standard_normal((T, 2, H, W)).astype(F32) * s) for s in (2.0, 3.0))
    fake[:, 0, 2, 3] = float("nan")                                  # no finite generated value in channel 0 and the speed
    acc = GridHist(spec, H, W, device="cpu")
    acc._buf[:-1] = torch.from_numpy(gridhist.host_table(spec, real.reshape(T, 2, -1).numpy(), fake.reshape(T, 2, -1).numpy())).reshape(-1)
    acc._buf[-1] = T
    m = QuantileMap.fit(acc)
    assert (m.H, m.W, m.fields) == (H, W, T) and m.spec == spec and m.nodes.shape == (3, 35, H * W) and m.nodes.dtype == torch.float32
    np.testing.assert_array_equal(R.bits(m.nodes.numpy()), R.bits(qmap.host_fit(acc.counts.numpy(), spec.lo, spec.width())))
    assert m.valid.dtype == torch.bool and m.valid.shape == (3, H, W)
    assert not m.valid[0, 2, 3] and not m.valid[2, 2, 3] and m.valid[1, 2, 3] and m.valid.sum() == 3 * H * W - 2
    edges, nodes = m.transfer()
    assert edges.shape == (3, 33) and nodes.shape == (3, 33, H, W) and nodes.dtype == np.float64
    np.testing.assert_array_equal(edges, spec.edges())
    np.testing.assert_array_equal(nodes[0, :, 2, 3], spec.edges()[0].astype(F32))         # the identity where a side is empty
    np.testing.assert_array_equal(nodes.reshape(3, 33, -1), m.nodes[:, :33].numpy())
    out = m.apply(fake)
    assert out.shape == (T, 3, H, W) and out.dtype == torch.float32
    nhwc = torch.zeros(T, H, W, 16, dtype=torch.bfloat16)
    nhwc[..., :2] = fake.permute(0, 2, 3, 1)
    seen = nhwc[..., :2].permute(0, 3, 1, 2).float()
    np.testing.assert_array_equal(R.bits(m.apply(nhwc, nhwc=True, channels=2).numpy()), R.bits(m.apply(seen).numpy()))
    keep = torch.full((T, 3, H, W), 7.0)
    part = m.apply(fake, n_valid=4, out=keep)
    assert part.shape == (4, 3, H, W) and torch.all(keep[4:] == 7.0)
    np.testing.assert_array_equal(R.bits(keep[:4].numpy()), R.bits(out[:4].numpy()))
    path = str(tmp_path / "map.npz")
    assert m.save(path) == path
    back = QuantileMap.load(path)
    assert back.spec == spec and back.spec.names == spec.names and np.array_equal(back.spec.inv_w, spec.inv_w)
    assert (back.H, back.W, back.fields) == (H, W, T) and torch.equal(back.valid, m.valid)
    np.testing.assert_array_equal(R.bits(back.nodes.numpy()), R.bits(m.nodes.numpy()))
    np.testing.assert_array_equal(R.bits(back.apply(fake).numpy()), R.bits(out.numpy()))
    plain = HistSpec(8, [-1.0], [1.0], speed=None)
    QuantileMap(plain, 1, 2, torch.zeros(1, 11, 2), torch.ones(1, 1, 2, dtype=torch.bool), 0).save(path)
    assert QuantileMap.load(path).spec == plain


def test_generate_without_a_map_is_unchanged_and_with_one_maps_each_chunk(monkeypatch):
    from oracle.emu_ops import EmuOps
    from downgan_amd import backend, synthetic
    from downgan_amd.networks.generator import Generator
    monkeypatch.setattr(backend, "make_ops", lambda dtype, device: EmuOps("f32"))
    torch.set_num_threads(4)
    coarse = torch.from_numpy(synthetic.tiles(3, 2, 16, seed=11)[0])
    G = Generator(16, 128, 2, 2, num_res_blocks=1)
    pad = torch.cat([coarse[2:], torch.zeros_like(coarse[:1])], 0)
    today = torch.cat([G.forward(coarse[:2]).cpu(), G.forward(pad)[:1].cpu()], 0)          # the chunk loop as it was, by hand
    got = G.generate(coarse, chunk_size=2)
    assert got.shape == (3, 2, 128, 128) and torch.equal(got.view(torch.int32), today.view(torch.int32))
    assert torch.equal(G.generate(coarse, 2, qmap=None).view(torch.int32), today.view(torch.int32))
    spec = HistSpec(64, [-6.0, -6.0], [6.0, 6.0], speed=None)
    real = today * 1.5 + 0.25
    table = gridhist.host_table(spec, real.reshape(3, 2, -1).numpy(), today.reshape(3, 2, -1).numpy())
    m = QuantileMap.fit(GridHistMaps(spec, 128, 128, True, torch.from_numpy(table), 3))
    mapped = G.generate(coarse, chunk_size=2, qmap=m)
    assert torch.equal(mapped.view(torch.int32), m.apply(today).view(torch.int32)) and not torch.equal(mapped, today)
