"""Distance maps without a GPU: the library's host reference (dg_distmap_host) against a numpy restatement of the definition
written here (a brute-force minimum over all set pixels, math.isqrt for dq and ring: not the library's algorithm) over the mask
zoo and the random fields of test_objects_cpu; the squared distances against scipy's distance_transform_edt where scipy imports;
known answers; ring and dq next to every square; spec validation, the ABI surface and the struct layout; the limits against
their closed forms; ``Distances`` on the explicit host path and its exact reduction over 2 gloo ranks.  Every comparison of
integers is exact equality; the only tolerance is 1e-12 on float64 results that hold a sqrt or a division."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from downgan_amd import _lib, distmap
from downgan_amd.distmap import Distances, DistSpec, HostOps, host_distmap, host_scalars

from .test_objects_cpu import np_values, zoo, zoo_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FAR = 1 << 30
GRIDS = [(1, 1), (1, 70), (70, 1), (5, 67), (33, 65)]


# ------------------------------------------------------------------------------------------------- the numpy restatement
def np_ring(d2):
    r = math.isqrt(d2)
    return r if r * r == d2 else r + 1


def np_dq(d2):
    return math.isqrt(d2 << 20)


def np_d2(mask):
    """int64 [H, W]: the squared distance to the nearest set pixel, the minimum over ALL set pixels (FAR for an empty mask)."""
    H, W = mask.shape
    hs, ws = np.nonzero(mask)
    if len(hs) == 0:
        return np.full((H, W), FAR, np.int64)
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.full((H, W), FAR, np.int64)
    for s in range(0, len(hs), 512):                                 # in slabs of set pixels: [H, W, 512] at most
        d = (hh[..., None] - hs[s:s + 512]) ** 2 + (ww[..., None] - ws[s:s + 512]) ** 2
        out = np.minimum(out, d.min(-1))
    return out


def np_masks(spec, x):
    """bool [nout, K, H, W] of one field x float32 [C, H, W]."""
    y = np_values(spec, x)
    with np.errstate(invalid="ignore"):
        return np.stack([np.stack([y[j] > F32(spec.thresholds[j, k]) for k in range(spec.K)]) for j in range(spec.nout)])


def np_distmap(spec, a, b):
    """(records int64 [nout, K, 11], rings int64 [nout, K, 2, nring + 2], d2 int32 [2, nout, K, H, W]) of one field pair."""
    m = np.stack([np_masks(spec, a), np_masks(spec, b)])
    _, nout, K, H, W = m.shape
    nb, cap = spec.nring + 2, spec.cutoff * 1024
    d2 = np.zeros((2, nout, K, H, W), np.int64)
    rec, rings = np.zeros((nout, K, 11), np.int64), np.zeros((nout, K, 2, nb), np.int64)
    for j in range(nout):
        for k in range(K):
            A, B = m[0, j, k], m[1, j, k]
            dA, dB = np_d2(A), np_d2(B)
            d2[0, j, k], d2[1, j, k] = dA, dB
            w = [np.array([cap if d == FAR else min(np_dq(int(d)), cap) for d in dd.reshape(-1)], dtype=object) for dd in (dA, dB)]
            diff = abs(w[0] - w[1])
            r = [int(A.sum()), int(B.sum()), int((A & B).sum())] + [-1] * 6 + [int(diff.sum()), int((diff * diff).sum())]
            both = r[0] > 0 and r[1] > 0
            for direction, (pix, dist, other) in enumerate(((B, dA, r[0]), (A, dB, r[1]))):
                d = [int(v) for v in dist[pix]]
                if both:
                    r[3 + 3 * direction:6 + 3 * direction] = [sum(np_dq(v) for v in d), sum(d), max(d)]
                for v in d:
                    rings[j, k, direction, min(np_ring(v), spec.nring) if other > 0 else spec.nring + 1] += 1
            rec[j, k] = r
    return rec, rings, d2.astype(np.int32)


def spec3(**kw):
    """3 output channels (2 + speed), 2 thresholds; a cutoff and a ring count small enough for every grid to pass them."""
    return DistSpec(2, speed=(0, 1), thresholds=(1.0, 2.0), **dict(dict(cutoff=6, nring=9), **kw))


def batch_fields(H, W):
    """The zoo and the random fields of test_objects_cpu, then two fields without any exceedance: paired with the next field, the
    batch then holds pairs of every kind (both, real only, generated only, neither) on every grid."""
    blank = np.full((2, H, W), -3.0, F32)
    return zoo_fields(H, W) + [("blank0", blank), ("blank1", blank.copy())]


def same(got, want, msg):
    for g, w, what in zip(got, want, ("records", "rings", "d2")):
        assert g.dtype == w.dtype and g.shape == w.shape, (msg, what, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (msg, what, np.argwhere(g != w)[:4], g[g != w][:4], w[g != w][:4])


# ------------------------------------------------------------------------------------------------- host reference == numpy
@pytest.mark.parametrize("grid", GRIDS)
def test_host_reference_equals_the_numpy_restatement(grid):
    H, W = grid
    spec = spec3()
    fields = batch_fields(H, W)
    kinds = set()
    for (name, a), (_, b) in zip(fields, fields[1:] + fields[:1]):
        got = host_distmap(spec, a, b)
        same(got, np_distmap(spec, a, b), f"{grid} {name}")
        one = host_distmap(spec, a)                                   # one series: the transform alone
        assert one.dtype == np.int32 and one.tobytes() == got[2][0].tobytes(), name
        kinds |= {(int(r[0] > 0), int(r[1] > 0)) for r in got[0].reshape(-1, 11)}
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("grid", GRIDS)
def test_squared_distances_equal_scipy(grid):
    ndimage = pytest.importorskip("scipy.ndimage")
    H, W = grid
    rng = np.random.default_rng(7 + 1000 * H + W)
    spec = DistSpec(1, speed=None, thresholds=(1.0,))
    masks = [rng.random((H, W)) < d for d in (0.01, 0.1, 0.3, 0.6, 0.95)] + [m for m in zoo(H, W).values()]
    for m in masks:
        d2 = host_distmap(spec, np.where(m, 2.0, 0.0).astype(F32)[None])[0, 0]
        if not m.any():
            assert (d2 == FAR).all()
            continue
        want = np.rint(ndimage.distance_transform_edt(~m) ** 2).astype(np.int32)
        assert np.array_equal(d2, want) and np.array_equal(d2, np_d2(m))


# ------------------------------------------------------------------------------------------------- known answers
SPEC1 = DistSpec(1, speed=None, thresholds=(1.0,), cutoff=8, nring=16)


def dot(H, W, *pixels):
    x = np.zeros((1, H, W), F32)
    for h, w in pixels:
        x[0, h, w] = 2.0
    return x


def test_one_pixel_and_a_shifted_copy():
    H, W = 19, 23
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for h0, w0 in ((0, 0), (H - 1, W - 1), (7, 11), (0, W - 1)):
        d2 = host_distmap(SPEC1, dot(H, W, (h0, w0)))[0, 0]
        assert np.array_equal(d2, (hh - h0) ** 2 + (ww - w0) ** 2)
    rec, rings, d2 = host_distmap(SPEC1, dot(H, W, (5, 6)), dot(H, W, (8, 10)))       # moved by (3, 4)
    assert rec[0, 0, :9].tolist() == [1, 1, 0, 5120, 25, 25, 5120, 25, 25]
    want = np.zeros((2, 18), np.int64)
    want[:, 5] = 1
    assert np.array_equal(rings[0, 0], want)
    cap = 8 * 1024
    wa, wb = ([min(np_dq(int(v)), cap) for v in d.reshape(-1)] for d in (d2[0, 0, 0], d2[1, 0, 0]))
    assert rec[0, 0, 9] == sum(abs(x - y) for x, y in zip(wa, wb)) and rec[0, 0, 10] == sum((x - y) ** 2 for x, y in zip(wa, wb))


def test_identical_empty_and_full_fields():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(2, 17, 29)).astype(F32) * 1.5
    spec = spec3()
    rec, rings, d2 = host_distmap(spec, x, x.copy())
    assert not rec[..., 3:].any() and (rec[..., 0] == rec[..., 1]).all() and (rec[..., 0] == rec[..., 2]).all() and rec[..., 0].min() > 0
    assert np.array_equal(rings[..., 0], np.stack([rec[..., 0]] * 2, -1)) and not rings[..., 1:].any()      # every pixel in ring bin 0
    assert d2[0].tobytes() == d2[1].tobytes()
    H, W = 6, 11
    one, none, full = dot(H, W, (2, 3)), dot(H, W), np.full((1, H, W), 2.0, F32)
    rec, rings, d2 = host_distmap(SPEC1, one, none)                   # A one pixel, B empty
    cap = 8 * 1024
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    gap = [min(np_dq(int(v)), cap) - cap for v in ((hh - 2) ** 2 + (ww - 3) ** 2).reshape(-1)]
    assert rec[0, 0].tolist() == [1, 0, 0, -1, -1, -1, -1, -1, -1, -sum(gap), sum(g * g for g in gap)]
    assert rings[0, 0, 1, 17] == 1 and rings.sum() == 1 and (d2[1] == FAR).all()
    rec, rings, _ = host_distmap(SPEC1, none, one)                    # the other way round
    assert rec[0, 0].tolist() == [0, 1, 0, -1, -1, -1, -1, -1, -1, -sum(gap), sum(g * g for g in gap)]
    assert rings[0, 0, 0, 17] == 1 and rings.sum() == 1
    rec, rings, d2 = host_distmap(SPEC1, none, none)
    assert rec[0, 0].tolist() == [0, 0, 0, -1, -1, -1, -1, -1, -1, 0, 0] and not rings.any() and (d2 == FAR).all()
    rec, rings, d2 = host_distmap(SPEC1, full, one)
    assert not d2[0].any() and rec[0, 0, :6].tolist() == [H * W, 1, 1, 0, 0, 0] and rec[0, 0, 8] == 3 * 3 + 7 * 7
    assert rings[0, 0, 0, 0] == 1 and rings[0, 0, 1, :9].sum() == H * W and rings[0, 0, 1, 0] == 1 and rings[0, 0, 1, 8] >= 1


def test_rings_accumulate_and_the_far_bin():
    """The library adds to the ring table; a ring at or past nring lands in bin nring."""
    spec = DistSpec(1, speed=None, thresholds=(1.0,), cutoff=2, nring=3)
    a, b = dot(1, 9, (0, 0)), dot(1, 9, (0, 2), (0, 3), (0, 8))
    s = spec.struct()
    rings = np.full((1, 1, 2, 5), 100, np.int64)
    rc = _lib.lib().dg_distmap_host(C.byref(s), a.ctypes.data, b.ctypes.data, 1, 1, 9, None, rings.ctypes.data, None)
    assert rc == 0 and (rings - 100)[0, 0].tolist() == [[0, 0, 1, 2, 0], [0, 0, 1, 0, 0]]      # rings 2, 3 (= nring), 8; ring 2


def test_special_values():
    """NaN is in no mask, +inf is, -inf is not; equality with the threshold is outside."""
    a = np.array([[[np.nan, np.inf, -np.inf, 1.0, np.nextafter(F32(1), F32(2)), 0.0, np.nan]]], F32)
    d2 = host_distmap(SPEC1, a)[0, 0, 0]
    assert d2.tolist() == [1, 0, 1, 1, 0, 1, 4]
    allnan = np.full((1, 3, 4), np.nan, F32)
    rec, rings, d2 = host_distmap(SPEC1, allnan, allnan)
    assert (d2 == FAR).all() and rec[0, 0].tolist() == [0, 0, 0, -1, -1, -1, -1, -1, -1, 0, 0] and not rings.any()


def test_ring_and_dq_next_to_every_square():
    for n in range(1, 2896):
        for d2 in (n * n - 1, n * n, n * n + 1):
            ring, dq, w = host_scalars(d2, 512)
            assert (ring, dq, w) == (np_ring(d2), np_dq(d2), min(np_dq(d2), 512 * 1024)), d2
    assert host_scalars(25, 512) == (5, 5120, 5120) and host_scalars(0, 1) == (0, 0, 0)
    assert host_scalars(FAR, 7) == (1 << 15, 1 << 25, 7 * 1024) and host_scalars(FAR - 1, 512)[:2] == (1 << 15, np_dq(FAR - 1))
    lib = _lib.lib()
    p = C.c_void_p(0x1000)
    for d2, cutoff in ((-1, 1), (FAR + 1, 1), (0, 0), (0, 513)):
        assert lib.dg_distmap_host_scalars(d2, cutoff, p, p, p) == -3
    assert lib.dg_distmap_host_scalars(1, 1, None, p, p) == -3


def test_speed_channel_and_affine_transform():
    rng = np.random.default_rng(4)
    spec = DistSpec(3, scale=[2.0, 0.5, 1.5], offset=[0.1, -0.2, 0.3], speed=(2, 0), thresholds=[[0.5], [0.0], [1.0], [2.5]],
                    cutoff=5, nring=7)
    a, b = rng.normal(size=(2, 3, 17, 23)).astype(F32)
    got = host_distmap(spec, a, b)
    same(got, np_distmap(spec, a, b), "affine + speed")
    assert got[0][..., :3].min() > 0


# ------------------------------------------------------------------------------------------------- spec, ABI, limits
def test_spec_validation():
    ok = dict(C=2, thresholds=(1.0, 2.0))
    good = DistSpec(**ok)
    assert (good.nout, good.K, good.cutoff, good.nring, good.names) == (3, 2, 32, 64, ["ch0", "ch1", "speed"])
    assert good == DistSpec(**ok) and good != DistSpec(cutoff=16, **ok) and good != DistSpec(nring=32, **ok)
    for kw, msg in ((dict(C=0), "input channels"), (dict(C=9), "input channels"), (dict(speed=(0, 2)), "speed channels"),
                    (dict(thresholds=()), "1 to 4 thresholds"), (dict(thresholds=(1, 2, 3, 4, 5)), "1 to 4 thresholds"),
                    (dict(thresholds=[[1.0], [2.0]]), "one list per output channel"), (dict(thresholds=(np.nan,)), "finite"),
                    (dict(scale=[1.0]), "one value per input channel"), (dict(scale=[np.inf, 1.0]), "finite"),
                    (dict(offset=[0.0, np.nan]), "finite"), (dict(cutoff=0), "cutoff"), (dict(cutoff=513), "cutoff"),
                    (dict(cutoff=2.5), "cutoff"), (dict(nring=0), "nring"), (dict(nring=129), "nring"), (dict(nring=1.0), "nring"),
                    (dict(names=["a"]), "names")):
        with pytest.raises(ValueError, match=msg):
            DistSpec(**dict(ok, **kw))
    z = DistSpec.zscore(1)
    assert z.speed is None and z.nout == 1 and z.thresholds.tolist() == [[1.0, 2.0]]
    p = DistSpec.physical({"u10": (1.0, 2.0), "v10": (-1.0, 3.0), "t2m": (280.0, 10.0)}, ["u10", "v10", "t2m"],
                          thresholds=[[5.0], [5.0], [290.0], [8.0]], cutoff=12)
    assert p.names == ["u10", "v10", "t2m", "speed"] and p.speed == (0, 1) and p.scale.tolist() == [2.0, 3.0, 10.0]
    s = p.struct()
    assert (s.speed_u, s.speed_v, s.nthr, s.nring, s.cutoff) == (0, 1, 1, 64, 12) and s.thr[3][0] == 8.0 and s.offset[2] == 280.0
    with pytest.raises(TypeError, match="DistSpec"):
        Distances("spec", 4, 4, ops=HostOps())
    with pytest.raises(ValueError, match="grid"):
        Distances(good, 4, 2049, ops=HostOps())
    acc = Distances(good, 4, 4, ops=HostOps())
    x = torch.zeros(2, 2, 4, 4)
    with pytest.raises(ValueError, match="4 x 4 grid"):
        acc.add(torch.zeros(2, 2, 4, 5), torch.zeros(2, 2, 4, 5))
    with pytest.raises(ValueError, match="differ in length"):
        acc.add(x, x[:1])
    with pytest.raises(ValueError, match="n_valid"):
        acc.add(x, x, n_valid=3)
    with pytest.raises(ValueError, match="input channels"):
        acc.add(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError, match="direction"):
        acc.result().ring_cdf(2)
    with pytest.raises(TypeError, match="DistSpec"):
        distmap.distance_transform(x, spec="spec", ops=HostOps())


def test_header_declares_and_library_exports_the_distmap_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert "Distance maps (csrc/distmap.hip)" in src
    for name, v in (("MAX_SIDE", "2048"), ("MAX_THR", "4"), ("MAX_RINGS", "128"), ("MAX_CUTOFF", "512"), ("COLS", "11"),
                    ("FAR", r"\(1 << 30\)")):
        assert re.search(rf"#define DG_DIST_{name} {v}(\s|$)", src), name
    assert (_lib.DIST_MAX_SIDE, _lib.DIST_MAX_THR, _lib.DIST_MAX_RINGS, _lib.DIST_MAX_CUTOFF, _lib.DIST_COLS, _lib.DIST_FAR) == \
        (distmap.SIDE_MAX, distmap.THR_MAX, distmap.RINGS_MAX, distmap.CUTOFF_MAX, distmap.COLS, distmap.FAR) == (2048, 4, 128, 512, 11, FAR)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"const dg_eof_fields*": C.POINTER(_lib.EofFields), "const dg_distmap_spec*": C.POINTER(_lib.DistmapSpec), "int": C.c_int,
             "int32_t": C.c_int32}
    for sym in ("dg_distmap_ws_bytes", "dg_distmap", "dg_distmap_host", "dg_distmap_host_scalars"):
        m = re.search(rf"\b(size_t|int) {sym}\s*\(([^)]*)\)", code)
        assert m, sym
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
        args = [" ".join(a.split()[:-1]) for a in m.group(2).replace("\n", " ").split(",")]
        assert _lib._PROTOS[sym] == [ctype.get(a, C.c_void_p) for a in args], (sym, args)
    assert _lib._RESTYPES["dg_distmap_ws_bytes"] is C.c_size_t
    assert "distmap.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()


def test_distmap_spec_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.DistmapSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(dg_distmap_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_distmap_spec, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("thr_row %zu\\n", sizeof(((dg_distmap_spec*)0)->thr[0]));', '  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert int(got["thr_row"]) == 4 * _lib.DIST_MAX_THR


def test_abi_rejects_bad_arguments_without_launching():
    """Every pointer is a made-up address: a call that passed the checks would fault instead of returning a status."""
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))

    def spec(**kw):
        s = DistSpec.zscore(2).struct()
        for k, v in kw.items():
            if k == "thr":
                s.thr[v[0]][v[1]] = v[2]
            elif k in ("scale", "offset"):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    good, p = spec(), C.c_void_p(0x2000)
    names = ("a", "b", "H", "W", "s", "ws", "records", "rings", "d2", "stream")
    base = dict(a=f(), b=f(), H=10, W=10, s=good, ws=p, records=p, rings=p, d2=p, stream=None)
    call = lambda **kw: lib.dg_distmap(*[dict(base, **kw)[k] for k in names])
    bad = [dict(a=None), dict(s=None), dict(ws=None), dict(records=None, rings=None, d2=None),          # nothing to compute
           dict(b=None), dict(b=None, records=None), dict(b=None, rings=None), dict(b=None, records=None, rings=None, d2=None),
           dict(b=f(T=3)), dict(b=f(C=1)), dict(b=f(P=99)), dict(H=10, W=11), dict(a=f(P=2049), b=f(P=2049), H=1, W=2049),
           dict(a=f(P=2049), b=f(P=2049), H=2049, W=1), dict(H=0, W=10), dict(s=spec(nthr=0)), dict(s=spec(nthr=5)),
           dict(s=spec(nring=0)), dict(s=spec(nring=129)), dict(s=spec(cutoff=0)), dict(s=spec(cutoff=513)),
           dict(s=spec(thr=(2, 1, math.nan))), dict(s=spec(thr=(0, 0, math.inf))), dict(s=spec(scale=(1, math.inf))),
           dict(s=spec(offset=(0, math.nan))), dict(s=spec(speed_u=2)), dict(s=spec(speed_v=-1)), dict(a=f(base=0)),
           dict(a=f(C=9), b=f(C=9)), dict(b=f(base=0))]
    for kw in bad:
        assert call(**kw) == -3, kw
    assert call(a=f(dtype=7)) == -2 and call(b=f(dtype=7)) == -2
    assert lib.dg_distmap_ws_bytes(f(), 10, 10, good) == 2 * 4 * 2 * 3 * 2 * 100          # two bytes per plane pixel, nothing else
    for args in ((f(), 10, 11, good), (None, 10, 10, good), (f(), 10, 10, None), (f(), 10, 10, spec(nring=0)),
                 (f(), 10, 10, spec(cutoff=600)), (f(), 10, 10, spec(nthr=5)), (f(P=2049), 1, 2049, good),
                 (f(), 10, 10, spec(thr=(1, 0, math.nan))), (f(), 10, 10, spec(speed_u=5))):
        assert lib.dg_distmap_ws_bytes(*args) == 0
    assert lib.dg_distmap_ws_bytes(f(T=1, P=2048 * 2048), 2048, 2048, good) == 2 * 2 * 3 * 2 * 2048 * 2048
    hn = ("s", "a", "b", "C", "H", "W", "records", "rings", "d2")
    hd = dict(s=good, a=p, b=p, C=2, H=4, W=4, records=p, rings=p, d2=p)
    host = lambda **kw: lib.dg_distmap_host(*[dict(hd, **kw)[k] for k in hn])
    for kw in (dict(s=None), dict(a=None), dict(C=0), dict(C=9), dict(C=1), dict(H=0), dict(W=2049), dict(records=None, rings=None, d2=None),
               dict(b=None), dict(b=None, records=None), dict(b=None, records=None, rings=None, d2=None), dict(s=spec(nring=200)),
               dict(s=spec(cutoff=0)), dict(s=spec(nthr=0)), dict(s=spec(thr=(0, 1, math.inf))), dict(s=spec(scale=(0, math.nan)))):
        assert host(**kw) == -3, kw


def test_limits_against_the_closed_forms():
    """The side limit, the largest cutoff and ring count.  One pixel at either end of a 2048-pixel line: the largest distance a
    side admits.  A side that is empty against one that is full gives every pixel the largest |w_A - w_B| = 512 * 1024: the
    bound of bad2 per pixel; times the 2^22 pixels of the largest grid it stays below 2^63, as do the other sums."""
    N, c = 2048, 512
    spec = DistSpec(1, speed=None, thresholds=(1.0,), cutoff=c, nring=128)
    for shape, far in (((1, N), (0, N - 1)), ((N, 1), (N - 1, 0))):
        a, b = dot(*shape, (0, 0)), dot(*shape, far)
        rec, rings, d2 = host_distmap(spec, a, b)
        line = np.arange(N, dtype=np.int64) ** 2
        assert np.array_equal(d2[0, 0, 0].reshape(-1), line) and np.array_equal(d2[1, 0, 0].reshape(-1), line[::-1])
        assert rec[0, 0, :9].tolist() == [1, 1, 0, 2047 * 1024, 2047 ** 2, 2047 ** 2, 2047 * 1024, 2047 ** 2, 2047 ** 2]
        w = np.minimum(np.arange(N) * 1024, c * 1024)
        diff = np.abs(w - w[::-1])
        assert rec[0, 0, 9] == diff.sum() and rec[0, 0, 10] == (diff * diff).sum()
        assert rings[0, 0, :, 128].tolist() == [1, 1] and rings.sum() == 2
        full = np.full((1,) + shape, 2.0, F32)
        rec, rings, _ = host_distmap(spec, dot(*shape), full)
        assert rec[0, 0].tolist() == [0, N, 0, -1, -1, -1, -1, -1, -1, N * c * 1024, N * (c * 1024) ** 2]
        assert rings[0, 0, 0, 129] == N and rings.sum() == N
    assert (c * 1024) ** 2 == 1 << 38 and (N * N) * (c * 1024) ** 2 == 1 << 60                      # bad2 of the largest grid
    assert (N * N) * np_dq(2 * (N - 1) ** 2) < 1 << 45 and (N * N) * 2 * (N - 1) ** 2 < 1 << 45       # sum_dq, sum_d2
    assert 2 * (N - 1) ** 2 < FAR and FAR + (N - 1) ** 2 < 1 << 31                                   # d2 and the scan's candidates in int32
    assert host_scalars(2 * (N - 1) ** 2, c)[1] == np_dq(2 * (N - 1) ** 2) < 1 << 22


# ------------------------------------------------------------------------------------------------- the accumulator
def run(a, b, spec, **kw):
    return distmap.distances(a, b, spec=spec, ops=HostOps(), **kw)


def test_distance_result_of_the_known_answers():
    H, W = 19, 23
    t = lambda *x: torch.from_numpy(np.stack(x))
    one, moved, none = dot(H, W, (5, 6)), dot(H, W, (8, 10)), dot(H, W)
    res = run(t(one, one, none, none, one), t(moved, none, moved, none, one), SPEC1, keep_records=True)
    assert {k: int(v[0, 0]) for k, v in res.pairs().items()} == {"both": 2, "real_only": 1, "fake_only": 1, "neither": 1}
    assert res.fields == 5 and res.records.shape == (5, 1, 1, 11) and res.records[0, 0, 0, :9].tolist() == [1, 1, 0, 5120, 25, 25, 5120, 25, 25]
    # the pairs of kind "both": one moved by 5 px, one identical: 5120 / 2 pixels / 1024
    assert res.med_fake_to_real()[0, 0] == 2.5 and res.med_real_to_fake()[0, 0] == 2.5 and res.med()[0, 0] == 2.5
    h = res.hausdorff()
    assert h["mean"][0, 0] == 2.5 and h["max"][0, 0] == 5.0
    assert res.rings()[0, 0].tolist() == [[1] + [0] * 4 + [1] + [0] * 11 + [1]] * 2
    assert res.ring_cdf("fake_to_real")[0, 0].tolist() == [0.5] * 5 + [1.0] * 11 and res.ring_cdf(1)[0, 0, 4] == 0.5
    assert res.displacement_quantile(0.5, 0) == [[0]] and res.displacement_quantile(0.9, "real_to_fake") == [[5]]
    bad1 = sum(int(r[9]) for r in res.records[:, 0, 0])
    bad2 = sum(int(r[10]) for r in res.records[:, 0, 0])
    assert abs(res.baddeley1()[0, 0] - bad1 / (5 * H * W) / 1024) <= 1e-12
    assert abs(res.baddeley2()[0, 0] - math.sqrt(bad2 / (5 * H * W)) / 1024) <= 1e-12 and res.baddeley2()[0, 0] > res.baddeley1()[0, 0] > 0
    s = res.summary()
    assert json.loads(json.dumps(s, allow_nan=False)) == s and s["pairs"] == {"both": [[2]], "real_only": [[1]], "fake_only": [[1]], "neither": [[1]]}
    assert isinstance(s["sums"]["bad2"][0][0], int) and s["sums"]["bad2"] == [[bad2]] and s["med"] == [[2.5]]
    with tempfile.TemporaryDirectory() as d:
        assert set(res.save(d)) == {"rings.npy", "ring_cdf_fake_to_real.npy", "ring_cdf_real_to_fake.npy", "summary.json"}
        assert json.load(open(os.path.join(d, "summary.json"))) == s and np.array_equal(np.load(os.path.join(d, "rings.npy")), res.rings())
    empty = run(t(none), t(none), SPEC1)
    assert np.isnan(empty.med()[0, 0]) and np.isnan(empty.hausdorff()["max"][0, 0]) and empty.baddeley2()[0, 0] == 0
    assert empty.summary()["med"] == [[None]] and empty.displacement_quantile(0.5, 0) == [[None]]
    far = DistSpec(1, speed=None, thresholds=(1.0,), cutoff=8, nring=3)
    assert run(t(one), t(moved), far).displacement_quantile(0.5, 0) == [[None]]       # ring 5 is past nring


def test_one_call_equals_field_by_field():
    rng = np.random.default_rng(9)
    a, b = (rng.normal(size=(4, 2, 19, 27)).astype(F32) * 1.2 for _ in range(2))
    b[3] = -5.0
    spec = spec3()
    whole = run(torch.from_numpy(a), torch.from_numpy(b), spec, keep_records=True)
    acc = Distances(spec, 19, 27, ops=HostOps(), keep_records=True)
    for t in range(4):
        acc.add(torch.from_numpy(a[t:t + 1]), torch.from_numpy(b[t:t + 1]))
    byfield = acc.result()
    assert whole.summary() == byfield.summary() and np.array_equal(whole.records, byfield.records) and acc.calls == 4
    for t in range(4):
        rec, _, _ = np_distmap(spec, a[t], b[t])
        assert np.array_equal(whole.records[t], rec)
    # field 3 has no generated exceedance in the components (its speed, 5 sqrt(2), exceeds everything)
    assert whole.pairs()["real_only"][:2].min() >= 1 and whole.pairs()["both"][:2].max() == 3 and whole.pairs()["both"][2].min() == 4
    # a workspace cap that cuts the batch; NHWC with padding == NCHW; n_valid
    cut = Distances(spec, 19, 27, ops=HostOps())
    cut.ws_cap = 2 * HostOps().distmap_ws_bytes(HostOps().eof_fields(torch.from_numpy(a[:1])), 19, 27, spec.struct())
    assert cut.add(torch.from_numpy(a), torch.from_numpy(b)).result().summary() == whole.summary() and cut.calls == 2
    pad = torch.full((4, 19, 27, 5), 9.0)
    pad[..., :2] = torch.from_numpy(a).permute(0, 2, 3, 1)
    nhwc = run(pad, torch.from_numpy(b), spec, nhwc=(True, False), channels=2, n_valid=3)
    first = run(torch.from_numpy(a[:3]), torch.from_numpy(b[:3]), spec)
    assert nhwc.summary() == first.summary() and nhwc.fields == 3
    d2 = distmap.distance_transform(torch.from_numpy(a), spec=spec, ops=HostOps())
    assert d2.dtype == torch.int32 and tuple(d2.shape) == (4, 3, 2, 19, 27)
    assert np.array_equal(d2[2].numpy(), host_distmap(spec, a[2]))


# ------------------------------------------------------------------------------------------------- reduce_
BIG = 1 << 60


def _rank_acc(rank, world):
    """The accumulator of one rank: real records of its share of the fields, then planted ones whose bad2 totals pass 2^63."""
    rng = np.random.default_rng(17)
    a, b = (rng.normal(size=(6, 2, 16, 16)).astype(F32) * 1.2 for _ in range(2))
    b[4:] = -5.0
    acc = Distances(spec3(), 16, 16, ops=HostOps())
    acc.add(torch.from_numpy(a[rank::world].copy()), torch.from_numpy(b[rank::world].copy()))
    planted = np.zeros((5, 3, 2, 11), np.int64)
    planted[..., 3:9] = -1
    planted[..., 9], planted[..., 10] = 1 << 30, BIG                # 16 * 16 pixels at the largest |w_A - w_B| would give less: planted
    planted[rank, 1, 1, :9] = [3, 2, 1, 7000 + rank, 90, 49 + 15 * rank, 8000, 100, 64]
    acc._pool(planted)
    acc.fields += 5
    return acc


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    res = _rank_acc(rank, world).reduce_(d).result()
    torch.save({"summary": res.summary(), "hsum": res._hsum, "hmax": res._hmax}, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_pool():
    one = _rank_acc(0, 1)                                            # all six fields, then both ranks' planted records
    planted = np.zeros((5, 3, 2, 11), np.int64)
    planted[..., 3:9] = -1
    planted[..., 9], planted[..., 10] = 1 << 30, BIG
    planted[1, 1, 1, :9] = [3, 2, 1, 7001, 90, 64, 8000, 100, 64]
    one._pool(planted)
    one.fields += 5
    ref = one.result()
    assert ref._s["bad2"][0][0] >= 10 * BIG > 1 << 63 and ref.fields == 16
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["summary"] == r1["summary"]
    want = ref.summary()
    floats = ("hausdorff",)
    assert {k: v for k, v in r0["summary"].items() if k not in floats} == {k: v for k, v in want.items() if k not in floats}
    assert np.array_equal(r0["hmax"], ref._hmax) and ref._hmax[1, 1] >= 64
    np.testing.assert_allclose(r0["hsum"], ref._hsum, rtol=1e-12, atol=1e-12)      # a float sum in another order
    assert r0["summary"]["sums"]["bad2"][0][0] == ref._s["bad2"][0][0]


# ------------------------------------------------------------------------------------------------- the trainer's defaults
def test_the_hook_is_off_by_default():
    import inspect
    from downgan_amd.engine import TrainEngine
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_distances is False and WassersteinGAN.distance_spec is None and WassersteinGAN.distance_results is None
    assert inspect.signature(WassersteinGAN.gen_batch_and_log_metrics).parameters["distances"].default is None
    assert inspect.signature(TrainEngine.metrics_pass).parameters["distances"].default is None
