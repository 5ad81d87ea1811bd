"""Exceedance objects without a GPU: the library's host reference (dg_objects_host, a flood fill) against a numpy restatement of
the definition written here (labels by repeated neighbour minima, records by bincount: not the library's algorithm) over a zoo of
patterns, random masks near the percolation density and special values, at both connectivities; the partition against
scipy.ndimage.label where scipy imports; the capacity contract; spec validation, the ABI surface and the struct layout; the known
answers of SAL and of the per-object scores through ``Objects`` on the explicit host path; the exact reduction over 2 gloo ranks.
Every comparison of tables is exact equality; the only tolerance is 1e-12 on the float64 SAL known answers."""
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

from downgan_amd import _lib, objects
from downgan_amd.objects import HostOps, Objects, ObjectSpec, host_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
TOP = (1 << 24) - 1


# ------------------------------------------------------------------------------------------------- the numpy restatement
def np_values(spec, x):
    """float32 [nout, H, W]: the output values of x float32 [C, H, W], every operation rounded to fp32 once."""
    y = [x[c].astype(F32) * F32(spec.scale[c]) + F32(spec.offset[c]) for c in range(spec.C)]
    if spec.speed is not None:
        u, v = y[spec.speed[0]], y[spec.speed[1]]
        with np.errstate(over="ignore", invalid="ignore"):
            y.append(np.sqrt(u * u + v * v))
    return np.stack(y)


def np_q(spec, y):
    with np.errstate(over="ignore", invalid="ignore"):
        t = y.astype(F32) * F32(spec.inv_quantum)
        return np.where(t >= F32(16777215.0), TOP, np.where(t > 0, np.rint(t), 0)).astype(np.int64)


def np_labels(mask, conn):
    """int64 [H, W]: the smallest linear index of every pixel's component (-1 where clear), by repeated neighbour minima."""
    H, W = mask.shape
    big = H * W
    lab = np.where(mask, np.arange(H * W).reshape(H, W), big)
    shifts = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if conn == 8 else [])
    while True:
        pad = np.full((H + 2, W + 2), big)
        pad[1:-1, 1:-1] = lab
        new = lab
        for dh, dw in shifts:
            new = np.minimum(new, pad[1 + dh:1 + dh + H, 1 + dw:1 + dw + W])
        new = np.where(mask, new, big)
        if np.array_equal(new, lab):
            return np.where(mask, lab, -1)
        lab = new


def np_objects(spec, a, b=None):
    """(table int64 [n, 12] sorted by (plane, root), per_plane int64 [2, nout, K]) of one field or field pair."""
    x = [a] + ([b] if b is not None else [])
    y = [np_values(spec, v) for v in x]
    _, H, W = a.shape
    hh, ww = np.divmod(np.arange(H * W), W)
    rows, per_plane = [], np.zeros((2, spec.nout, spec.K), np.int64)
    for side in range(len(x)):
        for j in range(spec.nout):
            q = np_q(spec, y[side][j]).reshape(-1)
            for k in range(spec.K):
                thr = F32(spec.thresholds[j, k])
                with np.errstate(invalid="ignore"):
                    mask = y[side][j] > thr
                    other = (y[1 - side][j] > thr).reshape(-1) if b is not None else np.zeros(H * W, bool)
                lab = np_labels(mask, spec.connectivity).reshape(-1)
                plane = (side * spec.nout + j) * spec.K + k
                for root in np.unique(lab[lab >= 0]):
                    m = lab == root
                    rows.append([plane, root, m.sum(), (m & other).sum(), q[m].sum(), (q[m] * hh[m]).sum(), (q[m] * ww[m]).sum(),
                                 q[m].max(), hh[m].min(), hh[m].max(), ww[m].min(), ww[m].max()])
                    per_plane[side, j, k] += 1
    return np.array(rows, np.int64).reshape(-1, 12), per_plane


# ------------------------------------------------------------------------------------------------- the zoo
def spiral(H, W):
    m = np.zeros((H, W), bool)
    t, b, l, r, first = 0, H - 1, 0, W - 1, True
    while t <= b and l <= r:
        m[t, (l if first else max(0, l - 2)):r + 1] = True           # top, joined to the end of the previous turn
        m[t:b + 1, r] = True
        if b - t >= 2:
            m[b, l:r + 1] = True
            m[t + 2:b + 1, l] = True
        t, b, l, r, first = t + 2, b - 2, l + 2, r - 2, False
    return m


def zoo(H, W):
    """{name: bool [H, W]}: the patterns of the issue, defined for every grid (degenerate ones included)."""
    hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = {"empty": np.zeros((H, W), bool), "full": np.ones((H, W), bool)}
    c = np.zeros((H, W), bool)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = True
    z["corners"] = c
    z["diagonal"] = hh == ww                                         # one object at 8, min(H, W) objects at 4
    z["antidiagonal"] = hh + ww == W - 1                             # the NE neighbour
    z["checkerboard"] = (hh + ww) % 2 == 0
    z["rings"] = np.minimum(np.minimum(hh, H - 1 - hh), np.minimum(ww, W - 1 - ww)) % 2 == 0
    z["spiral"] = spiral(H, W)
    s = hh % 2 == 0                                                  # rows joined alternately at the right and the left end
    s |= (hh % 4 == 1) & (ww == W - 1)
    s |= (hh % 4 == 3) & (ww == 0)
    z["serpentine"] = s
    z["comb"] = (ww % 2 == 0) | (hh == H - 1)                        # teeth that join only in the last row
    z["comb_up"] = (ww % 2 == 0) | (hh == 0)
    r = np.zeros((H, W), bool)                                       # runs that cross column 64 (at W = 67) in every phase
    for h in range(H):
        if h % 4 == 0:
            r[h, max(0, W - 8 - h % 5):] = True
        elif h % 4 == 1:
            r[h, :min(W, 62 + h % 6)] = True
        elif h % 4 == 2:
            r[h, min(W - 1, 61 + h % 5):min(W, 66)] = True
    z["runs64"] = r
    return z


def field_of(mask_a, mask_b, rng):
    """float32 [2, H, W]: channel c exceeds 1 where its mask is set (and 2 on about half of those pixels)."""
    H, W = mask_a.shape
    lo, hi = rng.uniform(-3, 0.9, (2, H, W)), rng.uniform(1.1, 3.0, (2, H, W))
    return np.where(np.stack([mask_a, mask_b]), hi, lo).astype(F32)


def zoo_fields(H, W, seed=0):
    """[(name, float32 [2, H, W])]: every pattern in channel 0 next to another one in channel 1, then random masks of density
    0.1, 0.5 and 0.59 (the site-percolation threshold of the square lattice: the largest, most tortuous clusters)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    z = zoo(H, W)
    names = list(z)
    out = [(n, field_of(z[n], z[names[(i + 5) % len(names)]], rng)) for i, n in enumerate(names)]
    for d in (0.1, 0.5, 0.59):
        out.append((f"random{d}", field_of(rng.random((H, W)) < d, rng.random((H, W)) < d, rng)))
    return out


def spec3(conn, **kw):
    """3 output channels (2 + speed), 2 thresholds."""
    return ObjectSpec(2, speed=(0, 1), thresholds=(1.0, 2.0), connectivity=conn, quantum=2.0 ** -6, **kw)


def check_table(got, want, msg):
    assert got.dtype == want.dtype == np.int64 and got.shape == want.shape, (msg, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (msg, got[(got != want).any(1)][:4], want[(got != want).any(1)][:4])


# ------------------------------------------------------------------------------------------------- host reference == numpy
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("grid", [(1, 1), (1, 70), (70, 1), (5, 67), (12, 9), (33, 21)])
def test_host_reference_equals_the_numpy_restatement(grid, conn):
    H, W = grid
    spec = spec3(conn)
    fields = zoo_fields(H, W)
    for (name, a), (_, b) in zip(fields, fields[1:] + fields[:1]):
        table, count, per_plane = host_objects(spec, a, b)
        want, wpp = np_objects(spec, a, b)
        check_table(table, want, f"{grid} {conn} {name}")
        assert count == len(want) and np.array_equal(per_plane, wpp)
        one, c1, pp1 = host_objects(spec, a)                          # one series: no overlap, side 1 empty
        w1, wpp1 = np_objects(spec, a)
        check_table(one, w1, f"{grid} {conn} {name} alone")
        assert c1 == len(w1) and np.array_equal(pp1, wpp1) and not pp1[1].any() and not one[:, 3].any()


def test_the_zoo_has_the_objects_it_promises():
    H, W = 9, 12
    z = zoo(H, W)
    n = lambda name, conn: len(np.unique(np_labels(z[name], conn)[z[name]]))
    assert n("empty", 8) == 0 and n("full", 4) == 1 and n("corners", 8) == 4
    assert n("diagonal", 8) == 1 and n("diagonal", 4) == 9 and n("antidiagonal", 8) == 1 and n("antidiagonal", 4) == 9
    assert n("checkerboard", 4) == 54 and n("checkerboard", 8) == 1
    assert n("rings", 4) == n("rings", 8) == 3 and n("spiral", 4) == 1 and n("serpentine", 4) == 1
    assert n("comb", 4) == 1 and n("comb_up", 4) == 1
    r = zoo(5, 67)["runs64"]
    assert r[0, 59:].all() and r[1, :63].all() and not r[1, 63:].any() and r[2, 63:66].all() and not r[2, :63].any()


def test_root_is_the_smallest_index_and_the_key_is_unique():
    spec = spec3(8)
    for name, a in zoo_fields(33, 21):
        table, _, _ = host_objects(spec, a)
        key = table[:, 0] * (33 * 21) + table[:, 1]
        assert (np.diff(key) > 0).all(), name                           # sorted by (plane, root), no key twice
        h, w = np.divmod(table[:, 1], 21)
        assert (h == table[:, 8]).all() and (w >= table[:, 10]).all() and (w <= table[:, 11]).all(), name
        y = np_values(spec, a)
        for row in table[:50]:
            j, k = (row[0] // spec.K) % spec.nout, row[0] % spec.K
            m = (y[j] > spec.thresholds[j, k]).reshape(-1)
            assert m[row[1]] and not m[:row[1]][np_labels(m.reshape(33, 21), 8).reshape(-1)[:row[1]] == row[1]].any()


@pytest.mark.parametrize("conn", [4, 8])
def test_partition_equals_scipy(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    spec = ObjectSpec(1, speed=None, thresholds=(1.0,), connectivity=conn, quantum=1.0)
    structure = np.ones((3, 3), int) if conn == 8 else None
    for name, a in zoo_fields(33, 21):
        table, count, _ = host_objects(spec, a[:1])
        lab, n = ndimage.label(a[0] > 1.0, structure=structure)
        assert n == count, name
        roots = sorted(int(np.flatnonzero(lab.reshape(-1) == i)[0]) for i in range(1, n + 1))
        areas = {int(np.flatnonzero(lab.reshape(-1) == i)[0]): int((lab == i).sum()) for i in range(1, n + 1)}
        assert roots == table[:, 1].tolist() and [areas[r] for r in roots] == table[:, 2].tolist(), name


def test_special_values():
    """NaN is in no mask, +inf is and saturates q, -inf is not; equality with the threshold is outside; a negative y above a
    negative threshold is an object of mass 0; t >= 16777215 saturates; rint rounds halves to even."""
    spec = ObjectSpec(1, speed=None, thresholds=(1.0,), connectivity=4, quantum=1.0)
    a = np.array([[[np.nan, np.inf, -np.inf, 1.0, np.nextafter(F32(1), F32(2)), 2.5, 3.5, 0.0]]], F32)
    table, count, _ = host_objects(spec, a)
    check_table(table, np_objects(spec, a)[0], "special")
    assert count == 2 and table[:, 1].tolist() == [1, 4] and table[0, 2:8].tolist() == [1, 0, TOP, 0, TOP, TOP]
    assert table[1, 2] == 3 and table[1, 4] == 1 + 2 + 4 and table[1, 7] == 4       # rint(2.5) = 2, rint(3.5) = 4
    neg = ObjectSpec(1, speed=None, thresholds=(-2.0,), connectivity=4, quantum=0.5)
    b = np.array([[[-1.0, -1.5, -3.0, 0.25, 0.75]]], F32)
    t2, c2, _ = host_objects(neg, b)
    check_table(t2, np_objects(neg, b)[0], "negative")
    assert c2 == 2 and t2[0].tolist() == [0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1]        # mass 0, qmax 0
    assert t2[1, 4] == 0 + 2 and t2[1, 6] == 2 * 4                                  # rint(0.5) = 0, rint(1.5) = 2
    sat = ObjectSpec(1, speed=None, thresholds=(0.0,), connectivity=8, quantum=2.0 ** -10)
    c = np.array([[[16383.9990234375, 16384.0, 1e30]]], F32)                        # t = 16777215, 16777216, huge
    t3, _, _ = host_objects(sat, c)
    check_table(t3, np_objects(sat, c)[0], "saturating")
    assert t3[0, 2] == 3 and t3[0, 4] == 3 * TOP and t3[0, 7] == TOP and t3[0, 6] == 3 * TOP


def test_speed_channel_and_affine_transform():
    rng = np.random.default_rng(3)
    spec = ObjectSpec(3, scale=[2.0, 0.5, 1.5], offset=[0.1, -0.2, 0.3], speed=(2, 0), thresholds=[[0.5], [0.0], [1.0], [2.5]],
                      connectivity=8, quantum=2.0 ** -8)
    a, b = rng.normal(size=(2, 3, 17, 23)).astype(F32)
    table, _, pp = host_objects(spec, a, b)
    want, wpp = np_objects(spec, a, b)
    check_table(table, want, "affine + speed")
    assert np.array_equal(pp, wpp) and pp.min() > 0 and table[:, 3].max() > 0


def test_capacity_too_small_counts_everything_and_writes_nothing_beyond():
    spec = spec3(4)
    a, b = zoo_fields(12, 9)[5][1], zoo_fields(12, 9)[8][1]           # checkerboard: many objects
    full, count, per_plane = host_objects(spec, a, b)
    assert count == len(full) > 40
    s = spec.struct()
    for cap in (0, 1, 17, count - 1, count, count + 3):
        buf = np.full((cap + 2, 12), -7, np.int64)                    # two guard rows behind the table
        cnt, pp = np.zeros(1, np.int64), np.zeros((2, spec.nout, spec.K), np.int64)
        rc = _lib.lib().dg_objects_host(C.byref(s), a.ctypes.data, b.ctypes.data, 2, 12, 9, buf.ctypes.data if cap else None, cap,
                                        cnt.ctypes.data, pp.ctypes.data)
        assert rc == 0 and cnt[0] == count and np.array_equal(pp, per_plane), cap
        n = min(cap, count)
        assert np.array_equal(buf[:n], full[:n]) and (buf[n:] == -7).all(), cap


# ------------------------------------------------------------------------------------------------- spec, ABI
def test_spec_validation():
    ok = dict(C=2, thresholds=(1.0, 2.0))
    good = ObjectSpec(**ok)
    assert (good.nout, good.K, good.connectivity, good.min_area, good.names) == (3, 2, 8, 1, ["ch0", "ch1", "speed"])
    assert float(good.inv_quantum) == 1024.0 and good == ObjectSpec(**ok) and good != ObjectSpec(connectivity=4, **ok)
    for kw, msg in ((dict(C=0), "input channels"), (dict(C=9), "input channels"), (dict(speed=(0, 2)), "speed channels"),
                    (dict(thresholds=()), "1 to 4 thresholds"), (dict(thresholds=(1, 2, 3, 4, 5)), "1 to 4 thresholds"),
                    (dict(thresholds=[[1.0], [2.0]]), "one list per output channel"), (dict(thresholds=(np.nan,)), "finite"),
                    (dict(scale=[1.0]), "one value per input channel"), (dict(scale=[np.inf, 1.0]), "finite"),
                    (dict(connectivity=6), "connectivity is 4 or 8"), (dict(quantum=0.0), "quantum"), (dict(quantum=-1.0), "quantum"),
                    (dict(quantum=np.inf), "quantum"), (dict(quantum=1e-60), "inverse in fp32"), (dict(min_area=0), "min_area"),
                    (dict(min_area=1.5), "min_area"), (dict(names=["a"]), "names")):
        with pytest.raises(ValueError, match=msg):
            ObjectSpec(**dict(ok, **kw))
    z = ObjectSpec.zscore(1)
    assert z.speed is None and z.nout == 1 and z.thresholds.tolist() == [[1.0, 2.0]]
    p = ObjectSpec.physical({"u10": (1.0, 2.0), "v10": (-1.0, 3.0), "t2m": (280.0, 10.0)}, ["u10", "v10", "t2m"],
                            thresholds=[[5.0], [5.0], [290.0], [8.0]], quantum=0.01)
    assert p.names == ["u10", "v10", "t2m", "speed"] and p.speed == (0, 1) and p.scale.tolist() == [2.0, 3.0, 10.0]
    s = p.struct()
    assert (s.speed_u, s.speed_v, s.nthr, s.connectivity) == (0, 1, 1, 8) and s.inv_quantum == F32(100.0) and s.thr[3][0] == 8.0
    with pytest.raises(TypeError, match="ObjectSpec"):
        Objects("spec", 4, 4, ops=HostOps())
    with pytest.raises(ValueError, match="grid"):
        Objects(good, 4, 2049, ops=HostOps())
    acc = Objects(good, 4, 4, ops=HostOps())
    x = torch.zeros(2, 2, 4, 4)
    with pytest.raises(ValueError, match="paired"):
        acc.add(x)
    with pytest.raises(ValueError, match="4 x 4 grid"):
        acc.add(torch.zeros(2, 2, 4, 5), torch.zeros(2, 2, 4, 5))
    with pytest.raises(ValueError, match="differ in length"):
        acc.add(x, x[:1])
    with pytest.raises(ValueError, match="n_valid"):
        acc.add(x, x, n_valid=3)
    with pytest.raises(ValueError, match="input channels"):
        acc.add(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4, 4))


def test_header_declares_and_library_exports_the_objects_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert "Exceedance objects (csrc/objects.hip)" in src
    for name, v in (("SIDE", 2048), ("THR", 4)):
        assert re.search(rf"#define DG_OBJ_MAX_{name} {v}\b", src), name
    assert re.search(r"#define DG_OBJ_COLS 12\b", src)
    assert (_lib.OBJ_MAX_SIDE, _lib.OBJ_MAX_THR, _lib.OBJ_COLS) == (objects.SIDE_MAX, objects.THR_MAX, objects.COLS) == (2048, 4, 12)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"const dg_eof_fields*": C.POINTER(_lib.EofFields), "const dg_objects_spec*": C.POINTER(_lib.ObjectsSpec), "int": C.c_int,
             "int64_t": C.c_int64}
    for sym in ("dg_objects_ws_bytes", "dg_objects", "dg_objects_host"):
        m = re.search(rf"\b(size_t|int) {sym}\s*\(([^)]*)\)", code)
        assert m, sym
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
        args = [" ".join(a.split()[:-1]) for a in m.group(2).replace("\n", " ").split(",")]
        assert _lib._PROTOS[sym] == [ctype.get(a, C.c_void_p) for a in args], (sym, args)
    assert _lib._RESTYPES["dg_objects_ws_bytes"] is C.c_size_t
    assert "objects.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()


def test_objects_spec_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.ObjectsSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(dg_objects_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_objects_spec, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("thr_row %zu\\n", sizeof(((dg_objects_spec*)0)->thr[0]));', '  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert int(got["thr_row"]) == 4 * _lib.OBJ_MAX_THR


def test_abi_rejects_bad_arguments_without_launching():
    """Every pointer is a made-up address: a call that passed the checks would fault instead of returning a status."""
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))

    def spec(**kw):
        s = ObjectSpec.zscore(2).struct()
        for k, v in kw.items():
            if k == "thr":
                s.thr[v[0]][v[1]] = v[2]
            elif k in ("scale", "offset"):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    good, p = spec(), C.c_void_p(0x2000)
    names = ("a", "b", "H", "W", "s", "ws", "table", "capacity", "count", "per_plane", "stream")
    base = dict(a=f(), b=f(), H=10, W=10, s=good, ws=p, table=p, capacity=8, count=p, per_plane=p, stream=None)
    call = lambda **kw: lib.dg_objects(*[dict(base, **kw)[k] for k in names])
    bad = [dict(a=None), dict(s=None), dict(ws=None), dict(count=None), dict(per_plane=None), dict(table=None), dict(capacity=-1),
           dict(b=f(T=3)), dict(b=f(C=1)), dict(b=f(P=99)), dict(H=10, W=11), dict(a=f(P=2049), b=f(P=2049), H=1, W=2049),
           dict(a=f(P=2049), b=f(P=2049), H=2049, W=1), dict(s=spec(connectivity=6)), dict(s=spec(connectivity=0)),
           dict(s=spec(nthr=0)), dict(s=spec(nthr=5)), dict(s=spec(inv_quantum=0.0)), dict(s=spec(inv_quantum=-1.0)),
           dict(s=spec(inv_quantum=math.inf)), dict(s=spec(inv_quantum=math.nan)), dict(s=spec(thr=(2, 1, math.nan))),
           dict(s=spec(thr=(0, 0, math.inf))), dict(s=spec(scale=(1, math.inf))), dict(s=spec(offset=(0, math.nan))),
           dict(s=spec(speed_u=2)), dict(s=spec(speed_v=-1)), dict(a=f(base=0)), dict(a=f(C=9), b=f(C=9))]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(a=f(dtype=7)) == -2 and call(b=f(dtype=7)) == -2
    assert lib.dg_objects_ws_bytes(f(), 10, 10, good) == 256 + 8 * 4 * 2 * 3 * 2 * 100
    assert lib.dg_objects_ws_bytes(f(), 10, 11, good) == 0 and lib.dg_objects_ws_bytes(None, 10, 10, good) == 0
    assert lib.dg_objects_ws_bytes(f(), 10, 10, spec(connectivity=5)) == 0
    # T 2 nout nthr ceil(P / 2) >= 2^31: more objects than the int32 slot ids of one call can number
    assert lib.dg_objects_ws_bytes(f(T=100, P=2048 * 2048), 2048, 2048, good) == 0
    assert lib.dg_objects_ws_bytes(f(T=85, P=2048 * 2048), 2048, 2048, good) > 0
    hn = ("s", "a", "b", "C", "H", "W", "table", "capacity", "count", "per_plane")
    hd = dict(s=good, a=p, b=p, C=2, H=4, W=4, table=p, capacity=4, count=p, per_plane=p)
    host = lambda **kw: lib.dg_objects_host(*[dict(hd, **kw)[k] for k in hn])
    for kw in (dict(s=None), dict(a=None), dict(C=0), dict(C=9), dict(H=0), dict(W=2049), dict(table=None), dict(capacity=-1),
               dict(count=None), dict(per_plane=None), dict(s=spec(connectivity=7)), dict(s=spec(inv_quantum=0.0)), dict(C=1)):
        assert host(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------- SAL and the scores
def blob(H, W, boxes, value=2.0):
    """float32 [1, 1, H, W]: ``value`` on the boxes (h0, h1, w0, w1; inclusive), 0 elsewhere."""
    x = np.zeros((1, 1, H, W), F32)
    for h0, h1, w0, w1 in boxes:
        x[0, 0, h0:h1 + 1, w0:w1 + 1] = value
    return torch.from_numpy(x)


SPEC1 = ObjectSpec(1, speed=None, thresholds=(1.0,), connectivity=8, quantum=0.25)


def run1(a, b, spec=SPEC1, **kw):
    return objects.objects(a, b, spec=spec, ops=HostOps(), **kw)


def test_identical_series_score_perfectly():
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.normal(size=(3, 2, 20, 31)).astype(F32))
    res = run1(x, x.clone(), spec=ObjectSpec.zscore(2, thresholds=(0.5, 1.0)))
    sal = res.sal()
    assert (sal["pairs"] > 0).all()
    for k in ("S", "A", "L1", "L2", "L", "abs_S", "abs_A", "abs_L"):
        assert np.array_equal(sal[k], np.zeros((3, 2))), k
    assert np.array_equal(res.pod(), np.ones((3, 2))) and np.array_equal(res.far(), np.zeros((3, 2)))
    assert np.array_equal(res.csi(), np.ones((3, 2))) and np.array_equal(res.counts()[0], res.counts()[1])
    assert np.array_equal(res.matched(), res.counts())


def test_a_shifted_object_moves_only_L1():
    H, W = 30, 40
    d = math.hypot(H - 1, W - 1)
    res = run1(blob(H, W, [(5, 9, 6, 12)]), blob(H, W, [(8, 12, 10, 16)]))          # shifted by (3, 4)
    p = res.sal_pairs()
    assert abs(p["L1"][0, 0, 0] - 5.0 / d) <= 1e-12 and p["S"][0, 0, 0] == 0 and p["A"][0, 0, 0] == 0 and p["L2"][0, 0, 0] == 0
    sal = res.sal()
    assert abs(sal["L"][0, 0] - 5.0 / d) <= 1e-12 and sal["pairs"][0, 0] == 1
    assert res.pod()[0, 0] == 1 and res.far()[0, 0] == 0                             # the boxes still share pixels
    assert not res.sal_undefined().any()


def test_doubled_intensities_move_only_A():
    """q doubles exactly on the fixed-point grid (2.0 / 0.25 = 8 -> 16): R_b = 2 R_a, A = (2 - 1) / 1.5 = 2 / 3; V = sum R_n^2 /
    qmax_n / R is unchanged (the 2^2 / 2 of the numerator against the 2 of R), S = 0; the centres do not move."""
    H, W = 24, 24
    boxes = [(2, 5, 3, 9), (12, 20, 10, 14)]
    p = run1(blob(H, W, boxes, 2.0), blob(H, W, boxes, 4.0)).sal_pairs()
    assert abs(p["A"][0, 0, 0] - 2.0 / 3.0) <= 1e-12 and p["S"][0, 0, 0] == 0 and p["L1"][0, 0, 0] == 0 and p["L2"][0, 0, 0] == 0


def test_one_object_against_four_scattered_ones():
    """Real: one 4 x 4 block of q = 8 (R = 128).  Generated: the same mass in four 2 x 2 blocks of q = 8 placed symmetrically
    around the same centre.  The centres of mass agree (L1 = 0); the real spread r is 0 and the generated one is the distance of
    the small blocks from the centre (L2 = 2 r_b / d > 0).  V = sum R_n (R_n / qmax_n) / R is 128 / 8 = 16 for the single object
    and 4 * 32 * (32 / 8) / 128 = 4 for the scattered ones: smaller, flatter objects, so S = (4 - 16) / 10 = -1.2 < 0."""
    H, W = 21, 21
    d = math.hypot(H - 1, W - 1)
    real = blob(H, W, [(9, 12, 9, 12)])
    fake = blob(H, W, [(2, 3, 2, 3), (2, 3, 18, 19), (18, 19, 2, 3), (18, 19, 18, 19)])
    res = run1(real, fake)
    p = res.sal_pairs()
    assert p["A"][0, 0, 0] == 0 and abs(p["L1"][0, 0, 0]) <= 1e-12
    assert abs(p["S"][0, 0, 0] + 1.2) <= 1e-12
    assert abs(p["L2"][0, 0, 0] - 2 * math.hypot(8, 8) / d) <= 1e-12
    assert res.pod()[0, 0] == 0 and res.far()[0, 0] == 1 and res.csi()[0, 0] == 0     # nothing overlaps


def test_an_invented_object_is_a_false_alarm():
    H, W = 16, 16
    real = blob(H, W, [(1, 3, 1, 3), (10, 12, 10, 12)])
    fake = blob(H, W, [(1, 3, 2, 4), (10, 12, 9, 11), (1, 2, 12, 14)])                # two displaced, one invented
    res = run1(real, fake)
    assert res.counts()[:, 0, 0].tolist() == [2, 3] and res.matched()[:, 0, 0].tolist() == [2, 2]
    assert res.pod()[0, 0] == 1 and abs(res.far()[0, 0] - 1 / 3) <= 1e-12 and abs(res.csi()[0, 0] - 2 / 3) <= 1e-12


def test_undefined_pairs_are_counted_by_kind():
    H, W = 8, 8
    one, none = blob(H, W, [(2, 3, 2, 3)]), blob(H, W, [])
    real = torch.cat([one, one, none, none])
    fake = torch.cat([one, none, one, none])
    res = run1(real, fake, keep_records=True)
    assert res.sal_undefined()[0, 0].tolist() == [1, 1, 1] and res.sal()["pairs"][0, 0] == 1
    p = res.sal_pairs()["S"][:, 0, 0]
    assert p[0] == 0 and np.isnan(p[1:]).all()
    assert res.empty_fields()[:, 0, 0].tolist() == [2, 2] and res.fields == 4
    assert res.records[:, 0].tolist() == [0, 0, 1, 2] and res.records[:, 1].tolist() == [0, 1, 0, 1]   # field, plane
    s = res.summary()
    assert json.loads(json.dumps(s, allow_nan=False)) == s and s["sal_undefined"] == {"real_only": [[1]], "fake_only": [[1]], "neither": [[1]]}
    assert isinstance(s["count"]["real"][0][0], int) and s["count"] == {"real": [[2]], "fake": [[2]]}
    empty = run1(none, none)
    assert np.isnan(empty.pod()[0, 0]) and np.isnan(empty.sal()["S"][0, 0]) and empty.summary()["pod"] == [[None]]
    # mass 0 objects (negative y above a negative threshold) exist for the counts but not for SAL
    neg = ObjectSpec(1, speed=None, thresholds=(-2.0,), connectivity=8, quantum=0.25)
    z = run1(torch.full((1, 1, 4, 4), -1.0), torch.full((1, 1, 4, 4), -1.0), spec=neg)
    assert z.counts()[:, 0, 0].tolist() == [1, 1] and z.sal_undefined()[0, 0].tolist() == [0, 0, 1] and z.mass_histogram()[0, 0, 0, 0] == 1


def test_pooled_tables_and_min_area():
    rng = np.random.default_rng(9)
    a, b = (rng.normal(size=(4, 2, 19, 27)).astype(F32) for _ in range(2))
    for min_area in (1, 3):
        spec = spec3(8, min_area=min_area)
        res = objects.objects(torch.from_numpy(a), torch.from_numpy(b), spec=spec, ops=HostOps())
        recs = [np_objects(spec, a[t], b[t])[0] for t in range(4)]
        allr = np.concatenate(recs)
        keep = allr[allr[:, 2] >= min_area]
        for side in range(2):
            for j in range(3):
                for k in range(2):
                    r = keep[keep[:, 0] == (side * 3 + j) * 2 + k]
                    assert res.counts()[side, j, k] == len(r)
                    cnt, area = res.area_histogram()
                    for bin_ in range(objects.AREA_BINS):
                        m = (r[:, 2] >= 1 << bin_) & (r[:, 2] < 2 << bin_)
                        assert cnt[side, j, k, bin_] == m.sum() and area[side, j, k, bin_] == r[m, 2].sum()
                    mh = res.mass_histogram()[side, j, k]
                    assert mh[0] == (r[:, 4] == 0).sum() and mh.sum() == len(r)
                    for bin_ in range(1, objects.MASS_BINS):
                        assert mh[bin_] == ((r[:, 4] >= 1 << (bin_ - 1)) & (r[:, 4] < 1 << bin_)).sum()
                    assert res.max_area()[side, j, k] == (r[:, 2].max() if len(r) else 0)
                    assert res.matched()[side, j, k] == (r[:, 3] > 0).sum()
                    empty = sum(1 for t in range(4) if not ((recs[t][:, 0] == (side * 3 + j) * 2 + k) & (recs[t][:, 2] >= min_area)).any())
                    assert res.empty_fields()[side, j, k] == empty
        assert res.fields == 4 and np.allclose(res.objects_per_field(), res.counts() / 4)
    one = objects.objects(torch.from_numpy(a), spec=spec3(8), ops=HostOps())
    assert one.counts().shape == (1, 3, 2) and not one.paired
    with pytest.raises(ValueError, match="needs real and generated"):
        one.pod()
    # whole batch == field by field; NHWC with padding == NCHW
    acc = Objects(spec3(8), 19, 27, ops=HostOps(), keep_records=True)
    for t in range(4):
        acc.add(torch.from_numpy(a[t:t + 1]), torch.from_numpy(b[t:t + 1]))
    whole = objects.objects(torch.from_numpy(a), torch.from_numpy(b), spec=spec3(8), ops=HostOps(), keep_records=True)
    assert acc.result().summary() == whole.summary() and np.array_equal(acc.result().records, whole.records)
    pad = torch.full((4, 19, 27, 5), 9.0)
    pad[..., :2] = torch.from_numpy(a).permute(0, 2, 3, 1)
    nhwc = objects.objects(pad, torch.from_numpy(b), spec=spec3(8), ops=HostOps(), nhwc=(True, False), channels=2, n_valid=3)
    first = objects.objects(torch.from_numpy(a[:3]), torch.from_numpy(b[:3]), spec=spec3(8), ops=HostOps())
    assert nhwc.summary() == first.summary() and nhwc.fields == 3


# ------------------------------------------------------------------------------------------------- reduce_
def _rank_data(world):
    rng = np.random.default_rng(17)
    a, b = (rng.normal(size=(6, 2, 16, 16)).astype(F32) for _ in range(2))
    b[4:] = -5.0                                                      # generated fields without any object: undefined pairs
    return a, b


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    a, b = _rank_data(world)
    acc = Objects(spec3(8), 16, 16, ops=HostOps())
    acc.add(torch.from_numpy(a[rank::world].copy()), torch.from_numpy(b[rank::world].copy()))
    res = acc.reduce_(d).result()
    torch.save({"summary": res.summary(), "tables": {k: v for k, v in res._t.items()}, "sal": res._sal, "und": res._undefined},
               os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_tables():
    a, b = _rank_data(2)
    ref = objects.objects(torch.from_numpy(a), torch.from_numpy(b), spec=spec3(8), ops=HostOps())
    assert ref.sal_undefined().sum() > 0
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["summary"] == r1["summary"] and r0["sal"].tobytes() == r1["sal"].tobytes()
    for k, v in ref._t.items():
        assert np.array_equal(r0["tables"][k], v), k                  # the integers exactly, the largest area by max
    assert np.array_equal(r0["und"], ref._undefined) and r0["summary"]["fields"] == 6
    assert np.array_equal(r0["sal"][..., 8], ref._sal[..., 8])        # the pair counts exactly
    np.testing.assert_allclose(r0["sal"], ref._sal, rtol=1e-12, atol=1e-12)   # float sums in another order
    ints = {k: v for k, v in r0["summary"].items() if k not in ("sal", "objects_per_field", "mean_area", "pod", "far", "csi")}
    assert ints == {k: ref.summary()[k] for k in ints}


# ------------------------------------------------------------------------------------------------- the trainer's defaults
def test_the_hook_is_off_by_default():
    import inspect
    from downgan_amd.engine import TrainEngine
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_objects is False and WassersteinGAN.objects_spec is None and WassersteinGAN.objects_results is None
    assert inspect.signature(WassersteinGAN.gen_batch_and_log_metrics).parameters["objects"].default is None
    assert inspect.signature(TrainEngine.metrics_pass).parameters["objects"].default is None
