"""Joint histograms without a GPU: the library's host bin rules (dg_hist2d_host_bins) against a numpy float32 restatement of the
definition -- the 1-D rule per axis and the direction rule, every multiply rounded to float32 -- on adversarial values; the
direction rule against float64 atan2 away from the sector boundaries; argument checks that fire before any library call; the ABI
surface and struct layouts; known answers of the derived statistics; and the trainer's opt-in hook on the emulated ops (a
test-local op class implements ``hist2d`` by the restatement), in one process, over 2 gloo ranks, and in the frequency-separation
trainer."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from downgan_amd import _lib, joint
from downgan_amd.joint import Axis, Joint, JointSpec

from .test_histograms_cpu import F32, SPECIAL, _loaders, edge_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSECS = (4, 8, 16, 36, 72)


# ------------------------------------------------------------------------------------------------- the definition in numpy
def view(s, Cn):
    """A dg_hist2d_spec (ctypes) as numpy float32 values."""
    return types.SimpleNamespace(
        C=Cn, npairs=s.npairs, su=s.speed_u, sv=s.speed_v, nsec=s.nsec, calm=F32(s.calm), tan=np.array(s.tan_k[:], dtype=F32),
        scale=np.array(s.scale[:Cn], dtype=F32), offset=np.array(s.offset[:Cn], dtype=F32),
        ax=[[(a.src, a.chan, a.nbins, F32(a.lo), F32(a.inv_w)) for a in s.ax[p]] for p in range(s.npairs)])


def bin_ref(y, lo, inv_w, nbins):
    """The 1-D rule: 0 underflow, 1 .. nbins interior, nbins + 1 overflow, nbins + 2 NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = ((y - lo).astype(F32) * inv_w).astype(F32)
        inner = np.where((t >= 0) & (t < nbins), t, 0).astype(np.int64) + 1
        return np.where(np.isnan(t), nbins + 2, np.where(t < 0, 0, np.where(t >= nbins, nbins + 1, inner)))


def dir_ref(yu, yv, s, calm, nsec, tan):
    """The direction rule, steps 1-8: float32 values, one float32 product per compare."""
    K = nsec // 4
    with np.errstate(over="ignore", invalid="ignore"):
        x, y = (-yu).astype(F32), (-yv).astype(F32)
        ax, ay = np.abs(x), np.abs(y)
        swap = ax > ay
        m, M = np.where(swap, ay, ax), np.where(swap, ax, ay)
        j = np.zeros(x.shape, dtype=np.int64)
        for k in range(1, K):
            j += m >= (M * F32(tan[k])).astype(F32)
        q = np.where(swap, 2 * K - 1 - j, j)
        h = np.where((x >= 0) & (y > 0), q, np.where((x > 0) & (y <= 0), 4 * K - 1 - q, np.where((x <= 0) & (y < 0), 4 * K + q,
                                                                                                8 * K - 1 - q)))
        idx = 1 + ((h + 1) >> 1) % nsec
        idx = np.where(s > calm, idx, 0)
        return np.where(np.isnan(yu) | np.isnan(yv), nsec + 2, idx)


def bins2_ref(v, xa, xb=None):
    """int64 [npairs, 2, n] of xa, xb float32 [C, n] under the spec view v."""
    n = xa.shape[1]
    ys, sp, dr = [], [], []
    for x in (xa, xb):
        if x is None:
            ys.append(None); sp.append(None); dr.append(None)
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            y = ((np.asarray(x, dtype=F32) * v.scale[:, None]).astype(F32) + v.offset[:, None]).astype(F32)
            s = d = None
            if v.su >= 0:
                u, w = y[v.su], y[v.sv]
                s = np.sqrt((u * u).astype(F32) + (w * w).astype(F32)).astype(F32)
                if v.nsec:
                    d = dir_ref(u, w, s, v.calm, v.nsec, v.tan)
        ys.append(y); sp.append(s); dr.append(d)
    out = np.empty((v.npairs, 2, n), dtype=np.int64)
    for p in range(v.npairs):
        for e, (src, chan, nb, lo, inv_w) in enumerate(v.ax[p]):
            out[p, e] = dr[src] if chan == v.C + 1 else bin_ref(sp[src] if chan == v.C else ys[src][chan], lo, inv_w, nb)
    return out


def tables_ref(spec, xa, xb=None):
    """The int64 tables of a JointSpec over xa, xb float32 [C, n], concatenated in pair order."""
    s = spec.struct()
    b = bins2_ref(view(s, spec.C), xa, xb)
    out = []
    for p, (nx, ny) in enumerate(spec.table_shapes()):
        out.append(np.bincount(b[p, 0] * ny + b[p, 1], minlength=nx * ny))
        assert len(out[-1]) == nx * ny
    return np.concatenate(out)


def check_host(spec, xa, xb=None):
    xa = np.ascontiguousarray(xa, dtype=F32)
    xb = None if xb is None else np.ascontiguousarray(xb, dtype=F32)
    got = joint.host_bins(spec, xa, xb)
    np.testing.assert_array_equal(got, bins2_ref(view(spec.struct(), spec.C), xa, xb))
    return got


def rose_spec(nsec, calm=0.0, bins=32, lim=6.0, **kw):
    c = lambda src, ch: Axis(src, ch, bins, -lim, lim)
    s = lambda src: Axis(src, "speed", bins, 0.0, lim * math.sqrt(2))
    return JointSpec([(Axis("a", "direction", nsec), s("a")), (c("a", 0), c("b", 0)), (Axis("b", "direction", nsec), c("b", 1)),
                      (s("a"), s("b"))], 2, calm=calm, **kw)


# ------------------------------------------------------------------------------------------------- the host rules
@pytest.mark.parametrize("nsec", NSECS)
def test_edges_specials_and_signed_zeros(nsec):
    spec = rose_spec(nsec)
    e = np.concatenate([edge_values(-6.0, 12 / 32, 32), SPECIAL])
    g = np.array(np.meshgrid(SPECIAL, SPECIAL)).reshape(2, -1)                  # every special in one or both components
    xa = np.concatenate([np.stack([e, np.roll(e, 7)]), g, np.stack([e[:len(SPECIAL)], SPECIAL])], axis=1)
    xb = np.concatenate([np.stack([np.roll(e, 3), e]), g[::-1], np.stack([SPECIAL, e[:len(SPECIAL)]])], axis=1)
    got = check_host(spec, xa, xb)
    nan = np.isnan(xa[0]) | np.isnan(xa[1])
    assert (got[0, 0][nan] == nsec + 2).all() and (got[0, 0][~nan] <= nsec).all()       # nsec + 1 is never used
    zero = (xa[0] == 0) & (xa[1] == 0)
    assert zero.sum() >= 4 and (got[0, 0][zero] == 0).all()                             # +-0, +-0 is calm


@pytest.mark.parametrize("nsec", NSECS)
def test_cardinal_directions_and_exact_diagonals(nsec):
    spec = rose_spec(nsec)
    K = nsec // 4
    # the wind FROM north blows towards -v: (u, v) = (0, -1); from east (-1, 0); from south (0, 1); from west (1, 0)
    card = np.array([[0, -1], [-1, 0], [0, 1], [1, 0]], dtype=F32).T * F32(2.5)
    got = check_host(spec, card, card)
    assert got[0, 0].tolist() == [1, 1 + K, 1 + 2 * K, 1 + 3 * K]
    r = np.array([0.37, 1.0, 3.0, 1e-30, 1e30], dtype=F32)
    diag = np.concatenate([np.stack([sx * r, sy * r]) for sx in (1, -1) for sy in (1, -1)], axis=1)
    check_host(spec, diag, diag[:, ::-1].copy())


@pytest.mark.parametrize("nsec", NSECS)
def test_points_on_a_sector_boundary_and_their_neighbours(nsec):
    spec = rose_spec(nsec)
    K = nsec // 4
    rng = np.random.default_rng(nsec)
    M = np.concatenate([rng.uniform(0.01, 6.0, 200), [1.0, 2.0, 1e-20, 1e20]]).astype(F32)
    pts = []
    for k in range(1, K):
        m0 = (M * spec.tan_k[k]).astype(F32)                                   # m == fp32(M * t_k): on the boundary
        for m in (m0, np.nextafter(m0, F32(0)), np.nextafter(m0, F32(np.inf))):
            for sx in (1, -1):
                for sy in (1, -1):
                    pts += [np.stack([sx * m, sy * M]), np.stack([sx * M, sy * m])]
    if not pts:                                                                 # nsec = 4: the only boundaries are the diagonals
        pts = [np.stack([M, M]), np.stack([np.nextafter(M, F32(0)), M]), np.stack([-M, np.nextafter(M, F32(0))])]
    x = np.concatenate(pts, axis=1).astype(F32)
    got = check_host(spec, x, -x)
    if K > 1:
        assert len(np.unique(got[0, 0])) == nsec                               # every sector is reached


def test_speed_equal_to_calm_and_its_neighbours():
    five = F32(5.0)
    x = np.array([[3.0, -3.0, 0.0, 5.0], [4.0, 4.0, -5.0, 0.0]], dtype=F32)     # s = 5 exactly
    for calm, is_calm in ((np.nextafter(five, F32(0)), False), (five, True), (np.nextafter(five, F32(10)), True)):
        spec = rose_spec(16, calm=float(calm))
        assert spec.calm == calm
        got = check_host(spec, x, x)
        assert ((got[0, 0] == 0) == is_calm).all()
    lo, hi = np.nextafter(five, F32(0)), np.nextafter(five, F32(10))
    s = np.array([lo, five, hi], dtype=F32)                                     # (0, s): s = |s| exactly
    got = check_host(rose_spec(8, calm=5.0), np.stack([np.zeros(3, F32), s]), np.stack([s, np.zeros(3, F32)]))
    assert (got[0, 0] == 0).tolist() == [True, True, False]


@pytest.mark.parametrize("nsec", NSECS)
def test_a_million_gaussian_points(nsec):
    rng = np.random.default_rng(100 + nsec)
    xa, xb = rng.standard_normal((2, 2, 1_000_000)).astype(F32) * F32(2)
    spec = rose_spec(nsec, calm=0.3, scale=[1.5, 0.75], offset=[0.25, -0.5])
    check_host(spec, xa, xb)


def _sectors(nsec, u, v):
    spec = JointSpec([(Axis("a", "direction", nsec), Axis("a", "speed", 4, 0.0, 10.0))], 2)
    return joint.host_bins(spec, np.stack([u, v]))[0, 0].astype(np.int64) - 1


@pytest.mark.parametrize("nsec", NSECS)
def test_direction_against_float64_atan2(nsec):
    rng = np.random.default_rng(7)
    u, v = rng.standard_normal((2, 1_000_000)).astype(F32)
    got = _sectors(nsec, u, v)
    w = 2 * np.pi / nsec
    t = np.arctan2(-u.astype(np.float64), -v.astype(np.float64)) / w + 0.5
    want = np.floor(t).astype(np.int64) % nsec
    frac = t - np.floor(t)
    far = np.minimum(frac, 1 - frac) * w > 1e-4
    print(f"nsec {nsec}: {(~far).mean() * 100:.3f} % within 1e-4 rad of a boundary, {(got != want).sum()} disagree in all")
    assert (~far).mean() <= 0.01
    np.testing.assert_array_equal(got[far], want[far])


@pytest.mark.parametrize("nsec", NSECS)
def test_quarter_turn_shifts_the_sector_by_a_quarter(nsec):
    rng = np.random.default_rng(9)
    u, v = rng.standard_normal((2, 100_000)).astype(F32)
    np.testing.assert_array_equal(_sectors(nsec, v, -u), (_sectors(nsec, u, v) + nsec // 4) % nsec)


# ------------------------------------------------------------------------------------------------- argument checks
def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("library or device touched before the arguments were checked")
    from downgan_amd import backend
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(backend, "make_ops", boom)
    monkeypatch.setattr(joint, "_ops", {})


@pytest.mark.parametrize("kw,match", [
    (dict(source="c", channel=0, bins=8, lo=0.0, hi=1.0), "source"),
    (dict(source="a", channel=-1, bins=8, lo=0.0, hi=1.0), "channel"),
    (dict(source="a", channel="gust", bins=8, lo=0.0, hi=1.0), "channel"),
    (dict(source="a", channel=0, bins=0, lo=0.0, hi=1.0), "bins"),
    (dict(source="a", channel=0, bins=2.5, lo=0.0, hi=1.0), "bins"),
    (dict(source="a", channel=0, bins=8), "lo and hi"),
    (dict(source="a", channel=0, bins=8, lo=1.0, hi=1.0), "lo < hi"),
    (dict(source="a", channel=0, bins=8, lo=0.0, hi=np.inf), "finite"),
    (dict(source="a", channel=0, bins=8, lo=-1e39, hi=0.0), "fp32"),
    (dict(source="a", channel=0, bins=4096, lo=0.0, hi=1e-42), "bin width"),
    (dict(source="a", channel="direction", bins=10), "multiple of 4"),
    (dict(source="a", channel="direction", bins=76), "multiple of 4"),
    (dict(source="a", channel="direction", bins=8, lo=0.0, hi=1.0), "no lo / hi"),
])
def test_axis_is_checked(monkeypatch, kw, match):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=match):
        Axis(**kw)


def test_spec_is_checked(monkeypatch):
    _no_library(monkeypatch)
    c = lambda src, ch, bins=8: Axis(src, ch, bins, 0.0, 1.0)
    d = lambda n: Axis("a", "direction", n)
    sp = Axis("a", "speed", 8, 0.0, 2.0)
    bad = [(dict(pairs=[], C=2), "pairs"), (dict(pairs=[(c("a", 0), c("b", 0))] * 9, C=2), "pairs"),
           (dict(pairs=[(c("a", 0), c("b", 2))], C=2), "channel 2"), (dict(pairs=[(c("a", 0), c("b", 0))], C=9), "C <="),
           (dict(pairs=[(c("a", 0), c("b", 0))], C=0), "C <="),
           (dict(pairs=[(c("a", 0, 125), c("b", 0, 126))], C=1, speed=None), "cells"),
           (dict(pairs=[(sp, c("a", 0))], C=2, speed=None), "speed pair"),
           (dict(pairs=[(d(8), c("a", 0))], C=2, speed=None), "speed pair"),
           (dict(pairs=[(c("a", 0), c("a", 0))], C=1), "speed"),                 # the default speed (0, 1) of one channel
           (dict(pairs=[(c("a", 0), c("a", 0))], C=3, speed=(0, 3)), "speed"),
           (dict(pairs=[(d(8), sp), (d(16), sp)], C=2), "sector count"),
           (dict(pairs=[(c("a", 0), c("b", 0))], C=2, calm=-0.5), "calm"),
           (dict(pairs=[(c("a", 0), c("b", 0))], C=2, calm=np.inf), "finite"),
           (dict(pairs=[(c("a", 0), c("b", 0))], C=2, scale=[1.0]), "scale"),
           (dict(pairs=[(c("a", 0), c("b", 0))], C=2, offset=[0.0, np.nan]), "finite"),
           (dict(pairs=[(c("a", 0), c("b", 0))], C=2, names=["x", "y"]), "names")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            JointSpec(**kw)
    with pytest.raises(TypeError, match="Axis"):
        JointSpec([(c("a", 0), "b")], 2)
    JointSpec([(c("a", 0, 125), c("b", 0, 125))], 1, speed=None)               # exactly CELLS_MAX cells


@pytest.mark.parametrize("a,b,kw,err,match", [
    (torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8), {}, ValueError, "C = 2"),
    (torch.zeros(2, 2, 8, 8), None, {}, ValueError, "b is None"),
    (torch.zeros(2, 2, 8, 8), torch.zeros(3, 2, 8, 8), {}, ValueError, "length"),
    (torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 9), {}, ValueError, "grid"),
    (torch.zeros(2, 2, 8, 8), torch.zeros(2, 8, 8, 4), {"nhwc": (False, True), "channels": 5}, ValueError, "channels"),
    (torch.zeros(2, 2, 8, 8, dtype=torch.float64), torch.zeros(2, 2, 8, 8), {}, TypeError, "fp32 or bf16"),
    (torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8, dtype=torch.float16), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 2, 8, 8), np.float32), torch.zeros(2, 2, 8, 8), {}, TypeError, "tensor"),
    (torch.zeros(2, 8, 8), torch.zeros(2, 2, 8, 8), {}, ValueError, "shape"),
    (torch.zeros(0, 2, 8, 8), torch.zeros(0, 2, 8, 8), {}, ValueError, "at least one"),
    (torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8), {"nhwc": (True, False, True)}, ValueError, "nhwc"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, a, b, kw, err, match):
    _no_library(monkeypatch)
    spec = JointSpec.zscore(2)
    with pytest.raises(err, match=match):
        joint.joint_histogram(a, spec, b, **kw)
    acc = joint.ValueJoint(spec, device="cpu")
    with pytest.raises(err, match=match):
        acc.add(a, b, **kw)
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            acc.add(torch.zeros(2, 2, 8, 8), torch.zeros(2, 2, 8, 8), n_valid=n)
    with pytest.raises(TypeError, match="JointSpec"):
        joint.joint_histogram(torch.zeros(1, 2, 4, 4), None)
    with pytest.raises(TypeError, match="JointSpec"):
        joint.ValueJoint([0.0, 1.0], device="cpu")
    with pytest.raises(ValueError, match="xb is None"):
        joint.host_bins(spec, np.zeros((2, 4), F32))
    with pytest.raises(ValueError, match=r"\[C = 2, n\]"):
        joint.host_bins(spec, np.zeros((3, 4), F32), np.zeros((3, 4), F32))


def test_constructors():
    z = JointSpec.zscore(2)
    assert z.names == ["rose_real", "rose_fake", "uv_real", "uv_fake", "ch0", "ch1", "speed"] and z.nsec == 36 and z.speed == (0, 1)
    assert z.table_shapes() == [(39, 67)] * 2 + [(99, 99)] * 4 + [(67, 67)]
    assert z.offsets()[-1] == 2 * 39 * 67 + 4 * 99 * 99 + 67 * 67 and len(z.offsets()) == 8
    assert JointSpec.zscore(3).npairs == 8 and JointSpec.zscore(3).names[-1] == "speed"
    assert JointSpec.zscore(5).npairs == 8 and JointSpec.zscore(5).names[-1] == "ch3"          # dropped from the end
    one = JointSpec.zscore(1)
    assert one.speed is None and one.npairs == 1 and one.uses_b
    s = z.struct()
    assert (s.npairs, s.speed_u, s.speed_v, s.nsec) == (7, 0, 1, 36) and s.ax[0][0].chan == 3 and s.ax[0][1].chan == 2
    assert s.ax[4][1].src == 1 and s.tan_k[0] == 0.0
    for k in range(1, 9):
        assert s.tan_k[k] == F32(math.tan(k * math.pi / 36))
    stats = {"u10": (0.5, 3.0), "v10": (-0.25, 2.0), "t2m": (280.0, 10.0)}
    p = JointSpec.physical(stats, ["t2m", "u10", "v10"], -40.0, 40.0)
    assert p.speed == (1, 2) and p.names == ["rose_real", "rose_fake", "uv_real", "uv_fake", "t2m", "u10", "v10", "speed"]
    assert p.scale.tolist() == [10.0, 3.0, 2.0] and p.offset.tolist() == [280.0, 0.5, -0.25] and p.calm == F32(0.5)
    assert p.pairs[2][0].channel == 1 and p.pairs[2][1].channel == 2 and p.pairs[7][0].hi == F32(40 * math.sqrt(2))
    assert p == JointSpec.physical(stats, ["t2m", "u10", "v10"], -40.0, 40.0) and p != z and z == JointSpec.zscore(2)
    assert z != JointSpec.zscore(2, nsec=16) and JointSpec.physical(stats, ["t2m"], -40.0, 40.0, speed=None).names == ["t2m"]


# ------------------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_joint_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    for name, val in (("PAIRS", 8), ("CELLS", 16384), ("SECTORS", 72)):
        assert re.search(rf"#define DG_HIST2D_MAX_{name} {val}\b", src), name
    for sym in ("dg_hist2d_ws_bytes", "dg_hist2d", "dg_hist2d_host_bins"):
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS
        assert hasattr(_lib.lib(), sym)
    assert (_lib.HIST2D_MAX_PAIRS, _lib.HIST2D_MAX_CELLS, _lib.HIST2D_MAX_SECTORS) == (8, 16384, 72)
    assert (joint.PAIRS_MAX, joint.CELLS_MAX, joint.SECTORS_MAX) == (8, 16384, 72)


def test_struct_layouts_match_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    pairs = [("dg_hist2d_axis", _lib.Hist2dAxis), ("dg_hist2d_spec", _lib.Hist2dSpec)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))

    def spec(ax=None, **kw):
        s = JointSpec.zscore(2).struct()
        for k, v in kw.items():
            setattr(s, k, v)
        for (p, e), fields in (ax or {}).items():
            for k, v in fields.items():
                setattr(s.ax[p][e], k, v)
        return C.byref(s)
    ws, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    call = lambda fa, fb, s, w=ws, o=out: lib.dg_hist2d(fa, fb, s, w, o, None)
    assert lib.dg_hist2d_ws_bytes(f(), f(), spec()) > 0
    bad_specs = [spec(npairs=0), spec(npairs=9), spec(ax={(2, 0): dict(nbins=126), (2, 1): dict(nbins=126)}),   # 129 * 129 cells
                 spec(ax={(4, 0): dict(nbins=0)}), spec(ax={(4, 1): dict(lo=float("nan"))}), spec(ax={(4, 1): dict(lo=float("inf"))}),
                 spec(ax={(5, 0): dict(inv_w=0.0)}), spec(ax={(5, 0): dict(inv_w=-1.0)}), spec(ax={(5, 0): dict(inv_w=float("inf"))}),
                 spec(ax={(4, 0): dict(chan=4)}), spec(ax={(4, 0): dict(chan=-1)}), spec(ax={(4, 0): dict(src=2)}),
                 spec(speed_u=-1, speed_v=-1),                                    # speed and direction axes without a speed pair
                 spec(speed_u=2), spec(speed_v=-1),
                 spec(ax={(0, 0): dict(nbins=32)}), spec(nsec=38), spec(nsec=76), spec(nsec=0),
                 spec(calm=-1.0), spec(calm=float("inf")), spec(calm=float("nan"))]
    for i, s in enumerate(bad_specs):
        assert call(f(), f(), s) == -1, i
        assert lib.dg_hist2d_ws_bytes(f(), f(), s) == 0, i
    good = spec()
    for fa, fb in ((None, f()), (f(base=0), f()), (f(), f(base=0)), (f(C=9), f(C=9)), (f(T=0), f(T=0)), (f(P=0), f(P=0)),
                   (f(), None),                                                    # src 1 with b NULL
                   (f(), f(T=5)), (f(), f(C=3)), (f(), f(P=96))):
        assert call(fa, fb, good) == -1
        assert lib.dg_hist2d_ws_bytes(fa, fb, good) == 0
    assert call(f(), f(), None) == -1 and call(f(), f(), good, None) == -1 and call(f(), f(), good, ws, None) == -1
    assert call(f(dtype=7), f(), good) == -2 and call(f(), f(dtype=7), good) == -2
    single = JointSpec([(Axis("a", 0, 8, 0.0, 1.0), Axis("a", 1, 8, 0.0, 1.0))], 2).struct()
    assert lib.dg_hist2d_ws_bytes(f(), None, C.byref(single)) > 0
    x = np.zeros((2, 4), F32)
    b = np.zeros((7, 2, 4), np.int32)
    assert lib.dg_hist2d_host_bins(spec(npairs=0), x.ctypes.data, x.ctypes.data, 2, 4, b.ctypes.data) == -1
    assert lib.dg_hist2d_host_bins(good, None, x.ctypes.data, 2, 4, b.ctypes.data) == -1
    assert lib.dg_hist2d_host_bins(good, x.ctypes.data, None, 2, 4, b.ctypes.data) == -1
    assert lib.dg_hist2d_host_bins(good, x.ctypes.data, x.ctypes.data, 2, 4, None) == -1
    assert lib.dg_hist2d_host_bins(good, x.ctypes.data, x.ctypes.data, 2, 4, b.ctypes.data) == 0


# ------------------------------------------------------------------------------------------------- derived statistics
def make_joint(spec, tables, fields=1):
    flat = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1) for t in tables])
    assert len(flat) == spec.offsets()[-1]
    return Joint(spec, torch.from_numpy(flat), fields)


def ab_spec(bins=16, lo=-2.0, hi=2.0, npairs=1):
    return JointSpec([(Axis("a", 0, bins, lo, hi), Axis("b", 0, bins, lo, hi))] * npairs, 1, speed=None)


def test_identity_table_has_the_entropy_of_x_and_no_bias():
    spec = ab_spec()
    rng = np.random.default_rng(1)
    c = rng.integers(1, 1000, 16)
    t = np.zeros((19, 19), np.int64)
    t[np.arange(1, 17), np.arange(1, 17)] = c
    j = make_joint(spec, [t])
    p = c / c.sum()
    np.testing.assert_allclose(j.mutual_information(0), -(p * np.log(p)).sum(), rtol=1e-12)
    assert np.abs(j.conditional_bias(0)).max() <= 1e-12
    np.testing.assert_allclose(j.conditional_mean(0), spec.pairs[0][0].centres(), rtol=1e-12)
    assert np.abs(j.conditional_std(0)).max() == 0.0
    w = spec.pairs[0][1].width()
    np.testing.assert_allclose(j.conditional_quantile(0, [0.25, 0.5, 1.0]),
                               (spec.pairs[0][1].centres() - w / 2)[:, None] + np.array([0.25, 0.5, 1.0])[None, :] * w, rtol=1e-12)
    mx, my = j.marginals(0)
    assert mx.tolist() == my.tolist() == [0] + c.tolist() + [0, 0]


def test_independent_table_has_no_mutual_information():
    spec = ab_spec()
    rng = np.random.default_rng(2)
    t = np.outer(rng.integers(0, 50, 19), rng.integers(0, 50, 19))
    t[-1, :] = 7                                                               # the NaN row and column are not counted
    t[:, -1] = 9
    assert abs(make_joint(spec, [t]).mutual_information(0)) <= 1e-12


def test_shift_by_k_bins_is_a_bias_of_k_widths_and_moments_match_numpy():
    spec = ab_spec()
    w = spec.pairs[0][0].width()
    for k in (1, 3, -2):
        t = np.zeros((19, 19), np.int64)
        rows = np.arange(4, 12)
        t[rows, rows + k] = 5 + rows
        b = make_joint(spec, [t]).conditional_bias(0)
        np.testing.assert_allclose(b[rows - 1], np.full(len(rows), k * w), rtol=1e-12)
        assert np.isnan(np.delete(b, rows - 1)).all()
    rng = np.random.default_rng(3)
    t = rng.integers(0, 30, (19, 19))
    j = make_joint(spec, [t])
    cen = spec.pairs[0][1].centres()
    for r in range(16):
        samples = np.repeat(cen, t[1 + r, 1:17])
        np.testing.assert_allclose(j.conditional_mean(0)[r], samples.mean(), rtol=1e-12)
        np.testing.assert_allclose(j.conditional_std(0)[r], samples.std(), rtol=1e-9)
        got = j.conditional_quantile(0, [0.1, 0.5, 0.9])[r]
        want = np.quantile(samples, [0.1, 0.5, 0.9], method="inverted_cdf")
        assert np.all(np.abs(got - want) <= w * (1 + 1e-9))
    with pytest.raises(ValueError, match="quantile"):
        j.conditional_quantile(0, 1.5)


def test_tv_and_js_distances():
    spec = ab_spec(npairs=3)
    rng = np.random.default_rng(4)
    a = rng.integers(0, 20, (19, 19))
    b = np.zeros((19, 19), np.int64)
    c = np.zeros((19, 19), np.int64)
    b[:9, :-1] = rng.integers(1, 20, (9, 18))
    c[9:-1, :-1] = rng.integers(1, 20, (9, 18))
    j = make_joint(spec, [a, b, c])
    assert j.tv_distance(0, 0) == 0.0 and j.js_divergence(0, 0) == 0.0
    assert j.tv_distance(1, 2) == pytest.approx(1.0, abs=1e-12) and j.js_divergence(1, 2) == pytest.approx(math.log(2), rel=1e-12)
    assert 0 < j.tv_distance(0, 1) < 1 and 0 < j.js_divergence(0, 1) <= math.log(2)
    assert j.tv_distance(0, 1) == pytest.approx(j.tv_distance(1, 0), rel=1e-12)
    other = make_joint(spec, [3 * a, b, c])                                     # a scaled table is the same distribution
    assert j.tv_distance(0, 0, other) == pytest.approx(0.0, abs=1e-15)
    P, Q = a[:-1, :-1] / a[:-1, :-1].sum(), b[:-1, :-1] / b[:-1, :-1].sum()
    assert j.tv_distance(0, 1) == pytest.approx(0.5 * np.abs(P - Q).sum(), rel=1e-12)
    with pytest.raises(ValueError, match="shape"):
        j.tv_distance(0, 0, make_joint(ab_spec(8), [np.zeros((11, 11))]))
    with pytest.raises(KeyError):
        j.table("nope")


def test_rose_and_direction_frequencies():
    spec = JointSpec([(Axis("a", "direction", 8), Axis("a", "speed", 5, 0.0, 10.0))], 2, names=["rose"])
    rng = np.random.default_rng(5)
    t = np.zeros((11, 8), np.int64)
    t[1:9, 1:6] = rng.integers(0, 40, (8, 5))
    t[0, 1] = 123                                                              # calm
    t[10, 7] = 55                                                              # NaN: not a finite point
    j = make_joint(spec, [t])
    calm, freq = j.rose("rose")
    n = t[:-1, :-1].sum()
    assert freq.shape == (8, 5) and calm == pytest.approx(123 / n, rel=1e-12)
    assert calm + freq.sum() == pytest.approx(1.0, rel=1e-12)
    np.testing.assert_allclose(freq, t[1:9, 1:6] / n, rtol=1e-12)
    d = j.direction_frequencies(0)
    np.testing.assert_allclose(d, t[1:9, :-1].sum(axis=1) / n, rtol=1e-12)
    assert calm + d.sum() == pytest.approx(1.0, rel=1e-12)
    assert spec.pairs[0][0].centres().tolist() == [0.0, 45.0, 90.0, 135.0, 180.0, 225.0, 270.0, 315.0]
    with pytest.raises(ValueError, match="direction"):
        make_joint(ab_spec(), [np.zeros((19, 19))]).rose(0)


# ------------------------------------------------------------------------------------------------- trainer hook, emulated
def joint_emu_ops():
    from oracle.emu_ops import EmuOps

    class JointEmuOps(EmuOps):
        """The emulated ops plus dg_hist2d's contract by the numpy restatement."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=t.shape[1] * t.shape[2])

        def hist2d_ws_bytes(self, fa, fb, spec):
            return 1

        def hist2d(self, fa, fb, s, counts):
            pl = lambda f: (f.t[..., :f.C].permute(3, 0, 1, 2) if f.nhwc else f.t[:, :f.C].permute(1, 0, 2, 3)
                            ).detach().float().cpu().numpy().reshape(f.C, -1)
            b = bins2_ref(view(s, fa.C), pl(fa), None if fb is None else pl(fb))
            o = 0
            for p in range(s.npairs):
                nx, ny = s.ax[p][0].nbins + 3, s.ax[p][1].nbins + 3
                counts[o:o + nx * ny] += torch.from_numpy(np.bincount(b[p, 0] * ny + b[p, 1], minlength=nx * ny))
                o += nx * ny

    return JointEmuOps("f32")


def _patch(setattr_):
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    setattr_(backend, "make_ops", lambda dtype, device: joint_emu_ops())
    setattr_(losses, "_ops", {})
    setattr_(joint, "_ops", {})


def _run_epoch(log_joint, dist=None, lo=0, step=1, batch=2, fs=False):
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.GAN.wasserstein_fs import WassersteinGANFS
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    torch.manual_seed(0)                                  # initial weights, the gradient penalty's alpha
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = (WassersteinGANFS if fs else WassersteinGAN)(G, C_, dist=dist)
    tr.log_joint = log_joint
    dl, tl = _loaders(lo, step, batch)
    tr.train(dl, tl, epochs=1)
    return tr


RVG = ["ch0", "ch1", "speed"]


def _check_summary(p, fields):
    assert {"pairs", "fields", "q", "calm", "direction_tv", "rose_tv", "uv_js", "real_vs_generated"} <= set(p)
    assert p["fields"] == fields and p["pairs"] == ["rose_real", "rose_fake", "uv_real", "uv_fake"] + RVG
    assert set(p["calm"]) == {"real", "fake"} and all(0 <= v <= 1 for v in p["calm"].values())
    assert 0 <= p["direction_tv"] <= 1 and 0 <= p["rose_tv"] <= 1 and 0 <= p["uv_js"] <= math.log(2) + 1e-12
    assert list(p["real_vs_generated"]) == RVG and p["q"] == [0.05, 0.5, 0.95, 0.99]
    for v in p["real_vs_generated"].values():
        assert v["mutual_information"] >= 0 and len(v["bias_at_q"]) == 4


def test_log_joint_off_leaves_the_summary_unchanged(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    assert WassersteinGAN.log_joint is False and WassersteinGAN.joint_spec is None and WassersteinGAN.joint_results is None
    off = _run_epoch(False).metrics_log[0]
    tr = _run_epoch(True)
    on = dict(tr.metrics_log[0])
    assert "joint" not in off
    d = on.pop("joint")
    assert json.dumps(on, sort_keys=True) == json.dumps(off, sort_keys=True)     # the hook adds a key and changes nothing else
    json.dumps(d)
    assert set(d) == {"train", "test"}
    _check_summary(d["train"], 2)
    _check_summary(d["test"], 4)
    from downgan_amd import synthetic
    coarse, fine = synthetic.tiles(6, 2, 16, seed=11)
    spec = JointSpec.zscore(2)
    res = tr.joint_results["test"]
    assert res.fields == 4 and res.spec == spec
    planar = lambda x: np.ascontiguousarray(x.transpose(1, 0, 2, 3)).reshape(2, -1)
    with torch.no_grad():
        fake = np.concatenate([tr.G(torch.from_numpy(coarse[a:a + 2])).float().numpy() for a in (2, 4)])
    np.testing.assert_array_equal(res.host(), tables_ref(spec, planar(fine[2:6]), planar(fake)))
    assert d["test"]["rose_tv"] == pytest.approx(res.tv_distance("rose_real", "rose_fake"), rel=1e-12)
    assert d["test"]["uv_js"] == pytest.approx(res.js_divergence("uv_real", "uv_fake"), rel=1e-12)
    assert d["test"]["real_vs_generated"]["ch1"]["mutual_information"] == pytest.approx(res.mutual_information("ch1"), rel=1e-12)
    # the marginals of the real-vs-generated table are the 1-D counts of either series
    b = bins2_ref(view(spec.struct(), 2), planar(fine[2:6]), planar(fake))
    mx, my = res.marginals("ch0")
    np.testing.assert_array_equal(mx, np.bincount(b[4, 0], minlength=99))
    np.testing.assert_array_equal(my, np.bincount(b[4, 1], minlength=99))


def test_log_joint_without_log_metrics(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    monkeypatch.setattr(WassersteinGAN, "log_metrics", False)
    s = _run_epoch(True).metrics_log[0]
    assert "train" not in s and s["joint"]["train"]["fields"] == 2 and s["joint"]["test"]["fields"] == 4


def test_frequency_separation_trainer_reports_joint(monkeypatch):
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    torch.set_num_threads(4)
    s = _run_epoch(True, fs=True).metrics_log[0]
    _check_summary(s["joint"]["train"], 2)
    _check_summary(s["joint"]["test"], 4)


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    import downgan_amd.config.hyperparams as hp
    _patch(setattr)
    hp.batch_size, hp.lr = 1, 0.0
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    tr = _run_epoch(True, dist=d, lo=rank, step=world, batch=1)
    torch.save({"summary": tr.metrics_log[0]["joint"], "tables": {k: v.host() for k, v in tr.joint_results.items()}},
               os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_tables(monkeypatch):
    """lr = 0 keeps G identical in both runs, so the generated fields are the same and only the reduction is tested."""
    import downgan_amd.config.hyperparams as hp
    _patch(monkeypatch.setattr)
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(hp, "lr", 0.0)
    torch.set_num_threads(4)
    tr = _run_epoch(True)
    ref, ref_t = tr.metrics_log[0]["joint"], tr.joint_results
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert json.dumps(r0["summary"], sort_keys=True) == json.dumps(r1["summary"], sort_keys=True)
    for part in ("train", "test"):
        np.testing.assert_array_equal(r0["tables"][part], ref_t[part].host())
        np.testing.assert_array_equal(r1["tables"][part], ref_t[part].host())
        assert json.dumps(r0["summary"][part], sort_keys=True) == json.dumps(ref[part], sort_keys=True)
