"""Field-deformation verification without a GPU: the integer numpy oracle (deform_ref) on fields with known answers (shifted
Gaussian blobs and thresholded smooth noise: the modal vector is the imposed shift, morphing lowers the squared error, a zero shift
gives d = 0), its tie rule and symmetry, the library's host reference (dg_deform_host, dg_deform_field_host, dg_deform_bound)
against the oracle byte for byte, the quantiser's edges, the derived scores of ``DeformResult`` on hand-made tables with every zero
denominator, spec and argument checks that fire before any library call, the ABI surface and struct layout, and the headroom
rules of ``Deformation`` (drain, chunks, limb all-reduce over 2 gloo ranks) on emulated ops (a test-local op class adds a numpy
``deform``).  Every comparison of sums and fields is equality of integers or bytes."""
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

from downgan_amd import _lib, deform, histograms
from downgan_amd.deform import Deformation, DeformResult, DeformSpec

from .deform_ref import F32, ORDER, deform_ref, ints, match_ref, max_disp, pyramid_ref, quantise_ref
from .test_gridstats_cpu import _no_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_all(spec, a, b):
    """(disp, scalars, field, morphed) of the library's host reference over the field pairs of a, b float32 [T, C, H, W]."""
    T, Cn, H, W = a.shape
    side = 2 * spec.D + 1
    disp, scal = np.zeros((spec.nout, 2, side, side), np.int64), np.zeros((spec.nout, 2, 5), np.int64)
    field, mor = np.full((T, spec.nout, 2, 2, H, W), -777, np.int16), np.full((T, spec.nout, 2, H, W), 99, np.uint8)
    s, lib = spec.struct(), _lib.lib()
    for t in range(T):
        xa, xb = np.ascontiguousarray(a[t], dtype=F32), np.ascontiguousarray(b[t], dtype=F32)
        _lib.check(lib.dg_deform_host(C.byref(s), xa.ctypes.data, xb.ctypes.data, Cn, H, W, disp.ctypes.data, scal.ctypes.data), "dg_deform_host")
        _lib.check(lib.dg_deform_field_host(C.byref(s), xa.ctypes.data, xb.ctypes.data, Cn, H, W, field[t].ctypes.data, mor[t].ctypes.data),
                   "dg_deform_field_host")
    return disp, scal, field, mor


def same(got, want, what):
    assert got[2].tobytes() == want[2].tobytes(), (what, "field", np.argwhere(got[2] != want[2])[:5].tolist())
    assert got[3].tobytes() == want[3].tobytes(), (what, "morphed")
    assert ints(got[0]) == ints(want[0]) and ints(got[1]) == ints(want[1]), (what, "sums")


def one_channel(F, lo=0.1, step=1 / 128):
    return DeformSpec(1, speed=None, lo=lo, step=step, levels=F)


def result_of(spec, want, H, W, T=1):
    return DeformResult(spec, H, W, want[0], want[1], T)


# ------------------------------------------------------------------------------------------------- the oracle: known answers
def blobs(H, W, centres, shift=(0, 0), sigma=4.0):
    """Gaussian blobs at ``centres`` moved by ``shift``, float32 [1, 1, H, W]."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    f = np.zeros((H, W))
    for k, (cy, cx) in enumerate(centres):
        s = sigma * (1 + 0.3 * k)
        f += (1.0 + 0.5 * k) * np.exp(-((y - cy - shift[0]) ** 2 + (x - cx - shift[1]) ** 2) / (2 * s * s))
    return f.astype(F32)[None, None]


def smooth(rng, shape, passes=6):
    x = rng.standard_normal(shape)
    for ax in (-2, -1):
        for _ in range(passes):
            x = (np.roll(x, 1, axis=ax) + x + np.roll(x, -1, axis=ax)) / 3.0
    return (x / x.std()).astype(F32)


def noise_pair(rng, H, W, shift, T=1, Cn=1):
    """Thresholded smooth noise and the same moved by ``shift`` (cut from a larger field: nothing wraps around)."""
    big = smooth(rng, (T, Cn, H + 64, W + 64), passes=10)
    big = np.where(big > 0.3, big, 0).astype(F32)
    a = big[..., 32:32 + H, 32:32 + W]
    b = big[..., 32 - shift[0]:32 - shift[0] + H, 32 - shift[1]:32 - shift[1] + W]
    return a.copy(), b.copy()


BLOB_CASES = [(1, (2, -3)), (1, (-6, 6)), (2, (5, 4)), (2, (-6, 7)), (3, (-9, 12))]
NOISE_CASES = [(1, (2, -3)), (1, (-6, 6)), (2, (5, 4)), (2, (-6, 7)), (3, (11, 9)), (3, (-9, 12))]


def known_pair(kind, F, shift):
    if kind == "blob":
        centres = [(20, 22), (30, 36)] if F < 3 else [(24, 28)]
        return one_channel(F), blobs(48, 56, centres), blobs(48, 56, centres, shift=shift)
    rng = np.random.default_rng(F * 100 + shift[0] * 7 + shift[1])
    return (one_channel(F, lo=0.3, step=1 / 64),) + noise_pair(rng, 64, 80, shift)


@pytest.mark.parametrize("kind,F,shift", [("blob", F, s) for F, s in BLOB_CASES] + [("noise", F, s) for F, s in NOISE_CASES])
def test_a_shifted_field_is_found_and_morphing_lowers_the_error(kind, F, shift):
    spec, a, b = known_pair(kind, F, shift)
    H, W = a.shape[2:]
    want = deform_ref(spec, a, b)
    r = result_of(spec, want, H, W)
    # b[p] = a[p - shift]: the target a finds its source at p + shift, the target b at p - shift
    assert r.modal_vector()[0].tolist() == [[float(shift[0]), float(shift[1])], [float(-shift[0]), float(-shift[1])]]
    n_t, n_e, sse_m, sse_r, en = (r.scalar(k)[0] for k in deform.SCALARS)
    for d in range(2):
        assert 0 < sse_m[d] < sse_r[d] and 0 < n_t[d] <= n_e[d] and en[d] > 0
        assert int(want[0][0, d].sum()) == n_t[d]                          # the table counts the target's non-empty pixels
    assert sse_r[0] == sse_r[1] and 0.0 < r.explained().min() and r.explained().max() < 1.0
    assert int(np.abs(want[2]).max()) <= max_disp(F)
    same(host_all(spec, a, b), want, f"{kind} F={F} {shift}")              # and the host reference agrees byte for byte


@pytest.mark.parametrize("kind,F", [("blob", 1), ("blob", 3), ("noise", 2), ("noise", 3)])
def test_a_zero_shift_gives_no_displacement_and_no_error(kind, F):
    spec, a, b = known_pair(kind, F, (0, 0))
    assert np.array_equal(a, b)
    want = deform_ref(spec, a, b)
    assert not want[2].any() and np.array_equal(want[3][:, :, 0], want[3][:, :, 1])
    r = result_of(spec, want, *a.shape[2:])
    assert ints(r.scalar("sse_morphed")) == [0, 0] == ints(r.scalar("sse_raw")) and ints(r.scalar("n_target")) == ints(r.scalar("n_either"))
    D = spec.D
    assert int(want[0][0, 0, D, D]) == int(r.scalar("n_target")[0, 0]) > 0 and r.dis().tolist() == [[0.0, 0.0]]
    same(host_all(spec, a, b), want, "zero shift")


def test_the_morphed_field_is_the_source_read_through_the_displacement():
    spec, a, b = known_pair("noise", 2, (5, 4))
    _, _, field, mor = deform_ref(spec, a, b)
    q = [quantise_ref(spec, x)[0, 0] for x in (a, b)]
    H, W = q[0].shape
    for d in range(2):
        src = q[1 - d]
        for y in range(0, H, 3):
            for x in range(0, W, 3):
                sy, sx = y + int(field[0, 0, d, 0, y, x]), x + int(field[0, 0, d, 1, y, x])
                assert int(mor[0, 0, d, y, x]) == (int(src[sy, sx]) if 0 <= sy < H and 0 <= sx < W else 0)


def test_the_oracle_against_explicit_loops_on_a_tiny_grid():
    """The shifted-view oracle against the definition written with loops and a dictionary lookup: 7 x 9, F = 2."""
    rng = np.random.default_rng(5)
    q = [rng.integers(0, 256, (7, 9)) * (rng.random((7, 9)) < 0.6) for _ in range(2)]
    F = 2
    pyr = [pyramid_ref(np.asarray(x, np.int64)[None], F) for x in q]
    dy, dx = match_ref(pyr[0], pyr[1], F)

    def at(a, y, x):
        return int(a[y, x]) if 0 <= y < a.shape[0] and 0 <= x < a.shape[1] else 0
    par = None
    for l in range(F, -1, -1):
        X, Y = pyr[0][l][0], pyr[1][l][0]
        h, w = X.shape
        assert (h, w) == (-(-7 // 2 ** l), -(-9 // 2 ** l))
        init = np.zeros((2, h, w), np.int64) if par is None else np.stack([2 * par[:, y >> 1, x >> 1] for y in range(h) for x in range(w)], 1).reshape(2, h, w)
        yp = np.array([[at(Y, y + init[0, y, x], x + init[1, y, x]) for x in range(w)] for y in range(h)])
        cur = np.zeros((2, h, w), np.int64)
        for y in range(h):
            for x in range(w):
                costs = [sum((at(X, y + wy, x + wx) - at(yp, y + wy + sy, x + wx + sx)) ** 2 for wy in range(-2, 3) for wx in range(-2, 3))
                         for sy, sx in ORDER]
                sy, sx = ORDER[costs.index(min(costs))]                    # index(): the first of equal costs
                cur[:, y, x] = sy + at(init[0], y + sy, x + sx), sx + at(init[1], y + sy, x + sx)
        par = cur
    assert np.array_equal(par[0], dy[0]) and np.array_equal(par[1], dx[0])
    assert ORDER[0] == (0, 0) and ORDER[1:5] == [(-1, 0), (0, -1), (0, 1), (1, 0)] and ORDER[-1] == (2, 2) and len(set(ORDER)) == 25


# ------------------------------------------------------------------------------------------------- ties and symmetry
@pytest.mark.parametrize("F", [1, 2, 3, 4])
def test_ties_choose_the_zero_shift(F):
    H, W = 21, 18
    spec = one_channel(F, lo=0.0, step=1 / 8)
    zero, full = np.full((1, 1, H, W), -1.0, F32), np.full((1, 1, H, W), 1e6, F32)
    rng = np.random.default_rng(F)
    some = np.where(smooth(rng, (1, 1, H, W)) > 0, F32(3.0), F32(-1.0)).astype(F32)
    for a, b, what in ((zero, zero, "both empty"), (full, full, "both saturated"), (some, zero, "empty source"), (zero, some, "empty target")):
        want = deform_ref(spec, a, b)
        got = host_all(spec, a, b)
        same(got, want, what)
        if what in ("both empty", "both saturated"):
            assert not want[2].any(), what
        else:
            d = 0 if what == "empty source" else 1                          # the direction whose source is empty never moves
            assert not want[2][:, :, d].any() and not want[3][:, :, d].any(), what
    both = deform_ref(spec, zero, zero)
    assert not both[0].sum() and ints(both[1]) == [0] * 10
    sat = result_of(spec, deform_ref(spec, full, full), H, W)
    assert ints(sat.scalar("n_target")) == [H * W] * 2 and ints(sat.scalar("energy")) == [255 * 255 * H * W] * 2
    assert ints(sat.scalar("sse_morphed")) == [0, 0]


def test_swapping_the_sides_swaps_the_directions():
    rng = np.random.default_rng(3)
    spec = DeformSpec(2, scale=[1.5, 0.8], offset=[0.2, -0.1], speed=(1, 0), lo=[0.3, 0.1, 0.6], step=[1 / 64, 1 / 128, 1 / 32], levels=2)
    a, b = noise_pair(rng, 23, 31, (3, -2), T=2, Cn=2)
    p, q = deform_ref(spec, a, b), deform_ref(spec, b, a)
    assert ints(q[0][:, ::-1]) == ints(p[0]) and ints(q[1][:, ::-1]) == ints(p[1])
    assert np.array_equal(q[2][:, :, ::-1], p[2]) and np.array_equal(q[3][:, :, ::-1], p[3])
    hp, hq = host_all(spec, a, b), host_all(spec, b, a)
    same(hp, p, "a, b")
    same(hq, q, "b, a")


# ------------------------------------------------------------------------------------------------- the host reference
@pytest.mark.parametrize("grid", [(1, 1), (1, 9), (6, 1), (5, 13), (16, 16), (37, 53), (33, 64)])
def test_host_reference_equals_the_oracle(grid):
    H, W = grid
    rng = np.random.default_rng(H * 100 + W)
    for F in (1, 2, 3, 4):
        for Cn, spec in ((1, one_channel(F, lo=0.2, step=1 / 32)),
                         (2, DeformSpec(2, scale=[3.0, 2.5], offset=[-1.5, 4.0], speed=(1, 0), lo=[0.0, 4.5, 5.0], step=[1 / 16, 1 / 32, 1 / 8], levels=F))):
            if Cn == 2 and F % 2:
                continue
            a = smooth(rng, (2, Cn, H, W)) if H * W > 1 else rng.standard_normal((2, Cn, H, W)).astype(F32)
            b = (np.roll(a, (min(2, H - 1), -min(3, W - 1)), axis=(2, 3)) + 0.05 * rng.standard_normal(a.shape)).astype(F32)
            want = deform_ref(spec, a, b)
            same(host_all(spec, a, b), want, f"{grid} F={F} C={Cn}")
            if H * W > 500:                                                # not degenerate
                assert all(int(v) > 0 for v in want[1][:, :, 0].reshape(-1)) and want[2].any()


def test_saturated_plateaus_reach_the_largest_costs():
    """Whole windows at q = 255 beside empty ground at F = 4: level-4 differences of 255 * 256, costs beyond 2^32."""
    H, W, F = 70, 45, 4
    spec = one_channel(F, lo=0.0, step=1 / 8)
    a = np.full((1, 1, H, W), -1.0, F32)
    a[..., :40, :24] = 1e4
    b = np.roll(a, (9, 5), axis=(2, 3)).copy()
    want = deform_ref(spec, a, b)
    pa, pb = (pyramid_ref(quantise_ref(spec, x)[0], F) for x in (a, b))
    assert int(pa[4].max()) == 255 * 256 and 25 * int(np.abs(pa[4] - pb[4]).max()) ** 2 > 1 << 32
    same(host_all(spec, a, b), want, "saturated")
    assert want[2].any() and set(np.unique(want[3]).tolist()) == {0, 255}   # (a featureless plateau has no one right vector)


def test_the_quantiser_edges():
    lo, step = F32(0.25), F32(1 / 64)
    below, above = np.nextafter(lo, F32(-1)), np.nextafter(lo, F32(1))
    vals = [lo, below, above, lo + 253 * step, lo + F32(253.5) * step, lo + 254 * step, np.nextafter(F32(lo + 254 * step), F32(0)), 1e30, 3e38,
            np.nan, np.inf, -np.inf, -3e38, 0.0, -0.0, lo + step, np.nextafter(F32(lo + step), F32(0))]
    want = [1, 0, 1, 254, 254, 255, 254, 255, 255, 0, 255, 0, 0, 0, 0, 2, 1]
    x = np.array(vals, F32).reshape(1, 1, 1, -1)
    spec = DeformSpec(1, speed=None, lo=float(lo), step=float(step), levels=1)
    assert quantise_ref(spec, x).reshape(-1).tolist() == want
    # identical fields never move, so the morphed field of the host reference is the quantised field itself
    got = host_all(spec, x, x)
    assert not got[2].any() and got[3][0, 0, 0].reshape(-1).tolist() == want == got[3][0, 0, 1].reshape(-1).tolist()
    # the speed channel and an affine transform in front of the quantiser
    sp = DeformSpec(2, scale=[2.0, 0.5], offset=[1.0, -1.0], speed=(0, 1), lo=[1.0, -1.0, 5.0], step=[0.5, 0.25, 1.0], levels=1)
    y = np.array([[3.0, 0.0, np.nan, -2.0], [8.0, 2.0, 1.0, np.inf]], F32).reshape(1, 2, 1, 4)
    # y0 = 7, 1, nan, -3; y1 = 3, 0, -0.5, inf; speed = sqrt(58), 1, nan, inf
    assert quantise_ref(sp, y)[0].reshape(3, 4).tolist() == [[13, 1, 0, 0], [17, 5, 3, 255], [3, 0, 0, 255]]
    assert host_all(sp, y, y)[3][0, :, 0].reshape(3, 4).tolist() == [[13, 1, 0, 0], [17, 5, 3, 255], [3, 0, 0, 255]]


def test_bound_is_its_formula():
    lib = _lib.lib()
    for H, W in [(1, 1), (5, 3), (128, 128), (2048, 2048), (1, 2048)]:
        assert lib.dg_deform_bound(H, W) == deform.bound(H, W) == 65025 * H * W
    for H, W in [(0, 5), (5, 0), (2049, 5), (5, 2049), (-1, 4)]:
        assert lib.dg_deform_bound(H, W) == 0
    assert [max_disp(F) for F in (1, 2, 3, 4)] == [deform.max_displacement(F) for F in (1, 2, 3, 4)] == [6, 14, 30, 62]


# ------------------------------------------------------------------------------------------------- the scores
def hand_result(tables, scalars, F=1, step=0.5, nout=1):
    spec = DeformSpec(nout, speed=None, lo=0.0, step=step, levels=F)
    D = spec.D
    disp = np.zeros((nout, 2, 2 * D + 1, 2 * D + 1), dtype=object)
    for (j, d), entries in tables.items():
        for (dy, dx), c in entries.items():
            disp[j, d, dy + D, dx + D] = c
    return DeformResult(spec, 10, 10, disp, np.array(scalars, dtype=object).reshape(nout, 2, 5), 2)


def test_scores_of_hand_made_tables():
    # direction 0: 6 pixels at (3, 4) (length 5), 2 at (0, 0), 2 at (0, -1); direction 1: 4 pixels at (-3, -4)
    r = hand_result({(0, 0): {(3, 4): 6, (0, 0): 2, (0, -1): 2}, (0, 1): {(-3, -4): 4}},
                    [[10, 16, 64, 256, 1000], [4, 4, 36, 256, 360]])
    assert r.dis().tolist() == [[(6 * 5 + 2) / 10, 5.0]]
    assert r.mean_vector().tolist() == [[[1.8, 2.2], [-3.0, -4.0]]]
    assert r.modal_vector().tolist() == [[[3.0, 4.0], [-3.0, -4.0]]]
    assert r.displacement_quantile(0.0).tolist() == [[0.0, 5.0]] and r.displacement_quantile(0.2).tolist() == [[0.0, 5.0]]
    assert r.displacement_quantile(0.3).tolist() == [[1.0, 5.0]] and r.displacement_quantile(0.5).tolist() == [[5.0, 5.0]]
    assert r.displacement_quantile(1.0).tolist() == [[5.0, 5.0]]
    # inv_step = 2: amp = sqrt(64 / 16) / 2 = 1, amp_raw = sqrt(256 / 16) / 2 = 2; direction 1: sqrt(36 / 4) / 2, sqrt(256 / 4) / 2
    assert r.amp().tolist() == [[1.0, 1.5]] and r.amp_raw().tolist() == [[2.0, 4.0]]
    assert r.explained().tolist() == [[0.75, 1 - 36 / 256]]
    assert r.dis_combined().tolist() == [(10 * 3.2 + 4 * 5.0) / 14] and r.amp_combined().tolist() == [(16 * 1.0 + 4 * 1.5) / 20]
    assert r.i0().tolist() == [5.0]                                       # sqrt(1000 / 10) / 2
    assert r.das().tolist() == [r.dis_combined()[0] / 6 + r.amp_combined()[0] / 5.0]
    assert r.das(d_max=10, i0=2.0).tolist() == [r.dis_combined()[0] / 10 + r.amp_combined()[0] / 2.0]
    rose = r.rose()
    assert rose.dtype == np.int64 and rose.shape == (1, 2, 13, 13) and rose[0, 0, 9, 10] == 6 and rose.sum() == 14
    s = r.summary()
    assert json.loads(json.dumps(s)) == s
    assert s["rose"][0][0] == [[0, -1, 2], [0, 0, 2], [3, 4, 6]] and s["scalars"]["sse_raw"] == [[256, 256]] and s["das"] == r.das().tolist()
    assert s["max_displacement"] == 6 and s["fields"] == 2 and s["median_displacement"] == [[5.0, 5.0]]
    # equal counts: the shorter vector is the mode
    tie = hand_result({(0, 0): {(3, 4): 2, (1, 0): 2, (0, 2): 2}}, [[6, 6, 0, 0, 6], [0, 0, 0, 0, 0]])
    assert tie.modal_vector()[0, 0].tolist() == [1.0, 0.0]
    # integers beyond int64 stay exact
    big = hand_result({(0, 0): {(0, 1): 1 << 70}}, [[1 << 70, 1 << 70, 1 << 80, 1 << 82, 1 << 90], [0] * 5])
    assert big.rose().dtype == object and big.sums()[0][0, 0, 6, 7] == 1 << 70 and big.dis()[0, 0] == 1.0 and big.explained()[0, 0] == 0.75
    assert big.summary()["scalars"]["energy"][0][0] == 1 << 90


def test_every_zero_denominator_is_nan_and_none():
    empty = hand_result({}, [[0] * 5, [0] * 5])
    for v in (empty.dis(), empty.mean_vector(), empty.modal_vector(), empty.displacement_quantile(0.5), empty.amp(), empty.amp_raw(),
              empty.explained(), empty.dis_combined(), empty.amp_combined(), empty.i0(), empty.das()):
        assert np.isnan(v).all()
    s = empty.summary()
    assert json.loads(json.dumps(s)) == s and s["das"] == [None] and s["dis"] == [[None, None]] and s["rose"] == [[[], []]]
    assert s["modal_vector"] == [[[None, None], [None, None]]] and s["explained"] == [[None, None]]
    # one direction empty: its scores are NaN, the combined ones use the other
    half = hand_result({(0, 1): {(1, 0): 3}}, [[0, 0, 0, 0, 0], [3, 4, 16, 64, 48]])
    assert np.isnan(half.dis()[0, 0]) and half.dis()[0, 1] == 1.0 and half.dis_combined().tolist() == [1.0]
    assert np.isnan(half.amp()[0, 0]) and half.amp()[0, 1] == 1.0 and half.amp_combined().tolist() == [1.0]
    assert np.isnan(half.i0()).all() and np.isnan(half.das()).all() and half.das(i0=2.0).tolist() == [1 / 6 + 0.5]
    assert np.isnan(half.das(d_max=0, i0=2.0)).all()
    # sse_raw = 0 with pixels: explained undefined, amp 0
    flat = hand_result({(0, 0): {(0, 0): 5}, (0, 1): {(0, 0): 5}}, [[5, 5, 0, 0, 20], [5, 5, 0, 0, 20]])
    assert np.isnan(flat.explained()).all() and flat.amp().tolist() == [[0.0, 0.0]] and flat.das().tolist() == [0.0]
    with pytest.raises(ValueError, match="quantile"):
        flat.displacement_quantile(1.5)


# ------------------------------------------------------------------------------------------------- spec and argument checks
@pytest.mark.parametrize("kw,match", [
    (dict(C=0), "input channels"), (dict(C=9), "input channels"), (dict(C=2, speed=(0, 2)), "speed"), (dict(C=2, speed=(0,)), "speed"),
    (dict(C=2, scale=[1.0]), "one value per input channel"), (dict(C=2, lo=[0.0, 1.0]), "one value per output channel"),
    (dict(C=2, step=[1.0, 1.0]), "one value per output channel"), (dict(C=1, speed=None, step=0.0), "step must be > 0"),
    (dict(C=1, speed=None, step=-1.0), "step must be > 0"), (dict(C=1, speed=None, step=1e-45), "inverse"),
    (dict(C=1, speed=None, levels=0), "levels"), (dict(C=1, speed=None, levels=5), "levels"), (dict(C=1, speed=None, levels=2.0), "levels"),
    (dict(C=2, names=["a"]), "names"),
])
def test_spec_is_checked(monkeypatch, kw, match):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match=match):
        DeformSpec(**kw)


def test_constructors():
    z = DeformSpec.zscore(2)
    assert (z.C, z.nout, z.speed, z.levels, z.D, z.names) == (2, 3, (0, 1), 3, 30, ["ch0", "ch1", "speed"])
    assert z.lo.tolist() == [0.5] * 3 and z.inv_step.tolist() == [64.0] * 3
    one = DeformSpec.zscore(1, lo=1.0, step=0.25, levels=4)
    assert one.speed is None and one.nout == 1 and one.D == 62 and one.inv_step.tolist() == [4.0]
    stats = {"u10": (0.5, 3.0), "v10": (-0.25, 2.0), "t2m": (280.0, 10.0)}
    p = DeformSpec.physical(stats, ["t2m", "u10", "v10"], lo=[285.0, 2.0, 2.0, 5.0], step=[0.1, 0.1, 0.1, 0.125], levels=2)
    assert p.speed == (1, 2) and p.names == ["t2m", "u10", "v10", "speed"]
    assert p.scale.tolist() == [10.0, 3.0, 2.0] and p.offset.tolist() == [280.0, 0.5, -0.25]
    assert p == DeformSpec.physical(stats, ["t2m", "u10", "v10"], lo=[285.0, 2.0, 2.0, 5.0], step=[0.1, 0.1, 0.1, 0.125], levels=2) and p != z
    assert p != DeformSpec.physical(stats, ["t2m", "u10", "v10"], lo=[285.0, 2.0, 2.0, 5.0], step=[0.1, 0.1, 0.1, 0.125], levels=3)
    assert p.inv_step[0] == F32(1) / F32(0.1) and p.inv_step[3] == 8.0      # the inverse of the fp32 step, rounded once
    s = p.struct()
    assert (s.speed_u, s.speed_v, s.levels) == (1, 2, 2) and s.lo[3] == 5.0 and s.inv_step[3] == 8.0 and s.scale[2] == 2.0 and s.offset[0] == 280.0
    n = DeformSpec(2, speed=None).struct()
    assert (n.speed_u, n.speed_v, n.levels) == (-1, -1, 3)


@pytest.mark.parametrize("x,kw,err,match", [
    (torch.zeros(2, 3, 8, 8), {}, ValueError, "C = 2"),
    (torch.zeros(2, 9, 8, 8), {}, ValueError, "C <="),
    (torch.zeros(2, 8, 8, 4), {"nhwc": True, "channels": 5}, ValueError, "channels"),
    (torch.zeros(2, 2, 8, 8, dtype=torch.float64), {}, TypeError, "fp32 or bf16"),
    (np.zeros((2, 2, 8, 8), np.float32), {}, TypeError, "tensor"),
    (torch.zeros(2, 8, 8), {}, ValueError, "shape"),
    (torch.zeros(0, 2, 8, 8), {}, ValueError, "at least one"),
    (torch.zeros(2, 2, 8, 4), {}, ValueError, "8 x 8 grid"),
])
def test_arguments_are_checked_before_any_library_call(monkeypatch, x, kw, err, match):
    _no_library(monkeypatch)
    spec = DeformSpec.zscore(2)
    good = torch.zeros(2, 2, 8, 8)
    acc = Deformation(spec, 8, 8, device="cpu")
    with pytest.raises(err, match=match):
        acc.add(good, x, nhwc=(False, kw.get("nhwc", False)), channels=kw.get("channels"))
    with pytest.raises(err, match=match):
        acc.add(x, good, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))
    if "grid" not in match:                                               # the one-shot forms take the grid from the fields
        for fn in (deform.deformation, deform.displacement_field):
            with pytest.raises(err, match=match):
                fn(x, good, spec=spec, nhwc=(kw.get("nhwc", False), False), channels=kw.get("channels"))


def test_accumulator_checks(monkeypatch):
    _no_library(monkeypatch)
    spec = DeformSpec.zscore(2)
    x = torch.zeros(2, 2, 8, 8)
    acc = Deformation(spec, 8, 8, device="cpu")
    for n in (0, 3, -1):
        with pytest.raises(ValueError, match="n_valid"):
            acc.add(x, x, n_valid=n)
    with pytest.raises(ValueError, match="differ in length"):
        acc.add(x, torch.zeros(3, 2, 8, 8))
    with pytest.raises(TypeError, match="DeformSpec"):
        Deformation(histograms.HistSpec.zscore(2), 8, 8, device="cpu")
    for fn in (deform.deformation, deform.displacement_field):
        with pytest.raises(TypeError, match="DeformSpec"):
            fn(x, x, spec=histograms.HistSpec.zscore(2))
    for H, W in ((0, 8), (8, 2049)):
        with pytest.raises(ValueError, match="grid"):
            Deformation(spec, H, W, device="cpu")
    assert acc.fields == 0 and acc._dev_disp.shape == (3, 2, 61 * 61) and acc._dev_scalars.shape == (3, 2, 5)
    assert acc._dev_disp.dtype == acc._dev_scalars.dtype == torch.int64 and acc.result().fields == 0


# ------------------------------------------------------------------------------------------------- the ABI
SYMBOLS = ("dg_deform_bound", "dg_deform_ws_bytes", "dg_deform", "dg_deform_field", "dg_deform_host", "dg_deform_field_host")


def test_header_declares_and_library_exports_the_deform_abi():
    src = open(os.path.join(ROOT, "include", "downgan_hip.h")).read()
    assert re.search(r"#define DG_DEFORM_MAX_LEVELS 4\b", src) and re.search(r"#define DG_DEFORM_MAX_SIDE 2048\b", src)
    assert re.search(r"#define DG_DEFORM_SCALARS 5\b", src) and "Field-deformation verification (csrc/deform.hip)" in src
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", src), sym
        assert sym in _lib.EXPORTS and hasattr(_lib.lib(), sym)
    assert (_lib.DEFORM_MAX_LEVELS, _lib.DEFORM_MAX_SIDE, _lib.DEFORM_SCALARS) == (deform.LEVELS_MAX, deform.SIDE_MAX, deform.NSCALARS) == (4, 2048, 5)
    assert len(deform.SCALARS) == 5 and "deform.hip" in open(os.path.join(ROOT, "downgan_amd", "csrc", "Makefile")).read()


def test_deform_spec_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.DeformSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof(dg_deform_spec));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_deform_spec, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_abi_rejects_bad_arguments_without_launching():
    """Every pointer is a made-up address: a call that passed the checks would fault instead of returning a status."""
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=4, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    good = DeformSpec.zscore(2).struct()

    def spec(**kw):
        s = DeformSpec.zscore(2).struct()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)
    ws, out = C.c_void_p(0x2000), C.c_void_p(0x3000)
    sums = lambda fa, fb, s, H=10, W=10, w=ws, o=out, o2=out: lib.dg_deform(fa, fb, H, W, s, w, o, o2, None)
    field = lambda fa, fb, s, H=10, W=10, w=ws, o=out, o2=None: lib.dg_deform_field(fa, fb, H, W, s, w, o, o2, None)
    g = C.byref(good)
    for call in (sums, field):
        assert call(f(base=0), f(), g) == -1 and call(f(), f(base=0), g) == -1 and call(None, f(), g) == -1 and call(f(), None, g) == -1
        assert call(f(C=9), f(C=9), g) == -1 and call(f(T=0), f(T=0), g) == -1 and call(f(ld_t=-1), f(), g) == -1
        assert call(f(), f(T=3), g) == -1 and call(f(), f(P=96), g) == -1 and call(f(C=3), f(C=2), g) == -1     # T / C / P differ
        assert call(f(), f(), g, H=10, W=9) == -1 and call(f(), f(), g, H=0, W=10) == -1                          # P != H * W
        assert call(f(P=2049), f(P=2049), g, H=1, W=2049) == -1 and call(f(P=2049), f(P=2049), g, H=2049, W=1) == -1
        assert call(f(), f(), None) == -1 and call(f(), f(), g, w=None) == -1 and call(f(), f(), g, o=None) == -1
        for bad in (dict(levels=0), dict(levels=5), dict(speed_u=2), dict(speed_v=-1), dict(scale=(1, float("inf"))),
                    dict(offset=(0, float("nan"))), dict(lo=(2, float("inf"))), dict(lo=(0, float("nan"))), dict(inv_step=(1, 0.0)),
                    dict(inv_step=(2, -1.0)), dict(inv_step=(0, float("inf"))), dict(inv_step=(0, float("nan")))):
            assert call(f(), f(), spec(**bad)) == -1, bad
            assert lib.dg_deform_ws_bytes(f(), 10, 10, spec(**bad)) == 0, bad
        assert call(f(C=1), f(C=1), g) == -1                             # speed channel 1 of a 1-channel field
        assert call(f(dtype=7), f(), g) == -2 and call(f(), f(dtype=7), g) == -2
    assert sums(f(), f(), g, o2=None) == -1
    # T * H * W <= 2^31: 512 fields of 2048 x 2048 are the most one call takes
    big = dict(P=2048 * 2048, ld_c=0, ld_t=0)
    assert lib.dg_deform_ws_bytes(f(T=512, **big), 2048, 2048, g) > 0
    assert lib.dg_deform_ws_bytes(f(T=513, **big), 2048, 2048, g) == 0 and sums(f(T=513, **big), f(T=513, **big), g, H=2048, W=2048) == -1
    # the workspace: per (t, j) two pyramids (1 + 2 (1/4 + 1/16 + 1/64) bytes a pixel) and two displacement sets (4 (1 + 1/4 + ..))
    m = dict(P=1 << 20, ld_c=1 << 20, ld_t=2 << 20)
    four = lib.dg_deform_ws_bytes(f(T=4, **m), 1024, 1024, g)
    per_plane = (1 << 20) * (1 + 2 * 21 / 64) + (1 << 20) * 4 * 85 / 64
    assert 4 * 3 * 2 * per_plane <= four <= 4 * 3 * 2 * per_plane + 4096
    assert lib.dg_deform_ws_bytes(f(C=9), 10, 10, g) == 0 and lib.dg_deform_ws_bytes(f(), 10, 9, g) == 0
    # the host references check their arguments too
    x = np.zeros((2, 4, 4), F32)
    o = np.zeros(3 * 2 * 61 * 61, np.int64)
    assert lib.dg_deform_host(g, x.ctypes.data, x.ctypes.data, 2, 4, 4, o.ctypes.data, None) == -1
    assert lib.dg_deform_host(g, None, x.ctypes.data, 2, 4, 4, o.ctypes.data, o.ctypes.data) == -1
    assert lib.dg_deform_host(spec(levels=0), x.ctypes.data, x.ctypes.data, 2, 4, 4, o.ctypes.data, o.ctypes.data) == -1
    assert lib.dg_deform_field_host(g, x.ctypes.data, x.ctypes.data, 2, 4, 4, None, None) == -1
    assert lib.dg_deform_field_host(g, x.ctypes.data, x.ctypes.data, 2, 0, 4, o.ctypes.data, None) == -1


# ------------------------------------------------------------------------------------------------- emulated ops
RECORD = []                  # (real, fake) float32 [T, C, H, W] of every emulated dg_deform call of this process


def deform_emu_ops():
    from oracle.emu_ops import EmuOps

    class DeformEmuOps(EmuOps):
        """The emulated ops plus dg_deform's contract in numpy (the oracle)."""

        @staticmethod
        def eof_fields(t, nhwc=False, channels=None):
            Cn = (t.shape[3] if channels is None else channels) if nhwc else t.shape[1]
            P = t.shape[1] * t.shape[2] if nhwc else t.shape[2] * t.shape[3]
            return types.SimpleNamespace(t=t, nhwc=nhwc, T=t.shape[0], C=Cn, P=P)

        def deform_ws_bytes(self, f, H, W, spec):
            return 1

        @staticmethod
        def _pair(fa, fb, s):
            def values(f):
                x = f.t[..., :f.C].permute(0, 3, 1, 2) if f.nhwc else f.t[:, :f.C]
                return x.detach().float().cpu().numpy().copy()
            speed = None if s.speed_u < 0 else (s.speed_u, s.speed_v)
            nout = fa.C + (speed is not None)
            spec = types.SimpleNamespace(nout=nout, levels=s.levels, speed=speed, scale=np.array(s.scale[:fa.C], F32),
                                         offset=np.array(s.offset[:fa.C], F32), lo=np.array(s.lo[:nout], F32),
                                         inv_step=np.array(s.inv_step[:nout], F32))
            return spec, values(fa), values(fb)

        def deform(self, fa, fb, H, W, s, disp, scalars):
            spec, a, b = self._pair(fa, fb, s)
            assert a.shape[2:] == (H, W) and fa.T * deform.bound(H, W) <= 1 << 62
            RECORD.append((a, b))
            d, sc, _, _ = deform_ref(spec, a, b)
            disp += torch.from_numpy(d.astype(np.int64)).reshape(disp.shape)
            scalars += torch.from_numpy(sc.astype(np.int64))

        def deform_field(self, fa, fb, H, W, s, field, morphed=None):
            spec, a, b = self._pair(fa, fb, s)
            _, _, f, m = deform_ref(spec, a, b)
            field.copy_(torch.from_numpy(f))
            if morphed is not None:
                morphed.copy_(torch.from_numpy(m))

    return DeformEmuOps("f32")


def _pairs(rng, sizes, H=8, W=8):
    out = []
    for n in sizes:
        a = smooth(rng, (n, 2, H, W), passes=2)
        out.append((torch.from_numpy(a), torch.from_numpy((np.roll(a, 1, axis=3) + 0.1 * rng.standard_normal(a.shape)).astype(F32))))
    return out


SMALL = dict(lo=0.1, step=1 / 64, levels=2)


def sums_of(r):
    return ints(r.sums()[0]) + ints(r.sums()[1])


def test_draining_and_chunking_leave_the_totals_unchanged(monkeypatch):
    rng = np.random.default_rng(6)
    spec = DeformSpec.zscore(2, **SMALL)
    batches = _pairs(rng, (2, 2, 6, 2, 2, 1))
    ops = deform_emu_ops()

    def run():
        acc = Deformation(spec, 8, 8, device="cpu", ops=ops)
        calls = len(RECORD)
        for a, b in batches:
            acc.add(a, b)
        return acc, acc.result(), [r[0].shape[0] for r in RECORD[calls:]]
    acc, plain, sizes = run()
    assert sizes == [2, 2, 6, 2, 2, 1] and acc.drains == 1               # one call per batch, drained once by result()
    mb = deform.bound(8, 8)
    assert acc._bound == mb == 65025 * 64
    monkeypatch.setattr(deform, "DRAIN_LIMIT", 4 * mb)                   # room for four fields on the device
    acc2, low, sizes2 = run()
    assert sizes2 == [2, 2, 4, 2, 2, 2, 1]                               # the batch of 6 is cut into 4 + 2
    assert acc2.drains >= 4                                              # ... and at least every second add drains first
    assert sums_of(low) == sums_of(plain) and low.fields == plain.fields == 15
    a, b = torch.cat([p[0] for p in batches]), torch.cat([p[1] for p in batches])
    want = deform_ref(spec, a.numpy(), b.numpy())
    assert sums_of(plain) == ints(want[0]) + ints(want[1]) and sum(ints(want[1][:, :, 0])) > 0
    monkeypatch.setattr(deform, "DRAIN_LIMIT", 1)                        # below one field's bound: one field per call
    acc3, one, sizes3 = run()
    assert sizes3 == [1] * 15 and sums_of(one) == sums_of(plain)
    # the workspace cap cuts a batch as well, and so does the pixel limit
    monkeypatch.setattr(deform, "DRAIN_LIMIT", 1 << 62)
    monkeypatch.setattr(ops, "deform_ws_bytes", lambda f, H, W, s: 100 * f.T)
    monkeypatch.setattr(deform, "WS_CAP", 350)                           # three fields per call
    acc5, capped, sizes5 = run()
    assert sizes5 == [2, 2, 3, 3, 2, 2, 1] and sums_of(capped) == sums_of(plain)
    monkeypatch.setattr(deform, "WS_CAP", 512 << 20)
    monkeypatch.setattr(deform, "PIXEL_LIMIT", 4 * 64)                   # four fields per call
    acc6, few, sizes6 = run()
    assert sizes6 == [2, 2, 4, 2, 2, 2, 1] and sums_of(few) == sums_of(plain)
    got = deform.displacement_field(a, b, spec=spec, ops=ops, morphed=True)
    assert got[0].numpy().tobytes() == want[2].tobytes() and got[1].numpy().tobytes() == want[3].tobytes()
    monkeypatch.setattr(deform, "PIXEL_LIMIT", 1 << 31)
    # n_valid: the padding fields are not read
    acc4 = Deformation(spec, 8, 8, device="cpu", ops=ops)
    junk = torch.full((3, 2, 8, 8), 9.0)
    for a_, b_ in batches:
        acc4.add(torch.cat([a_, junk[:2]]), torch.cat([b_, -junk[:2]]), n_valid=a_.shape[0])
    assert sums_of(acc4.result()) == sums_of(plain) and acc4.fields == 15
    # the one-shot forms, in NHWC with padded channels on one side
    nh = torch.full((15, 8, 8, 5), float("nan"))
    nh[..., :2] = b.permute(0, 2, 3, 1)
    once = deform.deformation(a, nh, spec=spec, nhwc=(False, True), channels=2, ops=ops)
    assert sums_of(once) == sums_of(plain) and once.summary() == plain.summary()
    f = deform.displacement_field(torch.cat([a, junk]), torch.cat([nh, nh[:3]]), spec=spec, nhwc=(False, True), channels=2, n_valid=15, ops=ops)
    assert f.dtype == torch.int16 and f.shape == (15, 3, 2, 2, 8, 8) and f.numpy().tobytes() == want[2].tobytes()


def _rank_pairs(rank, world):
    rng = np.random.default_rng(21)
    (a, b), = _pairs(rng, (6,), H=12, W=20)
    return a[rank::world], b[rank::world]


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from downgan_amd.dist import Dist
    d = Dist("gloo")
    a, b = _rank_pairs(rank, world)
    acc = Deformation(DeformSpec.zscore(2, **SMALL), 12, 20, device="cpu", ops=deform_emu_ops())
    acc._disp[0] += (1 << 70) + rank                                     # a total beyond int64 survives the limb all-reduce
    acc._scalars[-1] += (1 << 65) + 2 * rank
    res = acc.add(a, b).reduce_(d).result()
    torch.save({"sums": sums_of(res), "fields": res.fields, "summary": res.summary()}, os.path.join(outdir, f"r{rank}.pt"))
    d.barrier()


def test_two_gloo_ranks_give_the_single_process_sums():
    a, b = _rank_pairs(0, 1)
    spec = DeformSpec.zscore(2, **SMALL)
    ref = deform.deformation(a, b, spec=spec, ops=deform_emu_ops())
    want = sums_of(ref)
    w = deform_ref(spec, a.numpy(), b.numpy())
    assert want == ints(w[0]) + ints(w[1])
    want[0] += (2 << 70) + 1
    want[-1] += (2 << 65) + 2
    with tempfile.TemporaryDirectory() as d:
        from downgan_amd.dist import free_port
        mp.spawn(_worker, args=(2, free_port(), d), nprocs=2, join=True)
        r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0 == r1 and r0["sums"] == want and r0["fields"] == 6


def test_no_trainer_hook_yet():
    """The accumulator follows the protocol of the trainer's diagnostics (add / reduce_ / result -> summary), but this module is
    not wired into the trainer: the hook table and the metric sinks end where they ended."""
    from downgan_amd.engine import METRIC_SINKS
    from downgan_amd.GAN.wasserstein import HOOKS
    assert HOOKS[-1].key == "intensity_scale" and METRIC_SINKS[-1][0] == "intensity_scale"
    assert not any("deform" in h.key for h in HOOKS)
    assert all(callable(getattr(Deformation, m)) for m in ("add", "reduce_", "result")) and callable(DeformResult.summary)
