"""Field-deformation verification on the GPU (csrc/deform.hip) against the integer numpy oracle of deform_ref: the displacement
fields and the morphed fields byte for byte, and every sum, on the grids where each code path can go wrong (one pixel, a row
band wider than two tiles, ragged against the tile and against 2^F, exactly one tile wide, more than one tile each way), for
F = 1 .. 4 (both cost widths, the 62 KB table), T = 1 and 3, one channel and two channels with their speed, NCHW fp32 and padded
NHWC bf16, saturated windows (the largest costs), special values, accumulation, determinism, n_valid and chunking.  Every
comparison is equality of integers or bytes."""
import numpy as np
import pytest
import torch

from downgan_amd import deform
from downgan_amd.deform import Deformation, DeformSpec
from downgan_amd.histograms import _default_ops, _descriptor, _fields

from .deform_ref import F32, deform_ref, ints, max_disp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = [(1, 1), (5, 130), (37, 53), (64, 64), (130, 67)]


def smooth(rng, shape, passes=6):
    """Periodic smooth noise of about unit variance: white noise averaged over 3 points, ``passes`` times along each axis."""
    x = rng.standard_normal(shape)
    for ax in (-2, -1):
        for _ in range(passes):
            x = (np.roll(x, 1, axis=ax) + x + np.roll(x, -1, axis=ax)) / 3.0
    return (x / max(x.std(), 1e-9)).astype(F32)


def shifted_pair(rng, T, C, H, W, shift=(3, -2), noise=0.05):
    a = smooth(rng, (T, C, H, W))
    b = (np.roll(a, shift, axis=(2, 3)) + noise * rng.standard_normal(a.shape)).astype(F32)
    return a, b


def saturated_pair(rng, T, C, H, W, shift=(5, 9)):
    """Plateaus far above the top code beside empty ground: whole windows of q = 255, the largest costs at every level."""
    a = np.where(smooth(rng, (T, C, H, W), passes=12) > 0, F32(100.0), F32(-100.0)).astype(F32)
    if H * W > 64:
        a[..., : (H + 1) // 2, : (W + 1) // 2] = 100.0                  # one plateau of a quarter of the grid for certain
    return a, np.roll(a, shift, axis=(2, 3)).copy()


def padded_bf16(x, fill=7.0):
    """x float32 [T, C, H, W] -> ([T, H, W, 16] bf16 on the device with junk in the padding channels, the values it holds)."""
    T, C, H, W = x.shape
    xb = torch.from_numpy(x).to(torch.bfloat16)
    t = torch.full((T, H, W, 16), fill, dtype=torch.bfloat16)
    t[..., :C] = xb.permute(0, 2, 3, 1)
    return t.to(DEV), xb.float().numpy()


def device_all(ta, kwa, tb, kwb, spec, H, W, disp=None, scalars=None):
    """(disp, scalars, field, morphed) of one dg_deform and one dg_deform_field call over the whole batch."""
    o = _default_ops(torch.device(DEV))
    a, a_nhwc, Cn, T = _fields(ta, kwa.get("channels"), kwa.get("nhwc", False))
    b, b_nhwc, _, _ = _fields(tb, kwb.get("channels"), kwb.get("nhwc", False))
    ka, fa = _descriptor(o, a, a_nhwc, Cn)
    kb, fb = _descriptor(o, b, b_nhwc, Cn)
    side = 2 * spec.D + 1
    if disp is None:
        disp = torch.zeros(spec.nout, 2, side * side, dtype=torch.int64, device=DEV)
        scalars = torch.zeros(spec.nout, 2, 5, dtype=torch.int64, device=DEV)
    field = torch.full((T, spec.nout, 2, 2, H, W), -777, dtype=torch.int16, device=DEV)      # overwritten
    morphed = torch.full((T, spec.nout, 2, H, W), 99, dtype=torch.uint8, device=DEV)
    s = spec.struct()
    o.deform(fa, fb, H, W, s, disp, scalars)
    o.deform_field(fa, fb, H, W, s, field, morphed)
    return disp.cpu().numpy(), scalars.cpu().numpy(), field.cpu().numpy(), morphed.cpu().numpy()


def check(got, want, what):
    assert got[2].tobytes() == want[2].tobytes(), (what, "field", np.argwhere(got[2] != want[2])[:5].tolist())
    assert got[3].tobytes() == want[3].tobytes(), (what, "morphed", np.argwhere(got[3] != want[3])[:5].tolist())
    for name, g, w in zip(("disp", "scalars"), got[:2], want[:2]):
        g, w = ints(g), ints(w)
        assert g == w, (what, name, [(i, x, y) for i, (x, y) in enumerate(zip(g, w)) if x != y][:5])


@pytest.mark.parametrize("F", [1, 2, 3, 4])
@pytest.mark.parametrize("grid", GRIDS)
def test_exact_on_every_grid_and_depth(grid, F):
    H, W = grid
    rng = np.random.default_rng(1000 * H + 10 * W + F)
    # two channels and their speed, three fields, fp32 NCHW against padded bf16 NHWC (and the other way round at even F)
    spec = DeformSpec(2, scale=[1.5, 0.8], offset=[0.2, -0.1], speed=(1, 0), lo=[0.3, 0.1, 0.6], step=[1 / 64, 1 / 128, 1 / 32], levels=F)
    xa, xb = shifted_pair(rng, 3, 2, H, W, shift=(min(3, H - 1), -min(2, W - 1)))
    kw = {"nhwc": True, "channels": 2}
    if F % 2:
        (tb, sb), ta, sa = padded_bf16(xb), torch.from_numpy(xa).to(DEV), xa
        got = device_all(ta, {}, tb, kw, spec, H, W)
    else:
        (ta, sa), tb, sb = padded_bf16(xa), torch.from_numpy(xb).to(DEV), xb
        got = device_all(ta, kw, tb, {}, spec, H, W)
    want = deform_ref(spec, sa, sb)
    check(got, want, f"{grid} F={F} mixed layouts")
    if H * W > 1000:                                                      # not degenerate: pixels matched, vectors found
        assert all(int(v) > 0 for v in want[1][:, :, 0].reshape(-1)) and int(np.abs(want[2]).max()) >= 2
    # one channel, one field, saturated plateaus: the largest costs of every level
    one = DeformSpec(1, speed=None, lo=0.0, step=1 / 8, levels=F)
    ya, yb = saturated_pair(rng, 1, 1, H, W, shift=(min(5, H - 1), min(9, W - 1)))
    want = deform_ref(one, ya, yb)
    check(device_all(torch.from_numpy(ya).to(DEV), {}, torch.from_numpy(yb).to(DEV), {}, one, H, W), want, f"{grid} F={F} saturated")
    assert set(np.unique(want[3]).tolist()) <= {0, 255}
    if H * W > 1000:
        assert int(want[1][0, 0, 4]) >= 255 * 255 * (H * W // 4)          # a quarter of the grid at the top code


def test_special_values_and_bf16_on_both_sides():
    T, H, W = 2, 19, 70
    rng = np.random.default_rng(7)
    xa, xb = shifted_pair(rng, T, 2, H, W)
    special = np.array([np.nan, np.inf, -np.inf, 0.25, np.nextafter(F32(0.25), F32(0)), np.nextafter(F32(0.25), F32(1)), 3e38, -3e38], F32)
    for x in (xa, xb):
        idx = rng.integers(0, x.size, 200)
        x.reshape(-1)[idx] = special[rng.integers(0, special.size, 200)]
    spec = DeformSpec(2, speed=(0, 1), lo=0.25, step=1 / 64, levels=2)
    (ta, sa), (tb, sb) = padded_bf16(xa, fill=float("nan")), padded_bf16(xb, fill=float("inf"))
    kw = {"nhwc": True, "channels": 2}
    check(device_all(ta, kw, tb, kw, spec, H, W), deform_ref(spec, sa, sb), "special values, padded bf16")
    na, nb = torch.from_numpy(xa).to(torch.bfloat16).to(DEV), torch.from_numpy(xb).to(DEV)
    check(device_all(na, {}, nb, {}, spec, H, W), deform_ref(spec, sa, xb), "special values, nchw bf16 + fp32")


def test_call_invariants(monkeypatch):
    T, H, W = 5, 40, 77
    rng = np.random.default_rng(12)
    xa, xb = shifted_pair(rng, T, 2, H, W, shift=(-4, 6))
    spec = DeformSpec(2, lo=0.2, step=1 / 32, levels=3)
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    want = deform_ref(spec, xa, xb)
    p, q = device_all(a, {}, b, {}, spec, H, W), device_all(a, {}, b, {}, spec, H, W)
    for u, v in zip(p, q):
        assert u.tobytes() == v.tobytes()                                # two calls are bit-identical
    check(p, want, "one call")
    twice = device_all(a, {}, b, {}, spec, H, W, disp=torch.from_numpy(p[0]).to(DEV), scalars=torch.from_numpy(p[1]).to(DEV))
    assert ints(twice[0]) == [2 * v for v in ints(want[0])] and ints(twice[1]) == [2 * v for v in ints(want[1])]
    s = device_all(b, {}, a, {}, spec, H, W)                             # the sides swapped: the directions change places
    assert ints(s[0][:, ::-1]) == ints(p[0]) and ints(s[1][:, ::-1]) == ints(p[1])
    assert s[2][:, :, ::-1].tobytes() == p[2].tobytes() and s[3][:, :, ::-1].tobytes() == p[3].tobytes()
    # the modal vector of either direction is the imposed shift
    r = deform.deformation(a, b, spec=spec)
    assert r.fields == T and ints(r.sums()[0]) == ints(want[0]) and ints(r.sums()[1]) == ints(want[1])
    mv = r.modal_vector()
    assert mv[:, 0].tolist() == [[-4.0, 6.0]] * 3 and mv[:, 1].tolist() == [[4.0, -6.0]] * 3
    # batches cut differently, padding fields beyond n_valid
    acc = Deformation(spec, H, W, device=DEV)
    acc.add(a[:2], b[:2]).add(a[2:], b[2:])
    halves = acc.result()
    assert halves.fields == T and ints(halves.sums()[0]) == ints(want[0]) and ints(halves.sums()[1]) == ints(want[1])
    junk = torch.full((2, 2, H, W), 9.0, device=DEV)
    acc = Deformation(spec, H, W, device=DEV)
    acc.add(torch.cat([a[:2], junk]), torch.cat([b[:2], -junk]), n_valid=2).add(torch.cat([a[2:], junk]), torch.cat([b[2:], junk]), n_valid=3)
    padded = acc.result()
    assert padded.fields == T and ints(padded.sums()[0]) == ints(want[0]) and ints(padded.sums()[1]) == ints(want[1])
    f, m = deform.displacement_field(torch.cat([a, junk]), torch.cat([b, junk]), spec=spec, n_valid=T, morphed=True)
    assert f.shape == (T, 3, 2, 2, H, W) and f.cpu().numpy().tobytes() == want[2].tobytes() and m.cpu().numpy().tobytes() == want[3].tobytes()
    # a workspace cap of one field's worth: five calls instead of one, the same integers and bytes
    o = _default_ops(torch.device(DEV))
    per_field = o.deform_ws_bytes(o.eof_fields(a[:1]), H, W, spec.struct())
    assert 0 < per_field < o.deform_ws_bytes(o.eof_fields(a), H, W, spec.struct())
    monkeypatch.setattr(deform, "WS_CAP", per_field)
    calls = []
    real = o.deform
    monkeypatch.setattr(o, "deform", lambda fa, *args: (calls.append(fa.T), real(fa, *args))[1])
    chunked = deform.deformation(a, b, spec=spec, ops=o)
    assert calls == [1] * T and ints(chunked.sums()[0]) == ints(want[0]) and ints(chunked.sums()[1]) == ints(want[1])
    assert deform.displacement_field(a, b, spec=spec, ops=o).cpu().numpy().tobytes() == want[2].tobytes()


def test_largest_table_and_identical_fields():
    H, W, F = 130, 67, 4
    rng = np.random.default_rng(4)
    xa, _ = shifted_pair(rng, 1, 1, H, W)
    xb = np.roll(xa, (-40, 25), axis=(2, 3)).copy()                      # a shift that needs the top level's reach
    spec = DeformSpec(1, speed=None, lo=0.0, step=1 / 64, levels=F)
    assert max_disp(F) == 62 and spec.D == 62
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    want = deform_ref(spec, xa, xb)
    check(device_all(a, {}, b, {}, spec, H, W), want, "F = 4 far shift")
    assert int(np.abs(want[2]).max()) > 30                               # beyond what F = 3 can reach
    same = device_all(a, {}, a, {}, spec, H, W)
    assert not same[2].any() and ints(same[1][0, 0]) == ints(same[1][0, 1]) and int(same[1][0, 0, 2]) == 0 == int(same[1][0, 0, 3])
    centre = 62 * 125 + 62
    assert int(same[0][0, 0, centre]) == int(same[1][0, 0, 0]) == int(same[0][0, 0].sum()) > 0
