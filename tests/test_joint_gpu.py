"""Joint histograms on the GPU (csrc/joint.hip) against the numpy float32 restatement of the definition (test_joint_cpu.py): exact
tables in four layouts and mixed layouts, marginals equal to the 1-D value histograms bit for bit, the limits of a spec (a full
table, more than one group of pairs, 4 and 72 sectors, 8 channels), determinism, chunked accumulation, more than 2^32 values in
one call, and the trainer's opt-in hook.

The shape (3, 40, 37) has P = 1480, a multiple of 4 (the four-pixel path over three fields); (3, 41, 37) beside it has an odd P,
(1, 7, 13) fewer pixels than one workgroup, (2, 64, 64) more than one workgroup on the four-pixel path."""
import math

import numpy as np
import pytest
import torch

from downgan_amd import histograms, joint
from downgan_amd.GAN.dataloader import NativeBatch
from downgan_amd.histograms import HistSpec
from downgan_amd.joint import Axis, JointSpec

from .test_histograms_cpu import F32, SPECIAL, edge_values
from .test_joint_cpu import tables_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def planar(x):
    """[T, C, H, W] -> [C, T*H*W] float32."""
    return np.ascontiguousarray(np.asarray(x, dtype=F32).transpose(1, 0, 2, 3)).reshape(x.shape[1], -1)


def layout(x, name):
    """(input, nhwc flag, the values the kernel reads [C, n]) of x float32 [T, C, H, W] in one of the four layouts."""
    T, C, H, W = x.shape
    x32 = torch.from_numpy(x)
    if name == "nchw_f32":
        return x32.to(DEV), False, planar(x)
    xb = x32.to(torch.bfloat16)
    seen = planar(xb.float().numpy())
    if name == "nchw_bf16":
        return xb.to(DEV), False, seen
    pad = torch.full((T, H, W, 16), 7.0, dtype=torch.bfloat16)            # padding channels hold values that must not be read
    pad[..., :C] = xb.permute(0, 2, 3, 1)
    pad = pad.to(DEV)
    return (pad, True, seen) if name == "nhwc_bf16_padded" else (NativeBatch(pad, C), False, seen)


LAYOUTS = ("nchw_f32", "nchw_bf16", "nhwc_bf16_padded", "native_batch")


def specs():
    c = lambda src, ch: Axis(src, ch, 40, -5.0, 5.0)
    stats = {"u10": (0.5, 3.0), "v10": (-0.25, 2.0)}
    return [("zscore", JointSpec.zscore(2), True),
            ("physical", JointSpec.physical(stats, ["u10", "v10"], -20.0, 20.0, bins=80, nsec=16, speed_bins=50, calm=0.5), True),
            ("components", JointSpec([(c("a", 0), c("b", 0)), (c("a", 1), c("b", 1)), (c("a", 0), c("b", 1))], 2, speed=None), True),
            ("single", JointSpec([(Axis("a", "direction", 36), Axis("a", "speed", 64, 0.0, 8.5)), (c("a", 0), c("a", 1))], 2,
                                 calm=0.1), False)]


def data(rng, T, H, W):
    """(name, a, b): two series [T, 2, H, W]."""
    n = T * H * W
    edges = np.concatenate([edge_values(-6.0, 12 / 96, 96), SPECIAL])
    e = np.resize(edges, n).astype(F32)
    shape = lambda u, v: np.stack([u, v]).reshape(2, T, H, W).transpose(1, 0, 2, 3).copy()
    sp = rng.choice(np.concatenate([SPECIAL, [1.0, -2.0, 0.5]]).astype(F32), (2, 2, n))
    return [("edges", shape(e, np.roll(e, 1234)), shape(np.roll(e, 77), e[::-1])),
            ("gauss", (rng.standard_normal((T, 2, H, W)) * 2).astype(F32), (rng.standard_normal((T, 2, H, W)) * 2).astype(F32)),
            ("constant", np.full((T, 2, H, W), 1.25, F32), np.full((T, 2, H, W), -0.75, F32)),
            ("specials", shape(*sp[0]), shape(*sp[1]))]


def run(spec, a, b, a_nhwc=False, b_nhwc=False, **kw):
    return joint.joint_histogram(a, spec, b, nhwc=(a_nhwc, b_nhwc), **kw).host()


@pytest.mark.parametrize("shape", [(3, 40, 37), (3, 41, 37), (1, 7, 13), (2, 64, 64)])
def test_exact_tables_in_every_layout(shape):
    T, H, W = shape
    rng = np.random.default_rng(H * W)
    for dname, xa, xb in data(rng, T, H, W):
        refs = {}                                                           # (spec, f32 | bf16) -> reference tables
        for lname in LAYOUTS:
            a, a_nhwc, seen_a = layout(xa, lname)
            b, b_nhwc, seen_b = layout(xb, lname)
            kw = {"channels": 2} if lname == "nhwc_bf16_padded" else {}
            for sname, spec, two in specs():
                key = (sname, lname == "nchw_f32")
                if key not in refs:
                    refs[key] = tables_ref(spec, seen_a, seen_b if two else None)
                got = run(spec, a, b if two else None, a_nhwc, b_nhwc, **kw)
                np.testing.assert_array_equal(got, refs[key], err_msg=f"{shape} {dname} {lname} {sname}")


def test_mixed_layouts():
    rng = np.random.default_rng(11)
    for T, H, W in ((3, 40, 37), (2, 64, 64)):
        xa, xb = (rng.standard_normal((2, T, 2, H, W)) * 2).astype(F32)
        a, _, seen_a = layout(xa, "nchw_f32")
        b, _, seen_b = layout(xb, "nhwc_bf16_padded")
        spec = JointSpec.zscore(2)
        np.testing.assert_array_equal(run(spec, a, b, False, True, channels=2), tables_ref(spec, seen_a, seen_b))
        bb, _, seen_bb = layout(xb, "nchw_bf16")                             # one layout, two dtypes
        np.testing.assert_array_equal(run(spec, a, bb), tables_ref(spec, seen_a, seen_bb))
        np.testing.assert_array_equal(run(spec, b, a, True, False, channels=2), tables_ref(spec, seen_b, seen_a))


def test_marginals_equal_the_value_histograms():
    rng = np.random.default_rng(12)
    xa, xb = (rng.standard_normal((2, 3, 2, 48, 52)) * 3).astype(F32)
    xa[0, 0, :2, :5] = [np.nan, np.inf, -np.inf, 9.0, -9.0]
    top = 6.0 * math.sqrt(2.0)
    hs = HistSpec(64, [-6.0, -6.0, 0.0], [6.0, 6.0, top])
    c = lambda src, ch: Axis(src, ch, 64, -6.0, 6.0)
    s = lambda src: Axis(src, "speed", 64, 0.0, top)
    spec = JointSpec([(c("a", 0), c("a", 1)), (s("a"), s("b")), (c("b", 1), c("b", 0)), (Axis("b", "direction", 8), s("b"))], 2)
    for la, lb in (("nchw_f32", "nchw_f32"), ("nhwc_bf16_padded", "nhwc_bf16_padded"), ("nchw_f32", "nhwc_bf16_padded")):
        a, a_nhwc, _ = layout(xa, la)
        b, b_nhwc, _ = layout(xb, lb)
        j = joint.joint_histogram(a, spec, b, nhwc=(a_nhwc, b_nhwc), channels=2)
        ha = histograms.histogram(a, hs, nhwc=a_nhwc, channels=2).host()[0]
        hb = histograms.histogram(b, hs, nhwc=b_nhwc, channels=2).host()[0]
        np.testing.assert_array_equal(j.marginals(0)[0], ha[0])
        np.testing.assert_array_equal(j.marginals(0)[1], ha[1])
        np.testing.assert_array_equal(j.marginals(1)[0], ha[2])
        np.testing.assert_array_equal(j.marginals(1)[1], hb[2])
        np.testing.assert_array_equal(j.marginals(2)[0], hb[1])
        np.testing.assert_array_equal(j.marginals(2)[1], hb[0])
        np.testing.assert_array_equal(j.marginals(3)[1], hb[2])
        assert j.marginals(3)[0].sum() == xa[:, 0].size and j.fields == 3


def test_limits_of_a_spec():
    rng = np.random.default_rng(13)
    xa, xb = (rng.standard_normal((2, 2, 2, 33, 47)) * 2).astype(F32)
    a, _, sa = layout(xa, "nchw_f32")
    b, _, sb = layout(xb, "nchw_f32")
    full = JointSpec([(Axis("a", 0, 125, -5.0, 5.0), Axis("b", 1, 125, -5.0, 5.0))], 2)
    assert full.offsets()[-1] == joint.CELLS_MAX
    np.testing.assert_array_equal(run(full, a, b), tables_ref(full, sa, sb))
    for nsec in (4, 72):
        s = JointSpec([(Axis("a", "direction", nsec), Axis("b", "direction", nsec)),
                       (Axis("b", "direction", nsec), Axis("a", "speed", 30, 0.0, 6.0))], 2, calm=0.2)
        np.testing.assert_array_equal(run(s, a, b), tables_ref(s, sa, sb), err_msg=f"nsec {nsec}")
    # eight pairs in more than one group: the tables of zscore(3) hold 58720 cells, a group at most CELLS_MAX
    x3a, x3b = (rng.standard_normal((2, 2, 3, 33, 47)) * 2).astype(F32)
    z3 = JointSpec.zscore(3)
    assert z3.npairs == 8 and z3.offsets()[-1] > 3 * joint.CELLS_MAX
    for lname in ("nchw_f32", "nhwc_bf16_padded"):
        a3, fl, s3a = layout(x3a, lname)
        b3, _, s3b = layout(x3b, lname)
        np.testing.assert_array_equal(run(z3, a3, b3, fl, fl, channels=3), tables_ref(z3, s3a, s3b), err_msg=lname)
    # C = 8 with the speed of channels (6, 1)
    x8a, x8b = (rng.standard_normal((2, 2, 8, 21, 19)) * 2).astype(F32)
    c = lambda src, ch: Axis(src, ch, 50, -8.0, 8.0)
    s8 = JointSpec([(Axis("a", "direction", 16), Axis("a", "speed", 40, 0.0, 12.0)), (c("a", 7), c("b", 7)), (c("a", 6), c("a", 1)),
                    (c("b", 3), Axis("b", "speed", 40, 0.0, 12.0)), (c("a", 0), c("b", 5))], 8, speed=(6, 1),
                   scale=np.linspace(0.5, 2, 8), offset=np.linspace(-1, 1, 8))
    a8, b8 = torch.from_numpy(x8a).to(DEV), torch.from_numpy(x8b).to(DEV)
    np.testing.assert_array_equal(run(s8, a8, b8), tables_ref(s8, planar(x8a), planar(x8b)))
    n8 = lambda t: t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)     # 8 bf16 channels: one 16-byte load per pixel
    seen = lambda t: planar(n8(t).permute(0, 3, 1, 2).float().cpu().numpy())
    np.testing.assert_array_equal(run(s8, n8(a8), n8(b8), True, True), tables_ref(s8, seen(a8), seen(b8)))


def test_two_calls_are_bit_identical_and_chunks_add_up():
    rng = np.random.default_rng(7)
    a, b = (torch.from_numpy((rng.standard_normal((24, 2, 96, 80)) * 2).astype(F32)).to(DEV) for _ in range(2))
    spec = JointSpec.zscore(2)
    r1, r2 = joint.joint_histogram(a, spec, b), joint.joint_histogram(a, spec, b)
    assert r1.host().tobytes() == r2.host().tobytes()
    acc = joint.ValueJoint(spec, DEV)
    acc.add(a[:5], b[:5]).add(a[5:13], b[5:13]).add(a[13:], b[13:], n_valid=11)
    r = acc.result()
    assert r.fields == 24
    np.testing.assert_array_equal(r.host(), r1.host())
    np.testing.assert_array_equal(r1.host(), tables_ref(spec, planar(a.cpu().numpy()), planar(b.cpu().numpy())))


def test_more_than_2_to_the_32_values_in_one_call():
    T = 4100
    x = torch.full((T, 1024, 1024, 1), 0.5, dtype=torch.bfloat16, device=DEV)
    ax = Axis("a", 0, 96, -6.0, 6.0)
    spec = JointSpec([(ax, ax)], 1, speed=None)
    t = joint.joint_histogram(x, spec, nhwc=True).table(0)
    n = T * 1024 * 1024
    assert n > 2 ** 32
    k = 1 + int((F32(0.5) - F32(-6.0)) * F32(8.0))
    assert t[k, k] == n and t.sum() == n
    del x
    torch.cuda.empty_cache()


def test_trainer_hook(monkeypatch):
    from downgan_amd.GAN.wasserstein import WassersteinGAN

    from .test_histograms_gpu import _trainer_epoch
    monkeypatch.setattr(WassersteinGAN, "log_joint", True)
    tr, coarse, fine = _trainer_epoch(monkeypatch)
    d = tr.metrics_log[0]["joint"]
    assert d["train"]["fields"] == 2 and d["test"]["fields"] == 6
    spec = JointSpec.zscore(2)
    o = tr._engine.ops
    tables = []
    with torch.no_grad():
        for a in range(0, 8, 2):
            fake = tr.G(torch.from_numpy(coarse[a:a + 2])).to(o.device)         # the generator after the epoch's update
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)    # the real fields as the engine stages them
            tables.append(joint.joint_histogram(xf, spec, fake, channels=2, nhwc=(True, False)).host())
    res = tr.joint_results
    np.testing.assert_array_equal(res["train"].host(), tables[0])
    np.testing.assert_array_equal(res["test"].host(), sum(tables[1:]))
    assert d["test"]["rose_tv"] == pytest.approx(res["test"].tv_distance("rose_real", "rose_fake"), rel=1e-12)
    assert list(d["test"]["real_vs_generated"]) == ["ch0", "ch1", "speed"]
