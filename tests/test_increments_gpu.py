"""Increment histograms on the GPU (csrc/increments.hip) against the numpy float32 restatement of the definition
(test_increments_cpu.py): exact counts and ``finite`` in four layouts and in mixed layouts, the moments to 1e-12 * sum |term| (the
rule test_histograms_gpu.py applies to dg_hist's sums: fp64 unit round-off times the longest addition chain at these sizes); the
direction tables against dg_hist of the explicitly formed differences, bit for bit; transposition; the limits of a spec;
determinism and chunked accumulation; one cell above 2^32; and the trainer's opt-in hook.

Shapes: (3, 40, 37) has P % 4 == 0 with an odd W (rows are not 16-byte aligned: the element path), (3, 41, 37) an odd P,
(1, 7, 13) is smaller than a workgroup and than most lags, (2, 64, 64) takes the four-pixel path.  (1, 300, 520) with lags
(1, 3, 64, 255, 256) crosses every tile boundary of the kernel: in direction 0 the anchor tiles are 512 columns wide and, at a
staged width of 520, 47 rows high -- column tiles at 0 and 512 (the partners of the anchors in columns 256 .. 263 at lags 255 /
256 lie past column 512, in the halo) and seven row tiles; in direction 1 the strips are 64 columns wide (nine, the last of 8
columns) and hold 128 anchor rows above a 256-row halo -- row tiles at 0, 128 and 256, the last with fewer rows than the halo.
Along w that shape is still staged as whole rows (520 < 512 + 256), so (1, 40, 1100) with lags (1, 128, 256) adds the case the
benchmarked 1024-wide fields take: a direction-0 tile cut at its own staged width (768 columns at column 0, less than the row), the
next one starting inside the first one's halo (column 512), and a third of 76 columns; 32 rows per tile, so two row tiles."""
import numpy as np
import pytest
import torch

from downgan_amd import histograms, increments
from downgan_amd.histograms import HistSpec
from downgan_amd.increments import Increments, IncrementSpec

from .test_histograms_cpu import F32, SPECIAL
from .test_increments_cpu import assert_tables, spec_ref, totals
from .test_joint_gpu import LAYOUTS, data, layout

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def fields(seen, T, H, W):
    """[C, T*H*W] (the values the kernel reads, as ``layout`` returns them) -> [T, C, H, W]."""
    return np.ascontiguousarray(seen.reshape(seen.shape[0], T, H, W).transpose(1, 0, 2, 3))


def got_of(res, i):
    return res.counts[i], res.finite[i], res.moments[i]


SMALL_LAGS = (1, 2, 3, 12, 13, 36, 37, 64)                   # W - 1 and W of the 37-wide shapes, W of (7, 13), the side of 64 x 64
SHAPES = [((3, 40, 37), SMALL_LAGS), ((3, 41, 37), SMALL_LAGS), ((1, 7, 13), SMALL_LAGS), ((2, 64, 64), SMALL_LAGS),
          ((1, 300, 520), (1, 3, 64, 255, 256)), ((1, 40, 1100), (1, 128, 256))]


@pytest.mark.parametrize("shape,lags", SHAPES)
def test_exact_tables_in_every_layout(shape, lags):
    T, H, W = shape
    rng = np.random.default_rng(H * W)
    spec = IncrementSpec(2, speed=(0, 1), lags=lags, nbins=96, ranges=6.0)      # bin width 1 / 8: differences of the edges are edges
    for dname, xa, xb in data(rng, T, H, W):
        refs = {}                                                               # f32 | bf16 -> the reference tables of both series
        for lname in LAYOUTS:
            a, a_nhwc, seen_a = layout(xa, lname)
            b, b_nhwc, seen_b = layout(xb, lname)
            kw = {"channels": 2} if lname == "nhwc_bf16_padded" else {}
            key = lname == "nchw_f32"
            if key not in refs:
                refs[key] = [spec_ref(spec, fields(s, T, H, W), exact=False) for s in (seen_a, seen_b)]
            res = increments.increments(a, b, spec, nhwc=(a_nhwc, b_nhwc), **kw)
            assert res.nser == 2 and res.fields == T and (res.H, res.W) == (H, W)
            for i in (0, 1):
                assert_tables(got_of(res, i), refs[key][i], f"{shape} {dname} {lname} series {i}")
            np.testing.assert_array_equal(res.counts.sum(axis=-1), np.broadcast_to(totals(T, H, W, lags), (2, 3, 2, len(lags))))


def test_mixed_layouts_and_one_series():
    rng = np.random.default_rng(11)
    spec = IncrementSpec.zscore(2, lags=(1, 2, 4, 8, 16, 32, 36, 63))
    for T, H, W in ((3, 40, 37), (2, 64, 64)):
        xa, xb = (rng.standard_normal((2, T, 2, H, W)) * 2).astype(F32)
        a, _, seen_a = layout(xa, "nchw_f32")
        b, _, seen_b = layout(xb, "nhwc_bf16_padded")
        bb, _, seen_bb = layout(xb, "nchw_bf16")
        ra, rb, rbb = (spec_ref(spec, fields(s, T, H, W), exact=False) for s in (seen_a, seen_b, seen_bb))
        res = increments.increments(a, b, spec, nhwc=(False, True), channels=2)
        assert_tables(got_of(res, 0), ra)
        assert_tables(got_of(res, 1), rb)
        res = increments.increments(b, a, spec, nhwc=(True, False), channels=2)
        assert_tables(got_of(res, 0), rb)
        assert_tables(got_of(res, 1), ra)
        res = increments.increments(a, bb, spec)                                # one layout, two dtypes
        assert_tables(got_of(res, 1), rbb)
        one = increments.increments(bb, None, spec)
        assert one.nser == 1 and one.counts.shape[0] == 1
        assert_tables(got_of(one, 0), rbb)


def test_direction_tables_equal_the_value_histograms_of_the_differences():
    """Pins the kernel without the restatement: fp32 NCHW input, identity transform; the explicit differences are one rounded
    fp32 subtraction each (torch), binned by dg_hist under the same lo / inv_w."""
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((2, 2, 150, 203)) * 1.5).astype(F32)
    x[0, 0, :3, :7] = np.resize(SPECIAL, 21).reshape(3, 7)
    x[1, 1, 100:102, 190:203] = np.resize(SPECIAL, 26).reshape(2, 13)
    lags = (1, 2, 5, 64, 100, 149, 150, 202)
    spec = IncrementSpec(2, speed=None, lags=lags, nbins=128, ranges=4.0)
    hs = HistSpec(128, [-4.0, -4.0], [4.0, 4.0], speed=None)
    np.testing.assert_array_equal(hs.inv_w, spec.inv_w[:, 0])
    xd = torch.from_numpy(x).to(DEV)
    res = increments.increments(xd, None, spec)
    for l, r in enumerate(lags):
        for d, diff in ((0, xd[..., r:] - xd[..., :-r]), (1, xd[:, :, r:, :] - xd[:, :, :-r, :])):
            if diff.numel() == 0:
                assert res.counts[0, :, d, l].sum() == 0
                continue
            h = histograms.histogram(diff.contiguous(), hs).host()[0]
            np.testing.assert_array_equal(res.counts[0, :, d, l], h, err_msg=f"lag {r} direction {d}")


def test_transposition_swaps_the_directions():
    rng = np.random.default_rng(13)
    x = (rng.standard_normal((2, 2, 141, 530)) * 2).astype(F32)
    x[0, 1, 5, ::7] = np.inf
    x[1, 0, ::11, 3] = np.nan
    spec = IncrementSpec(2, lags=(1, 4, 63, 64, 140, 141, 200, 256), nbins=100, ranges=5.0)
    xd = torch.from_numpy(x).to(DEV)
    a = increments.increments(xd, None, spec)
    b = increments.increments(xd.transpose(2, 3).contiguous(), None, spec)
    np.testing.assert_array_equal(a.counts[:, :, 0], b.counts[:, :, 1])
    np.testing.assert_array_equal(a.counts[:, :, 1], b.counts[:, :, 0])
    np.testing.assert_array_equal(a.finite[:, :, ::-1], b.finite)
    scale = spec_ref(spec, x, exact=False)[3]
    assert np.all(np.abs(a.moments[0, :, ::-1] - b.moments[0]) <= 2e-12 * scale[:, ::-1])     # the same terms in another order


def test_limits_of_a_spec():
    rng = np.random.default_rng(14)
    # nbins = 512 with 8 lags and C = 8 plus the speed: 9 x 8 x 516 cells, five launch groups of at most two output channels
    x8 = (rng.standard_normal((2, 8, 21, 19)) * 2).astype(F32)
    s8 = IncrementSpec(8, scale=np.linspace(0.5, 2, 8), offset=np.linspace(-1, 1, 8), speed=(6, 1), lags=(1, 2, 3, 4, 5, 8, 13, 18),
                       nbins=512, ranges=np.linspace(1.0, 9.0, 72).reshape(9, 8))
    a8 = torch.from_numpy(x8).to(DEV)
    assert_tables(got_of(increments.increments(a8, None, s8), 0), spec_ref(s8, x8, exact=False))
    n8 = a8.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)                # 8 bf16 channels: one 16-byte load per pixel
    seen = n8.permute(0, 3, 1, 2).float().cpu().numpy()
    assert_tables(got_of(increments.increments(n8, None, s8, nhwc=True), 0), spec_ref(s8, seen, exact=False))
    # one bin
    x = (rng.standard_normal((2, 2, 33, 47)) * 2).astype(F32)
    s1 = IncrementSpec(2, lags=(1, 46), nbins=1, ranges=1.0)
    assert_tables(got_of(increments.increments(torch.from_numpy(x).to(DEV), None, s1), 0), spec_ref(s1, x, exact=False))
    # a single lag of 256, the largest
    x = (rng.standard_normal((1, 1, 258, 300)) * 2).astype(F32)
    s256 = IncrementSpec(1, speed=None, lags=(256,), nbins=64, ranges=8.0)
    res = increments.increments(torch.from_numpy(x).to(DEV), None, s256)
    assert_tables(got_of(res, 0), spec_ref(s256, x, exact=False))
    assert res.finite.reshape(-1).tolist() == [258 * 44, 2 * 300]


def test_two_calls_are_bit_identical_and_chunks_add_up():
    rng = np.random.default_rng(7)
    a, b = (torch.from_numpy((rng.standard_normal((24, 2, 96, 80)) * 2).astype(F32)).to(DEV) for _ in range(2))
    spec = IncrementSpec.zscore(2)
    r1, r2 = increments.increments(a, b, spec), increments.increments(a, b, spec)
    for u, v in zip(got_of(r1, slice(None)), got_of(r2, slice(None))):
        assert u.tobytes() == v.tobytes()
    acc = Increments(spec, DEV)
    acc.add(a[:5], b[:5]).add(a[5:13], b[5:13]).add(a[13:], b[13:], n_valid=11)
    r = acc.result()
    assert r.fields == 24
    np.testing.assert_array_equal(r.counts, r1.counts)
    np.testing.assert_array_equal(r.finite, r1.finite)
    for i, x in enumerate((a, b)):
        ref = spec_ref(spec, x.cpu().numpy(), exact=False)
        assert_tables(got_of(r1, i), ref)
        assert np.all(np.abs(r.moments[i] - r1.moments[i]) <= 2e-12 * ref[3])     # the same terms in three partial sums


def test_one_cell_above_2_to_the_32():
    """A constant 1024 x 1024 one-channel bf16 field presented 4110 times through a stride-0 descriptor (ld_t = 0).  (4100
    presentations stay below 2^32 at every lag: 4100 * 1024 * 1023 = 2^32 - 4096.)"""
    T, N, r = 4110, 1024, 1
    x = torch.full((1, N, N, 1), 0.5, dtype=torch.bfloat16, device=DEV).expand(T, N, N, 1)
    spec = IncrementSpec(1, speed=None, lags=(r,), nbins=4, ranges=2.0)
    res = increments.increments(x, None, spec, nhwc=True)
    n = T * N * (N - r)
    assert n > 2 ** 32
    k = 1 + int((F32(0.0) - F32(-2.0)) * F32(1.0))
    for d in (0, 1):
        assert res.counts[0, 0, d, 0, k] == n and res.counts[0, 0, d, 0].sum() == n and res.finite[0, 0, d, 0] == n
    assert not res.moments.any()
    assert res.summary()["real"]["flatness"] == [[[None], [None]]]


def test_trainer_hook(monkeypatch):
    from downgan_amd.GAN.wasserstein import WassersteinGAN

    from .test_histograms_gpu import _trainer_epoch
    monkeypatch.setattr(WassersteinGAN, "log_increments", True)
    tr, coarse, fine = _trainer_epoch(monkeypatch)
    d = tr.metrics_log[0]["increments"]
    assert d["train"]["fields"] == 2 and d["test"]["fields"] == 6
    spec = IncrementSpec.zscore(2)
    o = tr._engine.ops
    tables = []
    with torch.no_grad():
        for a in range(0, 8, 2):
            fake = tr.G(torch.from_numpy(coarse[a:a + 2])).to(o.device)         # the generator after the epoch's update
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)    # the real fields as the engine stages them
            tables.append(increments.increments(xf, fake, spec, channels=2, nhwc=(True, False)))
    res = tr.increment_results
    np.testing.assert_array_equal(res["train"].counts, tables[0].counts)
    np.testing.assert_array_equal(res["train"].finite, tables[0].finite)
    scale = np.abs(res["train"].moments[..., [1, 1, 2, 4, 4, 5]])                # sum |term| of u, |u|, u^2, u^3, |u|^3, u^4
    assert np.all(np.abs(res["train"].moments - tables[0].moments) <= 1e-12 * scale)
    np.testing.assert_array_equal(res["test"].counts, sum(t.counts for t in tables[1:]))
    np.testing.assert_array_equal(res["test"].finite, sum(t.finite for t in tables[1:]))
    scale = np.abs(res["test"].moments[..., [1, 1, 2, 4, 4, 5]])                 # sum |term| of u, |u|, u^2, u^3, |u|^3, u^4
    assert np.all(np.abs(res["test"].moments - sum(t.moments for t in tables[1:])) <= 4e-12 * scale)     # three partial sums
    assert d["test"]["channels"] == ["ch0", "ch1", "speed"] and d["test"]["lags"] == list(increments.DEFAULT_LAGS)
    assert d["test"]["w1"] == increments._jsonable(res["test"].w1())
