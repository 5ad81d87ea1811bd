"""Per-gridpoint statistics on the GPU (csrc/gridstats.hip) against the numpy definition (float32 transform, longdouble sums):
exact counts and extrema and bounded fp64 sums in four layouts, one series and pairs in different layouts, the direct and the
T-split path, determinism, chunked accumulation, padded channels, the largest and the smallest spec, the benchmarked
configuration's generated batch, and the trainer's opt-in hook."""
import os

import numpy as np
import pytest
import torch

from downgan_amd import _lib, gridstats
from downgan_amd.GAN.dataloader import NativeBatch
from downgan_amd.gridstats import GridSpec, GridStats

from .test_gridstats_cpu import LD, grid_ref, sum_bound
from .test_histograms_cpu import F32
from .test_histograms_gpu import layouts, planar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check(m, spec, a, b, T_total, what=""):
    """m (GridMaps) against the definition over the values read, a (and b) float32 [C, T, P]: counts and extrema exactly
    equal, every fp64 sum within (T_total + 8) 2^-52 sum |term| of the longdouble reference.  Prints the largest error as a
    fraction of the bound before asserting."""
    S, M, e, c = grid_ref(spec, a, b)
    gs, ge, gc = m.host()
    assert gs.shape == S.shape and ge.shape == e.shape and gc.shape == c.shape, (what, gs.shape, S.shape)
    np.testing.assert_array_equal(gc, c, err_msg=f"counts {what}")
    np.testing.assert_array_equal(ge, e, err_msg=f"extrema {what}")
    err, bound = np.abs(gs.astype(LD) - S), sum_bound(M, T_total)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err == 0, 0, np.inf))
    print(f"gridstats {what}: max |sum error| / bound = {float(frac.max()):.3g}")
    assert np.all(err <= bound), (what, float(frac.max()), np.argwhere(err > bound)[:5].tolist())


def cube(seen, T):
    """[C, T*P] (the order of test_histograms_gpu.planar) -> [C, T, P]."""
    return seen.reshape(seen.shape[0], T, -1)


THR_X = [0.5, 1.0, 2.0, 2.5, -2.0, 3.0, 4.0]               # inputs that land on a threshold of one of the specs below


def specs():
    return [("plain", GridSpec(2, speed=None)),
            ("speed", GridSpec(2, thresholds=[[0.5, 2.0], [0.5, 2.0], [5.0, 2.0]])),       # (3, 4) -> speed 5 exactly
            ("affine_speed_thr", GridSpec(2, scale=[3.0, 2.5], offset=[-1.5, 4.0], pivot=[-1.0, 4.5, 6.0],
                                          thresholds=[[1.5, 6.0, -7.5], [6.5, -1.0, 4.0], [6.0, 12.0, 0.0]]))]


def special_values():
    f = np.finfo(F32)
    on = np.array(THR_X, dtype=F32)
    return np.concatenate([on, np.nextafter(on, F32(-np.inf)), np.nextafter(on, F32(np.inf)),
                           np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, f.tiny, -f.tiny, np.inf, -np.inf, np.nan,
                                     f.max, -f.max, 1.2e38], dtype=F32)])      # f.max * 3 and 1.2e38 * 3 overflow to inf


def data(rng, T, H, W, shift=0):
    """float32 [T, 2, H, W]: Gaussian values with the special values planted at known (t, p) of both channels, (3, 4) pairs
    for the speed threshold, and one pixel that is never valid."""
    x = (rng.standard_normal((T, 2, H, W)) * 2).astype(F32)
    flat = x.transpose(1, 0, 2, 3).reshape(2, -1)                    # a copy: [C, T*P]
    sv = special_values()
    n = flat.shape[1]
    pos = (np.arange(len(sv)) * 7919 + 13 + shift) % n
    flat[0, pos] = sv
    flat[1, (pos + 5) % n] = sv[::-1]
    flat[0, (pos[:4] + 11) % n], flat[1, (pos[:4] + 11) % n] = 3.0, 4.0
    x = flat.reshape(2, T, H, W).transpose(1, 0, 2, 3).copy()
    if H * W > 20:
        x[:, 0, H - 1, W - 1] = np.nan                               # no valid value at all in channel 0 (and the speed)
    return x


def slices(T, P):
    return _lib.lib().dg_gridstats_slices(T, P)


@pytest.mark.parametrize("shape,split", [((3, 1000, 37), False), ((1, 7, 13), False), ((40, 64, 64), True), ((300, 16, 16), True)])
def test_exact_in_every_layout(shape, split):
    T, H, W = shape
    assert (slices(T, H * W) > 1) == split, slices(T, H * W)          # the last two shapes take the T-split path
    rng = np.random.default_rng(H * W)
    xa, xb = data(rng, T, H, W), data(rng, T, H, W, shift=3)
    la, lb = layouts(xa), layouts(xb)
    for sname, spec in specs():
        for i, (name, t, kw, seen) in enumerate(la):
            m = gridstats.gridstats(t, spec=spec, **kw)
            assert m.fields == T and not m.paired
            check(m, spec, cube(seen, T), None, T, f"{shape} {name} {sname}")
            # paired, the generated series in ANOTHER layout (and dtype) than the real one
            bname, tb, kwb, seen_b = lb[(i + 1) % len(lb)]
            nhwc = (kw.get("nhwc", False), kwb.get("nhwc", False))
            ch = kw.get("channels", kwb.get("channels"))
            m = gridstats.gridstats(t, tb, spec=spec, nhwc=nhwc, channels=ch)
            assert m.fields == T and m.paired
            check(m, spec, cube(seen, T), cube(seen_b, T), T, f"{shape} {name} + {bname} {sname}")
        # and the same layout on both sides (four pixels per thread where the planes allow it)
        for (name, t, kw, seen), (_, tb, _, seen_b) in zip(la, lb):
            m = gridstats.gridstats(t, tb, spec=spec, **kw)
            check(m, spec, cube(seen, T), cube(seen_b, T), T, f"{shape} {name} x 2 {sname}")


@pytest.mark.parametrize("shape", [(24, 96, 80), (64, 32, 32)])
def test_two_calls_are_bit_identical_and_chunks_add_up(shape):
    T, H, W = shape
    rng = np.random.default_rng(7)
    xa, xb = data(rng, T, H, W), data(rng, T, H, W, shift=1)
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    spec = specs()[2][1]
    for pair in (False, True):
        args = (a, b) if pair else (a,)
        p, q = gridstats.gridstats(*args, spec=spec), gridstats.gridstats(*args, spec=spec)
        for u, v in zip(p.host(), q.host()):
            assert u.tobytes() == v.tobytes()
    full = p
    sa, sb = planar(xa).reshape(2, T, -1), planar(xb).reshape(2, T, -1)
    check(full, spec, sa, sb, T, f"{shape} one call")
    if T == 24:
        acc = GridStats(spec, H, W, paired=True, device=DEV)
        junk = torch.full((3, 2, H, W), 9.0, device=DEV)
        acc.add(a[:5], b[:5]).add(a[5:13], b[5:13]).add(torch.cat([a[13:], junk]), torch.cat([b[13:], junk]), n_valid=11)
        r = acc.result()
        assert r.fields == 24 and acc.fields == 24
        np.testing.assert_array_equal(r.host()[2], full.host()[2])
        np.testing.assert_array_equal(r.host()[1], full.host()[1])
        check(r, spec, sa, sb, T, f"{shape} chunks 5 + 8 + 11")


def test_padded_channels_never_reach_a_result():
    """The padding channels of the NHWC store hold 7.0 (test_histograms_gpu.layouts): with speed = (1, 0) and every threshold
    below 7, any padded value read would show in the counts, the extrema and the sums."""
    T, H, W = 6, 24, 20
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((T, 2, H, W))).astype(F32).clip(-6, 6)
    spec = GridSpec(2, speed=(1, 0), thresholds=(6.5,))
    for name, t, kw, seen in layouts(x)[2:]:
        m = gridstats.gridstats(t, t, spec=spec, **kw)
        check(m, spec, cube(seen, T), cube(seen, T), T, f"padded {name}")
        assert m.host()[2][:2, 3:].sum() == 0 and m.max("real")[:2].max() <= 6.0
        assert np.all(m.bias() == 0) and np.all(m.rmse() == 0)


def test_largest_and_smallest_spec():
    rng = np.random.default_rng(8)
    thr = [[-1.0, 0.0, 1.0, 2.0]] * 8 + [[1.0, 2.0, 4.0, 8.0]]
    spec = GridSpec(8, scale=np.linspace(0.5, 2, 8), offset=np.linspace(-1, 1, 8), speed=(6, 1), thresholds=thr)
    assert spec.nout == 9 and spec.K == 4
    for T, H, W in ((5, 61, 67), (5, 60, 68), (37, 12, 20)):        # odd P, P % 4 == 0 (four pixels per thread), and a T-split
        xa, xb = (rng.standard_normal((T, 8, H, W)) * 4).astype(F32), (rng.standard_normal((T, 8, H, W)) * 4).astype(F32)
        xa[0, 3, 0, 0], xb[1, 6, 1, 1] = np.nan, np.inf
        a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
        sa, sb = planar(xa).reshape(8, T, -1), planar(xb).reshape(8, T, -1)
        check(gridstats.gridstats(a, b, spec=spec), spec, sa, sb, T, f"C = 8 nchw {T, H, W}")
        check(gridstats.gridstats(a, spec=spec), spec, sa, None, T, f"C = 8 nchw one series {T, H, W}")
        nhwc = b.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)    # 8 bf16 channels: one 16-byte load per pixel
        sn = planar(nhwc.permute(0, 3, 1, 2).float().cpu().numpy()).reshape(8, T, -1)
        check(gridstats.gridstats(a, nhwc, spec=spec, nhwc=(False, True)), spec, sa, sn, T, f"C = 8 nchw + nhwc bf16 {T, H, W}")
        check(gridstats.gridstats(nhwc, nhwc, spec=spec, nhwc=True), spec, sn, sn, T, f"C = 8 nhwc bf16 x 2 {T, H, W}")
    one = GridSpec.zscore(1)
    assert one.nout == 1
    for T, H, W in ((9, 33, 20), (9, 33, 21), (40, 16, 16)):
        x = (rng.standard_normal((T, 1, H, W)) * 2).astype(F32)
        t = torch.from_numpy(x).to(DEV)
        s = planar(x).reshape(1, T, -1)
        check(gridstats.gridstats(t, spec=one), one, s, None, T, f"C = 1 {T, H, W}")
        check(gridstats.gridstats(t, t.flip(0), spec=one), one, s, s[:, ::-1], T, f"C = 1 paired {T, H, W}")
        tb = t[:, 0].unsqueeze(-1).to(torch.bfloat16)                      # [T, H, W, 1]
        sb = planar(tb.permute(0, 3, 1, 2).float().cpu().numpy()).reshape(1, T, -1)
        check(gridstats.gridstats(tb, spec=one, nhwc=True), one, sb, None, T, f"C = 1 nhwc bf16 {T, H, W}")


def test_generated_batch_of_the_benchmarked_configuration():
    """configs[1]: B = 32, 2 x 1024^2 fields, generated and real both bf16 in the padded NHWC layout (16 channels), 2 channels
    + speed, paired.  For this size only, the reference is computed ON THE DEVICE in torch: the transform in float32 (scale 1,
    offset 0; the speed's square root in float64 and rounded to float32, which is the correctly rounded float32 root), the sums
    in float64 -- not in longdouble, which the factor 2 of the bound allows for."""
    T, N = 32, 1024
    g = torch.Generator(device=DEV).manual_seed(3)
    real = torch.randn(T, N, N, 16, generator=g, device=DEV).mul_(2.5).to(torch.bfloat16)
    fake = (real.float() * 0.8 + 0.6 * torch.randn(T, N, N, 16, generator=g, device=DEV)).to(torch.bfloat16)
    real[3, 5, 7, 0], fake[4, 5, 7, 1], real[:, 9, 9, 1] = float("nan"), float("inf"), float("-inf")
    spec = GridSpec.zscore(2)
    m = gridstats.gridstats(real, fake, spec=spec, nhwc=True, channels=2)
    gs, ge, gc = m.host()
    assert m.fields == T and gs.shape == (3, 12, N * N) and gc.shape == (3, 7, N * N)

    def outputs(x):
        u, v = x[..., 0].float().reshape(T, -1), x[..., 1].float().reshape(T, -1)
        return [u, v, torch.sqrt((u * u + v * v).double()).float()]
    ya, yb = outputs(real), outputs(fake)
    thr = [2.0, 3.0]
    worst = 0.0
    for j in range(3):
        a, b = ya[j], yb[j]
        fa, fb = torch.isfinite(a), torch.isfinite(b)
        both = fa & fb
        zero = torch.zeros((), dtype=torch.float64, device=DEV)
        ua, ub = torch.where(fa, a.double(), zero), torch.where(fb, b.double(), zero)          # pivot 0
        d = torch.where(both, b.double() - a.double(), zero)
        terms = [ua, ua ** 2, ua ** 3, ua ** 4, ub, ub ** 2, ub ** 3, ub ** 4, d, d.abs(), d * d, ua * ub]
        for r, t in enumerate(terms):
            want, mag = t.sum(dim=0).cpu().numpy(), t.abs().sum(dim=0).cpu().numpy()
            err, bound = np.abs(gs[j, r] - want), (T + 8) * 2.0 ** -52 * mag
            worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0, np.inf)))))
            assert np.all(err <= bound), (j, r, worst)
        inf = torch.tensor(float("inf"), device=DEV)
        for s, (y, f) in enumerate(((a, fa), (b, fb))):
            assert np.array_equal(gc[j, s], f.sum(dim=0).cpu().numpy())
            assert np.array_equal(ge[j, 2 * s], torch.where(f, y, inf).amin(dim=0).cpu().numpy())
            assert np.array_equal(ge[j, 2 * s + 1], torch.where(f, y, -inf).amax(dim=0).cpu().numpy())
            for k in range(2):
                assert np.array_equal(gc[j, 3 + 2 * s + k], (y > thr[k]).sum(dim=0).cpu().numpy())
        assert np.array_equal(gc[j, 2], both.sum(dim=0).cpu().numpy())
        del terms, ua, ub, d
    print(f"gridstats configs[1]: max |sum error| / bound = {worst:.3g}")
    assert gc[0, 0, 5 * N + 7] == T - 1 and gc[1, 1, 5 * N + 7] == T - 1 and gc[1, 0, 9 * N + 9] == 0 and gc[2, 2, 9 * N + 9] == 0
    del real, fake
    torch.cuda.empty_cache()


def _trainer_epoch(monkeypatch, map_dir):
    import downgan_amd.config.hyperparams as hp
    from downgan_amd import synthetic
    from downgan_amd.GAN import losses
    from downgan_amd.GAN.dataloader import NetCDFSR
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    monkeypatch.setattr(hp, "batch_size", 2)
    monkeypatch.setattr(losses, "_ops", {})
    torch.manual_seed(0)
    coarse, fine = synthetic.tiles(8, 2, 16, seed=21)
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = WassersteinGAN(G, C_)
    tr.log_maps = True
    tr.map_dir = map_dir
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 2), batch_size=2)           # one batch
    test = torch.utils.data.DataLoader(ds(2, 8), batch_size=2)            # three batches
    tr.train(train, test, epochs=1)
    return tr, coarse, fine


def test_trainer_hook(monkeypatch, tmp_path):
    tr, coarse, fine = _trainer_epoch(monkeypatch, str(tmp_path / "maps"))
    d = tr.metrics_log[0]["maps"]
    assert d["train"]["fields"] == 2 and d["test"]["fields"] == 6
    assert d["test"] == tr.map_results["test"].summary()
    spec = GridSpec.zscore(2)
    o = tr._engine.ops
    acc = GridStats(spec, 128, 128, paired=True, device=o.device)
    reals, fakes = [], []
    with torch.no_grad():
        for a in range(2, 8, 2):
            fake = tr.G(torch.from_numpy(coarse[a:a + 2]))                    # the generator after the epoch's update
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)  # the real fields as the trainer stages them
            acc.add(xf, fake.to(o.device), nhwc=(True, False), channels=2)
            reals.append(xf[..., :2].permute(0, 3, 1, 2).float().cpu().numpy())
            fakes.append(fake.float().cpu().numpy())
    again, got = acc.result(), tr.map_results["test"]
    assert again.fields == got.fields == 6
    np.testing.assert_array_equal(got.host()[2], again.host()[2])
    np.testing.assert_array_equal(got.host()[1], again.host()[1])
    sa, sb = planar(np.concatenate(reals)).reshape(2, 6, -1), planar(np.concatenate(fakes)).reshape(2, 6, -1)
    check(got, spec, sa, sb, 6, "trainer hook")
    check(again, spec, sa, sb, 6, "trainer hook, recomputed")
    assert d["test"]["nonfinite"] == {"real": [0, 0, 0], "fake": [0, 0, 0]}
    for part in ("train", "test"):
        folder = tmp_path / "maps" / "0" / part
        assert os.path.exists(folder / "summary.json")
        for k, v in tr.map_results[part].maps().items():
            np.testing.assert_array_equal(np.load(folder / (k + ".npy")), v)
