"""Fractions skill score on the GPU (csrc/fss.hip) against the integer numpy oracle of test_fss_cpu: sums, base rates and
per-field sums exactly equal in four layouts and in mixed pairs, a 1024 x 1024 pair whose table entries pass 2^16 and whose sums
pass 2^53 (and the 2^60 of the all-ones mask), special values in fp32 and bf16, determinism, chunked accumulation, padding fields
and padded channels, the largest and the smallest spec, and the trainer's opt-in hook.  Every comparison is integer equality."""
import numpy as np
import pytest
import torch

from downgan_amd import fss
from downgan_amd.fss import FractionsSkill, FssSpec
from downgan_amd.histograms import _default_ops, _descriptor, _fields

from .test_fss_cpu import fss_ref, ints, special_fields, special_spec
from .test_histograms_cpu import F32
from .test_histograms_gpu import layouts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOWS = (1, 3, 5, 9, 33, 129, 259)
# real masks of about 16 % and 2 % of the pixels: unit Gaussian components, Rayleigh speed
THRESHOLDS = [[1.0, 2.05], [1.0, 2.05], [1.91, 2.8]]


def correlated(rng, shape):
    """Unit-variance Gaussian fields [..., H, W], spatially correlated: white noise under a 5 x 5 box (periodic)."""
    x = rng.standard_normal(shape)
    return (sum(np.roll(x, (i, j), axis=(-2, -1)) for i in range(-2, 3) for j in range(-2, 3)) / 5.0).astype(F32)


def pair(rng, T, H, W, C=2, shift=3, noise=0.3):
    """(real, generated) float32 [T, C, H, W]: the generated side is the real one shifted by ``shift`` columns, noised."""
    a = correlated(rng, (T, C, H, W))
    b = (np.roll(a, shift, axis=3) + noise * correlated(rng, (T, C, H, W))).astype(F32)
    return a, b


def seen4(seen, T, H, W):
    """[C, T*P] (the order of test_histograms_gpu.planar) -> [T, C, H, W]."""
    return np.ascontiguousarray(seen.reshape(seen.shape[0], T, H, W).transpose(1, 0, 2, 3))


def device_sums(ta, kwa, tb, kwb, spec, H, W):
    """(sums, rates, per_field) of one dg_fss call over the whole batch, as lists of Python integers."""
    o = _default_ops(torch.device(DEV))
    a, a_nhwc, Cn, T = _fields(ta, kwa.get("channels"), kwa.get("nhwc", False))
    b, b_nhwc, _, _ = _fields(tb, kwb.get("channels"), kwb.get("nhwc", False))
    ka, fa = _descriptor(o, a, a_nhwc, Cn)
    kb, fb = _descriptor(o, b, b_nhwc, Cn)
    sums = torch.zeros(spec.nout, spec.K, spec.S, 3, dtype=torch.int64, device=DEV)
    rates = torch.zeros(spec.nout, spec.K, 2, dtype=torch.int64, device=DEV)
    per = torch.full((T, spec.nout, spec.K, spec.S, 3), -1, dtype=torch.int64, device=DEV)    # overwritten, not added to
    o.fss(fa, fb, H, W, spec.struct(), sums, rates, per)
    return sums.cpu().numpy(), rates.cpu().numpy(), per.cpu().numpy()


def check(got, want, what):
    for name, g, w in zip(("sums", "rates", "per_field"), got, want):
        g, w = ints(g), ints(w)
        assert g == w, (what, name, [(i, x, y) for i, (x, y) in enumerate(zip(g, w)) if x != y][:5])


@pytest.mark.parametrize("shape", [(3, 37, 53), (1, 7, 13), (2, 64, 64), (5, 130, 70)])
def test_exact_in_every_layout(shape):
    T, H, W = shape
    rng = np.random.default_rng(H * W)
    xa, xb = pair(rng, T, H, W)
    la, lb = layouts(xa), layouts(xb)
    spec = FssSpec(2, thresholds=THRESHOLDS, scales=WINDOWS)
    refs = {}

    def ref(i, j):
        if (i, j) not in refs:                                           # nchw_f32 reads fp32, the three others the same bf16 values
            refs[(i, j)] = fss_ref(spec, seen4(la[i][3], T, H, W), seen4(lb[j][3], T, H, W))
        return refs[(i, j)]
    for i, (name, t, kw, _) in enumerate(la):
        # the generated series in ANOTHER layout (and dtype) than the real one, and in the same
        for j in ((i + 1) % len(lb), i):
            bname, tb, kwb, _ = lb[j]
            want = ref(min(i, 1), min(j, 1))
            check(device_sums(t, kw, tb, kwb, spec, H, W), want, f"{shape} {name} + {bname}")
            if "nhwc" in kw or "nhwc" in kwb:
                nhwc, ch = (kw.get("nhwc", False), kwb.get("nhwc", False)), kw.get("channels", kwb.get("channels"))
                r = fss.fss(t, tb, spec=spec, nhwc=nhwc, channels=ch)
            else:
                r = fss.fss(t, tb, spec=spec)
            assert r.fields == T and ints(r.sums()) == ints(want[0]) and ints(r.rates()) == ints(want[1]), (shape, name, bname)
    S, R, _ = ref(0, 0)
    f = fss.FssResult(spec, H, W, S, R, T).fss()
    print(f"fss {shape}: base rates {R[:, :, 0].tolist()} of {T * H * W}, scores at n = 1 {f[:, :, 0].round(3).tolist()}, "
          f"at n = {WINDOWS[-1]} {f[:, :, -1].round(4).tolist()}")
    if H * W > 1000:                                                      # the score curve is not degenerate
        assert np.all(f[:, 0, 0] < 0.6) and np.all(f[:2, 0, -1] > 0.99) and np.all(np.diff(f[:, 0]) >= 0)


def test_a_1024_pair_passes_two_to_the_sixteen_and_fifty_three():
    N = 1024
    rng = np.random.default_rng(9)
    xa, xb = pair(rng, 1, N, N, C=1, shift=5)
    spec = FssSpec(1, speed=None, thresholds=(1.0,), scales=(1, 129, 1025, 2047))
    want = fss_ref(spec, xa, xb)
    assert int(want[1][0, 0, 0]) > 1 << 16 and int(want[0][0, 0, 3, 1]) > 1 << 53
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    check(device_sums(a, {}, b, {}, spec, N, N), want, "1024 x 1024")
    r = fss.fss(a, b, spec=spec)
    assert ints(r.sums()) == ints(want[0])
    ref = fss.FssResult(spec, N, N, want[0], want[1], 1)
    assert r.fss().tolist() == ref.fss().tolist() and r.skillful_scale().tolist() == ref.skillful_scale().tolist()
    ones, zeros = torch.ones(1, 1, N, N, device=DEV), torch.zeros(1, 1, N, N, device=DEV)
    top = fss.fss(ones, zeros, spec=FssSpec(1, speed=None, thresholds=(0.5,), scales=(2047,)))
    assert ints(top.sums()) == [1 << 60, 1 << 60, 0] and ints(top.rates()) == [1 << 20, 0]
    both = fss.fss(ones.to(torch.bfloat16), ones, spec=FssSpec(1, speed=None, thresholds=(0.5,), scales=(1, 2047)))
    assert ints(both.sums()) == [0, 1 << 20, 1 << 20, 0, 1 << 60, 1 << 60] and np.all(both.fss() == 1.0)


@pytest.mark.parametrize("shape", [(3, 16, 9), (2, 7, 13)])
def test_special_values_in_fp32_and_bf16(shape):
    T, H, W = shape
    rng = np.random.default_rng(T)
    xa, xb = special_fields(rng, T, H, W), np.roll(special_fields(rng, T, H, W), 2, axis=3)
    la, lb = layouts(xa), layouts(xb)
    for spec in (special_spec(), FssSpec(2, scale=[3.0, 2.5], offset=[-1.5, 4.0], speed=(1, 0),
                                         thresholds=[[1.5, 0.0], [6.5, 4.0], [6.0, 12.0]], scales=(1, 3, 5, 15, 27))):
        for (name, t, kw, seen), (_, tb, kwb, seen_b) in zip(la, lb):
            want = fss_ref(spec, seen4(seen, T, H, W), seen4(seen_b, T, H, W))
            check(device_sums(t, kw, tb, kwb, spec, H, W), want, f"special {shape} {name}")
            assert sum(ints(want[1])) > 0


def test_call_invariants():
    T, H, W = 6, 40, 52
    rng = np.random.default_rng(12)
    xa, xb = pair(rng, T, H, W)
    spec = FssSpec(2, thresholds=THRESHOLDS, scales=(1, 5, 33, 129))
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    want = fss_ref(spec, xa, xb)
    p, q = device_sums(a, {}, b, {}, spec, H, W), device_sums(a, {}, b, {}, spec, H, W)
    for u, v in zip(p, q):
        assert u.tobytes() == v.tobytes()                                # two calls are bit-identical
    check(p, want, "one call")
    acc = FractionsSkill(spec, H, W, device=DEV)
    acc.add(a[:3], b[:3]).add(a[3:], b[3:])
    halves = acc.result()
    assert halves.fields == T and ints(halves.sums()) == ints(want[0]) and ints(halves.rates()) == ints(want[1])
    junk = torch.full((3, 2, H, W), 9.0, device=DEV)                     # padding fields above every threshold
    acc = FractionsSkill(spec, H, W, device=DEV)
    acc.add(torch.cat([a[:2], junk]), torch.cat([b[:2], -junk]), n_valid=2).add(torch.cat([a[2:], junk]), torch.cat([b[2:], junk]), n_valid=4)
    padded = acc.result()
    assert padded.fields == T and ints(padded.sums()) == ints(want[0]) and ints(padded.rates()) == ints(want[1])


@pytest.mark.parametrize("fill", [float("nan"), 3e38, float("inf")])
def test_padded_channels_never_reach_a_result(fill):
    T, H, W = 3, 24, 20
    rng = np.random.default_rng(5)
    xa, xb = pair(rng, T, H, W)
    spec = FssSpec(2, speed=(1, 0), thresholds=THRESHOLDS, scales=(1, 7, 47))

    def padded(x):
        t = torch.full((T, H, W, 16), fill, dtype=torch.bfloat16)
        xb16 = torch.from_numpy(x).to(torch.bfloat16)
        t[..., :2] = xb16.permute(0, 2, 3, 1)
        return t.to(DEV), xb16.float().numpy()
    (ta, sa), (tb, sb) = padded(xa), padded(xb)
    want = fss_ref(spec, sa, sb)
    kw = {"nhwc": True, "channels": 2}
    check(device_sums(ta, kw, tb, kw, spec, H, W), want, f"padded with {fill}")
    r = fss.fss(ta, tb, spec=spec, **kw)
    assert ints(r.sums()) == ints(want[0]) and ints(r.rates()) == ints(want[1])


@pytest.mark.parametrize("cpad", [2, 3, 4, 8])
def test_fp32_channel_last_stores(cpad):
    """[T, H, W, c] fp32 stores (the resident feed's layout): 16-byte pixels take the one-load-per-pixel path, the others the
    element loads; the channels beyond C hold NaN."""
    T, H, W = 2, 19, 67
    rng = np.random.default_rng(cpad)
    xa, xb = pair(rng, T, H, W)
    spec = FssSpec(2, thresholds=THRESHOLDS, scales=(1, 3, 9, 65))
    want = fss_ref(spec, xa, xb)

    def store(x):
        t = torch.full((T, H, W, cpad), float("nan"))
        t[..., :2] = torch.from_numpy(x).permute(0, 2, 3, 1)
        return t.to(DEV)
    kw = {"nhwc": True, "channels": 2}
    check(device_sums(store(xa), kw, store(xb), kw, spec, H, W), want, f"fp32 [T, H, W, {cpad}]")
    check(device_sums(store(xa), kw, torch.from_numpy(xb).to(DEV), {}, spec, H, W), want, f"fp32 [T, H, W, {cpad}] + nchw")


def test_largest_and_smallest_spec():
    rng = np.random.default_rng(8)
    thr = [[-1.0, 0.0, 1.0, 2.0]] * 8 + [[1.0, 2.0, 3.0, 4.0]]
    spec = FssSpec(8, scale=np.linspace(0.5, 2, 8), offset=np.linspace(-1, 1, 8), speed=(6, 1), thresholds=thr,
                   scales=(1, 3, 5, 9, 17, 33, 65, 129))
    assert spec.nout == 9 and spec.K == 4 and spec.S == 8
    for T, H, W in ((2, 33, 20), (1, 61, 67)):
        xa, xb = pair(rng, T, H, W, C=8)
        xa[0, 3, 0, 0], xb[0, 6, 1, 1] = np.nan, np.inf
        a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
        check(device_sums(a, {}, b, {}, spec, H, W), fss_ref(spec, xa, xb), f"C = 8 nchw {T, H, W}")
        nhwc = b.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)    # 8 bf16 channels: one 16-byte load per pixel
        sn = nhwc.permute(0, 3, 1, 2).float().cpu().numpy()
        check(device_sums(a, {}, nhwc, {"nhwc": True}, spec, H, W), fss_ref(spec, xa, sn), f"C = 8 nchw + nhwc bf16 {T, H, W}")
        check(device_sums(nhwc, {"nhwc": True}, nhwc, {"nhwc": True}, spec, H, W), fss_ref(spec, sn, sn), f"C = 8 nhwc x 2 {T, H, W}")
    one = FssSpec(1, speed=None, thresholds=(0.5,), scales=(3,))
    assert (one.nout, one.K, one.S) == (1, 1, 1)
    for T, H, W in ((4, 33, 21), (1, 1, 1), (2, 1, 300), (2, 300, 1)):
        xa, xb = pair(rng, T, H, W, C=1, shift=1)
        a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
        check(device_sums(a, {}, b, {}, one, H, W), fss_ref(one, xa, xb), f"C = 1 {T, H, W}")
        tb = b[:, 0].unsqueeze(-1).to(torch.bfloat16)                    # [T, H, W, 1]
        sb = tb.permute(0, 3, 1, 2).float().cpu().numpy()
        check(device_sums(a, {}, tb, {"nhwc": True}, one, H, W), fss_ref(one, xa, sb), f"C = 1 nchw + nhwc bf16 {T, H, W}")


def test_trainer_hook(monkeypatch):
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
    tr.log_fss = True
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 4), batch_size=2)           # two batches
    test = torch.utils.data.DataLoader(ds(4, 8), batch_size=2)            # two batches
    tr.train(train, test, epochs=1)
    d = tr.metrics_log[0]["fss"]
    assert d["train"]["fields"] == 4 and d["test"]["fields"] == 4 and d["test"] == tr.fss_results["test"].summary()
    spec = FssSpec.zscore(2)
    o = tr._engine.ops
    reals, fakes = [], []
    with torch.no_grad():
        for a in range(4, 8, 2):
            fake = tr.G(torch.from_numpy(coarse[a:a + 2]))                    # the generator after the epoch's updates
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)  # the real fields as the trainer stages them
            reals.append(xf[..., :2].permute(0, 3, 1, 2).float().contiguous())
            fakes.append(fake.to(o.device).float().contiguous())
    real, fake = torch.cat(reals), torch.cat(fakes)
    once = fss.fss(real, fake, spec=spec)
    assert d["test"] == once.summary()
    want = fss_ref(spec, real.cpu().numpy(), fake.cpu().numpy())
    got = tr.fss_results["test"]
    assert ints(got.sums()) == ints(want[0]) and ints(got.rates()) == ints(want[1])
