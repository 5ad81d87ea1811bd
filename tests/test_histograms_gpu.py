"""Value histograms on the GPU (csrc/histogram.hip) against the numpy float32 definition: exact counts and extrema in four
layouts with affine / speed on and off, determinism, chunked accumulation, the largest spec, more than 2^32 values in one call,
the benchmarked configuration's generated batch, and the trainer's opt-in hook."""
import numpy as np
import pytest
import torch

from downgan_amd import histograms
from downgan_amd.GAN.dataloader import NativeBatch
from downgan_amd.histograms import HistSpec

from .test_histograms_cpu import F32, SPECIAL, edge_values, hist_ref, transform_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check(h, spec, seen, what=""):
    """h (Histogram) against the definition over seen float32 [C, n]: counts and extrema exact, moments to 1e-12."""
    counts, mom, ext = hist_ref(spec, seen)
    c, m, e = h.host()
    np.testing.assert_array_equal(c, counts, err_msg=f"counts {what}")
    np.testing.assert_array_equal(e, ext, err_msg=f"extrema {what}")
    y = transform_ref(spec, seen).astype(np.float64)
    scale = np.where(np.isfinite(y), np.abs(y), 0.0).sum(axis=1)      # the sums cancel: bound their error by sum |y|
    assert np.all(np.abs(m[:, 0] - mom[:, 0]) <= 1e-12 * scale), (what, m[:, 0], mom[:, 0])
    np.testing.assert_allclose(m[:, 1], mom[:, 1], rtol=1e-12, atol=0, err_msg=f"sums of squares {what}")


def planar(x):
    """[T, C, H, W] -> [C, T*H*W] float32."""
    return np.ascontiguousarray(np.asarray(x, dtype=F32).transpose(1, 0, 2, 3)).reshape(x.shape[1], -1)


def layouts(x):
    """(name, input, kwargs, the values the kernel reads [C, n]) of x float32 [T, C, H, W] (C = 2)."""
    T, C, H, W = x.shape
    x32 = torch.from_numpy(x)
    xb = x32.to(torch.bfloat16)
    seen_b = planar(xb.float().numpy())
    pad = torch.full((T, H, W, 16), 7.0, dtype=torch.bfloat16)            # padding channels hold values that must not be read
    pad[..., :C] = xb.permute(0, 2, 3, 1)
    pad = pad.to(DEV)
    return [("nchw_f32", x32.to(DEV), {}, planar(x)),
            ("nchw_bf16", xb.to(DEV), {}, seen_b),
            ("nhwc_bf16_padded", pad, {"nhwc": True, "channels": C}, seen_b),
            ("native_batch", NativeBatch(pad, C), {}, seen_b)]


def specs():
    return [("plain", HistSpec(2048, [-8.0, -8.0], [8.0, 8.0], speed=None)),
            ("speed", HistSpec(2048, [-8.0, -8.0, 0.0], [8.0, 8.0, 11.0])),
            ("affine_speed", HistSpec(1000, [-20.0, -5.0, 0.0], [10.0, 25.0, 30.0], scale=[3.0, 2.5], offset=[-1.5, 4.0])),
            ("affine", HistSpec(777, [-3.0, 0.0], [7.0, 1.0], scale=[0.7, 0.1], offset=[2.0, 0.5], speed=None))]


def data(rng, T, H, W):
    n = T * H * W
    edges = np.concatenate([edge_values(-8.0, 1 / 128, 2048), SPECIAL])
    e = np.resize(edges, n).astype(F32)
    return [("edges", np.stack([e, np.roll(e, 1234)]).reshape(2, T, H, W).transpose(1, 0, 2, 3).copy()),
            ("gauss", (rng.standard_normal((T, 2, H, W)) * 3).astype(F32)),
            ("constant", np.full((T, 2, H, W), 1.25, F32))]


@pytest.mark.parametrize("shape", [(3, 1000, 37), (1, 7, 13), (1, 64, 64)])
def test_exact_counts_in_every_layout(shape):
    T, H, W = shape
    rng = np.random.default_rng(H * W)
    for dname, x in data(rng, T, H, W):
        for name, t, kw, seen in layouts(x):
            for sname, spec in specs():
                check(histograms.histogram(t, spec, **kw), spec, seen, f"{shape} {dname} {name} {sname}")


def test_two_calls_are_bit_identical_and_chunks_add_up():
    rng = np.random.default_rng(7)
    x = torch.from_numpy((rng.standard_normal((24, 2, 96, 80)) * 2).astype(F32)).to(DEV)
    spec = HistSpec.zscore(2, bins=512, lim=6.0)
    a, b = histograms.histogram(x, spec), histograms.histogram(x, spec)
    for u, v in zip(a.host(), b.host()):
        assert u.tobytes() == v.tobytes()
    acc = histograms.ValueHistogram(spec, DEV)
    acc.add(x[:5]).add(x[5:13]).add(x[13:], n_valid=11)
    r = acc.result()
    assert r.fields == 24
    np.testing.assert_array_equal(r.host()[0], a.host()[0])
    np.testing.assert_array_equal(r.host()[2], a.host()[2])
    np.testing.assert_allclose(r.host()[1], a.host()[1], rtol=1e-12)
    check(a, spec, planar(x.cpu().numpy()))


def test_largest_spec():
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((5, 8, 61, 67)) * 4).astype(F32)
    spec = HistSpec(4096, [-10.0] * 8 + [0.0], [10.0] * 8 + [15.0], scale=np.linspace(0.5, 2, 8), offset=np.linspace(-1, 1, 8),
                    speed=(6, 1))
    assert spec.nout == 9
    t = torch.from_numpy(x).to(DEV)
    check(histograms.histogram(t, spec), spec, planar(x))
    nhwc = t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)            # 8 bf16 channels: one 16-byte load per pixel
    check(histograms.histogram(nhwc, spec, nhwc=True), spec, planar(nhwc.permute(0, 3, 1, 2).float().cpu().numpy()))


def test_more_than_2_to_the_32_values_in_one_call():
    T = 4100
    x = torch.full((T, 1024, 1024, 1), 0.5, dtype=torch.bfloat16, device=DEV)
    spec = HistSpec(2048, [-8.0], [8.0], speed=None)
    h = histograms.histogram(x, spec, nhwc=True)
    c, m, e = h.host()
    n = T * 1024 * 1024
    assert n > 2 ** 32
    b = 1 + int((F32(0.5) - F32(-8.0)) * F32(128.0))
    assert c[0, b] == n and c.sum() == n
    assert e.tolist() == [[0.5, 0.5]]
    np.testing.assert_allclose(m[0], [0.5 * n, 0.25 * n], rtol=1e-12)
    del x
    torch.cuda.empty_cache()


def test_generated_batch_of_the_benchmarked_configuration():
    """configs[1]: B = 32, 2 x 1024^2 generator outputs, bf16 in the padded NHWC layout (16 channels), 2 channels + speed."""
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(32, 1024, 1024, 16, generator=g, device=DEV).mul_(2.5).to(torch.bfloat16)
    spec = HistSpec.zscore(2)
    h = histograms.histogram(x, spec, channels=2, nhwc=True)
    seen = x[..., :2].permute(3, 0, 1, 2).float().cpu().numpy().reshape(2, -1)
    check(h, spec, seen)


def _trainer_epoch(monkeypatch):
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
    tr.log_distributions = True
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 2), batch_size=2)           # one batch
    test = torch.utils.data.DataLoader(ds(2, 8), batch_size=2)            # three batches
    tr.train(train, test, epochs=1)
    return tr, coarse, fine


def _sum(hs):
    return sum(h.host()[0] for h in hs)


def test_trainer_hook(monkeypatch):
    tr, coarse, fine = _trainer_epoch(monkeypatch)
    d = tr.metrics_log[0]["distributions"]
    assert d["train"]["fields"] == 2 and d["test"]["fields"] == 6
    spec = HistSpec.zscore(2)
    with torch.no_grad():
        fakes = [tr.G(torch.from_numpy(coarse[a:a + 2])) for a in range(0, 8, 2)]    # the generator after the epoch's update
        again = tr.G(torch.from_numpy(coarse[0:2]))
    assert torch.equal(fakes[0], again)
    fh = [histograms.histogram(f, spec) for f in fakes]
    res = tr.distribution_results
    np.testing.assert_array_equal(res["train"][1].host()[0], fh[0].host()[0])
    np.testing.assert_array_equal(res["test"][1].host()[0], _sum(fh[1:]))
    o = tr._engine.ops
    staged = []
    for a in range(0, 8, 2):
        xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
        o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)
        staged.append(histograms.histogram(xf, spec, channels=2, nhwc=True))
    np.testing.assert_array_equal(res["train"][0].host()[0], staged[0].host()[0])
    np.testing.assert_array_equal(res["test"][0].host()[0], _sum(staged[1:]))
    assert d["test"]["real"]["nan"] == [0, 0, 0]
    np.testing.assert_allclose(d["test"]["w1"], histograms.wasserstein1(*res["test"]), rtol=1e-12)
