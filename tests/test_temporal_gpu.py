"""Temporal diagnostics on the GPU (csrc/temporal.hip) against the library's host reference dg_temporal_host (itself pinned to a
numpy restatement by test_temporal_cpu): every output and both carried state arrays bit for bit in every layout and dtype, one
series and pairs in different layouts, the chunking contract, padded channels, the limits at a small grid, n_valid, and the
trainer's opt-in hook.  Every comparison is exact equality of bits (NaN payloads and the float64 sums included)."""
import os

import numpy as np
import pytest
import torch

from downgan_amd import temporal
from downgan_amd.GAN.dataloader import NativeBatch
from downgan_amd.temporal import ARRAYS, Temporal, TemporalResult, TemporalSpec

from .test_histograms_gpu import DEV
from .test_temporal_cpu import data, same_bits, specs

pytestmark = pytest.mark.gpu

CUTS = (2, 7, 8)                                                     # the chunks (2, 5, 1, rest)


def fields(rng, spec, T, H, W):
    """float32 [T, C, H, W] of test_temporal_cpu.data, spells planted across every boundary of CUTS."""
    return data(rng, spec, T, H * W, cuts=CUTS).reshape(T, spec.C, H, W)


def seen_of(t, nhwc, Cn):
    """The values the kernel reads, float32 [T, C, P]."""
    x = t.nhwc if isinstance(t, NativeBatch) else t
    x = x[..., :Cn].permute(0, 3, 1, 2) if nhwc or isinstance(t, NativeBatch) else x
    return np.ascontiguousarray(x.float().cpu().numpy().reshape(x.shape[0], Cn, -1))


def layouts(x, pad_to=16, fill=7.0):
    """(name, input, kwargs) of x float32 [T, C, H, W]: NCHW fp32 / bf16, the feed's [n, H, W, c] fp32 store, the padded NHWC
    bf16 store (16-byte aligned pixels; the padding channels hold ``fill``, which must not be read), the same as a NativeBatch,
    and two views whose field stride is odd (an fp32 one and a bf16 one that also starts one element off): one element per
    load."""
    T, Cn, H, W = x.shape
    x32 = torch.from_numpy(x).to(DEV)
    xb = x32.to(torch.bfloat16)
    pad = torch.full((T, H, W, pad_to), fill, dtype=torch.bfloat16, device=DEV)
    pad[..., :Cn] = xb.permute(0, 2, 3, 1)
    n = Cn * H * W
    big = torch.zeros(T, n + 1, device=DEV)
    big[:, :n] = x32.reshape(T, n)
    bigb = torch.zeros(T * (n + 1) + 1, dtype=torch.bfloat16, device=DEV)
    bigb[1:].view(T, n + 1)[:, :n] = xb.reshape(T, n)
    return [("nchw_f32", x32, {}), ("nchw_bf16", xb, {}),
            ("nhwc_f32_feed", torch.empty(T, H, W, Cn, device=DEV).copy_(x32.permute(0, 2, 3, 1)), {"nhwc": True}),
            ("nhwc_bf16_padded", pad, {"nhwc": True, "channels": Cn}), ("native_batch", NativeBatch(pad, Cn), {}),
            ("strided_f32", big[:, :n].view(T, Cn, H, W), {}), ("strided_bf16", bigb[1:].view(T, n + 1)[:, :n].view(T, Cn, H, W), {})]


def device_state(acc, ser):
    """The seven arrays of series ``ser`` of a Temporal accumulator as numpy arrays."""
    return {k: acc.arrays[k][ser].cpu().numpy() for k in ARRAYS}


def run(spec, H, W, a, b=None, kw=None, kwb=None, cuts=()):
    """A fresh accumulator fed (a, b) cut at ``cuts``."""
    kw, kwb = kw or {}, kwb or {}
    acc = Temporal(spec, H, W, paired=b is not None, device=DEV)
    T = (a.nhwc if isinstance(a, NativeBatch) else a).shape[0]
    edges = [0] + [c for c in cuts if 0 < c < T] + [T]
    cut = lambda t, lo, hi: NativeBatch(t.nhwc[lo:hi], t.channels) if isinstance(t, NativeBatch) else t[lo:hi]
    for lo, hi in zip(edges, edges[1:]):
        nhwc = (kw.get("nhwc", False), kwb.get("nhwc", False))
        acc.add(cut(a, lo, hi), None if b is None else cut(b, lo, hi), nhwc=nhwc, channels=kw.get("channels", kwb.get("channels")))
    assert acc.fields == T
    return acc


@pytest.mark.parametrize("shape", [(1, 1, 1), (50, 1, 1), (3, 7, 13), (40, 64, 64), (300, 16, 16), (5, 512, 512)])
def test_kernel_against_the_host_reference_in_every_layout(shape):
    """(1, 1, 1), (50, 1, 1): one thread; (3, 7, 13): P no multiple of 4, a ragged wave, a series shorter than the largest lag;
    (40, 64, 64): several workgroups per output channel; (300, 16, 16): a long walk; (5, 512, 512): the smallest grid on which a
    thread owns four pixels of an NCHW plane (the other layouts keep one pixel per thread there)."""
    T, H, W = shape
    big = H * W >= 512 * 512
    for sname, spec in (specs()[:1] if big else specs()):
        rng = np.random.default_rng(H * W + T)
        xa, xb = fields(rng, spec, T, H, W), fields(rng, spec, T, H, W)
        la, lb = layouts(xa), layouts(xb)
        if big:
            la, lb = [la[i] for i in (0, 1, 3)], [lb[i] for i in (1, 3, 0)]
        else:
            lb = lb[1:] + lb[:1]                                      # the generated series in ANOTHER layout (and dtype)
        host = {}

        def want(t, kw):
            seen = seen_of(t, kw.get("nhwc", False), spec.C)
            key = seen.tobytes()
            if key not in host:
                host[key] = temporal.host_temporal(spec, seen)
            return host[key]
        for (name, t, kw), (bname, tb, kwb) in zip(la, lb):
            one = run(spec, H, W, t, kw=kw)
            same_bits(device_state(one, 0), want(t, kw), f"{shape} {sname} {name}")
            pair = run(spec, H, W, t, tb, kw, kwb)
            same_bits(device_state(pair, 0), want(t, kw), f"{shape} {sname} {name} + {bname}: real")
            same_bits(device_state(pair, 1), want(tb, kwb), f"{shape} {sname} {name} + {bname}: fake")
        res = pair.result()
        ref = TemporalResult.from_state(spec, H, W, T, want(t, kw), want(tb, kwb))
        for k in ("spells", "cens", "spellmap", "ramps", "accnt"):
            np.testing.assert_array_equal(getattr(res, k), getattr(ref, k), err_msg=f"{shape} {sname} result {k}")
        assert res.fields == T and res.paired and res.acsum.tobytes() == ref.acsum.tobytes()


def test_the_result_does_not_depend_on_the_chunking():
    T, H, W = 40, 64, 64
    for sname, spec in specs():
        rng = np.random.default_rng(17)
        xa, xb = fields(rng, spec, T, H, W), fields(rng, spec, T, H, W)
        la, lb = layouts(xa), layouts(xb)
        for i, j in ((0, 3), (1, 5), (2, 0)):                         # pairs of different layouts and dtypes
            (name, t, kw), (bname, tb, kwb) = la[i], lb[j]
            whole = run(spec, H, W, t, tb, kw, kwb)
            again = run(spec, H, W, t, tb, kw, kwb)
            parts = run(spec, H, W, t, tb, kw, kwb, cuts=CUTS)
            for ser in (0, 1):
                same_bits(device_state(again, ser), device_state(whole, ser), f"{sname} {name} + {bname}: two runs")
                same_bits(device_state(parts, ser), device_state(whole, ser), f"{sname} {name} + {bname}: chunks (2, 5, 1, rest)")
            same_bits(device_state(whole, 0), temporal.host_temporal(spec, seen_of(t, kw.get("nhwc", False), spec.C)), f"{sname} host")
        name, t, kw = la[0]
        ones = run(spec, H, W, t, kw=kw, cuts=range(1, T))
        same_bits(device_state(ones, 0), device_state(run(spec, H, W, t, kw=kw), 0), f"{sname} {name}: chunks of 1")
        name, t, kw = la[3]
        ones = run(spec, H, W, t, kw=kw, cuts=range(1, T))
        same_bits(device_state(ones, 0), device_state(run(spec, H, W, t, kw=kw), 0), f"{sname} {name}: chunks of 1")


def test_padded_channels_never_reach_a_table():
    """The padding channels of the NHWC store hold 7.0, -inf or NaN: nothing changes, with the speed reading channels (1, 0)."""
    T, H, W = 12, 24, 20
    spec = TemporalSpec(2, speed=(1, 0), thresholds=[[0.5, -0.5], [0.5, -0.5], [1.0, 0.25]], below=(False, True), ndur=8, lags=(1, 4))
    x = fields(np.random.default_rng(5), spec, T, H, W)
    got = []
    for fill in (7.0, float("-inf"), float("nan")):
        for name, t, kw in layouts(x, fill=fill)[3:5]:
            got.append(device_state(run(spec, H, W, t, kw=kw, cuts=(5,)), 0))
    host = temporal.host_temporal(spec, seen_of(layouts(x)[3][1], True, 2))
    for g in got:
        same_bits(g, host, "padded channels")
    assert host["ramps"].sum() == (2 * T - 5) * 3 * H * W


def test_limits_at_a_small_grid():
    """nthr = 4, nlag = 4 with lag 24, ndur = 256, nbins = 512, 6 input channels + the speed, on (30, 8, 8); the padded store
    holds 8 bf16 channels: one 16-byte load per pixel of which 6 channels are read."""
    T, H, W = 30, 8, 8
    spec = TemporalSpec(6, scale=np.linspace(0.5, 2, 6), offset=np.linspace(-1, 1, 6), speed=(5, 1),
                        thresholds=[[1.0, 2.0, -1.0, -2.0]] * 6 + [[1.5, 2.5, 0.5, 0.25]], below=(False, False, True, True), ndur=256,
                        lags=(1, 7, 23, 24), nbins=512, ranges=6.0)
    assert spec.nout == 7 and spec.R == 24
    rng = np.random.default_rng(8)
    xa, xb = fields(rng, spec, T, H, W), fields(rng, spec, T, H, W)
    la, lb = layouts(xa, pad_to=8), layouts(xb, pad_to=8)
    for i, j in ((0, 3), (3, 1), (5, 6), (2, 4)):
        (name, t, kw), (bname, tb, kwb) = la[i], lb[j]
        for cuts in ((), CUTS):
            acc = run(spec, H, W, t, tb, kw, kwb, cuts=cuts)
            assert acc.arrays["spells"].shape == (2, 7, 4, 256) and acc.arrays["ramps"].shape == (2, 7, 4, 515)
            same_bits(device_state(acc, 0), temporal.host_temporal(spec, seen_of(t, kw.get("nhwc", False), 6)), f"{name} {cuts}")
            same_bits(device_state(acc, 1), temporal.host_temporal(spec, seen_of(tb, kwb.get("nhwc", False), 6)), f"{bname} {cuts}")


def test_n_valid_adds_the_leading_fields_and_the_next_call_continues():
    T, H, W = 24, 20, 12
    name, spec = specs()[0]
    rng = np.random.default_rng(7)
    xa, xb = fields(rng, spec, T, H, W), fields(rng, spec, T, H, W)
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    junk = torch.full((3, 2, H, W), 9.0, device=DEV)
    acc = Temporal(spec, H, W, paired=True, device=DEV)
    acc.add(torch.cat([a[:7], junk]), torch.cat([b[:7], junk]), n_valid=7)
    assert acc.fields == 7
    acc.add(torch.cat([a[7:], junk]), torch.cat([b[7:], junk]), n_valid=17)
    assert acc.fields == 24
    same_bits(device_state(acc, 0), temporal.host_temporal(spec, xa.reshape(T, 2, -1)), "n_valid real")
    same_bits(device_state(acc, 1), temporal.host_temporal(spec, xb.reshape(T, 2, -1)), "n_valid fake")
    one = temporal.temporal(a, b, spec=spec)
    res = acc.result()
    for k in ("spells", "cens", "spellmap", "ramps", "accnt"):
        np.testing.assert_array_equal(getattr(res, k), getattr(one, k), err_msg=k)
    assert res.acsum.tobytes() == one.acsum.tobytes() and res.cens.sum() > 0
    assert acc.nbytes == sum(v.numel() * v.element_size() for v in acc.arrays.values())


def test_a_call_longer_than_one_launch_takes():
    """2^20 + 3 fields of one pixel: the library cuts a call into launches of at most 2^20 fields (no uint32 cell of the LDS tables
    can wrap), which the chunking contract makes invisible."""
    T = 2 ** 20 + 3
    spec = TemporalSpec(1, speed=None, thresholds=[0.0], below=False, ndur=8, lags=(1, 3), nbins=8, ranges=4.0)
    x = np.random.default_rng(3).standard_normal((T, 1, 1)).astype(np.float32)
    x[2 ** 20 - 2:2 ** 20 + 2] = 1.0                                 # a spell across the launch boundary
    x[5], x[2 ** 20 + 1] = np.nan, np.inf
    acc = Temporal(spec, 1, 1, paired=False, device=DEV).add(torch.from_numpy(x.reshape(T, 1, 1, 1)).to(DEV))
    host = temporal.host_temporal(spec, x)
    same_bits(device_state(acc, 0), host, "2^20 + 3 fields")
    assert host["ramps"].sum() == 2 * T - 4 and host["accnt"][0, 0, 0] == T - 2


def _trainer_epoch(monkeypatch, on, tdir, lr=None):
    import downgan_amd.config.hyperparams as hp
    from downgan_amd import synthetic
    from downgan_amd.GAN import losses
    from downgan_amd.GAN.dataloader import NetCDFSR
    from downgan_amd.GAN.wasserstein import WassersteinGAN
    from downgan_amd.networks.critic import Critic
    from downgan_amd.networks.generator import Generator
    monkeypatch.setattr(hp, "batch_size", 2)
    if lr is not None:
        monkeypatch.setattr(hp, "lr", lr)
    monkeypatch.setattr(losses, "_ops", {})
    torch.manual_seed(0)
    coarse, fine = synthetic.tiles(8, 2, 16, seed=21)
    G, C_ = Generator(16, 128, 2, 2, num_res_blocks=1), Critic(16, 128, 2)
    tr = WassersteinGAN(G, C_)
    tr.log_temporal = on
    tr.temporal_dir = tdir
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 2), batch_size=2)           # one batch
    test = torch.utils.data.DataLoader(ds(2, 8), batch_size=2)            # three batches, in time order
    tr.train(train, test, epochs=1)
    return tr, coarse, fine


def test_trainer_hook(monkeypatch, tmp_path):
    tr, coarse, fine = _trainer_epoch(monkeypatch, True, str(tmp_path / "t"))
    d = tr.metrics_log[0]["temporal"]
    assert set(d) == {"test"} and d["test"]["fields"] == 6
    got = tr.temporal_results["test"]
    assert d["test"] == got.summary()
    spec = TemporalSpec.zscore(2)
    o = tr._engine.ops
    reals, fakes = [], []
    with torch.no_grad():
        for a in range(2, 8, 2):
            fake = tr.G(torch.from_numpy(coarse[a:a + 2]))                    # the generator after the epoch's update
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)  # the real fields as the trainer stages them
            reals.append(xf[..., :2].permute(0, 3, 1, 2).float().contiguous())
            fakes.append(fake.float().to(o.device).contiguous())
    want = temporal.temporal(torch.cat(reals), torch.cat(fakes), spec=spec)    # the concatenated series in one call
    assert got.fields == 6 and got.paired
    for k in ("spells", "cens", "spellmap", "ramps", "accnt"):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
    assert got.acsum.tobytes() == want.acsum.tobytes()
    folder = tmp_path / "t" / "0" / "test"
    names = {f"{s}_{k}.npy" for s in ("real", "fake") for k in ("spell_frequency", "mean_spell", "longest_spell", "autocorrelation",
                                                                "decorrelation_time", "spells", "censored", "ramps")}
    assert set(os.listdir(folder)) == names | {"autocorrelation_bias.npy", "summary.json"}
    for k, v in got.maps().items():
        np.testing.assert_array_equal(np.load(folder / (k + ".npy")), v)


def test_hook_off_leaves_the_epoch_unchanged(monkeypatch):
    """The same epoch with the hook on and off, lr = 0 so that both evaluate identical weights: the summaries hold the same
    keys but for "temporal", and the same metrics up to the order of the fp32 atomic sums behind them (the bound of
    test_gridhist_gpu.test_hook_off_leaves_the_epoch_unchanged: two orders of a sum of N <= 2^16 fp32 terms differ by about
    sqrt(N) 2^-24 sum |term| = 2^-16 sum |term|; 2^-13 is a factor 8 over that estimate)."""
    on, _, _ = _trainer_epoch(monkeypatch, True, None, lr=0.0)
    off, _, _ = _trainer_epoch(monkeypatch, False, None, lr=0.0)
    a, b = dict(on.metrics_log[0]), off.metrics_log[0]
    assert set(a.pop("temporal")) == {"test"}
    assert "temporal" not in b and off.temporal_results is None and set(a) == set(b)
    assert a["epoch"] == b["epoch"] and a["test_batches"] == b["test_batches"]
    for part in ("train", "test"):
        assert set(a[part]) == set(b[part]) and len(a[part]) >= 3
        for k, v in a[part].items():
            np.testing.assert_allclose(v, b[part][k], rtol=2.0 ** -13, atol=2.0 ** -13, err_msg=f"{part} {k}")
