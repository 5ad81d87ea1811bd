"""Per-gridpoint histograms on the GPU (csrc/gridhist.hip) against the numpy definition and the library's host references:
the exact table in every layout, one series and pairs in different layouts and dtypes, determinism and chunked accumulation,
the scan kernel on those tables and on hand-made ones, the largest table the limits allow at a small grid, and the trainer's
opt-in hook.  Every comparison of counts, ranks and distances is exact."""
import os

import numpy as np
import pytest
import torch

from downgan_amd import gridhist, histograms
from downgan_amd.gridhist import GridHist, GridHistMaps
from downgan_amd.histograms import HistSpec

from .test_gridhist_cpu import Q3, Q16, cube, data, hand_tables, scan_ref, specs, table_ref
from .test_histograms_cpu import F32
from .test_histograms_gpu import DEV, layouts, planar  # noqa: F401  (planar: the order seen_cube undoes)

pytestmark = pytest.mark.gpu


def seen_cube(seen, T):
    """[C, T*P] (the order of test_histograms_gpu.planar) -> [C, T, P]."""
    return seen.reshape(seen.shape[0], T, -1)


def as_host(seen, T):
    """[C, T*P] -> the [T, C, P] host_table takes."""
    return np.ascontiguousarray(seen_cube(seen, T).transpose(1, 0, 2))


def check_scan(m, q, what):
    """The device scan of the table of m against the numpy reference and the library's host reference."""
    t = m.table()
    ranks, dist = m.scan(q)
    want_r, want_d = scan_ref(t, list(q))
    host_r, host_d = gridhist.host_scan(t, q)
    np.testing.assert_array_equal(ranks, want_r, err_msg=f"ranks {what}")
    np.testing.assert_array_equal(ranks, host_r, err_msg=f"ranks vs host {what}")
    if m.paired:
        np.testing.assert_array_equal(dist, want_d, err_msg=f"dist {what}")
        np.testing.assert_array_equal(dist, host_d, err_msg=f"dist vs host {what}")
    else:
        assert dist is None and want_d is None and host_d is None


@pytest.mark.parametrize("shape", [(1, 7, 13), (3, 40, 37), (40, 64, 64), (300, 16, 16)])
def test_exact_table_in_every_layout(shape):
    """(1, 7, 13): P no multiple of 4, element-wise loads, a ragged last wave; (3, 40, 37): the tail of the four-pixel mode;
    (40, 64, 64) and (300, 16, 16): the fields split over workgroups that add into shared addresses."""
    T, H, W = shape
    for sname, spec in specs():
        rng = np.random.default_rng(H * W)
        xa, xb = data(rng, spec, T, H, W), data(rng, spec, T, H, W, shift=3)
        la, lb = layouts(xa), layouts(xb)
        refs = {}
        for i, (name, t, kw, seen) in enumerate(la):
            m = gridhist.gridhist(t, spec=spec, **kw)
            assert m.fields == T and not m.paired
            key = ("one", seen.tobytes())
            if key not in refs:
                refs[key] = table_ref(spec, seen_cube(seen, T))
                np.testing.assert_array_equal(gridhist.host_table(spec, as_host(seen, T)), refs[key], err_msg=f"host {shape} {sname}")
            np.testing.assert_array_equal(m.table(), refs[key], err_msg=f"{shape} {name} {sname}")
            # paired, the generated series in ANOTHER layout (and dtype) than the real one
            bname, tb, kwb, seen_b = lb[(i + 1) % len(lb)]
            nhwc = (kw.get("nhwc", False), kwb.get("nhwc", False))
            m = gridhist.gridhist(t, tb, spec=spec, nhwc=nhwc, channels=kw.get("channels", kwb.get("channels")))
            assert m.fields == T and m.paired
            want = table_ref(spec, seen_cube(seen, T), seen_cube(seen_b, T))
            np.testing.assert_array_equal(m.table(), want, err_msg=f"{shape} {name} + {bname} {sname}")
            if i == 0:
                np.testing.assert_array_equal(gridhist.host_table(spec, as_host(seen, T), as_host(seen_b, T)), want)
                check_scan(m, Q3, f"{shape} {name} + {bname} {sname}")
                check_scan(gridhist.gridhist(t, spec=spec, **kw), Q16 if T == 1 else [0.5], f"{shape} {name} {sname} one series")
        # and the same layout on both sides (four pixels per thread where the planes allow it)
        for (name, t, kw, seen), (_, tb, _, seen_b) in zip(la, lb):
            m = gridhist.gridhist(t, tb, spec=spec, **kw)
            np.testing.assert_array_equal(m.table(), table_ref(spec, seen_cube(seen, T), seen_cube(seen_b, T)),
                                          err_msg=f"{shape} {name} x 2 {sname}")


def test_two_calls_are_bit_identical_and_chunks_add_up():
    T, H, W = 24, 96, 80
    spec = specs()[1][1]
    rng = np.random.default_rng(7)
    xa, xb = data(rng, spec, T, H, W), data(rng, spec, T, H, W, shift=1)
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    for pair in (False, True):
        args = (a, b) if pair else (a,)
        p, q = gridhist.gridhist(*args, spec=spec), gridhist.gridhist(*args, spec=spec)
        assert p.table().tobytes() == q.table().tobytes()
    full = p.table()
    np.testing.assert_array_equal(full, gridhist.host_table(spec, xa.reshape(T, 2, -1), xb.reshape(T, 2, -1)))
    acc = GridHist(spec, H, W, paired=True, device=DEV)
    junk = torch.full((3, 2, H, W), 9.0, device=DEV)
    acc.add(a[:7], b[:7]).add(torch.cat([a[7:], junk]), torch.cat([b[7:], junk]), n_valid=17)      # n_valid < T: the leading fields
    assert acc.fields == 24 and acc.nbytes == full.nbytes
    np.testing.assert_array_equal(acc.result().table(), full, err_msg="chunks 7 + 17")
    one = GridHist(spec, H, W, paired=True, device=DEV)
    for t in range(T):
        one.add(a[t:t + 1], b[t:t + 1])
    np.testing.assert_array_equal(one.result().table(), full, err_msg="chunks 24 x 1")


def test_padded_channels_never_reach_the_table():
    """The padding channels of the NHWC store hold 7.0 (test_histograms_gpu.layouts): with speed = (1, 0) and every range
    ending below 7, any padded value read would show in an overflow row."""
    T, H, W = 6, 24, 20
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((T, 2, H, W))).astype(F32).clip(-6, 6)
    spec = HistSpec(64, [-6.5, -6.5, 0.0], [6.5, 6.5, 9.5], speed=(1, 0))
    for name, t, kw, seen in layouts(x)[2:]:
        m = gridhist.gridhist(t, t, spec=spec, **kw)
        tab = m.table()
        np.testing.assert_array_equal(tab, table_ref(spec, seen_cube(seen, T), seen_cube(seen, T)), err_msg=name)
        assert tab[:, :, 65:].sum() == 0 and tab[:, :, 0].sum() == 0
        assert np.all(m.w1() == 0) and np.all(m.ks() == 0) and np.all(m.quantile_bias(Q3) == 0)


@pytest.mark.parametrize("P", [1, 5, 64, 4099])
def test_scan_of_hand_made_tables(P):
    """The hand-made tables of the CPU tests, uploaded: one pixel per lane and its ragged wave (1, 5, 4099: more than one
    workgroup per output channel), four pixels per lane (64); S = 1 without dist and S = 2 with it; Q = 1, 3, 16."""
    for name, c in hand_tables(P):
        nout, bins = c.shape[0], c.shape[2] - 3
        spec = HistSpec(bins, [0.0] * nout, [1.0] * nout, speed=None)
        for q in ([0.5], Q3, Q16):
            pair = GridHistMaps(spec, 1, P, True, torch.from_numpy(c).to(DEV), 1)
            check_scan(pair, q, f"{name} P = {P} Q = {len(q)}")
            one = GridHistMaps(spec, 1, P, False, torch.from_numpy(c[:, 1:].copy()).to(DEV), 1)
            check_scan(one, q, f"{name} P = {P} Q = {len(q)} one series")


def test_largest_table_at_a_small_grid():
    """bins = 256, nout = 9 (eight channels plus the speed), P = 32 x 32, T = 5: the table, the scan, and the pooled counts
    against ``histograms.histogram`` of the same tensors."""
    T, H, W = 5, 32, 32
    rng = np.random.default_rng(8)
    spec = HistSpec(256, [-8.0] * 8 + [0.0], [8.0] * 8 + [12.0], scale=np.linspace(0.5, 2, 8), offset=np.linspace(-1, 1, 8),
                    speed=(6, 1))
    assert spec.nout == 9
    xa, xb = (rng.standard_normal((T, 8, H, W)) * 4).astype(F32), (rng.standard_normal((T, 8, H, W)) * 4).astype(F32)
    xa[0, 3, 0, 0], xb[1, 6, 1, 1] = np.nan, np.inf
    a, b = torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)
    nhwc = b.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)        # 8 bf16 channels: one 16-byte load per pixel
    sn = nhwc.permute(0, 3, 1, 2).float().cpu().numpy()
    for what, m, sa, sb in (("nchw x 2", gridhist.gridhist(a, b, spec=spec), xa, xb),
                            ("nchw + nhwc bf16", gridhist.gridhist(a, nhwc, spec=spec, nhwc=(False, True)), xa, sn),
                            ("nhwc bf16 x 2", gridhist.gridhist(nhwc, nhwc, spec=spec, nhwc=True), sn, sn)):
        assert m.counts.shape == (9, 2, 259, H * W)
        want = gridhist.host_table(spec, sa.reshape(T, 8, -1), sb.reshape(T, 8, -1))
        np.testing.assert_array_equal(m.table(), want, err_msg=what)
        np.testing.assert_array_equal(want, table_ref(spec, cube(sa), cube(sb)), err_msg=what)
        check_scan(m, Q16, what)
        for side, t, kw in (("real", nhwc if sa is sn else a, {"nhwc": sa is sn}), ("fake", nhwc if sb is sn else b, {"nhwc": sb is sn})):
            np.testing.assert_array_equal(m.pooled(side), histograms.histogram(t, spec, **kw).host()[0], err_msg=f"pooled {what} {side}")
    one = gridhist.gridhist(a, spec=spec)
    np.testing.assert_array_equal(one.table(), gridhist.host_table(spec, xa.reshape(T, 8, -1)))
    check_scan(one, Q3, "one series")


def _trainer_epoch(monkeypatch, on, qdir, lr=None):
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
    tr.log_quantile_maps = on
    tr.quantile_map_dir = qdir
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 2), batch_size=2)           # one batch
    test = torch.utils.data.DataLoader(ds(2, 8), batch_size=2)            # three batches
    tr.train(train, test, epochs=1)
    return tr, coarse, fine


def test_trainer_hook(monkeypatch, tmp_path):
    tr, coarse, fine = _trainer_epoch(monkeypatch, True, str(tmp_path / "q"))
    d = tr.metrics_log[0]["quantile_maps"]
    assert d["train"]["fields"] == 2 and d["test"]["fields"] == 6
    got = tr.quantile_map_results["test"]
    assert d["test"] == got.summary((0.5, 0.95, 0.99))
    spec = HistSpec.zscore(2, bins=64, lim=6.0)
    o = tr._engine.ops
    reals, fakes = [], []
    with torch.no_grad():
        for a in range(2, 8, 2):
            fake = tr.G(torch.from_numpy(coarse[a:a + 2]))                    # the generator after the epoch's update
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)  # the real fields as the trainer stages them
            reals.append(xf[..., :2].permute(0, 3, 1, 2).float().cpu().numpy())
            fakes.append(fake.float().cpu().numpy())
    ra, fa = np.concatenate(reals), np.concatenate(fakes)
    assert got.fields == 6 and got.paired and got.counts.is_cuda
    np.testing.assert_array_equal(got.table(), gridhist.host_table(spec, ra.reshape(6, 2, -1), fa.reshape(6, 2, -1)))
    check_scan(got, (0.5, 0.95, 0.99), "trainer hook")
    assert d["test"]["nan"] == {"real": [0, 0, 0], "fake": [0, 0, 0]}
    for part in ("train", "test"):
        folder = tmp_path / "q" / "0" / part
        assert os.path.exists(folder / "summary.json")
        for k, v in tr.quantile_map_results[part].maps((0.5, 0.95, 0.99)).items():
            np.testing.assert_array_equal(np.load(folder / (k + ".npy")), v)


def test_hook_off_leaves_the_epoch_unchanged(monkeypatch):
    """The same epoch with the hook on and off, lr = 0 so that both evaluate identical weights: the summaries hold the same
    keys but for "quantile_maps", and the same metrics up to the order of the fp32 atomic sums behind them (the deterministic
    mode does not cover the metric kernels' atomics).  Two orders of a sum of N <= 2^16 fp32 terms, each rounding of relative size
    u = 2^-24 and of either sign, differ by about sqrt(N) u sum |term| = 2^-16 sum |term|; every metric is a mean of terms of
    magnitude O(1) or below, so 2^-13 (a factor 8 over that estimate) bounds the difference relatively for the sums of one
    sign (MAE, MSE, MSSSIM) and absolutely for Wass."""
    on, _, _ = _trainer_epoch(monkeypatch, True, None, lr=0.0)
    off, _, _ = _trainer_epoch(monkeypatch, False, None, lr=0.0)
    a, b = dict(on.metrics_log[0]), off.metrics_log[0]
    assert set(a.pop("quantile_maps")) == {"train", "test"}
    assert "quantile_maps" not in b and off.quantile_map_results is None and set(a) == set(b)
    assert a["epoch"] == b["epoch"] and a["test_batches"] == b["test_batches"]
    for part in ("train", "test"):
        assert set(a[part]) == set(b[part]) and len(a[part]) >= 3
        for k, v in a[part].items():
            np.testing.assert_allclose(v, b[part][k], rtol=2.0 ** -13, atol=2.0 ** -13, err_msg=f"{part} {k}")
