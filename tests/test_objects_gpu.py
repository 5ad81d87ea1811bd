"""Exceedance objects on the GPU (csrc/objects.hip) against the library's host reference dg_objects_host (itself pinned to a numpy
restatement and to scipy by test_objects_cpu): the sorted device table equals the host table byte for byte over the pattern zoo
and random masks at every grid, both connectivities, every layout and dtype, one series and pairs in different layouts, n_valid,
chunking, the growth of a table that was too small, two runs, the limits against closed forms, and the trainer's opt-in hook."""
import numpy as np
import pytest
import torch

from downgan_amd import objects
from downgan_amd.histograms import _default_ops, _descriptor
from downgan_amd.objects import HostOps, Objects, ObjectSpec

from .test_histograms_gpu import DEV
from .test_objects_cpu import F32, TOP, spec3, zoo, zoo_fields
from .test_temporal_gpu import layouts

pytestmark = pytest.mark.gpu

HOST = HostOps()


def tables(o, spec, a, b=None, kw=None, kwb=None, capacity=None):
    """(table, per_plane, calls) as numpy arrays of one HipOps.objects / HostOps.objects call over whole batches."""
    kw, kwb = kw or {}, kwb or {}
    s = spec.struct()
    xa = a.nhwc if hasattr(a, "nhwc") else a
    nhwc_a = kw.get("nhwc", False) or hasattr(a, "nhwc")
    H, W = xa.shape[1:3] if nhwc_a else xa.shape[2:4]
    ka, fa = _descriptor(o, xa, nhwc_a, spec.C)                      # ka, kb: the tensors the descriptors point into stay alive
    kb, fb = None, None
    if b is not None:
        xb = b.nhwc if hasattr(b, "nhwc") else b
        kb, fb = _descriptor(o, xb, kwb.get("nhwc", False) or hasattr(b, "nhwc"), spec.C)
    args = {} if capacity is None else {"capacity": capacity}
    t, pp, calls = o.objects(fa, fb, H, W, s, **args)
    return t.cpu().numpy(), pp.cpu().numpy(), calls


def seen(t, kw):
    """The values the kernel reads, as a float32 NCHW tensor on the host."""
    x = t.nhwc if hasattr(t, "nhwc") else t
    Cn = kw.get("channels", t.channels if hasattr(t, "channels") else None)
    if kw.get("nhwc", False) or hasattr(t, "nhwc"):
        x = x[..., :Cn].permute(0, 3, 1, 2)
    return x.float().cpu().contiguous()


def same(got, want, msg):
    (gt, gp, _), (wt, wp, _) = got, want
    assert gt.dtype == wt.dtype == np.int64 and gt.shape == wt.shape, (msg, gt.shape, wt.shape)
    bad = (gt != wt).any(1)
    assert gt.tobytes() == wt.tobytes(), (msg, gt[bad][:4], wt[bad][:4])
    assert gp.tobytes() == wp.tobytes(), msg


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("grid", [(1, 1), (1, 70), (70, 1), (5, 67), (64, 64), (65, 130), (128, 128)])
def test_kernel_against_the_host_reference(grid, conn):
    """The whole zoo and the random masks as ONE batch (15 field pairs, 3 output channels, 2 thresholds: 180 planes), the
    generated side holding the next pattern.  (1, 1) .. (70, 1): one pixel, one row, one column; (5, 67): a ragged second chunk
    of every row; (64, 64): exactly one chunk; (65, 130): three chunks, the last of two pixels; (128, 128): many workgroups."""
    H, W = grid
    spec = spec3(conn)
    f = zoo_fields(H, W)
    a = torch.from_numpy(np.stack([x for _, x in f]))
    b = torch.from_numpy(np.stack([x for _, x in f[1:] + f[:1]]))
    want = tables(HOST, spec, a, b)
    got = tables(_default_ops(DEV), spec, a.to(DEV), b.to(DEV))
    same(got, want, f"{grid} {conn}")
    assert len(want[0]) > 0 and want[1].sum() == len(want[0])
    one = tables(_default_ops(DEV), spec, a.to(DEV))                 # b NULL: no overlap, side 1 empty
    same(one, tables(HOST, spec, a), f"{grid} {conn} alone")
    assert not one[0][:, 3].any() and not one[1].reshape(-1, 2, 6)[:, 1].any()


def test_every_layout_and_dtype():
    rng = np.random.default_rng(11)
    T, H, W = 3, 20, 67
    spec = spec3(8)
    xa, xb = (rng.normal(size=(T, 2, H, W)).astype(F32) * 1.5 for _ in range(2))
    la, lb = layouts(xa), layouts(xb)
    lb = lb[1:] + lb[:1]                                              # the generated series in ANOTHER layout (and dtype)
    o = _default_ops(DEV)
    for (name, t, kw), (bname, tb, kwb) in zip(la, lb):
        want = tables(HOST, spec, seen(t, kw), seen(tb, kwb))
        same(tables(o, spec, t, tb, kw, kwb), want, f"{name} + {bname}")
        assert len(want[0]) > 100 and want[0][:, 3].max() > 0


def test_n_valid_and_chunking():
    rng = np.random.default_rng(12)
    T, H, W = 5, 33, 70
    spec = spec3(4, min_area=2)
    a, b = (torch.from_numpy(rng.normal(size=(T, 2, H, W)).astype(F32) * 1.5) for _ in range(2))
    whole = objects.objects(a.to(DEV), b.to(DEV), spec=spec, keep_records=True)
    acc = Objects(spec, H, W, device=DEV, keep_records=True)
    for t in range(T):
        acc.add(a[t:t + 1].to(DEV), b[t:t + 1].to(DEV))
    byfield = acc.result()
    host = objects.objects(a, b, spec=spec, ops=HOST, keep_records=True)
    assert whole.summary() == byfield.summary() == host.summary() and whole.fields == T
    assert whole.records.tobytes() == byfield.records.tobytes() == host.records.tobytes() and len(host.records) > 500
    for k, v in whole.sal_pairs().items():
        assert v.tobytes() == byfield.sal_pairs()[k].tobytes() == host.sal_pairs()[k].tobytes(), k
    part = objects.objects(a.to(DEV), b.to(DEV), spec=spec, n_valid=3, keep_records=True)
    first = objects.objects(a[:3], b[:3], spec=spec, ops=HOST, keep_records=True)
    assert part.fields == 3 and part.summary() == first.summary() and part.records.tobytes() == first.records.tobytes()


def test_a_table_that_is_too_small_grows():
    """The 64 x 64 checkerboard at connectivity 4: 2048 one-pixel objects per plane, 4096 in the pair, into 16 rows."""
    spec = ObjectSpec(1, speed=None, thresholds=(1.0,), connectivity=4, quantum=0.5)
    board = zoo(64, 64)["checkerboard"]
    a = torch.from_numpy(np.where(board, 3.0, 0.0).astype(F32)[None, None])
    b = torch.from_numpy(np.where(~board, 2.0, 0.0).astype(F32)[None, None])
    o = _default_ops(DEV)
    ka, fa = _descriptor(o, a.to(DEV), False, 1)                      # ka, kb keep the device copies alive
    kb, fb = _descriptor(o, b.to(DEV), False, 1)
    table = torch.full((16 + 4, 12), -7, dtype=torch.int64, device=DEV)
    count, per_plane = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV)
    o.objects_raw(fa, fb, 64, 64, spec.struct(), table[:16], count, per_plane)
    assert int(count) == 4096 and per_plane.tolist() == [2048, 2048]     # the true count from the first call
    assert (table[16:] == -7).all()                                     # nothing beyond the capacity
    got = tables(o, spec, a.to(DEV), b.to(DEV), capacity=16)
    assert got[2] == 2                                                  # one call to learn the count, one to fill the table
    want = tables(HOST, spec, a, b)
    same(got, want, "grown")
    assert len(got[0]) == 4096 and (got[0][:, 2] == 1).all() and not got[0][:, 3].any() and set(got[0][:2048, 4]) == {6}
    exact = tables(o, spec, a.to(DEV), b.to(DEV), capacity=4096)
    assert exact[2] == 1
    same(exact, want, "capacity == count")


def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(13)
    spec = spec3(8)
    a, b = (torch.from_numpy((rng.random((4, 2, 96, 130)) < 0.59).astype(F32) * 2.5).to(DEV) for _ in range(2))
    o = _default_ops(DEV)
    r1, r2 = tables(o, spec, a, b), tables(o, spec, a, b)
    same(r1, r2, "two runs")
    same(r1, tables(HOST, spec, a.cpu(), b.cpu()), "percolation")
    assert r1[0][:, 2].max() > 1000                                   # a spanning cluster


def test_limits_against_the_closed_forms():
    """One 2048 x 2048 plane, all set, every q saturated: the largest sums a record can hold."""
    N = 2048
    spec = ObjectSpec(1, speed=None, thresholds=(0.0,), connectivity=4, quantum=2.0 ** -10)
    x = torch.full((1, 1, N, N), 1e30, device=DEV)
    table, per_plane, _ = tables(_default_ops(DEV), spec, x)
    moment = TOP * N * (N * (N - 1) // 2)
    assert table.tolist() == [[0, 0, N * N, 0, N * N * TOP, moment, moment, TOP, 0, N - 1, 0, N - 1]]
    assert per_plane.tolist() == [1, 0] and moment < 1 << 57


def _trainer_epoch(monkeypatch, on):
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
    tr.log_objects = on
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 2), batch_size=2)           # one batch
    test = torch.utils.data.DataLoader(ds(2, 8), batch_size=2)            # three batches
    tr.train(train, test, epochs=1)
    return tr, coarse, fine


def test_trainer_hook(monkeypatch):
    tr, coarse, fine = _trainer_epoch(monkeypatch, True)
    d = tr.metrics_log[0]["objects"]
    assert set(d) == {"train", "test"} and d["test"]["fields"] == 6 and d["train"]["fields"] == 2
    got = tr.objects_results["test"]
    assert d["test"] == got.summary() and d["test"]["channels"] == ["ch0", "ch1", "speed"] and d["test"]["grid"] == [128, 128]
    o = tr._engine.ops
    acc = Objects(ObjectSpec.zscore(2), 128, 128, device=o.device)
    with torch.no_grad():
        for a in range(2, 8, 2):                                          # the same pairs, batch by batch, by hand
            fake = tr.G(torch.from_numpy(coarse[a:a + 2]))                # the generator after the epoch's update
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)   # the real fields as the trainer stages them
            acc.add(xf[..., :2].permute(0, 3, 1, 2).float().contiguous(), fake.float().to(o.device).contiguous())
    want = acc.result()
    assert d["test"] == want.summary() and sum(map(sum, d["test"]["count"]["real"])) > 0
    for k, v in want.sal_pairs().items():
        assert v.tobytes() == got.sal_pairs()[k].tobytes(), k
    off, _, _ = _trainer_epoch(monkeypatch, False)
    assert "objects" not in off.metrics_log[0] and off.objects_results is None
