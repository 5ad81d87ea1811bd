"""Distance maps on the GPU (csrc/distmap.hip) against the library's host reference dg_distmap_host (itself pinned to a numpy
restatement and to scipy by test_distmap_cpu): records, ring table and squared distances equal the host's byte for byte over the
pattern zoo and random masks at every grid, every layout and dtype, one series and pairs in different layouts, n_valid, chunking
under a small workspace cap, two runs, rejected calls, the limits against closed forms, and the trainer's opt-in hook."""
import ctypes as C

import numpy as np
import pytest
import torch

from downgan_amd import _lib, distmap
from downgan_amd.distmap import Distances, DistSpec, HostOps
from downgan_amd.histograms import _default_ops, _descriptor

from .test_distmap_cpu import F32, FAR, batch_fields, dot, np_dq, spec3
from .test_histograms_gpu import DEV
from .test_temporal_gpu import layouts

pytestmark = pytest.mark.gpu

HOST = HostOps()


def call(o, spec, a, b=None, kw=None, kwb=None):
    """(records, rings, d2) as numpy arrays of ONE ops.distmap call over whole batches (b None: d2 alone, its side-1 planes
    prefilled with -7)."""
    kw, kwb = kw or {}, kwb or {}
    s = spec.struct()
    xa = a.nhwc if hasattr(a, "nhwc") else a
    nhwc_a = kw.get("nhwc", False) or hasattr(a, "nhwc")
    H, W = xa.shape[1:3] if nhwc_a else xa.shape[2:4]
    T = xa.shape[0]
    ka, fa = _descriptor(o, xa, nhwc_a, spec.C)                      # ka, kb: the tensors the descriptors point into stay alive
    d2 = torch.full((T, 2, spec.nout, spec.K, H * W), -7, dtype=torch.int32, device=o.device)
    if b is None:
        o.distmap(fa, None, H, W, s, d2=d2)
        return (d2.cpu().numpy(),)
    xb = b.nhwc if hasattr(b, "nhwc") else b
    kb, fb = _descriptor(o, xb, kwb.get("nhwc", False) or hasattr(b, "nhwc"), spec.C)
    records = torch.full((T, spec.nout, spec.K, 11), -7, dtype=torch.int64, device=o.device)
    rings = torch.zeros(spec.nout, spec.K, 2, spec.nring + 2, dtype=torch.int64, device=o.device)
    o.distmap(fa, fb, H, W, s, records=records, rings=rings, d2=d2)
    return records.cpu().numpy(), rings.cpu().numpy(), d2.cpu().numpy()


def seen(t, kw):
    """The values the kernel reads, as a float32 NCHW tensor on the host."""
    x = t.nhwc if hasattr(t, "nhwc") else t
    Cn = kw.get("channels", t.channels if hasattr(t, "channels") else None)
    if kw.get("nhwc", False) or hasattr(t, "nhwc"):
        x = x[..., :Cn].permute(0, 3, 1, 2)
    return x.float().cpu().contiguous()


def same(got, want, msg):
    assert len(got) == len(want)
    for g, w, what in zip(got, want, ("records", "rings", "d2") if len(got) == 3 else ("d2",)):
        assert g.dtype == w.dtype and g.shape == w.shape, (msg, what, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (msg, what, np.argwhere(g != w)[:4], g[g != w][:4], w[g != w][:4])


@pytest.mark.parametrize("grid", [(1, 1), (1, 70), (70, 1), (5, 67), (64, 64), (65, 130), (128, 128), (3, 2048), (2048, 3), (40, 1100)])
def test_kernel_against_the_host_reference(grid):
    """The whole zoo, the random masks and two blank fields as ONE batch (17 field pairs, 3 output channels, 2 thresholds), the
    generated side holding the next pattern.  (1, 1) .. (70, 1): one pixel, one row, one column; (5, 67): a ragged wave; (64, 64):
    exactly one wave per row; (65, 130): a row above one wave, columns that divide no block; (128, 128): many workgroups;
    (3, 2048), (2048, 3): the side limit, a row longer than the block, the tallest column; (40, 1100): threads that own more than
    one pixel of a row."""
    H, W = grid
    spec = spec3()
    f = batch_fields(H, W)
    a = torch.from_numpy(np.stack([x for _, x in f]))
    b = torch.from_numpy(np.stack([x for _, x in f[1:] + f[:1]]))
    want = call(HOST, spec, a, b)
    got = call(_default_ops(DEV), spec, a.to(DEV), b.to(DEV))
    same(got, want, f"{grid}")
    rec = want[0].reshape(-1, 11)
    kinds = {(int(r[0] > 0), int(r[1] > 0)) for r in rec}
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)} and rec[:, 2].max() > 0            # pairs of every kind, some overlap
    assert (rec[(rec[:, 0] == 0) | (rec[:, 1] == 0), 3:9] == -1).all() and want[1].sum() == rec[:, 0].sum() + rec[:, 1].sum()


@pytest.mark.parametrize("grid", [(1, 70), (5, 67), (65, 130), (40, 1100)])
def test_one_series(grid):
    """b NULL: the distance transform alone, side 1 of the d2 array untouched."""
    H, W = grid
    spec = spec3()
    a = torch.from_numpy(np.stack([x for _, x in batch_fields(H, W)]))
    got = distmap.distance_transform(a.to(DEV), spec=spec)
    want = distmap.distance_transform(a, spec=spec, ops=HOST)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(a), 3, 2, H, W) and got.cpu().numpy().tobytes() == want.numpy().tobytes()
    assert (want == FAR).any() and (want == 0).any()
    raw = call(_default_ops(DEV), spec, a.to(DEV))[0]
    assert (raw[:, 1] == -7).all() and raw[:, 0].tobytes() == want.numpy().tobytes()


def test_every_layout_and_dtype():
    rng = np.random.default_rng(11)
    T, H, W = 3, 20, 67
    spec = spec3()
    xa, xb = (rng.normal(size=(T, 2, H, W)).astype(F32) * 1.2 for _ in range(2))
    la, lb = layouts(xa), layouts(xb)
    lb = lb[1:] + lb[:1]                                              # the generated series in ANOTHER layout (and dtype)
    o = _default_ops(DEV)
    for (name, t, kw), (bname, tb, kwb) in zip(la, lb):
        want = call(HOST, spec, seen(t, kw), seen(tb, kwb))
        same(call(o, spec, t, tb, kw, kwb), want, f"{name} + {bname}")
        assert want[0][..., :2].min() > 0 and want[0][..., 2].max() > 0 and want[1][..., 1:].sum() > 100
        same(call(o, spec, t, None, kw), call(HOST, spec, seen(t, kw)), f"{name} alone")


def test_n_valid_and_chunking():
    rng = np.random.default_rng(12)
    T, H, W = 5, 33, 70
    spec = spec3()
    a, b = (torch.from_numpy(rng.normal(size=(T, 2, H, W)).astype(F32) * 1.2) for _ in range(2))
    b[3, :] = -5.0                                                    # no generated exceedance in the components of field 3
    whole = distmap.distances(a.to(DEV), b.to(DEV), spec=spec, keep_records=True)
    acc = Distances(spec, H, W, device=DEV, keep_records=True)
    for t in range(T):
        acc.add(a[t:t + 1].to(DEV), b[t:t + 1].to(DEV))
    byfield = acc.result()
    host = distmap.distances(a, b, spec=spec, ops=HOST, keep_records=True)
    assert whole.summary() == byfield.summary() == host.summary() and whole.fields == T
    assert whole.records.tobytes() == byfield.records.tobytes() == host.records.tobytes()
    assert whole.pairs()["real_only"][0, 0] == 1 and whole.pairs()["both"][0, 0] == 4
    cut = Distances(spec, H, W, device=DEV, keep_records=True)
    cut.ws_cap = 2 * (2 * 2 * 3 * 2 * H * W)                          # two fields per call: three calls
    res = cut.add(a.to(DEV), b.to(DEV)).result()
    assert cut.calls == 3 and res.summary() == host.summary() and res.records.tobytes() == host.records.tobytes()
    part = distmap.distances(a.to(DEV), b.to(DEV), spec=spec, n_valid=3, keep_records=True)
    first = distmap.distances(a[:3], b[:3], spec=spec, ops=HOST, keep_records=True)
    assert part.fields == 3 and part.summary() == first.summary() and part.records.tobytes() == first.records.tobytes()


def test_two_runs_give_identical_bytes():
    rng = np.random.default_rng(13)
    spec = spec3(cutoff=32, nring=64)
    a, b = (torch.from_numpy((rng.random((4, 2, 96, 130)) < 0.02).astype(F32) * 2.5).to(DEV) for _ in range(2))
    o = _default_ops(DEV)
    r1, r2 = call(o, spec, a, b), call(o, spec, a, b)
    same(r1, r2, "two runs")
    same(r1, call(HOST, spec, a.cpu(), b.cpu()), "sparse masks")
    assert r1[0][..., 5].max() > 100                                  # sparse masks: long scans


def test_rejected_calls_launch_nothing():
    o = _default_ops(DEV)
    lib = _lib.lib()
    H, W = 6, 10
    spec = spec3()
    x = torch.ones(2, 2, H, W, device=DEV) * 3
    kx, fx = _descriptor(o, x, False, 2)
    ws = torch.empty(o.distmap_ws_bytes(fx, H, W, spec.struct()), dtype=torch.uint8, device=DEV)
    records = torch.full((2, 3, 2, 11), -7, dtype=torch.int64, device=DEV)
    rings = torch.full((3, 2, 2, spec.nring + 2), -7, dtype=torch.int64, device=DEV)
    d2 = torch.full((2, 2, 3, 2, H * W), -7, dtype=torch.int32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def run(a=fx, b=fx, h=H, w=W, s=None, wsp=ptr(ws), rec=ptr(records), ring=ptr(rings), d=ptr(d2)):
        s = spec.struct() if s is None else s
        return lib.dg_distmap(C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, h, w, C.byref(s), wsp,
                              rec, ring, d, o._stream())

    def bad(**kw):
        s = spec.struct()
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    short = _lib.EofFields(base=fx.base, dtype=fx.dtype, T=1, C=fx.C, P=fx.P, ld_t=fx.ld_t, ld_c=fx.ld_c, ld_p=fx.ld_p)
    other = _lib.EofFields(base=fx.base, dtype=7, T=fx.T, C=fx.C, P=fx.P, ld_t=fx.ld_t, ld_c=fx.ld_c, ld_p=fx.ld_p)
    assert run(b=short) == -3 and run(h=W, w=H + 1) == -3 and run(wsp=None) == -3 and run(rec=None, ring=None, d=None) == -3
    assert run(b=None) == -3 and run(b=None, rec=None, ring=None, d=None) == -3 and run(a=None) == -3
    assert run(s=bad(nthr=5)) == -3 and run(s=bad(nring=129)) == -3 and run(s=bad(cutoff=0)) == -3 and run(s=bad(speed_u=2)) == -3
    assert run(b=other) == -2
    torch.cuda.synchronize()
    assert (records == -7).all() and (rings == -7).all() and (d2 == -7).all()
    assert run() == 0                                                 # and the same buffers in a valid call
    torch.cuda.synchronize()
    assert (records[..., :3] == H * W).all() and not records[..., 3:].any() and (d2 == 0).all()


def test_limits_against_the_closed_forms():
    """One 2048 x 2048 field at the largest cutoff and ring count.  A pixel in either far corner: every pixel scans its whole
    row (the scan's worst case), the tallest columns, the largest distance 2 * 2047^2.  Then an empty side against a full one:
    every pixel at the largest |w_A - w_B|, bad2 = 2^60, the largest value a record can hold."""
    N, c = 2048, 512
    spec = DistSpec(1, speed=None, thresholds=(1.0,), cutoff=c, nring=128)
    o = _default_ops(DEV)
    a, b = torch.zeros(1, 1, N, N, device=DEV), torch.zeros(1, 1, N, N, device=DEV)
    a[0, 0, 0, 0] = b[0, 0, N - 1, N - 1] = 2.0
    rec, rings, d2 = call(o, spec, a, b)
    i = np.arange(N, dtype=np.int64)
    want = i[:, None] ** 2 + i[None, :] ** 2
    assert np.array_equal(d2[0, 0, 0, 0].reshape(N, N), want) and np.array_equal(d2[0, 1, 0, 0].reshape(N, N), want[::-1, ::-1])
    far = 2 * (N - 1) ** 2
    n = want << 20
    dq = np.sqrt(n.astype(np.float64)).astype(np.int64)               # a first guess, corrected in integers
    dq -= dq * dq > n
    dq += (dq + 1) * (dq + 1) <= n
    assert dq[N - 1, N - 1] == np_dq(far) and dq[3, 4] == 5120
    w = np.minimum(dq, c * 1024)
    diff = np.abs(w - w[::-1, ::-1])
    assert rec[0, 0, 0].tolist() == [1, 1, 0, np_dq(far), far, far, np_dq(far), far, far, int(diff.sum()), int((diff * diff).sum())]
    assert rings[0, 0, :, 128].tolist() == [1, 1] and rings.sum() == 2
    rec, rings, d2 = call(o, spec, torch.zeros(1, 1, N, N, device=DEV), torch.full((1, 1, N, N), 2.0, device=DEV))
    assert rec[0, 0, 0].tolist() == [0, N * N, 0, -1, -1, -1, -1, -1, -1, N * N * c * 1024, 1 << 60]
    assert rings[0, 0, 0, 129] == N * N and rings.sum() == N * N and (d2[0, 0] == FAR).all() and not d2[0, 1].any()


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
    tr.log_distances = on
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 2), batch_size=2)           # one batch
    test = torch.utils.data.DataLoader(ds(2, 8), batch_size=2)            # three batches
    tr.train(train, test, epochs=1)
    return tr, coarse, fine


def test_trainer_hook(monkeypatch):
    tr, coarse, fine = _trainer_epoch(monkeypatch, True)
    d = tr.metrics_log[0]["distances"]
    assert set(d) == {"train", "test"} and d["test"]["fields"] == 6 and d["train"]["fields"] == 2
    got = tr.distance_results["test"]
    assert d["test"] == got.summary() and d["test"]["channels"] == ["ch0", "ch1", "speed"] and d["test"]["grid"] == [128, 128]
    o = tr._engine.ops
    acc = Distances(DistSpec.zscore(2), 128, 128, device=o.device)
    with torch.no_grad():
        for a in range(2, 8, 2):                                          # the same pairs, batch by batch, by hand
            fake = tr.G(torch.from_numpy(coarse[a:a + 2]))                # the generator after the epoch's update
            xf = o.zeros(2, 128, 128, tr._engine.G.np_p)
            o.nchw_to_nhwc(torch.from_numpy(fine[a:a + 2]).to(o.device), xf)   # the real fields as the trainer stages them
            acc.add(xf[..., :2].permute(0, 3, 1, 2).float().contiguous(), fake.float().to(o.device).contiguous())
    want = acc.result()
    assert d["test"] == want.summary() and sum(map(sum, d["test"]["pixels"]["real"])) > 0
    off, _, _ = _trainer_epoch(monkeypatch, False)
    assert "distances" not in off.metrics_log[0] and off.distance_results is None
