"""Empirical quantile mapping on the GPU (csrc/qmap.hip) against the library's host references, which test_qmap_cpu.py holds
to the numpy definition: the fit kernel on hand-made and random tables in both pixel ownerships, the apply kernel in every
layout and dtype on planted values, determinism, chunking, ``n_valid``, the chain gridhist -> fit -> apply -> gridhist on the
device, and ``Generator.generate(qmap=)``.  Every comparison of nodes and mapped values is of bit patterns."""
import numpy as np
import pytest
import torch

from downgan_amd import gridhist, qmap
from downgan_amd.histograms import HistSpec, _default_ops
from downgan_amd.qmap import QuantileMap

from . import qmap_ref as R
from .test_gridhist_cpu import data, specs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ops():
    return _default_ops(torch.device(DEV))


def device_fit(c, lo, width, offset=False):
    """ops.qmap_fit of the table c (numpy); ``offset``: table and nodes start one element into their allocations, so that no
    row is aligned for 16-byte accesses and the one-pixel path runs whatever P is."""
    nout, _, nb3, P = c.shape
    k = 1 if offset else 0
    cbuf = torch.zeros(c.size + k, dtype=torch.int32, device=DEV)
    counts = cbuf[k:].view(c.shape)
    counts.copy_(torch.from_numpy(c))
    nbuf = torch.full((nout * nb3 * P + k + 64,), 77.0, dtype=torch.float32, device=DEV)
    nodes = nbuf[k:k + nout * nb3 * P].view(nout, nb3, P)
    ops().qmap_fit(counts, lo, width, nodes)
    assert torch.all(nbuf[:k] == 77.0) and torch.all(nbuf[k + nout * nb3 * P:] == 77.0)          # nothing written outside
    return nodes.cpu().numpy()


# ------------------------------------------------------------------------------------------------- fit
@pytest.mark.parametrize("bins", [1, 64, 256])
def test_fit_equals_the_host_reference(bins):
    """P = 1, 5: one ragged wave of the one-pixel path; 252, 1000, 4096: four pixels per lane, the last workgroup ragged, more than
    one workgroup; each again with the table offset by one element (the one-pixel path at every P)."""
    lo, width = R.spec_axes(bins)
    for P in (1, 5, 252, 1000, 4096):
        rng = np.random.default_rng(bins * 10000 + P)
        c = R.random_table(P, bins, rng)
        want = qmap.host_fit(c, lo, width)
        for offset in (False, True):
            np.testing.assert_array_equal(R.bits(device_fit(c, lo, width, offset)), R.bits(want), err_msg=f"random P {P} offset {offset}")


@pytest.mark.parametrize("bins", [1, 2, 64, 256])
def test_fit_of_the_hand_made_tables(bins):
    lo, width = R.spec_axes(bins, nout=3)
    for P in (5, 67, 252):
        c = R.hand_table(P, bins, np.random.default_rng(bins + P), nout=3)
        want = qmap.host_fit(c, lo, width)
        for offset in (False, True):
            np.testing.assert_array_equal(R.bits(device_fit(c, lo, width, offset)), R.bits(want), err_msg=f"hand P {P} offset {offset}")
    np.testing.assert_array_equal(R.bits(want), R.bits(R.fit_ref(c, lo, width)))


# ------------------------------------------------------------------------------------------------- apply
def layouts(x):
    """(name, the tensor the descriptor points into, its eof_fields, the values the kernel reads [T, C, P]) of x float32
    [T, 2, H, W].  The padding of every padded store is NaN and the host reference sees the real channels alone: a padded value
    that is read shows in the comparison."""
    T, Cn, H, W = x.shape
    P = H * W
    o = ops()
    x32 = torch.from_numpy(x).to(DEV)
    xb = x32.to(torch.bfloat16)
    seen32, seen_b = x.reshape(T, Cn, P), xb.float().cpu().numpy().reshape(T, Cn, P)
    pad = torch.full((T, H, W, 16), float("nan"), dtype=torch.bfloat16, device=DEV)           # the generator's store
    pad[..., :Cn] = xb.permute(0, 2, 3, 1)
    three = torch.full((T, H, W, 3), float("nan"), dtype=torch.float32, device=DEV)           # 12-byte pixels: HIST_ANY, ld_c = 1
    three[..., :Cn] = x32.permute(0, 2, 3, 1)
    wide = torch.full((T, Cn + 1, P + 3), float("nan"), dtype=torch.float32, device=DEV)      # strided planes off 16-byte alignment
    wide[:, :Cn, 1:P + 1] = x32.reshape(T, Cn, P)
    return [("nchw_f32", x32, o.eof_fields(x32), seen32),
            ("nchw_bf16", xb, o.eof_fields(xb), seen_b),
            ("nhwc_bf16_padded", pad, o.eof_fields(pad, nhwc=True, channels=Cn), seen_b),
            ("nhwc_f32_any", three, o.eof_fields(three, nhwc=True, channels=Cn), seen32),
            ("strided_f32_any", wide, o.eof_fields(wide[:, :Cn, 1:P + 1]), seen32)]


@pytest.mark.parametrize("grid", [(8, 8), (12, 21), (64, 64)])
@pytest.mark.parametrize("name,spec", specs())
def test_apply_equals_the_host_reference(name, spec, grid):
    """one_bin: 4 rows; affine_speed: 64 bins, an affine transform and the speed; fine: 256 bins, the transfer functions beyond
    64 KiB of LDS.  8 x 8: one workgroup, a full wave; 12 x 21: a ragged last workgroup; 64 x 64: 64 workgroups.  T = 1 and 5
    leave waves without a field, 33 runs the unrolled loop and its tail and is cut into slices."""
    H, W = grid
    P = H * W
    rng = np.random.default_rng(P + spec.bins)
    nodes = qmap.host_fit(R.hand_table(P, spec.bins, rng, spec.nout), spec.lo, spec.width())
    dn = torch.from_numpy(nodes).to(DEV)
    s = spec.struct()
    for T in (1, 5, 33):
        x = data(rng, spec, T, H, W)
        for lname, keep, f, seen in layouts(x):
            want = qmap.host_apply(spec, seen, nodes)
            out = torch.full((T * spec.nout * P + 64,), 77.0, dtype=torch.float32, device=DEV)
            ops().qmap_apply(f, s, dn, out[:T * spec.nout * P])
            assert torch.all(out[T * spec.nout * P:] == 77.0), (lname, T)
            got = out[:T * spec.nout * P].view(T, spec.nout, P).cpu().numpy()
            np.testing.assert_array_equal(R.bits(got), R.bits(want), err_msg=f"{name} {grid} T {T} {lname}")


def test_bin_counts_around_the_64_kib_boundary_in_any_order():
    """The apply kernel opts in to more than 64 KiB of dynamic LDS once per kernel instance and device.  253 bins stay below the
    boundary; 254 (65792 B) is the first call above it, 255 and 256 (66304 B) follow on the SAME instance and need more than that
    first call did.  The instance is float x one 16-byte load per pixel ([T, H, W, 4] fp32), which no other test of this file
    launches, so the order here is the order the process sees."""
    T, H, W = 5, 12, 21
    P = H * W
    rng = np.random.default_rng(254)
    x = (rng.standard_normal((T, 2, H, W)) * 2).astype(np.float32)
    four = torch.full((T, H, W, 4), float("nan"), dtype=torch.float32, device=DEV)
    four[..., :2] = torch.from_numpy(x).to(DEV).permute(0, 2, 3, 1)
    f = ops().eof_fields(four, nhwc=True, channels=2)
    for bins in (253, 254, 255, 256, 254):
        spec = HistSpec(bins, [-4.0, -4.0], [4.0, 4.0], speed=None)
        nodes = qmap.host_fit(R.random_table(P, bins, rng), spec.lo, spec.width())
        out = torch.empty(T, 2, P, dtype=torch.float32, device=DEV)
        ops().qmap_apply(f, spec.struct(), torch.from_numpy(nodes).to(DEV), out)
        np.testing.assert_array_equal(R.bits(out.cpu().numpy()), R.bits(qmap.host_apply(spec, x.reshape(T, 2, P), nodes)), err_msg=f"bins {bins}")


def pair(T, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    real = torch.randn(T, 2, H, W, generator=g)
    fake = 0.4 + 1.3 * torch.randn(T, 2, H, W, generator=g)
    return real.to(DEV), fake.to(DEV)


def test_two_calls_chunks_and_n_valid():
    T, H, W = 33, 24, 20
    spec = HistSpec.zscore(2, bins=64, lim=6.0)
    real, fake = pair(T, H, W)
    fake[3, 0, 2, 5] = float("nan")
    m, m2 = (qmap.quantile_map(real, fake, spec=spec) for _ in range(2))
    assert m.nodes.is_cuda and m.valid.is_cuda and m.fields == T and torch.equal(m.nodes.view(torch.int32), m2.nodes.view(torch.int32))
    table = gridhist.host_table(spec, real.reshape(T, 2, -1).cpu().numpy(), fake.reshape(T, 2, -1).cpu().numpy())
    np.testing.assert_array_equal(R.bits(m.nodes.cpu().numpy()), R.bits(qmap.host_fit(table, spec.lo, spec.width())))
    full = m.apply(fake)
    assert full.shape == (T, 3, H, W) and full.is_cuda and torch.equal(full.view(torch.int32), m.apply(fake).view(torch.int32))
    np.testing.assert_array_equal(R.bits(full.cpu().numpy().reshape(T, 3, -1)),
                                  R.bits(qmap.host_apply(spec, fake.reshape(T, 2, -1).cpu().numpy(), m.nodes.cpu().numpy())))
    for chunk in (1, 5, 33):
        parts = torch.cat([m.apply(fake[i:i + chunk]) for i in range(0, T, chunk)])
        assert torch.equal(parts.view(torch.int32), full.view(torch.int32)), chunk
    keep = torch.full((T, 3, H, W), 7.0, device=DEV)
    part = m.apply(fake, n_valid=13, out=keep)
    assert part.shape == (13, 3, H, W) and torch.all(keep[13:] == 7.0) and torch.equal(keep[:13].view(torch.int32), full[:13].view(torch.int32))
    pad = torch.full((T, H, W, 16), float("nan"), dtype=torch.bfloat16, device=DEV)
    pad[..., :2] = fake.permute(0, 2, 3, 1)
    seen = pad[..., :2].permute(0, 3, 1, 2).float().contiguous()
    assert torch.equal(m.apply(pad, nhwc=True, channels=2).view(torch.int32), m.apply(seen).view(torch.int32))
    assert torch.equal(m.apply(fake.cpu()).view(torch.int32), full.cpu().view(torch.int32))        # a CPU batch: the host reference


@pytest.fixture(scope="module")
def chain():
    """gridhist -> QuantileMap.fit -> apply -> gridhist(real, corrected) -> QuantileMap.fit, all on the device: 32 x 32, T = 64."""
    T, H, W = 64, 32, 32
    spec = HistSpec(64, [-6.0, -6.0], [6.0, 6.0], speed=None)
    real, fake = pair(T, H, W)
    before = gridhist.gridhist(real, fake, spec=spec)
    m = QuantileMap.fit(before)
    corrected = m.apply(fake)
    after = gridhist.gridhist(real, corrected, spec=spec)
    return spec, before, m, after, QuantileMap.fit(after)


def test_mapping_on_the_device_lowers_the_pooled_w1(chain):
    spec, before, m, after, again = chain
    assert m.valid.all() and after.fields == before.fields == 64
    w_before, w_after = before.w1().mean(), after.w1().mean()
    print(f"pooled binned W1 before {w_before:.4f}, after {w_after:.4f}")
    assert w_after < w_before


def test_refitting_after_the_mapping_gives_the_identity_within_one_node_bin(chain):
    """The second fit is the identity to within one node's bin: a corrected value of generated bin i lies between the first map's
    nodes n_i and n_{i+1}, so the corrected cumulative count at a real edge e lies between the generated counts at the two first-map
    nodes L <= e <= U that enclose e, whose real quantiles are L and U themselves; with the binning of the second table the
    refitted node of e lies in [L - w, U + w].  (It is NOT within one bin WIDTH of e everywhere: with 64 fields per pixel the node
    intervals of the tails are many bins wide, and on the host reference 8629 of the 133120 nodes of this chain lie further than w
    from their edge, up to 18.5 w -- a property of the definition's "nearest point of the flat interval", not of the kernels.)"""
    spec, before, m, after, again = chain
    edges, n1 = m.transfer()
    _, n2 = again.transfer()
    valid = (m.valid & again.valid).cpu().numpy()
    w = spec.width()
    worst, worst_narrow, narrow, total = 0.0, 0.0, 0, 0
    for j in range(spec.nout):
        a, b = n1[j].reshape(spec.bins + 1, -1), n2[j].reshape(spec.bins + 1, -1)
        e = edges[j][:, None]
        L = np.where(a[None, :, :] <= e[:, None, :], a[None, :, :], -np.inf).max(axis=1)          # [edge, P]
        U = np.where(a[None, :, :] >= e[:, None, :], a[None, :, :], np.inf).min(axis=1)
        L, U = np.where(np.isfinite(L), L, e), np.where(np.isfinite(U), U, e)
        ok = valid[j].reshape(-1)
        dev = np.maximum(np.maximum(L - w[j] - b, b - U - w[j]), 0)[:, ok]
        worst = max(worst, float(dev.max()) / w[j])
        # where the first map's node interval around e is itself at most one bin wide, both readings of "one node's bin" agree:
        # there the refitted node lies within w of its edge
        tight = ((U - L) <= w[j] * (1 + 1e-6))[:, ok]
        narrow += int(tight.sum())
        total += tight.size
        worst_narrow = max(worst_narrow, float((np.abs(b - e)[:, ok][tight]).max()) / w[j])
    print(f"largest excursion beyond the enclosing node interval + w: {worst:.3g} w; "
          f"nodes further than w from their edge: {(np.abs(n2 - edges[:, :, None, None]) > w[:, None, None, None] * (1 + 1e-6)).sum()} of {n2.size}")
    print(f"edges whose first-map node interval is at most w: {narrow} of {total}; largest |node - edge| there: {worst_narrow:.3g} w")
    assert worst <= 1e-5                                              # fp32 nodes against float64 edges
    assert narrow >= total // 2 and worst_narrow <= 1 + 1e-5          # and that is no empty statement: most edges are such


def test_generate_with_a_map_equals_mapping_the_generated_fields():
    from downgan_amd import synthetic
    from downgan_amd.networks.generator import Generator
    coarse, fine = synthetic.tiles(3, 2, 16, seed=11)
    coarse, fine = torch.from_numpy(coarse), torch.from_numpy(fine)
    G = Generator(16, 128, 2, 2, num_res_blocks=1)
    plain = G.generate(coarse[:3], 2)
    spec = HistSpec(64, [-6.0, -6.0], [6.0, 6.0], speed=None)
    m = qmap.quantile_map(fine.to(DEV), plain.to(DEV), spec=spec)
    mapped = G.generate(coarse[:3], chunk_size=2, qmap=m)
    assert mapped.shape == plain.shape == (3, 2, 128, 128) and not mapped.is_cuda
    assert torch.equal(mapped.view(torch.int32), m.apply(plain).view(torch.int32)) and not torch.equal(mapped, plain)
    assert torch.equal(G.generate(coarse[:3], 2, qmap=None).view(torch.int32), plain.view(torch.int32))
