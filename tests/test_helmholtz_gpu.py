"""Helmholtz spectra on the GPU (csrc/spectra.hip, dg_helmholtz / dg_helmholtz_cross) against the float64 definition: plane
waves with known answers up to N = 2048 (the Nyquist lines included), purely rotational, purely divergent and mixed flows built
from potentials through three layout pairs, the identities that tie the planes to each other, to the one-sided call and to
``cross_rapsd``, the in-workgroup multi-batch loop, chunking and accumulation, the per-part effective resolution end to end, and
the trainer's opt-in hook.

Tolerance: every plane within 1e-4 of the float64 reference RELATIVE TO THE RING'S KINETIC ENERGY (the co-planes: to
sqrt(ke_a ke_b)), never relative to rot or div themselves, which vanish for pure flows.  torch's fp32 fft2 on the CPU stays within
5e-7 of float64 in that measure on these inputs (asserted <= 1e-5 in the multi-batch test), so 1e-4 leaves two orders of margin."""
import functools

import numpy as np
import pytest
import torch

from downgan_amd import spectra

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4


# ------------------------------------------------------------------------------------------------ the float64 definition
def ring_index(N):
    f = np.fft.fftfreq(N) * N
    return np.floor(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2) + 0.5).astype(int)


def _ring_means(planes, N):
    K = N // 2 + 1
    k = ring_index(N).ravel()
    cnt = np.bincount(k)[:K]
    flat = planes.reshape(-1, N * N)
    out = np.stack([np.bincount(k, weights=p)[:K] / cnt for p in flat])
    return out.reshape(planes.shape[:-2] + (K,))


def _parts(u, v, scale, fft2):
    N = u.shape[-1]
    U = scale[0] * fft2(np.asarray(u, dtype=np.float64)).astype(np.complex128)
    V = scale[1] * fft2(np.asarray(v, dtype=np.float64)).astype(np.complex128)
    f = np.fft.fftfreq(N) * N
    kx, ky = f[None, :], f[:, None]                       # kx along the LAST axis (W), ky along axis -2 (H)
    k2 = kx ** 2 + ky ** 2
    g = np.where(k2 == 0, 0.0, 1.0 / np.where(k2 == 0, 1.0, k2)) / (2.0 * N * N)
    return U, V, kx * V - ky * U, kx * U + ky * V, g


def helm_ref(x, scale=(1.0, 1.0), fft2=np.fft.fft2):
    """The definition, float64: x [T, 2, N, N] (u, v) -> [T, 3, N/2 + 1] (ke, rot, div).  Another fft2 (an fp32 one) shows what
    its precision alone costs on the same inputs."""
    N = x.shape[-1]
    U, V, R, D, g = _parts(x[:, 0], x[:, 1], scale, fft2)
    ke = (np.abs(U) ** 2 + np.abs(V) ** 2) / (2.0 * N * N)
    return np.stack([_ring_means(p, N) for p in (ke, np.abs(R) ** 2 * g, np.abs(D) ** 2 * g)], axis=-2)


def helm_cross_ref(a, b, scale=(1.0, 1.0), fft2=np.fft.fft2):
    """a, b [T, 2, N, N] -> [T, 8, N/2 + 1]: ke, rot, div of a, of b, co_rot, co_div."""
    N = a.shape[-1]
    _, _, Ra, Da, g = _parts(a[:, 0], a[:, 1], scale, fft2)
    _, _, Rb, Db, _ = _parts(b[:, 0], b[:, 1], scale, fft2)
    co = [_ring_means(np.real(x * np.conj(y)) * g, N) for x, y in ((Ra, Rb), (Da, Db))]
    return np.concatenate([helm_ref(a, scale, fft2), helm_ref(b, scale, fft2), np.stack(co, axis=-2)], axis=-2)


FFT32 = lambda x: torch.fft.fft2(torch.from_numpy(x).float()).numpy()


def potential_flows(rng, T, N, slope):
    """(rotational, divergent) flows [T, 2, N, N] whose ring-mean kinetic energy falls as k^-slope: psi, chi are power-law Gaussian
    fields with the Nyquist rows and columns zeroed in Fourier space (with them the Nyquist ring is not pure: 1.3e-3 at
    N = 16), differentiated spectrally: (u, v) = (-d psi / dH, d psi / dW) and (d chi / dW, d chi / dH)."""
    f = np.fft.fftfreq(N) * N
    kx, ky = f[None, :], f[:, None]
    r = np.sqrt(kx ** 2 + ky ** 2)
    r[0, 0] = 1.0
    flows = []
    for which in ("rot", "div"):
        P = np.fft.fft2(rng.standard_normal((T, N, N))) * r ** (-(slope + 2) / 2)
        P[:, N // 2, :] = 0.0
        P[:, :, N // 2] = 0.0
        if which == "rot":
            uh, vh = -1j * ky * P, 1j * kx * P
        else:
            uh, vh = 1j * kx * P, 1j * ky * P
        flows.append(np.stack([np.real(np.fft.ifft2(uh)), np.real(np.fft.ifft2(vh))], axis=1))
    return flows


def offset(x):
    """The constants 1/N and -2/N on u and v: ring 0 is well conditioned."""
    N = x.shape[-1]
    y = x.copy()
    y[:, 0] += 1.0 / N
    y[:, 1] -= 2.0 / N
    return y


def boundary_pairs(N, n):
    """n frequency pairs (a, b), 0 < a, b < N/2, with a^2 + b^2 = k^2 + k (the outer edge of ring k), largest k first."""
    out = []
    for k in range(N // 2, 0, -1):
        for a in range(1, N // 2):
            b2 = k * k + k - a * a
            if b2 <= 0:
                break
            b = int(round(np.sqrt(b2)))
            if b * b == b2 and 0 < b < N // 2:
                out.append((a, b, k))
                break
        if len(out) == n:
            return out
    return out


def check_planes(got, ref, what, tol=TOL):
    """|got - ref| <= tol * ke_ref per ring ([..., 3, K] or [..., 8, K]; the co-planes against sqrt(ke_a ke_b))."""
    if ref.shape[-2] == 3:
        den = np.broadcast_to(ref[..., 0:1, :], ref.shape)
    else:
        ka, kb = ref[..., 0:1, :], ref[..., 3:4, :]
        den = np.concatenate([np.broadcast_to(ka, ka.shape[:-2] + (3, ka.shape[-1])),
                              np.broadcast_to(kb, kb.shape[:-2] + (3, kb.shape[-1])),
                              np.broadcast_to(np.sqrt(ka * kb), ka.shape[:-2] + (2, ka.shape[-1]))], axis=-2)
    assert (den > 0).all(), what
    err = np.abs(got - ref) / den
    worst = [float(err[..., p, :].max()) for p in range(ref.shape[-2])]
    print(what, "max |got - ref| / ke per plane", ["%.2e" % w for w in worst])
    assert max(worst) <= tol, (what, worst)
    return max(worst)


# ----------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("N", [16, 32, 2048])
def test_known_answer_plane_waves(N):
    """(u, v) = (au, av) cos(2 pi (p col + q row) / N + 0.7): planes * 4 count[k0] / N^2 = (au^2 + av^2, (p av - q au)^2 / k2,
    (p au + q av)^2 / k2) on ring k0 = floor(|(p, q)| + 1/2) and nothing elsewhere; on the Nyquist lines (2, N/2) and (N/2, 3)
    the values follow the no-cross-term rule, ((p av)^2 + (q au)^2) / k2 and ((p au)^2 + (q av)^2) / k2.  N = 32: the radix-2
    last stage; N = 2048: one FFT per workgroup, five rings per thread, and one wave on the outer edge of a ring.
    Bound on ring k0: 1e-5 of the kinetic energy (an fp32 FFT of a single wave is good to about 1e-6; the rotational part of a
    divergent wave is a difference of two products of that accuracy, so it is bounded against ke, not against itself)."""
    pq = [(1, 0, None, False), (N // 4, N // 8 + 1, None, False), (N // 2 - 1, 1, None, False)]
    if N == 2048:
        edge = boundary_pairs(N, 1)
        assert len(edge) == 1
        pq = pq[2:] + [(edge[0][0], edge[0][1], edge[0][2], False)]
    pq += [(2, N // 2, None, True), (N // 2, 3, None, True)]
    if N == 16:
        pq.append((N // 2, 1, None, True))                    # (8, 3) lies in the dropped corner (ring 9): (8, 1) is in ring 8
    h = np.arange(N)
    cases = []
    for p, q, k_edge, nyq in pq:
        n = float(np.hypot(p, q))
        for au, av in ((p / n, q / n), (-q / n, p / n), (1.0, 1.0)):
            cases.append((p, q, k_edge, nyq, au, av))
    x = torch.empty(len(cases), 2, N, N)
    for i, (p, q, _, _, au, av) in enumerate(cases):
        c = torch.from_numpy(np.cos(2 * np.pi * ((p * h[None, :] + q * h[:, None]) % N) / N + 0.7))
        x[i, 0] = au * c
        x[i, 1] = av * c
    got = spectra.helmholtz_rapsd(x.to(DEV), per_field=True).cpu().numpy()
    assert got.shape == (len(cases), 3, N // 2 + 1)
    counts = spectra.ring_counts(N)
    for i, (p, q, k_edge, nyq, au, av) in enumerate(cases):
        k0 = int(np.floor(np.sqrt(p * p + q * q) + 0.5))
        assert k_edge is None or k0 == k_edge
        k2 = p * p + q * q
        if k0 > N // 2:                                       # a wave in the dropped corner leaves every ring empty
            assert (N, p, q) == (16, 8, 3)
            assert np.abs(got[i]).max() <= 1e-7 * N * N * (au * au + av * av), (p, q, au, av)
            continue
        if nyq:
            want = (au * au + av * av, ((p * av) ** 2 + (q * au) ** 2) / k2, ((p * au) ** 2 + (q * av) ** 2) / k2)
        else:
            want = (au * au + av * av, (p * av - q * au) ** 2 / k2, (p * au + q * av) ** 2 / k2)
        norm = got[i, :, k0] * 4.0 * counts[k0] / (N * N)
        rest = np.abs(np.delete(got[i], k0, axis=1)).max()
        print(N, (p, q), (round(au, 3), round(av, 3)), norm, want, rest / (N * N))
        assert np.abs(norm - want).max() <= 1e-5 * want[0], (p, q, au, av, norm, want)
        assert rest <= 1e-7 * N * N * want[0], (p, q, au, av, rest)
    # (1, 1) on (2, N/2): rot = div = ke / 2 -- doubling one member of the conjugate pair would give 0.75 / 1.25 at N = 32
    i = cases.index((2, N // 2, None, True, 1.0, 1.0))
    k0 = int(np.floor(np.hypot(2, N // 2) + 0.5))
    np.testing.assert_allclose(got[i, 1:, k0] / got[i, 0, k0], [0.5, 0.5], atol=1e-5)


# --------------------------------------------------------------------------------------------- flows through the layouts
def _sides(x64, C=2):
    """name -> (device tensor, nhwc, the float64 values the kernel sees [T, C, N, N]) of one side."""
    x32 = torch.from_numpy(x64.astype(np.float32))
    T, _, N, _ = x32.shape
    pad = torch.zeros(T, N, N, 16, dtype=torch.bfloat16)
    pad[..., :C] = x32.permute(0, 2, 3, 1).to(torch.bfloat16)
    pad[..., C:] = 7.0                                        # padding channels hold garbage that must not be read
    return {"nchw_f32": (x32.to(DEV), False, x32.double().numpy()),
            "nhwc_f32": (x32.permute(0, 2, 3, 1).contiguous().to(DEV), True, x32.double().numpy()),
            "nhwc_bf16_padded": (pad.to(DEV), True, pad[..., :C].permute(0, 3, 1, 2).double().numpy())}


LAYOUT_PAIRS = [("nchw_f32", "nchw_f32"), ("nhwc_f32", "nhwc_bf16_padded"), ("nhwc_bf16_padded", "nchw_f32")]
FLOW_PAIRS = [("rot", "div"), ("div", "mix"), ("mix", "rot")]     # (side a, side b) of the three layout pairs


@functools.lru_cache(maxsize=2)
def _flow_case(N, slope, T=2):
    rng = np.random.default_rng(1000 * N + slope)
    rot, div = potential_flows(rng, T, N, slope)
    for flow, foreign in ((rot, 2), (div, 1)):                # the flows are what they claim, in float64
        s = helm_ref(flow)
        assert (s[:, foreign] <= 1e-12 * s[:, 0]).all(), (N, slope, foreign)
    flows = {"rot": offset(rot), "div": offset(div), "mix": offset(rot + 0.3 * div)}
    return {name: _sides(x) for name, x in flows.items()}


def _one(side, **kw):
    return spectra.helmholtz_rapsd(side[0], channels=2, nhwc=side[1], **kw)


def _two(sa, sb, **kw):
    return spectra.helmholtz_cross(sa[0], sb[0], nhwc=sa[1], nhwc_b=sb[1], channels=2, **kw)


@pytest.mark.parametrize("N", [16, 128, 1024])
@pytest.mark.parametrize("slope", [0, 2, 3])
def test_pure_and_mixed_flows_match_float64(N, slope):
    """Every plane against float64 on the values the kernel sees.  A pure flow additionally has no foreign part beyond 1e-4 ke
    per ring, checked on the fp32 sides: rounding a flow to bf16 adds white noise of 1e-6 of its variance, which is neither
    rotational nor divergent and exceeds 1e-4 of the ring's energy where a steep spectrum has fallen below it."""
    F = _flow_case(N, slope)
    for (la, lb), (fa, fb) in zip(LAYOUT_PAIRS, FLOW_PAIRS):
        a, b = F[fa][la], F[fb][lb]
        ref = helm_cross_ref(a[2], b[2])
        got = _two(a, b, per_field=True).cpu().numpy()
        assert got.shape == ref.shape == (2, 8, N // 2 + 1)
        check_planes(got, ref, (N, slope, fa, la, fb, lb))
        check_planes(_two(a, b).cpu().numpy(), ref.mean(0), (N, slope, fa, la, fb, lb, "mean"))
        check_planes(_one(a, per_field=True).cpu().numpy(), ref[:, 0:3], (N, slope, fa, la, "one-sided"))
        for flow, layout, p0 in ((fa, la, 0), (fb, lb, 3)):
            foreign = {"rot": 2, "div": 1}.get(flow)
            if foreign is not None and layout != "nhwc_bf16_padded":
                worst = (got[:, p0 + foreign] / ref[:, p0]).max()
                print((N, slope, flow, layout), "foreign part / ke", worst)
                assert worst <= TOL, (N, slope, flow, layout, worst)
    s = helm_ref(F["mix"]["nchw_f32"][2])
    ratio = s[:, 2, 1:N // 2].sum(-1) / s[:, 1, 1:N // 2].sum(-1)
    assert (0.02 < ratio).all() and (ratio < 0.4).all(), ratio              # the mix is 1 : 0.3 in amplitude, about 0.09 in energy


@pytest.mark.parametrize("N", [16, 128, 1024])
def test_identities(N):
    F = _flow_case(N, 2)
    mix = F["mix"]
    x, _, seen = mix["nchw_f32"]
    one = _one(mix["nchw_f32"], per_field=True)
    s = one.cpu().numpy()
    ke = s[:, 0]
    # rot + div = ke on every ring k >= 1, and the mean has neither part
    assert (np.abs(s[:, 1, 1:] + s[:, 2, 1:] - ke[:, 1:]) <= 1e-6 * ke[:, 1:]).all(), \
        (np.abs(s[:, 1, 1:] + s[:, 2, 1:] - ke[:, 1:]) / ke[:, 1:]).max()
    assert (s[:, 1:, 0] == 0).all() and (ke[:, 0] > 0).all()
    # exchanging the pair is the call on swapped channels
    swapped = x[:, [1, 0]].contiguous()
    assert torch.equal(spectra.helmholtz_rapsd(x, pair=(1, 0), per_field=True), spectra.helmholtz_rapsd(swapped, per_field=True))
    # rows that run the other way: the call on the row-flipped fields
    flipped = torch.flip(x, dims=(2,)).contiguous()
    down = spectra.helmholtz_rapsd(x, rows_up=False, per_field=True).cpu().numpy()
    check_planes(down, spectra.helmholtz_rapsd(flipped, per_field=True).cpu().numpy(), (N, "rows_up=False"))
    check_planes(down, helm_ref(seen, (1.0, -1.0)), (N, "rows_up=False against float64"))
    assert np.abs(down - s)[:, 1:].max() > 10 * TOL * ke.min()             # and the direction matters for a mixed flow
    # scale: the call on pre-scaled inputs
    pre = torch.stack([2.0 * x[:, 0], -3.0 * x[:, 1]], dim=1).contiguous()
    scaled = spectra.helmholtz_rapsd(x, scale=(2.0, -3.0), per_field=True).cpu().numpy()
    check_planes(scaled, spectra.helmholtz_rapsd(pre, per_field=True).cpu().numpy(), (N, "scale"))
    check_planes(scaled, helm_ref(seen, (2.0, -3.0)), (N, "scale against float64"))
    for (la, lb), (fa, fb) in zip(LAYOUT_PAIRS, FLOW_PAIRS):
        a, b = F[fa][la], F[fb][lb]
        ab = _two(a, b, per_field=True)
        # planes 0-5 are the one-sided calls, bit for bit
        assert torch.equal(ab[:, 0:3], _one(a, per_field=True)), (la, lb)
        assert torch.equal(ab[:, 3:6], _one(b, per_field=True)), (la, lb)
        # the co-planes are symmetric in (a, b), and those of (a, a) are a's own
        ba = _two(b, a, per_field=True)
        assert torch.equal(ba[:, 0:3], ab[:, 3:6]) and torch.equal(ba[:, 3:6], ab[:, 0:3]), (la, lb)
        assert torch.equal(ba[:, 6:8], ab[:, 6:8]), (la, lb)
        aa = _two(a, a, per_field=True)
        assert torch.equal(aa[:, 6], aa[:, 1]) and torch.equal(aa[:, 7], aa[:, 2]), (la, lb)
        assert torch.equal(aa[:, 3:6], aa[:, 0:3]), (la, lb)
        # two calls are bit-identical
        assert torch.equal(_two(a, b, per_field=True), ab), (la, lb)
        assert torch.equal(_two(a, b), _two(a, b)), (la, lb)
        # co_rot + co_div = (co_u + co_v) / 2 of cross_rapsd, and Cauchy-Schwarz per part
        g = ab.cpu().numpy()
        cross = spectra.cross_rapsd(a[0], b[0], channels=2, nhwc=a[1], nhwc_b=b[1], per_field=True).cpu().numpy()
        bound = np.sqrt(g[:, 0] * g[:, 3])
        gap = np.abs(g[:, 6] + g[:, 7] - 0.5 * cross[:, :, 2].sum(1))[:, 1:] / bound[:, 1:]
        print((N, la, lb), "co_rot + co_div against cross_rapsd / sqrt(ke_a ke_b)", gap.max())
        assert gap.max() <= TOL, (la, lb, gap.max())
        for pa, pb, pc in ((1, 4, 6), (2, 5, 7)):
            assert (np.abs(g[:, pc]) <= np.sqrt(g[:, pa] * g[:, pb]) * (1 + 1e-6) + 1e-7 * bound).all(), (la, lb, pc)


def test_multi_batch_loop_in_one_workgroup():
    """T = 2048 pairs at N = 64: every pair is ONE slice (S = 1) and one workgroup walks the two line batches (32 + 1 lines)
    through the same LDS buffers, with side a's U, V in registers across side b's transforms.  With T = 3 each batch has a
    workgroup of its own (S = 2).  torch's fp32 FFT on the CPU stays within 1e-5 (measured 5e-7) of float64 on these inputs in
    the measure of the bound, so a failure cannot be blamed on them."""
    N, T = 64, 2048
    rng = np.random.default_rng(64)
    rot, div = potential_flows(rng, T, N, 2)
    rot2, div2 = potential_flows(rng, T, N, 2)
    a64 = offset(rot + 0.3 * div)
    b64 = offset(0.7 * rot + 0.5 * rot2 + 0.3 * div2)
    a, b = torch.from_numpy(a64.astype(np.float32)), torch.from_numpy(b64.astype(np.float32))
    ref = helm_cross_ref(a.double().numpy(), b.double().numpy())
    cpu32 = helm_cross_ref(a.numpy(), b.numpy(), fft2=FFT32)
    margin = check_planes(cpu32, ref, "fp32 FFT on the CPU", tol=1e-5)
    ad, bd = a.to(DEV), b.to(DEV)
    got = spectra.helmholtz_cross(ad, bd, per_field=True)
    assert got.shape == (T, 8, N // 2 + 1)
    check_planes(got.cpu().numpy(), ref, "T = 2048")
    assert torch.equal(got[:, 0:3], spectra.helmholtz_rapsd(ad, per_field=True))
    assert torch.equal(got[:, 3:6], spectra.helmholtz_rapsd(bd, per_field=True))
    assert torch.equal(spectra.helmholtz_cross(ad[:3], bd[:3], per_field=True), got[:3])
    assert torch.equal(spectra.helmholtz_rapsd(ad[:3], per_field=True), got[:3, 0:3])


def test_chunked_and_accumulated(monkeypatch):
    """Differently ordered fp64 sums of at most 24 terms agree to rtol 1e-12 on the six one-sided planes (sums of non-negative
    terms) and on the co-planes as long as no ring mean of them, which may change sign from pair to pair, cancels below 1e-3 of
    the sum of its terms' magnitudes; asserted.  Ring 0 of rot, div and the co-planes is exactly zero in every call."""
    N, T = 256, 24
    rng = np.random.default_rng(5)
    rot, div = potential_flows(rng, T, N, 3)
    rot2, div2 = potential_flows(rng, T, N, 3)
    a64 = offset(rot + 0.3 * div)
    b64 = offset(0.7 * rot + 0.5 * rot2 + 0.2 * div + 0.2 * div2)
    a, b = (torch.from_numpy(v.astype(np.float32)).to(DEV) for v in (a64, b64))
    pf = spectra.helmholtz_cross(a, b, per_field=True)
    m1 = spectra.helmholtz_cross(a, b)
    assert (pf[:, [1, 2, 4, 5, 6, 7], 0] == 0).all()

    def close(x, want):
        np.testing.assert_allclose(x.cpu().numpy(), want.cpu().numpy(), rtol=1e-12, atol=0)

    for n in (24, 17):
        co = pf[:n, 6:8, 1:]
        cancel = (co.sum(0).abs() / co.abs().sum(0)).min().item()
        print("co-planes of", n, "pairs: smallest |sum| / sum of |terms|", cancel)
        assert cancel >= 1e-3, (n, cancel)
    close(m1, pf.mean(0))
    monkeypatch.setattr(spectra, "WS_CAP", 3 << 20)          # 1.06 MB of half spectra per pair: 2 pairs a call
    ops = spectra._default_ops(torch.device(DEV))
    assert spectra._helm_chunk(ops, T, N, True) <= 3 and spectra._helm_chunk(ops, T, N, False) <= 6
    assert torch.equal(spectra.helmholtz_cross(a, b, per_field=True), pf)
    assert torch.equal(spectra.helmholtz_rapsd(a, per_field=True), pf[:, 0:3])
    close(spectra.helmholtz_cross(a, b), m1)
    close(spectra.helmholtz_rapsd(b), m1[3:6])
    acc = spectra.HelmholtzSpectrum(N, device=DEV)
    acc.add(a[:10], b[:10]).add(a[10:], b[10:], n_valid=7)
    assert acc.count == 17
    close(acc.mean(), pf[:17].mean(0))


def test_effective_resolution_per_part_end_to_end():
    """b takes a's rotational Fourier part unchanged and its divergent part negated above ring kc: the generator has the real
    field's vortical flow at every scale and only invents its divergent flow below N / kc grid points.  A single-channel
    coherence cannot show that; here coh_rot = +1 everywhere, coh_div = +1 up to kc and -1 beyond."""
    N, kc = 128, 12
    rng = np.random.default_rng(12)
    rot, div = potential_flows(rng, 2, N, 2)
    sign = np.where(ring_index(N) <= kc, 1.0, -1.0)
    div_b = np.real(np.fft.ifft2(np.fft.fft2(div) * sign))
    a64, b64 = offset(rot + div), offset(rot + div_b)
    a, b = torch.from_numpy(a64.astype(np.float32)), torch.from_numpy(b64.astype(np.float32))
    s = spectra.helmholtz_cross(a.to(DEV), b.to(DEV))
    coh = spectra.helmholtz_coherence(s)
    print("coh_rot", coh[0, kc - 2:kc + 3], "coh_div", coh[1, kc - 2:kc + 3])
    assert np.isnan(coh[:, 0]).all()
    np.testing.assert_allclose(coh[0, 1:], 1.0, atol=1e-4)
    np.testing.assert_allclose(coh[1, 1:kc + 1], 1.0, atol=1e-4)
    np.testing.assert_allclose(coh[1, kc + 1:], -1.0, atol=1e-4)
    k_eff = spectra.effective_resolution(coh)
    assert k_eff.tolist() == [N // 2, kc]
    assert spectra.wavelength_px(k_eff, N).tolist() == [2.0, N / kc]
    # what the scalar diagnostics see: u's coherence is a blend of the two parts and crosses no threshold at kc
    frac = spectra.divergent_fraction(s)
    np.testing.assert_allclose(frac[0, 1:], frac[1, 1:], atol=1e-4)        # the two sides have the same split at every scale
    slope = spectra.spectral_slope(s.cpu().numpy()[[1, 2, 4, 5]], 4, N // 4)
    assert np.abs(slope - (-2.0)).max() < 0.4, slope                       # the potentials were drawn for ring means ~ k^-2


# ------------------------------------------------------------------------------------------------------------- trainer
KEYS = set(spectra.HELM_CROSS_PLANES) | {"div_frac_real", "div_frac_fake", "coh_rot", "coh_div", "k_eff_rot", "k_eff_div",
                                         "wavelength_px_rot", "wavelength_px_div", "fields"}


def _trainer_epoch(monkeypatch, log_helmholtz):
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
    tr.log_spectra = True                                     # rapsd of the same fields, through the sibling hook
    tr.log_helmholtz = log_helmholtz
    ds = lambda a, b: NetCDFSR(torch.from_numpy(coarse[a:b]), torch.from_numpy(fine[a:b]))
    train = torch.utils.data.DataLoader(ds(0, 2), batch_size=2)           # one batch
    test = torch.utils.data.DataLoader(ds(2, 8), batch_size=2)            # three batches
    tr.train(train, test, epochs=1)
    return tr, coarse, fine


def test_trainer_hook(monkeypatch):
    tr, coarse, fine = _trainer_epoch(monkeypatch, True)
    summary = tr.metrics_log[0]
    hz = summary.pop("helmholtz")
    assert set(hz) == {"train", "test"}
    assert hz["train"]["fields"] == 2 and hz["test"]["fields"] == 6
    for part in ("train", "test"):
        d = hz[part]
        assert set(d) == KEYS
        for key in KEYS - {"k_eff_rot", "k_eff_div", "wavelength_px_rot", "wavelength_px_div", "fields"}:
            assert np.array(d[key]).shape == (65,), key
        s = np.stack([d[name] for name in spectra.HELM_CROSS_PLANES])
        frac, coh = spectra.divergent_fraction(s), spectra.helmholtz_coherence(s)
        np.testing.assert_array_equal(d["div_frac_real"], frac[0])
        np.testing.assert_array_equal(d["div_frac_fake"], frac[1])
        np.testing.assert_array_equal(d["coh_rot"], coh[0])
        np.testing.assert_array_equal(d["coh_div"], coh[1])
        assert np.nanmax(np.abs(coh)) <= 1 + 1e-6
        for i, what in enumerate(("rot", "div")):
            k, w = d["k_eff_" + what], d["wavelength_px_" + what]
            assert isinstance(k, int) and k == spectra.effective_resolution(coh[i], tr.helmholtz_threshold)
            assert 0 <= k <= 64 and w == (128 / k if k else np.inf)
        # the kinetic energy is half the sum of the two channels' power spectra, which the sibling hook reports
        for side in ("real", "fake"):
            p = np.array(summary["spectra"][part][side])
            np.testing.assert_allclose(d["ke_" + side], 0.5 * (p[0] + p[1]), rtol=1e-5)
        assert (np.abs(s[1, 1:] + s[2, 1:] - s[0, 1:]) <= 1e-6 * s[0, 1:]).all()
        assert (np.abs(s[4, 1:] + s[5, 1:] - s[3, 1:]) <= 1e-6 * s[3, 1:]).all()
    tr_off, _, _ = _trainer_epoch(monkeypatch, False)
    off = tr_off.metrics_log[0]
    assert "helmholtz" not in off
    assert off.keys() == summary.keys()
    for part in ("train", "test"):
        for k, v in off[part].items():
            assert v == pytest.approx(summary[part][k], rel=1e-6, abs=1e-7), (part, k)
        for k in ("real", "fake", "lsd"):
            np.testing.assert_allclose(off["spectra"][part][k], summary["spectra"][part][k], rtol=1e-6, err_msg=f"{part} {k}")
        assert off["spectra"][part]["fields"] == summary["spectra"][part]["fields"]
