"""dg_cross_rapsd, dg_helmholtz and dg_helmholtz_cross on the MI355X (csrc/spectra.hip), frequency by frequency
(tests/spectra_rings_ref.py): every frequency of a 16 x 16, 32 x 32 and 64 x 64 grid as a pair of vector fields of its own, all
pairs of an N in one call, against the analytic answer; the bit identities and the call variants (scale, rows_up, pair) on the
same tensors; and one frequency on every ring at N = 128, 512 and 2048 against the float64 full-spectrum definition.

The bounds are the project's own (tests/test_helmholtz_gpu.py, tests/test_coherence_gpu.py, tests/test_spectra_rings_gpu.py):
single waves to 1e-5 of the plane's phase-independent envelope on the ring that holds the wave and to 1e-7 N^2 times the
amplitude factor on every other ring (the float64 definition on the same fp32 samples sits at 1e-7 and 1e-16 there:
tests/test_spectra_rings_cpu.py), multi-frequency fields to 1e-4 of the ring's kinetic energy."""
import functools

import numpy as np
import pytest
import torch

from downgan_amd import spectra
from tests import spectra_rings_ref as S
from tests.test_spectra_rings_gpu import RAPSD_PTS, _column_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4                # multi-frequency fields, per ring, against float64 (the CPU file's PAIR_TOL)


def _flat(cross):
    """[F, 2, 3, K] -> [F, 6, K]: the comparator takes one plane axis."""
    return cross.reshape(cross.shape[0], 6, cross.shape[-1])


@functools.lru_cache(maxsize=1)
def _exhaustive_calls(N):
    """The four entry points on all N (N/2 + 1) pairs of an N, each ONE library call: device tensors."""
    A, B = (torch.from_numpy(x).to(DEV) for x in S.exhaustive_pair(N))
    F = A.shape[0]
    assert F == N * (N // 2 + 1)
    ops = spectra._default_ops(torch.device(DEV))
    assert spectra._helm_chunk(ops, F, N, True) == F and spectra._helm_chunk(ops, F, N, False) == F
    assert spectra._cross_chunk(ops, F, 2, N) == F
    # one column workgroup per pair (per field); at N = 64 it walks two line batches, side a's U, V in registers meanwhile
    plan = (1, 2) if N == 64 else (1, 1)
    assert _column_plan(F, N) == plan and _column_plan(2 * F, N) == plan
    return {"A": A, "B": B,
            "pair": spectra.helmholtz_cross(A, B, per_field=True),
            "one_a": spectra.helmholtz_rapsd(A, per_field=True),
            "one_b": spectra.helmholtz_rapsd(B, per_field=True),
            "cross": spectra.cross_rapsd(A, B, per_field=True)}


def _check_all(N, got, scale=(1.0, 1.0), pair=(0, 1), tag=""):
    """pair [F, 8, K], one_a, one_b [F, 3, K] (and cross [F, 2, 3, K]) against the analytic answer, every frequency."""
    counts = spectra.ring_counts(N)
    want_h, want_c, k0 = S.exhaustive_pair_expected(N, counts, scale, pair)
    e_h, amp_h, e_c, amp_c = S.exhaustive_pair_envelopes(N, counts, scale, pair)
    F, K = want_h.shape[0], N // 2 + 1
    assert got["pair"].shape == (F, 8, K) and got["one_a"].shape == got["one_b"].shape == (F, 3, K)
    S.check_exhaustive(tag + "helmholtz_cross", got["pair"].cpu().numpy(), want_h, k0, e_h, amp_h, N)
    S.check_exhaustive(tag + "helmholtz_rapsd(a)", got["one_a"].cpu().numpy(), want_h[:, 0:3], k0, e_h[:, 0:3], amp_h[:, 0:3], N)
    S.check_exhaustive(tag + "helmholtz_rapsd(b)", got["one_b"].cpu().numpy(), want_h[:, 3:6], k0, e_h[:, 3:6], amp_h[:, 3:6], N)
    if "cross" in got:
        assert got["cross"].shape == (F, 2, 3, K)
        S.check_exhaustive(tag + "cross_rapsd", _flat(got["cross"].cpu().numpy()), _flat(want_c), k0, e_c.reshape(F, 6),
                           amp_c.reshape(F, 6), N)
    corner = k0 > N // 2                                            # asserted above within bounds; they are in the set
    assert corner.any() and not want_h[corner].any()


@pytest.mark.parametrize("N", [16, 32, 64])
def test_every_frequency_of_the_pair_spectra(N):
    _check_all(N, _exhaustive_calls(N))


@pytest.mark.parametrize("N", [16, 32, 64])
def test_identities_at_every_frequency(N):
    c = _exhaustive_calls(N)
    A, B, pair, cross = c["A"], c["B"], c["pair"], c["cross"]
    assert torch.equal(pair[:, 0:3], c["one_a"]) and torch.equal(pair[:, 3:6], c["one_b"])
    aa = spectra.helmholtz_cross(A, A, per_field=True)
    assert torch.equal(aa[:, 6], aa[:, 1]) and torch.equal(aa[:, 7], aa[:, 2]) and torch.equal(aa[:, 3:6], aa[:, 0:3])
    assert torch.equal(aa[:, 0:3], c["one_a"])
    bb = spectra.helmholtz_cross(B, B, per_field=True)
    assert torch.equal(bb[:, 6], bb[:, 1]) and torch.equal(bb[:, 7], bb[:, 2]) and torch.equal(bb[:, 0:3], c["one_b"])
    assert torch.equal(spectra.helmholtz_cross(A, B, per_field=True), pair)
    assert torch.equal(cross[:, :, 0], spectra.rapsd(A, per_field=True))
    assert torch.equal(cross[:, :, 1], spectra.rapsd(B, per_field=True))
    # co_rot + co_div = (co_u + co_v) / 2 on the rings k >= 1 (the mean has neither part): the Helmholtz kernels against the
    # cross kernel, per frequency
    counts = spectra.ring_counts(N)
    _, _, k0 = S.exhaustive_pair_expected(N, counts)
    e_h, amp_h, _, _ = S.exhaustive_pair_envelopes(N, counts)
    g, x = pair.cpu().numpy(), cross.cpu().numpy()
    assert (g[:, [1, 2, 4, 5, 6, 7], 0] == 0).all()
    gap = np.abs(g[:, 6] + g[:, 7] - 0.5 * x[:, :, 2].sum(1))[:, 1:]                # [F, K - 1]
    k0 = k0 - 1
    inside = (k0 >= 0) & (k0 < N // 2)
    f = np.nonzero(inside)[0]
    on = gap[f, k0[f]] / e_h[f, 6]
    rest = gap.copy()
    rest[f, k0[f]] = 0.0
    off = rest.max(1) / (N * N * amp_h[:, 6])
    print(f"[rings-pair] N={N} co_rot + co_div against cross_rapsd: on the ring {on.max():.3e} of E, elsewhere {off.max():.3e} N^2 amp")
    a, b = S.exhaustive_freqs(N)
    i = f[int(np.argmax(on))]
    assert on.max() <= S.ON_TOL, (int(a[i]), int(b[i]), int(k0[i]) + 1, on.max())
    i = int(np.argmax(off))
    assert off.max() <= 2 * S.OFF_TOL, (int(a[i]), int(b[i]), int(k0[i]) + 1, off.max())  # a sum of two bounded terms


VARIANTS = {"scale": ({"scale": (2.0, -3.0)}, (2.0, -3.0), (0, 1)),
            "rows_down": ({"rows_up": False}, (1.0, -1.0), (0, 1)),
            "pair_exchanged": ({"pair": (1, 0)}, (1.0, 1.0), (1, 0))}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_call_variants_at_every_frequency(variant):
    """scale = (2, -3): the known answer with (xu, xv) -> (2 xu, -3 xv); rows_up = False: xv -> -xv; pair = (1, 0): u and v
    exchanged.  The same bounds."""
    N = 16
    kw, scale, pair = VARIANTS[variant]
    c = _exhaustive_calls(N)
    got = {"pair": spectra.helmholtz_cross(c["A"], c["B"], per_field=True, **kw),
           "one_a": spectra.helmholtz_rapsd(c["A"], per_field=True, **kw),
           "one_b": spectra.helmholtz_rapsd(c["B"], per_field=True, **kw)}
    _check_all(N, got, scale, pair, tag=variant + " ")
    assert torch.equal(got["pair"][:, 0:3], got["one_a"]) and torch.equal(got["pair"][:, 3:6], got["one_b"])
    base = c["pair"].cpu().numpy()
    assert np.abs(got["pair"].cpu().numpy() - base)[:, [1, 2, 6, 7]].max() > 1e-3 * np.abs(base).max()   # the variant matters


@functools.lru_cache(maxsize=1)
def _one_per_ring_case(N):
    """fp32 (A, B) [n, 2, N, N] and the float64 references on those values; N = 2048: the outer-edge and the mirrored field."""
    fields = (1, 3) if N == 2048 else (0, 1, 2, 3)
    A, B = (torch.from_numpy(x.astype(np.float32)) for x in S.one_per_ring_pair(N, fields))
    counts = spectra.ring_counts(N)
    seen = A.double().numpy(), B.double().numpy()
    return A, B, S.helm_cross_ref(*seen, counts), S.cross_ref(*seen, counts)


@pytest.mark.parametrize("N", [128, 512, 2048])
def test_one_frequency_on_every_ring_pair(N):
    """N = 128: S = 5 slices of lines per field; N = 2048: one line per batch and five rings per thread."""
    A, B, ref_h, ref_c = _one_per_ring_case(N)
    T = A.shape[0]
    s, _ = _column_plan(T, N)
    assert (N, s) in ((128, 5), (512, 65), (2048, 1024)) and (N < 2048 or RAPSD_PTS // N == 1)
    ad, bd = A.to(DEV), B.to(DEV)
    pair = spectra.helmholtz_cross(ad, bd, per_field=True)
    one_a, one_b = spectra.helmholtz_rapsd(ad, per_field=True), spectra.helmholtz_rapsd(bd, per_field=True)
    cross = spectra.cross_rapsd(ad, bd, per_field=True)
    assert pair.shape == ref_h.shape and cross.shape == ref_c.shape
    worst = {"helmholtz_cross": S.helm_measure(pair.cpu().numpy(), ref_h),
             "helmholtz_rapsd(a)": S.helm_measure(one_a.cpu().numpy(), ref_h[:, 0:3]),
             "helmholtz_rapsd(b)": S.helm_measure(one_b.cpu().numpy(), ref_h[:, 3:6]),
             "cross_rapsd": list(S.cross_measure(cross.cpu().numpy(), ref_c))}
    for name, w in worst.items():
        print(f"[rings-pair] N={N} one per ring, {name}: worst error per plane against float64 {['%.2e' % v for v in w]} (bound {TOL:.0e})")
    for name, w in worst.items():
        assert np.isfinite(w).all() and max(w) <= TOL, (N, name, w)
    assert torch.equal(pair[:, 0:3], one_a) and torch.equal(pair[:, 3:6], one_b)
