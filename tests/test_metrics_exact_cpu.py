"""The references, comparators and size guards of tests/metrics_ref.py on the host: ``EmuOps`` passes every small and view case of
the table through the same comparators the GPU file uses (integer cases in bits, random cases under the same bounds), each located
mutation of the emulation is rejected by the case meant for it, and ``GAN/losses.py``'s divergence / vorticity path runs on the
emulation against the reference's known answers."""
import numpy as np
import pytest
import torch

from oracle.emu_ops import EmuOps
from tests import metrics_ref as M

HOST_CASES = [c for c in M.CASES if c[3] in ("small", "view")]
BITS, SUMS = "differ in bits", "sums differ"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_emu_ops_pass_every_small_and_view_case(case, dtype):
    _, fn, kw, _ = case
    fn(EmuOps(dtype), dtype, **kw)


def test_case_table_has_the_three_sizes_and_unique_ids():
    ids = [c[0] for c in M.CASES]
    assert len(set(ids)) == len(ids)
    assert {c[3] for c in M.CASES} == {"small", "view", "large"}
    for cid, _, kw, size in M.CASES:
        assert (size == "large") == ("expect" in kw), cid


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_size_guards_follow_the_shape_a_case_runs(dtype):
    """Each case, asked for its size property at a shape one step too small for it, refuses before it launches anything."""
    ops = EmuOps(dtype)
    shrunk = [(M.case_avgpool, dict(shapes=[(1672, 1672)], planes=(3,))),                 # 3 * 836 * 836 = 2,096,688 <= 8192 * 256
              (M.case_minmax_located, dict(pixels=65536, C=2)),
              (M.case_normalise, dict(shape=(1, 1448, 1448), C=2, layout="dense")),         # 2,096,704
              (M.case_div_vort, dict(shape=(1, 513, 513))),                               # 512 * 512 = 1024 * 256
              (M.case_stage, dict(npix=4096 * 256, c=1))]
    for fn, kw in shrunk:
        with pytest.raises(AssertionError, match="size guard: .* one grid-stride trip"):
            fn(ops, dtype, expect="second_trip", **kw)
    with pytest.raises(AssertionError, match="size guard: .* cap of .* is not reached"):       # exactly 2048 workgroups: the cap is met, not passed
        M.case_moments(ops, dtype, sizes=(4 * 256 * 2048 + 3,), expect="cap")
    with pytest.raises(AssertionError, match="size guard: .* cap of .* is not reached"):       # 2048 * 2047 * 4 chunks want 65504 workgroups
        M.case_lowpass_large(ops, dtype, shape=(1, 2048, 2047), C=4 * M.epc(dtype), expect="cap")
    for dt in ("f32", "bf16"):
        N, H, W = M.lowpass_large_shape(dt)
        assert M._cdiv(N * H * W * (16 // M.epc(dt)), 256) > M.FS_BLOCKS


# ------------------------------------------------------------------------------------------------------------------ located mutations
def _rejects(fn, why):
    """The comparator must refuse the mutant for the intended reason, not through a shape or dtype assert."""
    with pytest.raises(AssertionError, match=why):
        fn()


def _maps(X, Y, params):
    """The emulation's SSIM / CS maps (EmuOps.ssim_level up to its plane sums)."""
    win = torch.tensor([params.g[i] for i in range(params.win)], dtype=torch.float32)

    def gf(t):
        Cn = t.shape[1]
        w = win.view(1, 1, -1, 1).repeat(Cn, 1, 1, 1)
        return torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, w, groups=Cn), w.transpose(2, 3), groups=Cn)
    mu1, mu2 = gf(X), gf(Y)
    s1, s2, s12 = gf(X * X) - mu1 * mu1, gf(Y * Y) - mu2 * mu2, gf(X * Y) - mu1 * mu2
    cs = (2 * s12 + params.C2) / (s1 + s2 + params.C2)
    return ((2 * mu1 * mu2 + params.C1) / (mu1 * mu1 + mu2 * mu2 + params.C1)) * cs, cs


class ColumnShort(EmuOps):
    def ssim_level(self, X, Y, params, sums):                     # 1. the valid map one column short
        ss, cs = _maps(X, Y, params)
        sm = sums.view(-1, 2)
        sm[:, 0] += ss[..., :-1].flatten(2).sum(-1).flatten()
        sm[:, 1] += cs[..., :-1].flatten(2).sum(-1).flatten()


class WindowFlipped(EmuOps):
    def ssim_level(self, X, Y, params, sums):                     # 2. g[win - 1 - k] for g[k]
        flipped = M.ssim_params([params.g[params.win - 1 - i] for i in range(params.win)], params.C1, params.C2)
        super().ssim_level(X, Y, flipped, sums)


class PoolPadsHigh(EmuOps):
    def avgpool2(self, inp, out):                                 # 3. padding on the bottom / right
        out.copy_(torch.nn.functional.avg_pool2d(torch.nn.functional.pad(inp, (0, inp.shape[3] % 2, 0, inp.shape[2] % 2)), 2))


class ClampShort(EmuOps):
    @staticmethod
    def _clamped(L, d):                                           # 4. the far border clamps one short
        return (torch.arange(L) + d).clamp(0, max(L - 2, 0))


class FoldL1(EmuOps):
    @classmethod
    def _fold_matrix(cls, L):                                     # 5. the fold weight of a one-pixel axis is 5, not 1
        return torch.ones(1, 1) if L == 1 else super()._fold_matrix(L)


class MinmaxSkipsLast(EmuOps):
    def minmax(self, x, c_real, partial, minmax):                 # 6. the last pixel is never looked at
        super().minmax(x.reshape(1, 1, -1, x.shape[-1])[:, :, :-1], c_real, partial, minmax)


class WindowFirst(EmuOps):
    def div_vort_sums(self, hr, fake, sums):                      # 7. the [:-1, :-1] window
        def dv(t):
            t = torch.nan_to_num(t.double())
            dudy, dvdx = t[:, 1:, :-1, 0] - t[:, :-1, :-1, 0], t[:, :-1, 1:, 1] - t[:, :-1, :-1, 1]
            return dudy + dvdx, dvdx - dudy
        (dr, vr), (df, vf) = dv(hr), dv(fake)
        five = lambda r, f: [r.sum(), (r * r).sum(), f.sum(), (f * f).sum(), (r * f).sum()]
        sums += torch.stack(five(dr, df) + five(vr, vf))


class TailDropped(EmuOps):
    def moments(self, x, acc):                                    # 8. the n % 4 tail is dropped
        super().moments(x.flatten()[:x.numel() & ~3], acc) if x.numel() >= 4 else None


MUTANTS = [
    ("valid-map-one-column-short", ColumnShort, M.case_ssim_count, dict(win=7, rot=2), SUMS),
    ("window-index-flipped", WindowFlipped, M.case_ssim_located, dict(), "outside the bound"),
    ("pooling-pads-bottom-right", PoolPadsHigh, M.case_avgpool, dict(), BITS),
    ("lowpass-clamp-one-short", ClampShort, M.case_lowpass, dict(C=8), BITS),
    ("adjoint-fold-weight-at-L1", FoldL1, M.case_lowpass, dict(C=8), "lowpass5_adjoint .*" + BITS),
    ("minmax-skips-last-pixel", MinmaxSkipsLast, M.case_minmax_located, dict(pixels=257, C=8, layout="ld16"), SUMS),
    ("div-vort-window-first", WindowFirst, M.case_div_vort, dict(shape=(2, 9, 13)), SUMS),
    ("moments-tail-dropped", TailDropped, M.case_moments, dict(sizes=(5, 7)), SUMS),
]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_located_mutation_is_rejected_by_its_case(mutant):
    _, cls, fn, kw, why = mutant
    fn(EmuOps("f32"), "f32", **kw)                                # the unmutated emulation passes the very same case
    _rejects(lambda: fn(cls("f32"), "f32", **kw), why)


def test_fold_mutant_is_caught_at_a_one_pixel_axis_only():
    """The L = 1 mutation leaves every L >= 2 shape alone: it is the (1, 1, 1), (1, 1, 7) and (2, 5, 1) shapes that catch it."""
    for L in (2, 3, 4, 5, 6, 9):
        assert torch.equal(FoldL1._fold_matrix(L), EmuOps._fold_matrix(L))
    assert float(EmuOps._fold_matrix(1)) == 5.0
    # the fold weights of the emulation against the map they are defined by
    for L in (1, 2, 3, 4, 5, 6, 9):
        A = torch.zeros(L, L)
        for dlt in range(-2, 3):
            for p, q in enumerate(M.clamp_map(L, dlt)):
                A[q, p] += 1
        assert torch.equal(A, EmuOps._fold_matrix(L)) and float(A.sum()) == 5.0 * L


def test_emulated_ssim_of_identical_planes_is_the_exact_count():
    """Case 5(a) on the emulation itself, outside the table: both sums of X == Y are the count of valid pixels."""
    p = M.ssim_params(M.gauss(7), *M.K_REF)
    X = torch.rand(1, 3, 46, 39, generator=torch.Generator().manual_seed(3))
    sums = torch.zeros(6)
    EmuOps("f32").ssim_level(X, X.clone(), p, sums)
    assert torch.equal(sums, torch.full((6,), 40.0 * 33.0))


def test_located_condition_holds_from_float64_alone():
    """The generator's own condition: at every position the smallest |map - 1| among the affected pixels is at least 8 x the bound."""
    p = M.ssim_params(M.G_ASYM, M.LOC_C, M.LOC_C)
    assert abs(sum(M.G_ASYM) - 1.0) == 0.0 and M.G_ASYM != M.G_ASYM[::-1]
    for pos in M.located_positions():
        M.located_reference(pos, p)
    assert M.located_additions() == 17


def test_divergence_and_vorticity_losses_on_the_emulation(monkeypatch):
    """GAN/losses.py's divergence / vorticity path on EmuOps.div_vort_sums: the reference's known answers and the CPU restatement."""
    from downgan_amd import backend
    from downgan_amd.GAN import losses
    from oracle import physics
    monkeypatch.setattr(backend, "make_ops", lambda dtype, device: EmuOps("f32"))
    monkeypatch.setattr(losses, "_ops", {})
    hr, fake = physics.reference_test_fixture()
    assert np.isclose(losses.divergence_loss(hr, fake).item(), physics.KNOWN["divergence"], atol=physics.KNOWN["atol"])
    assert np.isclose(losses.vorticity_loss(hr, fake).item(), physics.KNOWN["vorticity"], atol=physics.KNOWN["atol"])
    assert abs(losses.divergence_loss(hr, fake).item() - physics.divergence_loss(hr, fake)) < 1e-6
    assert abs(losses.vorticity_loss(hr, fake).item() - physics.vorticity_loss(hr, fake)) < 1e-6


def test_emulated_minmax_skips_nan_like_the_kernel():
    x = torch.tensor([[1.0, float("nan")], [float("nan"), float("nan")], [-2.0, float("nan")]]).view(1, 1, 3, 2)
    mm = torch.zeros(4)
    EmuOps("f32").minmax(x, 2, None, mm)
    assert mm.tolist() == [-2.0, 1.0, float("inf"), float("-inf")]
