"""The tables of tests/fp8_quant_ref.py through the CPU oracle (EmuOps.mx_quant, uq_quant, block_exp_max, exp_from_amax) against the
integer reference: every bf16 pattern and every fp32 cut / tail under every scale byte of EXPS, the leader / follower blocks of the
MX rule, the exponent chain at its edges.  That validates the reference, the tables and the steering of the GPU file
(tests/test_fp8_quant_exact_gpu.py) without a GPU.

The mutation checks apply one wrong rule each to a copy of the emulation's rule -- ties rounded away from zero, overflow written as
NaN, the maximum taken over 16 of the 32 channels, the scale exponent rounded instead of floored, subnormal inputs flushed to zero --
and require that the table fails, that the reported pattern belongs to the class the mutation acts on, and that no pattern outside
that class differs: the tables do reach each class, and the comparator does notice."""
import numpy as np
import pytest
import torch

from downgan_amd.ops import Conv
from oracle.emu_ops import EmuOps
from tests import fp8_quant_ref as R

TABLES = {"uniform_bf16": (R.uniform_bf16, "bf16"), "uniform_f32": (R.uniform_f32, "f32"),
          "mx_bf16": (R.mx_blocks_bf16, "bf16"), "mx_f32": (R.mx_blocks_f32, "f32")}


def col_exps(exps, shape):
    return np.broadcast_to(np.repeat(np.asarray(exps), 32), shape)


# ---------------------------------------------------------------------------------------------- the emulation against the reference
@pytest.mark.parametrize("name", ["uniform_bf16", "uniform_f32"])
def test_uq_quant_on_every_pattern_and_scale_edge(name):
    fn, fmt = TABLES[name]
    tab = fn()
    x = R.to_torch(tab, fmt)
    for rot in range(len(R.EXPS)):
        exps = R.rotated_exps(rot)
        q, _ = EmuOps.uq_quant(x, torch.from_numpy(exps))
        ref = R.ref_uniform(tab.reshape(-1, 4, 32), exps, fmt).reshape(tab.shape)
        msg = R.first_mismatch(q.numpy(), ref, tab, col_exps(exps, tab.shape))
        assert msg is None, f"{name} rotation {rot}: {msg}"


@pytest.mark.parametrize("name", sorted(TABLES))
def test_mx_quant_on_the_block_tables(name):
    fn, fmt = TABLES[name]
    tab = fn()
    q, s, _ = EmuOps.mx_quant(R.to_torch(tab, fmt))
    rq, rs = R.ref_mx(tab.reshape(-1, 4, 32), fmt)
    assert np.array_equal(s.numpy(), rs), np.argwhere(s.numpy() != rs)[:4].tolist()
    msg = R.first_mismatch(q.numpy(), rq.reshape(tab.shape), tab, np.broadcast_to(np.repeat(rs, 32, axis=-1), tab.shape))
    assert msg is None, f"{name}: {msg}"


def test_poisoned_block_has_scale_byte_247():
    """include/downgan_hip.h: a block that holds a NaN / Inf is 32 x 0x7F with scale byte 247 (exponent field 255 - 8)."""
    tab = R.mx_blocks_bf16()
    blocks = tab.reshape(-1, 32)
    non = (((blocks >> 7) & 0xff) == 255).any(-1)
    assert int(non.sum()) == 256
    q, s, _ = EmuOps.mx_quant(R.to_torch(tab, "bf16"))
    assert bool((s.numpy().reshape(-1)[non] == R.POISON_SCALE).all()) and bool((q.numpy().reshape(-1, 32)[non] == 0x7f).all())
    assert not bool((q.numpy().reshape(-1, 32)[~non] == 0x7f).any())


def test_reference_spot_values():
    """Hand-worked bytes: the reference is not only self-consistent."""
    one = 0x3f80
    assert R.ref_e4m3(one, 127).item() == 0x38                       # 1.0
    assert R.ref_e4m3(0x43e0, 127).item() == 0x7e                    # 448
    assert R.ref_e4m3(0x43e8, 127).item() == 0x7e                    # 464: the tie between 448 and 480 goes to the even 448
    assert R.ref_e4m3(0x43f0, 127).item() == 0x7e                    # 480 saturates
    assert R.ref_e4m3(0xc3f0, 127).item() == 0xfe
    assert R.ref_e4m3(0x3b00, 127).item() == 0x01                    # 2^-9: the smallest subnormal
    assert R.ref_e4m3(0x3a80, 127).item() == 0x00                    # 2^-10: tie between 0 and 2^-9 -> even
    assert R.ref_e4m3(0x3b40, 127).item() == 0x02                    # 1.5 * 2^-9 = tie between 1 and 2 units -> 2
    assert R.ref_e4m3(0x3f88, 127).item() == 0x38                    # 1 + 2^-4: tie, kept mantissa even -> down
    assert R.ref_e4m3(0x3f98, 127).item() == 0x3a                    # 1.1875: tie, kept mantissa odd -> up
    assert R.ref_e4m3(0x3f80, 254).item() == 0x00 and R.ref_e4m3(0x7f7f, 254).item() == 0x40   # 2^-127 scale: 3.39e38 / 2^127 ~ 1.99 -> 2.0
    assert R.ref_e4m3(0x0001, 0).item() == 0x08 and R.ref_e4m3(0x0040, 0).item() == 0x38       # bf16 subnormals 2^-133 and 2^-127 over 2^-127: 2^-6 and 1
    assert R.ref_e4m3(0x3f800000, 127, "f32").item() == 0x38 and R.ref_e4m3(0x3f880001, 127, "f32").item() == 0x39


@pytest.mark.parametrize("nb", [4, 12, 28, 64])
def test_block_exp_max_of_the_emulation(nb):
    emu = EmuOps("f32")
    for rows in (1, 3, 64 * (256 // (nb // 4)) + 37):
        for margin in (0, 1, 8):
            sc, old, want = R.exp_case(rows, nb, nb + 8, margin, seed=rows + margin)
            out = torch.from_numpy(old.copy())
            emu.block_exp_max(torch.from_numpy(sc)[:, :nb], out, margin=margin)
            assert np.array_equal(out.numpy(), want), (rows, nb, margin)


@pytest.mark.parametrize("nb", [4, 17, 64])
def test_exp_from_amax_of_the_emulation(nb):
    emu = EmuOps("f32")
    for margin in (0, 1, 8):
        for seed in range(5):
            a, old, want = R.amax_case(nb, margin, seed)
            census = torch.from_numpy(a.astype(np.uint32).view(np.int32).copy())
            out = torch.from_numpy(old.copy())
            emu.exp_from_amax(census, out, margin=margin)
            assert np.array_equal(out.numpy(), want), (nb, margin, seed, out.tolist(), want.tolist())
            assert int(census.abs().sum()) == 0


def test_exp_cases_reach_their_edges():
    seen_old, seen_out = set(), set()
    for margin in (0, 1, 8):
        sc, old, want = R.exp_case(3, 12, 12, margin, seed=margin)
        v = sc.astype(np.int64).max(0) + margin
        seen_old |= {("zero", 0), ("one", 1)} & {("zero", int(old[0])), ("one", int(old[1]))}
        assert int(old[2]) == min(254, int(v[2]) + 1) and int(want[2]) == min(254, int(v[2]))       # v + 1: no decay
        assert int(old[3]) == min(254, int(v[3]) + 2) and int(want[3]) == int(old[3]) - 1          # v + 2: falls by one only
        assert int(want[1]) == 254 and int(want[0]) == margin
        seen_out |= set(want.tolist())
    assert {0, 254} <= seen_out
    a, _, _ = R.amax_case(64, 1, 0)
    assert {0, 1, 246, 247} <= set(R.scale_byte_of_bits(a).tolist())


# ---------------------------------------------------------------------------------------------------------- steering of the GPU file
def test_straight_line_keys_are_those_of_the_dispatch_switch():
    """The GPU file states for each fused launch whether its key has a straight-line epilogue instance or falls to the general one;
    the list it uses must be the `case` labels of halo_epilogue's switch."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "downgan_amd", "csrc", "gg_common.h")).read()
    body = src[src.index("switch (key) {"):]
    body = body[:body.index("default: run(")]
    cases = {int(m) for m in re.findall(r"case (\d+): run\(std::integral_constant<int, \1>", body)}
    assert cases == set(R.STRAIGHT_LINE), sorted(cases ^ set(R.STRAIGHT_LINE))
    assert R.epi_key(act=1.0, out_q=1, out_u=1) == 2305 and R.epi_key(r1=1, out_q=1, out_u=1, act=1.0) == 2313
    assert R.epi_key(mask_bits=1, out_q=1, out_u=1, skip_y=True) == 6402 and R.epi_key(mask=1, out_q=1) == 288


def test_first_layer_steering_is_exact_on_the_oracle():
    xg, w, bias, d, drop_c = R.first_layer_steering()
    _, H, W, _ = xg.shape
    emu = EmuOps("bf16", f8_critic=True)
    cv = Conv(1, H, W, 16, 128, 1, False, cin_real=2, net="C")
    x = R.to_torch(xg.reshape(-1, 16), "bf16").reshape(1, H, W, 16)
    y = torch.zeros(1, H, W, 128, dtype=torch.bfloat16)
    emu.conv_fwd(cv, x, torch.from_numpy(w).reshape(-1).to(torch.bfloat16), y, bias=torch.from_numpy(bias))
    want = (x[..., 0:1].float() * torch.from_numpy(np.ldexp(np.float32(1), -d))).to(torch.bfloat16)
    want[..., drop_c] = 0
    assert torch.equal(want.view(torch.int16) & 0x7fff, y.view(torch.int16) & 0x7fff)
    assert (H * W) % 64 != 0 and len(R.dm_pairs(R.from_torch(y).reshape(-1, 4, 32))) == 21 * 128
    lead = np.array([int(np.argmin(d[32 * b:32 * b + 32])) for b in range(4)])
    assert tuple(lead) == R.LANES


def test_stride2_data_gradient_steering_is_exact_on_the_oracle():
    dyg, wd, d, vals = R.s2_dgrad_steering()
    _, Ho, Wo, _ = dyg.shape
    emu = EmuOps("bf16", f8_critic=True)
    cv = Conv(1, 2 * Ho, 2 * Wo, 128, 256, 2, False, net="C")
    assert emu.f8_eligible(cv, "dgrad")
    dy = R.to_torch(dyg.reshape(-1, 256), "bf16").reshape(1, Ho, Wo, 256)
    dx = torch.zeros(1, 2 * Ho, 2 * Wo, 128, dtype=torch.bfloat16)
    emu.conv_dgrad(cv, dy, torch.from_numpy(wd).reshape(-1).to(torch.bfloat16), dx)
    v = np.zeros(Ho * Wo, dtype=np.int64); v[:vals.size] = vals
    want = (R.to_torch(v.reshape(-1, 1), "bf16").float().reshape(1, Ho, Wo, 1) * torch.from_numpy(np.ldexp(np.float32(1), -d))).to(torch.bfloat16)
    assert torch.equal(want.repeat_interleave(2, 1).repeat_interleave(2, 2), dx)
    assert len(R.dm_pairs(R.from_torch(dx).reshape(-1, 4, 32))) == 21 * 128


# ------------------------------------------------------------------------------------------------------------------ mutations
def cast_rne(v):
    return v.to(torch.float8_e4m3fn).view(torch.uint8)


def cast_ties_away(v):
    """torch's cast, except that an exact tie goes to the neighbour of larger magnitude."""
    q = cast_rne(v).to(torch.int32)
    code, sign = q & 0x7f, q & 0x80
    mag = v.double().abs()
    deq = lambda c: c.to(torch.uint8).view(torch.float8_e4m3fn).double()
    other = torch.where(deq(code) > mag, code - 1, code + 1).clamp(0, 0x7e)
    tie = (deq(code) - mag).abs() == (deq(other) - mag).abs()
    return torch.where(tie & (other > code), other, code).bitwise_or(sign).to(torch.uint8)


def uq_rule(x, exps, cast=cast_rne, clamp=True, flush=False):
    """EmuOps.uq_quant, restated with the places the mutations act on."""
    Cc = x.shape[-1]
    v = x.float().reshape(-1, Cc // 32, 32)
    if flush:
        v = torch.where(((v.view(torch.int32) >> 23) & 0xff) == 0, torch.zeros(()), v)
    scale = torch.ldexp(torch.ones(Cc // 32), exps.reshape(-1).int() - 127).view(1, -1, 1)
    t = v / scale
    q8 = cast(t.clamp(-448.0, 448.0) if clamp else t)
    q8 = torch.where(torch.isfinite(v.abs().amax(-1))[..., None], q8, torch.full_like(q8, 0x7F))
    return q8.reshape(x.shape)


def mx_rule(x, lanes=32, rounded=False, flush=False):
    """EmuOps.mx_quant, restated likewise."""
    Cc = x.shape[-1]
    v = x.float().reshape(-1, Cc // 32, 32)
    if flush:
        v = torch.where(((v.view(torch.int32) >> 23) & 0xff) == 0, torch.zeros(()), v)
    amax = v.abs()[..., :lanes].amax(-1)
    bits = amax.contiguous().view(torch.int32)
    if rounded:                                           # round(log2 amax): up from a mantissa of sqrt(2)
        bits = bits + torch.where(((bits & 0x7fffff) >= 0x3504f3) & (bits < 0x7f800000), 1 << 23, 0).to(torch.int32)
    e = (((bits >> 23) & 0xff) - 8).clamp(min=0)
    scale = torch.ldexp(torch.ones_like(amax), e - 127)
    q8 = cast_rne((v / scale[..., None]).clamp(-448.0, 448.0))
    q8 = torch.where(torch.isfinite(v.abs().amax(-1))[..., None], q8, torch.full_like(q8, 0x7F))
    return q8.reshape(x.shape), e.to(torch.uint8)


def uniform_runs(name, **mut):
    """-> per rotation (table, reference info, bytes of the mutated rule, differing elements)."""
    fn, fmt = TABLES[name]
    tab = fn()
    x = R.to_torch(tab, fmt)
    for rot in range(len(R.EXPS)):
        exps = R.rotated_exps(rot)
        info = R.ref_uniform_info(tab.reshape(-1, 4, 32), exps, fmt)
        got = uq_rule(x, torch.from_numpy(exps), **mut).numpy().reshape(-1, 4, 32)
        yield tab.reshape(-1, 4, 32), info, got, ~R.bytes_match(got, info["byte"]), exps


def test_the_restated_rules_are_the_emulation():
    for name, (fn, fmt) in TABLES.items():
        x = R.to_torch(fn(), fmt)
        exps = torch.from_numpy(R.rotated_exps(3))
        assert torch.equal(uq_rule(x, exps), EmuOps.uq_quant(x, exps)[0])
        q, s, _ = EmuOps.mx_quant(x)
        q2, s2 = mx_rule(x)
        assert torch.equal(q, q2) and torch.equal(s.reshape(-1), s2.reshape(-1))


@pytest.mark.parametrize("name", ["uniform_bf16", "uniform_f32"])
def test_mutation_ties_away_from_zero_is_caught_at_ties(name):
    classes = set()
    for tab, info, got, bad, exps in uniform_runs(name, cast=cast_ties_away):
        assert not bool((bad & ~info["tie"]).any()), "a pattern that is no tie differs"
        if bad.any():
            first = tuple(np.argwhere(bad)[0])
            assert info["tie"][first] and not info["odd"][first]             # ties to even go wrong where the kept integer is even
            classes |= R.tie_classes({k: (v & bad if k == "tie" else v) for k, v in info.items()})
    assert {("normal", "even"), (-7, "even"), (-8, "even"), (-10, "even")} <= classes, classes


@pytest.mark.parametrize("name", ["uniform_bf16", "uniform_f32"])
def test_mutation_overflow_as_nan_is_caught_at_saturation(name):
    n = 0
    for tab, info, got, bad, exps in uniform_runs(name, clamp=False):
        assert not bool((bad & ~info["sat"]).any()), "a pattern that does not saturate differs"
        if bad.any():
            first = tuple(np.argwhere(bad)[0])
            assert int(info["byte"][first]) & 0x7f == 0x7e and int(got[first]) & 0x7f == 0x7f
            n += int(bad.sum())
    assert n > 1000


@pytest.mark.parametrize("name", ["uniform_bf16", "uniform_f32"])
def test_mutation_flushed_subnormals_is_caught_at_subnormal_inputs(name):
    fmt = TABLES[name][1]
    n = 0
    for tab, info, got, bad, exps in uniform_runs(name, flush=True):
        b32 = R.f32_bits(tab, fmt)
        sub = (((b32 >> 23) & 0xff) == 0) & ((b32 & 0x7fffff) != 0)
        assert not bool((bad & ~sub).any()), "a pattern that is no subnormal differs"
        if bad.any():
            first = tuple(np.argwhere(bad)[0])
            assert sub[first] and int(exps[first[1]]) <= 9 and int(got[first]) & 0x7f == 0
            n += int(bad.sum())
    assert n > 100


@pytest.mark.parametrize("name", ["mx_bf16", "mx_f32"])
def test_mutation_maximum_over_16_channels_is_caught_at_leaders_in_the_upper_half(name):
    fn, fmt = TABLES[name]
    tab = fn()
    blocks = tab.reshape(-1, 32)
    _, rs = R.ref_mx(blocks, fmt)
    _, s = mx_rule(R.to_torch(tab, fmt), lanes=16)
    bad = s.numpy().reshape(-1) != rs
    mag = R.f32_bits(blocks, fmt) & 0x7fffffff
    upper = (mag[:, 16:].max(-1) >> 23) > (mag[:, :16].max(-1) >> 23)        # the exponent is set by lanes 16 .. 31 alone
    assert bad.any() and np.array_equal(bad, upper & (rs > 0) | bad & upper), "scale bytes differ outside the blocks led from the upper half"
    assert not bool((bad & ~upper).any())
    first = int(np.argwhere(bad)[0][0])
    assert int(mag[first].argmax()) in (16, 31), int(mag[first].argmax())
    assert {int(mag[i].argmax()) for i in np.argwhere(bad).reshape(-1)} >= {16, 31}


@pytest.mark.parametrize("name", ["mx_bf16", "mx_f32"])
def test_mutation_rounded_scale_exponent_is_caught_at_large_mantissas(name):
    fn, fmt = TABLES[name]
    tab = fn()
    blocks = tab.reshape(-1, 32)
    _, rs = R.ref_mx(blocks, fmt)
    _, s = mx_rule(R.to_torch(tab, fmt), rounded=True)
    bad = s.numpy().reshape(-1) != rs
    amax = (R.f32_bits(blocks, fmt) & 0x7fffffff).max(-1)
    assert bad.any() and not bool((bad & ((amax & 0x7fffff) < 0x3504f3)).any()), "a block whose largest mantissa is below sqrt(2) differs"
    first = int(np.argwhere(bad)[0][0])
    assert (int(amax[first]) & 0x7fffff) >= 0x3504f3 and int(s.reshape(-1)[first]) == int(rs[first]) + 1


@pytest.mark.parametrize("name", ["mx_bf16", "mx_f32"])
def test_mutation_flushed_subnormals_is_caught_in_the_blocks(name):
    fn, fmt = TABLES[name]
    tab = fn()
    rq, rs = R.ref_mx(tab.reshape(-1, 4, 32), fmt)
    q, s = mx_rule(R.to_torch(tab, fmt), flush=True)
    bad = ~R.bytes_match(q.numpy().reshape(rq.shape), rq)
    b32 = R.f32_bits(tab.reshape(rq.shape), fmt)
    sub = (((b32 >> 23) & 0xff) == 0) & ((b32 & 0x7fffff) != 0)
    assert bad.any() and not bool((bad & ~sub).any())
    assert sub[tuple(np.argwhere(bad)[0])]
