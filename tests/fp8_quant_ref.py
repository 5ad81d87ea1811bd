"""Integer reference of the fp8 quantisers and the value tables the exact quantiser tests run on (CPU: test_fp8_quant_exact_cpu.py
against oracle/emu_ops.py; GPU: test_fp8_quant_exact_gpu.py against csrc/quant.hip and the fused copies of csrc/gg_common.h).

The reference works on bit patterns only -- shift, remainder, compare on int64 -- and shares nothing with the implementations it
judges: no float division, no float8 cast, nothing of oracle/ or EmuOps.  A source value is sig * 2^(Ex - 150) (sig = the 24-bit
significand of its fp32 pattern, Ex = max(1, exponent field)); divided by 2^(e - 127) it is sig * 2^(Ex - e - 23), which is rounded
to nearest even on the OCP E4M3 grid (step 2^(k - 3) in the binade [2^k, 2^(k + 1)), k >= -6; step 2^-9 below 2^-6) and saturated
at +-448 (0x7E / 0xFE).  A bf16 pattern is the fp32 pattern with sixteen zero bits behind it.

Every table function asserts its own coverage from the reference alone (`assert_coverage`): all 254 finite non-zero E4M3 codes,
both zeros, both saturated codes reached by a magnitude above 448, 0x7F by poison, and every exact-tie class (normal range and
each subnormal binade that can tie, kept mantissa even and odd where both exist)."""
import functools

import numpy as np

EXPS_EDGE = (0, 1, 2, 7, 8, 9, 245, 246, 247, 253, 254)
EXPS_MID = (100, 119, 127, 135, 150)
EXPS = EXPS_EDGE + EXPS_MID                                 # 16 scale bytes: four column blocks x four groups, rotated
TAILS16 = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)   # the bits an fp32 source carries behind a bf16 pattern
MX_E = (0, 1, 7, 8, 9, 10, 119, 127, 135, 253, 254)          # exponent fields of the block leaders
LANES = (0, 15, 16, 31)
POISON_SCALE = 247                                           # scale byte of a block that holds a NaN / Inf: 255 - 8


def f32_bits(bits, fmt):
    """bf16 patterns (fmt 'bf16') or fp32 patterns (fmt 'f32') -> fp32 patterns as int64."""
    b = np.asarray(bits).astype(np.int64)
    return (b & 0xffff) << 16 if fmt == "bf16" else b & 0xffffffff


def _decompose(b32):
    E = (b32 >> 23) & 0xff
    m = b32 & 0x7fffff
    sig = np.where(E > 0, m | (1 << 23), m)
    return (b32 >> 31) & 1, E, sig, np.maximum(E, 1)


def _bit_length(sig):
    L = np.zeros_like(sig)
    for i in range(24):
        L += (sig >= (1 << i)).astype(np.int64)
    return L


def ref_e4m3_info(bits, e, fmt="bf16"):
    """-> dict of int64 / bool arrays: byte (the E4M3 code; 0x7F for a NaN / Inf source), sat (magnitude above 448), tie (the dropped
    bits were exactly half a step), odd (parity of the kept integer before rounding), k (floor(log2 |quotient|), -99 for zero)."""
    b32 = f32_bits(bits, fmt)
    e = np.broadcast_to(np.asarray(e).astype(np.int64), b32.shape)
    sign, E, sig, Ex = _decompose(b32)
    L = _bit_length(sig)
    t = Ex - e - 23                                           # |quotient| = sig * 2^t
    k = L - 1 + t                                             # floor(log2 |quotient|) where sig > 0
    big = (k >= 9) & (sig > 0)                                # >= 512: saturates whatever the mantissa
    s = np.maximum(k, -6) - 3                                 # exponent of the grid step
    shift = np.clip(s - t, -3, 40)                            # k < 9 keeps a left shift within 3 bits; 40 bits clear any 24-bit sig
    right = np.maximum(shift, 0)
    n = np.where(shift >= 0, sig >> right, sig << np.maximum(-shift, 0))
    rem = np.where(shift > 0, sig & ((np.int64(1) << right) - 1), 0)
    half = np.where(shift > 0, np.int64(1) << np.maximum(right - 1, 0), 1)
    tie = (shift > 0) & (rem == half) & ~big
    odd = (n & 1) == 1
    n = n + ((rem > half) | (tie & odd)).astype(np.int64)
    normal = k >= -6
    carry = normal & (n == 16)                                # rounded up into the next binade
    kk = np.where(carry, k + 1, k)
    nn = np.where(carry, 8, n)
    code = np.where(normal, ((kk + 7) << 3) | (nn - 8), n)    # subnormal: code = n (n == 8 is the smallest normal, 0x08)
    sat = big | (normal & (code >= 0x7f))
    code = np.where(sat, 0x7e, code)
    code = np.where(sig == 0, 0, code)
    byte = (sign << 7) | code
    nonfinite = E == 255
    byte = np.where(nonfinite, 0x7f, byte)
    fin = ~nonfinite
    return dict(byte=byte, sat=sat & fin & (sig > 0), tie=tie & fin & (sig > 0), odd=odd, k=np.where((sig > 0) & fin, k, -99), nonfinite=nonfinite)


def ref_e4m3(bits, e, fmt="bf16"):
    """Source bit pattern(s) and scale byte(s) -> the byte OCP E4M3 gives for x / 2^(e - 127) (0x7F for a NaN / Inf source)."""
    return ref_e4m3_info(bits, e, fmt)["byte"].astype(np.uint8)


def _poison(info, nonfinite_block):
    out = dict(info)
    p = np.broadcast_to(nonfinite_block[..., None], info["byte"].shape)
    out["byte"] = np.where(p, 0x7f, info["byte"])
    for key in ("sat", "tie"):
        out[key] = info[key] & ~p
    out["k"] = np.where(p, -99, info["k"])
    out["poison"] = p
    return out


def ref_uniform_info(blocks, exps, fmt="bf16"):
    """blocks [..., nb, 32] patterns, exps [nb] -> info of the uniform-scale copy: a block that holds a NaN / Inf is 32 x 0x7F."""
    b32 = f32_bits(blocks, fmt)
    info = ref_e4m3_info(blocks, np.asarray(exps).astype(np.int64)[:, None], fmt)
    return _poison(info, (((b32 >> 23) & 0xff) == 255).any(-1))


def ref_uniform(blocks, exps, fmt="bf16"):
    return ref_uniform_info(blocks, exps, fmt)["byte"].astype(np.uint8)


def mx_scale_bytes(blocks, fmt="bf16"):
    """Block rule of include/downgan_hip.h: max(0, exponent field of the largest magnitude - 8); a NaN / Inf has field 255 -> 247."""
    b32 = f32_bits(blocks, fmt)
    return np.maximum(((b32 & 0x7fffffff).max(-1) >> 23) - 8, 0)


def ref_mx_info(blocks, fmt="bf16"):
    b32 = f32_bits(blocks, fmt)
    sc = mx_scale_bytes(blocks, fmt)
    info = _poison(ref_e4m3_info(blocks, sc[..., None], fmt), (((b32 >> 23) & 0xff) == 255).any(-1))
    info["scale"] = sc
    return info


def ref_mx(blocks, fmt="bf16"):
    """blocks [..., 32] patterns -> (bytes uint8 [..., 32], scale bytes uint8 [...])."""
    info = ref_mx_info(blocks, fmt)
    return info["byte"].astype(np.uint8), info["scale"].astype(np.uint8)


def bytes_match(got, ref):
    """Equality of bytes, except that either zero byte is accepted where the reference is +-0."""
    got, ref = np.asarray(got).astype(np.int64), np.asarray(ref).astype(np.int64)
    return (got == ref) | (((ref & 0x7f) == 0) & ((got & 0x7f) == 0))


def first_mismatch(got, ref, src=None, exps=None):
    """None, or a description of the first differing element (index, source pattern, scale byte, both bytes)."""
    bad = ~bytes_match(got, ref)
    if not bad.any():
        return None
    idx = tuple(int(i) for i in np.argwhere(bad)[0])
    msg = f"{int(bad.sum())} bytes differ; first at {idx}: got 0x{int(np.asarray(got)[idx]):02x}, reference 0x{int(np.asarray(ref)[idx]):02x}"
    if src is not None:
        msg += f", source pattern 0x{int(np.asarray(src)[idx]):x}"
    if exps is not None:
        ex = np.broadcast_to(np.asarray(exps), bad.shape)
        per = {int(e): int((bad & (ex == e)).sum()) for e in np.unique(ex[bad])}
        msg += f", scale byte {int(ex[idx])}; differing bytes per scale byte {per}"
    return msg


# ---------------------------------------------------------------------------------------------------------------- coverage
TIE_CLASSES = ([("normal", p) for p in ("even", "odd")] + [(-7, "even"), (-7, "odd"), (-8, "even"), (-8, "odd"), (-9, "odd"), (-10, "even")])


def tie_classes(info):
    """The exact-tie classes present: ('normal', parity) for k >= -6 and (k, parity) for the subnormal binades -7 .. -10 (at k = -9 the
    kept integer is 1, at k = -10 it is 0: one parity each)."""
    got = set()
    tie, k, odd = info["tie"], info["k"], info["odd"]
    for par, sel in (("even", ~odd), ("odd", odd)):
        if (tie & sel & (k >= -6)).any():
            got.add(("normal", par))
        for kk in (-7, -8, -9, -10):
            if (tie & sel & (k == kk)).any():
                got.add((kk, par))
    return got


def assert_coverage(infos, what):
    """A condition on the table, judged from the reference alone."""
    codes, ties = set(), set()
    sat = {0x7e: False, 0xfe: False}
    poison = False
    for info in infos:
        byte = info["byte"]
        codes |= set(np.unique(byte).tolist())
        for c in sat:
            sat[c] = sat[c] or bool((info["sat"] & (byte == c)).any())
        poison = poison or bool((info.get("poison", np.zeros(1, dtype=bool)) & (byte == 0x7f)).any())
        ties |= tie_classes(info)
    want = set(range(0x00, 0x7f)) | set(range(0x80, 0xff))
    assert want <= codes, (what, "missing codes", sorted(hex(c) for c in want - codes))
    assert all(sat.values()), (what, "saturation not reached", sat)
    assert poison, (what, "no poisoned block")
    assert set(TIE_CLASSES) <= ties, (what, "missing tie classes", sorted(map(str, set(TIE_CLASSES) - ties)))


# ------------------------------------------------------------------------------------------------------------------ tables
def rotated_exps(rot, nb=4):
    """Scale bytes of the nb column blocks in launch `rot`: over the 16 launches every column meets every entry of EXPS."""
    return np.array([EXPS[(j + rot) % len(EXPS)] for j in range(nb)], dtype=np.uint8)


def _rows128(flat, pad):
    n = -(-flat.size // 128) * 128
    return np.concatenate([flat, np.full(n - flat.size, pad, dtype=flat.dtype)]).reshape(-1, 128)


def _nonfinite_blocks(patterns, filler):
    """One block per non-finite pattern: alone among finite values (filler[i], cycled), at lane 0, 15, 16, 31 in turn."""
    blocks = np.empty((len(patterns), 32), dtype=np.int64)
    for i, p in enumerate(patterns):
        blocks[i] = np.roll(filler, i)[:32]
        blocks[i, LANES[i % 4]] = p
    return blocks


@functools.lru_cache(maxsize=None)
def uniform_bf16():
    """[rows, 128] int64 bf16 patterns: all 65 280 finite ones 32 to a block, then each of the 256 non-finite ones alone in a block of
    finite values; rows = 574 (no multiple of a 256-thread workgroup's 64 rows)."""
    allp = np.arange(65536, dtype=np.int64)
    fin = allp[((allp >> 7) & 0xff) != 255]
    non = allp[((allp >> 7) & 0xff) == 255]
    assert fin.size == 65280 and non.size == 256
    tab = np.concatenate([fin.reshape(-1, 32), _nonfinite_blocks(non, fin[0x3c00:0x3c00 + 512:3])]).reshape(-1, 128)
    assert tab.shape == (574, 128) and np.unique(tab).size == 65536
    infos = [ref_uniform_info(tab.reshape(-1, 4, 32), rotated_exps(r), "bf16") for r in range(len(EXPS))]
    assert_coverage(infos, "UNIFORM_BF16")
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def uniform_f32():
    """[rows, 128] int64 fp32 patterns: every sign, exponent field and cut (19 .. 23 dropped mantissa bits), all values of the kept
    bits times the tails {0, 1, half - 1, half, half + 1, all ones}; the non-finite fields in rows of their own."""
    vals = []
    for cut in range(19, 24):
        kept = np.arange(1 << (23 - cut), dtype=np.int64) << cut
        half = 1 << (cut - 1)
        tails = np.array([0, 1, half - 1, half, half + 1, (1 << cut) - 1], dtype=np.int64)
        vals.append((kept[:, None] | tails[None, :]).reshape(-1))
    mant = np.concatenate(vals)                                   # 186 mantissas
    E = np.arange(256, dtype=np.int64)
    pat = ((np.arange(2, dtype=np.int64)[:, None, None] << 31) | (E[None, :, None] << 23) | mant[None, None, :])
    fin = pat[:, :255, :].transpose(1, 0, 2).reshape(-1)          # exponent field slowest: a block holds neighbours in magnitude
    non = pat[:, 255, :].reshape(-1)
    tab = np.concatenate([_rows128(fin, 0), _rows128(non, 0x7fc00000)])
    assert tab.shape[0] % 64 != 0 and fin.size + non.size == 2 * 256 * 186
    infos = [ref_uniform_info(tab.reshape(-1, 4, 32), rotated_exps(r), "f32") for r in range(len(EXPS))]
    assert_coverage(infos, "UNIFORM_F32")
    tab.setflags(write=False)
    return tab


def _mx_blocks_for(Ef, fmt):
    """Blocks whose leader has exponent field Ef: every mantissa, sign and lane of LANES for the leader; the followers run through every
    (d, mantissa, sign), d = Ef - exponent field in 0 .. 20 (as far as the field stays >= 0) -- with every tail of TAILS16 in fp32."""
    sh = 16 if fmt == "f32" else 0
    ds = np.arange(0, min(20, Ef) + 1, dtype=np.int64)
    fol = ((np.arange(2, dtype=np.int64)[None, None, :] << 15) | ((Ef - ds)[:, None, None] << 7) | np.arange(128, dtype=np.int64)[None, :, None]).reshape(-1)
    if fmt == "f32":
        fol = ((fol[:, None] << 16) | np.array(TAILS16, dtype=np.int64)[None, :]).reshape(-1)
    lead = ((np.arange(2, dtype=np.int64)[:, None] << 15) | (Ef << 7) | np.arange(128, dtype=np.int64)[None, :]).reshape(-1)
    nblk = max(4 * lead.size, -(-fol.size // 31))
    blocks = np.resize(fol, nblk * 31).reshape(nblk, 31)
    out = np.empty((nblk, 32), dtype=np.int64)
    for i, lane in enumerate(LANES):
        sel = np.arange(i, nblk, 4)
        ld = lead[(sel // 4) % lead.size] << sh
        if fmt == "f32":                                          # the largest fp32 value of the binade still has field Ef: floor, not round
            ld = np.where((sel // 4) % 2 == 1, ld | 0xffff, ld)
        out[sel] = np.insert(blocks[sel], lane, ld, axis=1)
    return out


def _mx_table(fmt):
    sh = 16 if fmt == "f32" else 0
    parts = [_mx_blocks_for(Ef, fmt) for Ef in MX_E]
    zero = np.zeros((1, 32), dtype=np.int64)
    equal = np.full((2, 32), 0x40b3 << sh, dtype=np.int64)          # 32 equal magnitudes (5.59375), mixed signs in the second
    equal[1, ::3] |= 0x8000 << sh
    non16 = np.arange(65536, dtype=np.int64)
    non16 = non16[((non16 >> 7) & 0xff) == 255]
    filler = (np.arange(0x3c00, 0x3c00 + 512, 3, dtype=np.int64)) << sh
    nonb = _nonfinite_blocks(non16 << sh, filler)
    blocks = np.concatenate(parts + [zero, equal, nonb])
    pad = (-blocks.shape[0]) % 4
    blocks = np.concatenate([blocks, np.zeros((pad, 32), dtype=np.int64)])
    tab = blocks.reshape(-1, 128)
    info = ref_mx_info(blocks, fmt)
    assert_coverage([info], f"MX_BLOCKS[{fmt}]")
    sc = set(np.unique(info["scale"]).tolist())
    assert {0, 1, 2, 111, 119, 127, 245, 246, POISON_SCALE} <= sc, sorted(sc)
    tab.setflags(write=False)
    return tab


@functools.lru_cache(maxsize=None)
def mx_blocks_bf16():
    return _mx_table("bf16")


@functools.lru_cache(maxsize=None)
def mx_blocks_f32():
    return _mx_table("f32")


def to_torch(tab, fmt):
    """[rows, C] int64 patterns -> a torch tensor of that dtype with exactly those bits."""
    import torch
    if fmt == "bf16":
        return torch.from_numpy(tab.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)
    return torch.from_numpy(tab.astype(np.uint32).view(np.int32).copy()).view(torch.float32)


def from_torch(t):
    """A bf16 / fp32 torch tensor (CPU) -> its bit patterns as int64."""
    import torch
    if t.dtype == torch.bfloat16:
        return t.contiguous().view(torch.int16).numpy().astype(np.int64) & 0xffff
    return t.contiguous().view(torch.int32).numpy().astype(np.int64) & 0xffffffff


def finite_rows(tab, fmt):
    """The rows of a table that hold no NaN / Inf (identity steering multiplies neighbours by zero: Inf * 0 would be NaN)."""
    E = (f32_bits(tab, fmt) >> 23) & 0xff
    return tab[(E != 255).all(-1)]


def grid_for(rows, W=40):
    """(H, W) of the smallest grid of 40-pixel rows that holds `rows` pixels and ends in a partial 64-pixel tile."""
    H = -(-rows // W)
    while (H * W) % 64 == 0:
        H += 1
    return H, W


def as_grid(tab, H, W):
    """[rows, C] -> [1, H, W, C], zero pixels behind the table."""
    out = np.zeros((H * W, tab.shape[1]), dtype=np.int64)
    out[:tab.shape[0]] = tab
    return out.reshape(1, H, W, tab.shape[1])


# ---------------------------------------------------------------------------------------------------------- exponent chain
def scale_byte_of_bits(amax_bits):
    """E8M0 byte of a magnitude given as an fp32 bit pattern: max(0, exponent field - 8)."""
    return np.maximum(((np.asarray(amax_bits).astype(np.int64) >> 23) & 0xff) - 8, 0)


def exp_update_ref(v, old, margin):
    """dg_block_exp_max / dg_exp_from_amax after the maximum: add the margin, fall by at most one below a non-zero old value, clamp."""
    v = np.asarray(v).astype(np.int64) + int(margin)
    old = np.asarray(old).astype(np.int64)
    v = np.where((old > 0) & (v + 1 < old), old - 1, v)
    return np.minimum(v, 254)


def exp_case(rows, nb, ld, margin, seed):
    """-> (scales uint8 [rows, ld], old uint8 [nb], expected uint8 [nb]): column 0 all zero, column 1 holds a 254, the others random in
    0 .. 254 with their maximum in one random row; old = 0, 1, v + 1, v + 2, 254 in turn (v = maximum + margin)."""
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 200, size=(rows, ld), dtype=np.int64)
    sc[:, 0] = 0
    sc[rng.integers(0, rows), 1] = 254
    for b in range(2, nb):
        sc[rng.integers(0, rows), b] = 200 + (b * 7) % 55
    v = sc[:, :nb].max(0) + margin
    old = np.array([(0, 1, v[b] + 1, v[b] + 2, 254)[b % 5] for b in range(nb)], dtype=np.int64)
    old = np.minimum(old, 254)
    return sc.astype(np.uint8), old.astype(np.uint8), exp_update_ref(sc[:, :nb].max(0), old, margin).astype(np.uint8)


AMAX_PATTERNS = (0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x03ffffff, 0x04000000, 0x047fffff, 0x04800000, 0x3f800000,
                 0x3fffffff, 0x43e00000, 0x7b000000, 0x7b7fffff, 0x7effffff, 0x7f7fffff, 0x7f800000, 0x7fc00000)


def amax_case(nb, margin, seed):
    """-> (census int64 [nb] bit patterns, old [nb], expected [nb]) for dg_exp_from_amax: the edges of AMAX_PATTERNS, then random."""
    rng = np.random.default_rng(seed)
    a = np.array([AMAX_PATTERNS[i] if i < len(AMAX_PATTERNS) else int(rng.integers(0, 0x7f800000)) for i in range(nb)], dtype=np.int64)
    a = np.roll(a, seed % nb)
    v = scale_byte_of_bits(a)
    old = np.minimum(np.array([(0, 1, v[b] + margin + 1, v[b] + margin + 2, 254)[(b + seed) % 5] for b in range(nb)], dtype=np.int64), 254)
    return a, old.astype(np.uint8), exp_update_ref(v, old, margin).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------- steering
def dm_pairs(ybits, fmt="bf16"):
    """The distinct (d, mantissa) pairs of the non-zero finite elements of blocks [..., 32] of bf16 patterns, d = exponent field of
    the block's largest magnitude - exponent field of the element, d <= 20: what a fused launch's stored output offers its quantiser."""
    b = np.asarray(ybits).astype(np.int64).reshape(-1, 32)
    E = (b >> 7) & 0xff
    lead = ((b & 0x7fff).max(-1) >> 7)[:, None]
    ok = ((b & 0x7fff) != 0) & (lead != 255) & (lead - E <= 20)
    return set(zip((lead - E)[ok].tolist(), (b & 0x7f)[ok].tolist()))


DROP_B = 100       # the detector channel of the first-layer steering: bias 2^100 cancelled by -2^100 * 1.0 at every REAL pixel


def first_layer_steering():
    """Critic features.0 geometry (16 -> 128 channels, two real inputs) steered onto the tables: channel 0 of pixel p holds a table
    value (every leader exponent of MX_E x 128 mantissas x both signs), channel 1 holds 1.0; output channel c multiplies channel 0 by
    2^-d(c) on the centre tap, d = 0 for the block's leader lane (LANES[block]) and 1 .. 20 in turn for the followers.  Channel
    DROP_C has weight 0 on the table value, -2^100 on the 1.0 and bias 2^100: exactly 0 at every pixel of the tensor, 2^100 at any
    pixel a kernel computed behind its end (inputs read as 0), which must not reach the census.  (The first-layer kernel computes
    none: its partial last workgroup stops at its last 16-pixel group.  The channel pins that.)
    -> (x patterns [1, H, W, 16], w float32 [128, 9, 16], bias float32 [128], d [128], DROP_C)"""
    vals = np.array([(s << 15) | (Ef << 7) | m for Ef in MX_E for m in range(128) for s in (0, 1)], dtype=np.int64)
    H, W = grid_for(vals.size, 48)       # the first-layer kernel's fused copies need rows of a multiple of 16 pixels
    assert W % 16 == 0 and (H * W // 16) % 4 != 0 and H % 16 != 0        # its last workgroup (four 16-pixel groups) is partial
    x = np.zeros((H * W, 16), dtype=np.int64)
    x[:vals.size, 0] = vals
    x[:, 1] = 0x3f80
    d = np.zeros(128, dtype=np.int64)
    for blk in range(4):
        fol = [l for l in range(32) if l != LANES[blk]]
        for i, l in enumerate(fol):
            d[32 * blk + l] = 1 + i % 20
    drop_c = 32 * 3 + 5
    w = np.zeros((128, 9, 16), dtype=np.float32)
    w[np.arange(128), 4, 0] = np.ldexp(np.float32(1), -d).astype(np.float32)
    w[drop_c, 4, 0] = 0
    w[drop_c, 4, 1] = -np.ldexp(np.float32(1), DROP_B)
    bias = np.zeros(128, dtype=np.float32)
    bias[drop_c] = np.ldexp(np.float32(1), DROP_B)
    return x.reshape(1, H, W, 16), w, bias, d, drop_c


S2_E = (119, 127, 135)


def s2_dgrad_steering():
    """Stride-2 data gradient 256 -> 128 channels on the MXFP8 kernel, steered: adjoint channel 0 of pixel q holds the upper four
    significand bits of a table value, channel 1 the lower four, channel 2 a guard 2^(E + 1) with weight 0 that fixes the block's scale
    so that both parts are E4M3 values (the MX quantiser of the operand is then lossless).  Taps (1,1), (1,2), (2,1), (2,2) of the
    data-gradient pack carry 2^-d(ci) on adjoint channels 0 and 1: every input pixel receives exactly one adjoint pixel, so
    dx[p, ci] = value(q(p)) * 2^-d(ci) exactly.  -> (dy patterns [1, Ho, Wo, 256], wd float32 [128, 9, 256], d [128])"""
    vals = np.array([(s << 15) | (Ef << 7) | m for Ef in S2_E for m in range(128) for s in (0, 1)], dtype=np.int64)
    Ho, Wo = 25, 33
    assert vals.size <= Ho * Wo and (4 * Ho * Wo) % 64 != 0
    dy = np.zeros((Ho * Wo, 256), dtype=np.int64)
    hi = vals & 0xfff0
    E, lo4, sign = (vals >> 7) & 0xff, vals & 0xf, vals & 0x8000
    # lo4 * 2^(E - 127 - 7) as a bf16 pattern: normalise the four bits
    L = _bit_length(lo4)
    lo = np.where(lo4 > 0, sign | ((E - 8 + L) << 7) | (((lo4 << (8 - L)) & 0x7f)), 0)
    dy[:vals.size, 0], dy[:vals.size, 1], dy[:vals.size, 2] = hi, lo, (E + 1) << 7
    d = np.zeros(128, dtype=np.int64)
    for blk in range(4):
        fol = [l for l in range(32) if l != LANES[blk]]
        for i, l in enumerate(fol):
            d[32 * blk + l] = 1 + i % 20
    wd = np.zeros((128, 9, 256), dtype=np.float32)
    for tap in (4, 5, 7, 8):
        wd[:, tap, 0] = wd[:, tap, 1] = np.ldexp(np.float32(1), -d).astype(np.float32)
    return dy.reshape(1, Ho, Wo, 256), wd, d, vals


# ------------------------------------------------------------------------------------------------------- epilogue instances
# the flag combinations for which halo_epilogue (csrc/gg_common.h) compiles a straight-line epilogue; every other key is served by
# the general instance, whose flags are read at run time
STRAIGHT_LINE = {0, 1, 2, 5, 8, 24, 32, 64, 128, 192, 257, 264, 280, 288, 2305, 2312, 2328, 2336, 258, 261, 2306, 2309, 4353, 4354,
                 4357, 6402, 6405}


def epi_key(act=None, mask_bits=None, out_bits=None, r1=None, r2=None, accumulate=False, out_q=None, out_u=None, skip_y=False,
            mask=None, mask_last=False, **_):
    """key0 of halo_epilogue, plus its activation-mask bit (mask_c0 = 0 here)."""
    return ((1 if act is not None else 0) | (2 if mask_bits is not None else 0) | (4 if out_bits is not None else 0)
            | (8 if r1 is not None else 0) | (16 if r2 is not None else 0) | (64 if accumulate else 0) | (256 if out_q is not None else 0)
            | (2048 if out_u is not None else 0) | (4096 if skip_y else 0) | ((128 if mask_last else 32) if mask is not None else 0))
