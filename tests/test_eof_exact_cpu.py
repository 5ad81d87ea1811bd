"""Tests of the exact EOF tests themselves (tests/eof_ref.py; there is no CPU emulation of csrc/eof.hip): every case's integer
budget holds, every float64 reference equals a second statement in explicit loops, the table reaches every branch it names, and
for each fault the table exists to catch the case's OWN data would show it: the faulty result differs from the reference in at
least one bit (a case whose data cannot show its fault is a defect of the table)."""
import numpy as np
import pytest

from downgan_amd import eof as eof_mod
from tests import eof_ref as R
from tests.conv_ref import SENTINEL
from tests.elementwise_ref import INT_LIMIT


def _bits_differ(a, b, what, dtype=np.float64):
    """Number of elements whose bit patterns differ (> 0 asserted, and printed: the mutation reports that it changes expected bits)."""
    a, b = np.ascontiguousarray(a, dtype=dtype), np.ascontiguousarray(b, dtype=dtype)
    assert a.shape == b.shape
    view = {4: np.uint32, 8: np.uint64}[a.itemsize]
    n = int((a.view(view) != b.view(view)).sum())
    print(f"[mutation] {what}: {n} of {a.size} expected elements change")
    assert n > 0, f"{what}: the case's data cannot show the fault"
    return n


@pytest.mark.parametrize("cid", [c.id for c in R.CASES])
def test_budget(cid):
    assert R.budget(R.BY_ID[cid]) < INT_LIMIT


def test_fp32_cases_use_the_budget():
    """The one-slice Gram cases take the largest deviations their budget leaves (the bound of their chains stands within 5 % of
    2^24); the one-sign case's slabs stay below 2^24 while its diagonal total lies above."""
    for cid in (f"gram-T77-C2-P{R.P0}-ns1", "gram-T33-C8-P1517-ns1"):
        assert R.budget(R.BY_ID[cid]) > 0.95 * INT_LIMIT, cid
    case = R.ONE_SIGN
    inp = R.inputs(case)
    (_, mu), = inp["mus"]
    x, sl = inp["x"], R.slice_len(case.P, case.nslice)
    d = (x - mu[None]).astype(np.float64)
    assert (d > 0).all()
    for s in range(case.nslice):
        slab = np.einsum("icp,jcp->cij", d[..., s * sl:(s + 1) * sl], d[..., s * sl:(s + 1) * sl])
        assert 0.5 * INT_LIMIT < slab.max() < INT_LIMIT
    assert np.diagonal(R.ref_gram(x, mu), axis1=1, axis2=2).min() > INT_LIMIT


def test_table_reaches_every_branch():
    tags = {}
    for c in R.CASES:
        for t in R.covers(c):
            tags.setdefault(t, []).append(c.id)
    gram = set().union(*(R.covers(c) for c in R.CASES if c.kind == "gram"))
    need_gram = {f"NC={n}" for n in range(1, 9)} | {"chain=two-level", "chain=one-level", "lane-guard", "fold", "folds=3",
                                                      "ragged-chunk-in-long-slice", "empty-slice", "64-pixel-slices", "row-tiles=1",
                                                      "row-tiles=2", "row-tiles=3", "one-sign", "NaN-padding-channels",
                                                      "fmt=nchw_f32", "fmt=nhwc_f32", "fmt=nhwc_bf16_pad"}
    assert need_gram <= gram, need_gram - gram
    proj = set().union(*(R.covers(c) for c in R.CASES if c.kind == "project"))
    need_proj = {"row-tiles=1", "row-tiles=2", "E=ckp", "E=kcp", "E=shared", "m=given", "m=None", "mixed-dtype", "chain=one-level",
                 "fold", "ragged-chunk-in-long-slice", "64-pixel-slices"} | {f"K={k}" for k in (1, 13, 16, 17, 33, 64)}
    assert need_proj <= proj, need_proj - proj
    need = {f"{k}-KB={kb}" for k in ("components", "reconstruct") for kb in (16, 32, 48, 64)}
    need |= {"NaN-padding-columns", "mu=given", "mu=None"} | {f"sign-row={name}" for name, _, _ in R.SIGN_ROWS}
    need |= {f"fmt={f}" for f in R.FORMATS}
    assert need <= set(tags), need - set(tags)
    # the rotating attributes of the projection meet every channel count and every batch size
    for attr, values in (("layout", R.E_LAYOUTS), ("centred", (True, False)), ("nslice", R.P_NSLICE), ("fmt", R.P_FMTS)):
        for key in ("C", "T", "K"):
            seen = {(getattr(c, key), getattr(c, attr)) for c in R.CASES if c.kind == "project"}
            keys = {getattr(c, key) for c in R.CASES if c.kind == "project"}
            assert seen == {(k, v) for k in keys for v in values}, (attr, key)
    rec = [c for c in R.CASES if c.kind == "reconstruct"]
    for attr, values in (("layout", ("ckp", "kcp")), ("centred", (True, False)), ("T", (1, 5))):
        for key in ("C", "K", "P"):
            assert {(getattr(c, key), getattr(c, attr)) for c in rec} == {(k, v) for k in {getattr(c, key) for c in rec} for v in values}
    comp = [c for c in R.CASES if c.kind == "components"]
    assert {c.fmt for c in comp} == set(R.FORMATS) and {c.fmt for c in R.CASES if c.kind == "mean"} == set(R.FORMATS)


# ---------------------------------------------------------------------------------------- references against explicit loops
def test_references_equal_explicit_loops():
    g = R.BY_ID[R.FIRST[0]]
    inp = R.inputs(g)
    x = inp["x"]
    for _, mu in inp["mus"]:
        G = np.zeros((g.C, g.T, g.T))
        for c in range(g.C):
            for i in range(g.T):
                for j in range(g.T):
                    G[c, i, j] = float(sum(int(x[i, c, p] - mu[c, p]) * int(x[j, c, p] - mu[c, p]) for p in range(g.P)))
        assert np.array_equal(R.ref_gram(x, mu), G)
    m = R.inputs(R.BY_ID["mean-T5-C1-nchw_f32"])["x"][:, :, :40]
    want = np.array([[np.float32(float(sum(int(v) for v in m[:, c, p])) / 5.0) for p in range(40)] for c in range(1)], dtype=np.float32)
    assert np.array_equal(R.ref_mean(m).view(np.uint32), want.view(np.uint32))
    rng = np.random.default_rng(3)
    B, Cn, K, P, T = 3, 2, 3, 23, 5
    y, mu, E = rng.integers(-200, 201, (B, Cn, P)), rng.integers(-64, 65, (Cn, P)), rng.integers(-31, 32, (Cn, K, P))
    for m_ in (mu, None):
        Z = np.array([[[float(sum(int(y[b, c, p] - (0 if m_ is None else m_[c, p])) * int(E[c, k, p]) for p in range(P)))
                        for k in range(K)] for c in range(Cn)] for b in range(B)])
        assert np.array_equal(R.ref_project(y, m_, E), Z)
    Zi = rng.integers(-900, 901, (B, Cn, K))
    for m_ in (mu, None):
        out = np.array([[[float(sum(int(Zi[b, c, k]) * int(E[c, k, p]) for k in range(K)) + (0 if m_ is None else int(m_[c, p])))
                          for p in range(P)] for c in range(Cn)] for b in range(B)])
        assert np.array_equal(R.ref_reconstruct(Zi, E, m_), out)
    x, A = mu[None] + rng.integers(-5, 6, (T, Cn, P)), rng.integers(-3, 4, (Cn, T, K))     # small values: ties do occur
    Er, words = R.ref_components(x, mu, A)
    ties = 0
    for c in range(Cn):
        for k in range(K):
            row = [sum(int(A[c, t, k]) * int(x[t, c, p] - mu[c, p]) for t in range(T)) for p in range(P)]
            best = 0
            for p in range(P):
                if abs(row[p]) > abs(row[best]):
                    best = p
            ties += sum(abs(v) == abs(row[best]) for v in row) > 1
            neg = row[best] < 0
            assert words[c, k] == R.amax_word(row[best], best)
            want = np.array([-float(v) if neg else float(v) for v in row], dtype=np.float32)
            assert np.array_equal(Er[c, k].view(np.uint32), want.view(np.uint32)), (c, k)
    assert ties > 0
    assert R.amax_word(0.0, 0) == 0xffffffff and R.amax_word(-1.0, 2) == (0x3f800000 << 32 | 0xfffffffd) - (1 << 63)


def test_sign_rule_rows_and_the_host_statement():
    """The constructed rows give the flips and positions they were built for; eof.sign_rule (the host statement of dg_eof_flip)
    agrees with the reference on the same rows."""
    for case in R.SIGNRULE:
        inp = R.inputs(case)
        E, words = R.ref_components(inp["x"], inp["mu"], inp["A"])
        flip, pos = R.signrule_expected(case)
        raw = np.einsum("ctk,tcp->ckp", inp["A"], inp["x"] - inp["mu"][None]).astype(np.float64)
        for c in range(2):
            assert np.array_equal(eof_mod.sign_rule(raw[c]), E[c].astype(np.float64)), c
            for k, (name, plants, _) in enumerate(R.SIGN_ROWS):
                assert (words[c, k] < 0) == flip[c, k], (c, name)
                assert 0xffffffff - (int(words[c, k]) & 0xffffffff) == pos[c, k], (c, name)
                if plants:
                    assert E[c, k, pos[c, k]] == R.SIGN_MAX and np.abs(E[c, k]).max() == R.SIGN_MAX
                    assert (np.abs(raw[c, k]) == R.SIGN_MAX).sum() == len(plants)
                else:
                    assert not E[c, k].any() and words[c, k] == 0xffffffff


# ---------------------------------------------------------------------------------------------------------- mutation checks
def _gram_without(case, drop):
    """The Gram a kernel would return that loses the pixels ``drop`` (bool [P])."""
    inp = R.inputs(case)
    name, mu = inp["mus"][0]
    keep = ~drop
    return R.ref_gram(inp["x"], mu), R.ref_gram(inp["x"][..., keep], mu[..., keep])


def test_mutation_dropping_the_last_pixel():
    for cid in (R.FIRST[0], f"gram-T77-C2-P{R.P0}-ns1", f"gram-T77-C2-P{R.P0}-ns24", "gram-T33-C7-P1517-ns1"):
        case = R.BY_ID[cid]
        drop = np.arange(case.P) == case.P - 1
        _bits_differ(*_gram_without(case, drop), f"{cid}: the last pixel dropped")
    case = next(c for c in R.CASES if c.kind == "project" and c.nslice == 1 and c.T == 70)
    inp = R.inputs(case)
    y = inp["y"].copy()
    y[..., -1] = 0 if inp["m"] is None else inp["m"][..., -1]
    _bits_differ(R.ref_project(inp["y"], inp["m"], inp["E"]), R.ref_project(y, inp["m"], inp["E"]), f"{case.id}: the last pixel dropped")


def test_mutation_dropping_a_fold_boundary():
    """The chunk that ends at the 512th pixel of a slice (where tot += acc fires) is lost."""
    case = R.BY_ID[f"gram-T77-C2-P{R.P0}-ns1"]
    assert "folds=3" in R.covers(case)
    kp = R.kp_of(case.C)
    for edge in (512, 1024):
        drop = (np.arange(case.P) >= edge - kp) & (np.arange(case.P) < edge)
        _bits_differ(*_gram_without(case, drop), f"{case.id}: the chunk before pixel {edge} dropped")
    drop = np.arange(case.P) >= 1536 - kp                      # the ragged last chunk, which ends at the third fold
    assert 0 < drop.sum() < kp
    _bits_differ(*_gram_without(case, drop), f"{case.id}: the ragged last chunk dropped")


def test_mutation_shifting_a_slice_boundary():
    for cid in (f"gram-T77-C2-P{R.P0}-ns5", f"gram-T77-C2-P{R.P0}-ns7", "gram-T33-C5-P1517-ns3"):
        case = R.BY_ID[cid]
        sl = R.slice_len(case.P, case.nslice)
        drop = (np.arange(case.P) >= sl) & (np.arange(case.P) < sl + 64)       # slice 1 begins 64 pixels late
        _bits_differ(*_gram_without(case, drop), f"{cid}: a slice boundary shifted by 64")


def test_mutation_skipping_the_mirror():
    for T in (65, 130):
        case = R.BY_ID[f"gram-T{T}-C2-P{R.P0}-ns3"]
        inp = R.inputs(case)
        G = R.ref_gram(inp["x"], inp["mus"][0][1])
        assert np.array_equal(G, G.transpose(0, 2, 1))
        bad = G.copy()
        bad[:, np.tril_indices(T, -1)[0], np.tril_indices(T, -1)[1]] = SENTINEL      # what the destination held before
        _bits_differ(G, bad, f"{case.id}: the lower triangle not written")
        # a tile mirrored WITHOUT being transposed shows as well: the off-diagonal tile is not symmetric in itself
        if T >= 128:
            tile = G[:, :64, 64:128]
            _bits_differ(tile, tile.transpose(0, 2, 1), f"{case.id}: the off-diagonal tile mirrored untransposed")


def test_mutation_breaking_ties_to_the_highest_index():
    for case in R.SIGNRULE:
        inp = R.inputs(case)
        E, words = R.ref_components(inp["x"], inp["mu"], inp["A"])
        Eb, wb = R.ref_components(inp["x"], inp["mu"], inp["A"], tie_highest=True)
        tied = [k for k, (_, plants, _) in enumerate(R.SIGN_ROWS) if len(plants) == 2]
        for c in range(2):
            for k in tied:
                assert words[c, k] != wb[c, k]
                _bits_differ(E[c, k], Eb[c, k], f"{case.id} channel {c} row {R.SIGN_ROWS[k][0]}: tie to the highest index", np.float32)


def test_mutation_reading_a_padding_channel():
    for cid in ("gram-T33-C3-P1517-ns3-nhwc_bf16_pad", "signrule-nhwc_bf16_pad"):
        case = R.BY_ID[cid]
        inp = R.inputs(case)
        store = R.host_store(inp["x"], case.fmt)
        good, bad = R.seen(store, case.fmt, case.C), R.seen(store, case.fmt, case.C, c0=1)
        assert np.array_equal(good, inp["x"].astype(np.float64)) and np.isnan(bad[:, -1]).all()
        mu = inp["mus"][0][1] if case.kind == "gram" else inp["mu"]
        _bits_differ(R.ref_gram(good, mu), R.ref_gram(bad, mu), f"{cid}: one padding channel read")


def test_mutation_exchanging_ld_k_and_ld_c():
    cases = [c for c in R.CASES if c.kind in ("project", "reconstruct") and c.layout in ("kcp", "ckp") and c.C > 1 and c.K > 1]
    assert {c.layout for c in cases} == {"kcp", "ckp"} and {c.kind for c in cases} == {"project", "reconstruct"}
    for case in cases[::7]:
        inp = R.inputs(case)
        store, ld_k, ld_c = R.e_store(inp["E"], case.layout)
        good, bad = R.e_read(store, case.K, case.C, case.P, ld_k, ld_c), R.e_read(store, case.K, case.C, case.P, ld_c, ld_k)
        assert np.array_equal(good, inp["E"].astype(np.float64))
        if case.kind == "project":
            _bits_differ(R.ref_project(inp["y"], inp["m"], good), R.ref_project(inp["y"], inp["m"], bad), f"{case.id}: ld_k / ld_c exchanged")
        else:
            _bits_differ(R.ref_reconstruct(inp["Z"], good, inp["mu"]), R.ref_reconstruct(inp["Z"], bad, inp["mu"]),
                         f"{case.id}: ld_k / ld_c exchanged")


def test_nan_padding_columns_and_channels_are_in_the_inputs():
    """The NaN a kernel must not read is really there: a reference that takes a padding column of A, or channel C of the padded
    store, is NaN throughout."""
    case = R.BY_ID["components-T5-K17-C2-" + next(c.fmt for c in R.CASES if c.id.startswith("components-T5-K17-C2-"))]
    inp = R.inputs(case)
    A = np.concatenate([inp["A"].astype(np.float64), np.full((case.C, case.T, 32 - case.K), np.nan)], axis=2)
    E, _ = R.ref_components(inp["x"], inp["mu"], A[..., :case.K])
    raw = np.einsum("ctk,tcp->ckp", A[..., 1:case.K + 1], (inp["x"] - inp["mu"][None]).astype(np.float64))
    assert np.isnan(raw[:, -1]).all() and not np.isnan(E).any()
