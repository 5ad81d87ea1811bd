"""EOF analysis on the MI355X (csrc/eof.hip): kernels against float64 numpy on ragged shapes in every input layout, the fit
against sklearn and the reference (tests/golden/eof.json), determinism, and a full-size fit from the resident feed.
These are tolerance tests of real-valued data; every kernel, channel count, component width, slice length and layout is pinned bit
for bit on integer data by tests/test_eof_exact_gpu.py (case table and float64 references: tests/eof_ref.py)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from downgan_amd import eof as eof_mod
from downgan_amd.GAN import losses
from downgan_amd.GAN.dataloader import NetCDFSR, ResidentLoader
from downgan_amd.ops import HipOps
from tests import eof_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eof.json")


@pytest.fixture(scope="module")
def ops():
    return HipOps("f32", DEV)


def _layouts(x32):
    """(name, fields descriptor source, the fp64 values it holds [T, C, H, W]) for NCHW fp32, NHWC fp32 and NHWC bf16."""
    nchw = x32.to(DEV).contiguous()
    nhwc = x32.permute(0, 2, 3, 1).contiguous().to(DEV)
    nhwc_b = nhwc.to(torch.bfloat16)
    return [("nchw_f32", nchw, False, x32.double()),
            ("nhwc_f32", nhwc, True, x32.double()),
            ("nhwc_bf16", nhwc_b, True, nhwc_b.float().permute(0, 3, 1, 2).cpu().double())]


def _cos_check(E, ref):
    """sign-exact, 1 - cos <= 1e-5 per component (rows of E [K, P] against ref [K, P], float64)."""
    E, ref = np.asarray(E, np.float64), np.asarray(ref, np.float64)
    cos = np.sum(E * ref, 1) / (np.linalg.norm(E, axis=1) * np.linalg.norm(ref, axis=1))
    assert np.all(cos > 0), cos                      # no flipped component
    assert np.max(1 - cos) <= 1e-5, 1 - cos


def test_kernels_against_float64_numpy_ragged(ops):
    T, Cn, H, W, K, B = 77, 2, 60, 76, 13, 5
    P = H * W
    x32 = eof_fixture.fields(0, T, Cn, H, W).float()
    y32 = eof_fixture.fields(500, B, Cn, H, W).float()
    for name, src, nhwc, x in _layouts(x32):
        f = ops.eof_fields(src, nhwc=nhwc)
        X = x.reshape(T, Cn, P).numpy()
        mu_ref = X.mean(0)
        mu = torch.empty(Cn, P, dtype=torch.float32, device=DEV)
        ops.eof_mean(f, mu)
        np.testing.assert_allclose(mu.cpu().numpy(), mu_ref, rtol=0, atol=1e-6 * np.abs(mu_ref).max(), err_msg=name)
        G = torch.empty(Cn, T, T, dtype=torch.float64, device=DEV)
        ops.eof_gram(f, mu, G)
        Xc = X - mu.cpu().double().numpy()[None]
        for c in range(Cn):
            Gr = Xc[:, c] @ Xc[:, c].T
            err = np.linalg.norm(G[c].cpu().numpy() - Gr) / np.linalg.norm(Gr)
            assert err <= 1e-6, (name, c, err)
        e = eof_mod.EOF(K, ops=ops).fit(x32 if name == "nchw_f32" else _loader_of(src))
        for c in range(Cn):
            Vt, var, ratio = _sk(X[:, c], K)
            _cos_check(e.components_[c].cpu().numpy(), Vt)
            np.testing.assert_allclose(e.explained_variance_[c].cpu().numpy(), var, rtol=1e-5, err_msg=name)
            np.testing.assert_allclose(e.explained_variance_ratio_[c].cpu().numpy(), ratio, rtol=1e-5, err_msg=name)
        # transform / inverse_transform against float64 numpy with the fitted arrays
        Y = y32.double().reshape(B, Cn, P).numpy()
        Ed = e.components_.cpu().double().numpy()
        md = e.mean_.cpu().double().numpy()
        Z = e.transform(y32.to(DEV))
        Zr = np.einsum("bcp,ckp->bck", Y - md[None], Ed)
        np.testing.assert_allclose(Z.cpu().numpy(), Zr, rtol=0, atol=1e-5 * np.abs(Zr).max(), err_msg=name)
        R = e.inverse_transform(Z)
        Rr = np.einsum("bck,ckp->bcp", Z.cpu().double().numpy(), Ed) + md[None]
        np.testing.assert_allclose(R.reshape(B, Cn, P).cpu().numpy(), Rr, rtol=0, atol=1e-5 * np.abs(Rr).max(), err_msg=name)


def _sk(Xc_t, K):
    """sklearn PCA(svd_solver="full") in float64 numpy: (components with svd_flip(u_based_decision=False), variance, ratio)."""
    Xc = Xc_t - Xc_t.mean(0)
    _, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    i = np.argmax(np.abs(Vt), axis=1)
    Vt = Vt * np.sign(Vt[np.arange(Vt.shape[0]), i])[:, None]
    return Vt[:K], (S ** 2 / (Xc.shape[0] - 1))[:K], (S ** 2 / np.sum(S ** 2))[:K]


def _loader_of(store):
    """A ResidentLoader around an existing [n, H, W, c] store (the fit reads ``store_f`` in place)."""
    n, H, W, c = store.shape
    dt = "bf16" if store.dtype == torch.bfloat16 else "f32"
    coarse = torch.zeros(n, H // 8 or 1, W // 8 or 1, c, dtype=store.dtype, device=store.device)
    return ResidentLoader(None, 1, dtype=dt, device=DEV, _stores=(coarse, store))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden_fit(golden, ops):
    g = golden
    x = eof_fixture.fields(0, g["T"] + g["held"], g["C"], g["H"], g["W"]).float()
    return eof_mod.EOF(g["K"], ops=ops).fit(x[:g["T"]]), x[g["T"]:]


def test_fit_against_sklearn_golden(golden, golden_fit):
    g, (e, held) = golden, golden_fit
    ks, ps = np.array(g["sample_k"]), np.array(g["sample_p"])
    for c in range(g["C"]):
        E = e.components_[c].cpu().double().numpy()
        got = E[ks, ps]
        ref = np.array(g[f"comp{c}"])
        np.testing.assert_array_equal(np.sign(got[np.abs(ref) > 1e-4]), np.sign(ref[np.abs(ref) > 1e-4]))
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5 * np.abs(E).max())
        np.testing.assert_allclose(e.explained_variance_[c].cpu().numpy(), g[f"var{c}"], rtol=1e-5)
        np.testing.assert_allclose(e.explained_variance_ratio_[c].cpu().numpy(), g[f"ratio{c}"], rtol=1e-5)
        ch = e.channel(c)
        Z = ch.transform(held[:, c].reshape(g["held"], -1))
        ref = np.array(g[f"transform{c}"])
        np.testing.assert_allclose(Z.cpu().numpy(), ref, rtol=0, atol=1e-5 * np.abs(ref).max())
    Z = e.transform(held)
    for c in range(g["C"]):
        np.testing.assert_allclose(Z[:, c].cpu().numpy(), g[f"transform{c}"], rtol=0, atol=1e-5 * np.abs(g[f"transform{c}"]).max())


def test_eof_loss_and_low_pass_against_the_reference(golden, golden_fit):
    g, (e, held) = golden, golden_fit
    X = e.components_.permute(1, 0, 2).contiguous()          # [K, C, P], what the reference's callers hold
    hr, fake = held[:4], held[4:]
    got = losses.eof_loss(X, hr.to(DEV), fake.to(DEV), DEV)
    assert isinstance(got, float)
    assert abs(got - g["eof_loss"]) <= 1e-5 * abs(g["eof_loss"]), (got, g["eof_loss"])
    idx = np.array(g["lows_index"])
    tr = (e.channel(0), e.channel(1))
    Z = torch.stack([tr[c].transform(hr[:, c].reshape(4, -1)) for c in range(2)], dim=1)
    lows = losses.low_pass_eof_batch(Z, X, hr.to(DEV), tr, DEV)
    assert tuple(lows.shape) == tuple(g["lows_shape"])
    np.testing.assert_allclose(lows.reshape(-1)[idx].cpu().numpy(), g["lows"], rtol=0, atol=1e-5 * g["lows_absmax"])
    lows_f = losses.low_pass_eof_batch(None, X, fake.to(DEV), tr, DEV, fake=True)
    np.testing.assert_allclose(lows_f.reshape(-1)[idx].cpu().numpy(), g["lows_fake"], rtol=0, atol=1e-5 * g["lows_fake_absmax"])
    # foreign transformers (sklearn-style objects holding float64 numpy arrays) are staged once and give the same answer
    foreign = tuple(types.SimpleNamespace(mean_=t.mean_.cpu().double().numpy(), components_=t.components_.cpu().double().numpy())
                    for t in tr)
    lows_s = losses.low_pass_eof_batch(None, X.cpu(), fake, foreign, DEV, fake=True)
    np.testing.assert_allclose(lows_s.reshape(-1)[idx].cpu().numpy(), g["lows_fake"], rtol=0, atol=1e-5 * g["lows_fake_absmax"])
    assert len([k for k in losses._staged_pca if k[0] in (id(foreign[0]), id(foreign[1]))]) == 2
    losses.low_pass_eof_batch(None, X, fake, foreign, DEV, fake=True)
    assert len([k for k in losses._staged_pca if k[0] in (id(foreign[0]), id(foreign[1]))]) == 2


def test_fit_and_projection_are_bit_identical(ops):
    x = eof_fixture.fields(0, 77, 2, 60, 76).float()
    a = eof_mod.EOF(13, ops=ops).fit(x)
    b = eof_mod.EOF(13, ops=ops).fit(x)
    assert torch.equal(a.mean_, b.mean_) and torch.equal(a.components_, b.components_)
    assert torch.equal(a.explained_variance_, b.explained_variance_)
    y = eof_fixture.fields(300, 9, 2, 60, 76).float().to(DEV)
    assert torch.equal(a.transform(y), a.transform(y))
    f = ops.eof_fields(x.to(DEV))
    mu = torch.empty(2, 60 * 76, dtype=torch.float32, device=DEV)
    ops.eof_mean(f, mu)
    G1 = torch.empty(2, 77, 77, dtype=torch.float64, device=DEV)
    G2 = torch.empty_like(G1)
    ops.eof_gram(f, mu, G1)
    ops.eof_gram(f, mu, G2)
    assert torch.equal(G1, G2)


def test_full_size_fit_from_the_resident_feed(ops):
    T, Cn, H, W, K = 1024, 2, 1024, 1024, 20
    P = H * W
    store = torch.empty(T, H, W, Cn, dtype=torch.bfloat16, device=DEV)
    for a in range(0, T, 32):
        store[a:a + 32] = eof_fixture.fields(a, min(32, T - a), Cn, H, W, device=DEV).permute(0, 2, 3, 1).to(torch.bfloat16)
    loader = _loader_of(store)
    e = eof_mod.EOF(K, ops=ops).fit(loader)
    E = e.components_
    for c in range(Cn):
        I = (E[c].double() @ E[c].double().T).cpu().numpy()
        np.testing.assert_allclose(I, np.eye(K), rtol=0, atol=1e-4)
    # the fit data's projection: zero mean, per-component variance = explained_variance_
    Zs = []
    for a in range(0, T, 64):
        Zs.append(e.transform(store[a:a + 64].permute(0, 3, 1, 2).float()).double())
    Z = torch.cat(Zs).cpu().numpy()                           # [T, C, K]
    var = e.explained_variance_.cpu().double().numpy()
    assert np.max(np.abs(Z.mean(0)) / np.sqrt(var)) <= 1e-4
    np.testing.assert_allclose(Z.var(0, ddof=1), var, rtol=1e-4)
    # the same values as an fp32 NCHW fit
    x32 = store.permute(0, 3, 1, 2).float().contiguous()
    del loader
    f = eof_mod.EOF(K, ops=ops).fit(x32)
    del x32
    np.testing.assert_allclose(f.explained_variance_.cpu().numpy(), e.explained_variance_.cpu().numpy(), rtol=1e-5)
    for c in range(Cn):
        d = (f.components_[c] - e.components_[c]).abs().max().item()
        assert d <= 1e-5 * e.components_[c].abs().max().item(), (c, d)
