"""Same-named counterparts of the metric / loss functions of the reference (DoWnGAN/GAN/losses.py) for the four that the
training loop uses (hyperparams.py:38-43 ``metrics_to_calculate``): NCHW tensors in, 0-dim fp32 tensor out (the reference's
caller does ``.detach().cpu().item()`` on every return, mlflow_epoch.py:58-61), all arithmetic in the HIP kernels (no torch
fallback; raises without the native library or a GPU).

  content_loss(hr, fake, device)      losses.py:40-55   nn.L1Loss()            -> dg_l1
  content_MSELoss(hr, fake, device)   losses.py:58-70   nn.MSELoss()           -> dg_sqdiff
  SSIM_Loss(x, y, device)             losses.py:12-38   MS-SSIM of the batch-min-max-normalised fields (pytorch_msssim,
                                                        win 7, data_range 1)   -> csrc/metrics.hip via msssim.MsSsim
  wass_loss(real, fake, device)       losses.py:8-9     real - fake
  divergence_loss / vorticity_loss    losses.py:119-193 std-normalised MSE of finite-difference fields -> dg_div_vort_sums
  eof_loss(X, hr, fake, device)       losses.py:72-116  std-normalised MSE of the (uncentred) projections on EOFs X [K, C, P]
                                                        -> dg_eof_project; returns a Python float like the reference
  low_pass_eof_batch(Z, pcas, fine, transformer, device, fake=False)
                                      losses.py:196-228 sum_k Z[b, c, k] pcas[k, c] for c = 0, 1 (no mean added back); with
                                                        fake, Z = the transformers' centred projections of `fine`
                                                        -> dg_eof_project, dg_eof_reconstruct

Unlike the reference's SSIM_Loss this one does NOT normalise its arguments in place (the reference's mutation is a side
effect that nothing downstream reads: the metrics pass is the last use of the batch, wasserstein.py:138-146).
"""
from __future__ import annotations

import torch

from .. import layout
from ..msssim import MsSsim
from .. import backend

_ops = {}
_ms = {}


def _o(device=None):
    key = str(device or "cuda:0")
    if key not in _ops:
        _ops[key] = backend.make_ops("f32", key if key.startswith("cuda") else "cuda:0")
    return _ops[key]


def _native(o, t):
    N, C, H, W = t.shape
    out = o.zeros(N, H, W, layout.pad16(C))
    o.nchw_to_nhwc(t.to(o.device, torch.float32).contiguous(), out)
    return out


def _scalar(o, v):
    """0-dim fp32 tensor on the compute device, like the reference's loss modules return."""
    return torch.tensor(float(v), dtype=torch.float32, device=o.device)


def wass_loss(real, fake, device=None):
    return real - fake


def content_loss(hr, fake, device=None):
    o = _o(device)
    acc = o.zeros(1, dtype=torch.float32)
    o.l1(_native(o, hr), _native(o, fake), acc)
    return _scalar(o, float(acc.item()) / hr.numel())


def content_MSELoss(hr, fake, device=None):
    o = _o(device)
    acc = o.zeros(1, dtype=torch.float32)
    o.sqdiff(_native(o, hr), _native(o, fake), acc)
    return _scalar(o, float(acc.item()) / hr.numel())


def SSIM_Loss(x, y, device=None, reduction="mean", window_size=11):
    """``reduction`` / ``window_size`` are accepted and ignored exactly like in the reference (it hard-codes win_size=7)."""
    o = _o(device)
    N, C, H, W = x.shape
    key = (str(o.device), N, C, H, W)
    if key not in _ms:
        _ms[key] = MsSsim(o, N, H, W, c_real=C)
    return _scalar(o, _ms[key](_native(o, x), _native(o, y)))


def _std_normalised_mse(m, n):
    """MSE(r / std(r), f / std(f)) from {sum r, sum r^2, sum f, sum f^2, sum r f} (float64), torch.std = unbiased."""
    sr, srr, sf, sff, srf = m
    var_r = (srr - sr * sr / n) / (n - 1)
    var_f = (sff - sf * sf / n) / (n - 1)
    return (srr / var_r - 2.0 * srf / (var_r * var_f) ** 0.5 + sff / var_f) / n


def _div_vort(hr, fake, device):
    o = _o(device)
    sums = torch.zeros(10, dtype=torch.float64, device=o.device)
    o.div_vort_sums(_native(o, hr), _native(o, fake), sums)
    N, _, H, W = hr.shape
    return sums.cpu().tolist(), N * (H - 1) * (W - 1)


def divergence_loss(hr, fake, device=None):
    """losses.py:119-156 (u = channel 0 differenced along H, v = channel 1 along W)."""
    m, n = _div_vort(hr, fake, device)
    return _scalar(_o(device), _std_normalised_mse(m[:5], n))


def vorticity_loss(hr, fake, device=None):
    """losses.py:158-193."""
    m, n = _div_vort(hr, fake, device)
    return _scalar(_o(device), _std_normalised_mse(m[5:], n))


def _eof_project(o, y, E, K, ld_k, ld_c, m=None):
    """Z [B, C, K] fp32 = (y - m) . E over the pixels of the NCHW batch y (one launch pair, csrc/eof.hip)."""
    y = y.detach().to(o.device, torch.float32).contiguous()
    Z = torch.empty(y.shape[0], y.shape[1], K, dtype=torch.float32, device=o.device)
    o.eof_project(o.eof_fields(y), m, E, K, ld_k, ld_c, Z)
    return Z


def eof_loss(X, hr, fake, device=None):
    """losses.py:72-116.  X [K, C, P]: hr, fake [B, C, H, W] are projected (uncentred) on X[k, c]; each of the two projection sets
    [B, K, C] is divided by its own unbiased std over all its values; the MSE of the two is returned as a float (``.item()``)."""
    o = _o(device)
    K, Cx, P = X.shape
    B, Cn, H, W = hr.shape
    assert Cx == Cn and P == H * W and tuple(fake.shape) == tuple(hr.shape), (tuple(X.shape), tuple(hr.shape), tuple(fake.shape))
    E = torch.as_tensor(X).detach().to(o.device, torch.float32).contiguous()
    zr = _eof_project(o, hr, E, K, Cn * P, P).double().cpu()
    zf = _eof_project(o, fake, E, K, Cn * P, P).double().cpu()
    return float(((zf / zf.std() - zr / zr.std()) ** 2).mean())


_staged_pca = {}


def _pca_arrays(o, t):
    """(mean_ [P], components_ [K, P]) of a transformer as fp32 device tensors: a native channel view's own, or a foreign object's
    (a fitted sklearn PCA, say) staged once and cached."""
    if torch.is_tensor(t.components_) and t.components_.device == o.device and t.components_.dtype == torch.float32 \
            and t.components_.is_contiguous() and t.mean_.is_contiguous():
        return t.mean_, t.components_
    key = (id(t), id(t.mean_), id(t.components_), str(o.device))
    if key not in _staged_pca:
        m = torch.as_tensor(t.mean_).to(o.device, torch.float32).contiguous()
        e = torch.as_tensor(t.components_).to(o.device, torch.float32).contiguous()
        _staged_pca[key] = (t, m, e)
    return _staged_pca[key][1], _staged_pca[key][2]


def low_pass_eof_batch(Z, pcas, fine, transformer, device=None, fake=False):
    """losses.py:196-228.  pcas [K, C, P], Z [B, C, K] (channels 0 and 1 used) -> lows [B, 2, H, W] with
    lows[b, c] = sum_k Z[b, c, k] pcas[k, c] (no mean added back).  With ``fake`` Z is recomputed from ``fine`` through
    ``transformer[0]`` / ``transformer[1]`` (centred projections, like sklearn's ``transform``)."""
    o = _o(device)
    B, H, W = fine.size(0), fine.size(2), fine.size(3)
    P = H * W
    E = torch.as_tensor(pcas).detach().to(o.device, torch.float32).contiguous()
    K, Cp = E.shape[0], E.shape[1]
    assert E.shape[2] == P and Cp >= 2, (tuple(E.shape), P)
    if fake:
        y = fine.detach().to(o.device, torch.float32).contiguous()
        parts = []
        for c in range(2):
            m, comps = _pca_arrays(o, transformer[c])
            Zc = torch.empty(B, 1, comps.shape[0], dtype=torch.float32, device=o.device)
            o.eof_project(o.eof_fields(y[:, c:c + 1]), m, comps, comps.shape[0], P, 0, Zc)
            parts.append(Zc)
        Z = torch.cat(parts, dim=1)
    else:
        Z = torch.as_tensor(Z)[:, :2].to(o.device, torch.float32).contiguous()
    assert Z.shape[2] == K, (tuple(Z.shape), K)
    lows = torch.empty(B, 2, H, W, dtype=torch.float32, device=o.device)
    o.eof_reconstruct(Z, E, Cp * P, P, P, None, lows)
    return lows


metrics_to_calculate = {"MAE": content_loss, "MSE": content_MSELoss, "MSSSIM": SSIM_Loss, "Wass": wass_loss}   # hyperparams.py:38-43
