"""EOF analysis: one PCA per channel of a time series of fields, fitted and applied on the GPU (csrc/eof.hip).

The reference fits sklearn ``PCA`` on the host, one per variable (DoWnGAN/helpers/prep_gan.py:226-255, and the
``(transformer_u, transformer_v)`` pair of DoWnGAN/GAN/losses.py:196-199).  ``EOF`` does the same fit without copying the fields
to the host:

  dg_eof_mean        mu[c, p]                                   fp64 accumulation
  dg_eof_gram        G_c = Xc Xc^T, Xc the centred fields       f32 MFMA, split over the pixels, fixed-order fp64 slice sum
  host               eigh of each fp64 G_c (T x T, T <= 8192), top K eigenpairs, A = V^T / sqrt(lambda)
  dg_eof_components  E_c = A Xc, then sklearn's sign rule        (svd_flip(u_based_decision=False): the entry of largest magnitude
                                                                  of every component is positive)

With X = U S V^T the SVD of the centred data, G = U S^2 U^T, so the rows of E are sklearn's ``components_`` (V^T, unit norm),
``explained_variance_`` is lambda / (T - 1) and ``explained_variance_ratio_`` lambda / trace(G).  Every reduction runs in a fixed
order: two fits of the same data are bit-identical.
"""
from __future__ import annotations

import numpy as np
import torch

from . import backend

T_MAX = 8192          # the host eigensolver works on a dense T x T matrix
K_MAX = 64
C_MAX = 8


def check_limits(T, C, K):
    """ValueError naming the limit an (T snapshots, C channels, K components) fit breaks."""
    if not 2 <= T <= T_MAX:
        raise ValueError(f"EOF fit needs 2 <= T <= {T_MAX} snapshots (got T = {T}): the host eigensolver bounds T")
    if C < 1 or C > C_MAX:
        raise ValueError(f"EOF fit takes 1 <= C <= {C_MAX} channels (got C = {C})")
    if not 1 <= K <= min(K_MAX, T - 1):
        raise ValueError(f"EOF fit needs 1 <= n_components <= min({K_MAX}, T - 1) = {min(K_MAX, T - 1)} (got {K})")


def host_finish(G, K):
    """Host side of the fit for one channel: G [T, T] fp64 centred Gram -> (lam [K] descending, A [K, T] = V^T / sqrt(lam),
    explained_variance [K], explained_variance_ratio [K])."""
    G = np.asarray(G, dtype=np.float64)
    T = G.shape[0]
    w, V = np.linalg.eigh(G)
    order = np.argsort(w, kind="stable")[::-1][:K]
    lam = w[order]
    V = V[:, order]
    A = (V / np.sqrt(np.maximum(lam, np.finfo(np.float64).tiny))).T
    return lam, A, lam / (T - 1), lam / np.trace(G)


def sign_rule(E):
    """sklearn's svd_flip(u_based_decision=False) on the rows of E [K, P]: the entry of largest magnitude (lowest index on ties)
    of every row becomes positive.  The device applies the same rule (dg_eof_flip); this is its host statement."""
    E = np.array(E, dtype=np.float64, copy=True)
    i = np.argmax(np.abs(E), axis=1)
    s = np.sign(E[np.arange(E.shape[0]), i])
    s[s == 0] = 1.0
    return E * s[:, None]


class EOFChannel:
    """One channel of a fitted ``EOF`` with sklearn ``PCA``'s attribute names (device tensors): what the reference passes as
    ``transformer_u`` / ``transformer_v``."""

    def __init__(self, eof, c):
        self._eof, self.channel = eof, c
        self.mean_ = eof.mean_[c]
        self.components_ = eof.components_[c]
        self.explained_variance_ = eof.explained_variance_[c]
        self.explained_variance_ratio_ = eof.explained_variance_ratio_[c]
        self.n_components = self.n_components_ = eof.n_components

    def transform(self, X):
        """X [B, P] (or [B, H, W]) -> Z [B, K] fp32 on the device: (X - mean_) components_^T (sklearn ``PCA.transform``)."""
        o = self._eof.ops
        X = torch.as_tensor(X)
        B = X.shape[0]
        y = X.reshape(B, 1, -1).to(o.device, torch.float32).contiguous()
        P = y.shape[2]
        assert P == self.mean_.numel(), (P, self.mean_.numel())
        K = self.n_components
        Z = torch.empty(B, 1, K, dtype=torch.float32, device=o.device)
        o.eof_project(o.eof_fields(y), self.mean_, self.components_, K, P, 0, Z)
        return Z[:, 0]

    def inverse_transform(self, Z):
        """Z [B, K] -> [B, P] fp32: Z components_ + mean_."""
        o = self._eof.ops
        Z = torch.as_tensor(Z).to(o.device, torch.float32).reshape(-1, 1, self.n_components).contiguous()
        P = self.mean_.numel()
        out = torch.empty(Z.shape[0], 1, P, dtype=torch.float32, device=o.device)
        o.eof_reconstruct(Z, self.components_, P, 0, P, self.mean_, out)
        return out[:, 0]


class EOF:
    """``EOF(n_components).fit(fields)``: one PCA per channel.  ``fields`` is an NCHW tensor [T, C, H, W] (fp32, host or device)
    or a ``ResidentLoader``, whose fine store [T, H, W, c] is read in place.  Attributes (device tensors): ``mean_`` [C, P],
    ``components_`` [C, K, P], ``explained_variance_`` [C, K], ``explained_variance_ratio_`` [C, K]."""

    def __init__(self, n_components, device="cuda:0", ops=None):
        self.n_components = int(n_components)
        self._device, self._ops = device, ops

    @property
    def ops(self):
        if self._ops is None:
            self._ops = backend.make_ops("f32", self._device)
        return self._ops

    def fit(self, fields):
        K = self.n_components
        if hasattr(fields, "store_f"):                       # ResidentLoader: [n, H, W, c] in the compute dtype, no copy
            store = fields.store_f
            T, H, W, Cn = store.shape
            check_limits(T, Cn, K)
            if self._ops is None:
                self._device = str(store.device)
            o = self.ops
            src, f = store, o.eof_fields(store, nhwc=True)
        else:
            x = torch.as_tensor(fields)
            assert x.dim() == 4, "fields: [T, C, H, W]"
            T, Cn, H, W = x.shape
            check_limits(T, Cn, K)
            o = self.ops
            src = x.to(o.device, torch.float32).contiguous()
            f = o.eof_fields(src)
        P = H * W
        dev = o.device
        mu = torch.empty(Cn, P, dtype=torch.float32, device=dev)
        o.eof_mean(f, mu)
        G = torch.empty(Cn, T, T, dtype=torch.float64, device=dev)
        o.eof_gram(f, mu, G)
        Gh = G.cpu().numpy()
        KB = (K + 15) // 16 * 16
        A = np.zeros((Cn, T, KB), dtype=np.float32)
        var, ratio = np.zeros((Cn, K)), np.zeros((Cn, K))
        for c in range(Cn):
            _, Ac, var[c], ratio[c] = host_finish(Gh[c], K)
            A[c, :, :K] = Ac.T
        E = torch.empty(Cn, K, P, dtype=torch.float32, device=dev)
        amax = torch.empty(Cn, K, dtype=torch.int64, device=dev)
        o.eof_components(f, mu, torch.from_numpy(A).to(dev), K, E, amax)
        torch.cuda.current_stream(dev).synchronize()         # src / A may be freed on return
        self.mean_, self.components_ = mu, E
        self.explained_variance_ = torch.from_numpy(var).to(dev, torch.float32)
        self.explained_variance_ratio_ = torch.from_numpy(ratio).to(dev, torch.float32)
        self.n_samples_, self.shape_ = T, (Cn, H, W)
        return self

    def transform(self, Y):
        """Y [B, C, H, W] -> Z [B, C, K] fp32: the centred projection of every channel on its components."""
        o = self.ops
        Cn, H, W = self.shape_
        y = torch.as_tensor(Y).to(o.device, torch.float32).contiguous()
        assert tuple(y.shape[1:]) == (Cn, H, W), (tuple(y.shape), self.shape_)
        K, P = self.n_components, H * W
        Z = torch.empty(y.shape[0], Cn, K, dtype=torch.float32, device=o.device)
        o.eof_project(o.eof_fields(y), self.mean_, self.components_, K, P, K * P, Z)
        return Z

    def inverse_transform(self, Z):
        """Z [B, C, K] -> [B, C, H, W] fp32 with the mean added back."""
        o = self.ops
        Cn, H, W = self.shape_
        Z = torch.as_tensor(Z).to(o.device, torch.float32).contiguous()
        K, P = self.n_components, H * W
        assert tuple(Z.shape[1:]) == (Cn, K), (tuple(Z.shape), (Cn, K))
        out = torch.empty(Z.shape[0], Cn, H, W, dtype=torch.float32, device=o.device)
        o.eof_reconstruct(Z, self.components_, P, K * P, P, self.mean_, out)
        return out

    def channel(self, c):
        return EOFChannel(self, c)


def get_eofs_and_project(ncomp, X, device="cuda:0"):
    """Mirror of prep_gan.py:226-255: X [T, H, W] (one variable) -> (EOFs [K, P], Z [T, K], pca), device tensors; ``pca`` is the
    channel view (``EOFChannel``) with sklearn's attribute names."""
    x = torch.as_tensor(np.asarray(X) if not torch.is_tensor(X) else X)
    T, H, W = x.shape
    pca = EOF(ncomp, device=device).fit(x.reshape(T, 1, H, W)).channel(0)
    return pca.components_, pca.transform(x.reshape(T, H * W)), pca
