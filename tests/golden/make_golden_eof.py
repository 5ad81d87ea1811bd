"""Generate tests/golden/eof.json from the REAL reference and sklearn (build container only).

Run:  python tests/golden/make_golden_eof.py      (needs sklearn and the reference checkout: $DOWNGAN_REFERENCE, default
      a `reference` directory beside this repository)

The fields come from the analytic formula of tests/eof_fixture.py (T = 100 fit snapshots, 8 held-out ones, C = 2, 64 x 64),
rounded to fp32 like the native fit reads them.  Recorded: sklearn PCA(20, svd_solver="full") per channel (explained_variance_,
256 sampled components_ entries, transform of the 8 held-out snapshots), the reference's eof_loss of one (hr, fake) pair and
sampled entries of its low_pass_eof_batch with fake=False and fake=True.  The reference's losses module imports pytorch_msssim,
absent here and not on the recorded path: an inert placeholder satisfies it.  Data only.
"""
from __future__ import annotations

import importlib.machinery
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("DOWNGAN_REFERENCE", os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), "reference"))

import eof_fixture  # noqa: E402

T, TH, C, H, W, K, NS = 100, 8, 2, 64, 64, 20, 256


class _Inert(types.ModuleType):
    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return object


def sample_index(n_rows, n_cols, n):
    """Deterministic (row, col) samples shared with the tests."""
    i = np.arange(n, dtype=np.int64)
    return (i % n_rows).tolist(), ((i * 2654435761) % n_cols).tolist()


def main():
    from sklearn.decomposition import PCA
    sys.path.insert(0, REF)
    m = _Inert("pytorch_msssim")
    m.__spec__ = importlib.machinery.ModuleSpec("pytorch_msssim", None)
    sys.modules["pytorch_msssim"] = m
    from DoWnGAN.GAN import losses as ref

    x = eof_fixture.fields(0, T + TH, C, H, W).to(torch.float32)
    fit, held = x[:T], x[T:]
    P = H * W
    pcas, out = [], {"T": T, "held": TH, "C": C, "H": H, "W": W, "K": K}
    rows, cols = sample_index(K, P, NS)
    out["sample_k"], out["sample_p"] = rows, cols
    for c in range(C):
        p = PCA(K, svd_solver="full").fit(fit[:, c].reshape(T, P).double().numpy())
        pcas.append(p)
        out[f"var{c}"] = p.explained_variance_.tolist()
        out[f"ratio{c}"] = p.explained_variance_ratio_.tolist()
        out[f"comp{c}"] = p.components_[rows, cols].tolist()
        out[f"transform{c}"] = p.transform(held[:, c].reshape(TH, P).double().numpy()).tolist()
    X = torch.from_numpy(np.stack([p.components_ for p in pcas], axis=1)).float()      # [K, C, P]
    hr, fake = held[:4], held[4:]
    out["eof_loss"] = ref.eof_loss(X, hr, fake, torch.device("cpu"))
    Z = torch.stack([torch.from_numpy(pcas[c].transform(hr[:, c].reshape(4, P).double().numpy())) for c in range(C)], dim=1)
    lows = ref.low_pass_eof_batch(Z, X, hr, pcas, torch.device("cpu"), fake=False)
    lows_f = ref.low_pass_eof_batch(None, X, fake, pcas, torch.device("cpu"), fake=True)
    n = lows.numel()
    idx = ((np.arange(NS, dtype=np.int64) * 2654435761) % n).tolist()
    out["lows_shape"] = list(lows.shape)
    out["lows_index"] = idx
    out["lows"] = lows.reshape(-1)[idx].double().tolist()
    out["lows_absmax"] = float(lows.abs().max())
    out["lows_fake"] = lows_f.reshape(-1)[idx].double().tolist()
    out["lows_fake_absmax"] = float(lows_f.abs().max())
    with open(os.path.join(HERE, "eof.json"), "w") as f:
        json.dump(out, f)
    print("wrote", os.path.join(HERE, "eof.json"), os.path.getsize(os.path.join(HERE, "eof.json")), "bytes")


if __name__ == "__main__":
    main()
