"""Analytic field series for the EOF tests (tests/test_eof_*.py, tests/golden/make_golden_eof.py).

x[t, c, y, x] = sum_m 2^(-m/4) s_m(t) phi_m,c(y, x)  +  noise(t, c, y, x)

30 smooth modes: phi_m,c = cos(2 pi (kx x / W + ky y / H) + 0.7 c + 0.3 m) with distinct wavenumbers (kx, ky), time signals
s_m(t) = sin(2 pi 0.0137 (m + 1) t + 0.5 m), and integer-hash noise of amplitude 1e-3.  The geometric amplitudes keep the
eigenvalues well apart (about a factor sqrt(2) between neighbours), so component directions and signs are stable, while the 20
leading ones stay within three decades of each other: an fp32 Gram resolves them to ~1e-6 (a steeper spectrum would push the
trailing eigenvalues under the fp32 rounding of the leading ones); the formula regenerates the same data on any machine
(no RNG stream, no reference, no sklearn).  Computed in float64 with torch, on the host or on a device, a chunk of snapshots at
a time.
"""
from __future__ import annotations

import math

import torch

N_MODES = 30


def _noise(t, C, H, W, device):
    n = ((t.view(-1, 1, 1, 1) * C + torch.arange(C, device=device).view(1, -1, 1, 1)) * H
         + torch.arange(H, device=device).view(1, 1, -1, 1)) * W + torch.arange(W, device=device).view(1, 1, 1, -1)
    m = 0xFFFFFFFF
    h = (n * 0x9E3779B1) & m
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & m
    h = h ^ (h >> 13)
    return (h.to(torch.float64) / 2.0 ** 32 - 0.5) * 2e-3


def fields(t0, T, C, H, W, device="cpu", chunk=64):
    """[T, C, H, W] float64 for snapshots t0 .. t0 + T - 1."""
    yy = torch.arange(H, device=device, dtype=torch.float64).view(H, 1) / H
    xx = torch.arange(W, device=device, dtype=torch.float64).view(1, W) / W
    out = torch.empty(T, C, H, W, dtype=torch.float64, device=device)
    for a in range(0, T, chunk):
        t = torch.arange(t0 + a, t0 + min(T, a + chunk), device=device)
        tf = t.to(torch.float64)
        acc = _noise(t, C, H, W, device)
        for m in range(N_MODES):
            kx, ky = m % 6, m // 6 + 1
            s = torch.sin(2 * math.pi * 0.0137 * (m + 1) * tf + 0.5 * m).view(-1, 1, 1, 1)
            for c in range(C):
                phi = torch.cos(2 * math.pi * (kx * xx + ky * yy) + 0.7 * c + 0.3 * m)
                acc[:, c] += 2.0 ** (-m / 4) * s[:, 0] * phi
        out[a:a + len(t)] = acc
    return out
