"""Times the EOF path (csrc/eof.hip) on one GPU and writes one JSON record.

  fit of T = 1024 and T = 4096 snapshots of 2 x 1024^2 fields read in place from a ResidentLoader store, bf16 and fp32:
      dg_eof_mean, dg_eof_gram (TFLOP/s against the 157.3 TFLOP/s f32 MFMA peak), host eigh, dg_eof_components + dg_eof_flip
  projection (dg_eof_project) and reconstruction (dg_eof_reconstruct) of a batch of 32, K = 20 (GB/s against HBM)

Usage: python tools/eof_bench.py [--T 1024 4096] [--dtypes bf16 f32] [--out record.json]
Kernel times are device-event times of the launches (each call warmed up once, then the median of --reps); the host eigh time is
a host clock around numpy's eigh of every channel's fp64 Gram.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from downgan_amd import _lib, eof  # noqa: E402
from downgan_amd.GAN.dataloader import ResidentLoader  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402

F32_MFMA_PEAK = 157.3e12
HBM_MEASURED = 6.29e12          # float4 copy on MI355X (MI355X_MICROARCH: 79 % of the 8 TB/s spec)


def timed(fn, reps):
    ts = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts))


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:16]


def fill_store(T, H, W, C, dtype, dev):
    """Smooth random-phase fields (low rank + noise) generated on the device, a chunk at a time."""
    store = torch.empty(T, H, W, C, dtype=dtype, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    modes = torch.randn(30, H, W, C, generator=g, device=dev) * (2.0 ** (-torch.arange(30, device=dev) / 4)).view(30, 1, 1, 1)
    for a in range(0, T, 64):
        n = min(64, T - a)
        coef = torch.randn(n, 30, generator=g, device=dev)
        x = (coef @ modes.view(30, -1)).view(n, H, W, C) + 1e-3 * torch.randn(n, H, W, C, generator=g, device=dev)
        store[a:a + n] = x.to(dtype)
    return store


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "f32"])
    ap.add_argument("--H", type=int, default=1024)
    ap.add_argument("--W", type=int, default=1024)
    ap.add_argument("--K", type=int, default=20)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    C, H, W, K, B = 2, a.H, a.W, a.K, a.B
    P = H * W
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "eof_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "eof.hip")), "C": C, "H": H, "W": W, "K": K, "runs": []}
    for T in a.T:
        for dt in a.dtypes:
            tdt = torch.bfloat16 if dt == "bf16" else torch.float32
            store = fill_store(T, H, W, C, tdt, dev)
            loader = ResidentLoader(None, 1, dtype=dt, device=dev, ops=ops if dt == "f32" else None,
                                    _stores=(torch.zeros(T, 1, 1, C, dtype=tdt, device=dev), store))
            esz = store.element_size()
            f = ops.eof_fields(loader.store_f, nhwc=True)
            mu = torch.empty(C, P, dtype=torch.float32, device=dev)
            G = torch.empty(C, T, T, dtype=torch.float64, device=dev)
            t_mean = timed(lambda: ops.eof_mean(f, mu), a.reps)
            t_gram = timed(lambda: ops.eof_gram(f, mu, G), a.reps)
            Gh = G.cpu().numpy()
            t0 = time.perf_counter()
            KB = (K + 15) // 16 * 16
            A = np.zeros((C, T, KB), dtype=np.float32)
            for c in range(C):
                A[c, :, :K] = eof.host_finish(Gh[c], K)[1].T
            t_eigh = time.perf_counter() - t0
            Ad = torch.from_numpy(A).to(dev)
            E = torch.empty(C, K, P, dtype=torch.float32, device=dev)
            amax = torch.empty(C, K, dtype=torch.int64, device=dev)
            t_comp = timed(lambda: ops.eof_components(f, mu, Ad, K, E, amax), a.reps)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e = eof.EOF(K, ops=ops).fit(loader)
            torch.cuda.synchronize()
            t_fit = time.perf_counter() - t0
            ns, ntiles = ops.eof_gram_slices(T, C, P)
            gram_alg = C * T * (T + 1) / 2 * 2.0 * P           # upper triangle incl. diagonal
            gram_exec = C * ntiles * 64 * 64 * 2.0 * P         # 64 x 64 tiles as executed
            read = float(T) * C * P * esz
            r = {"T": T, "dtype": dt, "gram_slices": ns, "gram_tiles": ntiles,
                 "mean_s": t_mean, "mean_GBps": read / t_mean / 1e9, "mean_hbm_frac": read / t_mean / HBM_MEASURED,
                 "gram_s": t_gram, "gram_TFLOPs_alg": gram_alg / t_gram / 1e12, "gram_TFLOPs_exec": gram_exec / t_gram / 1e12,
                 "gram_frac_f32_mfma_peak": gram_alg / t_gram / F32_MFMA_PEAK,
                 "host_eigh_s": t_eigh,
                 "components_s": t_comp, "components_GBps": (read + C * K * P * 4.0) / t_comp / 1e9,
                 "fit_total_s": t_fit}
            if T == a.T[0]:
                y = store[:B].permute(0, 3, 1, 2).float().contiguous()
                Z = torch.empty(B, C, K, dtype=torch.float32, device=dev)
                fy = ops.eof_fields(y)
                t_proj = timed(lambda: ops.eof_project(fy, e.mean_, e.components_, K, P, K * P, Z), a.reps)
                out = torch.empty(B, C, P, dtype=torch.float32, device=dev)
                t_rec = timed(lambda: ops.eof_reconstruct(Z, e.components_, P, K * P, P, e.mean_, out), a.reps)
                pb = (B * C * P + K * C * P + C * P) * 4.0
                rb = (K * C * P + C * P + B * C * P) * 4.0
                r.update({"project_B": B, "project_s": t_proj, "project_GBps": pb / t_proj / 1e9, "project_hbm_frac": pb / t_proj / HBM_MEASURED,
                          "reconstruct_s": t_rec, "reconstruct_GBps": rb / t_rec / 1e9, "reconstruct_hbm_frac": rb / t_rec / HBM_MEASURED})
                del y, out
            print(json.dumps(r), flush=True)
            rec["runs"].append(r)
            del store, loader, f, e, G, E
            torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
