"""Times the Helmholtz spectra (csrc/spectra.hip, downgan_amd.spectra.helmholtz_rapsd / helmholtz_cross) on one GPU next to
``cross_rapsd`` on the same tensors in the same run, and prints one JSON record.

Cases (T = 32 fields of 2 channels, fp32 NCHW, N in {128, 1024}):
  helmholtz_ms         helmholtz_rapsd(a): two row passes (u and v of one field), one column pass over two half spectra
  helmholtz_cross_ms   helmholtz_cross(a, b): four row passes, one column pass over four half spectra, eight planes
  cross_c1_ms          cross_rapsd(a[:, :1], b[:, :1]): two row passes, one column pass over two half spectra -- THE YARDSTICK of
                       the one-sided call, which moves the same bytes
  cross_c2_ms          cross_rapsd(a, b): four row passes, two column workgroups' worth of lines per pair -- the yardstick of the
                       paired call
Each is ms per call (device events, warmed up, median of --reps); ``calls`` is the number of library calls the batch is split
into under spectra.WS_CAP.  bytes_moved counts the fields read once and the half-spectrum buffers written and read once.

Usage: python tools/helmholtz_bench.py [--reps 10] [--out record.json]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from downgan_amd import _lib, spectra  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402

HBM_MEASURED = 6.29e12          # float4 copy on MI355X (79 % of the 8 TB/s spec)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    T = a.T
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "spectra_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "spectra.hip")), "T": T,
           "yardstick": "cross_rapsd with C = 1 (one-sided) and C = 2 (paired) on the same tensors, same process", "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for N in (128, 1024):
        K = N // 2 + 1
        xa = torch.randn(T, 2, N, N, generator=g, device=dev)
        xb = torch.randn(T, 2, N, N, generator=g, device=dev)
        a1, b1 = xa[:, :1].contiguous(), xb[:, :1].contiguous()
        t_one = timed(lambda: spectra.helmholtz_rapsd(xa, ops=ops), a.reps)
        t_two = timed(lambda: spectra.helmholtz_cross(xa, xb, ops=ops), a.reps)
        t_c1 = timed(lambda: spectra.cross_rapsd(a1, b1, ops=ops), a.reps)
        t_c2 = timed(lambda: spectra.cross_rapsd(xa, xb, ops=ops), a.reps)
        spec = T * K * N * 8                                         # one component's fp32 complex half spectra
        field = T * N * N * 4                                        # one component's values
        moved_one, moved_two = 2 * field + 4 * spec, 4 * field + 8 * spec
        r = {"case": f"nchw_f32_{N}", "N": N, "helmholtz_ms": t_one * 1e3, "cross_c1_ms": t_c1 * 1e3, "ratio_one": t_one / t_c1,
             "helmholtz_cross_ms": t_two * 1e3, "cross_c2_ms": t_c2 * 1e3, "ratio_two": t_two / t_c2,
             "bytes_moved_one": moved_one, "bytes_moved_two": moved_two,
             "GBps_one": moved_one / t_one / 1e9, "GBps_two": moved_two / t_two / 1e9,
             "hbm_frac_one": moved_one / t_one / HBM_MEASURED, "hbm_frac_two": moved_two / t_two / HBM_MEASURED,
             "calls_one": -(-T // spectra._helm_chunk(ops, T, N, False)), "calls_two": -(-T // spectra._helm_chunk(ops, T, N, True)),
             "calls_c1": -(-T // spectra._cross_chunk(ops, T, 1, N)), "calls_c2": -(-T // spectra._cross_chunk(ops, T, 2, N))}
        print(json.dumps(r), flush=True)
        rec["cases"].append(r)
        del xa, xb, a1, b1
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
