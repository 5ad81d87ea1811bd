"""Times the cross spectra (csrc/spectra.hip, downgan_amd.spectra.cross_rapsd) on one GPU against their baseline in the same
run, rapsd(a) + rapsd(b) on the same tensors, and prints one JSON record.

Cases (B = 32 pairs of C = 2 channels, N in {128, 1024}):
  nchw_f32_N              both sides [32, 2, N, N] fp32
  nhwc_bf16_padded_N      both sides [32, N, N, 16] bf16, the 2 leading channels read (the generator's output layout)
Each case records ms per call of both (device events, warmed up, median of --reps), their ratio cross / (rapsd + rapsd), the
bytes the cross spectra move (both sides' fields read once + both half-spectrum buffers written and read) and the effective GB/s.
The row passes of the two are the same kernels on the same data and the column pass reads the same bytes once, so the byte count
predicts a ratio near 1; what differs is the column pass's LDS footprint (64 KB against 48 KB per workgroup) and, under
spectra.WS_CAP, the number of calls a batch is split into (``calls`` in the record).

Usage: python tools/coherence_bench.py [--reps 10] [--out record.json]
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
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    B, C = a.B, 2
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "spectra_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "spectra.hip")), "B": B, "C": C,
           "baseline": "rapsd(a) + rapsd(b) on the same tensors, same process", "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def make(layout, N):
        if layout == "nchw_f32":
            return torch.randn(B, C, N, N, generator=g, device=dev), {}
        x = torch.empty(B, N, N, 16, dtype=torch.bfloat16, device=dev)
        x.copy_(torch.randn(B, N, N, 16, generator=g, device=dev))
        return x, {"nhwc": True, "channels": C}

    for N in (128, 1024):
        for layout in ("nchw_f32", "nhwc_bf16_padded"):
            K = N // 2 + 1
            (xa, kw), (xb, _) = make(layout, N), make(layout, N)
            t_cross = timed(lambda: spectra.cross_rapsd(xa, xb, ops=ops, **kw), a.reps)
            t_pair = timed(lambda: (spectra.rapsd(xa, ops=ops, **kw), spectra.rapsd(xb, ops=ops, **kw)), a.reps)
            fields = 2 * B * C * N * N * xa.element_size()               # both sides' values, read once
            spec = 2 * B * C * K * N * 8                                 # both fp32 complex half spectra
            moved = fields + 2 * spec                                    # ... written once and read once
            tc = spectra._cross_chunk(ops, B, C, N)
            r = {"case": f"{layout}_{N}", "N": N, "shape": list(xa.shape), "dtype": str(xa.dtype).replace("torch.", ""),
                 "cross_ms": t_cross * 1e3, "rapsd_pair_ms": t_pair * 1e3, "ratio": t_cross / t_pair,
                 "bytes_fields": fields, "bytes_workspace_rw": 2 * spec, "bytes_moved": moved,
                 "GBps": moved / t_cross / 1e9, "hbm_frac": moved / t_cross / HBM_MEASURED,
                 "ws_bytes": ops.cross_rapsd_ws_bytes(tc, C, N), "calls": -(-B // tc),
                 "rapsd_calls": 2 * -(-B // spectra._chunk(ops, B, C, N))}
            print(json.dumps(r), flush=True)
            rec["cases"].append(r)
            del xa, xb
            torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
