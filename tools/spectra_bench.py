"""Times the radially averaged power spectra (csrc/spectra.hip, downgan_amd.spectra.rapsd) on one GPU and prints one JSON record.

Cases (B = 32 fields of C = 2 channels):
  nhwc_bf16_padded_1024   the generator's output at BASELINE configs[1]: [32, 1024, 1024, 16] bf16, the 2 leading channels read
  nhwc_bf16_padded_128    the same layout at N = 128
  nchw_f32_1024           [32, 2, 1024, 1024] fp32
Each case records ms per call (device events, warmed up, median of --reps), the bytes the algorithm moves (the fields read once +
the half-spectrum workspace written and read), the effective GB/s, and the ratio to one TrainEngine.metrics_pass at configs[1]
(timed in the same process; --no-metrics-pass skips it).

Usage: python tools/spectra_bench.py [--reps 10] [--out record.json]
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
CFG2 = (32, 128, 128, 2, 16)    # bench.py WORKLOADS["cfg2"] = BASELINE configs[1]: B, S, filters, cin, residual blocks


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


def metrics_pass_s(reps):
    from downgan_amd import synthetic
    from downgan_amd.engine import HyperParams, TrainEngine
    B, S, F_, cin, nrb = CFG2
    ops = HipOps("bf16", "cuda:0")
    eng = TrainEngine(ops, S, F_, cin, B, HyperParams(batch_size=B), num_res_blocks=nrb)
    eng.G.load_state_dict(synthetic.generator_params(F_, cin, 2, nrb))
    eng.C.load_state_dict(synthetic.critic_params(F_, 8 * S, 2))
    coarse, fine = synthetic.tiles(B, cin, S)
    xc = ops.zeros(B, S, S, eng.G.cin_p); ops.nchw_to_nhwc(torch.from_numpy(coarse).cuda(), xc)
    xf = ops.zeros(B, 8 * S, 8 * S, eng.G.np_p); ops.nchw_to_nhwc(torch.from_numpy(fine).cuda(), xf)
    t = timed(lambda: eng.metrics_pass(xc, xf), reps)
    del eng, xc, xf
    torch.cuda.empty_cache()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--no-metrics-pass", action="store_true")
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    B, C = a.B, 2
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "spectra_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "spectra.hip")), "B": B, "C": C, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    cases = []
    for N in (1024, 128):
        x = torch.empty(B, N, N, 16, dtype=torch.bfloat16, device=dev)
        x.copy_(torch.randn(B, N, N, 16, generator=g, device=dev))
        cases.append((f"nhwc_bf16_padded_{N}", x, {"nhwc": True, "channels": C}, N))
    cases.append(("nchw_f32_1024", torch.randn(B, C, 1024, 1024, generator=g, device=dev), {}, 1024))
    for name, x, kw, N in cases:
        K = N // 2 + 1
        t = timed(lambda: spectra.rapsd(x, ops=ops, **kw), a.reps)
        fields = B * C * N * N * x.element_size()                    # the values the spectra need, read once
        footprint = x.numel() * x.element_size()                     # the tensor as stored (padded channels included)
        spec = B * C * K * N * 8                                     # fp32 complex half spectra, written once and read once
        moved = fields + 2 * spec
        r = {"case": name, "N": N, "shape": list(x.shape), "dtype": str(x.dtype).replace("torch.", ""), "ms": t * 1e3,
             "bytes_fields": fields, "bytes_stored": footprint, "bytes_workspace_rw": 2 * spec, "bytes_moved": moved,
             "GBps": moved / t / 1e9, "hbm_frac": moved / t / HBM_MEASURED,
             "ws_bytes": ops.rapsd_ws_bytes(B, C, N)}
        print(json.dumps(r), flush=True)
        rec["cases"].append(r)
    del cases, x
    torch.cuda.empty_cache()
    if not a.no_metrics_pass:
        mp = metrics_pass_s(max(3, a.reps // 3))
        rec["metrics_pass_cfg2_ms"] = mp * 1e3
        for r in rec["cases"]:
            r["ratio_to_metrics_pass"] = r["ms"] / (mp * 1e3)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
