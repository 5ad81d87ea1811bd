"""Times the value histograms (csrc/histogram.hip, downgan_amd.histograms.histogram) on one GPU and prints one JSON record.

Cases (B = 32 fields of C = 2 channels + their speed, 2048 bins, HistSpec.zscore(2)):
  nhwc_bf16_padded_1024_gauss   the generator's output at BASELINE configs[1]: [32, 1024, 1024, 16] bf16, the 2 leading channels
                                read, Gaussian values
  nchw_f32_1024_gauss           [32, 2, 1024, 1024] fp32
  nhwc_bf16_padded_1024_const   the configs[1] layout holding one value: every lane of a wave adds to one LDS bin (the
                                contention worst case)
Each case records ms per call (device events, warmed up, median of --reps), the bytes the histograms need (the values read
once) and the bytes stored (the tensor's footprint, padding included), the effective GB/s on each, and the ratio to one
TrainEngine.metrics_pass at configs[1] (timed in the same process; --no-metrics-pass skips it).

Usage: python tools/hist_bench.py [--reps 10] [--out record.json]
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

from downgan_amd import _lib, histograms  # noqa: E402
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
    B, C, N = a.B, 2, 1024
    spec = histograms.HistSpec.zscore(C)
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "histogram_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "histogram.hip")), "B": B, "C": C,
           "bins": spec.bins, "nout": spec.nout, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    pad = torch.empty(B, N, N, 16, dtype=torch.bfloat16, device=dev)
    pad.copy_(torch.randn(B, N, N, 16, generator=g, device=dev))
    cases = [("nhwc_bf16_padded_1024_gauss", pad, {"nhwc": True, "channels": C}),
             ("nchw_f32_1024_gauss", torch.randn(B, C, N, N, generator=g, device=dev), {}),
             ("nhwc_bf16_padded_1024_const", torch.full((B, N, N, 16), 1.25, dtype=torch.bfloat16, device=dev),
              {"nhwc": True, "channels": C})]
    for name, x, kw in cases:
        acc = histograms.ValueHistogram(spec, dev, ops=ops)
        t = timed(lambda: acc.add(x, **kw), a.reps)
        need = B * C * N * N * x.element_size()                      # the values the histograms need, read once
        stored = x.numel() * x.element_size()                        # the tensor as stored (padded channels included)
        r = {"case": name, "shape": list(x.shape), "dtype": str(x.dtype).replace("torch.", ""), "ms": t * 1e3,
             "bytes_needed": need, "bytes_stored": stored, "GBps_needed": need / t / 1e9, "GBps_stored": stored / t / 1e9,
             "hbm_frac_stored": stored / t / HBM_MEASURED, "ws_bytes": ops.hist_ws_bytes(ops.eof_fields(x[:1], **kw), spec.struct())}
        print(json.dumps(r), flush=True)
        rec["cases"].append(r)
    del cases, x, pad
    torch.cuda.empty_cache()
    if not a.no_metrics_pass:
        mp = metrics_pass_s(max(3, a.reps // 3))
        rec["metrics_pass_cfg2_ms"] = mp * 1e3
        for r in rec["cases"]:
            r["ratio_to_metrics_pass"] = r["ms"] / (mp * 1e3)
            r["ratio_real_plus_fake"] = 2 * r["ms"] / (mp * 1e3)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
