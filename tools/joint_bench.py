"""Times the joint histograms (csrc/joint.hip, downgan_amd.joint.ValueJoint) on one GPU and prints one JSON record.

The pair of series of BASELINE configs[1]: real and generated [32, 1024, 1024, 16] bf16 in the padded NHWC layout, the 2 leading
channels read, under JointSpec.zscore(2) (7 pairs, 48919 cells: the roses and (u, v) densities of both series, the
real-vs-generated densities of u, v and the speed).  Cases:
  gauss      Gaussian values in both series
  const      one value per series: every lane of a wave adds to one LDS cell per pair (the contention worst case)
Each case records ms per ``add`` (device events, warmed up, median of --reps), the bytes stored (both tensors, padding included)
and the bytes needed (the values read, once), the effective GB/s on each -- and as the yardstick the same for two dg_hist calls
(HistSpec.zscore(2)) over the same two series.

The LDS budget of a workgroup is a compile-time constant of joint.hip (DG_JOINT_LDS_CELLS): to compare budgets, build the A/B
library (`make -C downgan_amd/csrc joint147`) and run this tool once per library with DG_LIB_OVERRIDE pointing at it and --label
naming it; --merge adds the record to the cases of an existing --out file instead of replacing it.

Usage: python tools/joint_bench.py [--reps 10] [--label lds64] [--out profiles/joint_bench_cfg2.json] [--merge]
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

from downgan_amd import _lib, histograms, joint  # noqa: E402
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
    ap.add_argument("--label", default="default", help="names the library build in the record (e.g. the LDS budget)")
    ap.add_argument("--out", default=None, help="also write the record (indented JSON) to this file")
    ap.add_argument("--merge", action="store_true", help="append this run to the runs of an existing --out file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    B, C, N = a.B, 2, 1024
    jspec, hspec = joint.JointSpec.zscore(C), histograms.HistSpec.zscore(C)
    run = {"label": a.label, "lib": os.path.basename(_lib.LIB_PATH), "lib_sha16": sha(_lib.LIB_PATH),
           "joint_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "joint.hip")), "B": B, "C": C,
           "pairs": jspec.names, "cells": jspec.offsets()[-1], "hist_bins": hspec.bins, "reps": a.reps, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def gauss():
        x = torch.empty(B, N, N, 16, dtype=torch.bfloat16, device=dev)
        x.copy_(torch.randn(B, N, N, 16, generator=g, device=dev))
        return x
    kw = {"nhwc": True, "channels": C}
    for name, make in (("gauss", lambda: (gauss(), gauss())),
                       ("const", lambda: (torch.full((B, N, N, 16), 1.25, dtype=torch.bfloat16, device=dev),
                                          torch.full((B, N, N, 16), -0.75, dtype=torch.bfloat16, device=dev)))):
        xa, xb = make()
        accj = joint.ValueJoint(jspec, dev, ops=ops)
        ha, hb = histograms.ValueHistogram(hspec, dev, ops=ops), histograms.ValueHistogram(hspec, dev, ops=ops)
        tj = timed(lambda: accj.add(xa, xb, **kw), a.reps)

        def two_hists():
            ha.add(xa, **kw)
            hb.add(xb, **kw)
        th = timed(two_hists, a.reps)
        need = 2 * B * C * N * N * xa.element_size()                  # the values both diagnostics need, read once
        stored = 2 * xa.numel() * xa.element_size()                   # the two tensors as stored (padded channels included)
        r = {"case": name, "shape": list(xa.shape), "dtype": "bfloat16", "bytes_needed": need, "bytes_stored": stored,
             "hist2d_ms": tj * 1e3, "hist2d_GBps_needed": need / tj / 1e9, "hist2d_GBps_stored": stored / tj / 1e9,
             "hist2d_hbm_frac_stored": stored / tj / HBM_MEASURED,
             "hist_x2_ms": th * 1e3, "hist_x2_GBps_needed": need / th / 1e9, "hist_x2_GBps_stored": stored / th / 1e9,
             "hist2d_over_hist_x2": tj / th}
        print(json.dumps(r), flush=True)
        run["cases"].append(r)
        del xa, xb, accj, ha, hb
        torch.cuda.empty_cache()
    rec = {"gpu": torch.cuda.get_device_name(0), "runs": [run]}
    if a.out and a.merge and os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        rec["runs"] = [r for r in old.get("runs", []) if r.get("label") != a.label] + [run]
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
