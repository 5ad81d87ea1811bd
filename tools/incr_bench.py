"""Times the increment histograms (csrc/increments.hip, downgan_amd.increments.Increments) on one GPU and prints one JSON record.

The benchmarked evaluation shape: 32 fields of 2 channels, 1024 x 1024, as bf16 in the padded NHWC layout ([32, 1024, 1024, 16],
the 2 leading channels read) and as fp32 NCHW, under IncrementSpec.zscore(2) (the default 8 lags, 128 bins, 2 components + the
speed: 3 x 2 x 8 tables per series).  One series per timed call.  Cases:
  gauss      Gaussian values
  const      one value: every lane of a wave adds to one LDS cell per lag (the contention worst case of a peaked distribution)
Each case records, in ms per call (device events, warmed up, median of --reps):
  incr       (a) dg_incr
  hist       (b) dg_hist on the same fields (HistSpec.zscore(2)): the cost of reading the input once and binning it
  torch      (c) the same counts formed with stock torch ops: per output channel, direction and lag a slice-subtract and one
             torch.histc (gauss / nchw_f32 only: the layout a user of stock ops would hold; the speed is formed once, untimed)
and incr / hist.  The naive all-global variant (d) and the per-wave sub-tables are compile-time variants of increments.hip: build
the A/B libraries (`make -C downgan_amd/csrc incr_naive incr_sub4`) and run this tool once per library with --lib pointing at it and
--label naming it; --merge adds the record to the runs of an existing --out file instead of replacing it.

Usage: python tools/incr_bench.py [--reps 10] [--lib PATH] [--label tiled] [--out profiles/incr_bench.json] [--merge]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _lib_arg():
    """--lib must reach _lib before it is imported (the path is fixed at import)."""
    for i, v in enumerate(sys.argv):
        if v == "--lib" and i + 1 < len(sys.argv):
            os.environ["DG_LIB_OVERRIDE"] = os.path.abspath(sys.argv[i + 1])
        elif v.startswith("--lib="):
            os.environ["DG_LIB_OVERRIDE"] = os.path.abspath(v[6:])


_lib_arg()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from downgan_amd import _lib, histograms, increments  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402


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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:16]


def torch_increments(y, spec):
    """The counts of the interior bins with stock ops: y fp32 [T, nout, H, W] (the speed already appended)."""
    out = []
    for j in range(spec.nout):
        for d in (0, 1):
            for l, r in enumerate(spec.lags):
                diff = y[:, j, :, r:] - y[:, j, :, :-r] if d == 0 else y[:, j, r:, :] - y[:, j, :-r, :]
                R = float(spec.ranges[j, l])
                out.append(torch.histc(diff, bins=spec.nbins, min=-R, max=R))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--lib", default=None, help="an A/B build of the library (sets DG_LIB_OVERRIDE)")
    ap.add_argument("--label", default="tiled", help="names the library build in the record")
    ap.add_argument("--no-torch", action="store_true", help="skip the stock-ops comparison (A/B runs)")
    ap.add_argument("--out", default=None, help="also write the record (indented JSON) to this file")
    ap.add_argument("--merge", action="store_true", help="append this run to the runs of an existing --out file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    B, C, N = a.B, 2, 1024
    ispec, hspec = increments.IncrementSpec.zscore(C), histograms.HistSpec.zscore(C)
    run = {"label": a.label, "lib": os.path.basename(_lib.LIB_PATH), "lib_sha16": sha(_lib.LIB_PATH),
           "increments_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "increments.hip")), "B": B, "C": C, "N": N,
           "lags": list(ispec.lags), "nbins": ispec.nbins, "hist_bins": hspec.bins, "reps": a.reps, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def make(case, lname):
        if lname == "nhwc_bf16_padded":
            x = torch.empty(B, N, N, 16, dtype=torch.bfloat16, device=dev)
            x.copy_(torch.randn(B, N, N, 16, generator=g, device=dev)) if case == "gauss" else x.fill_(1.25)
            return x, {"nhwc": True, "channels": C}
        x = torch.randn(B, C, N, N, generator=g, device=dev) if case == "gauss" else torch.full((B, C, N, N), 1.25, device=dev)
        return x, {}
    for case in ("gauss", "const"):
        for lname in ("nhwc_bf16_padded", "nchw_f32"):
            x, kw = make(case, lname)
            acc = increments.Increments(ispec, dev, ops=ops)
            h = histograms.ValueHistogram(hspec, dev, ops=ops)
            ti = timed(lambda: acc.add(x, **kw), a.reps)
            th = timed(lambda: h.add(x, **kw), a.reps)
            need = B * C * N * N * x.element_size()                       # the values read, once
            stored = x.numel() * x.element_size()                         # the tensor as stored (padded channels included)
            r = {"case": case, "layout": lname, "shape": list(x.shape), "bytes_needed": need, "bytes_stored": stored,
                 "incr_ms": ti[0] * 1e3, "incr_ms_min_max": [ti[1] * 1e3, ti[2] * 1e3],
                 "hist_ms": th[0] * 1e3, "hist_ms_min_max": [th[1] * 1e3, th[2] * 1e3], "incr_over_hist": ti[0] / th[0],
                 "increments_per_s": float(acc.result().finite.sum()) / (a.reps + 1) / ti[0]}
            if case == "gauss" and lname == "nchw_f32" and not a.no_torch:
                y = torch.cat([x, torch.sqrt(x[:, :1] * x[:, :1] + x[:, 1:2] * x[:, 1:2])], dim=1)
                tt = timed(lambda: torch_increments(y, ispec), a.reps)
                r.update(torch_ms=tt[0] * 1e3, torch_ms_min_max=[tt[1] * 1e3, tt[2] * 1e3], torch_over_incr=tt[0] / ti[0])
                del y
            print(json.dumps(r), flush=True)
            run["cases"].append(r)
            del x, acc, h
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
