"""Times the exceedance objects (csrc/objects.hip, downgan_amd.objects.Objects.add) on one GPU and writes one JSON record.

Cases: C = 2 channels + their speed, 2 thresholds (12 planes per field pair), connectivity 8, NCHW fp32, at 128 x 128 (32 field
pairs) and 1024 x 1024 (4 field pairs), on three inputs:
  smooth    standardised fields with spatial structure (a 5 x 5 box filter of white noise, scaled), the generated side displaced
            by 3 pixels and noised: the shape of real use
  noise     white noise thresholded at density 0.59, the site-percolation threshold of the square lattice: the largest and most
            tortuous clusters, the worst case of the union-find
  all_set   every pixel above every threshold: one object per plane, every atomic of the statistics pass aimed at one record
            (the contention case the lane-combining of that pass exists for)
Each case records, per field pair: ms of the device work alone (one dg_objects call with a table that is large enough, device
events, warmed up, median of --reps), ms of ``Objects.add`` (host clock: the call, the read-back of the count, the sort, the copy
of the records and the pooling on the host), the number of objects, and on the same inputs the time of the host reference
dg_objects_host and of scipy.ndimage.label over the same 12 masks (labelling only, no statistics; where scipy imports).  The ratio
to one TrainEngine.metrics_pass at configs[1] (32 fields of 1024 x 1024) without the hook is taken per field, timed in the same
process (--no-metrics-pass skips it).

The split per kernel comes from runs of their own under the profiler, one per case:
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/objects_bench.py --trace smooth_1024
and is merged into a record written earlier with --merge <record> --stats smooth_1024=<dir> (repeatable).

Usage: python tools/objects_bench.py [--reps 5] [--out profiles/objects_bench.json]
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from downgan_amd import _lib, objects  # noqa: E402
from downgan_amd.histograms import _descriptor  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import metrics_pass_s, sha, timed  # noqa: E402

C = 2
GRIDS = {128: 32, 1024: 4}                                          # side -> field pairs per batch
INPUTS = ("smooth", "noise", "all_set")


def make(kind, B, N, dev):
    g = torch.Generator(device=dev).manual_seed(N)
    if kind == "smooth":
        real = torch.nn.functional.avg_pool2d(torch.randn(B, C, N, N, generator=g, device=dev), 5, 1, 2) * 5.0
        fake = torch.roll(real, 3, dims=3) + 0.3 * torch.randn(B, C, N, N, generator=g, device=dev)
    elif kind == "noise":
        real, fake = (1.59 - torch.rand(B, C, N, N, generator=g, device=dev) for _ in range(2))   # y > 1 on 59 % of the pixels
    else:
        real, fake = (torch.full((B, C, N, N), 3.0, device=dev) for _ in range(2))
    return real.contiguous(), fake.contiguous()


def device_call(ops, spec, real, fake, N):
    """A closure that runs one dg_objects call over the whole batch into a table that is large enough, and the object count."""
    ka, fa = _descriptor(ops, real, False, C)
    kb, fb = _descriptor(ops, fake, False, C)
    s = spec.struct()
    count = torch.zeros(1, dtype=torch.int64, device=real.device)
    per_plane = torch.zeros(fa.T * 2 * spec.nout * spec.K, dtype=torch.int64, device=real.device)
    ops.objects_raw(fa, fb, N, N, s, torch.empty(0, 12, dtype=torch.int64, device=real.device), count, per_plane)
    n = int(count)
    table = torch.empty(max(n, 1), 12, dtype=torch.int64, device=real.device)
    keep = (ka, kb)
    return (lambda: ops.objects_raw(fa, fb, N, N, s, table, count, per_plane)), n, keep


def kernel_split(directory):
    """{kernel: {"calls", "avg_us", "total_us"}} of the obj_* kernels in a rocprofv3 --stats directory."""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if "obj_" not in name:
                    continue
                short = name[name.index("obj_"):].split("(")[0]
                e = out.setdefault(short, {"calls": 0, "total_us": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_us"] += float(row["TotalDurationNs"]) * 1e-3
    for e in out.values():
        e["avg_us"] = e["total_us"] / max(1, e["calls"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-metrics-pass", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip dg_objects_host and scipy")
    ap.add_argument("--trace", default=None, help="CASE (e.g. smooth_1024): run only that case's device call, for a profiler run")
    ap.add_argument("--stats", action="append", default=[], help="CASE=DIR: merge the kernel split of a profiler run")
    ap.add_argument("--merge", default=None, help="a record written earlier: only add the --stats splits to it (no GPU work)")
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    if a.merge:
        with open(a.merge) as f:
            rec = json.load(f)
        for item in a.stats:
            case, directory = item.split("=", 1)
            rec.setdefault("kernel_split", {})[case] = kernel_split(directory)
        with open(a.out or a.merge, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out or a.merge)
        return
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    spec = objects.ObjectSpec.zscore(C)
    if a.trace:
        kind, N = a.trace.rsplit("_", 1)
        N = int(N)
        real, fake = make(kind, GRIDS[N], N, dev)
        call, n, keep = device_call(ops, spec, real, fake, N)
        for _ in range(1 + a.reps):
            call()
        torch.cuda.synchronize()
        print(json.dumps({"traced": a.trace, "objects": n, "calls": 2 + a.reps}))
        return
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "objects_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "objects.hip")), "C": C, "nout": spec.nout,
           "thresholds": spec.K, "connectivity": spec.connectivity, "planes_per_pair": 2 * spec.nout * spec.K, "cases": []}
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for N, B in GRIDS.items():
        for kind in INPUTS:
            real, fake = make(kind, B, N, dev)
            call, n, keep = device_call(ops, spec, real, fake, N)
            t_dev = timed(call, a.reps)
            acc = objects.Objects(spec, N, N, device=dev, ops=ops)
            acc.add(real, fake)                                      # warm: the table capacity the ops object remembers
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                acc.add(real, fake)
                ts.append(time.perf_counter() - t0)
            t_add = float(np.median(ts))
            r = {"case": f"{kind}_{N}", "grid": N, "pairs": B, "objects_per_pair": n / B, "ms_per_pair_device": t_dev * 1e3 / B,
                 "ms_per_pair_add": t_add * 1e3 / B, "ns_per_pixel_plane": t_dev * 1e9 / (B * 2 * spec.nout * spec.K * N * N),
                 "ws_bytes": ops.objects_ws_bytes(ops.eof_fields(real), N, N, spec.struct())}
            if not a.no_host:
                xa, xb = real[0].cpu().numpy(), fake[0].cpu().numpy()
                t0 = time.perf_counter()
                _, hn, _ = objects.host_objects(spec, xa, xb, capacity=max(1, 2 * n // B + 1024))
                r["ms_per_pair_host"] = (time.perf_counter() - t0) * 1e3
                r["host_objects_pair0"] = hn
                if ndimage is not None:
                    masks = []
                    for x in (xa, xb):
                        for y in (x[0], x[1], np.sqrt(x[0] * x[0] + x[1] * x[1])):
                            masks += [y > 1.0, y > 2.0]
                    t0 = time.perf_counter()
                    found = sum(ndimage.label(m, structure=np.ones((3, 3), int))[1] for m in masks)
                    r["ms_per_pair_scipy_label"] = (time.perf_counter() - t0) * 1e3
                    r["scipy_objects_pair0"] = found
            print(json.dumps(r), flush=True)
            rec["cases"].append(r)
            del acc, call, keep, real, fake
            torch.cuda.empty_cache()
    if not a.no_metrics_pass:
        mp = metrics_pass_s(max(3, a.reps // 2))
        rec["metrics_pass_cfg2_ms"] = mp * 1e3
        rec["metrics_pass_cfg2_ms_per_field"] = mp * 1e3 / 32
        for r in rec["cases"]:
            if r["grid"] == 1024:
                r["ratio_to_metrics_pass_per_field"] = r["ms_per_pair_add"] / (mp * 1e3 / 32)
    for item in a.stats:
        case, directory = item.split("=", 1)
        rec.setdefault("kernel_split", {})[case] = kernel_split(directory)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
