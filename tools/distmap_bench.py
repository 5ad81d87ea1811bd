"""Times the distance maps (csrc/distmap.hip, downgan_amd.distmap.Distances.add) on one GPU and writes one JSON record.

Cases: batch 32, C = 2 channels + their speed, 2 thresholds (12 planes per field pair), NCHW fp32, at 128 x 128 and 1024 x 1024,
on two inputs:
  smooth    standardised fields with spatial structure (a 5 x 5 box filter of white noise, scaled), the generated side displaced
            by 3 pixels and noised, at the z-score thresholds 1 and 2: the shape of real use
  corner    one set pixel in a corner of every plane (the opposite corner on the generated side): every pixel of every row scans
            to the row's end, the worst case of the outward scan
Each case records: ms of the device work alone (one dg_distmap call over the whole batch into records and rings, device events,
warmed up, median of --reps), the same with the d2 output, ms of ``Distances.add`` (host clock: the calls under the workspace
cap, the read-back of the records and the pooling on the host), the bytes of workspace of the whole batch, and on the masks of
the first pair the time of the host reference dg_distmap_host (not on the 1024 x 1024 corner case, where it needs minutes) and
of scipy.ndimage.distance_transform_edt (the transform only; where scipy imports).  The share of one TrainEngine.metrics_pass at
configs[1] (32 fields of 1024 x 1024) without the hook is ``ms_add`` of the 1024 x 1024 cases over that pass, timed in the same
process (--no-metrics-pass skips it).

Usage: python tools/distmap_bench.py [--reps 5] [--out profiles/distmap_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from downgan_amd import _lib, distmap  # noqa: E402
from downgan_amd.histograms import _descriptor  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import metrics_pass_s, sha, timed  # noqa: E402

C, B = 2, 32
GRIDS = (128, 1024)
INPUTS = ("smooth", "corner")


def make(kind, N, dev):
    g = torch.Generator(device=dev).manual_seed(N)
    if kind == "smooth":
        real = torch.nn.functional.avg_pool2d(torch.randn(B, C, N, N, generator=g, device=dev), 5, 1, 2) * 5.0
        fake = torch.roll(real, 3, dims=3) + 0.3 * torch.randn(B, C, N, N, generator=g, device=dev)
    else:
        real, fake = (torch.full((B, C, N, N), -3.0, device=dev) for _ in range(2))
        real[:, :, 0, 0] = 3.0
        fake[:, :, N - 1, N - 1] = 3.0
    return real.contiguous(), fake.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-metrics-pass", action="store_true")
    ap.add_argument("--no-host", action="store_true", help="skip dg_distmap_host and scipy")
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    spec = distmap.DistSpec.zscore(C)
    s = spec.struct()
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "distmap_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "distmap.hip")), "C": C, "nout": spec.nout,
           "thresholds": spec.K, "cutoff": spec.cutoff, "nring": spec.nring, "pairs": B, "planes_per_pair": 2 * spec.nout * spec.K,
           "cases": []}
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for N in GRIDS:
        for kind in INPUTS:
            real, fake = make(kind, N, dev)
            ka, fa = _descriptor(ops, real, False, C)
            kb, fb = _descriptor(ops, fake, False, C)
            records = torch.empty(B, spec.nout, spec.K, distmap.COLS, dtype=torch.int64, device=dev)
            rings = torch.zeros(spec.nout, spec.K, 2, spec.nring + 2, dtype=torch.int64, device=dev)
            t_dev = timed(lambda: ops.distmap(fa, fb, N, N, s, records=records, rings=rings), a.reps)
            d2 = torch.empty(B, 2, spec.nout, spec.K, N * N, dtype=torch.int32, device=dev)
            t_d2 = timed(lambda: ops.distmap(fa, fb, N, N, s, records=records, rings=rings, d2=d2), a.reps)
            del d2
            acc = distmap.Distances(spec, N, N, device=dev, ops=ops)
            acc.add(real, fake)                                      # warm
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                acc.add(real, fake)
                ts.append(time.perf_counter() - t0)
            t_add = float(np.median(ts))
            res = acc.result()
            r = {"case": f"{kind}_{N}", "grid": N, "ms_device": t_dev * 1e3, "ms_device_with_d2": t_d2 * 1e3, "ms_add": t_add * 1e3,
                 "calls_per_add": acc.calls // (1 + a.reps), "ns_per_pixel_plane": t_dev * 1e9 / (B * 2 * spec.nout * spec.K * N * N),
                 "ws_bytes": ops.distmap_ws_bytes(fa, N, N, s), "med_fake_to_real_px": res.summary()["med_fake_to_real"]}
            if not a.no_host:
                xa, xb = real[0].cpu().numpy(), fake[0].cpu().numpy()
                if kind == "smooth" or N <= 128:                     # the host reference needs minutes on the 1024 x 1024 corner case
                    t0 = time.perf_counter()
                    distmap.host_distmap(spec, xa, xb)
                    r["ms_host_one_pair"] = (time.perf_counter() - t0) * 1e3
                if ndimage is not None:
                    masks = []
                    for x in (xa, xb):
                        for y in (x[0], x[1], np.sqrt(x[0] * x[0] + x[1] * x[1])):
                            masks += [y > 1.0, y > 2.0]
                    t0 = time.perf_counter()
                    for m in masks:
                        if m.any():
                            ndimage.distance_transform_edt(~m)
                    r["ms_scipy_edt_one_pair"] = (time.perf_counter() - t0) * 1e3
            print(json.dumps(r), flush=True)
            rec["cases"].append(r)
            del acc, real, fake, ka, kb, records, rings
            torch.cuda.empty_cache()
    if not a.no_metrics_pass:
        mp = metrics_pass_s(max(3, a.reps // 2))
        rec["metrics_pass_cfg2_ms"] = mp * 1e3
        for r in rec["cases"]:
            if r["grid"] == 1024:
                r["share_of_metrics_pass"] = r["ms_add"] / (mp * 1e3)
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
