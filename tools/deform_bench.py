"""Times the field-deformation verification (csrc/deform.hip, one dg_deform call through ops.deform) on one GPU, beside dg_fss over
its default windows on the same tensors, and prints one JSON record.

Cases (C = 2 channels + their speed, F = 3 levels; batch 32; the real side [32, 2, N, N] fp32 NCHW, the generated side
[32, N, N, 16] bf16 padded NHWC of which the 2 leading channels are read), N = 128 and N = 1024.
Each case records, for both calls, ms per call (device events; every shape warmed up; the two calls alternate inside one timed
loop and the median of --reps windows of --inner calls each is reported), the workspace bytes, the ratio of the two times, and
the pixel-directions per second of the matcher (fields x output channels x 2 directions x H W over the call time).

The share of the call that the level-0 matching kernel takes is a kernel time, so it comes from a run of its own under
rocprofv3, merged into the record afterwards:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o deform -- python tools/deform_bench.py --profile 1024 --calls 5
    python tools/deform_bench.py --merge-stats DIR/.../deform_kernel_stats.csv --profile 1024 --out profiles/deform_bench.json
``static`` holds what was counted in the disassembly of the library as built (no run needed): see DESIGN.md.

Usage: python tools/deform_bench.py [--reps 7] [--inner 5] [--out profiles/deform_bench.json]
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

C, B, LEVELS = 2, 32, 3
# counted in the ISA of deform_match_kernel<unsigned char, unsigned int> (hipcc -O3 --offload-arch=gfx950 -S): one pass of the
# shift loop serves a thread's 8 pixels with 200 vector-ALU instructions and 30 LDS reads of two dwords each
STATIC = {"valu_per_shift_per_thread": 200, "lds_reads_per_shift_per_thread": 30, "pixels_per_thread": 8, "shifts": 25,
          "valu_per_pixel_direction": 200 * 25 / 8, "lds_reads_per_pixel_direction": 30 * 25 / 8,
          "separable_estimate_per_pixel_direction": 25 * 12, "vgprs": 126, "lds_bytes_per_workgroup": 26208}


def window(fn, inner):
    """Seconds per call of ``inner`` back-to-back calls between two device events."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def tensors(N, dev, g):
    """Standardised fields with some spatial structure; the generated side displaced by a few pixels and noised."""
    import torch
    real = (torch.nn.functional.avg_pool2d(torch.randn(B, C, N, N, generator=g, device=dev), 5, 1, 2) * 5.0).contiguous()
    fake32 = torch.roll(real, (3, -2), dims=(2, 3)) + 0.1 * torch.randn(B, C, N, N, generator=g, device=dev)
    fake = torch.zeros(B, N, N, 16, dtype=torch.bfloat16, device=dev)
    fake[..., :C] = fake32.permute(0, 2, 3, 1)
    return real, fake


def merge_stats(path, N, out):
    """Add the kernel shares of a rocprofv3 kernel-stats CSV (a --profile N run) to the case N of the record in ``out``."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    name = next(k for k in rows[0] if k.lower() == "name")
    total = next(k for k in rows[0] if "total" in k.lower() and "ns" in k.lower())
    ours = {r[name]: float(r[total]) for r in rows if "deform_" in r[name]}
    s = sum(ours.values())
    short = lambda n: re.search(r"deform_\w+(<[^>]*>)?", n).group(0)
    shares = {short(n): v / s for n, v in sorted(ours.items(), key=lambda kv: -kv[1])}
    level0 = sum(v for n, v in ours.items() if "deform_match_kernel<unsigned char" in n or "deform_match_kernelIh" in n) / s
    with open(out) as f:
        rec = json.load(f)
    case = next(c for c in rec["cases"] if c["N"] == N)
    case["kernel_shares"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own", "of_deform_kernel_time": shares,
                             "level0_match_share": level0}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(case["kernel_shares"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    ap.add_argument("--profile", type=int, default=None, metavar="N", help="only run --calls dg_deform calls at N x N (under a profiler)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--merge-stats", default=None, metavar="CSV", help="merge a kernel-stats CSV of a --profile N run into --out; no GPU")
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.profile, a.out)

    import numpy as np
    import torch
    from downgan_amd import _lib, deform, fss
    from downgan_amd.ops import HipOps
    from hist_bench import sha
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    dspec, fspec = deform.DeformSpec.zscore(C, levels=LEVELS), fss.FssSpec.zscore(C)
    side = 2 * dspec.D + 1
    g = torch.Generator(device=dev).manual_seed(0)

    def calls_of(N, real, fake):
        fa, fb = ops.eof_fields(real), ops.eof_fields(fake, nhwc=True, channels=C)
        disp = torch.zeros(dspec.nout, 2, side * side, dtype=torch.int64, device=dev)
        scal = torch.zeros(dspec.nout, 2, deform.NSCALARS, dtype=torch.int64, device=dev)
        fsums = torch.zeros(fspec.nout, fspec.K, fspec.S, 3, dtype=torch.int64, device=dev)
        frates = torch.zeros(fspec.nout, fspec.K, 2, dtype=torch.int64, device=dev)
        sd, sf = dspec.struct(), fspec.struct()
        run_d = lambda: ops.deform(fa, fb, N, N, sd, disp, scal)
        run_f = lambda: ops.fss(fa, fb, N, N, sf, fsums, frates)
        return fa, sd, sf, disp, scal, run_d, run_f

    if a.profile:
        real, fake = tensors(a.profile, dev, g)
        run_d = calls_of(a.profile, real, fake)[5]
        for _ in range(a.calls):
            run_d()
        torch.cuda.synchronize()
        return

    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "deform_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "deform.hip")), "C": C, "nout": dspec.nout,
           "levels": LEVELS, "max_displacement": dspec.D, "batch": B, "fss_windows": list(fspec.scales), "reps": a.reps, "inner": a.inner,
           "static": STATIC, "cases": []}
    for N in (128, 1024):
        real, fake = tensors(N, dev, g)
        fa, sd, sf, disp, scal, run_d, run_f = calls_of(N, real, fake)
        for fn in (run_d, run_f):                                        # warm up both shapes
            window(fn, 2)
        disp.zero_(); scal.zero_()
        run_d()
        torch.cuda.synchronize()
        once = (disp.clone(), scal.clone())
        disp.zero_(); scal.zero_()
        run_d()
        torch.cuda.synchronize()
        same = bool((disp == once[0]).all().item() and (scal == once[1]).all().item())     # two calls are bit-identical
        r0 = deform.DeformResult(dspec, N, N, disp.cpu().numpy().reshape(dspec.nout, 2, side, side), scal.cpu().numpy(), B)
        td, tf = [], []
        for _ in range(a.reps):                                          # alternate the two calls
            td.append(window(run_d, a.inner))
            tf.append(window(run_f, a.inner))
        pixdir = B * dspec.nout * 2 * N * N
        r = {"N": N, "real": [list(real.shape), "float32"], "fake": [list(fake.shape), "bfloat16"], "bit_identical": same,
             "modal_vector_ch0": r0.modal_vector()[0].tolist(), "explained_ch0": r0.explained()[0].tolist(), "pixel_directions": pixdir}
        for name, ts, ws in (("deform", td, ops.deform_ws_bytes(fa, N, N, sd)), ("fss_default", tf, ops.fss_ws_bytes(fa, N, N, sf))):
            t = float(np.median(ts))
            r[name] = {"ms": t * 1e3, "ms_min": min(ts) * 1e3, "ms_max": max(ts) * 1e3, "ws_bytes": ws}
        r["deform"]["pixel_directions_per_s"] = pixdir / (r["deform"]["ms"] * 1e-3)
        r["deform_over_fss"] = r["deform"]["ms"] / r["fss_default"]["ms"]
        print(json.dumps(r), flush=True)
        rec["cases"].append(r)
        del real, fake, fa
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
