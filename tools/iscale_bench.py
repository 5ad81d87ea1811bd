"""Times the intensity-scale verification (csrc/iscale.hip, one dg_iscale call through ops.iscale) on one GPU, beside dg_fss with
the single window (1,) on the same tensors, and prints one JSON record.

Cases (C = 2 channels + their speed, two thresholds per channel; batch 32; the real side [32, 2, N, N] fp32 NCHW, the generated
side [32, N, N, 16] bf16 padded NHWC of which the 2 leading channels are read), N = 128 and N = 1024.
Each case records, for both calls, ms per call (device events; every shape warmed up; the two calls alternate inside one timed
loop and the median of --reps windows of --inner calls each is reported), the bytes the call must read (every stored byte of both
series once: 8 bytes per pixel of the real side, 32 of the generated side -- 16 of them are used, but the pixels lie 32 bytes
apart, so every cache line of the store is fetched), the effective read bandwidth bytes / time, its fraction of the 6.29 TB/s a float4 copy reaches on this GPU, and the workspace bytes of
either call.  dg_fss at window 1 reads the same bytes and in addition writes and re-reads its uint32 tables.

Usage: python tools/iscale_bench.py [--reps 7] [--inner 20] [--out profiles/iscale_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from downgan_amd import _lib, fss, iscale  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import sha  # noqa: E402

COPY_RATE = 6.29e12          # bytes/s of a float4 copy on the MI355X: the stream rate the fractions refer to


def window(fn, inner):
    """Seconds per call of ``inner`` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    C, B = 2, 32
    ispec, fspec = iscale.IscaleSpec.zscore(C), fss.FssSpec.zscore(C, scales=(1,))
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "iscale_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "iscale.hip")), "C": C, "nout": ispec.nout,
           "thresholds": ispec.K, "batch": B, "copy_rate": COPY_RATE, "reps": a.reps, "inner": a.inner, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)
    for N in (128, 1024):
        # standardised fields with some spatial structure; the generated side displaced by a few pixels and noised
        real = (torch.nn.functional.avg_pool2d(torch.randn(B, C, N, N, generator=g, device=dev), 5, 1, 2) * 5.0).contiguous()
        fake32 = torch.roll(real, 3, dims=3) + 0.3 * torch.randn(B, C, N, N, generator=g, device=dev)
        fake = torch.zeros(B, N, N, 16, dtype=torch.bfloat16, device=dev)
        fake[..., :C] = fake32.permute(0, 2, 3, 1)
        del fake32
        fa, fb = ops.eof_fields(real), ops.eof_fields(fake, nhwc=True, channels=C)
        L = iscale.log_side(N, N) + 1
        isums = torch.zeros(ispec.nout, ispec.K, L, 3, dtype=torch.int64, device=dev)
        fsums = torch.zeros(fspec.nout, fspec.K, 1, 3, dtype=torch.int64, device=dev)
        frates = torch.zeros(fspec.nout, fspec.K, 2, dtype=torch.int64, device=dev)
        si, sf = ispec.struct(), fspec.struct()
        run_i = lambda: ops.iscale(fa, fb, N, N, si, isums)
        run_f = lambda: ops.fss(fa, fb, N, N, sf, fsums, frates)
        for fn in (run_i, run_f):                                        # warm up both shapes
            window(fn, 3)
        isums.zero_(); fsums.zero_(); frates.zero_()
        run_i(); run_f()
        torch.cuda.synchronize()
        same = bool((isums[:, :, 0] == fsums[:, :, 0]).all().item())     # level 0 = dg_fss's D, A, B at window 1
        ti, tf = [], []
        for _ in range(a.reps):                                          # alternate the two calls
            ti.append(window(run_i, a.inner))
            tf.append(window(run_f, a.inner))
        read = real.numel() * 4 + fake.numel() * 2                       # every stored byte of both series, once
        r = {"N": N, "real": [list(real.shape), "float32"], "fake": [list(fake.shape), "bfloat16"], "read_bytes": read,
             "level0_equals_fss": same, "levels": L}
        for name, ts, ws in (("iscale", ti, ops.iscale_ws_bytes(fa, N, N, si)), ("fss_win1", tf, ops.fss_ws_bytes(fa, N, N, sf))):
            t = float(np.median(ts))
            r[name] = {"ms": t * 1e3, "ms_min": min(ts) * 1e3, "ms_max": max(ts) * 1e3, "read_TBps": read / t / 1e12,
                       "fraction_of_copy_rate": read / t / COPY_RATE, "ws_bytes": ws}
        r["iscale_over_fss"] = r["iscale"]["ms"] / r["fss_win1"]["ms"]
        print(json.dumps(r), flush=True)
        rec["cases"].append(r)
        del real, fake, fa, fb
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
