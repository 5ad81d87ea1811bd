"""Times the per-gridpoint histograms (csrc/gridhist.hip: downgan_amd.gridhist.GridHist.add and the scan kernel behind
GridHistMaps) on one GPU and prints one JSON record.

Cases (C = 2 channels + their speed, HistSpec.zscore(2, bins, lim=6), paired, T = 32 fields per add):
  nchw_f32_<N>            2 x [32, 2, N, N] fp32 (four pixels per thread)
  nhwc_bf16_padded_<N>    the generator's output paired with the real fields in the same layout: 2 x [32, N, N, 16] bf16, the 2
                          leading channels read (one 16-byte load per pixel)
for N in {128, 1024} and bins in {64, 256} (--bins).  At N = 128 the pixels alone do not fill the chip and the fields are cut
into slices over the workgroups.  Each case records ms per ``add`` and ms per scan (Q = 3) as device events, warmed up, the
median of --reps with the GPU otherwise idle, the table bytes, the number of 4-byte atomic adds an ``add`` would issue without
run combining (T * nout * 2 * P, an upper bound) and, as the baseline, a torch implementation of the same table on the same
device: transform, bucketise by the same bin rule in fp32, ``scatter_add_`` into [.., P].  The baseline's table is compared with
the kernel's before anything is timed.  Every case is timed on three kinds of data (--data), all of unit variance:
  iid        independent in t and in space: no runs of equal rows, and the lanes of a wave fall into unrelated rows (the worst case)
  smooth_xy  independent in t, smooth in space (white noise under a 15 x 15 box mean): what the trainer's hook sees, shuffled
             batches of smooth fields -- no runs, but neighbouring lanes share rows
  ar1_t      independent in space, an AR(1) series of coefficient 0.95 in t per pixel: consecutive fields of an ordered series,
             where runs of equal rows occur

Usage: python tools/gridhist_bench.py [--reps 10] [--bins 64 256] [--sizes 128 1024] [--data iid smooth_xy ar1_t] [--out record.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from downgan_amd import _lib, gridhist, histograms  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import sha, timed  # noqa: E402


def torch_table(spec, xs, counts):
    """The same table in torch: xs = (real, fake) as float32 [T, C, P] views; counts int32 [nout, 2, bins + 3, P] +=."""
    dev = counts.device
    lo, inv_w = (torch.from_numpy(v).to(dev) for v in (spec.lo, spec.inv_w))
    ones = None
    for s, x in enumerate(xs):
        y = x * torch.from_numpy(spec.scale).to(dev)[None, :, None] + torch.from_numpy(spec.offset).to(dev)[None, :, None]
        if spec.speed is not None:
            u, v = y[:, spec.speed[0]], y[:, spec.speed[1]]
            y = torch.cat([y, torch.sqrt(u * u + v * v)[:, None]], dim=1)
        t = (y - lo[None, :, None]) * inv_w[None, :, None]
        row = torch.where(t < 0, 0, torch.where(t >= spec.bins, spec.bins + 1, 1 + t.clamp(0, spec.bins - 1).to(torch.int64)))
        row = torch.where(torch.isnan(t), spec.bins + 2, row)        # [T, nout, P]
        if ones is None:
            ones = torch.ones_like(row, dtype=torch.int32)
        counts[:, s].scatter_add_(1, row.permute(1, 0, 2), ones.permute(1, 0, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bins", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--data", nargs="+", default=["iid", "smooth_xy", "ar1_t"], choices=["iid", "smooth_xy", "ar1_t"])
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    C, T = 2, 32
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "gridhist_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "gridhist.hip")), "C": C, "T": T, "Q": 3, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def series(N, kind):
        """[T, C, N, N] fp32 of unit variance (the kinds of the module docstring)."""
        x = torch.randn(T, C, N, N, generator=g, device=dev)
        if kind == "smooth_xy":
            x = torch.nn.functional.avg_pool2d(x, 15, stride=1, padding=7, count_include_pad=False)
            x = x / x.std()
        elif kind == "ar1_t":
            for t in range(1, T):
                x[t] = 0.95 * x[t - 1] + (1 - 0.95 ** 2) ** 0.5 * x[t]
        return x.contiguous()

    def padded(x):
        t = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 16, dtype=torch.bfloat16, device=dev)
        t[..., :C] = x.permute(0, 2, 3, 1)
        return t

    for N, kind in ((N, kind) for N in a.sizes for kind in a.data):
        real, fake = series(N, kind), series(N, kind)
        P = N * N
        for layout in ("nchw_f32", "nhwc_bf16_padded"):
            xs, kw = ((real, fake), {}) if layout == "nchw_f32" else ((padded(real), padded(fake)), {"nhwc": True, "channels": C})
            seen = [v.reshape(T, C, P) if layout == "nchw_f32" else v[..., :C].permute(0, 3, 1, 2).float().reshape(T, C, P) for v in xs]
            for bins in a.bins:
                spec = histograms.HistSpec.zscore(C, bins=bins, lim=6.0)
                acc = gridhist.GridHist(spec, N, N, paired=True, device=dev, ops=ops)
                acc.add(*xs, **kw)
                ref = torch.zeros_like(acc.counts)
                torch_table(spec, seen, ref)
                same = bool(torch.equal(ref, acc.counts))
                t_add = timed(lambda: acc.add(*xs, **kw), a.reps)
                t_torch = timed(lambda: torch_table(spec, seen, ref), max(3, a.reps // 3))
                del ref
                maps = acc.result()
                c, qs = maps.counts, (0.5, 0.95, 0.99)
                ranks = torch.empty(spec.nout, 2, 3, 3, P, dtype=torch.int32, device=dev)
                dist = torch.empty(spec.nout, 2, P, dtype=torch.int64, device=dev)
                t_scan = timed(lambda: ops.gridhist_scan(c, qs, ranks, dist), a.reps)
                r = {"case": f"{layout}_{N}", "data": kind, "bins": bins, "shape": list(xs[0].shape), "dtype": str(xs[0].dtype).replace("torch.", ""),
                     "table_bytes": acc.nbytes, "adds_upper_bound": T * spec.nout * 2 * P, "matches_torch": same,
                     "add_ms": t_add * 1e3, "scan_ms": t_scan * 1e3, "torch_add_ms": t_torch * 1e3, "torch_over_hip": t_torch / t_add,
                     "add_Gadds_per_s_upper": T * spec.nout * 2 * P / t_add / 1e9, "scan_GBps_table_read_twice": 2 * acc.nbytes / t_scan / 1e9}
                print(json.dumps(r), flush=True)
                rec["cases"].append(r)
                del acc, maps, c, ranks, dist
                torch.cuda.empty_cache()
            del xs, seen
        del real, fake
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
