"""Times the per-gridpoint statistics (csrc/gridstats.hip, downgan_amd.gridstats.GridStats.add) on one GPU and prints one JSON
record.

Cases (C = 2 channels + their speed, GridSpec.zscore(2): two thresholds per channel):
  nhwc_bf16_padded_1024_paired  the generator's output at BASELINE configs[1] paired with the real fields in the same layout:
                                2 x [32, 1024, 1024, 16] bf16, the 2 leading channels read (one 16-byte load per pixel)
  nchw_f32_1024_paired          2 x [32, 2, 1024, 1024] fp32 (four pixels per thread)
  resident_feed_bf16_128        the resident feed's store, one series: [4096, 128, 128, 2] bf16; P alone does not fill the
                                chip, so the fields are cut into dg_gridstats_slices(T, P) slices (the T-split path)
Each case records ms per ``add`` (device events, warmed up, median of --reps), the input bytes the statistics need (the values
read once) and the bytes stored (the tensors' footprint, padding included), the accumulator bytes read and written by one
``add`` (the T-split path adds its workspace traffic), the effective GB/s on needed, stored and stored + accumulator bytes,
and the ratio to two yardsticks timed in the same process: dg_hist over the same input tensors (one ValueHistogram.add per
series) and one TrainEngine.metrics_pass at configs[1] (--no-metrics-pass skips it).

Usage: python tools/gridstats_bench.py [--reps 10] [--out record.json]
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

from downgan_amd import _lib, gridstats, histograms  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import HBM_MEASURED, metrics_pass_s, sha, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-metrics-pass", action="store_true")
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    C, N = 2, 1024
    spec, hspec = gridstats.GridSpec.zscore(C), histograms.HistSpec.zscore(C)
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "gridstats_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "gridstats.hip")), "C": C, "nout": spec.nout,
           "thresholds": spec.K, "hbm_copy_Bps": HBM_MEASURED, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def padded(B):
        t = torch.empty(B, N, N, 16, dtype=torch.bfloat16, device=dev)
        t.copy_(torch.randn(B, N, N, 16, generator=g, device=dev))
        return t

    def cases():
        yield "nhwc_bf16_padded_1024_paired", (padded(32), padded(32)), {"nhwc": True, "channels": C}
        yield "nchw_f32_1024_paired", (torch.randn(32, C, N, N, generator=g, device=dev), torch.randn(32, C, N, N, generator=g, device=dev)), {}
        feed = torch.empty(4096, 128, 128, C, dtype=torch.bfloat16, device=dev)
        feed.copy_(torch.randn(4096, 128, 128, C, generator=g, device=dev))
        yield "resident_feed_bf16_128", (feed,), {"nhwc": True}

    for name, xs, kw in cases():
        x = xs[0]
        paired = len(xs) == 2
        T = x.shape[0]
        H, W = (x.shape[1], x.shape[2]) if kw.get("nhwc") else (x.shape[2], x.shape[3])
        P = H * W
        acc = gridstats.GridStats(spec, H, W, paired=paired, device=dev, ops=ops)
        t = timed(lambda: acc.add(*xs, **kw), a.reps)
        hists = [histograms.ValueHistogram(hspec, dev, ops=ops) for _ in xs]
        th = timed(lambda: [h.add(v, **kw) for h, v in zip(hists, xs)], a.reps)
        need = len(xs) * T * C * P * x.element_size()                # the values the statistics need, read once
        stored = sum(v.numel() * v.element_size() for v in xs)       # the tensors as stored (padded channels included)
        state = sum(b.numel() * b.element_size() for b in (acc._sums, acc._ext, acc._cnt))
        S = _lib.lib().dg_gridstats_slices(T, P)
        # one slice: the accumulators are read and written once; S slices: S partial states written and read, then the same
        acc_read, acc_written = (state, state) if S == 1 else (state * (S + 1), state * (S + 1))
        moved = stored + acc_read + acc_written
        r = {"case": name, "shape": list(x.shape), "series": len(xs), "dtype": str(x.dtype).replace("torch.", ""), "slices": S,
             "ms": t * 1e3, "bytes_needed": need, "bytes_stored": stored, "acc_bytes_read": acc_read,
             "acc_bytes_written": acc_written, "GBps_needed": need / t / 1e9, "GBps_stored": stored / t / 1e9,
             "GBps_moved": moved / t / 1e9, "hbm_frac_moved": moved / t / HBM_MEASURED,
             "ws_bytes": ops.gridstats_ws_bytes(ops.eof_fields(x, **kw), paired, spec.struct()),
             "dg_hist_same_tensors_ms": th * 1e3, "ratio_to_dg_hist": t / th}
        print(json.dumps(r), flush=True)
        rec["cases"].append(r)
        del acc, hists, xs, x
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
