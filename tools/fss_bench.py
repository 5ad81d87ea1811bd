"""Times the fractions skill score (csrc/fss.hip, downgan_amd.fss.FractionsSkill.add) on one GPU and prints one JSON record.

Cases (C = 2 channels + their speed, FssSpec.zscore(2): two thresholds per channel, the eight default window sides 1 .. 129):
  nhwc_bf16_padded_1024  the generator's output at BASELINE configs[1] paired with the real fields in the same layout:
                         2 x [32, 1024, 1024, 16] bf16, the 2 leading channels read (one 16-byte load per pixel)
  nchw_f32_1024          2 x [32, 2, 1024, 1024] fp32
Each case records ms per ``add`` (device events, warmed up, median of --reps), the number of dg_fss calls the batch is cut into
under fss.WS_CAP, the workspace bytes of one call, the table bytes written per batch (one uint32 summed-area table per field,
series, output channel and threshold; written by the row pass, read and written by the column pass), the corner reads the
window pass issues (8 per pixel, table pair and scale), and the ratio to one TrainEngine.metrics_pass at configs[1] without the
hook, timed in the same process (--no-metrics-pass skips it).

Usage: python tools/fss_bench.py [--reps 5] [--out profiles/fss_bench_first.json]
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

from downgan_amd import _lib, fss  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import metrics_pass_s, sha, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-metrics-pass", action="store_true")
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    C, N, B = 2, 1024, 32
    spec = fss.FssSpec.zscore(C)
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "fss_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "fss.hip")), "C": C, "nout": spec.nout,
           "thresholds": spec.K, "scales": list(spec.scales), "ws_cap": fss.WS_CAP, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def padded(x):
        t = torch.zeros(B, N, N, 16, dtype=torch.bfloat16, device=dev)
        t[..., :C] = x.permute(0, 2, 3, 1)
        return t

    # standardised fields with some spatial structure; the generated side displaced by a few pixels and noised
    real = torch.nn.functional.avg_pool2d(torch.randn(B, C, N, N, generator=g, device=dev), 5, 1, 2) * 5.0
    fake = torch.roll(real, 3, dims=3) + 0.3 * torch.randn(B, C, N, N, generator=g, device=dev)

    def cases():
        yield "nhwc_bf16_padded_1024", (padded(real), padded(fake)), {"nhwc": True, "channels": C}
        yield "nchw_f32_1024", (real, fake), {}

    for name, xs, kw in cases():
        acc = fss.FractionsSkill(spec, N, N, device=dev, ops=ops)
        t = timed(lambda: acc.add(*xs, **kw), a.reps)
        f1 = ops.eof_fields(xs[0][:1], **kw)
        ws1 = ops.fss_ws_bytes(f1, N, N, spec.struct())
        tc = max(1, min(B, fss.WS_CAP // ws1))
        planes = B * 2 * spec.nout * spec.K
        res = acc.result()
        r = {"case": name, "shape": list(xs[0].shape), "dtype": str(xs[0].dtype).replace("torch.", ""), "ms": t * 1e3,
             "calls_per_add": -(-B // tc), "fields_per_call": tc, "ws_bytes_per_call": ops.fss_ws_bytes(ops.eof_fields(xs[0][:tc], **kw), N, N, spec.struct()),
             "table_bytes": planes * N * N * 4, "corner_reads": planes * N * N * spec.S * 4,
             "ns_per_pixel_plane_scale": t * 1e9 / (planes / 2 * N * N * spec.S),
             "fss_ch0": res.fss()[0].tolist(), "drains": acc.drains}
        print(json.dumps(r), flush=True)
        rec["cases"].append(r)
        del acc, xs
        torch.cuda.empty_cache()
    del real, fake
    torch.cuda.empty_cache()
    if not a.no_metrics_pass:
        mp = metrics_pass_s(max(3, a.reps // 2))
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
