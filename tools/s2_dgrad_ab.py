#!/usr/bin/env python3
"""A/B of the two stride-2 data-gradient kernels of the critic's 128 -> 128 channel layer (features.2) in one process:
the weight-stationary streaming kernel (csrc/conv_s2dgrad.hip) against the merged halo launch (conv_halo.hip, SEG),
switched with dg_set_s2_dgrad_stream, in alternating pairs on random data, both epilogues of the train step.
Prints one JSON document: per run ms, TFLOP/s and algorithmic bytes/s; per epilogue whether the results are bit-equal."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from downgan_amd.ops import Conv, HipOps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="", help="'stream' or 'seg': run one arm only (counter passes)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    o = HipOps("bf16")
    N, H = args.batch, args.size
    cv = Conv(N, H, H, 128, 128, 2, False, net="C")
    g = torch.Generator().manual_seed(0)
    dy = torch.randn(N, H // 2, H // 2, 128, generator=g).to(torch.bfloat16).cuda()
    w = (torch.randn(128 * 9 * 128, generator=g) * 0.05).to(torch.bfloat16).cuda()
    bits = torch.randint(-32768, 32768, (N, H, H, 2, 4), generator=g, dtype=torch.int32).to(torch.int16).cuda()
    dx = o.zeros(N, H, H, 128)
    flops = o.conv_flops(cv)
    # dx written, dy read, weights, and the 1-bit masks where they are read
    alg = {"plain": 2.0 * (dx.numel() + dy.numel() + w.numel()), "mask_bits": 2.0 * (dx.numel() + dy.numel() + w.numel()) + 2.0 * bits.numel()}
    eps = {"plain": {}, "mask_bits": dict(mask_bits=bits, mask_slope=0.2)}
    arms = [("stream", 1), ("seg", 0)]
    if args.only:
        arms = [a for a in arms if a[0] == args.only]
    res = {"batch": N, "size": H, "iters": args.iters, "alg_bytes": alg, "flops": flops, "runs": [], "bit_equal": {}}

    def timed(mode, ep):
        prev = o.lib.dg_set_s2_dgrad_stream(mode)
        try:
            o.conv_dgrad(cv, dy, w, dx, **ep)
            kinds = o.lib.dg_last_conv_kernels()
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.iters):
                o.conv_dgrad(cv, dy, w, dx, **ep)
            e.record()
            torch.cuda.synchronize()
        finally:
            o.lib.dg_set_s2_dgrad_stream(prev)
        return s.elapsed_time(e) / args.iters, kinds

    for name, ep in eps.items():
        if len(arms) == 2:
            out = {}
            for arm, mode in arms:
                dx.fill_(3.0)
                timed(mode, ep)
                out[arm] = dx.clone() if N * H * H <= 1 << 24 else dx[:: max(N // 2, 1)].clone()
            res["bit_equal"][name] = bool(torch.equal(out["stream"], out["seg"]))
            del out
        for pair in range(args.pairs):
            for arm, mode in arms:
                ms, kinds = timed(mode, ep)
                res["runs"].append({"epilogue": name, "pair": pair, "arm": arm, "kernels": kinds, "ms": round(ms, 4),
                                    "tflops": round(flops / ms / 1e9, 1), "alg_tb_per_s": round(alg[name] / ms / 1e9, 3)})
                print(res["runs"][-1], flush=True)
    txt = json.dumps(res, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
