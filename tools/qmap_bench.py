"""Times empirical quantile mapping (csrc/qmap.hip: downgan_amd.qmap.QuantileMap.apply and the fit kernel behind
QuantileMap.fit) on one GPU and prints one JSON record.

Cases (C = 2 channels + their speed, HistSpec.zscore(2, bins, lim=6), T = 32 fields per apply):
  nchw_f32_<N>            [32, 2, N, N] fp32
  nhwc_bf16_padded_<N>    the generator's output: [32, N, N, 16] bf16, the 2 leading channels read (one 16-byte load per pixel)
for N in {128, 1024} and bins in --bins (default 64).  At N = 128 the pixels alone do not fill the chip and the fields are cut into
slices over the workgroups.  Each case records, as device events, warmed up, the median of --reps with the GPU otherwise idle:
  apply_ms, apply_GBps     the bytes moved are the fields read (every byte of a padded pixel counts: the load brings it), the nodes
                           read once and the output written
  fit_ms, fit_GBps         the table read once and the nodes written
  copy_*_GBps              THE YARDSTICK, measured in the same run on the same card: a device-to-device copy that moves the same
                           number of bytes (half of them read, half written), for apply and for fit
  torch_apply_ms           for reference, a plain torch formulation of the same map on the same device: transform, row, ``gather`` of
                           two nodes, lerp (its result is compared with the kernel's before anything is timed: the two differ by
                           roundings only, since torch does not keep the order of operations)
and the ratios apply / copy and fit / copy.

Usage: python tools/qmap_bench.py [--reps 10] [--bins 64] [--sizes 128 1024] [--out record.json]
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

from downgan_amd import _lib, gridhist, histograms, qmap  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import sha, timed  # noqa: E402


def torch_apply(spec, x, nodes):
    """The same map in torch: x float32 [T, C, P], nodes float32 [nout, bins + 3, P] -> float32 [T, nout, P]."""
    dev = x.device
    lo, inv_w = (torch.from_numpy(v).to(dev) for v in (spec.lo, spec.inv_w))
    y = x * torch.from_numpy(spec.scale).to(dev)[None, :, None] + torch.from_numpy(spec.offset).to(dev)[None, :, None]
    if spec.speed is not None:
        u, v = y[:, spec.speed[0]], y[:, spec.speed[1]]
        y = torch.cat([y, torch.sqrt(u * u + v * v)[:, None]], dim=1)
    t = (y - lo[None, :, None]) * inv_w[None, :, None]
    b = spec.bins
    k = t.clamp(0, b - 1).nan_to_num(0.0).to(torch.int64)
    k = torch.where(t < b, k, torch.zeros_like(k)).permute(1, 0, 2)                   # [nout, T, P]
    n0, n1 = nodes.gather(1, k).permute(1, 0, 2), nodes.gather(1, k + 1).permute(1, 0, 2)
    inner = n0 + (t - k.permute(1, 0, 2).to(torch.float32)) * (n1 - n0)
    out = torch.where(t < 0, y + nodes[None, :, b + 1], torch.where(t >= b, y + nodes[None, :, b + 2], inner))
    return torch.where(torch.isnan(t), torch.full_like(out, float("nan")), out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bins", type=int, nargs="+", default=[64])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    C, T = 2, 32
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "qmap_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "qmap.hip")), "C": C, "T": T, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def copy_rate(nbytes):
        """GB/s of a device-to-device copy that moves ``nbytes`` in all."""
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_(generator=g)
        dst = torch.empty_like(src)
        t = timed(lambda: dst.copy_(src), a.reps)
        del src, dst
        return nbytes // 8 * 8 / t / 1e9

    for N in a.sizes:
        P = N * N
        real = torch.randn(T, C, N, N, generator=g, device=dev)
        fake = 0.4 + 1.3 * torch.randn(T, C, N, N, generator=g, device=dev)
        padded = torch.zeros(T, N, N, 16, dtype=torch.bfloat16, device=dev)
        padded[..., :C] = fake.permute(0, 2, 3, 1)
        for bins in a.bins:
            spec = histograms.HistSpec.zscore(C, bins=bins, lim=6.0)
            maps = gridhist.gridhist(real, fake, spec=spec, ops=ops)
            m = qmap.QuantileMap.fit(maps, ops=ops)
            nodes = torch.empty_like(m.nodes)
            table_bytes, node_bytes = maps.counts.numel() * 4, m.nodes.numel() * 4
            t_fit = timed(lambda: ops.qmap_fit(maps.counts, spec.lo, spec.width(), nodes), a.reps)
            fit_bytes = table_bytes + node_bytes
            copy_fit = copy_rate(fit_bytes)
            for layout, x, kw in (("nchw_f32", fake, {}), ("nhwc_bf16_padded", padded, {"nhwc": True, "channels": C})):
                out = torch.empty(T, spec.nout, N, N, dtype=torch.float32, device=dev)
                m.apply(x, out=out, **kw)
                seen = (x if layout == "nchw_f32" else x[..., :C].permute(0, 3, 1, 2).float()).reshape(T, C, P).contiguous()
                ref = torch_apply(spec, seen, m.nodes)
                diff = float((ref - out.view(T, spec.nout, P)).abs().nan_to_num(0.0).max())
                t_apply = timed(lambda: m.apply(x, out=out, **kw), a.reps)
                t_torch = timed(lambda: torch_apply(spec, seen, m.nodes), max(3, a.reps // 3))
                del ref
                apply_bytes = x.numel() * x.element_size() + node_bytes + out.numel() * 4
                copy_apply = copy_rate(apply_bytes)
                r = {"case": f"{layout}_{N}", "bins": bins, "shape": list(x.shape), "dtype": str(x.dtype).replace("torch.", ""),
                     "apply_bytes": apply_bytes, "fit_bytes": fit_bytes, "max_abs_diff_to_torch": diff,
                     "apply_ms": t_apply * 1e3, "apply_GBps": apply_bytes / t_apply / 1e9, "copy_apply_GBps": copy_apply,
                     "apply_over_copy": apply_bytes / t_apply / 1e9 / copy_apply,
                     "fit_ms": t_fit * 1e3, "fit_GBps": fit_bytes / t_fit / 1e9, "copy_fit_GBps": copy_fit,
                     "fit_over_copy": fit_bytes / t_fit / 1e9 / copy_fit,
                     "torch_apply_ms": t_torch * 1e3, "torch_over_hip": t_torch / t_apply}
                print(json.dumps(r), flush=True)
                rec["cases"].append(r)
                del out, seen
                torch.cuda.empty_cache()
            del maps, m, nodes
            torch.cuda.empty_cache()
        del real, fake, padded
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            json.dump(rec, fo, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
