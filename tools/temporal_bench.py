"""Times the temporal diagnostics (csrc/temporal.hip: downgan_amd.temporal.Temporal.add) on one GPU and prints one JSON record.

Cases (C = 2 channels + their speed, TemporalSpec.zscore(2): 4 thresholds, lags (1, 2, 3, 6), 128 ramp bins; paired, T = 32 fields
per add, an AR(1) series of coefficient 0.9 in t per pixel so that spells last):
  nchw_f32_<N>            2 x [32, 2, N, N] fp32 (four pixels per thread at N = 1024, one at N = 128)
  nhwc_bf16_padded_<N>    the generator's output paired with the real fields in the same layout: 2 x [32, N, N, 16] bf16, the 2
                          leading channels read (one 16-byte load per pixel and output channel)
for N in {128, 1024}.  The fields of a call are never cut into time slices (the chunking contract), so at N = 128 the launch has
16384 pixels x 3 output channels per series: few waves, bound by latency.  Each case records ms per ``add`` as device events,
warmed up, the median of --reps with the GPU otherwise idle; ``input_bytes`` is the floor -- every byte of the channels read,
once -- and ``input_GBps`` the rate against it; the kernel reads every field 1 + nlag times (the partners of the ramps come from the
caches) and reads and writes ``state_bytes`` of per-pixel state once per call.  The baseline is a straightforward torch
implementation of the same definition on the same device (a Python loop over t of elementwise, bincount and index ops, the
history kept as a tensor); its integers are compared with the kernel's before anything is timed.

Usage: python tools/temporal_bench.py [--reps 10] [--sizes 128 1024] [--out profiles/temporal_bench.json]
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

from downgan_amd import _lib, temporal  # noqa: E402
from downgan_amd.ops import HipOps  # noqa: E402
from hist_bench import sha, timed  # noqa: E402


class TorchTemporal:
    """The definition in torch for S series of [T, C, P] float32 views: the same arrays as ``temporal.Temporal`` plus the last R
    output values as a tensor."""

    def __init__(self, spec, S, P, dev):
        tdt = {"int32": torch.int32, "int64": torch.int64, "float32": torch.float32, "float64": torch.float64}
        name = lambda dt: np.dtype(dt).name
        self.spec, self.t0 = spec, 0
        self.a = {k: torch.zeros(shape, dtype=tdt[name(dt)], device=dev)
                  for k, (shape, dt) in spec.shapes(S, P).items()}
        self.past = torch.full((S, spec.R, spec.nout, P), float("nan"), device=dev)      # y at times t0 - R .. t0 - 1
        f = lambda v: torch.from_numpy(v).to(dev)
        self.scale, self.offset, self.thr = f(spec.scale)[None, :, None], f(spec.offset)[None, :, None], f(spec.thresholds)
        self.lo, self.inv_w = f(spec.lo), f(spec.inv_w)

    def add(self, xs):
        sp, A = self.spec, self.a
        for s, x in enumerate(xs):
            y = x * self.scale + self.offset
            if sp.speed is not None:
                u, v = y[:, sp.speed[0]], y[:, sp.speed[1]]
                y = torch.cat([y, torch.sqrt(u * u + v * v)[:, None]], dim=1)
            y = torch.cat([self.past[s], y])                          # [R + T, nout, P]
            for t in range(x.shape[0]):
                yt = y[sp.R + t]
                for k in range(sp.nthr):
                    cond = (yt < self.thr[:, k, None]) if sp.below[k] else (yt > self.thr[:, k, None])
                    run = A["open"][s, :, k]
                    ended = ~cond & (run > 0)
                    rows = (run.clamp(max=sp.ndur) - 1).clamp(min=0).to(torch.int64)
                    A["spells"][s, :, k].scatter_add_(1, rows, ended.to(torch.int64))
                    A["spellmap"][s, :, k, 0] += ended
                    A["spellmap"][s, :, k, 1] += torch.where(ended, run, 0)
                    run.copy_(torch.where(cond, run + 1, 0))
                    A["spellmap"][s, :, k, 2] = torch.maximum(A["spellmap"][s, :, k, 2], run)
                fin, yd = torch.isfinite(yt), yt.double()
                A["accnt"][s, :, 0] += fin
                A["acsum"][s, :, 0] += torch.where(fin, yd, 0.0)
                A["acsum"][s, :, 1] += torch.where(fin, yd * yd, 0.0)
                for l, tau in enumerate(sp.lags):
                    if self.t0 + t - tau < 0:
                        continue
                    yl = y[sp.R + t - tau]
                    q = (yt - yl - self.lo[:, l, None]) * self.inv_w[:, l, None]
                    row = torch.where(q < 0, 0, torch.where(q >= sp.nbins, sp.nbins + 1, 1 + q.clamp(0, sp.nbins - 1).to(torch.int64)))
                    row = torch.where(torch.isnan(q), sp.nbins + 2, row)
                    A["ramps"][s, :, l].scatter_add_(1, row, torch.ones_like(row))
                    both, yld = fin & torch.isfinite(yl), yl.double()
                    A["accnt"][s, :, 1 + l] += both
                    A["acsum"][s, :, 2 + 2 * l] += torch.where(both, yd * yld, 0.0)
                    A["acsum"][s, :, 3 + 2 * l] += torch.where(both, yd + yld, 0.0)
            self.past[s] = y[y.shape[0] - sp.R:]
        self.t0 += xs[0].shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--out", default=None, help="also write the whole record (indented JSON) to this file")
    a = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps("f32", dev)
    C, T = 2, 32
    spec = temporal.TemporalSpec.zscore(C)
    rec = {"gpu": torch.cuda.get_device_name(0), "lib_sha16": sha(_lib.LIB_PATH),
           "temporal_hip_sha16": sha(os.path.join(ROOT, "downgan_amd", "csrc", "temporal.hip")), "C": C, "T": T, "nthr": spec.nthr,
           "lags": list(spec.lags), "nbins": spec.nbins, "ndur": spec.ndur, "cases": []}
    g = torch.Generator(device=dev).manual_seed(0)

    def series(N):
        x = torch.randn(T, C, N, N, generator=g, device=dev)
        for t in range(1, T):
            x[t] = 0.9 * x[t - 1] + (1 - 0.9 ** 2) ** 0.5 * x[t]
        return x.contiguous()

    def padded(x):
        t = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 16, dtype=torch.bfloat16, device=dev)
        t[..., :C] = x.permute(0, 2, 3, 1)
        return t

    for N in a.sizes:
        real, fake = series(N), series(N)
        P = N * N
        for layout in ("nchw_f32", "nhwc_bf16_padded"):
            xs, kw = ((real, fake), {}) if layout == "nchw_f32" else ((padded(real), padded(fake)), {"nhwc": True, "channels": C})
            seen = [v.reshape(T, C, P) if layout == "nchw_f32" else v[..., :C].permute(0, 3, 1, 2).float().reshape(T, C, P) for v in xs]
            acc = temporal.Temporal(spec, N, N, paired=True, device=dev, ops=ops)
            ref = TorchTemporal(spec, 2, P, dev)
            for _ in range(2):                                       # the second call continues the first: the carried state
                acc.add(*xs, **kw)
                ref.add(seen)
            ints = all(bool(torch.equal(ref.a[k], acc.arrays[k])) for k in ("open", "spells", "spellmap", "ramps", "accnt"))
            sums = float((ref.a["acsum"] - acc.arrays["acsum"]).abs().max())
            t_add = timed(lambda: acc.add(*xs, **kw), a.reps)
            t_torch = timed(lambda: ref.add(seen), max(2, a.reps // 5))
            es = xs[0].element_size()
            inp = 2 * T * C * P * es
            state = 2 * (acc.nbytes - acc.arrays["spells"].numel() * 8 - acc.arrays["ramps"].numel() * 8)
            r = {"case": f"{layout}_{N}", "shape": list(xs[0].shape), "dtype": str(xs[0].dtype).replace("torch.", ""),
                 "integers_match_torch": ints, "acsum_max_abs_diff_to_torch": sums, "add_ms": t_add * 1e3, "input_bytes": inp,
                 "input_GBps": inp / t_add / 1e9, "state_bytes": state, "reads_per_field": 1 + spec.nlag,
                 "input_and_state_GBps": (inp + state) / t_add / 1e9, "torch_add_ms": t_torch * 1e3, "torch_over_hip": t_torch / t_add}
            print(json.dumps(r), flush=True)
            rec["cases"].append(r)
            del acc, ref, xs, seen
            torch.cuda.empty_cache()
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
