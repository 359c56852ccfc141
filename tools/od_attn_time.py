#!/usr/bin/env python3
"""Times mhaq_amd.od_attention.psa_attention forward plus backward with HIP events against the eager three-statement chain of the
reference's Attention.forward (torch autograd) on the same device, alternating the two, and reports the peak memory each side
adds.  Default: B = 16, nh = 2, N = 400 (a 640^2 input) and N = 1600 (1280^2), float32 and bfloat16.  Prints one JSON line per
configuration; needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mhaq_amd.od_attention import psa_attention  # noqa: E402


def eager(qkv, nh, addend):
    b, _, h, w = qkv.shape
    q, k, v = qkv.view(b, nh, 128, h * w).split([32, 32, 64], dim=2)
    attn = ((q.transpose(-2, -1) @ k) * 32 ** -0.5).softmax(dim=-1)
    return (v @ attn.transpose(-2, -1)).view(b, nh * 64, h, w) + addend


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--sides", type=int, nargs="+", default=[20, 40])
    ap.add_argument("--dtypes", nargs="+", default=["float32", "bfloat16"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("od_attn_time.py measures on the GPU only: no device found")
    for side in a.sides:
        for name in a.dtypes:
            dtype = getattr(torch, name)
            gen = torch.Generator().manual_seed(side)
            qkv = torch.randn(a.batch, a.heads * 128, side, side, generator=gen).to(dtype).cuda().requires_grad_(True)
            addend = torch.randn(a.batch, a.heads * 64, side, side, generator=gen).to(dtype).cuda()
            go = torch.randn(a.batch, a.heads * 64, side, side, generator=gen).to(dtype).cuda()
            sides = (("kernels", lambda: psa_attention(qkv, a.heads, addend)), ("eager", lambda: eager(qkv, a.heads, addend)))
            times, peak = {"kernels": [], "eager": []}, {}
            for it in range(a.warmup + a.iters):
                for which, fn in sides:
                    qkv.grad = None
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn().backward(go)
                    t1.record()
                    t1.synchronize()
                    if it >= a.warmup:
                        times[which].append(t0.elapsed_time(t1))
            for which, fn in sides:          # what a step adds on top of its inputs, at its peak
                qkv.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                fn().backward(go)
                torch.cuda.synchronize()
                peak[which] = torch.cuda.max_memory_allocated() - base
            q = lambda v: [round(x, 4) for x in statistics.quantiles(v, n=10)[::8]]      # the 10th and 90th percentile
            med = {n: statistics.median(v) for n, v in times.items()}
            n = side * side
            print(json.dumps({"tool": "od_attn_time", "device": torch.cuda.get_device_name(0), "B": a.batch, "nh": a.heads, "N": n,
                              "dtype": name, "iters": a.iters, "kernels_ms_median": round(med["kernels"], 4),
                              "kernels_ms_p10_p90": q(times["kernels"]), "eager_ms_median": round(med["eager"], 4),
                              "eager_ms_p10_p90": q(times["eager"]), "speedup_median": round(med["eager"] / med["kernels"], 2),
                              "kernels_peak_bytes": peak["kernels"], "eager_peak_bytes": peak["eager"],
                              "lse_and_D_bytes": 2 * a.batch * a.heads * n * 4,
                              "one_score_tensor_bytes": a.batch * a.heads * n * n * qkv.element_size()}), flush=True)


if __name__ == "__main__":
    main()
