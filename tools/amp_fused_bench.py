#!/usr/bin/env python3
"""What the ReLU / residual-add forms of the 16-bit activation kernels cost and save on one GPU; prints ONE JSON line
(profiles/r12_amp_fused.txt holds a run).

  kernels  mhaq_fq_act_relu_fwd_x16 / mhaq_fq_act_relu_bwd_partials_x16 in their three forms -- relu_fq (z -> y),
           add_relu_fq_a (z, addend -> y, a; backward with g_a), relu_fq_a (z -> y, a; backward with g_a) -- next to the
           plain mhaq_fq_act_fwd_x16 / mhaq_fq_act_bwd_partials_x16, bf16, STE with in-kernel signs, on the dominant
           ResNet-18 activation [250,64,56,56] channels_last.  HIP events around every call, median of --reps; every call
           takes the next of --sets buffer sets, so that no call finds its inputs in the 256 MB last-level cache because
           the call before it left them there.  bytes_per_elem is what the form moves; frac_peak is against 8 TB/s.
  step     (--step) tools/amp_bench.py's ResNet-18 batch-250 bf16 step, captured, in THIS process's configuration:
           MHAQ_FUSE_BLOCKS=0 in the environment gives the unfused side of an A/B, run process by process.

usage: tools/amp_fused_bench.py [--reps R] [--sets S] | --step [--steps K] [--warmup W]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import amp_bench  # noqa: E402  (seeds the private MIOpen database before torch touches MIOpen)

import torch  # noqa: E402

PEAK = 8.0e12


def timed_rotating(calls, reps):
    """Median microseconds of one call; call k runs calls[k % len(calls)]."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k in range(len(calls)):
        calls[k]()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(ev):
        a.record()
        calls[k % len(calls)]()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2]


def kernels(dev, reps, nsets):
    from mhaq_amd import _lib, ops
    L = _lib.lib()
    st = ops._stream
    shape = (250, 64, 56, 56)
    n = 250 * 64 * 56 * 56
    dt = _lib.DT_BF16
    gen = torch.Generator(device=dev).manual_seed(3)

    def t16(scale):
        return (torch.randn(shape, device=dev, generator=gen) * scale).bfloat16().contiguous(memory_format=torch.channels_last)
    sets = [dict(z=t16(2.0), add=t16(1.0), g=t16(1.0), ga=t16(1.0), y=t16(0.0), a=t16(0.0), gx=t16(0.0))
            for _ in range(nsets)]
    ls, lq, b = (torch.tensor([v], device=dev) for v in (-3.0, 2.0, -2.0))
    params = torch.empty(5, device=dev)
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    npart = _lib.C.c_int32(0)
    P = lambda t: t.data_ptr()  # noqa: E731

    def fwd_plain(s):
        return lambda: _lib.check(L.mhaq_fq_act_fwd_x16(P(s["z"]), P(s["y"]), n, dt, P(ls), P(lq), P(b), P(params), None,
                                                        None, None, 0, st()), "fwd")

    def bwd_plain(s):
        return lambda: _lib.check(L.mhaq_fq_act_bwd_partials_x16(P(s["z"]), P(s["g"]), P(s["gx"]), n, dt, P(params), 0,
                                                                 None, 7, 1, None, P(ws), nb, _lib.C.byref(npart), st()),
                                  "bwd")

    def fwd_relu(s, add, a):
        return lambda: _lib.check(L.mhaq_fq_act_relu_fwd_x16(P(s["z"]), P(s["add"]) if add else None, P(s["y"]),
                                                             P(s["a"]) if a else None, n, dt, P(ls), P(lq), P(b),
                                                             P(params), st()), "relu_fwd")

    def bwd_relu(s, ga):
        return lambda: _lib.check(L.mhaq_fq_act_relu_bwd_partials_x16(P(s["z"]), P(s["g"]), P(s["ga"]) if ga else None,
                                                                      P(s["gx"]), n, dt, P(params), 0, 7, 1, None, P(ws),
                                                                      nb, _lib.C.byref(npart), st()), "relu_bwd")

    fwd_plain(sets[0])()                              # publishes params for the backward calls
    torch.cuda.synchronize()
    out = {"tensor": "[250,64,56,56] channels_last bf16", "elements": n, "reps": reps, "buffer_sets": nsets}

    def rec(name, make_f, fb, make_b, bb):
        tf = timed_rotating([make_f(s) for s in sets], reps)
        tb = timed_rotating([make_b(s) for s in sets], reps)
        out[name] = {"fwd_us": round(tf, 2), "bwd_us": round(tb, 2), "bytes_per_elem": {"fwd": fb, "bwd": bb},
                     "fwd_frac_peak": round(fb * n / (tf * 1e-6) / PEAK, 3),
                     "bwd_frac_peak": round(bb * n / (tb * 1e-6) / PEAK, 3)}

    rec("plain_x16", fwd_plain, 4, bwd_plain, 6)
    rec("relu_fq", lambda s: fwd_relu(s, False, False), 4, lambda s: bwd_relu(s, False), 6)
    rec("add_relu_fq_a", lambda s: fwd_relu(s, True, True), 8, lambda s: bwd_relu(s, True), 8)
    rec("relu_fq_a", lambda s: fwd_relu(s, False, True), 6, lambda s: bwd_relu(s, True), 8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    rec = {"tool": "amp_fused_bench", "device": torch.cuda.get_device_name(0)}
    if args.step:
        from mhaq_amd import fused_blocks
        rec["fuse_blocks"] = fused_blocks.enabled_by_env()
        rec["bf16_captured"] = amp_bench.step(dev, True, True, args.steps, max(args.warmup, 4))
    else:
        rec["kernels"] = kernels(dev, args.reps, args.sets)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
