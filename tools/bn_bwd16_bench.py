#!/usr/bin/env python3
"""The 16-bit BatchNorm backward (mhaq_fq_bn_bwd_x16) on one GPU: stand-alone per shape, and inside the bf16 step.

  default  per shape (the five student shapes of ResNet-18 at batch 250, channels_last, --dtype bf16): the framework's own
           16-bit backward (_batch_norm_impl_index_backward on the forward's saved tensors: what a bf16 step runs without
           this route) against mhaq_fq_bn_bwd_x16 of the product library and of any --lib builds of the same kernels (the
           forced cache policies; see below).  Method of profiles/r10_bn_bwd_micro.txt: before every timed call a 1 GiB buffer
           is written and dy is rewritten; --reps timed calls after one warm-up, HIP events around the whole backward (three
           launches); min and median.  Bytes are algorithmic: x and dy read twice, dx written once = 10 B per element.
           Every library's dx, dweight and dbias are first checked to be the product library's bits.
  --step   tools/amp_bench.py's ResNet-18 batch-250 bf16 step, captured, in THIS process's configuration:
           MHAQ_BN_BACKWARD_X16=1 in the environment gives the new side of an A/B, run process by process.  Prints ONE JSON line.

Forced cache policies are builds of csrc/bn_bwd.hip with the thresholds overridden (first letter: loads of the reduction,
second: of dx; p = default policy, n = non-temporal), e.g. for "pn":
    hipcc $(make -s -C mhaq_amd/csrc print-flags) -DMHAQ_BN16_REDUCE_NT_ELEMS=INT64_MAX -DMHAQ_BN16_DX_NT_ELEMS=0 \\
          -shared -o pn.so mhaq_amd/csrc/bn_bwd.hip
usage: tools/bn_bwd16_bench.py [--out FILE] [--lib LABEL=PATH ...] [--reps R] [--dtype bf16|fp16] | --step [--steps K] [--warmup W]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import amp_bench  # noqa: E402  (seeds the private MIOpen database before torch touches MIOpen)

import torch  # noqa: E402

from mhaq_amd import _lib  # noqa: E402

SHAPES = [(250, 64, 112, 112), (250, 64, 56, 56), (250, 128, 28, 28), (250, 256, 14, 14), (250, 512, 7, 7)]
EPS = 1e-5


def load(path):
    """A build of csrc/bn_bwd.hip alone: only the two entry points timed here."""
    L = ctypes.CDLL(path)
    for name in ("mhaq_fq_bn_bwd_x16_workspace_bytes", "mhaq_fq_bn_bwd_x16"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return L


def micro(args):
    dev = "cuda:0"
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    code = _lib.DT_BF16 if args.dtype == "bf16" else _lib.DT_F16
    libs = [("product", _lib.lib())] + [(s.split("=", 1)[0], load(s.split("=", 1)[1])) for s in args.lib]
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda a: ctypes.c_void_p(a.data_ptr())
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    rows = []
    for shape in SHAPES:
        n, c, h, w = shape
        m, elems = n * h * w, n * c * h * w
        gen = torch.Generator(device=dev).manual_seed(1)
        cl = torch.channels_last
        x = (torch.randn(shape, device=dev, generator=gen) * 2 + 1).to(dtype).contiguous(memory_format=cl)
        dy0 = torch.randn(shape, device=dev, generator=gen).to(dtype).contiguous(memory_format=cl)
        dy = dy0.clone(memory_format=torch.preserve_format)
        gamma, beta = torch.randn(c, device=dev, generator=gen), torch.randn(c, device=dev, generator=gen)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        fwd = torch.ops.aten._batch_norm_impl_index(x, gamma, beta, rm, rv, True, 0.1, EPS, True)
        mean, invstd, reserve, impl = fwd[1], fwd[2], fwd[3], fwd[4]
        del fwd
        dx = torch.empty_like(x)
        dw, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
        nb = libs[0][1].mhaq_fq_bn_bwd_x16_workspace_bytes(m, c)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def stock():
            torch.ops.aten._batch_norm_impl_index_backward(impl, x, dy, gamma, rm, rv, mean, invstd, True, EPS,
                                                           [True, True, True], reserve)

        def hip(L):
            assert L.mhaq_fq_bn_bwd_x16(P(x), P(dy), P(mean), P(invstd), P(gamma), P(dx), P(dw), P(db), m, c, code, P(ws),
                                        nb, st) == 0

        def timed(fn):
            out = []
            for i in range(args.reps + 1):
                flush.fill_(float(i))
                dy.copy_(dy0)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                if i:
                    out.append(a.elapsed_time(e) * 1e3)
            return min(out), statistics.median(out)

        def row(variant, mm):
            rows.append(f"{str(shape):>20s} {elems / 1e6:8.1f} {variant:>8s} {mm[0]:8.1f} {mm[1]:8.1f} "
                        f"{10 * elems / mm[0] / 1e6:22.2f}")
            print(rows[-1], flush=True)

        hip(libs[0][1])
        ref = [t.clone() for t in (dx, dw, db)]
        for label, L in libs[1:]:                 # the cache policy changes no bit
            assert L.mhaq_fq_bn_bwd_x16_workspace_bytes(m, c) == nb
            hip(L)
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(ref, (dx, dw, db))), label
        del ref
        row("miopen", timed(stock))
        for label, L in libs:
            row(label, timed(lambda: hip(L)))
        del x, dy, dy0, dx, ws
        torch.cuda.empty_cache()
    head = (f"BatchNorm backward per shape in {args.dtype}, one {torch.cuda.get_device_name(0)}, one call: the framework's own "
            f"16-bit backward (_batch_norm_impl_index_backward on the\nforward's saved tensors) against mhaq_fq_bn_bwd_x16 "
            f"(product) and forced cache policies of the same kernels (first letter: loads of the reduction,\nsecond: of dx; "
            f"p = default policy, n = non-temporal).  Before every timed call a 1 GiB buffer is written and dy is rewritten; "
            f"{args.reps} timed calls after one\nwarm-up, HIP events around the whole backward (three launches).\n\n"
            f"{'shape':>20s} {'elems':>8s} {'variant':>8s} {'min us':>8s} {'med us':>8s}   TB/s(min, 10 B/elem)\n")
    text = head + "\n".join(rows) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
    ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    if not args.step:
        return micro(args)
    from mhaq_amd import _ext, bn_backward
    rec = {"tool": "bn_bwd16_bench", "device": torch.cuda.get_device_name(0), "bn_backward_x16": bn_backward.x16_enabled()}
    rec["bf16_captured"] = amp_bench.step(torch.device("cuda:0"), True, True, args.steps, max(args.warmup, 4))
    rec["x16_backwards_recorded"] = _ext.ext().bn_hip_backwards_x16()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
