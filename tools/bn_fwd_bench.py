#!/usr/bin/env python3
"""The HIP BatchNorm training forward (mhaq_fq_bn_fwd; with --dtype bf16 | fp16: mhaq_fq_bn_fwd_x16) on one GPU, stand-alone
per shape.

Per shape (the five student shapes of ResNet-18 at batch 250, fp32 channels_last): the framework's own training forward
(_batch_norm_impl_index: what the step runs without MHAQ_BN_FORWARD=1) against mhaq_fq_bn_fwd of the product library and of
any --lib builds of the same kernels (the forced cache policies; see below), all in the same call.  Method of
profiles/r10_bn_bwd_micro.txt: before every timed call a 1 GiB buffer is written and x is rewritten; --reps timed calls after
one warm-up, HIP events around the whole forward (three launches); min and median.  Bytes are algorithmic: x read twice, y
written once = 12 B per element.  Every library's y, statistics and running statistics are first checked to be the product
library's bits, and the product's y is held against the framework's (largest difference in units of |y| + 1; printed).

Forced cache policies are builds of csrc/bn_bwd.hip with the thresholds overridden (first letter: loads of the reduction,
second: of the normalisation; p = default policy, n = non-temporal), e.g. for "pn":
    hipcc $(make -s -C mhaq_amd/csrc print-flags) -DMHAQ_BN_FWD_REDUCE_NT_ELEMS=INT64_MAX -DMHAQ_BN_FWD_NORM_NT_ELEMS=0 \\
          -shared -o pn.so mhaq_amd/csrc/bn_bwd.hip
--dtype bf16 | fp16: x and y in that type (the convolution's output under autocast), the framework's own 16-bit forward against
mhaq_fq_bn_fwd_x16; 6 B per element; the thresholds of a forced build are MHAQ_BN_FWD16_REDUCE_NT_ELEMS / _NORM_NT_ELEMS.
--step: tools/amp_bench.py's ResNet-18 batch-250 bf16 step, captured, in THIS process's configuration (MHAQ_BN_BACKWARD_X16=1 with
MHAQ_BN_FORWARD_X16=1 in the environment gives the new side of an A/B, run process by process).  Prints ONE JSON line.
usage: tools/bn_fwd_bench.py [--dtype fp32|bf16|fp16] [--out FILE] [--lib LABEL=PATH ...] [--reps R] | --step [--steps K] [--warmup W]"""
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
NAMES = ("mhaq_fq_bn_fwd_workspace_bytes", "mhaq_fq_bn_fwd")
NAMES_X16 = ("mhaq_fq_bn_fwd_x16_workspace_bytes", "mhaq_fq_bn_fwd_x16")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def load(path, names=NAMES):
    """A build of csrc/bn_bwd.hip alone: only the two entry points timed here."""
    L = ctypes.CDLL(path)
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp32")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    if args.step:
        from mhaq_amd import _ext, bn_backward
        rec = {"tool": "bn_fwd_bench", "device": torch.cuda.get_device_name(0), "bn_backward_x16": bn_backward.x16_enabled(),
               "bn_forward_x16": bn_backward.hip_forward_x16_enabled()}
        rec["bf16_captured"] = amp_bench.step(torch.device("cuda:0"), True, True, args.steps, max(args.warmup, 4))
        rec["x16_forwards_recorded"] = _ext.ext().bn_hip_forwards_x16()
        rec["x16_backwards_recorded"] = _ext.ext().bn_hip_backwards_x16()
        print(json.dumps(rec), flush=True)
        return
    dev = "cuda:0"
    dtype = DTYPES[args.dtype]
    x16 = dtype is not torch.float32
    names = NAMES_X16 if x16 else NAMES
    code = {torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16}.get(dtype)
    bpe = 6 if x16 else 12                    # algorithmic bytes per element: x read twice, y written once
    libs = [("product", _lib.lib())] + [(s.split("=", 1)[0], load(s.split("=", 1)[1], names)) for s in args.lib]
    query = lambda L, m, c: getattr(L, names[0])(m, c)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda a: ctypes.c_void_p(a.data_ptr())
    rows, notes = [], []
    for shape in SHAPES:
        n, c, h, w = shape
        m, elems = n * h * w, n * c * h * w
        gen = torch.Generator(device=dev).manual_seed(1)
        x0 = (torch.randn(shape, device=dev, generator=gen) * 2 + 1).to(dtype).contiguous(memory_format=torch.channels_last)
        x = x0.clone(memory_format=torch.preserve_format)
        gamma, beta = torch.randn(c, device=dev, generator=gen), torch.randn(c, device=dev, generator=gen)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        y = torch.empty_like(x)
        mean, invstd = torch.empty(c, device=dev), torch.empty(c, device=dev)
        nb = query(libs[0][1], m, c)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def stock():
            return torch.ops.aten._batch_norm_impl_index(x, gamma, beta, rm, rv, True, 0.1, EPS, True)

        def hip(L):
            if x16:
                assert L.mhaq_fq_bn_fwd_x16(P(x), P(gamma), P(beta), P(y), P(mean), P(invstd), P(rm), P(rv), 0.1, EPS, m, c,
                                            code, P(ws), nb, st) == 0
                return
            assert L.mhaq_fq_bn_fwd(P(x), P(gamma), P(beta), P(y), P(mean), P(invstd), P(rm), P(rv), 0.1, EPS, m, c, P(ws),
                                    nb, st) == 0

        def timed(fn):
            out = []
            for i in range(args.reps + 1):
                flush.fill_(float(i))
                x.copy_(x0)
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
                        f"{bpe * elems / mm[0] / 1e6:22.2f}")
            print(rows[-1], flush=True)

        def fresh(L):
            rm.zero_()
            rv.fill_(1.0)
            hip(L)
            return [t.clone() for t in (y, mean, invstd, rm, rv)]

        ref = fresh(libs[0][1])
        for label, L in libs[1:]:                 # the cache policy changes no bit
            assert query(L, m, c) == nb
            bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(ref, fresh(L))), label
        rm.zero_()
        rv.fill_(1.0)
        fw = stock()
        notes.append(f"{str(shape):>20s}  max |y - y_miopen| / (|y| + 1) = {float(((ref[0].float() - fw[0].float()).abs() / (fw[0].float().abs() + 1)).max()):.2e}"
                     f"   max rel. mean {float(((ref[1] - fw[1]).abs() / fw[1].abs().clamp_min(1e-30)).max()):.2e}"
                     f"  invstd {float(((ref[2] - fw[2]).abs() / fw[2].abs()).max()):.2e}")
        del ref, fw
        row("miopen", timed(stock))
        for label, L in libs:
            row(label, timed(lambda: hip(L)))
        del x, x0, y, ws
        torch.cuda.empty_cache()
    head = (f"BatchNorm training forward per shape in {args.dtype}, one {torch.cuda.get_device_name(0)}, one call: the framework's own "
            f"forward (_batch_norm_impl_index) against {names[1]}\n(product) and forced cache policies of the same kernels "
            f"(first letter: loads of the reduction, second: of the normalisation; p = default policy,\nn = non-temporal).  "
            f"Before every timed call a 1 GiB buffer is written and x is rewritten; {args.reps} timed calls after one warm-up, "
            f"HIP events around the\nwhole forward (three launches).\n\n"
            f"{'shape':>20s} {'elems':>8s} {'variant':>8s} {'min us':>8s} {'med us':>8s}   TB/s(min, {bpe} B/elem)\n")
    text = head + "\n".join(rows) + "\n\nThe product against the framework's forward on the same inputs (nothing is asserted):\n" + \
        "\n".join(notes) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
