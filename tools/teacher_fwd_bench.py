#!/usr/bin/env python3
"""The frozen teacher's elementwise chain on one GPU, stand-alone per place and shape: torch's separate launches against the
fused one (mhaq_fq_bn_infer_act / mhaq_fq_bn_relu_pool3s2).

Per place of ResNet-18 at batch 250 (channels_last; --dtype fp32, or bf16 / fp16 for what a teacher under torch.autocast
sees: mhaq_fq_bn_infer_act_x16 / mhaq_fq_bn_relu_pool3s2_x16) the chain a stock eval teacher runs -- F.batch_norm on the running
statistics, the in-place ReLU, the residual add, the stem's max pool -- against the one launch of the product library and of
any --lib builds of the same kernels (forced cache policies; see below), all in the same call.  Method of
tools/bn_fwd_bench.py: before every timed call a 1 GiB buffer is written and the inputs are rewritten; --reps timed calls after
one warm-up, HIP events around the whole chain; min and median.  Bytes are algorithmic, per element of the place's input
(fp32; half of it for a 16-bit dtype):
    stem        chain 8 (bn) + 8 (relu) + 5 (pool) = 21      fused 5
    mid         chain 8 + 8 = 16                             fused 8
    end         chain 8 + 12 (add) + 8 = 28                  fused 12
    end_ds      chain 8 + 8 + 12 + 8 = 36                    fused 12
The last lines weight the minima by the places' counts per step.  Every library's output is first checked to be the product
library's bits.

Forced cache policies are builds of csrc/bn_bwd.hip with the rule overridden (first letter: loads, second: stores; p = default
policy, n = non-temporal), e.g. for "nn":
    hipcc $(make -s -C mhaq_amd/csrc print-flags) -DMHAQ_BN_INFER_NT_ELEMS=0 -DMHAQ_BN_INFER_ST_NT=1 \\
          -shared -o nn.so mhaq_amd/csrc/bn_bwd.hip
The 16-bit kernels have their own three: -DMHAQ_BN_INFER16_NT_ELEMS=0 (or a huge value: never), -DMHAQ_BN_INFER16_ST_NT=1 and
the occupancy threshold -DMHAQ_BN_INFER16_BIG_ELEMS=0 (or a huge value).

--step: tools/amp_bench.py's ResNet-18 batch-250 bf16 step, captured, in THIS process's configuration (one JSON line):
MHAQ_TEACHER_FUSED_X16=1 in the environment gives the switched-on side of an A/B, run process by process.
usage: tools/teacher_fwd_bench.py [--dtype fp32|bf16|fp16] [--out FILE] [--lib LABEL=PATH ...] [--reps R] [--batch N]
       tools/teacher_fwd_bench.py --step [--steps K] [--warmup W]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools import amp_bench  # noqa: E402,F401  (seeds the private MIOpen database before torch touches MIOpen)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mhaq_amd import _lib  # noqa: E402

# (place, C, H = W of the place's input, launches per step)
PLACES = [("stem", 64, 112, 1),
          ("mid", 64, 56, 2), ("end", 64, 56, 2),
          ("mid", 128, 28, 2), ("end", 128, 28, 1), ("end_ds", 128, 28, 1),
          ("mid", 256, 14, 2), ("end", 256, 14, 1), ("end_ds", 256, 14, 1),
          ("mid", 512, 7, 2), ("end", 512, 7, 1), ("end_ds", 512, 7, 1)]
BYTES = {"stem": (21, 5), "mid": (16, 8), "end": (28, 12), "end_ds": (36, 12)}
MODE = {"mid": 0, "end": 1, "end_ds": 2}
EPS = 1e-5
NAMES = ("mhaq_fq_bn_infer_consts", "mhaq_fq_bn_infer_act", "mhaq_fq_bn_relu_pool3s2", "mhaq_fq_bn_infer_act_x16",
         "mhaq_fq_bn_relu_pool3s2_x16")
DTYPES = {"fp32": (torch.float32, 0), "bf16": (torch.bfloat16, _lib.DT_BF16), "fp16": (torch.float16, _lib.DT_F16)}


def load(path):
    """A build of csrc/bn_bwd.hip alone: only the entry points timed here."""
    L = ctypes.CDLL(path)
    for name in NAMES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return L


def step(args):
    """One process of the step A/B: the bf16 captured step with the switches as the environment has them."""
    from mhaq_amd import _ext, frozen_blocks
    E = _ext.ext()
    n0 = E.teacher_fused_calls(), E.teacher_fused_x16_calls()
    rec = {"tool": "teacher_fwd_bench", "device": torch.cuda.get_device_name(0),
           "teacher_fused_x16": frozen_blocks.x16_enabled(False),
           "bf16_captured": amp_bench.step(torch.device("cuda:0"), True, True, args.steps, max(args.warmup, 4))}
    rec["fused_launches_recorded"] = E.teacher_fused_calls() - n0[0]
    rec["x16_launches_recorded"] = E.teacher_fused_x16_calls() - n0[1]
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--dtype", choices=sorted(DTYPES), default="fp32")
    ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.backends.cudnn.benchmark = False
    if args.step:
        return step(args)
    dev = "cuda:0"
    dtype, dt = DTYPES[args.dtype]
    bscale = dtype.itemsize / 4
    libs = [("product", _lib.lib())] + [(s.split("=", 1)[0], load(s.split("=", 1)[1])) for s in args.lib]
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())
    rows = []
    tot = {"chain": [0.0, 0.0]}
    for place, c, hw, count in PLACES:
        shape = (args.batch, c, hw, hw)
        m, elems = args.batch * hw * hw, args.batch * c * hw * hw
        gen = torch.Generator(device=dev).manual_seed(1)
        mk = lambda: (torch.randn(shape, device=dev, generator=gen) * 2 + 1).to(dtype).contiguous(memory_format=torch.channels_last)
        x0, b0 = mk(), (mk() if place in ("end", "end_ds") else None)
        x, b = x0.clone(memory_format=torch.preserve_format), (None if b0 is None else b0.clone(memory_format=torch.preserve_format))
        bn = [[torch.randn(c, device=dev, generator=gen), torch.rand(c, device=dev, generator=gen) + 0.5,
               torch.randn(c, device=dev, generator=gen), torch.randn(c, device=dev, generator=gen)] for _ in range(2)]
        k = [torch.empty(3, c, device=dev) for _ in range(2)]
        y = torch.empty((args.batch, c, (hw - 1) // 2 + 1, (hw - 1) // 2 + 1) if place == "stem" else shape, device=dev,
                        dtype=dtype).contiguous(memory_format=torch.channels_last)

        def chain():
            t = F.batch_norm(x, bn[0][0], bn[0][1], bn[0][2], bn[0][3], False, 0.1, EPS)
            if place == "stem":
                return F.max_pool2d(F.relu_(t), 3, 2, 1)
            if place == "mid":
                return F.relu_(t)
            r = b if place == "end" else F.batch_norm(b, bn[1][0], bn[1][1], bn[1][2], bn[1][3], False, 0.1, EPS)
            return F.relu_(t + r)

        def fused(L):
            ds = place == "end_ds"
            if place == "stem" and dt:
                rc = L.mhaq_fq_bn_relu_pool3s2_x16(P(x), P(k[0]), P(y), args.batch, hw, hw, c, dt, st)
            elif place == "stem":
                rc = L.mhaq_fq_bn_relu_pool3s2(P(x), P(k[0]), P(y), args.batch, hw, hw, c, st)
            elif dt:
                rc = L.mhaq_fq_bn_infer_act_x16(P(x), P(k[0]), P(b) if ds else None, P(k[1]) if ds else None,
                                                None if ds or place == "mid" else P(b), P(y), m, c, MODE[place], dt, st)
            else:
                rc = L.mhaq_fq_bn_infer_act(P(x), P(k[0]), P(b) if ds else None, P(k[1]) if ds else None,
                                            None if ds or place == "mid" else P(b), P(y), m, c, MODE[place], st)
            assert rc == 0, rc

        def timed(fn):
            out = []
            for i in range(args.reps + 1):
                flush.fill_(float(i))
                x.copy_(x0)
                if b is not None:
                    b.copy_(b0)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                if i:
                    out.append(a.elapsed_time(e) * 1e3)
            return min(out), statistics.median(out)

        def row(variant, mm, bpe):
            bpe = bpe * bscale
            rows.append(f"{place:>7s} {str(shape):>20s} x{count} {elems / 1e6:8.1f} {variant:>8s} {mm[0]:8.1f} {mm[1]:8.1f} "
                        f"{bpe:4.1f} B/elem {bpe * elems / mm[0] / 1e6:8.2f}")
            print(rows[-1], flush=True)
            t = tot.setdefault(variant, [0.0, 0.0])
            t[0] += count * mm[0]
            t[1] += count * bpe * elems

        ref = None
        for label, L in libs:
            for j in range(2):
                assert L.mhaq_fq_bn_infer_consts(P(bn[j][0]), P(bn[j][1]), P(bn[j][2]), P(bn[j][3]), EPS, c, P(k[j]), st) == 0
            fused(L)
            if ref is None:
                ref = y.clone()
                want = chain()
                print(f"{place:>7s} {str(shape):>20s}  max |fused - chain| / (|chain| + 1) = "
                      f"{float(((ref.float() - want.float()).abs() / (want.float().abs() + 1)).max()):.2e}", flush=True)
                del want
            else:
                bits = torch.int32 if dtype is torch.float32 else torch.int16
                assert torch.equal(ref.view(bits), y.view(bits)), label      # the cache policy changes no bit
        del ref
        row("chain", timed(chain), BYTES[place][0])
        for label, L in libs:
            row(label, timed(lambda: fused(L)), BYTES[place][1])
        del x, x0, b, b0, y
        torch.cuda.empty_cache()
    head = (f"The frozen teacher's elementwise chain per place in {args.dtype}, batch {args.batch}, one {torch.cuda.get_device_name(0)}, "
            f"one call: torch's separate launches (chain)\nagainst the fused launch of the product library and of forced cache "
            f"policies of the same kernels (first letter: loads,\nsecond: stores; p = default policy, n = non-temporal).  Before "
            f"every timed call a 1 GiB buffer is written and the inputs are\nrewritten; {args.reps} timed calls after one "
            f"warm-up, HIP events around the whole chain.\n\n"
            f"{'place':>7s} {'shape':>20s} {'n':>2s} {'Melems':>8s} {'variant':>8s} {'min us':>8s} {'med us':>8s} "
            f"{'bytes':>11s} {'TB/s(min)':>8s}\n")
    sums = "\n".join(f"per step, weighted by the counts: {v:>8s} {t[0] / 1e3:7.3f} ms  {t[1] / 1e9:6.2f} GB  {t[1] / t[0] / 1e6:5.2f} TB/s"
                     for v, t in tot.items())
    text = head + "\n".join(rows) + "\n\n" + sums + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
