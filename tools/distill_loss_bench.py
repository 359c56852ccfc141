#!/usr/bin/env python3
"""The distillation loss on one GPU, stand-alone: the framework's chain (the reference modules' torch statements,
tests/distill_ref.py: torch_loss) forward + backward against mhaq_amd.loss.FusedDistillLoss forward + backward, on
[250, 1000], [128, 100] and [1000, 100] logits, float32 and bfloat16, all six kinds.

Times: HIP events around one forward + backward, --reps timed calls after --warmup, alternating the two sides; median and
minimum in microseconds.  Both sides are enqueued by the host one call at a time, so a figure is the larger of the device
work and the host's enqueue time of that side -- what the serial phase of a training step sees.
Launches: counted by `rocprofv3 --kernel-trace --stats` runs of this file's own (--count-child: K and 2K iterations of one
side and kind, the difference of the kernel calls / K), no counters in those runs.
usage: tools/distill_loss_bench.py [--out FILE] [--reps R] [--warmup W] [--no-counts]"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mhaq_amd.loss import FusedDistillLoss  # noqa: E402
from tests import distill_ref as R  # noqa: E402

DEV = "cuda:0"
SHAPES = [(250, 1000), (128, 100), (1000, 100)]
DTYPES = [torch.float32, torch.bfloat16]


def sides(kind, shape, dtype):
    """-> {"torch": fn, "fused": fn}: one forward + backward each, on the same logits."""
    x32, t32 = R.logits(shape, 4.0, seed=shape[0] + shape[1], device=DEV)
    x = x32.to(dtype).requires_grad_(True)
    t = t32.to(dtype)
    crit = FusedDistillLoss(kind)

    def run_torch():
        x.grad = None
        # under autocast the framework's softmax ops run in float32 on the 16-bit logits, as in the trainer
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype != torch.float32):
            loss = R.torch_loss(kind, x, t)
        loss.backward()

    def run_fused():
        x.grad = None
        crit(x, t).backward()
    return {"torch": run_torch, "fused": run_fused}


def time_pair(fns, reps, warmup):
    out = {k: [] for k in fns}
    for i in range(warmup + reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                out[k].append(1e3 * a.elapsed_time(b))
    return {k: (statistics.median(v), min(v)) for k, v in out.items()}


def count_child(side, kind, iters):
    import warnings
    warnings.simplefilter("ignore")
    fn = sides(kind, SHAPES[0], torch.float32)[side]
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()


def kernel_calls(side, kind, iters):
    """Kernel launches of a --count-child run, from rocprofv3's kernel statistics."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--count-child", side, str(kind), str(iters)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel_stats.csv")
        return sum(int(row["Calls"]) for f in files for row in csv.DictReader(open(f)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--count-child", nargs=3, metavar=("SIDE", "KIND", "ITERS"))
    a = ap.parse_args()
    if a.count_child:
        return count_child(a.count_child[0], int(a.count_child[1]), int(a.count_child[2]))
    import warnings
    warnings.simplefilter("ignore")
    lines = ["# tools/distill_loss_bench.py --reps %d --warmup %d: forward + backward, HIP events, microseconds" %
             (a.reps, a.warmup),
             "# %-26s %-11s %-9s %9s %9s %9s %9s %7s" % ("kind", "shape", "dtype", "torch med", "torch min", "fused med",
                                                         "fused min", "ratio")]
    for shape in SHAPES:
        for dtype in DTYPES:
            for kind in R.KINDS:
                r = time_pair(sides(kind, shape, dtype), a.reps, a.warmup)
                lines.append("  %-26s %-11s %-9s %9.1f %9.1f %9.1f %9.1f %7.2f" % (
                    R.NAMES[kind], "%dx%d" % shape, str(dtype)[6:], r["torch"][0], r["torch"][1], r["fused"][0],
                    r["fused"][1], r["torch"][0] / r["fused"][0]))
                print(lines[-1], flush=True)
    if not a.no_counts:
        lines.append("# kernel launches per forward + backward at %dx%d float32 (rocprofv3 --kernel-trace --stats, calls of a "
                     "20-iteration run minus those of a 10-iteration run, / 10)" % SHAPES[0])
        fused = (kernel_calls("fused", R.SKL, 20) - kernel_calls("fused", R.SKL, 10)) / 10.0
        lines.append("  %-26s fused %5.1f   (the same two entry points serve every kind)" % (R.NAMES[R.SKL], fused))
        print(lines[-1], flush=True)
        for kind in R.KINDS:
            n = (kernel_calls("torch", kind, 20) - kernel_calls("torch", kind, 10)) / 10.0
            lines.append("  %-26s torch %5.1f" % (R.NAMES[kind], n))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
