#!/usr/bin/env python3
"""The classification head on one GPU, stand-alone: the framework's chain against the fused calls on [250, 1000], [128, 10]
and [1000, 100] logits, float32 and bfloat16, in the two places the trainer has them:

  train     cross_entropy forward + backward                  against  mhaq_amd.loss.FusedCrossEntropy forward + backward
  validate  cross_entropy; argmax, eq, mean; topk, eq, any,   against  mhaq_amd.cls_metrics.cls_metrics
            mean (no gradient)

Times: HIP events around one call of a side, --reps timed calls after --warmup, alternating the two sides; median and
minimum in microseconds.  Both sides are enqueued by the host one call at a time, so a figure is the larger of the device
work and the host's enqueue time of that side -- what the serial phase of a step sees.
Launches: counted by `rocprofv3 --kernel-trace --stats` runs of this file's own (--count-child: K and 2K iterations of one
side, the difference of the kernel calls / K), no counters in those runs.
usage: tools/cls_head_bench.py [--out FILE] [--reps R] [--warmup W] [--no-counts]"""
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
import torch.nn.functional as F  # noqa: E402

from mhaq_amd.cls_metrics import cls_metrics  # noqa: E402
from mhaq_amd.loss import FusedCrossEntropy  # noqa: E402

DEV = "cuda:0"
SHAPES = [(250, 1000), (128, 10), (1000, 100)]
DTYPES = [torch.float32, torch.bfloat16]
PLACES = ["train", "validate"]


def sides(place, shape, dtype):
    """-> {"torch": fn, "fused": fn}: one call each, on the same logits and labels."""
    gen = torch.Generator().manual_seed(shape[0] + shape[1])
    x = (torch.randn(shape, generator=gen) * 4.0).to(DEV).to(dtype).requires_grad_(place == "train")
    y = torch.randint(0, shape[1], (shape[0],), generator=gen).to(DEV)
    crit = FusedCrossEntropy()
    # under autocast the framework's cross_entropy runs in float32 on the 16-bit logits, as in the trainer
    amp = lambda: torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype != torch.float32)      # noqa: E731

    def train_torch():
        x.grad = None
        with amp():
            loss = F.cross_entropy(x, y)
        loss.backward()

    def train_fused():
        x.grad = None
        crit(x, y).backward()

    @torch.no_grad()
    def validate_torch():
        with amp():
            loss = F.cross_entropy(x, y)
        top1 = (x.argmax(1) == y).float().mean()
        top5 = (x.topk(5, dim=1).indices == y[:, None]).any(1).float().mean()
        return loss, top1, top5

    def validate_fused():
        return cls_metrics(x, y, topk=5)
    return ({"torch": train_torch, "fused": train_fused} if place == "train"
            else {"torch": validate_torch, "fused": validate_fused})


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


def count_child(place, side, iters):
    import warnings
    warnings.simplefilter("ignore")
    fn = sides(place, SHAPES[0], torch.float32)[side]
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()


def kernel_calls(place, side, iters):
    """Kernel launches of a --count-child run, from rocprofv3's kernel statistics."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--count-child", place, side, str(iters)]
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
    ap.add_argument("--count-child", nargs=3, metavar=("PLACE", "SIDE", "ITERS"))
    a = ap.parse_args()
    if a.count_child:
        return count_child(a.count_child[0], a.count_child[1], int(a.count_child[2]))
    import warnings
    warnings.simplefilter("ignore")
    lines = ["# tools/cls_head_bench.py --reps %d --warmup %d: HIP events, microseconds" % (a.reps, a.warmup),
             "# %-9s %-11s %-9s %9s %9s %9s %9s %7s" % ("place", "shape", "dtype", "torch med", "torch min", "fused med",
                                                        "fused min", "ratio")]
    for place in PLACES:
        for shape in SHAPES:
            for dtype in DTYPES:
                r = time_pair(sides(place, shape, dtype), a.reps, a.warmup)
                lines.append("  %-9s %-11s %-9s %9.1f %9.1f %9.1f %9.1f %7.2f" % (
                    place, "%dx%d" % shape, str(dtype)[6:], r["torch"][0], r["torch"][1], r["fused"][0], r["fused"][1],
                    r["torch"][0] / r["fused"][0]))
                print(lines[-1], flush=True)
    if not a.no_counts:
        lines.append("# kernel launches per call at %dx%d float32 (rocprofv3 --kernel-trace --stats, calls of a 20-iteration run "
                     "minus those of a 10-iteration run, / 10)" % SHAPES[0])
        for place in PLACES:
            for side in ("torch", "fused"):
                n = (kernel_calls(place, side, 20) - kernel_calls(place, side, 10)) / 10.0
                lines.append("  %-9s %-5s %5.1f" % (place, side, n))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
