#!/usr/bin/env python3
"""The super-resolution validation metrics on one GPU, stand-alone: the framework's chain (tests/sr_metrics_ref.py: chain32 --
div, L1, clamp, luminance, PSNR, average pool, five 11 x 11 depthwise convolutions, the SSIM maps and their means) against
mhaq_amd.sr_metrics.sr_metrics (three HIP launches), in one process on the same tensors.

Shapes: 1x3x1356x2040 (a DIV2K validation image, pool factor 5), 1x3x512x512 (factor 2), 1x3x256x256 and 24x3x96x96.
Times: HIP events around one call, --reps timed calls after --warmup, alternating the two sides; median and minimum in
microseconds.  Every call takes the next of a ring of (sr, hr) pairs that together exceed the 256 MB Infinity Cache, so that
neither side reads its inputs out of a cache the previous call filled.  Both sides are enqueued by the host one op at a time: a
figure is the larger of the device work and the host's enqueue time of that side.
Bytes: the fused side's algorithmic traffic -- one read of sr and hr, the pooled planes written and read once -- over its
median time.
Launches: counted by `rocprofv3 --kernel-trace --stats` runs of this file's own (--count-child: K and 2K iterations of one
side, the difference of the kernel calls / K), no counters in those runs.
usage: tools/sr_metrics_bench.py [--out FILE] [--reps R] [--warmup W] [--no-counts]"""
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

from mhaq_amd.sr_metrics import sr_metrics, ssim_pool_factor  # noqa: E402
from tests import sr_metrics_ref as R  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 3, 1356, 2040), (1, 3, 512, 512), (1, 3, 256, 256), (24, 3, 96, 96)]
RING_BYTES = 300e6


def ring(shape, dtype=torch.float32, limit=256):
    """(sr, hr) pairs on the device, more than the Infinity Cache holds in total."""
    n, c, h, w = shape
    pair = 2 * n * c * h * w * torch.empty(0, dtype=dtype).element_size()
    count = max(2, min(limit, int(RING_BYTES // pair) + 1))
    sr, hr = R.images(n, c, h, w, noise=0.05, seed=h + w)
    sr, hr = sr.to(DEV).to(dtype), hr.to(DEV).to(dtype)
    return [(sr + 0.001 * i, hr.clone()) for i in range(count)]


def sides(pairs):
    state = {"torch": 0, "fused": 0}

    def nxt(k):
        state[k] = (state[k] + 1) % len(pairs)
        return pairs[state[k]]

    def run_torch():
        return R.chain32(*nxt("torch"))

    def run_fused():
        return sr_metrics(*nxt("fused"))
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


def algorithmic_bytes(shape, esize=4, luminance=True):
    n, c, h, w = shape
    f = ssim_pool_factor(h, w)
    p = 1 if luminance else c
    return 2 * n * c * h * w * esize + 2 * (2 * n * p * (h // f) * (w // f) * 4)


def count_child(side, shape_index, iters):
    import warnings
    warnings.simplefilter("ignore")
    fn = sides(ring(SHAPES[shape_index], limit=2))[side]
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()


def kernel_calls(side, shape_index, iters):
    """Kernel launches of a --count-child run, from rocprofv3's kernel statistics."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--count-child", side, str(shape_index), str(iters)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel_stats.csv")
        return sum(int(row["Calls"]) for f in files for row in csv.DictReader(open(f)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-counts", action="store_true")
    ap.add_argument("--count-child", nargs=3, metavar=("SIDE", "SHAPE", "ITERS"))
    a = ap.parse_args()
    if a.count_child:
        return count_child(a.count_child[0], int(a.count_child[1]), int(a.count_child[2]))
    import warnings
    warnings.simplefilter("ignore")
    lines = ["# tools/sr_metrics_bench.py --reps %d --warmup %d: one validation record, HIP events, microseconds; float32, luminance"
             % (a.reps, a.warmup),
             "# %-16s %4s %5s %10s %10s %10s %10s %7s %9s %10s" % ("shape", "pool", "pairs", "torch med", "torch min",
                                                                   "fused med", "fused min", "ratio", "alg MB", "fused GB/s")]
    for shape in SHAPES:
        pairs = ring(shape)
        r = time_pair(sides(pairs), a.reps, a.warmup)
        nbytes = algorithmic_bytes(shape)
        lines.append("  %-16s %4d %5d %10.1f %10.1f %10.1f %10.1f %7.2f %9.2f %10.1f" % (
            "%dx%dx%dx%d" % shape, ssim_pool_factor(shape[2], shape[3]), len(pairs), r["torch"][0], r["torch"][1],
            r["fused"][0], r["fused"][1], r["torch"][0] / r["fused"][0], nbytes / 1e6, nbytes / (r["fused"][0] * 1e-6) / 1e9))
        print(lines[-1], flush=True)
        del pairs
        torch.cuda.empty_cache()
    if not a.no_counts:
        lines.append("# kernel launches per record (rocprofv3 --kernel-trace --stats, calls of a 20-iteration run minus those of a "
                     "10-iteration run, / 10); the fused side's count includes the fill that clears its flag word")
        for idx in (0, 3):
            for side in ("fused", "torch"):
                n = (kernel_calls(side, idx, 20) - kernel_calls(side, idx, 10)) / 10.0
                lines.append("  %-16s %-6s %5.1f" % ("%dx%dx%dx%d" % SHAPES[idx], side, n))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
