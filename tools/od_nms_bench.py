#!/usr/bin/env python3
"""The detection validation leg on one GPU, stand-alone: device time of its stages -- the key launch (mhaq_fq_od_keys), the
sort of the key rows (torch.sort, plumbing), the NMS (mhaq_fq_od_nms, two launches) -- and of the COCO matching
(mhaq_fq_od_match) on the YOLO head's output for a 640 px COCO batch, [16, 84, 8400], at the reference's conf_thr = 0.001, and
on a small one, [4, 84, 2100] (320 px).

The NMS stage's time depends on the data, so each shape is timed in two regimes of seeded synthetic predictions (boxes of
20-200 px at random places of the image):
  sparse   scores = sigmoid(1.5 * z - 10), z normal: about 2 % of the (anchor, class) pairs are candidates, below max_nms
  dense    scores uniform in (0, 1): every pair is a candidate, every image is cut to max_nms = 30000 (the worst case)
Times: HIP events around one call of a stage, --reps timed calls after --warmup, the stages in turn, over --buffers different
predictions in rotation (no call finds its own input warm in a cache); median and minimum in microseconds.  A stage is
enqueued by the host one call at a time, so a figure is the larger of its device work and its enqueue time.
usage: tools/od_nms_bench.py [--out FILE] [--reps R] [--warmup W] [--buffers N]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mhaq_amd import ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [(16, 84, 8400, 640.0), (4, 84, 2100, 320.0)]
REGIMES = ["sparse", "dense"]
CONF, IOU, MAX_WH, MAX_NMS, MAX_DET = 0.001, 0.65, 7680.0, 30000, 100
GT_PER_IMAGE = 8


def prediction(shape, regime, seed):
    B, rows, A, px = shape
    g = torch.Generator().manual_seed(seed)
    p = torch.empty(B, rows, A)
    p[:, 0:2] = torch.rand(B, 2, A, generator=g) * px
    p[:, 2:4] = torch.rand(B, 2, A, generator=g) * 180 + 20
    if regime == "dense":
        p[:, 4:] = torch.rand(B, rows - 4, A, generator=g)
    else:
        p[:, 4:] = torch.sigmoid(torch.randn(B, rows - 4, A, generator=g) * 1.5 - 10)
    return p.to(DEV)


def ground_truth(shape, seed):
    B, rows, _, px = shape
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(B * GT_PER_IMAGE, 2, generator=g) * (px - 200)
    wh = torch.rand(B * GT_PER_IMAGE, 2, generator=g) * 180 + 20
    box = torch.cat([xy, xy + wh], 1).to(DEV)
    label = torch.randint(0, rows - 4, (B * GT_PER_IMAGE,), generator=g).to(DEV)
    off = (torch.arange(B + 1) * GT_PER_IMAGE).to(DEV)
    return box, label, off


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, 1e3 * a.elapsed_time(b)


def bench(shape, regime, reps, warmup, nbuf):
    preds = [prediction(shape, regime, 100 + i) for i in range(nbuf)]
    gt_box, gt_label, gt_off = ground_truth(shape, 7)
    nc = shape[1] - 4
    t = {k: [] for k in ("keys", "sort", "nms", "match")}
    info = None
    for i in range(warmup + reps):
        pred = preds[i % nbuf]
        keys, t_keys = timed(lambda: ops.od_keys(pred, CONF))
        skeys, t_sort = timed(lambda: torch.sort(keys, dim=1).values)
        (det, count, n_cand, flags), t_nms = timed(lambda: ops.od_nms_sorted(pred, skeys, IOU, MAX_WH, MAX_NMS, MAX_DET))
        _, t_match = timed(lambda: ops.od_match(det, count, gt_box, gt_label, gt_off, nc, flags))
        if i >= warmup:
            for k, v in zip(t, (t_keys, t_sort, t_nms, t_match)):
                t[k].append(v)
        if info is None:
            info = (float(n_cand.float().mean()), float(count.float().mean()), int(flags.item()))
    return {k: (statistics.median(v), min(v)) for k, v in t.items()}, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--buffers", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/od_nms_bench.py measures device time: it needs an MI355X (nothing is measured without one)")
    lines = ["# tools/od_nms_bench.py --reps %d --warmup %d --buffers %d: HIP events, microseconds; conf_thr %g, iou_thr %g, "
             "max_nms %d, max_det %d, float32, %d ground-truth boxes per image"
             % (a.reps, a.warmup, a.buffers, CONF, IOU, MAX_NMS, MAX_DET, GT_PER_IMAGE),
             "# %-14s %-7s %10s %8s %5s | %9s %9s | %9s %9s | %9s %9s | %9s %9s | %10s"
             % ("shape", "regime", "candidates", "kept", "flags", "keys med", "keys min", "sort med", "sort min", "nms med",
                "nms min", "match med", "match min", "sort share")]
    for shape in SHAPES:
        for regime in REGIMES:
            r, (cand, kept, flags) = bench(shape, regime, a.reps, a.warmup, a.buffers)
            three = r["keys"][0] + r["sort"][0] + r["nms"][0]
            lines.append("  %-14s %-7s %10.0f %8.1f %5d | %9.1f %9.1f | %9.1f %9.1f | %9.1f %9.1f | %9.1f %9.1f | %9.0f%%"
                         % ("%dx%dx%d" % shape[:3], regime, cand, kept, flags, *r["keys"], *r["sort"], *r["nms"], *r["match"],
                            100.0 * r["sort"][0] / three))
            print(lines[-1], flush=True)
    lines.append("# candidates / kept: means per image of the first prediction; sort share: the sort's median over the sum of "
                 "the three stages' medians")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
