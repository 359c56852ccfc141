#!/usr/bin/env python3
"""Times mhaq_amd.od_loss (decode, assignment, loss) forward plus backward with HIP events against the eager fp32 restatement
of the same criterion (tests/od_loss_ref.py with assign_ref, torch autograd) on the same device, alternating the two.
Shape: B = 16, a 640^2 input (A = 8400), nc = 80, 40 boxes per image.  Prints one JSON line; needs an MI355X."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mhaq_amd import od_loss as OL  # noqa: E402
from tests import od_loss_ref as R  # noqa: E402
from tests.od_assign_ref import assign_ref, make_case  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--boxes", type=int, default=40)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("od_loss_time.py measures on the GPU only: no device found")
    gt = {n: t.cuda() for n, t in make_case(1, a.size, (a.boxes,) * a.batch, a.boxes, a.nc).items()}
    outs = [o.cuda().requires_grad_(True) for o in R.head_outputs(1, a.size, R.S3, a.batch, a.nc, torch.float32)]
    go = torch.ones(3, device="cuda")

    def kernels():
        r = OL.od_loss(outs, R.S3, gt["gt_labels"], gt["gt_bboxes"], gt["mask_gt"], a.nc)
        return torch.stack((r["loss_box"], r["loss_cls"], r["loss_dfl"]))

    def eager():
        d = R.decode_ref([o.detach() for o in outs], R.S3)
        rec = assign_ref(dict(gt, pd_scores=d["pd_scores"], pd_bboxes=d["pd_bboxes"], anc_points=d["anc_points"]), a.nc, 10, 0.5,
                         6.0, dtype=torch.float32)
        rec["scores_sum"] = rec["scores_sum"].reshape(1)
        return R.loss_ref(outs, R.S3, rec, gt["gt_bboxes"])

    times = {"kernels": [], "eager": []}
    for it in range(a.warmup + a.iters):
        for name, fn in (("kernels", kernels), ("eager", eager)):
            for o in outs:
                o.grad = None
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            (fn() * go).sum().backward()
            t1.record()
            t1.synchronize()
            if it >= a.warmup:
                times[name].append(t0.elapsed_time(t1))
    q = lambda v: [round(x, 4) for x in statistics.quantiles(v, n=10)[::8]]      # the 10th and 90th percentile
    med = {n: statistics.median(v) for n, v in times.items()}
    print(json.dumps({"tool": "od_loss_time", "device": torch.cuda.get_device_name(0), "B": a.batch, "A": outs[0].shape[2] ** 2
                      + outs[1].shape[2] ** 2 + outs[2].shape[2] ** 2, "nc": a.nc, "boxes": a.boxes, "iters": a.iters,
                      "kernels_ms_median": round(med["kernels"], 4), "kernels_ms_p10_p90": q(times["kernels"]),
                      "eager_ms_median": round(med["eager"], 4), "eager_ms_p10_p90": q(times["eager"]),
                      "speedup_median": round(med["eager"] / med["kernels"], 2)}))


if __name__ == "__main__":
    main()
