"""Object-detection training: the YOLO task-aligned target assignment as HIP kernels (csrc/od_assign.hip).

What the reference's `Assigner.forward` does per step -- about sixty eager launches over ten [B, G, A] tensors, a Python loop
of `top_k` scatters and a host read of the device -- comes out of three launches with no host synchronisation and no
[B, G, A] array, so a step with this assigner inside can be captured as a graph.  `Assigner` is a drop-in for the reference's
module (`loss.assigner = mhaq_amd.od_assign.Assigner(nc, top_k=10, alpha=0.5, beta=6.0)`); `od_assign` returns the whole
record.  include/mhaq_fq.h has the contract and the deviations, DESIGN section 19 the launch plan.
"""
from __future__ import annotations

import torch

from . import ops
from .od_metrics import FLAG_LABEL_RANGE, FLAG_NONFINITE, check_od_flags  # noqa: F401  (the flag word's bits and its reader)


def _rows(t: torch.Tensor, b: int, name: str) -> torch.Tensor:
    """[B, G] float32 from the reference's [B, G, 1] (or [B, G]) labels / mask."""
    if t.dim() == 3 and t.shape[2] == 1:
        t = t.reshape(t.shape[0], t.shape[1])
    if t.dim() != 2 or t.shape[0] != b:
        raise ValueError(f"{name} must be [B, G] or [B, G, 1]")
    return t.to(torch.float32).contiguous()


def od_assign(pd_scores: torch.Tensor, pd_bboxes: torch.Tensor, anc_points: torch.Tensor, gt_labels: torch.Tensor,
              gt_bboxes: torch.Tensor, mask_gt: torch.Tensor, nc: int, top_k: int = 10, alpha: float = 0.5, beta: float = 6.0,
              eps: float = 1e-9) -> dict:
    """The assignment of a batch.  `pd_scores` [B, A, nc] (sigmoided) and `pd_bboxes` [B, A, 4] (xyxy, pixels) are float32,
    bfloat16 or float16 device tensors of one dtype; `anc_points` [A, 2], `gt_labels` [B, G(, 1)], `gt_bboxes` [B, G, 4] and
    `mask_gt` [B, G(, 1)] are taken as float32.  Returns device tensors: `target_bboxes` [B, A, 4] and `target_scores`
    [B, A, nc] (float32), `fg_mask` [B, A] (bool), `target_gt_idx` [B, A] (int32), `scores_sum` [1] (float32, the sum of
    `target_scores`) and `flags` (one int32 word for check_od_flags).  Nothing here waits for the device."""
    for t in (pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt):
        if not isinstance(t, torch.Tensor):
            raise TypeError("every input must be a tensor")
    if pd_scores.dim() != 3 or pd_scores.shape[2] != int(nc):
        raise ValueError(f"pd_scores must be [B, A, {int(nc)}], got {list(pd_scores.shape)}")
    b = pd_scores.shape[0]
    tb, ts, fg, gi, ssum, flags = ops.od_assign(
        pd_scores.detach().contiguous(), pd_bboxes.detach().contiguous(), anc_points.detach().to(torch.float32).contiguous(),
        _rows(gt_labels.detach(), b, "gt_labels"), gt_bboxes.detach().to(torch.float32).contiguous(),
        _rows(mask_gt.detach(), b, "mask_gt"), top_k, alpha, beta, eps)
    return {"target_bboxes": tb, "target_scores": ts, "fg_mask": fg, "target_gt_idx": gi, "scores_sum": ssum, "flags": flags}


class Assigner(torch.nn.Module):
    """The reference's `Assigner`: its constructor, its `forward`, its three results.  The whole record of the last call
    (`scores_sum`, `flags`, `target_gt_idx` besides the three) is kept on `self.last`."""

    def __init__(self, nc=80, top_k=13, alpha=1.0, beta=6.0, eps=1e-9):
        super().__init__()
        self.top_k = top_k
        self.nc = nc
        self.alpha = alpha
        self.beta = beta
        self.eps = eps
        self.last = None

    @torch.no_grad()
    def forward(self, pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt):
        self.last = od_assign(pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt, self.nc, self.top_k, self.alpha,
                              self.beta, self.eps)
        return self.last["target_bboxes"], self.last["target_scores"], self.last["fg_mask"]
