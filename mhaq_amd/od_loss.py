"""Object-detection training: the YOLO criterion -- box decode, task-aligned assignment, CIoU / DFL / BCE and their backward -- as
a stream-ordered chain of HIP launches on the head's raw outputs (csrc/od_loss.hip, csrc/od_assign.hip).

The reference's `ComputeYoloLoss.__call__` cats and permutes the logits, runs a dense BCE against a target with one non-zero per
row, gathers by boolean masks and reads the device four times per step.  Here decode (one launch), the assignment (three), the
loss (two) and its backward (one) read the levels where they are, with no host read, so the step can be captured as a graph.
`od_loss` is the functional form, `ComputeYoloLoss` the drop-in for the reference's class.  include/mhaq_fq.h has the contract
and the deviations, DESIGN section 20 the launch plan.
"""
from __future__ import annotations

import torch

from . import ops
from .od_assign import od_assign


class _OdLoss(torch.autograd.Function):
    """loss [3] = (box, cls, dfl) of the head's outputs under a fixed assignment record; backward is one launch."""

    @staticmethod
    def forward(ctx, strides, nc, reg_max, gains, record, *outputs):
        fg, gi, ts, ssum, gl, gb = record
        outputs = [t.detach() for t in outputs]
        loss, denom = ops.od_loss_fwd(outputs, strides, nc, reg_max, fg, gi, ts, ssum, gl, gb, gains)
        ctx.args = (strides, nc, reg_max, gains, (fg, gi, ts, gl, gb), denom)
        ctx.save_for_backward(*outputs)
        return loss

    @staticmethod
    def backward(ctx, grad):
        strides, nc, reg_max, gains, rec, denom = ctx.args
        grads = ops.od_loss_bwd(list(ctx.saved_tensors), strides, nc, reg_max, *rec, grad.to(torch.float32).contiguous(), denom,
                                gains)
        return (None, None, None, None, None, *grads)


def od_loss(outputs, strides, gt_labels, gt_bboxes, mask_gt, nc, reg_max=16, gains=(7.5, 0.5, 1.5), top_k=10, alpha=0.5,
            beta=6.0) -> dict:
    """The criterion of a batch.  `outputs`: the head's levels, dense [B, 4 * reg_max + nc, H, W] device tensors of one dtype
    (float32, bfloat16 or float16), `strides` their strides in pixels; `gt_labels` [B, G(, 1)], `gt_bboxes` [B, G, 4] (xyxy,
    pixels) and `mask_gt` [B, G(, 1)].  Returns `loss_box`, `loss_cls`, `loss_dfl` (0-dim float32, times `gains`, with autograd
    into `outputs`) and the assigner's record (`target_bboxes`, `target_scores`, `fg_mask`, `target_gt_idx`, `scores_sum`,
    `flags`).  Nothing here waits for the device."""
    outputs = [t.contiguous() for t in outputs]
    strides = tuple(float(s) for s in strides)
    gains = tuple(float(g) for g in gains)
    with torch.no_grad():
        pd_bboxes, pd_scores, anc = ops.od_decode(outputs, strides, nc, reg_max)
        rec = od_assign(pd_scores, pd_bboxes, anc, gt_labels, gt_bboxes, mask_gt, nc, top_k, alpha, beta)
        b = pd_scores.shape[0]
        gl = gt_labels.detach().reshape(b, -1).to(torch.float32).contiguous()
        gb = gt_bboxes.detach().to(torch.float32).contiguous()
    loss = _OdLoss.apply(strides, int(nc), int(reg_max), gains,
                         (rec["fg_mask"], rec["target_gt_idx"], rec["target_scores"], rec["scores_sum"], gl, gb), *outputs)
    box, cls, dfl = loss.unbind(0)
    return {"loss_box": box, "loss_cls": cls, "loss_dfl": dfl, **rec}


class ComputeYoloLoss(torch.nn.Module):
    """The reference's `ComputeYoloLoss`: its constructor (`model.head` gives `stride`, `nc`, `no`, `ch`; `params` the gains
    `box`, `cls`, `dfl`), its `__call__(outputs, targets)` with `targets = {"idx", "labels", "boxes"}` (boxes as normalised
    xywh), its three results.  The whole result of the last call stays on `self.last`."""

    def __init__(self, model, params, device="cuda:0"):
        super().__init__()
        head = (model.module if hasattr(model, "module") else model).head
        self.params = params
        self.stride = head.stride
        self.nc = head.nc
        self.no = head.no
        self.reg_max = head.ch
        self.device = device
        self.last = None

    def targets_to_rows(self, outputs, targets):
        """[B, G, 5] rows (label, xyxy in pixels) padded with zeros, G = the largest count of an image, and their mask."""
        b = outputs[0].shape[0]
        idx = targets["idx"].reshape(-1).to(self.device)
        rows = torch.cat((targets["labels"].reshape(-1, 1).to(self.device), targets["boxes"].reshape(-1, 4).to(self.device)),
                         1).to(torch.float32)
        if rows.shape[0] == 0:
            gt = torch.zeros(b, 0, 5, device=self.device)
        else:
            counts = torch.bincount(idx.long(), minlength=b)
            gt = torch.zeros(b, int(counts.max()), 5, device=self.device)       # the one host read, as in the reference
            order = torch.argsort(idx, stable=True)
            first = torch.cumsum(counts, 0) - counts
            slot = torch.arange(rows.shape[0], device=self.device) - first[idx[order].long()]
            gt[idx[order].long(), slot] = rows[order]
            h, w = (float(v) * float(self.stride[0]) for v in outputs[0].shape[2:])
            cx, cy, bw, bh = (gt[..., 1] * w, gt[..., 2] * h, gt[..., 3] * w, gt[..., 4] * h)
            gt = torch.stack((gt[..., 0], cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), -1)
        return gt, (gt[..., 1:].sum(2, keepdim=True) > 0).to(torch.float32)

    def forward(self, outputs, targets):
        gt, mask_gt = self.targets_to_rows(outputs, targets)
        self.last = od_loss(list(outputs), [float(s) for s in self.stride], gt[..., :1], gt[..., 1:], mask_gt, self.nc,
                            self.reg_max, (self.params["box"], self.params["cls"], self.params["dfl"]))
        return self.last["loss_box"], self.last["loss_cls"], self.last["loss_dfl"]
