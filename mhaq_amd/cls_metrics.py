"""Classification validation: cross-entropy, top-1 and top-k accuracy of a batch in two HIP launches (csrc/cls_head.hip).

What the reference's classification validation step logs (vision_cls_module.py:17-26, 67-77 -- the criterion, then
torchmetrics' `Accuracy_top1` and `Accuracy_top5`) comes out of one call on the logits, with no host synchronisation; the
one host read is `check_cls_flags`.  DESIGN section 17 has the definitions and the measurements.
"""
from __future__ import annotations

import torch

from . import _lib
from . import ops

FLAG_NONFINITE = 2     # bit 1: the nll of a valid row is not finite
FLAG_TARGET_RANGE = 4  # bit 2: a label that is neither ignore_index nor in [0, C)


def cls_metrics(logits: torch.Tensor, target: torch.Tensor, topk: int = 5, ignore_index: int = -100) -> dict:
    """Loss and accuracy of a batch.  `logits` is [..., C] on the GPU (float32, bfloat16 or float16; seen as [-1, C]),
    `target` the int64 labels of its rows.  Returns device tensors: `loss` (0-dim, the mean cross-entropy over the rows
    whose label is not `ignore_index`), `Accuracy_top1` and `Accuracy_top5` (0-dim; the second is the top-`topk` accuracy
    and keeps the reference's key name whatever `topk` is), `counts` ([3] int64: valid rows, top-1 hits, top-k hits), `nll`
    and `rank` ([rows]; the label's position in a stable descending sort of its row, C on ignored rows) and `flags` (one
    int32 word for check_cls_flags).  Nothing here waits for the device."""
    for t, name in ((logits, "logits"), (target, "target")):
        if not t.is_cuda:
            raise _lib.MhaqFqError(f"{name} is on {t.device}: the classification head runs only as HIP kernels on an "
                                   "MI355X (no CPU fallback by design)")
    if logits.dim() < 1:
        raise ValueError("logits must have at least one dimension")
    c = logits.shape[-1]
    x = logits.detach().reshape(-1, c).contiguous()
    y = target.detach().reshape(-1).contiguous()
    loss, acc, counts, nll, rank, flags = ops.cls_head(x, y, topk, ignore_index, True)
    return {"loss": loss[0], "Accuracy_top1": acc[0], "Accuracy_top5": acc[1], "counts": counts, "nll": nll, "rank": rank,
            "flags": flags}


def check_cls_flags(flags: torch.Tensor, nonfinite: bool = False) -> int:
    """The one host read of a record: raises IndexError when a label lay out of range (the framework's CPU message; on
    the device its own loss aborts the process there) and, only if `nonfinite` is set, FloatingPointError when the nll of
    a valid row was not finite.  Returns the flag word."""
    word = int(flags.reshape(-1)[0].item())
    if word & FLAG_TARGET_RANGE:
        raise IndexError("Target (a label that is neither ignore_index nor in [0, C)) is out of bounds.")
    if nonfinite and word & FLAG_NONFINITE:
        raise FloatingPointError("the cross-entropy of a row is not finite: a NaN or an infinity in its logits")
    return word


class ClsValidationMeter:
    """Sums of the per-batch counts and of loss * valid rows over the validation batches, kept as tensors on the
    records' device (`update` never waits for the device).  `compute` gives `Accuracy_top1`, `Accuracy_top5` and
    `val_loss` as ratios of the accumulated sums: the batch-size-weighted means of the per-batch values, which is what
    the reference's logger forms over an epoch.  A record is what cls_metrics returns (`loss`, `counts`) or what
    QATTrainer.validate_step returns with cls_metrics on (`val_loss`, `correct`)."""

    def __init__(self):
        self.reset()

    def reset(self) -> None:
        self._counts = None      # [3] int64: valid rows, top-1 hits, top-k hits
        self._loss = None        # 0-dim float64: sum over batches of loss * valid rows

    def update(self, rec: dict) -> None:
        counts = rec["correct"] if "correct" in rec else rec["counts"]
        loss = rec["val_loss"] if "val_loss" in rec else rec["loss"]
        counts = counts.detach().to(torch.int64)
        v = counts[0]
        # a batch without a valid row has a NaN loss and weight 0: it adds nothing
        part = torch.where(v > 0, loss.detach().double() * v.double(), torch.zeros((), dtype=torch.float64, device=v.device))
        if self._counts is None:
            self._counts, self._loss = counts.clone(), part
        else:
            self._counts = self._counts + counts
            self._loss = self._loss + part

    def compute(self) -> dict:
        if self._counts is None:
            return {}
        v = self._counts[0].double()
        return {"Accuracy_top1": self._counts[1].double() / v, "Accuracy_top5": self._counts[2].double() / v,
                "val_loss": self._loss / v}
