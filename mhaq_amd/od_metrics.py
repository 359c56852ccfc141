"""Object-detection validation: the YOLO head's non-maximum suppression and COCO's matching of its output against the ground
truth as HIP kernels (csrc/od_nms.hip), and the mean average precision the reference logs from them.

What the reference's detection validation step does per batch (`MeanAveragePrecisionYolo.update(self.forward(x), target)`:
`non_max_suppression` -- a host loop over the images with several synchronisations each and a wall-clock break --,
`decode_yolo_nms`, a metrics library's COCO evaluation) comes out of `od_nms` and `od_match` with no host synchronisation;
the host reads are `od_decode`, `check_od_flags` and `OdValidationMeter.compute`.  DESIGN section 18 has the contract and the
measurements.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

FLAG_NONFINITE = 1      # bit 0: a NaN or infinite box coordinate among the candidates that were walked
FLAG_TRUNCATED = 2      # bit 1: an image had more than max_nms candidates
FLAG_LABEL_RANGE = 4    # bit 2: a ground-truth label outside [0, nc)

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)      # T_k of od_match's bit k


def od_nms(pred: torch.Tensor, conf_thr: float = 0.001, iou_thr: float = 0.65, max_det: int = 100, max_nms: int = 30000,
           max_wh: float = 7680.0) -> dict:
    """Non-maximum suppression of a batch.  `pred` is what the YOLO head returns in eval mode: a contiguous [B, 4 + nc, A]
    tensor on the GPU (float32, bfloat16 or float16), rows 0-3 cx, cy, w, h in pixels, rows 4.. the sigmoided class scores.
    Returns device tensors: `det` ([B, max_det, 6] float32: x1, y1, x2, y2, score, class in kept order, zero rows beyond the
    count), `count` and `n_candidates` ([B] int32) and `flags` (one int32 word for check_od_flags), and `num_classes` (the
    host integer od_match needs).  The defaults are the reference's.  Nothing here waits for the device."""
    if not isinstance(pred, torch.Tensor):
        raise TypeError("pred must be a tensor")
    det, count, n_cand, flags = ops.od_nms(pred.detach(), conf_thr, iou_thr, max_wh, max_nms, max_det)
    return {"det": det, "count": count, "n_candidates": n_cand, "flags": flags, "num_classes": pred.shape[1] - 4}


def od_decode(rec: dict) -> list:
    """The per-image `boxes` [n, 4] / `scores` [n] / `labels` [n] (int64) dicts a metrics library is handed (the reference's
    decode_yolo_nms).  Reads `count`: one host synchronisation."""
    det = rec["det"]
    count = rec["det_count"] if "det_count" in rec else rec["count"]
    out = []
    for d, n in zip(det, count.tolist()):
        out.append({"boxes": d[:n, :4], "scores": d[:n, 4], "labels": d[:n, 5].to(torch.int64)})
    return out


def _to_device(t: torch.Tensor, dev, dtype) -> torch.Tensor:
    """`t` on `dev` as `dtype`; a host tensor goes through pinned memory, so that the copy is enqueued and the host goes on
    (a plain .to() of pageable memory waits for the stream)."""
    if t.device.type == "cpu" and t.numel():
        t = t.to(dtype).pin_memory()
        return t.to(dev, non_blocking=True)
    return t.to(device=dev, dtype=dtype)


def od_match(rec: dict, target: list) -> dict:
    """COCO's greedy matching of od_nms' record against the ground truth of its batch.  `target` is the list of
    {"boxes": [G_i, 4] xyxy, "labels": [G_i]} dicts of the images (tensors on any device); the offsets come from their shapes
    on the host, so nothing waits for the device.  Returns what `rec` held plus `tp` ([B, max_det] int32, bit k = matched at
    IOU_THRESHOLDS[k]), `gt_labels` ([G] int64), `gt_offsets` ([B + 1] int64) and `flags` with bit 2 OR-ed in (a new word:
    rec's own is left alone)."""
    det = rec["det"]
    if len(target) != det.shape[0]:
        raise ValueError(f"target has {len(target)} images, the record {det.shape[0]}")
    dev = det.device
    offs = [0]
    for t in target:
        if t["boxes"].shape[0] != t["labels"].shape[0] or (t["boxes"].shape[0] and tuple(t["boxes"].shape[1:]) != (4,)):
            raise ValueError("a target's boxes must be [G_i, 4] and its labels [G_i]")
        offs.append(offs[-1] + int(t["labels"].shape[0]))
    boxes = [_to_device(t["boxes"].detach().reshape(-1, 4), dev, torch.float32) for t in target]
    labels = [_to_device(t["labels"].detach().reshape(-1), dev, torch.int64) for t in target]
    gt_box = torch.cat(boxes).contiguous() if offs[-1] else torch.zeros((0, 4), dtype=torch.float32, device=dev)
    gt_label = torch.cat(labels).contiguous() if offs[-1] else torch.zeros((0,), dtype=torch.int64, device=dev)
    gt_off = _to_device(torch.tensor(offs, dtype=torch.int64), dev, torch.int64)
    flags = rec["flags"].clone()
    tp = ops.od_match(det, rec["count"], gt_box, gt_label, gt_off, rec["num_classes"], flags)
    return {**rec, "tp": tp, "gt_labels": gt_label, "gt_offsets": gt_off, "flags": flags}


def check_od_flags(flags: torch.Tensor, nonfinite: bool = False) -> int:
    """The one host read of a record's flag word: raises ValueError when a ground-truth label lay outside [0, nc) and, only if
    `nonfinite` is set, FloatingPointError when a candidate box had a NaN or infinite coordinate.  Returns the word."""
    word = int(flags.reshape(-1)[0].item())
    if word & FLAG_LABEL_RANGE:
        raise ValueError("a ground-truth label is outside [0, num_classes)")
    if nonfinite and word & FLAG_NONFINITE:
        raise FloatingPointError("a candidate box has a NaN or infinite coordinate")
    return word


def _average_precision(scores: np.ndarray, tp: np.ndarray, npig: int) -> float:
    """pycocotools' accumulate for one class and one threshold: `scores` / `tp` (bool) of the class's detections in image
    order, `npig` its ground-truth boxes."""
    if scores.size == 0:
        return 0.0
    order = np.argsort(-scores, kind="mergesort")
    hit = tp[order]
    tps, fps = np.cumsum(hit, dtype=np.float64), np.cumsum(~hit, dtype=np.float64)
    recall = tps / npig
    precision = tps / (fps + tps + np.spacing(1))
    for i in range(precision.size - 1, 0, -1):
        if precision[i] > precision[i - 1]:
            precision[i - 1] = precision[i]
    idx = np.searchsorted(recall, np.linspace(0.0, 1.0, 101), side="left")
    q = np.zeros(101, dtype=np.float64)
    ok = idx < precision.size
    q[ok] = precision[idx[ok]]
    return float(np.mean(q))


class OdValidationMeter:
    """Keeps the small device tensors of the validation batches' records (`update` never waits for the device) and forms
    COCO's `mAP` (IoU 0.50:0.95) and `mAP_50` over all of them in `compute`: one host read, then float64 on the host
    (pycocotools' accumulate for area = all, maxDets = the records' max_det).  A record is what od_match returns (`det`,
    `count`, `tp`, `gt_labels`) or what QATTrainer.validate_step returns for task "od" (`det_count` for `count`).
    `num_classes`, if given, drops ground-truth labels at or above it (negative ones are always dropped): the boxes od_match
    ignored and flagged."""

    def __init__(self, num_classes: int | None = None):
        self.num_classes = num_classes
        self.reset()

    def reset(self) -> None:
        self._recs = []

    def update(self, rec: dict) -> None:
        count = rec["det_count"] if "det_count" in rec else rec["count"]
        self._recs.append((rec["det"].detach(), count.detach(), rec["tp"].detach(), rec["gt_labels"].detach()))

    def compute(self) -> dict:
        if not self._recs:
            return {}
        parts, sizes = [], []
        for det, count, tp, lab in self._recs:                   # everything as int32 words: one tensor, one copy
            for t in (det[..., 4:6].contiguous(), count.contiguous(), tp.contiguous(), lab.contiguous()):
                w = t.reshape(-1).view(torch.int32) if t.numel() else t.new_empty(0, dtype=torch.int32)
                parts.append(w)
                sizes.append(w.numel())
        host = torch.cat(parts).cpu().numpy()                    # the one host read
        scores, classes, hits, labels = [], [], [], []
        pos = 0
        for r, (det, _, _, _) in enumerate(self._recs):
            b, m = det.shape[0], det.shape[1]
            words = []
            for j in range(4):
                words.append(host[pos:pos + sizes[4 * r + j]])
                pos += sizes[4 * r + j]
            sc = words[0].view(np.float32).reshape(b, m, 2)
            n = words[1]
            tp = words[2].reshape(b, m)
            labels.append(words[3].view(np.int64))
            for i in range(b):
                scores.append(sc[i, :n[i], 0])
                classes.append(sc[i, :n[i], 1].astype(np.int64))
                hits.append(tp[i, :n[i]])
        scores, classes, hits, labels = (np.concatenate(v) for v in (scores, classes, hits, labels))
        labels = labels[labels >= 0]
        if self.num_classes is not None:
            labels = labels[labels < self.num_classes]
        if labels.size == 0:
            return {"mAP": -1.0, "mAP_50": -1.0}
        ap = []
        for c in np.unique(labels):
            sel = classes == c
            npig = int(np.sum(labels == c))
            s, h = scores[sel].astype(np.float64), hits[sel]
            ap.append([_average_precision(s, ((h >> k) & 1).astype(bool), npig) for k in range(len(IOU_THRESHOLDS))])
        ap = np.asarray(ap, dtype=np.float64)
        return {"mAP": float(np.mean(ap)), "mAP_50": float(np.mean(ap[:, 0]))}
