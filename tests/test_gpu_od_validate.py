"""GPU (-m gpu): QATTrainer.validate_step with task "od" -- the detection record of the trainer's own eval output (NMS and COCO
matching, mhaq_amd/od_metrics.py) and OdValidationMeter over two batches -- against the oracle (tests/od_ref.py) on the same
predictions: the record on bits, the mean average precision within 1e-13 (101 fp64 terms that are ratios of small integers,
summed in possibly another order)."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import od_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC, H, W = 3, 8, 10                       # A = 80 anchors
BIT_WIDTH_KEYS = ["mean_weights_bit_width", "actual_weights_bit_width", "actual_weights_max_bit_width",
                  "mean_activations_bit_width", "actual_activations_bit_width", "actual_activations_max_bit_width", "converged"]


class TinyHead(nn.Module):
    """A stand-in for the YOLO head in eval mode: a 3 x 3 convolution (the layer the trainer quantizes; it leaves 1 x 1
    convolutions alone), a 1 x 1 convolution and a reshape to [B, 4 + nc, A], boxes in pixels, scores through a sigmoid."""

    def __init__(self):
        super().__init__()
        self.body = nn.Conv2d(3, 8, 3, padding=1)
        self.act = nn.ReLU()
        self.head = nn.Conv2d(8, 4 + NC, 1)

    def forward(self, x):
        y = self.head(self.act(self.body(x))).flatten(2)
        return torch.cat([y[:, 0:2] * 25 + 30, y[:, 2:4].abs() * 20 + 4, torch.sigmoid(y[:, 4:] * 4)], 1)


def _trainer(**kw):
    import mhaq_amd as M
    from mhaq_amd import ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(0)
    ops.manual_seed(1)
    calib = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(9)).to(DEV)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=8, weight_bit=8, distillation=False,
                    excluded_layers=(), task="od", **kw)
    return QATTrainer(TinyHead(), cfg, DEV, calib_batches=[calib], distributed=False)


def _targets(out, seed):
    """Ground truth cut from the prediction itself: per image a few of its boxes in xyxy, some exact, some moved, labelled
    with their best class, and one box of a class of its own far away."""
    g = torch.Generator().manual_seed(seed)
    out = out.float().cpu()
    targets = []
    for b in range(out.shape[0]):
        pick = torch.randperm(out.shape[2], generator=g)[:5 + b]
        cx, cy, w, h = (out[b, i, pick] for i in range(4))
        boxes = torch.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
        boxes = boxes + (torch.rand(boxes.shape, generator=g) - 0.5) * torch.tensor([0.0, 2.0, 4.0, 0.0, 1.0, 3.0])[:5 + b, None]
        labels = out[b, 4:, pick].argmax(0)
        targets.append({"boxes": torch.cat([boxes, torch.tensor([[500.0, 500.0, 520.0, 520.0]])]),
                        "labels": torch.cat([labels, torch.tensor([(b + 1) % NC])])})
    return targets


def test_validate_step_records_the_detections_of_the_trainers_own_eval_output():
    from mhaq_amd.od_metrics import OdValidationMeter, check_od_flags, od_decode
    tr = _trainer(od_conf_thr=0.3, od_iou_thr=0.5, od_max_det=20)
    outs = []
    hook = tr.net.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone()))
    meter, batches = OdValidationMeter(num_classes=NC), []
    g = torch.Generator().manual_seed(4)
    try:
        for step in range(2):
            x = torch.randn(2, 3, H, W, generator=g).to(DEV)
            tr.module.eval()
            with torch.no_grad():
                targets = _targets(tr.net(x), seed=step)
            tr.module.train()
            outs.clear()
            rec = tr.validate_step(x, targets)
            assert list(rec) == ["det", "det_count", "tp", "gt_labels", "gt_offsets", "metric_flags", "val_loss"] + BIT_WIDTH_KEYS
            assert rec["val_loss"].dim() == 0 and float(rec["val_loss"]) == 0.0 and check_od_flags(rec["metric_flags"]) == 0
            assert len(outs) == 1 and tuple(outs[0].shape) == (2, 4 + NC, H * W)
            ref = R.nms(R.to_f32(outs[0]), conf_thr=0.3, iou_thr=0.5, max_det=20)
            gt_box = torch.cat([t["boxes"] for t in targets]).numpy()
            gt_label = torch.cat([t["labels"] for t in targets]).numpy()
            gt_off = np.cumsum([0] + [len(t["labels"]) for t in targets])
            ref_tp, _ = R.match(ref["det"], ref["count"], gt_box, gt_label, gt_off, NC)
            assert torch.equal(rec["det"].cpu().view(torch.int32), torch.from_numpy(ref["det"].view(np.int32)))
            assert torch.equal(rec["det_count"].cpu(), torch.from_numpy(ref["count"])) and int(ref["count"].min()) > 2
            assert torch.equal(rec["tp"].cpu(), torch.from_numpy(ref_tp)) and ref_tp.any()
            assert torch.equal(rec["gt_labels"].cpu(), torch.from_numpy(gt_label)) and rec["gt_offsets"].tolist() == gt_off.tolist()
            dec = od_decode(rec)
            assert [len(d["scores"]) for d in dec] == ref["count"].tolist() and dec[0]["labels"].dtype == torch.int64
            meter.update(rec)
            batches.append((ref["det"], ref["count"], ref_tp, gt_label))
    finally:
        hook.remove()
    got, want = meter.compute(), R.mean_ap(batches)
    print("mAP", got["mAP"], want["mAP"], "mAP_50", got["mAP_50"], want["mAP_50"])
    assert 0.0 < want["mAP"] < want["mAP_50"] <= 1.0
    assert abs(got["mAP"] - want["mAP"]) <= 1e-13 and abs(got["mAP_50"] - want["mAP_50"]) <= 1e-13


def test_the_detection_head_runs_under_autocast_on_the_16_bit_output():
    tr = _trainer(autocast_dtype=torch.bfloat16, od_conf_thr=0.3)
    outs = []
    hook = tr.net.register_forward_hook(lambda m, i, o: outs.append(o.detach().clone()))
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)
    try:
        rec = tr.validate_step(x, [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.int64)}] * 2)
    finally:
        hook.remove()
    ref = R.nms(R.to_f32(outs[0]), conf_thr=0.3)
    assert torch.equal(rec["det"].cpu().view(torch.int32), torch.from_numpy(ref["det"].view(np.int32)))
    assert torch.equal(rec["det_count"].cpu(), torch.from_numpy(ref["count"])) and not rec["tp"].any()


def test_classification_record_keeps_its_keys():
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=4, weight_bit=4,
                    excluded_layers=("features.init_block.conv", "output"), warmup=2, distillation=False)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4, 3, 32, 32, generator=g).to(DEV)
    y = torch.randint(0, 10, (4,), generator=g).to(DEV)
    tr = QATTrainer(nets.resnet20_cifar(10), cfg, DEV, calib_batches=[x], distributed=False)
    rec = tr.validate_step(x, y)
    assert list(rec) == ["val_loss", "top1"] + BIT_WIDTH_KEYS
