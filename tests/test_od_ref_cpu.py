"""CPU: the detection oracle (tests/od_ref.py) against the reference's own non_max_suppression, the closed forms of the
average precision (both the oracle's and OdValidationMeter's host arithmetic), the IoU tie rules, and the host-side argument
checks of the detection face.  Nothing here launches a kernel."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import od_ref as R

REF_NMS = "/root/reference/src/models/od/utils/yolo_nms.py"
TOL = 1e-13      # 101 fp64 terms that are ratios of small integers, summed in possibly another order


# ---------------------------------------------------------------- (a) the real reference against the oracle
@pytest.fixture(scope="module")
def reference_nms():
    path = os.environ.get("MHAQ_REFERENCE_NMS", REF_NMS)
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")

    def nms(boxes, scores, iou_threshold):                 # torchvision.ops.nms with the oracle's sweep written out
        order = np.argsort(-scores.numpy(), kind="stable")
        kept, _ = R.sweep(list(boxes.numpy()[order]), iou_threshold)
        return torch.from_numpy(order[kept].astype(np.int64))

    stand_in = types.ModuleType("torchvision")
    stand_in.ops = types.SimpleNamespace(nms=nms)
    saved = sys.modules.get("torchvision")
    sys.modules["torchvision"] = stand_in
    try:
        spec = importlib.util.spec_from_file_location("_reference_yolo_nms", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            del sys.modules["torchvision"]
        else:
            sys.modules["torchvision"] = saved
    mod.time = lambda: 0.0                                 # the wall-clock break never fires
    return mod


@pytest.mark.parametrize("nc", [1, 3, 80])
def test_reference_non_max_suppression_equals_the_oracle(reference_nms, nc):
    pred = R.random_pred(2, nc, 90, field=60.0, seed=nc, frac=1.0 if nc < 80 else 0.06)
    out = reference_nms.non_max_suppression(pred.clone(), 0.05, 0.65)
    ours = R.nms(pred.numpy(), conf_thr=0.05, iou_thr=0.65, max_det=100, max_nms=30000, max_wh=7680.0)
    assert len(out) == 2
    for b in range(2):
        n = int(ours["count"][b])
        assert n > 3 and tuple(out[b].shape) == (n, 6)
        assert np.array_equal(out[b].numpy().view(np.int32), ours["det"][b, :n].view(np.int32)), (nc, b)
    assert ours["flags"] == 0 and (ours["n_cand"] > ours["count"]).all()


def test_oracle_truncates_to_max_nms_and_flags_it():
    pred = R.random_pred(1, 1, 90, seed=5)
    full = R.nms(pred.numpy(), conf_thr=0.05, max_nms=30000)
    cut = R.nms(pred.numpy(), conf_thr=0.05, max_nms=20)
    assert full["flags"] == 0 and cut["flags"] == 2 and cut["n_cand"][0] == full["n_cand"][0] == 90
    a, c, s = R.sorted_candidates(pred[0].numpy(), 0.05)
    assert (np.diff(s) < 0).all()
    kept = set(map(float, cut["det"][0, :cut["count"][0], 4]))
    assert kept <= set(map(float, s[:20])) and cut["count"][0] <= full["count"][0]


# ---------------------------------------------------------------- (b) closed forms of the meter
def _rec(dets, gts, max_det=4):
    """dets: per image [(box, score, cls)], gts: per image [(box, label)] -> an od_match record from the oracle's matching."""
    B = len(dets)
    det, count = np.zeros((B, max_det, 6), np.float32), np.zeros(B, np.int32)
    for b, rows in enumerate(dets):
        count[b] = len(rows)
        for r, (box, s, c) in enumerate(rows):
            det[b, r, :4], det[b, r, 4], det[b, r, 5] = box, s, c
    gt_box = np.asarray([g[0] for im in gts for g in im], np.float32).reshape(-1, 4)
    gt_label = np.asarray([g[1] for im in gts for g in im], np.int64)
    gt_off = np.cumsum([0] + [len(im) for im in gts])
    tp, _ = R.match(det, count, gt_box, gt_label, gt_off, nc=8)
    return det, count, tp, gt_label


def _both(batches):
    """mAP / mAP_50 of the oracle and of OdValidationMeter's host arithmetic on the same records."""
    from mhaq_amd.od_metrics import OdValidationMeter
    ref = R.mean_ap(batches)
    m = OdValidationMeter()
    for det, count, tp, lab in batches:
        m.update({"det": torch.from_numpy(det), "count": torch.from_numpy(count), "tp": torch.from_numpy(tp),
                  "gt_labels": torch.from_numpy(lab)})
    got = m.compute()
    for k in ("mAP", "mAP_50"):
        assert abs(got[k] - ref[k]) <= TOL, (k, got[k], ref[k])
    return ref


BOX = [10.0, 10.0, 30.0, 30.0]


def test_one_exact_detection_scores_one():
    r = _both([_rec([[(BOX, 0.9, 2)]], [[(BOX, 2)]])])
    assert abs(r["mAP"] - 1.0) <= TOL and abs(r["mAP_50"] - 1.0) <= TOL


def test_iou_of_0p6_counts_at_three_thresholds():
    det_box = [10.0, 10.0, 30.0, 22.0]                      # 20 x 12 inside 20 x 20: IoU 0.6
    rec = _rec([[(det_box, 0.9, 0)]], [[(BOX, 0)]])
    assert rec[2][0, 0] == 0b111
    r = _both([rec])
    assert abs(r["mAP_50"] - 1.0) <= TOL and abs(r["mAP"] - 0.3) <= TOL


def test_tp_fp_tp_over_two_ground_truths():
    far = [100.0, 100.0, 120.0, 120.0]
    box2 = [50.0, 50.0, 70.0, 70.0]
    rec = _rec([[(BOX, 0.9, 1), (far, 0.8, 1), (box2, 0.7, 1)]], [[(BOX, 1), (box2, 1)]])
    assert list(rec[2][0, :3]) == [1023, 0, 1023]
    r = _both([rec])
    want = (51 + 50 * (2.0 / 3.0)) / 101
    assert abs(r["mAP"] - want) <= TOL and abs(r["mAP_50"] - want) <= TOL


def test_a_class_without_detections_halves_the_mean_and_no_ground_truth_gives_minus_one():
    r = _both([_rec([[(BOX, 0.9, 2)]], [[(BOX, 2), (BOX, 5)]])])
    assert abs(r["mAP"] - 0.5) <= TOL and abs(r["mAP_50"] - 0.5) <= TOL
    r = _both([_rec([[(BOX, 0.9, 2)]], [[]])])
    assert r == {"mAP": -1.0, "mAP_50": -1.0}


def test_detections_of_two_updates_are_ranked_together():
    a = _rec([[(BOX, 0.5, 0)]], [[(BOX, 0)]])
    b = _rec([[([100.0, 100.0, 120.0, 120.0], 0.9, 0)]], [[(BOX, 0)]])      # a higher-scored false positive, later batch
    r = _both([a, b])
    # ranked FP, TP over two ground truths: recall 0, 0.5; precision 0, 0.5 -> 51 samples of 0.5
    assert abs(r["mAP_50"] - 51 * 0.5 / 101) <= TOL


def test_thresholds_are_numpy_linspace():
    from mhaq_amd import od_metrics
    assert np.array_equal(od_metrics.IOU_THRESHOLDS, R.THRESHOLDS) and R.THRESHOLDS[8] != 0.9


# ---------------------------------------------------------------- (c) the IoU tie rule
def test_iou_of_exactly_one_half_is_not_suppressed_and_is_matched():
    wide, unit = np.asarray([0, 0, 2, 1], np.float32), np.asarray([0, 0, 1, 1], np.float32)
    assert R.iou32(wide, R.area32(wide), unit, R.area32(unit)) == np.float32(0.5)
    kept, _ = R.sweep([wide, unit], 0.5)
    assert kept == [0, 1]                                   # strict comparison
    kept, _ = R.sweep([wide, unit], np.nextafter(np.float32(0.5), np.float32(0)))
    assert kept == [0]
    det = np.zeros((1, 2, 6), np.float32)
    det[0, 0] = [0, 0, 2, 1, 0.9, 0]
    tp, flag = R.match(det, np.asarray([1], np.int32), unit[None], np.asarray([0]), np.asarray([0, 1]), nc=1)
    assert tp[0, 0] == 1 and flag == 0                      # >= at T_0, and at no higher threshold


def test_zero_area_pair_is_nan_and_does_not_suppress():
    p = np.asarray([5, 5, 5, 5], np.float32)
    assert np.isnan(R.iou32(p, R.area32(p), p, R.area32(p)))
    assert R.sweep([p, p], 0.0)[0] == [0, 1]


# ---------------------------------------------------------------- (d) host-side argument checks
def test_od_needs_a_gpu_and_unknown_tasks_are_still_refused():
    import dataclasses

    from torch import nn

    from mhaq_amd import _lib
    from mhaq_amd.od_metrics import check_od_flags, od_nms
    from mhaq_amd.qat import QATConfig, QATTrainer
    cfg = QATConfig()
    assert (cfg.task, cfg.od_conf_thr, cfg.od_iou_thr, cfg.od_max_det) == ("cls", 0.001, 0.65, 100)
    assert {"od_conf_thr", "od_iou_thr", "od_max_det"} <= {f.name for f in dataclasses.fields(QATConfig)}
    with pytest.raises(_lib.MhaqFqError, match="od"):
        QATTrainer(nn.Conv2d(3, 7, 1), QATConfig(task="od", distillation=False), "cpu")
    with pytest.raises(ValueError, match=r'"cls", "sr" or "od"'):
        QATTrainer(nn.Conv2d(3, 7, 1), QATConfig(task="detect"), "cpu")
    with pytest.raises(_lib.MhaqFqError, match="no CPU fallback by design"):
        od_nms(torch.zeros(1, 7, 16))
    assert check_od_flags(torch.tensor([3], dtype=torch.int32)) == 3
    with pytest.raises(FloatingPointError):
        check_od_flags(torch.tensor([1], dtype=torch.int32), nonfinite=True)
    with pytest.raises(ValueError):
        check_od_flags(torch.tensor([4], dtype=torch.int32))


def test_library_refuses_bad_detection_arguments_before_any_launch():
    import ctypes

    from mhaq_amd import _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)
    W = L.mhaq_fq_od_nms_chunk()
    assert W >= 64 and W % 64 == 0
    assert L.mhaq_fq_od_keys(None, 0, 1, 3, 8, 0.1, fake, None) == -1
    assert L.mhaq_fq_od_keys(fake, 3, 1, 3, 8, 0.1, fake, None) == -1
    assert L.mhaq_fq_od_keys(fake, 0, 1, 3, 8, -0.1, fake, None) == -1
    assert L.mhaq_fq_od_keys(fake, 0, 1, 3, 8, float("nan"), fake, None) == -1
    assert L.mhaq_fq_od_keys(odd, 0, 1, 3, 8, 0.1, fake, None) == -3
    assert L.mhaq_fq_od_keys(fake, 0, 1, 3, 1 << 30, 0.1, fake, None) == -4
    ws = L.mhaq_fq_od_nms_workspace_bytes(2)
    assert ws >= 8
    nms = lambda **k: L.mhaq_fq_od_nms(fake, 0, fake, 2, 3, 8, k.get("iou", 0.65), 7680.0, k.get("max_nms", 30000),      # noqa: E731
                                       k.get("max_det", 100), k.get("det", fake), fake, fake, fake, fake, k.get("ws", ws), None)
    assert nms(max_det=0) == -1 and nms(max_nms=0) == -1 and nms(iou=float("nan")) == -1
    assert nms(ws=4) == -2 and nms(det=odd) == -3 and nms(max_det=1025) == -4
    mws = L.mhaq_fq_od_match_workspace_bytes(5)
    assert mws >= 50 and L.mhaq_fq_od_match_workspace_bytes(0) == 0
    assert L.mhaq_fq_od_match(fake, fake, 2, 100, 3, None, fake, fake, 5, fake, fake, fake, mws, None) == -1
    assert L.mhaq_fq_od_match(fake, fake, 2, 100, 3, fake, fake, fake, 5, fake, fake, fake, 8, None) == -2
    assert L.mhaq_fq_od_match(fake, fake, 2, 100, 3, fake, odd, fake, 5, fake, fake, fake, mws, None) == -3
    assert L.mhaq_fq_od_match(fake, fake, 2, 2000, 3, fake, fake, fake, 5, fake, fake, fake, mws, None) == -4
