"""GPU (-m gpu): COCO's greedy matching (mhaq_fq_od_match, csrc/od_nms.hip) through mhaq_amd.od_metrics.od_match against the
definition restated in numpy (tests/od_ref.py).  The results are integers (one bit per IoU threshold) and the overlaps are
singly rounded fp32 operations, so every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import od_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOX = (10.0, 10.0, 30.0, 30.0)


def device_match(det, count, targets, nc):
    """od_match on a hand-made od_nms record -> (tp numpy, flag word)."""
    from mhaq_amd.od_metrics import od_match
    rec = {"det": torch.from_numpy(det).to(DEV), "count": torch.from_numpy(count).to(DEV),
           "flags": torch.zeros(1, dtype=torch.int32, device=DEV), "num_classes": nc}
    out = od_match(rec, targets)
    assert int(rec["flags"].item()) == 0 and out["tp"].dtype == torch.int32 and out["tp"].shape == rec["det"].shape[:2]
    assert out["gt_offsets"].tolist() == np.cumsum([0] + [len(t["labels"]) for t in targets]).tolist()
    return out["tp"].cpu().numpy(), int(out["flags"].item())


def match(dets, gts, nc=3, max_det=6):
    """dets: per image [(box, score, cls)], gts: per image [(box, label)] -> (tp, flags), checked against the oracle."""
    B = len(dets)
    det, count = np.zeros((B, max_det, 6), np.float32), np.zeros(B, np.int32)
    for b, rows in enumerate(dets):
        count[b] = len(rows)
        for r, (box, s, c) in enumerate(rows):
            det[b, r, :4], det[b, r, 4], det[b, r, 5] = box, s, c
    targets = [{"boxes": torch.tensor([g[0] for g in im], dtype=torch.float32).reshape(-1, 4),
                "labels": torch.tensor([g[1] for g in im], dtype=torch.int64)} for im in gts]
    gt_box = np.asarray([g[0] for im in gts for g in im], np.float32).reshape(-1, 4)
    gt_label = np.asarray([g[1] for im in gts for g in im], np.int64)
    gt_off = np.cumsum([0] + [len(im) for im in gts])
    tp, flags = device_match(det, count, targets, nc)
    ref_tp, ref_flags = R.match(det, count, gt_box, gt_label, gt_off, nc)
    assert np.array_equal(tp, ref_tp), (tp, ref_tp)
    assert flags == ref_flags
    return tp, flags


def random_images(sizes, nc=3, max_det=12, seed=0):
    """Per image G_i random ground-truth boxes in a 100 px field and max_det detections: jittered copies of them (every
    overlap from none to exact) with classes that mostly agree, in descending score order."""
    g = torch.Generator().manual_seed(seed)
    dets, gts = [], []
    for G in sizes:
        xy = torch.rand(G, 2, generator=g) * 80
        wh = torch.rand(G, 2, generator=g) * 15 + 5
        gt = torch.cat([xy, xy + wh], 1)
        lab = torch.randint(0, nc, (G,), generator=g)
        gts.append([(gt[i].tolist(), int(lab[i])) for i in range(G)])
        rows = []
        for r in range(max_det):
            if G and r % 4 != 3:
                i = int(torch.randint(0, G, (1,), generator=g))
                box = (gt[i] + (torch.rand(4, generator=g) - 0.5) * (r % 3) * 3).tolist()
                c = int(lab[i]) if r % 5 else (int(lab[i]) + 1) % nc
            else:
                box, c = [5.0 * r, 5.0, 5.0 * r + 12, 20.0], r % nc
            rows.append((box, 0.95 - 0.05 * r, c))
        dets.append(rows)
    return dets, gts


def test_ground_truth_counts_around_the_wavefront_width():
    dets, gts = random_images([0, 1, 63, 64, 65], seed=1)
    tp, flags = match(dets, gts, max_det=12)
    assert flags == 0 and not tp[0].any() and tp[2:].any(axis=1).all()
    assert len({int(v) for v in tp.reshape(-1)}) > 3          # several different sets of thresholds occur


def test_more_ground_truth_than_two_strides_and_a_full_detection_list():
    dets, gts = random_images([150, 7], max_det=20, seed=2)
    tp, _ = match(dets, gts, max_det=20)
    assert tp.any()


def test_two_detections_compete_for_one_ground_truth():
    near = (11.0, 10.0, 31.0, 30.0)                           # IoU 19/21 with BOX
    other = (12.0, 10.0, 32.0, 30.0)                          # IoU 18/22 with BOX: the next best for the second detection
    tp, _ = match([[(BOX, 0.9, 1), (near, 0.8, 1)]], [[(BOX, 1), (other, 1)]])
    assert tp[0, 0] == 1023
    assert tp[0, 1] == 1023 & ~(1 << 9)                       # falls to `other`: 19/21 = 0.905 against it misses 0.95 only
    tp, _ = match([[(BOX, 0.9, 1), (near, 0.8, 1)]], [[(BOX, 1)]])
    assert list(tp[0, :2]) == [1023, 0]                       # ... or to none


def test_equal_iou_against_two_ground_truths_takes_the_higher_index():
    tall, wide = (0.0, 0.0, 10.0, 12.0), (0.0, 0.0, 12.0, 10.0)
    tp, _ = match([[((0.0, 0.0, 10.0, 10.0), 0.9, 0), (wide, 0.8, 0)]], [[(tall, 0), (wide, 0)]])
    # the first detection overlaps both by 100/120 and takes `wide` (index 1); the second is `wide` itself and is left
    # with `tall` (100/140 = 0.714) at the thresholds 0.5 .. 0.7; from 0.85 on the first is unmatched and `wide` is free
    assert list(tp[0, :2]) == [0b0001111111, 0b1110011111]


def test_class_mismatch_never_matches():
    tp, _ = match([[(BOX, 0.9, 1), (BOX, 0.8, 0)]], [[(BOX, 0)]])
    assert list(tp[0, :2]) == [0, 1023]


def test_a_detection_matched_at_the_three_lowest_thresholds_only():
    tp, _ = match([[((10.0, 10.0, 30.0, 22.0), 0.9, 2)]], [[(BOX, 2)]])      # IoU 0.6
    assert tp[0, 0] == 0b111
    tp, _ = match([[((0.0, 0.0, 2.0, 1.0), 0.9, 0)]], [[((0.0, 0.0, 1.0, 1.0), 0)]])      # IoU exactly 0.5: >= T_0
    assert tp[0, 0] == 1


def test_labels_out_of_range_set_bit_2_and_are_ignored():
    dets = [[(BOX, 0.9, 2), ((50.0, 50.0, 60.0, 60.0), 0.8, 0)], [(BOX, 0.7, 1)]]
    clean = [[(BOX, 2), ((50.0, 50.0, 60.0, 60.0), 0)], [(BOX, 1)]]
    dirty = [[(BOX, 3), (BOX, 2), ((50.0, 50.0, 60.0, 60.0), -1), ((50.0, 50.0, 60.0, 60.0), 0)], [(BOX, 1), (BOX, 1 << 40)]]
    tp0, f0 = match(dets, clean)
    tp1, f1 = match(dets, dirty)
    assert f0 == 0 and f1 == 4 and np.array_equal(tp0, tp1) and tp0[0, 0] == 1023


def test_images_without_detections_and_a_batch_without_ground_truth():
    dets, gts = random_images([5, 9, 4], seed=5, max_det=6)
    dets[1] = []
    tp, _ = match(dets, gts)
    assert not tp[1].any() and tp[0].any() and tp[2].any()
    tp, flags = match([[(BOX, 0.9, 0)], []], [[], []])
    assert not tp.any() and flags == 0


def test_bits_of_nms_flags_are_kept_and_calls_repeat():
    from mhaq_amd.od_metrics import od_match
    dets, gts = random_images([20, 3], seed=7, max_det=6)
    det = np.zeros((2, 6, 6), np.float32)
    for b, rows in enumerate(dets):
        for r, (box, s, c) in enumerate(rows):
            det[b, r, :4], det[b, r, 4], det[b, r, 5] = box, s, c
    targets = [{"boxes": torch.tensor([g[0] for g in im]), "labels": torch.tensor([g[1] for g in im])} for im in gts]
    targets[1]["labels"][0] = 3
    rec = {"det": torch.from_numpy(det).to(DEV), "count": torch.tensor([6, 6], dtype=torch.int32, device=DEV),
           "flags": torch.tensor([3], dtype=torch.int32, device=DEV), "num_classes": 3}
    on_device = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b = od_match(rec, on_device), od_match(rec, targets)      # host targets travel through pinned memory
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(a["flags"].item()) == 7 and int(rec["flags"].item()) == 3
    assert torch.equal(a["tp"], b["tp"]) and torch.equal(a["gt_labels"], b["gt_labels"]) and a["tp"].any()
