"""The detection validation contract of include/mhaq_fq.h (mhaq_fq_od_keys / _nms / _match) and OdValidationMeter's average
precision, restated in plain numpy: fp32 elementwise arithmetic in explicit np.float32 steps, the greedy sweep as a double
loop over the sorted candidates, the accumulation in fp64.  Shares no code with mhaq_amd/od_metrics.py."""
import numpy as np
import torch

F = np.float32
NO_KEY = np.iinfo(np.int64).max
THRESHOLDS = np.linspace(0.5, 0.95, 10)


def to_f32(t):
    """A tensor (any float dtype) as float32 numpy: the conversion up is exact."""
    return t.detach().cpu().to(torch.float32).numpy()


def _min(p, q):
    return q if q < p else p


def _max(p, q):
    return q if p < q else p


def iou32(bi, ai, bj, aj):
    """The contract's overlap of box i (the kept box / the detection) and box j, every step one fp32 operation."""
    with np.errstate(all="ignore"):
        iw = _max(F(0), F(_min(bi[2], bj[2]) - _max(bi[0], bj[0])))
        ih = _max(F(0), F(_min(bi[3], bj[3]) - _max(bi[1], bj[1])))
        inter = F(iw * ih)
        return F(inter / F(F(ai + aj) - inter))


def area32(b):
    with np.errstate(all="ignore"):
        return F(F(b[2] - b[0]) * F(b[3] - b[1]))


def sweep(boxes, iou_thr, max_keep=None):
    """Greedy suppression over boxes already in order (areas taken on the boxes as given).  -> (kept indices, walked)."""
    areas = [area32(b) for b in boxes]
    kept, walked = [], 0
    thr = F(iou_thr)
    for j in range(len(boxes)):
        if max_keep is not None and len(kept) == max_keep:
            break
        walked = j + 1
        ok = True
        for i in kept:
            if iou32(boxes[i], areas[i], boxes[j], areas[j]) > thr:
                ok = False
                break
        if ok:
            kept.append(j)
    return kept, walked


def sorted_candidates(img, conf_thr):
    """img: [4 + nc, A] float32 -> the (a, c, score) of the candidates in the contract's order, through the 64-bit keys."""
    nc, A = img.shape[0] - 4, img.shape[1]
    s = img[4:]
    with np.errstate(invalid="ignore"):
        cand = s > F(conf_thr)
    c, a = np.nonzero(cand)
    bits = s[c, a].view(np.int32).astype(np.int64)
    assert (bits >= 0).all()
    keys = ((np.int64(0x7FFFFFFF) - bits) << np.int64(32)) | (a.astype(np.int64) * nc + c)
    assert len(set(keys.tolist())) == keys.size and (keys < NO_KEY).all()
    order = np.argsort(keys, kind="stable")
    return a[order], c[order], s[c, a][order]


def boxes_of(img, a, c, max_wh):
    """-> (un-offset xyxy [n, 4], offset xyxy [n, 4]) in fp32 steps."""
    with np.errstate(all="ignore"):
        cx, cy, w, h = (img[i, a].astype(F) for i in range(4))
        hw, hh = (w / F(2)).astype(F), (h / F(2)).astype(F)
        box = np.stack([cx - hw, cy - hh, cx + hw, cy + hh], 1).astype(F)
        o = (c.astype(F) * F(max_wh)).astype(F)
        return box, (box + o[:, None]).astype(F)


def nms(pred, conf_thr=0.001, iou_thr=0.65, max_det=100, max_nms=30000, max_wh=7680.0):
    """pred: float32 numpy [B, 4 + nc, A] -> dict of det [B, max_det, 6], count [B], n_cand [B], flags (int)."""
    B = pred.shape[0]
    det = np.zeros((B, max_det, 6), dtype=F)
    count, n_cand, flags = np.zeros(B, np.int32), np.zeros(B, np.int32), 0
    for b in range(B):
        a, c, s = sorted_candidates(pred[b], conf_thr)
        n_cand[b] = a.size
        if a.size > max_nms:
            flags |= 2
        a, c, s = a[:max_nms], c[:max_nms], s[:max_nms]
        box, obox = boxes_of(pred[b], a, c, max_wh)
        kept, walked = sweep(list(obox), iou_thr, max_det)
        if not np.isfinite(box[:walked]).all():
            flags |= 1
        count[b] = len(kept)
        for r, j in enumerate(kept):
            det[b, r, :4], det[b, r, 4], det[b, r, 5] = box[j], s[j], F(c[j])
    return {"det": det, "count": count, "n_cand": n_cand, "flags": flags}


def match(det, count, gt_box, gt_label, gt_off, nc):
    """-> (tp int32 [B, max_det] with bit k = matched at THRESHOLDS[k], flag bit 4 or 0)."""
    B, max_det = det.shape[0], det.shape[1]
    tp = np.zeros((B, max_det), np.int32)
    gt_box = np.asarray(gt_box, dtype=F).reshape(-1, 4)
    flag = 4 if any(int(v) < 0 or int(v) >= nc for v in gt_label) else 0
    for b in range(B):
        gs = range(int(gt_off[b]), int(gt_off[b + 1]))
        for k, T in enumerate(THRESHOLDS):
            taken = set()
            for d in range(int(count[b])):
                cls, db = int(det[b, d, 5]), det[b, d, :4]
                best, best_g = None, -1
                for g in gs:
                    if int(gt_label[g]) != cls or g in taken:
                        continue
                    v = iou32(db, area32(db), gt_box[g], area32(gt_box[g]))
                    if not float(v) >= T:
                        continue
                    if best_g < 0 or v >= best:
                        best, best_g = v, g
                if best_g >= 0:
                    taken.add(best_g)
                    tp[b, d] |= 1 << k
    return tp, flag


def average_precision(scores, hit, npig):
    """One class, one threshold: scores / hit of its detections over all images in order; fp64."""
    nd = len(scores)
    if nd == 0:
        return 0.0
    order = sorted(range(nd), key=lambda i: -float(scores[i]))       # python's sort is stable
    tp = fp = 0.0
    rc, pr = [], []
    for i in order:
        if hit[i]:
            tp += 1.0
        else:
            fp += 1.0
        rc.append(tp / npig)
        pr.append(tp / (tp + fp + np.spacing(1)))
    for i in range(nd - 1, 0, -1):
        pr[i - 1] = max(pr[i - 1], pr[i])
    total = 0.0
    for r in np.linspace(0.0, 1.0, 101):
        i = int(np.searchsorted(np.asarray(rc), r, side="left"))
        total += pr[i] if i < nd else 0.0
    return total / 101.0


def mean_ap(batches):
    """batches: list of (det [B, max_det, 6], count [B], tp [B, max_det], gt_label [G]) numpy -> {"mAP", "mAP_50"}."""
    per_class, npig = {}, {}
    for det, count, tp, gt_label in batches:
        for v in gt_label:
            npig[int(v)] = npig.get(int(v), 0) + 1
        for b in range(det.shape[0]):
            for d in range(int(count[b])):
                per_class.setdefault(int(det[b, d, 5]), []).append((float(det[b, d, 4]), int(tp[b, d])))
    if not npig:
        return {"mAP": -1.0, "mAP_50": -1.0}
    ap = []
    for c in sorted(npig):
        rows = per_class.get(c, [])
        ap.append([average_precision([s for s, _ in rows], [(t >> k) & 1 for _, t in rows], npig[c]) for k in range(10)])
    ap = np.asarray(ap, dtype=np.float64)
    return {"mAP": float(ap.mean()), "mAP_50": float(ap[:, 0].mean())}


def make_pred(boxes_per_image, nc, A, dtype=torch.float32):
    """A prediction tensor [B, 4 + nc, A] from per-image lists of (anchor, cx, cy, w, h, {class: score}); every other score 0."""
    B = len(boxes_per_image)
    p = torch.zeros(B, 4 + nc, A, dtype=torch.float32)
    for b, rows in enumerate(boxes_per_image):
        for a, cx, cy, w, h, sc in rows:
            p[b, 0, a], p[b, 1, a], p[b, 2, a], p[b, 3, a] = cx, cy, w, h
            for c, s in sc.items():
                p[b, 4 + c, a] = s
    return p.to(dtype)


def random_pred(B, nc, A, field=60.0, seed=0, frac=1.0, distinct=True):
    """Random boxes in a `field` px square with distinct scores in (0.05, 1); only a fraction `frac` of the (a, c) pairs
    scores above 0.05, the rest get 0."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(B, 4 + nc, A)
    p[:, 0:2] = torch.rand(B, 2, A, generator=g) * field
    p[:, 2:4] = torch.rand(B, 2, A, generator=g) * (field / 3) + 2.0
    n = B * nc * A
    s = (torch.randperm(n, generator=g).float() + 1.0) / (n + 1.0) * 0.9 + 0.05 if distinct else torch.rand(n, generator=g)
    s = s.reshape(B, nc, A)
    if frac < 1.0:
        s = torch.where(torch.rand(B, nc, A, generator=g) < frac, s, torch.zeros(()))
    p[:, 4:] = s
    return p
