"""A plain torch restatement of the task-aligned assignment's contract (include/mhaq_fq.h, mhaq_fq_od_assign) with its fixed
tie rules, and the seeded cases its tests share.  It runs in the dtype it is given on inputs upcast exactly."""
import math

import torch

STRIDES = (8, 16, 32)
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# id: (seed, image size, valid ground truth per image, rows G, nc, top_k, alpha, beta, prediction dtype); the seeds are chosen
# so that margin >= 1e-3 (assign_ref)
CASES = {
    "a84-below-one-tile-b3": (1, 64, (4, 0, 2), 4, 80, 10, 0.5, 6.0, F32),
    "a84-b3-padded-rows-k13-alpha1": (2, 64, (7, 3, 0), 7, 80, 13, 1.0, 6.0, F32),
    "a525-crosses-tiles-b3": (3, 160, (7, 4, 0), 7, 80, 10, 0.5, 6.0, F32),
    "a525-b1-g1-nc1-k1": (4, 160, (1,), 1, 1, 1, 0.5, 6.0, F32),
    "a10-equals-k-b3": (5, 24, (3, 0, 1), 3, 80, 10, 0.5, 6.0, F32),
    "b1-g0": (6, 64, (0,), 0, 80, 10, 0.5, 6.0, F32),
    "bf16-a525-b3": (7, 160, (7, 2, 0), 7, 80, 10, 0.5, 6.0, BF16),
    "f16-a84-b3-alpha1": (8, 64, (7, 5, 0), 7, 80, 10, 1.0, 6.0, F16),
    "nc3-scalar-stores-b3": (9, 160, (7, 1, 0), 7, 3, 10, 0.5, 6.0, F32),
    "a21504-lds-above-64k-b3": (10, 1024, (4, 0, 1), 4, 80, 13, 1.0, 6.0, F32),
    "g300-packed-count-word-b3": (72, 160, (300, 0, 5), 300, 80, 10, 0.5, 6.0, F32),
}
# The edges of the exponents, of top_k and of the expand kernel's row length (tests/test_gpu_od_assign_edges.py): the fields of
# CASES and a tweak that edge_case() applies -- "zero": every third anchor's scores are exactly 0; "tie": no tweak, but the
# outcome rests on the library's tie rule, so the row has no margin and the reference's Assigner cannot be compared (with
# alpha == beta == 0 every in-box metric is 1, and torch.topk's choice among equals is unspecified).
EDGE_CASES = {
    "exp-powf-0.75-2.5": (21, 160, (7, 3, 0), 7, 80, 10, 0.75, 2.5, F32, None),
    "exp-odd-3-identity-1": (22, 160, (7, 3, 0), 7, 80, 10, 3.0, 1.0, F32, None),
    "exp-odd-7-5": (21, 160, (7, 3, 0), 7, 80, 10, 7.0, 5.0, F32, None),
    "exp-2-last-integer-64": (22, 160, (7, 3, 0), 7, 80, 10, 2.0, 64.0, F32, None),
    "exp-2-powf-65": (22, 160, (7, 3, 0), 7, 80, 10, 2.0, 65.0, F32, None),
    "exp-alpha0-zero-scores": (23, 160, (7, 3, 0), 7, 80, 10, 0.0, 6.0, F32, "zero"),
    "exp-beta0": (163, 160, (7, 3, 0), 7, 80, 10, 0.5, 0.0, F32, None),
    "exp-6-sqrt-beta": (21, 160, (7, 3, 0), 7, 80, 10, 6.0, 0.5, F32, None),
    "exp-both-0": (21, 160, (7, 3, 0), 7, 80, 10, 0.0, 0.0, F32, "tie"),
    "exp-bf16-powf-0.75-2.5": (21, 160, (7, 3, 0), 7, 80, 10, 0.75, 2.5, BF16, None),
    "k32-full-selection": (21, 160, (7, 3, 0), 7, 80, 32, 0.5, 6.0, F32, None),
    "nc2-scalar-rows-shorter-than-a-store": (21, 160, (7, 3, 0), 7, 2, 10, 0.5, 6.0, F32, None),
    "nc4-one-store-per-row": (21, 160, (7, 3, 0), 7, 4, 10, 0.5, 6.0, F32, None),
    "nc5-scalar-odd-rows": (21, 160, (7, 3, 0), 7, 5, 10, 0.5, 6.0, F32, None),
    "nc8-two-stores-per-row": (21, 160, (7, 3, 0), 7, 8, 10, 0.5, 6.0, F32, None),
}


def edge_case(name):
    """-> (case, nc, top_k, alpha, beta, needs a margin) of a row of EDGE_CASES."""
    seed, size, counts, g, nc, k, alpha, beta, dtype, tweak = EDGE_CASES[name]
    c = make_case(seed, size, counts, g, nc)
    if tweak == "zero":
        c["pd_scores"][:, ::3] = 0.0
    c["pd_scores"], c["pd_bboxes"] = c["pd_scores"].to(dtype), c["pd_bboxes"].to(dtype)
    return c, nc, k, alpha, beta, tweak != "tie"


def anchors(size):
    """Pixel centres of the strides' cells at offset 0.5: 84 anchors for a 64^2 image, 525 for 160^2, 10 for 24^2."""
    pts = []
    for s in STRIDES:
        n = size // s
        c = (torch.arange(n, dtype=torch.float32) + 0.5) * s
        yy, xx = torch.meshgrid(c, c, indexing="ij")
        pts.append(torch.stack((xx, yy), -1).view(-1, 2))
    return torch.cat(pts)


def make_case(seed, size, counts, max_g, nc, dtype=torch.float32):
    """Seeded inputs: predictions jittered around the anchors; per image `counts[i]` ground-truth boxes padded to `max_g` rows
    with mask 0 -- two large overlapping ones (many anchors, multi-assignment), one smaller than a stride cell, random ones."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=gen)
    anc = anchors(size)
    a, b = anc.shape[0], len(counts)
    half = size * (0.08 + 0.25 * rnd(b, a, 4))
    pd_bboxes = torch.cat((anc - half[..., :2], anc + half[..., 2:]), -1) + size * 0.03 * (rnd(b, a, 4) - 0.5)
    pd_scores = torch.sigmoid(2.0 * torch.randn(b, a, nc, generator=gen))
    gt_bboxes, gt_labels, mask = torch.zeros(b, max_g, 4), torch.zeros(b, max_g, 1), torch.zeros(b, max_g, 1)
    for i, n in enumerate(counts):
        for j in range(n):
            if j == 0:
                box = torch.tensor([0.07, 0.11, 0.83, 0.78]) * size
            elif j == 1:
                box = torch.tensor([0.23, 0.19, 0.96, 0.93]) * size
            elif j == 2:
                c = size * (0.2 + 0.6 * rnd(2))
                box = torch.cat((c - 1.5, c + 1.5))
            else:
                c, wh = size * (0.25 + 0.5 * rnd(2)), size * (0.1 + 0.2 * rnd(2))
                box = torch.cat((c - wh, c + wh))
            gt_bboxes[i, j], gt_labels[i, j], mask[i, j] = box, float(torch.randint(nc, (1,), generator=gen)), 1.0
    return {"pd_scores": pd_scores.to(dtype), "pd_bboxes": pd_bboxes.to(dtype), "anc_points": anc, "gt_labels": gt_labels,
            "gt_bboxes": gt_bboxes, "mask_gt": mask}


def ciou(box1, box2, eps=1e-7):
    """compute_iou of the reference (yolo_loss.py:20-46), CIoU, in its order of operations."""
    x1, y1, x2, y2 = box1.unbind(-1)
    p1, q1, p2, q2 = box2.unbind(-1)
    w1, h1, w2, h2 = x2 - x1, y2 - y1 + eps, p2 - p1, q2 - q1 + eps
    inter = (torch.minimum(x2, p2) - torch.maximum(x1, p1)).clamp(0) * (torch.minimum(y2, q2) - torch.maximum(y1, q1)).clamp(0)
    iou = inter / (w1 * h1 + w2 * h2 - inter + eps)
    cw, ch = torch.maximum(x2, p2) - torch.minimum(x1, p1), torch.maximum(y2, q2) - torch.minimum(y1, q1)
    c2 = cw ** 2 + ch ** 2 + eps
    rho2 = ((p1 + p2 - x1 - x2) ** 2 + (q1 + q2 - y1 - y2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)).pow(2)
    return iou - (rho2 / c2 + v * (v / (v - iou + (1 + eps))))


def assign_ref(case, nc, top_k, alpha, beta, eps=1e-9, dtype=torch.float64):
    """The contract on `case` (the tensors the kernel sees, any device) in `dtype`.  Returns the kernel's record plus `margin`."""
    sc, pb, anc = case["pd_scores"].to(dtype), case["pd_bboxes"].to(dtype), case["anc_points"].to(dtype)
    gb32 = case["gt_bboxes"].float()
    b, a, g = pb.shape[0], pb.shape[1], gb32.shape[1]
    dev = pb.device
    out = {"target_bboxes": torch.zeros(b, a, 4, device=dev), "target_scores": torch.zeros(b, a, nc, dtype=dtype, device=dev),
           "fg_mask": torch.zeros(b, a, dtype=torch.bool, device=dev), "scores_sum": torch.zeros((), dtype=dtype, device=dev),
           "target_gt_idx": torch.zeros(b, a, dtype=torch.int64, device=dev), "flags": 0, "margin": math.inf}
    if g == 0 or b * a == 0:
        return out
    gb, lab, masked = gb32.to(dtype), case["gt_labels"].reshape(b, g).to(dtype), case["mask_gt"].reshape(b, g) != 0
    lab_ok = (lab >= 0) & (lab < nc)
    valid = masked & lab_ok
    d = torch.cat((anc[None, None] - gb[:, :, None, :2], gb[:, :, None, 2:] - anc[None, None]), -1)
    inb = d.amin(-1) > eps
    score = sc.transpose(1, 2).gather(1, torch.where(lab_ok, lab, 0).long()[:, :, None].expand(b, g, a))
    finite = torch.isfinite(pb).all(-1)[:, None] & torch.isfinite(gb).all(-1)[:, :, None] & torch.isfinite(score)
    pair = inb & valid[:, :, None]
    ok = pair & finite
    zero = torch.zeros((), dtype=dtype, device=dev)
    ov = torch.where(ok, ciou(gb[:, :, None], pb[:, None]).clamp(0), zero)
    m = torch.where(ok, torch.where(ok, score, zero).pow(alpha) * ov.pow(beta), zero)
    order = torch.sort(m, dim=-1, descending=True, stable=True)          # ties: the lower anchor index first
    chosen = torch.zeros(b, g, a, dtype=torch.bool, device=dev).scatter_(2, order.indices[..., :top_k], True)
    pos = chosen & pair
    multi = pos.sum(1) > 1
    first = torch.zeros_like(pos).scatter_(1, ov.argmax(1, keepdim=True), True)      # argmax: the first maximum
    pos = torch.where(multi[:, None], first, pos)
    fg, gi = pos.any(1), pos.int().argmax(1)
    bi = torch.arange(b, device=dev)[:, None]
    # step 6; a NaN label is class 0 and one beyond int32 its largest value (both lie outside [0, nc) or on an invalid row)
    label = torch.nan_to_num(lab[bi, gi], nan=0.0, posinf=2.0 ** 31, neginf=0.0).clamp(0, 2.0 ** 31).long()
    mp = m * pos
    pam, pov = mp.amax(-1, keepdim=True), (ov * pos).amax(-1, keepdim=True)
    norm = torch.where(mp > 0, mp * pov / (pam + eps), zero).amax(1)          # step 8: 0 where m is 0, also with eps == 0
    hit = fg & (label < nc)
    out["target_scores"][hit.nonzero(as_tuple=True) + (label[hit],)] = norm[hit]
    out.update(target_bboxes=gb32[bi, gi], fg_mask=fg, target_gt_idx=gi, scores_sum=norm.sum(),
               flags=(1 if bool((pair & ~finite).any()) else 0) | (4 if bool((masked & ~lab_ok).any()) else 0))
    if a > top_k:                                 # (i) the gap between the k-th and the (k+1)-th metric of a valid ground truth
        kth, nxt = order.values[..., top_k - 1], order.values[..., top_k]
        sel = valid & (kth > 0)
        if bool(sel.any()):
            out["margin"] = float(((kth - nxt) / kth)[sel].min())
    if bool(multi.any()) and g > 1:               # (ii) the gap between the two largest overlaps of a multi-assigned anchor
        top2 = ov.topk(2, dim=1).values
        sel = multi & (top2[:, 0] > 0)
        if bool(sel.any()):
            out["margin"] = min(out["margin"], float(((top2[:, 0] - top2[:, 1]) / top2[:, 0])[sel].min()))
    return out


def predictions(anc, b, nc, seed, extent):
    """pd_scores [b, A, nc] and pd_bboxes [b, A, 4] jittered around the anchors `anc`, as make_case draws them."""
    gen = torch.Generator().manual_seed(seed)
    a = anc.shape[0]
    half = extent * (0.08 + 0.25 * torch.rand(b, a, 4, generator=gen))
    pd_bboxes = torch.cat((anc - half[..., :2], anc + half[..., 2:]), -1) + extent * 0.03 * (torch.rand(b, a, 4, generator=gen) - 0.5)
    return torch.sigmoid(2.0 * torch.randn(b, a, nc, generator=gen)), pd_bboxes


def hand_case(anc, nc, rows, g, seed=0, extent=160.0, far=False):
    """One image on the anchors `anc` with the ground truth `rows` = {row index: (box, label, mask)} among `g` rows, every
    other row zeros with mask 0.  `far`: every prediction lies far from every box (all overlaps are 0)."""
    sc, pb = predictions(anc, 1, nc, seed, extent)
    if far:
        pb = torch.tensor([9000.0, 9000.0, 9010.0, 9010.0]).expand(1, anc.shape[0], 4).clone()
    gt_bboxes, gt_labels, mask = torch.zeros(1, g, 4), torch.zeros(1, g, 1), torch.zeros(1, g, 1)
    for j, (box, label, m) in rows.items():
        gt_bboxes[0, j], gt_labels[0, j], mask[0, j] = torch.tensor(box, dtype=torch.float32), label, m
    return {"pd_scores": sc, "pd_bboxes": pb, "anc_points": anc.clone(), "gt_labels": gt_labels, "gt_bboxes": gt_bboxes,
            "mask_gt": mask}


def grid(nx, ny, stride=8.0):
    """A hand-made anchor grid: nx * ny cell centres at one stride, row by row."""
    yy, xx = torch.meshgrid((torch.arange(ny, dtype=torch.float32) + 0.5) * stride,
                            (torch.arange(nx, dtype=torch.float32) + 0.5) * stride, indexing="ij")
    return torch.stack((xx, yy), -1).view(-1, 2)


def run(case, nc, k, alpha, beta, eps=1e-9):
    """The kernels on `case`: -> (the case on the device, the record of mhaq_amd.od_assign)."""
    from mhaq_amd import od_assign as OA
    dev = {n: t.cuda() for n, t in case.items()}
    return dev, OA.od_assign(dev["pd_scores"], dev["pd_bboxes"], dev["anc_points"], dev["gt_labels"], dev["gt_bboxes"],
                             dev["mask_gt"], nc, k, alpha, beta, eps)


def check(rec, dev, nc, k, alpha, beta, need_margin, eps=1e-9, label=""):
    """Discrete outputs equal the fp64 restatement; continuous ones lie within twice the error of the framework's own fp32
    chain (the restatement in fp32 on the same device) against fp64."""
    from tests.sr_metrics_ref import within_bar
    r64 = assign_ref(dev, nc, k, alpha, beta, eps)
    r32 = assign_ref(dev, nc, k, alpha, beta, eps, dtype=torch.float32)
    if need_margin:
        assert r64["margin"] >= 1e-3                     # a condition on the inputs, not a tolerance on the kernel
    for name in ("fg_mask", "target_gt_idx", "target_bboxes"):
        assert torch.equal(rec[name].to(r64[name].dtype), r64[name]), name
    assert torch.equal(rec["target_scores"] != 0, r64["target_scores"] != 0)
    assert int(rec["flags"].item()) == r64["flags"]
    ts, ts32, ts64 = (r["target_scores"].double() for r in (rec, r32, r64))
    err, bar = float((ts - ts64).abs().max()) if ts.numel() else 0.0, float((ts32 - ts64).abs().max()) if ts.numel() else 0.0
    ok, frac = within_bar(rec["scores_sum"], r32["scores_sum"], r64["scores_sum"], 1.0)  # its own bar + 8 ulp32, as for
    print(f"bars {label}: target_scores kernel {err:.3e} fp32 chain {bar:.3e} fraction of 2x {err / (2 * bar) if bar else 0.0:.3f}; "
          f"scores_sum fraction {frac:.3f}")                                             # every scalar of this suite
    assert err <= 2 * bar and ok
    return r64
