"""A plain torch restatement of the detection criterion's contract (include/mhaq_fq.h: mhaq_fq_od_decode, mhaq_fq_od_loss_fwd,
mhaq_fq_od_loss_bwd) in the dtype it is given -- decode, the three losses from a given assignment record, the gradients by
autograd -- and the seeded cases its tests share."""
import functools
import math

import torch
import torch.nn.functional as F

from tests.od_assign_ref import assign_ref, make_case

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
R, GAINS, ONE, S3 = 16, (7.5, 0.5, 1.5), (1.0, 1.0, 1.0), (8, 16, 32)
# id: (seed, image size, strides, valid ground truth per image, rows G, nc, the head's dtype, grad_out); the seeds are chosen so
# that the conditions of test_gpu_od_loss.py hold on the fp64 restatement
CASES = {
    "a84-full-tile-then-two-short-levels-b3": (1, 64, S3, (4, 0, 2), 4, 80, F32, ONE),
    "a525-ragged-tiles-b3-padded-rows-grad-out": (2, 160, S3, (7, 4, 0), 7, 80, F32, (0.5, 2.0, -1.0)),
    "a1344-dfl-clamp-nc3-b1": (3, 256, S3, (4,), 4, 3, F32, ONE),
    "g0-b1": (4, 64, S3, (0,), 0, 80, F32, ONE),
    "nc1-b1": (5, 160, S3, (2,), 2, 1, F32, ONE),
    "nc130-ragged-second-class-chunk-b3": (6, 64, S3, (4, 0, 2), 4, 130, F32, ONE),
    "two-levels-a80-b2": (12, 64, (8, 16), (4, 0), 4, 3, F32, ONE),
    "bf16-a525-b3": (8, 160, S3, (7, 2, 0), 7, 80, BF16, (0.5, 2.0, -1.0)),
    "f16-a84-b3": (10, 64, S3, (4, 0, 2), 4, 80, F16, ONE),
}


def head_outputs(seed, size, strides, b, nc, dtype):
    """The head's levels [b, 4 * R + nc, n, n]: class logits 2 * randn, distribution logits peaked at a random bin."""
    gen = torch.Generator().manual_seed(1000 + seed)
    outs = []
    for s in strides:
        n = size // s
        hi = max(2, min(R, n // 2 + 1))                      # sides of about the image's scale on every level
        peak = F.one_hot(torch.randint(hi, (b, 4, n, n), generator=gen), R).permute(0, 1, 4, 2, 3)
        dist = torch.randn(b, 4, R, n, n, generator=gen) + 4.0 * peak
        outs.append(torch.cat((dist.reshape(b, 4 * R, n, n), 2.0 * torch.randn(b, nc, n, n, generator=gen)), 1).to(dtype))
    return outs


def decode_ref(outputs, strides):
    """-> dict: dist [B, A, 4 R] and cls [B, A, nc] logits, anc [A, 2] and pb [B, A, 4] in cells, st [A, 1], and the decode
    call's three outputs pd_bboxes, pd_scores, anc_points."""
    x0 = outputs[0]
    b, no = x0.shape[:2]
    x = torch.cat([o.reshape(b, no, -1) for o in outputs], 2)
    dist, cls = x[:, :4 * R].permute(0, 2, 1), x[:, 4 * R:].permute(0, 2, 1)
    anc, st = [], []
    for o, s in zip(outputs, strides):
        yy, xx = torch.meshgrid(torch.arange(o.shape[2], dtype=x0.dtype, device=x0.device) + 0.5,
                                torch.arange(o.shape[3], dtype=x0.dtype, device=x0.device) + 0.5, indexing="ij")
        anc.append(torch.stack((xx, yy), -1).view(-1, 2))
        st.append(torch.full((anc[-1].shape[0], 1), float(s), dtype=x0.dtype, device=x0.device))
    anc, st = torch.cat(anc), torch.cat(st)
    e = dist.reshape(b, -1, 4, R).softmax(3).matmul(torch.arange(R, dtype=x0.dtype, device=x0.device))
    pb = torch.cat((anc - e[..., :2], anc + e[..., 2:]), -1)
    return dict(dist=dist, cls=cls, anc=anc, st=st, pb=pb, pd_bboxes=pb * st, pd_scores=cls.sigmoid(), anc_points=anc * st)


def ciou(box1, box2, eps=1e-7):
    """compute_iou of the reference in its order of operations, alpha a constant as under its no_grad."""
    x1, y1, x2, y2 = box1.unbind(-1)
    p1, q1, p2, q2 = box2.unbind(-1)
    w1, h1, w2, h2 = x2 - x1, y2 - y1 + eps, p2 - p1, q2 - q1 + eps
    inter = (torch.minimum(x2, p2) - torch.maximum(x1, p1)).clamp(0) * (torch.minimum(y2, q2) - torch.maximum(y1, q1)).clamp(0)
    iou = inter / (w1 * h1 + w2 * h2 - inter + eps)
    cw, ch = torch.maximum(x2, p2) - torch.minimum(x1, p1), torch.maximum(y2, q2) - torch.minimum(y1, q1)
    c2 = cw ** 2 + ch ** 2 + eps
    rho2 = ((p1 + p2 - x1 - x2) ** 2 + (q1 + q2 - y1 - y2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)).pow(2)
    return iou - (rho2 / c2 + v * (v / (v - iou + (1 + eps))).detach())


def dfl_targets(d, rec, gt_bboxes):
    """-> (tb [B, A, 4] the target boxes in cells, the clamped DFL targets [B, A, 4])."""
    b, a = d["pb"].shape[:2]
    tb = torch.zeros(b, a, 4, dtype=d["pb"].dtype, device=d["pb"].device)
    if gt_bboxes.shape[1]:
        tb = gt_bboxes.to(tb.dtype)[torch.arange(b, device=tb.device)[:, None], rec["target_gt_idx"].long()] / d["st"]
    return tb, torch.cat((d["anc"] - tb[..., :2], tb[..., 2:] - d["anc"]), -1).clamp(0, R - 1 - 0.01)


def loss_ref(outputs, strides, rec, gt_bboxes, gains=GAINS):
    """-> [3]: the box, cls and dfl losses times `gains`, in the dtype of `outputs`, from the record `rec`."""
    d = decode_ref(outputs, strides)
    dtype, fg = outputs[0].dtype, rec["fg_mask"]
    ts, denom = rec["target_scores"].to(dtype), rec["scores_sum"].to(dtype).clamp(min=1).reshape(())
    l_cls = F.binary_cross_entropy_with_logits(d["cls"], ts, reduction="none").sum() / denom
    tb, tgt = dfl_targets(d, rec, gt_bboxes)
    w = ts.sum(-1)[fg]
    l_box = ((1.0 - ciou(d["pb"][fg], tb[fg])) * w).sum() / denom
    tgt = tgt[fg]
    tl = tgt.long()
    wl = (tl + 1) - tgt
    logp = d["dist"][fg].reshape(-1, 4, R).log_softmax(-1)
    dfl = -(logp.gather(-1, tl[..., None])[..., 0] * wl + logp.gather(-1, tl[..., None] + 1)[..., 0] * (1 - wl)).mean(-1)
    return torch.stack((l_box * gains[0], l_cls * gains[1], (dfl * w).sum() / denom * gains[2]))


@functools.lru_cache(maxsize=None)
def reference(name, device):
    """What every test of case `name` needs, computed once and left unchanged: the inputs on `device`, the assignment record
    (assign_ref in fp64 on the fp64 decode, then in the kernel's types), per dtype (loss [3], the levels' gradients under
    grad_out, the decode dict), and `conditions`, what the GPU test asserts about the inputs."""
    seed, size, strides, counts, g, nc, dtype, go = CASES[name]
    gt = {n: t.to(device) for n, t in make_case(seed, size, counts, g, nc).items()}
    outs = [o.to(device) for o in head_outputs(seed, size, strides, len(counts), nc, dtype)]
    d64 = decode_ref([o.double() for o in outs], strides)
    rec = assign_ref(dict(gt, pd_scores=d64["pd_scores"], pd_bboxes=d64["pd_bboxes"], anc_points=d64["anc_points"]), nc, 10, 0.5, 6.0)
    rec = dict(rec, target_scores=rec["target_scores"].float(), scores_sum=rec["scores_sum"].float().reshape(1),
               target_gt_idx=rec["target_gt_idx"].int())
    out = dict(outs=outs, strides=strides, nc=nc, grad_out=torch.tensor(go, device=device), rec=rec, gt=gt, dtype=dtype)
    for dt in (torch.float64, torch.float32):
        leaves = [o.to(dt, copy=True).requires_grad_(True) for o in outs]
        loss = loss_ref(leaves, strides, rec, gt["gt_bboxes"])
        grads = torch.autograd.grad((loss * out["grad_out"].to(dt)).sum(), leaves)
        out[dt] = (loss.detach(), grads, {n: t.detach() for n, t in decode_ref(leaves, strides).items()})
    # counted on the fp64 restatement: foreground anchors, levels holding one, (image, tile) pairs with both kinds of anchor and
    # with background only, DFL targets at the clamp and with tl == R - 2
    fg, hw = rec["fg_mask"].cpu(), torch.tensor([o.shape[2] * o.shape[3] for o in outs])
    level = torch.repeat_interleave(torch.arange(len(hw)), hw)
    tile = torch.cat([torch.arange(int(n)) // 64 + 1000 * i for i, n in enumerate(hw)])
    per_tile = [fg[:, tile == t] for t in tile.unique()]
    tgt = dfl_targets(out[torch.float64][2], rec, gt["gt_bboxes"])[1].cpu()[fg]
    out["conditions"] = dict(fg=int(fg.sum()), levels=len(level[fg.any(0)].unique()), clamped=int((tgt >= R - 1 - 0.01).sum()),
                             tl14=int((tgt.long() == R - 2).sum()), mixed=sum(int((m.any(1) & ~m.all(1)).sum()) for m in per_tile),
                             background=sum(int((~m.any(1)).sum()) for m in per_tile))
    return out

