"""GPU: the detection criterion's kernels (csrc/od_loss.hip) against the fp64 restatement of their contract (tests/od_loss_ref.py),
each case on ONE assignment record (assign_ref in fp64 on the fp64 decode).  Bars (tests/distill_ref.py): MARGIN times the error of
the eager fp32 restatement on the device, plus 8 ulp32 for a loss and 8 * 2^-24 * max|fp64| for a tensor's max-norm -- the gradient
per level and channel group, plus half an ulp of the stored dtype per element of a 16-bit head.  Measured shares: DESIGN section 20."""
from types import SimpleNamespace

import pytest
import torch

from mhaq_amd import od_loss as OL
from mhaq_amd import ops
from tests import od_loss_ref as R
from tests.distill_ref import grad_bar, loss_bar
from tests.od_assign_ref import assign_ref

pytestmark = pytest.mark.gpu
F64, F32, BAND = torch.float64, torch.float32, 64
BIG, LOSSES = "a525-ragged-tiles-b3-padded-rows-grad-out", ("loss_box", "loss_cls", "loss_dfl")


def half_ulp(g64, dtype):
    """Half an ulp of |g64| in a 16-bit `dtype`, per element (0 for float32): the one rounding of the stored gradient."""
    if dtype is F32:
        return torch.zeros_like(g64)
    mant, emin = (7, -126) if dtype is torch.bfloat16 else (10, -14)
    return torch.exp2(((torch.frexp(g64.abs().clamp_min(2.0 ** -140))[1] - 1).clamp_min(emin) - mant - 1).double())


def run_kernels(r):
    """decode, loss forward and backward on the case's record; the gradients land in NaN-filled buffers between NaN bands."""
    outs, rec = r["outs"], r["rec"]
    gl, gb = r["gt"]["gt_labels"].reshape(outs[0].shape[0], -1).contiguous(), r["gt"]["gt_bboxes"]
    record = (rec["fg_mask"], rec["target_gt_idx"], rec["target_scores"])
    dec = ops.od_decode(outs, r["strides"], r["nc"])
    loss, denom = ops.od_loss_fwd(outs, r["strides"], r["nc"], 16, *record, rec["scores_sum"], gl, gb, R.GAINS)
    bufs = [torch.full((o.numel() + 2 * BAND,), float("nan"), dtype=o.dtype, device="cuda") for o in outs]
    grads = ops.od_loss_bwd(outs, r["strides"], r["nc"], 16, *record, gl, gb, r["grad_out"], denom, R.GAINS,
                            out=[b[BAND:-BAND].view(o.shape) for b, o in zip(bufs, outs)])
    for b in bufs:               # no stray write, and every element written
        assert bool(b[:BAND].isnan().all()) and bool(b[-BAND:].isnan().all()) and not bool(b[BAND:-BAND].isnan().any())
    return [*dec, loss, *grads]


def shares_of_the_bars(loss, grads, chain, ref, dtype):
    """The share of its bar that each loss and each (level, channel group) of the gradient uses."""
    (l32, g32), (l64, g64) = chain, ref
    shares = {n: abs(float(loss[k]) - float(l64[k])) / loss_bar(l32[k].detach(), l64[k]) for k, n in enumerate(LOSSES)}
    for i, (g, a, b) in enumerate(zip(grads, g32, g64)):
        for part, sl in (("dist", slice(0, 4 * R.R)), ("cls", slice(4 * R.R, None))):
            allowed = grad_bar(a[:, sl], b[:, sl]) + half_ulp(b[:, sl], dtype)
            shares[f"grad{i}-{part}"] = float(((g[:, sl].double() - b[:, sl]).abs() / allowed.clamp_min(1e-300)).max())
    return shares


@pytest.mark.parametrize("name", R.CASES)
def test_kernels_against_the_restatement(name):
    r = R.reference(name, "cuda")
    c = r["conditions"]                                     # on the inputs; they are not tolerances
    assert not r["gt"]["gt_bboxes"].shape[1] or (c["fg"] >= 8 and c["levels"] >= 2 and c["mixed"] >= 1 and c["background"] >= 1), c
    assert not name.startswith("a1344") or (c["clamped"] >= 1 and c["tl14"] >= 1), c
    got, again = run_kernels(r), run_kernels(r)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got, again))
    (l64, g64, d64), (l32, g32, d32) = r[F64], r[F32]
    shares = {n: float((t.double() - d64[n]).abs().max()) / grad_bar(d32[n], d64[n])
              for n, t in zip(("pd_bboxes", "pd_scores", "anc_points"), got[:3])}
    shares.update(shares_of_the_bars(got[3], got[4:], (l32, g32), (l64, g64), r["dtype"]))
    print(f"bar shares {name}: " + ", ".join(f"{n} {v:.3f}" for n, v in shares.items()))
    assert max(shares.values()) <= 1.0, shares


def step(r, leaves):
    """od_loss forward and backward under the case's grad_out -> (its result, loss [3], the gradients of `leaves`)."""
    for t in leaves:
        t.grad = None
    gt = r["gt"]
    res = OL.od_loss(leaves, r["strides"], gt["gt_labels"], gt["gt_bboxes"], gt["mask_gt"], r["nc"])
    loss = torch.stack([res[n] for n in LOSSES])
    (loss * r["grad_out"]).sum().backward()
    return res, loss.detach(), [t.grad for t in leaves]


def test_od_loss_end_to_end_with_the_kernel_assigner():
    """Against the restatement with assign_ref; its fp32 form end to end sets the bars, the case's margin keeps the discrete
    outcome apart from rounding."""
    r = R.reference(BIG, "cuda")
    assert r["rec"]["margin"] >= 1e-3
    res, loss, grads = step(r, [o.clone().requires_grad_(True) for o in r["outs"]])
    assert torch.equal(res["fg_mask"], r["rec"]["fg_mask"]) and torch.equal(res["target_gt_idx"], r["rec"]["target_gt_idx"])
    assert all(res[n].dim() == 0 and res[n].dtype is F32 for n in LOSSES)
    l32 = [o.to(F32, copy=True).requires_grad_(True) for o in r["outs"]]
    d32 = R.decode_ref([t.detach() for t in l32], r["strides"])
    rec32 = assign_ref(dict(r["gt"], pd_scores=d32["pd_scores"], pd_bboxes=d32["pd_bboxes"], anc_points=d32["anc_points"]),
                       r["nc"], 10, 0.5, 6.0, dtype=F32)
    loss32 = R.loss_ref(l32, r["strides"], dict(rec32, scores_sum=rec32["scores_sum"].reshape(1)), r["gt"]["gt_bboxes"])
    g32 = torch.autograd.grad((loss32 * r["grad_out"]).sum(), l32)
    shares = shares_of_the_bars(loss, grads, (loss32, g32), r[F64][:2], F32)
    print("bar shares end to end: " + ", ".join(f"{n} {v:.3f}" for n, v in shares.items()))
    assert max(shares.values()) <= 1.0, shares


def test_compute_yolo_loss_is_a_drop_in():
    r = R.reference(BIG, "cuda")
    gt, nc = r["gt"], r["nc"]
    head = SimpleNamespace(stride=torch.tensor([8.0, 16.0, 32.0]), nc=nc, no=4 * R.R + nc, ch=R.R)
    crit = OL.ComputeYoloLoss(SimpleNamespace(head=head), {"box": 7.5, "cls": 0.5, "dfl": 1.5}, device="cuda")
    valid = gt["mask_gt"][..., 0] != 0
    box = gt["gt_bboxes"][valid]
    targets = {"idx": valid.nonzero()[:, 0].float(), "labels": gt["gt_labels"][valid].reshape(-1),
               "boxes": torch.cat(((box[:, :2] + box[:, 2:]) / 2, box[:, 2:] - box[:, :2]), 1) / 160.0}
    rows, mask = crit.targets_to_rows(r["outs"], targets)
    assert torch.equal(mask, gt["mask_gt"]) and torch.equal(rows[..., :1], gt["gt_labels"])
    assert float((rows[..., 1:] - gt["gt_bboxes"]).abs().max()) <= 1e-3
    leaves, twins = ([o.clone().requires_grad_(True) for o in r["outs"]] for _ in range(2))
    out = crit(leaves, targets)
    sum(out).backward()
    want = OL.od_loss(twins, r["strides"], rows[..., :1], rows[..., 1:], mask, nc)
    sum(want[n] for n in LOSSES).backward()
    assert all(torch.equal(x, want[n]) for x, n in zip(out, LOSSES))
    assert all(torch.equal(x.grad, y.grad) and bool(x.grad.isfinite().all()) for x, y in zip(leaves, twins))


def test_the_functional_path_can_be_captured_forward_and_backward():
    r = R.reference("a84-full-tile-then-two-short-levels-b3", "cuda")
    leaves = [o.clone().requires_grad_(True) for o in r["outs"]]

    def run():
        _, loss, grads = step(r, leaves)
        return [loss, *grads]

    eager = [t.clone() for t in run()]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = run()
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        for t in out:
            t.zero_()
        graph.replay()
        assert all(torch.equal(x, y) for x, y in zip(out, eager))


def test_shapes_beyond_the_ranges_raise_value_error():
    r = R.reference("g0-b1", "cuda")
    with pytest.raises(ValueError):
        ops.od_decode(r["outs"], r["strides"], r["nc"], reg_max=8)
    with pytest.raises(ValueError):
        ops.od_decode(r["outs"] + r["outs"][:2], (8, 16, 32, 64, 128), r["nc"])
