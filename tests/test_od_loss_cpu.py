"""CPU: the restatement of the detection criterion (tests/od_loss_ref.py) against the reference's own BoxLoss / compute_iou /
BCEWithLogitsLoss path in fp32, and the C ABI's argument checks of the mhaq_fq_od_decode / od_loss calls, which need no GPU."""
import ctypes
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

from mhaq_amd import _lib, od_loss  # noqa: F401  (the module and its symbols must exist)
from tests import od_loss_ref as R

REF_LOSS = "/root/reference/src/models/od/loss/yolo_loss.py"
WITH_BOXES = [n for n, c in R.CASES.items() if c[6] is torch.float32 and c[4]]      # the reference is fp32; G > 0


@pytest.fixture(scope="module")
def reference_module():
    if not os.path.exists(REF_LOSS):
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("_reference_yolo_loss", REF_LOSS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", WITH_BOXES)
def test_reference_losses_equal_the_restatement(reference_module, name):
    """fp32 against fp32 on the CPU, from one assignment record: the reference's statements of __call__ around its assigner.
    Its masked gather reorders the sums, hence a few ulp32 on a loss and 1e-6 * max|g| on a gradient."""
    r = R.reference(name, "cpu")
    rec, strides, nc = r["rec"], r["strides"], r["nc"]
    head = SimpleNamespace(stride=torch.tensor(strides, dtype=torch.float32), nc=nc, no=4 * R.R + nc, ch=R.R)
    crit = reference_module.ComputeYoloLoss(SimpleNamespace(head=head), {}, device="cpu")
    leaves = [o.clone().requires_grad_(True) for o in r["outs"]]
    x = torch.cat([i.view(leaves[0].shape[0], crit.no, -1) for i in leaves], dim=2)
    pred_distri, pred_scores = (t.permute(0, 2, 1).contiguous() for t in x.split((4 * R.R, nc), dim=1))
    anchor_points, stride_tensor = reference_module.make_anchors(leaves, strides, offset=0.5)
    pred_bboxes = crit.box_decode(anchor_points, pred_distri)
    ts, tss = rec["target_scores"], rec["scores_sum"].clamp(min=1).reshape(())
    target_bboxes = r["gt"]["gt_bboxes"][torch.arange(x.shape[0])[:, None], rec["target_gt_idx"].long()] / stride_tensor
    loss_cls = crit.cls_loss(pred_scores, ts).sum() / tss
    loss_box, loss_dfl = crit.box_loss(pred_distri, pred_bboxes, anchor_points, target_bboxes, ts, tss, rec["fg_mask"])
    loss = torch.stack((loss_box, loss_cls, loss_dfl)) * torch.tensor(R.GAINS)
    grads = torch.autograd.grad((loss * r["grad_out"]).sum(), leaves)
    want, want_grads, _ = r[torch.float32]
    assert bool(((loss - want).abs() <= 2 * 2.0 ** -23 * want.abs()).all()), (loss, want)
    for g, w in zip(grads, want_grads):
        assert float((g - w).abs().max()) <= 1e-6 * float(w.abs().max())


def test_argument_errors_are_returned_before_any_launch():
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()                      # host memory: a call that launched anything would not return a code
    p = ctypes.addressof(buf)
    nb = L.mhaq_fq_od_loss_workspace_bytes(2, 84, 3)
    assert nb == 2 * (84 // 64 + 3) * 24 and L.mhaq_fq_od_loss_workspace_bytes(0, 84, 3) == 0

    def call(fn, levels=3, dtype=_lib.DT_F32, b=2, reg_max=16, h=(8, 4, 2), stride=(8.0, 16.0, 32.0), level0=p, ws=p, ws_bytes=nb,
             **null):
        q = lambda name: None if name in null else p
        n = len(h)
        table = ((ctypes.c_void_p * n)(level0, *[p] * (n - 1)), (ctypes.c_int32 * n)(*h), (ctypes.c_int32 * n)(*h),
                 (ctypes.c_float * n)(*stride), levels, dtype, b, 80, reg_max)
        if fn == "decode":
            return L.mhaq_fq_od_decode(*table, q("pd_bboxes"), q("pd_scores"), q("anc"), None)
        rec = (q("fg"), q("gi"), q("ts"))
        if fn == "fwd":
            return L.mhaq_fq_od_loss_fwd(*table, *rec, q("ssum"), q("gl"), q("gb"), 3, 7.5, 0.5, 1.5, q("loss"), q("denom"), ws,
                                         ws_bytes, None)
        grads = None if "grads" in null else (ctypes.c_void_p * n)(*[p] * n)
        return L.mhaq_fq_od_loss_bwd(*table, *rec, q("gl"), q("gb"), 3, q("go"), q("denom"), 7.5, 0.5, 1.5, grads, None)

    for fn, names in (("decode", ("pd_bboxes", "pd_scores", "anc")), ("fwd", ("fg", "gi", "ts", "ssum", "gl", "gb", "loss", "denom")),
                      ("bwd", ("fg", "gi", "ts", "gl", "gb", "go", "denom", "grads"))):
        for name in names:
            assert call(fn, **{name: True}) == -1, (fn, name)
        assert call(fn, level0=None) == -1 and call(fn, dtype=7) == -1 and call(fn, levels=0) == -1
        assert call(fn, stride=(8.0, 0.0, 32.0)) == -1 and call(fn, h=(8, -1, 2)) == -1
        assert call(fn, reg_max=8) == -4 and call(fn, b=1 << 16) == -4
        assert call(fn, levels=5, h=(8, 4, 2, 1, 1), stride=(8.0, 16.0, 32.0, 64.0, 128.0)) == -4
        assert call(fn, h=(128, 96, 2)) == -4                              # 25 604 anchors > 24 576
        assert call(fn, level0=p + 2) == -3
    assert call("fwd", ws=None) == -1 and call("fwd", ws_bytes=nb - 1) == -2 and call("fwd", ws=p + 4) == -3
