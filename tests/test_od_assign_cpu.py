"""CPU: the restatement of the task-aligned assignment (tests/od_assign_ref.py) against the reference's own Assigner, and the
C ABI's argument checks of mhaq_fq_od_assign, which need no GPU."""
import ctypes
import importlib.util
import os

import pytest
import torch

from mhaq_amd import _lib, od_assign  # noqa: F401  (the module and its symbols must exist)
from tests import od_assign_ref as R

REF_LOSS = "/root/reference/src/models/od/loss/yolo_loss.py"

RANDOM_CASES = [n for n, c in R.CASES.items() if c[8] is torch.float32 and c[3]]      # the reference is fp32; G > 0
# ... and the rows of the edge table whose outcome does not rest on the library's tie rule (torch.topk leaves ties open)
RANDOM_CASES += [n for n, c in R.EDGE_CASES.items() if c[8] is torch.float32 and c[9] != "tie"]


@pytest.fixture(scope="module")
def reference_assigner():
    if not os.path.exists(REF_LOSS):
        pytest.skip("the reference tree is not on this machine")
    spec = importlib.util.spec_from_file_location("_reference_yolo_loss", REF_LOSS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Assigner


@pytest.mark.parametrize("name", RANDOM_CASES)
def test_reference_assigner_equals_the_restatement(reference_assigner, name):
    """fp32 against fp32 on the CPU.  The inputs are well separated (margin), so the reference's unspecified tie orders
    cannot show, and all three results are equal on bits."""
    if name in R.EDGE_CASES:
        c, nc, k, alpha, beta, _ = R.edge_case(name)
    else:
        seed, size, counts, g, nc, k, alpha, beta, _ = R.CASES[name]
        c = R.make_case(seed, size, counts, g, nc)
    assert R.assign_ref(c, nc, k, alpha, beta)["margin"] >= 1e-3
    tb, ts, fg = reference_assigner(nc=nc, top_k=k, alpha=alpha, beta=beta)(
        c["pd_scores"], c["pd_bboxes"], c["anc_points"], c["gt_labels"], c["gt_bboxes"], c["mask_gt"])
    ref = R.assign_ref(c, nc, k, alpha, beta, dtype=torch.float32)
    assert torch.equal(fg, ref["fg_mask"])
    assert torch.equal(tb, ref["target_bboxes"])
    assert torch.equal(ts, ref["target_scores"])


def test_argument_errors_are_returned_before_any_launch():
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()                      # host memory: a call that launched anything would not return a code
    p = ctypes.addressof(buf)
    nb = L.mhaq_fq_od_assign_workspace_bytes(2, 3, 84, 10)

    def call(dtype=_lib.DT_F32, a=84, top_k=10, ws=p, ws_bytes=nb, **null):
        ptr = lambda name: None if name in null else p
        return L.mhaq_fq_od_assign(ptr("pd_scores"), ptr("pd_bboxes"), dtype, ptr("anc"), ptr("gt_labels"), ptr("gt_bboxes"),
                                   ptr("mask_gt"), 2, a, 80, 3, top_k, 0.5, 6.0, 1e-9, ptr("tb"), ptr("ts"), ptr("fg"),
                                   ptr("gi"), ptr("ssum"), ptr("flags"), ws, ws_bytes, None)

    for name in ("pd_scores", "pd_bboxes", "anc", "gt_labels", "gt_bboxes", "mask_gt", "tb", "ts", "fg", "gi", "ssum", "flags"):
        assert call(**{name: True}) == -1, name
    assert call(ws=None) == -1
    assert call(a=9) == -1                              # A < top_k
    assert call(dtype=7) == -1
    assert call(ws_bytes=nb - 1) == -2
    assert call(a=1 << 20) == -4 and call(a=64, top_k=33) == -4


def test_workspace_grows_with_rows_and_anchors_not_with_their_product():
    ws = _lib.lib().mhaq_fq_od_assign_workspace_bytes
    b, g, a, k = 4, 64, 8400, 10
    base = ws(b, g, a, k)
    assert 0 < base <= 8 * (b * g * (k + 1) + 2 * b * a + 2 * b) + 64 < b * g * a
    assert ws(b, 2 * g, a, k) - base <= 8 * b * g * (k + 1) and ws(b, g, 2 * a, k) - base <= 8 * 2 * b * a
    assert ws(b, g, a, 2 * k) > base and ws(0, g, a, k) == 0
