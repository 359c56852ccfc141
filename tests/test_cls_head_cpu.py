"""CPU: the classification head's checker (tests/cls_head_ref.py) against the framework in float64, the C ABI's symbols and
argument errors through ctypes with fake pointers (no launch), the host-side switches and refusals, and the epoch meter's
arithmetic.  The kernels themselves are tested on the device (tests/test_gpu_cls_head.py)."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mhaq_amd import _lib
from tests import cls_head_ref as R

ids_shape = lambda s: "%dx%d" % s          # noqa: E731


# ---------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("shape", R.CPU_SHAPES, ids=ids_shape)
def test_reference_equals_the_frameworks_cross_entropy_and_its_autograd_in_float64(shape):
    x, y = R.plain_case(shape)
    ref = R.head64(x, y)
    x64 = x.double().requires_grad_(True)
    loss = F.cross_entropy(x64, y, ignore_index=R.IGNORE)
    (g,) = torch.autograd.grad(loss, x64)
    loss = loss.detach()
    nll = F.cross_entropy(x64.detach(), y, ignore_index=R.IGNORE, reduction="none")
    assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 * abs(float(loss))
    assert float((ref["nll"] - nll).abs().max()) <= 1e-12 * float(nll.abs().max())
    assert float((ref["gunit"] - g).abs().max()) <= 1e-12 * float(g.abs().max())
    if shape[0] > 3:
        assert not bool(ref["valid"][3]) and float(ref["nll"][3]) == 0 and not bool(ref["gunit"][3].any())
        assert int(ref["counts"][0]) == shape[0] - 1


def test_reference_with_every_row_ignored_is_nan_with_zero_gradient_like_the_framework():
    x, _ = R.plain_case((5, 37))
    y = torch.full((5,), R.IGNORE)
    ref = R.head64(x, y)
    assert torch.isnan(ref["loss"]) and torch.isnan(F.cross_entropy(x.double(), y))
    assert not bool(ref["gunit"].any()) and ref["counts"].tolist() == [0, 0, 0] and ref["acc"].tolist() == [0.0, 0.0]
    assert ref["rank"].tolist() == [37] * 5


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("shape", [(16, 10), (16, 100), (5, 37), (3, 1028)], ids=ids_shape)
def test_rank_below_k_is_topk_membership_on_tie_free_rows(shape, k):
    rows, cols = shape
    gen = torch.Generator().manual_seed(rows * cols)
    x = torch.stack([torch.randperm(cols, generator=gen).float() - cols / 2 for _ in range(rows)])    # distinct values
    y = torch.randint(0, cols, (rows,), generator=gen)
    member = (x.topk(min(k, cols), dim=1).indices == y[:, None]).any(1)
    for rank in (R.sort_rank(x, y), R.count_rank(x, y)):
        assert torch.equal(rank < k, member)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", R.CPU_SHAPES, ids=ids_shape)
def test_counting_form_equals_the_stable_sort_and_rank_zero_is_argmax_on_ties_zeros_nan_and_inf(shape, dtype):
    for variant in R.edge_variants(shape):
        x, y = R.edge_case(shape, dtype, variant)
        srt, cnt = R.sort_rank(x, y), R.count_rank(x, y)
        assert torch.equal(srt, cnt), (variant, srt, cnt)
        valid = R.valid_rows(y, shape[1])
        assert torch.equal((srt == 0)[valid], (x.float().argmax(1) == y)[valid]), variant
        assert bool((srt[~valid] == shape[1]).all())


# ---------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_entry_points_are_exported_and_bound_and_the_abi_version_stays(L):
    for name in ("mhaq_fq_cls_head_workspace_bytes", "mhaq_fq_cls_head_fwd"):
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
    assert L.mhaq_fq_abi_version() == 4
    assert L.mhaq_fq_cls_head_workspace_bytes(250) == 250 * 16
    assert L.mhaq_fq_cls_head_workspace_bytes(0) == 0 and L.mhaq_fq_cls_head_workspace_bytes(-3) == 0


def test_argument_errors_arrive_in_the_stated_order_without_a_launch(L):
    fake, odd2, odd4 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1004)
    nb = 8 * 16

    def call(x=fake, dt=0, target=fake, rows=8, cols=10, ii=-100, topk=5, loss=fake, acc=fake, counts=fake, nll=fake, rank=fake,
             gunit=fake, flags=fake, ws=fake, wsb=nb):
        return L.mhaq_fq_cls_head_fwd(x, dt, target, rows, cols, ii, topk, loss, acc, counts, nll, rank, gunit, flags, ws, wsb,
                                      None)

    # -1: a required pointer, a size, topk, the dtype -- whatever else is wrong with the call
    for kw in (dict(x=None), dict(target=None), dict(loss=None), dict(acc=None), dict(counts=None), dict(flags=None),
               dict(ws=None), dict(rows=0), dict(cols=0), dict(rows=-1), dict(topk=0), dict(dt=3), dict(dt=-1)):
        assert call(**kw) == -1, kw
        assert call(**{**dict(wsb=0, nll=odd2, cols=1 << 31), **kw}) == -1, kw
    # -2: the workspace, ahead of alignment and range
    assert call(wsb=nb - 1) == -2
    assert call(wsb=nb - 1, x=ctypes.c_void_p(0x1001)) == -2
    assert call(rows=1 << 40, wsb=nb) == -2
    # -3: alignment, ahead of the range
    assert call(x=ctypes.c_void_p(0x1001)) == -3 and call(x=odd2) == -3
    for kw in (dict(target=odd4), dict(counts=odd4), dict(ws=odd4), dict(loss=odd2), dict(acc=odd2), dict(nll=odd2),
               dict(rank=odd2), dict(gunit=odd2), dict(flags=odd2)):
        assert call(**kw) == -3, kw
        assert call(**kw, cols=1 << 31) == -3, kw
    # -4: beyond the grid bound
    assert call(cols=1 << 31) == -4
    assert call(rows=1 << 31, wsb=(1 << 31) * 16) == -4
    assert call(x=odd2, dt=1, cols=1 << 31) == -4          # every earlier check passed: 16-bit logits need 2-byte alignment only
    assert call(nll=None, rank=None, gunit=None, cols=1 << 31) == -4       # the nullable outputs may be NULL


# ---------------------------------------------------------------------------------------------- host logic
def test_config_defaults_are_off_and_the_environment_overrides(monkeypatch):
    from mhaq_amd import loss as Lm
    from mhaq_amd.qat import QATConfig
    cfg = QATConfig()
    assert cfg.fused_cross_entropy is False and cfg.cls_metrics is False
    for env, fn in ((Lm.ENV_SWITCH_CE, Lm.ce_fused_enabled), (Lm.ENV_SWITCH_CLS_METRICS, Lm.cls_metrics_enabled)):
        monkeypatch.delenv(env, raising=False)
        assert fn(False) is False and fn(True) is True
        monkeypatch.setenv(env, "1")
        assert fn(False) is True
        monkeypatch.setenv(env, "0")
        assert fn(True) is False
        monkeypatch.setenv(env, " ")
        assert fn(True) is True and fn(False) is False
    assert (Lm.ENV_SWITCH_CE, Lm.ENV_SWITCH_CLS_METRICS) == ("MHAQ_CE_FUSED", "MHAQ_CLS_METRICS")


def test_only_the_default_cross_entropy_is_replaced():
    from mhaq_amd.loss import is_default_cross_entropy

    class Sub(nn.CrossEntropyLoss):
        pass

    assert is_default_cross_entropy(nn.CrossEntropyLoss()) and is_default_cross_entropy(nn.CrossEntropyLoss(ignore_index=3))
    for crit in (nn.CrossEntropyLoss(weight=torch.ones(10)), nn.CrossEntropyLoss(label_smoothing=0.1),
                 nn.CrossEntropyLoss(reduction="sum"), nn.CrossEntropyLoss(reduction="none"), Sub(), nn.NLLLoss(), nn.L1Loss()):
        assert not is_default_cross_entropy(crit), crit


def test_cpu_tensors_are_refused_not_computed():
    from mhaq_amd.cls_metrics import cls_metrics
    from mhaq_amd.loss import FusedCrossEntropy
    x, y = R.plain_case((5, 37))
    with pytest.raises(_lib.MhaqFqError, match="no CPU fallback"):
        cls_metrics(x, y)
    with pytest.raises(_lib.MhaqFqError, match="no CPU fallback"):
        FusedCrossEntropy()(x, y)


def test_fused_cross_entropy_refuses_what_it_does_not_compute():
    from mhaq_amd.loss import FusedCrossEntropy
    assert FusedCrossEntropy().ignore_index == -100 and FusedCrossEntropy(ignore_index=7).ignore_index == 7
    with pytest.raises(NotImplementedError, match="weights"):
        FusedCrossEntropy(weight=torch.ones(10))
    with pytest.raises(NotImplementedError, match="smoothing"):
        FusedCrossEntropy(label_smoothing=0.1)
    for red in ("sum", "none"):
        with pytest.raises(NotImplementedError, match="reduction"):
            FusedCrossEntropy(reduction=red)


def test_check_cls_flags_reads_the_word():
    from mhaq_amd.cls_metrics import FLAG_NONFINITE, FLAG_TARGET_RANGE, check_cls_flags
    assert (FLAG_NONFINITE, FLAG_TARGET_RANGE) == (2, 4)
    word = lambda v: torch.tensor([v], dtype=torch.int32)      # noqa: E731
    assert check_cls_flags(word(0)) == 0 and check_cls_flags(word(2)) == 2
    with pytest.raises(FloatingPointError):
        check_cls_flags(word(2), nonfinite=True)
    for v in (4, 6):
        with pytest.raises(IndexError, match=r"Target .* is out of bounds\."):
            check_cls_flags(word(v))


# ---------------------------------------------------------------------------------------------- the meter
def _rec(loss, v, c1, ck, validate_keys=False):
    loss, counts = torch.tensor(loss, dtype=torch.float32), torch.tensor([v, c1, ck])
    return {"val_loss": loss, "correct": counts} if validate_keys else {"loss": loss, "counts": counts}


def test_meter_is_the_batch_size_weighted_mean_over_unequal_batches_and_skips_an_all_ignored_one():
    from mhaq_amd.cls_metrics import ClsValidationMeter
    m = ClsValidationMeter()
    assert m.compute() == {}
    m.update(_rec(0.5, 16, 4, 12))
    m.update(_rec(float("nan"), 0, 0, 0))                     # every row ignored: a NaN loss of weight 0
    m.update(_rec(2.0, 3, 3, 3, validate_keys=True))
    out = m.compute()
    assert float(out["Accuracy_top1"]) == 7 / 19 and float(out["Accuracy_top5"]) == 15 / 19
    assert float(out["val_loss"]) == (0.5 * 16 + 2.0 * 3) / 19
    # ... which is the weighted mean of the per-batch values
    assert float(out["Accuracy_top1"]) == pytest.approx((16 * (4 / 16) + 3 * (3 / 3)) / 19, rel=1e-15)
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in out.values())
    m.reset()
    assert m.compute() == {}
    m.update(_rec(1.25, 8, 1, 2))
    out = m.compute()
    assert (float(out["val_loss"]), float(out["Accuracy_top1"]), float(out["Accuracy_top5"])) == (1.25, 1 / 8, 2 / 8)
