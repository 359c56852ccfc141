"""Loss wrappers the QAT step needs:

  FusedPotentialLoss        task loss + bit-width hinge, prediction/target form
                            (/root/reference/src/quantization/gdnsq/gdnsq_loss.py:6-86)
  FusedPotentialLossNoPred  same with a precomputed base loss (gdnsq_loss.py:88-168)
                            -- both with the hinge arithmetic in the HIP library (mhaq_fq_potential_loss_fwd / _bwd)
  SymmetricalKL             distillation loss of the ResNet-18 configs (src/aux/loss/symm_kl_loss.py)
  FusedDistillLoss          the six softmax-family distillation losses of src/aux/loss in the HIP library
                            (mhaq_fq_distill_loss_fwd / _bwd: 2 + 1 launches)
  FusedCrossEntropy         nn.CrossEntropyLoss() on hard labels in the HIP library (mhaq_fq_cls_head_fwd: 2 + 1 launches)
  distillation_criterion    a config's `distillation_loss` string -> module (gdnsq_quant.py: get_loss)

(The torch restatement of the two PotentialLoss modules is checker code and lives in oracle/loss.py.)
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch import nn


class _FusedPotential(nn.Module):
    """The same loss with its arithmetic in one HIP launch per direction (ops.potential_loss): ~25 scalar
    launches forward and ~30 backward become 1 + 1.  The module state {loss_sum, cnt, t} lives in a 3-float
    device block that the kernel reads (and, in training mode, advances) itself, so a step captured in a
    hipGraph sees the current values at every replay.  This is what the QAT trainer uses on the GPU; the
    attribute names are the reference's (gdnsq_loss.py:14-30, 73-84)."""

    def __init__(self, criterion, p=1, a=8, w=4, lossless=False):
        super().__init__()
        self.criterion = criterion
        self.p = p
        self.at, self.wt = a, w
        self.lossless = lossless
        self.register_buffer("_state", torch.tensor([0.0, 1.0, 0.0]), persistent=False)   # loss_sum, cnt, t
        self._t = 0.0
        self._stats = None

    # -- state, with the reference's attribute names ---------------------------------------------------
    @property
    def loss_sum(self):
        return self._state[0]

    @loss_sum.setter
    def loss_sum(self, v):
        self._state[0:1].copy_(torch.as_tensor(v, dtype=torch.float32).reshape(1))

    @property
    def cnt(self) -> int:
        return int(round(float(self._state[1])))           # host sync: for logging / tests only

    @cnt.setter
    def cnt(self, v):
        self._state[1:2].fill_(float(v))

    @property
    def t(self) -> float:
        return self._t

    @t.setter
    def t(self, v):
        v = float(v)
        if v != self._t:
            self._state[2:3].fill_(v)      # one tiny launch, only when the temperature moves
        self._t = v

    def _combine(self, base, las, laq, lws, lwq):
        from . import ops
        if self._state.device != lws.device:
            self._state = self._state.to(lws.device)
        self.base_loss = base
        ploss, self._stats = ops.potential_loss(base, las, laq, lws, lwq, self._state, self.at, self.wt, self.p,
                                                self.lossless, self.training)
        return ploss

    def _stat(i):  # noqa: N805 -- attribute views of the stats block of the last forward
        return property(lambda self: torch.tensor(1.0) if self._stats is None else self._stats[i])

    wloss, aloss, rloss = _stat(1), _stat(2), _stat(3)
    s_weight_loss, q_weight_loss, s_act_loss, q_act_loss = _stat(7), _stat(8), _stat(9), _stat(10)
    weight_reg_loss = _stat(11)
    del _stat


class FusedPotentialLoss(_FusedPotential):
    def forward(self, output, target):
        prd, las, laq, lws, lwq = output
        return self._combine(self.criterion(prd, target), las, laq, lws, lwq)


class FusedPotentialLossNoPred(_FusedPotential):
    def forward(self, output):
        bloss, las, laq, lws, lwq = output
        return self._combine(bloss, las, laq, lws, lwq)


class SymmetricalKL(nn.Module):
    def forward(self, input, target):
        x = F.log_softmax(input, dim=1)
        y = F.log_softmax(target, dim=1)
        return (F.kl_div(x, y, log_target=True, reduction="batchmean")
                + F.kl_div(y, x, log_target=True, reduction="batchmean"))


# ----------------------------------------------------------------------------- fused distillation losses
# the reference's config strings (gdnsq_quant.py: get_loss) of the six softmax-family losses -> MHAQ_FQ_DISTILL_*
DISTILL_KINDS = {
    "Cross-Entropy": 0,
    "Symmetrical Cross-Entropy": 1,
    "KL": 2,
    "Symmetrical KL": 3,
    "JSD": 4,
    "Hellinger": 5,
}
ENV_SWITCH_DISTILL = "MHAQ_DISTILL_FUSED"


def distill_fused_enabled(configured: bool = False) -> bool:
    """The trainer's switch: `configured` (QATConfig.fused_distill_loss) unless MHAQ_DISTILL_FUSED is set, which then
    decides: "1" / "true" / "on" / "yes" enable the fused loss, anything else disables it."""
    return _env_switch(ENV_SWITCH_DISTILL, configured)


def _env_switch(name: str, configured: bool) -> bool:
    v = os.environ.get(name)
    if v is None or not v.strip():
        return bool(configured)
    return v.strip().lower() in ("1", "true", "on", "yes")


def distill_fused_launches() -> int:
    """Kernel launches of mhaq_fq_distill_loss_fwd (two per call) and _bwd (one) so far in this process."""
    from . import _ext
    return int(_ext.ext().distill_fused_launches())


class FusedDistillLoss(nn.Module):
    """One of the six softmax-family distillation losses of the reference (src/aux/loss: distill_ce.py, symm_ce_loss.py,
    kl_loss.py, symm_kl_loss.py, jsdloss.py, hellinger.py) in the HIP library: two launches forward
    (mhaq_fq_distill_loss_fwd: one workgroup per row of logits, then a one-workgroup sum), one backward
    (mhaq_fq_distill_loss_bwd), where the framework runs log_softmax / kl_div / sum chains and their autograd mirror.

    `kind` is a config string of DISTILL_KINDS or its MHAQ_FQ_DISTILL_* number.  forward(input, target) takes device
    tensors of one shape, float32, bfloat16 or float16 each (the two may differ), [rows, C] or any shape seen as [-1, C]
    over its last dimension, and returns a 0-dim float32 loss; the gradient goes to `input` alone, in its dtype.  There
    is no CPU arithmetic: a CPU tensor raises MhaqFqError."""

    def __init__(self, kind):
        super().__init__()
        if isinstance(kind, str):
            if kind not in DISTILL_KINDS:
                raise NotImplementedError(f"FusedDistillLoss: unknown loss {kind!r}; valid: {sorted(DISTILL_KINDS)}")
            self.name, self.kind = kind, DISTILL_KINDS[kind]
        else:
            names = {v: k for k, v in DISTILL_KINDS.items()}
            if int(kind) not in names:
                raise NotImplementedError(f"FusedDistillLoss: unknown kind {kind!r}")
            self.name, self.kind = names[int(kind)], int(kind)

    def extra_repr(self):
        return repr(self.name)

    def forward(self, input, target):
        from . import _ext
        from ._lib import MhaqFqError
        if not (input.is_cuda and target.is_cuda):
            raise MhaqFqError("FusedDistillLoss runs only as HIP kernels: input and target must be device tensors "
                              "(no CPU fallback by design)")
        if input.shape != target.shape or input.dim() < 1:
            raise ValueError(f"FusedDistillLoss: input {tuple(input.shape)} and target {tuple(target.shape)} must have "
                             "one shape of at least one dimension")
        c = input.shape[-1]
        return _ext.ext().distill_loss(input.reshape(-1, c).contiguous(), target.detach().reshape(-1, c).contiguous(),
                                       self.kind)


# ----------------------------------------------------------------------------- fused hard-label cross-entropy
ENV_SWITCH_CE = "MHAQ_CE_FUSED"
ENV_SWITCH_CLS_METRICS = "MHAQ_CLS_METRICS"


def ce_fused_enabled(configured: bool = False) -> bool:
    """The trainer's switch: `configured` (QATConfig.fused_cross_entropy) unless MHAQ_CE_FUSED is set, which then decides
    (as distill_fused_enabled)."""
    return _env_switch(ENV_SWITCH_CE, configured)


def cls_metrics_enabled(configured: bool = False) -> bool:
    """`configured` (QATConfig.cls_metrics) unless MHAQ_CLS_METRICS is set, which then decides."""
    return _env_switch(ENV_SWITCH_CLS_METRICS, configured)


def is_default_cross_entropy(criterion) -> bool:
    """True for an nn.CrossEntropyLoss -- the class itself, not a subclass -- without class weights or label smoothing
    and with the mean reduction: what FusedCrossEntropy computes (its ignore_index may be any)."""
    return (type(criterion) is nn.CrossEntropyLoss and criterion.weight is None and criterion.label_smoothing == 0.0
            and criterion.reduction == "mean")


def cls_head_launches() -> int:
    """Kernel launches of the compiled classification-head node so far in this process: two per forward, one per backward."""
    from . import _ext
    return int(_ext.ext().cls_head_launches())


class FusedCrossEntropy(nn.Module):
    """nn.CrossEntropyLoss() with its default arguments on int64 class labels, in the HIP library: two launches forward
    (mhaq_fq_cls_head_fwd: one workgroup per row of logits, then a one-workgroup sum), one backward
    (mhaq_fq_distill_loss_bwd), where the framework runs log_softmax / nll_loss and their autograd mirror.  Only
    `ignore_index` can be set: class weights, label smoothing and the other reductions are refused.

    forward(input, target) takes device logits of any shape seen as [-1, C] over the last dimension (float32, bfloat16 or
    float16) and the int64 labels of its rows, and returns a 0-dim float32 loss; the gradient has the logits' dtype.  A
    label that is neither ignore_index nor in [0, C) does not abort the process as the framework's device assert does: its
    row is ignored and bit 2 of `last_flags` (a device word; cls_metrics.check_cls_flags reads it) is set.  There is no CPU
    arithmetic: a CPU tensor raises MhaqFqError."""

    def __init__(self, weight=None, ignore_index: int = -100, reduction: str = "mean", label_smoothing: float = 0.0):
        super().__init__()
        if weight is not None:
            raise NotImplementedError("FusedCrossEntropy: class weights are not supported")
        if label_smoothing != 0.0:
            raise NotImplementedError("FusedCrossEntropy: label smoothing is not supported")
        if reduction != "mean":
            raise NotImplementedError(f"FusedCrossEntropy: reduction {reduction!r} is not supported, only 'mean'")
        self.ignore_index = int(ignore_index)
        self.last_flags = None

    def extra_repr(self):
        return f"ignore_index={self.ignore_index}"

    def forward(self, input, target):
        from . import _ext
        from ._lib import MhaqFqError
        if not (input.is_cuda and target.is_cuda):
            raise MhaqFqError("FusedCrossEntropy runs only as HIP kernels: input and target must be device tensors "
                              "(no CPU fallback by design)")
        if input.dim() < 1 or target.dtype != torch.int64 or target.numel() * input.shape[-1] != input.numel():
            raise ValueError(f"FusedCrossEntropy: input {tuple(input.shape)} needs one int64 class label per row of its "
                             f"last dimension, got a {target.dtype} target of shape {tuple(target.shape)}")
        c = input.shape[-1]
        loss, self.last_flags = _ext.ext().cls_head_loss(input.reshape(-1, c).contiguous(),
                                                         target.detach().reshape(-1).contiguous(), self.ignore_index)
        return loss


def distillation_criterion(name: str, fused: bool = False) -> nn.Module:
    """The distillation loss a config names (`distillation_loss`; gdnsq_quant.py: get_loss).  "L1" and "L2" are the
    framework's modules.  "Symmetrical KL" is the framework chain SymmetricalKL() -- what QATTrainer always used --
    unless `fused`; the five other softmax-family names have no earlier behaviour here and are always FusedDistillLoss."""
    if name == "L1":
        return nn.L1Loss()
    if name == "L2":
        return nn.MSELoss()
    if name == "Symmetrical KL" and not fused:
        return SymmetricalKL()
    if name in DISTILL_KINDS:
        return FusedDistillLoss(name)
    raise NotImplementedError(f"distillation_loss {name!r} is invalid; valid options are: "
                              f"{['L1', 'L2'] + list(DISTILL_KINDS)}")
