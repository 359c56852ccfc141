"""Training BatchNorm2d with the framework's forward and the HIP backward (csrc/bn_bwd.hip).

In a float32 channels_last training step the BatchNorm backward is three MIOpen launches per layer on the critical path
(two reads for dgamma / dbeta, a finalize, two reads and a write for dx) that run well short of the memory rate on all
but the largest tensors.  The compiled node `bn_train` (csrc/torch_binding.cpp, BatchNormTrainFn) keeps the forward
exactly as F.batch_norm runs it -- at::_batch_norm_impl_index: y, the saved statistics and the running statistics keep
their bits -- and replaces only the backward, by mhaq_fq_bn_bwd, where that applies (a dense float32 channels_last device
tensor with C % 4 == 0); everywhere else the node calls the backward autograd itself would have called.  The gradients
of the HIP path differ from the stock ones by summation order only.

install() switches the CLASS of every module whose exact type is nn.BatchNorm2d (HipBackwardBatchNorm2d is a subclass
that adds a forward and nothing else): module names, named_modules() order, state_dict keys, copy.deepcopy and
isinstance(m, nn.BatchNorm2d) are what they were; SyncBatchNorm and subclasses are left alone.  The decision is taken per
call: the original forward runs in eval mode, with track_running_stats=False or affine=False, on a CPU tensor and on a
non-float32 input (so under autocast, where the convolution in front hands over a 16-bit tensor).

16-bit inputs.  install(model, x16=True) also sends a bf16 / fp16 device input (float32 parameters) through the node and
enables its 16-bit backward (mhaq_fq_bn_bwd_x16: the fp32 arithmetic on the exactly upcast x and dy, dx rounded to
nearest-even once; C % 8 == 0 and a dy of x's dtype, else the node falls back to the framework's backward, bit for bit).
The forward is still the framework's (unless hip_forward_x16, below, is set as well).  This is OFF by default -- it changes the gradient bits of every bf16 run --:
QATConfig.hip_bn_backward_16bit=True switches it on per trainer, MHAQ_BN_BACKWARD_X16=1 (or "true" / "on") in the
environment for an unchanged benchmark; the variable, when set, overrides the configuration either way.

forward_pooled() is the same module with the ResNet stem's max pool behind it in one node (fused_blocks.FusedResNet18 calls
it; csrc/torch_binding.cpp, BatchNormPoolTrainFn): same forward bits, and a backward that never materializes the pool's
gradient.  float32 by default (takes_pooled_node): a 16-bit stem stays maxpool(bn(c)), with the 16-bit backward above where
enabled, unless the 16-bit pooled node below is switched on.

Pooled node, 16-bit.  install(model, x16=True, pool_x16=True) lets forward_pooled() take a bf16 / fp16 input.  The node never
calls the framework's 16-bit BatchNorm forward: mhaq_fq_bn_fwd_x16 without an output leaves the statistics (two launches),
mhaq_fq_bn_norm_pool3s2_fwd_x16 normalizes and pools in one more -- the BatchNorm output and int64 indices are never written --,
and the backward is mhaq_fq_bn_pool_bwd_x16.  Every output, statistic and gradient is, bit for bit, that of
max_pool2d(bn(c)) with x16 and hip_forward_x16.  Where the compiled side finds the input ineligible (NCHW, C % 8 != 0,
N * H * W == 1) it runs exactly that composition under the module's other flags.  Like hip_forward_x16 it has an effect only
TOGETHER with x16.  OFF by default -- the stem's y and its saved and running statistics become the HIP forward's --:
QATConfig.fuse_stem_pool_16bit=True per trainer (next to hip_bn_backward_16bit), MHAQ_STEM_POOL_X16=1 in the environment (next
to MHAQ_BN_BACKWARD_X16=1), with the same semantics.

HIP forward.  install(model, hip_forward=True) also runs the FORWARD of a float32 input on the kernels of csrc/bn_bwd.hip
(mhaq_fq_bn_fwd: shifted fp64 sums, statistics rounded once, y = (x - mean) * (gamma * invstd) + beta); the node falls back to
the framework's forward, bit for bit, where that does not apply (NCHW, C % 4 != 0).  16-bit inputs keep the framework's
forward under this flag.  OFF by default -- it changes the bits of y and of the saved and running statistics --:
QATConfig.hip_bn_forward=True switches it on per trainer, MHAQ_BN_FORWARD=1 in the environment for an unchanged benchmark,
with the semantics of MHAQ_BN_BACKWARD_X16.

HIP forward, 16-bit.  install(model, x16=True, hip_forward_x16=True) runs the forward of a bf16 / fp16 input on
mhaq_fq_bn_fwd_x16: the same contract on the exactly upcast input -- float32 statistics, y rounded to nearest-even once --,
with C % 8 == 0 and N * H * W >= 2, else the framework's forward bit for bit.  It has an effect only TOGETHER with x16: the
16-bit HIP backward is the only backward of such a node, so hip_forward_x16 alone changes nothing (and does not raise).  The
stem keeps maxpool(bn(c)) on the unpooled node (without pool_x16).  OFF by default -- it changes the bits of y and of the saved and running
statistics of every bf16 run --: QATConfig.hip_bn_forward_16bit=True per trainer (next to hip_bn_backward_16bit),
MHAQ_BN_FORWARD_X16=1 in the environment (next to MHAQ_BN_BACKWARD_X16=1), with the same semantics.

MHAQ_BN_BACKWARD=0 in the environment keeps QATTrainer from installing (A/B runs of an unchanged benchmark);
QATConfig.hip_bn_backward=False does the same per trainer.
"""
from __future__ import annotations

import os

import torch
from torch import nn

ENV_SWITCH = "MHAQ_BN_BACKWARD"
ENV_SWITCH_X16 = "MHAQ_BN_BACKWARD_X16"
ENV_SWITCH_FORWARD = "MHAQ_BN_FORWARD"
ENV_SWITCH_FORWARD_X16 = "MHAQ_BN_FORWARD_X16"
ENV_SWITCH_POOL_X16 = "MHAQ_STEM_POOL_X16"
_X16 = "_mhaq_bn_x16"          # per-module flag in the instance __dict__ (not a parameter, buffer or state_dict entry)
_HIP_FWD = "_mhaq_bn_hip_forward"      # likewise
_HIP_FWD_X16 = "_mhaq_bn_hip_forward_x16"      # likewise
_POOL_X16 = "_mhaq_bn_pool_x16"      # likewise


def enabled_by_env() -> bool:
    """False when MHAQ_BN_BACKWARD=0 (or "false" / "off") is set."""
    return os.environ.get(ENV_SWITCH, "1").strip().lower() not in ("0", "false", "off", "no")


def x16_enabled(configured: bool = False) -> bool:
    """The 16-bit route's switch: `configured` (QATConfig.hip_bn_backward_16bit) unless MHAQ_BN_BACKWARD_X16 is set, which
    then decides: "1" / "true" / "on" / "yes" enable it, anything else disables it."""
    return _env_or(ENV_SWITCH_X16, configured)


def hip_forward_enabled(configured: bool = False) -> bool:
    """The HIP forward's switch: `configured` (QATConfig.hip_bn_forward) unless MHAQ_BN_FORWARD is set, which then decides,
    as in x16_enabled()."""
    return _env_or(ENV_SWITCH_FORWARD, configured)


def hip_forward_x16_enabled(configured: bool = False) -> bool:
    """The 16-bit HIP forward's switch: `configured` (QATConfig.hip_bn_forward_16bit) unless MHAQ_BN_FORWARD_X16 is set, which
    then decides, as in x16_enabled().  The forward runs only where the 16-bit backward's switch is on as well."""
    return _env_or(ENV_SWITCH_FORWARD_X16, configured)


def pool_x16_enabled(configured: bool = False) -> bool:
    """The 16-bit pooled stem node's switch: `configured` (QATConfig.fuse_stem_pool_16bit) unless MHAQ_STEM_POOL_X16 is set,
    which then decides, as in x16_enabled().  The node runs only where the 16-bit backward's switch is on as well."""
    return _env_or(ENV_SWITCH_POOL_X16, configured)


def _env_or(name: str, configured: bool) -> bool:
    v = os.environ.get(name)
    if v is None or not v.strip():
        return bool(configured)
    return v.strip().lower() in ("1", "true", "on", "yes")


class HipBackwardBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d whose training forward goes through the compiled node; nn.BatchNorm2d.forward runs otherwise."""

    def takes_node(self, input) -> bool:
        """True when this call goes through the compiled node (forward() and forward_pooled() decide alike)."""
        if (not self.training or not self.track_running_stats or not self.affine or not input.is_cuda
                or self.weight.dtype != torch.float32):
            return False
        return input.dtype == torch.float32 or (self.takes_x16() and input.dtype in (torch.bfloat16, torch.float16))

    def takes_x16(self) -> bool:
        """True when install(..., x16=True) enabled the 16-bit backward for this module."""
        return bool(self.__dict__.get(_X16, False))

    def takes_hip_forward(self) -> bool:
        """True when install(..., hip_forward=True) enabled the HIP forward (of float32 inputs) for this module."""
        return bool(self.__dict__.get(_HIP_FWD, False))

    def takes_hip_forward_x16(self) -> bool:
        """True when install(..., hip_forward_x16=True) enabled the HIP forward of 16-bit inputs for this module (it runs only
        where takes_x16() holds as well)."""
        return bool(self.__dict__.get(_HIP_FWD_X16, False))

    def takes_pool_x16(self) -> bool:
        """True when install(..., pool_x16=True) enabled the 16-bit pooled node for this module (it runs only where takes_x16()
        holds as well)."""
        return bool(self.__dict__.get(_POOL_X16, False))

    def takes_pooled_node(self, input) -> bool:
        """True when forward_pooled() applies: a float32 input, or a 16-bit one on a module with x16 and pool_x16."""
        if not self.takes_node(input):
            return False
        return input.dtype == torch.float32 or (self.takes_x16() and self.takes_pool_x16())

    def _step_average_factor(self) -> float:
        """The bookkeeping of _BatchNorm.forward (training mode, tracked statistics): counts the batch, returns the
        exponential average factor of this call."""
        exponential_average_factor = 0.0 if self.momentum is None else self.momentum
        if self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
            if self.momentum is None:
                exponential_average_factor = 1.0 / float(self.num_batches_tracked)
            else:
                exponential_average_factor = self.momentum
        return exponential_average_factor

    def _node(self, entry, input, *more):
        self._check_input_dim(input)
        return entry(input, self.weight, self.bias, self.running_mean, self.running_var, self._step_average_factor(),
                     self.eps, torch.backends.cudnn.enabled, *more)

    def forward(self, input):
        if not self.takes_node(input):
            return super().forward(input)
        from . import _ext
        x16 = input.dtype != torch.float32
        return self._node(_ext.ext().bn_train, input, x16, not x16 and self.takes_hip_forward(),
                          x16 and self.takes_x16() and self.takes_hip_forward_x16())

    def forward_pooled(self, input):
        """max_pool2d(self(input), 3, 2, 1) as one node (bn_pool_train: the BatchNorm output is not kept, the backward
        gathers its dy from the pooled gradient).  Call only when takes_pooled_node(input) holds.  A 16-bit input the compiled
        side finds ineligible (NCHW, C % 8 != 0, N * H * W == 1) runs as max_pool2d(self(input), 3, 2, 1) there, under this
        module's other flags."""
        from . import _ext
        if input.dtype == torch.float32:
            return self._node(_ext.ext().bn_pool_train, input, self.takes_hip_forward())
        return self._node(_ext.ext().bn_pool_train, input, False, self.takes_x16(), self.takes_pool_x16(),
                          self.takes_x16() and self.takes_hip_forward_x16())


def install(model: nn.Module, x16: bool = False, hip_forward: bool = False, hip_forward_x16: bool = False,
            pool_x16: bool = False) -> int:
    """Give every nn.BatchNorm2d of `model` (the exact type) the forward above; x16=True also enables the 16-bit backward
    on them, hip_forward=True the HIP forward of float32 inputs, hip_forward_x16=True (with x16) that of 16-bit inputs,
    pool_x16=True (with x16) the pooled node on 16-bit inputs.  Returns the number of modules switched."""
    switched = 0
    for m in model.modules():
        if type(m) is nn.BatchNorm2d:
            m.__class__ = HipBackwardBatchNorm2d
            if x16:
                m.__dict__[_X16] = True
            if hip_forward:
                m.__dict__[_HIP_FWD] = True
            if hip_forward_x16:
                m.__dict__[_HIP_FWD_X16] = True
            if pool_x16:
                m.__dict__[_POOL_X16] = True
            switched += 1
    return switched


def uninstall(model: nn.Module) -> None:
    for m in model.modules():
        if type(m) is HipBackwardBatchNorm2d:
            m.__class__ = nn.BatchNorm2d
            m.__dict__.pop(_X16, None)
            m.__dict__.pop(_HIP_FWD, None)
            m.__dict__.pop(_HIP_FWD_X16, None)
            m.__dict__.pop(_POOL_X16, None)
