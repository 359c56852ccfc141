"""The elementwise chain of a FROZEN nets.ResNet18 -- the distillation teacher -- in one HIP launch per place.

A stock eval-mode ResNet-18 runs, between its convolutions, one launch per module: 20 BatchNorms, 17 in-place ReLUs, 8
residual adds and the stem's max pool, each a full pass over an activation tensor.  With the parameters and running
statistics frozen, a BatchNorm is y = (x - mean) * a + beta with per-channel constants that are computed ONCE
(mhaq_fq_bn_infer_consts), and what follows it rides in the same pass (mhaq_fq_bn_infer_act, mhaq_fq_bn_relu_pool3s2;
include/mhaq_fq.h):

  stem        conv1 -> [bn1 -> relu -> maxpool]                            the BatchNorm output is never stored
  mid-block   conv1 -> [bn1 -> relu] -> conv2
  block end   conv2 -> [bn2 (+ downsample.1 of downsample.0(x), or + x) -> add -> relu]

17 launches per forward instead of 46.  The arithmetic is the training forward's, not the
framework's eval kernel's: outputs agree with the stock modules to fp32 rounding, not bit for bit.

install() switches the CLASS of the stock modules (FrozenBasicBlock / FrozenResNet18 are subclasses that add a forward and
nothing else): module names, named_modules() order, state_dict keys, copy.deepcopy and torch.save(model) are what they
were.  The decision to fuse is taken per call and per place; the stock modules run otherwise.  A place is fused only
  - in eval mode (the container and the BatchNorm), with grad disabled or nothing that enters the place requiring grad,
  - where the BatchNorm is exactly nn.BatchNorm2d with running statistics, float32 on the input's device,
  - on dense channels_last float32 device tensors with C % 4 == 0 (under torch.autocast the inputs are 16-bit: stock path,
    unless the module is flagged for 16-bit inputs, below),
  - when no forward, pre-forward or backward hook sits on a module whose forward would be bypassed (the BatchNorm, the
    nn.ReLU, the downsample Sequential, the pool) and no global module hook is registered,
  - for the stem, with a pool that is exactly nn.MaxPool2d(3, 2, 1).

Each BatchNorm keeps its [3, C] constant slab next to it (allocated at install: its address is stable for a captured graph)
with the (_version, data_ptr) of weight, bias, running_mean and running_var and the eps it was computed from; a call that
finds another key -- load_state_dict, an optimizer step, a reassigned tensor -- recomputes the slab with one launch on the
current stream before it is used.

MHAQ_TEACHER_FUSED=0 in the environment keeps QATTrainer from installing on its teacher (A/B runs of an unchanged
benchmark); QATConfig.fuse_teacher=False does the same per trainer.

16-bit inputs (opt-in).  install(model, x16=True) flags each switched module (a plain entry in the
instance __dict__: no parameter, buffer or state_dict key; kept by deepcopy, dropped by uninstall; read with takes_x16()).  A
flagged place is also fused when every tensor that enters it is a dense channels_last device tensor of ONE 16-bit dtype with
C % 8 == 0 -- what a teacher under torch.autocast sees -- on mhaq_fq_bn_infer_act_x16 / mhaq_fq_bn_relu_pool3s2_x16: the fp32
arithmetic on the upcast inputs, rounded once into the input's dtype.  A place with mixed dtypes runs the stock modules; every
other condition, the slabs and their refresh key are the ones above; an unflagged module behaves as before.
QATConfig.fuse_teacher_16bit switches it on per trainer; MHAQ_TEACHER_FUSED_X16, when set, decides either way.
"""
from __future__ import annotations

import os

import torch
from torch import nn

from . import _ext, nets
from .fused_blocks import _hook_free, _is_stem_pool, _no_global_hooks
from .ops import BN2_ADD_RELU, BN_ADD_RELU, BN_RELU

ENV_SWITCH = "MHAQ_TEACHER_FUSED"
ENV_SWITCH_X16 = "MHAQ_TEACHER_FUSED_X16"
_HOLD = "_mhaq_frozen"
_X16 = "_mhaq_frozen_x16"      # per-module flag in the instance __dict__ (not a parameter, buffer or state_dict entry)


def enabled_by_env() -> bool:
    """False when MHAQ_TEACHER_FUSED=0 (or "false" / "off") is set."""
    return os.environ.get(ENV_SWITCH, "1").strip().lower() not in ("0", "false", "off", "no")


def x16_enabled(configured: bool = False) -> bool:
    """The 16-bit route's switch: `configured` (QATConfig.fuse_teacher_16bit) unless MHAQ_TEACHER_FUSED_X16 is set, which then
    decides: "1" / "true" / "on" / "yes" enable it, anything else disables it (as MHAQ_BN_BACKWARD_X16, bn_backward.py)."""
    v = os.environ.get(ENV_SWITCH_X16)
    if v is None or not v.strip():
        return bool(configured)
    return v.strip().lower() in ("1", "true", "on", "yes")


def takes_x16(module) -> bool:
    """True for a switched module that install(..., x16=True) flagged."""
    return bool(module.__dict__.get(_X16, False))


class _Consts:
    """The constant slab of one BatchNorm and what it was computed from (key None: not yet computed)."""

    def __init__(self, channels, device):
        self.slab = torch.empty(3, channels, dtype=torch.float32, device=device)
        self.key = None
        self.usable = False


def _key(bn):
    """What the slab depends on: identity and version of the four vectors, and eps."""
    return tuple(None if t is None else (t._version, t.data_ptr())
                 for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)) + (bn.eps,)


def _refresh(bn, hold, key) -> None:
    """Recompute the slab from the BatchNorm as it is now (one launch on the current stream), or mark it unusable."""
    dev = hold.slab.device
    vecs = (bn.running_mean, bn.running_var, bn.weight, bn.bias)
    hold.usable = all(t is None or (t.dtype is torch.float32 and t.device == dev and t.is_contiguous()
                                    and t.numel() == hold.slab.shape[1]) for t in vecs)
    if hold.usable:
        w, b = (None if t is None else t.detach() for t in vecs[2:])
        _ext.ext().bn_infer_consts(vecs[0].detach(), vecs[1].detach(), w, b, float(bn.eps), hold.slab)
    hold.key = key


def _fusable_tensor(x, x16=False) -> bool:
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        return False
    if x.dtype is torch.float32:
        lane = 4
    elif x16 and (x.dtype is torch.bfloat16 or x.dtype is torch.float16):
        lane = 8                    # channels in a lane's 16 bytes
    else:
        return False
    return (x.is_cuda and x.numel() > 0 and x.shape[1] % lane == 0 and x.is_contiguous(memory_format=torch.channels_last)
            and x.data_ptr() % 16 == 0)


def _grad_free(*tensors) -> bool:
    return not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in tensors)


def _consts(bn, x, x16=False):
    """The up-to-date constant slab of `bn` if this call may replace bn(x) by the fused launch, else None."""
    hold = bn.__dict__.get(_HOLD)
    if (hold is None or type(bn) is not nn.BatchNorm2d or bn.training or bn.running_mean is None or bn.running_var is None
            or not _hook_free(bn) or not _fusable_tensor(x, x16) or x.device != hold.slab.device
            or x.shape[1] != hold.slab.shape[1] or not _grad_free(x, bn.weight, bn.bias)):
        return None
    key = _key(bn)
    if key != hold.key:
        _refresh(bn, hold, key)
    return hold.slab if hold.usable else None


def _like(t, x) -> bool:
    """t can be the second stream of a launch over x (a fusable x: of its dtype, 16-bit or not)."""
    return (isinstance(t, torch.Tensor) and t.dtype is x.dtype and _fusable_tensor(t, True) and t.shape == x.shape
            and t.stride() == x.stride() and t.device == x.device)


def _conv_bn(ds) -> bool:
    """A downsample branch whose BatchNorm can ride in the block end's launch: Sequential(conv, BatchNorm), hook-free."""
    return (type(ds) is nn.Sequential and list(ds._modules) == ["0", "1"] and type(ds._modules["1"]) is nn.BatchNorm2d
            and _hook_free(ds))


class FrozenBasicBlock(nets.BasicBlock):
    """nets.BasicBlock with the fused places; the stock modules run wherever a place cannot be fused."""

    def forward(self, x):
        if self.training or type(self.relu) is not nn.ReLU or not _hook_free(self.relu) or not _no_global_hooks():
            return nets.BasicBlock.forward(self, x)
        x16 = takes_x16(self)
        c1 = self.conv1(x)
        k1 = _consts(self.bn1, c1, x16)
        # mid-block: [bn1 -> relu]
        out = _ext.ext().bn_infer_act(c1, k1, BN_RELU, x16=x16) if k1 is not None else self.relu(self.bn1(c1))
        c2 = self.conv2(out)
        k2 = _consts(self.bn2, c2, x16)
        # block end: [bn2 (+ the downsample branch's BatchNorm) -> add -> relu]
        ds = self.downsample
        if k2 is not None and _conv_bn(ds):
            d = ds._modules["0"](x)
            kd = _consts(ds._modules["1"], d, x16)
            if kd is not None and _like(d, c2):
                return _ext.ext().bn_infer_act(c2, k2, BN2_ADD_RELU, x2=d, consts2=kd, x16=x16)
            identity = ds._modules["1"](d)
        else:
            identity = x if ds is None else ds(x)
        if k2 is not None and _like(identity, c2) and _grad_free(identity):
            return _ext.ext().bn_infer_act(c2, k2, BN_ADD_RELU, residual=identity, x16=x16)
        return self.relu(self.bn2(c2) + identity)


class FrozenResNet18(nets.ResNet18):
    """nets.ResNet18 whose stem BatchNorm, ReLU and pool are one launch."""

    def forward(self, x):
        c = self.conv1(x)
        k = None
        if (not self.training and type(self.relu) is nn.ReLU and _is_stem_pool(self.maxpool)
                and _hook_free(self.relu, self.maxpool) and _no_global_hooks()
                and isinstance(c, torch.Tensor) and c.dim() == 4 and c.shape[0] * c.shape[2] * c.shape[3] < 2 ** 31):
            k = _consts(self.bn1, c, takes_x16(self))
        x = _ext.ext().bn_relu_pool(c, k, x16=takes_x16(self)) if k is not None else self.maxpool(self.relu(self.bn1(c)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def _batchnorms(m):
    """The BatchNorms a switched module may fuse."""
    if type(m) is FrozenResNet18:
        return [m.bn1]
    ds = m.downsample
    return [m.bn1, m.bn2] + ([ds._modules["1"]] if _conv_bn(ds) else [])


def install(model: nn.Module, x16: bool = False) -> int:
    """Give every stock nets.BasicBlock and nets.ResNet18 of `model` the fused eval forward, and each of their BatchNorms
    that lives on a GPU its constant slab.  Returns the number of modules switched.  A model on the CPU is switched too and
    runs the stock modules (it has no slabs; install again after moving it).  x16: flag the switched modules so that their
    places take 16-bit inputs too (takes_x16(); without it a module installed earlier loses the flag)."""
    switched = 0
    for m in list(model.modules()):
        if type(m) is nets.BasicBlock:
            m.__class__ = FrozenBasicBlock
        elif type(m) is nets.ResNet18:
            m.__class__ = FrozenResNet18
        elif type(m) not in (FrozenBasicBlock, FrozenResNet18):
            continue
        switched += 1
        if x16:
            m.__dict__[_X16] = True
        else:
            m.__dict__.pop(_X16, None)
        for bn in _batchnorms(m):
            rm = getattr(bn, "running_mean", None)
            if type(bn) is nn.BatchNorm2d and isinstance(rm, torch.Tensor) and rm.is_cuda and bn.num_features % 4 == 0:
                # a plain attribute kept off nn.Module's registries: nothing in the state_dict, no new buffer
                bn.__dict__[_HOLD] = _Consts(bn.num_features, rm.device)
    return switched


def uninstall(model: nn.Module) -> None:
    for m in model.modules():
        if type(m) in (FrozenBasicBlock, FrozenResNet18):
            for bn in _batchnorms(m):
                bn.__dict__.pop(_HOLD, None)
            m.__dict__.pop(_X16, None)
            m.__class__ = nets.BasicBlock if type(m) is FrozenBasicBlock else nets.ResNet18
