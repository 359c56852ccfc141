"""ReLU and residual add inside the activation quantizer's kernels, for nets.BasicBlock and the nets.ResNet18 stem.

A quantized BasicBlock runs a NoisyAct directly behind each of its ReLUs:

  mid-block   bn1 -> relu -> conv2.activations_quantizer -> conv2.0
  block end   relu(bn2(..) + identity) -> the NEXT block's conv1.activations_quantizer (and its residual branch)
  stem        bn1 -> relu -> maxpool -> layer1.0.conv1.activations_quantizer (and layer1.0's residual branch)

As separate modules these are two or three full passes over the activation tensor per direction next to the quantizer's
own (torch's add, clamp_min, threshold_backward and autograd's accumulation of the two gradients of the ReLU output).
NoisyAct.forward_fused (ops.act_relu_layer -> mhaq_fq_act_relu_fwd / _bwd) takes the ReLU's input instead: one forward and
one backward kernel per place, and every value -- y, a, the gradients, the parameter gradients, the random signs -- is
the one the separate modules give (ReLU, a two-term fp32 add and a mask are exact elementwise operations).  Under
torch.autocast the tensors are 16-bit and the same places take mhaq_fq_act_relu_*_x16, which give the BITS of the separate
16-bit modules: the 16-bit add and the accumulation of the two gradients round, and the kernels round where those launches
round (the accumulated gradient twice; include/mhaq_fq.h, DESIGN.md sections 10-11).

  * Block end: the producing block quantizes for its consumer.  It returns a = relu(bn2 + identity) as before, an ordinary
    tensor, and pins the consumer's quantized input to it (`a._mhaq_fq = (quantizer, y)`); the consumer takes it off and
    feeds its conv1.0 directly.  The last block of the net has no quantizer behind it and keeps add + relu.
  * Stem: maxpool(relu(t)) == relu(maxpool(t)) in value and in gradient (max is monotone; a window whose maximum is not
    positive sends no gradient either way), so the pool runs on the BatchNorm output and the ReLU moves into layer1.0's
    first quantizer, on a quarter of the elements.

install() switches the CLASS of the stock modules (FusedBasicBlock / FusedResNet18 are subclasses that add a forward and
nothing else): module names, named_modules() order, state_dict keys, copy.deepcopy and torch.save(model) are what they
were.  The decision to fuse is taken per call and per place; the original forward runs otherwise.  A place is fused only
  - in training mode, on dense device tensors that are float32 or, under torch.autocast, of the autocast dtype (the addend
    sharing z's dtype and strides),
  - with the stock mhaq_amd.layers.NoisyAct, not disabled, not AEWGS,
  - when no forward, pre-forward or backward hook sits on a module whose forward would be bypassed or whose input would
    change (the nn.ReLU, the NoisyAct, the wrapping Sequential; for a block end also the two blocks and their containers,
    which hand the pinned tensor on; for the stem also the pool) and no global module hook is registered.
Eval mode, calibration and hook-based observers therefore always see the original modules.  BatchNorm is untouched: the
fused path is the same under DDP and SyncBatchNorm.

  * Stem pool: where the stem's bn1 is a bn_backward.HipBackwardBatchNorm2d that takes its compiled node on this input and
    the pool is exactly nn.MaxPool2d(3, 2, 1), both hook-free, BatchNorm and pool run as ONE node
    (HipBackwardBatchNorm2d.forward_pooled): the [N,64,112,112] BatchNorm output is not kept for the backward, no int64
    indices are written, and the BatchNorm backward gathers its dy from the pooled gradient instead of reading one the
    pool's backward wrote.  Same bits in every output and gradient.  fp32 by default: under autocast
    takes_pooled_node() is false and the stem runs maxpool(bn(c)) in front of the fused quantizer, also where the BatchNorm's
    own 16-bit backward is enabled -- unless bn_backward.install(x16=True, pool_x16=True) flagged the module, which makes
    takes_pooled_node() true for a 16-bit input and sends it through the 16-bit pooled node (opt-in,
    the stem's y and statistics become the HIP forward's).

MHAQ_FUSE_BLOCKS=0 in the environment keeps QATTrainer from installing (A/B runs of an unchanged benchmark);
QATConfig.fuse_blocks=False does the same per trainer.  MHAQ_STEM_POOL=0 / QATConfig.fuse_stem_pool=False keep only the
stem pool's node out (install(stem_pool=False)).
"""
from __future__ import annotations

import os

import torch
from torch import nn
from torch.nn.modules import module as _nn_module

from . import nets
from .bn_backward import HipBackwardBatchNorm2d
from .layers import NoisyAct

ENV_SWITCH = "MHAQ_FUSE_BLOCKS"
ENV_SWITCH_STEM_POOL = "MHAQ_STEM_POOL"
_TAG = "_mhaq_fq"
_STEM_POOL = "_mhaq_stem_pool"


def enabled_by_env() -> bool:
    """False when MHAQ_FUSE_BLOCKS=0 (or "false" / "off") is set."""
    return os.environ.get(ENV_SWITCH, "1").strip().lower() not in ("0", "false", "off", "no")


def stem_pool_enabled_by_env() -> bool:
    """False when MHAQ_STEM_POOL=0 (or "false" / "off") is set."""
    return os.environ.get(ENV_SWITCH_STEM_POOL, "1").strip().lower() not in ("0", "false", "off", "no")


def _hook_free(*mods) -> bool:
    for m in mods:
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks:
            return False
    return True


def _no_global_hooks() -> bool:
    return not (_nn_module._global_forward_hooks or _nn_module._global_forward_pre_hooks
                or _nn_module._global_backward_hooks or _nn_module._global_backward_pre_hooks)


def _wrapped_quantizer(seq):
    """The stock NoisyAct of a wrapped convolution -- Sequential(activations_quantizer, "0"), wrap.quantize_model -- or None."""
    if type(seq) is not nn.Sequential or len(seq._modules) != 2:
        return None
    q = seq._modules.get("activations_quantizer")
    if type(q) is not NoisyAct or "0" not in seq._modules:
        return None
    return q


def _bypassable(seq, relu):
    """The quantizer of `seq` if this call may skip seq.forward and relu.forward, else None."""
    q = _wrapped_quantizer(seq)
    if q is None or type(relu) is not nn.ReLU or not _hook_free(seq, relu):
        return None
    return q


def _take_pinned(x, seq):
    """The quantized input a producing block pinned to x for the quantizer of `seq`, or None."""
    tag = getattr(x, _TAG, None) if isinstance(x, torch.Tensor) else None
    if tag is None:
        return None
    delattr(x, _TAG)
    return tag[1] if tag[0] is seq._modules.get("activations_quantizer") else None


def _is_stem_pool(mp) -> bool:
    """Exactly nn.MaxPool2d(3, 2, 1): the one geometry mhaq_fq_maxpool3s2_fwd / mhaq_fq_bn_pool_bwd implement."""
    def both(v, k):
        return v == k or v == (k, k) or v == [k, k]
    return (type(mp) is nn.MaxPool2d and both(mp.kernel_size, 3) and both(mp.stride, 2) and both(mp.padding, 1)
            and both(mp.dilation, 1) and not mp.ceil_mode and not mp.return_indices)


class FusedBasicBlock(nets.BasicBlock):
    """nets.BasicBlock with the fused places; nets.BasicBlock.forward is what runs wherever a place cannot be fused."""

    def forward(self, x):
        y1 = _take_pinned(x, self.conv1)
        fusing = self.training and _no_global_hooks()
        out = self.conv1._modules["0"](y1) if y1 is not None else self.conv1(x)
        z = self.bn1(out)
        # mid-block: bn1 -> [relu -> quantizer] -> conv2.0
        q2 = _bypassable(self.conv2, self.relu) if fusing else None
        if q2 is not None and q2.can_fuse_relu(z):
            y2, _ = q2.forward_fused(z)
            out = self.conv2._modules["0"](y2)
        else:
            out = self.conv2(self.relu(z))
        out = self.bn2(out)
        identity = x if self.downsample is None else self.downsample(x)
        # block end: [add -> relu -> the consumer's quantizer]
        nxt = self.__dict__.get("_mhaq_next") if fusing else None
        if nxt is not None and nxt.training and type(nxt) is FusedBasicBlock:
            qn = _bypassable(nxt.conv1, self.relu)
            if (qn is not None and _hook_free(self, nxt, *self.__dict__.get("_mhaq_path", ()))
                    and qn.can_fuse_relu(out, identity)):
                y, a = qn.forward_fused(out, identity, want_act=True)
                setattr(a, _TAG, (qn, y))
                return a
        return self.relu(out + identity)


class FusedResNet18(nets.ResNet18):
    """nets.ResNet18 whose stem ReLU runs behind the pool, inside layer1.0's first quantizer."""

    def forward(self, x):
        first = self.layer1[0] if len(self.layer1) else None
        c = self.conv1(x)
        t = None
        fused = False
        if (self.training and _no_global_hooks() and type(first) is FusedBasicBlock and first.training
                and type(self.maxpool) is nn.MaxPool2d):
            q = _bypassable(first.conv1, self.relu)
            # (BatchNorm and pool keep dtype, device and density: what holds for the convolution's output holds for theirs)
            if q is not None and _hook_free(self.maxpool, self.layer1, first) and q.can_fuse_relu(c):
                bn = self.bn1
                if (self.__dict__.get(_STEM_POOL) and type(bn) is HipBackwardBatchNorm2d and bn.takes_pooled_node(c)
                        and _is_stem_pool(self.maxpool) and _hook_free(bn)):
                    p = bn.forward_pooled(c)
                else:
                    t = bn(c)
                    p = self.maxpool(t)
                y, a = q.forward_fused(p, None, want_act=True)
                setattr(a, _TAG, (q, y))
                x, fused = a, True
        if not fused:
            x = self.maxpool(self.relu(self.bn1(c) if t is None else t))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def _fusable_block(m) -> bool:
    return type(m) is nets.BasicBlock and (_wrapped_quantizer(m.conv1) is not None
                                           or _wrapped_quantizer(m.conv2) is not None)


def install(model: nn.Module, stem_pool: bool = True) -> int:
    """Give every quantized nets.BasicBlock of `model` (wrap.quantize_model with the stock layers) the fused forward, and
    a nets.ResNet18 the fused stem and the links from each block to its consumer.  Returns the number of modules switched;
    a model wrapped with other layer classes (the CPU checker's) is left alone.  stem_pool: whether a fused stem may run
    its BatchNorm and pool as one node."""
    switched = 0
    for m in list(model.modules()):
        if _fusable_block(m):
            m.__class__ = FusedBasicBlock
            switched += 1
    for m in list(model.modules()):
        if type(m) is nets.ResNet18:
            layers = [m.layer1, m.layer2, m.layer3, m.layer4]
            if not all(type(lay) is nn.Sequential for lay in layers):
                continue
            chain = [(b, lay) for lay in layers for b in lay]
            if not chain or any(type(b) is not FusedBasicBlock for b, _ in chain):
                continue
            for (b, lay), (nb, nlay) in zip(chain, chain[1:]):
                # plain references kept off nn.Module's registries: no new submodule, nothing in the state_dict
                b.__dict__["_mhaq_next"] = nb
                b.__dict__["_mhaq_path"] = (lay,) if nlay is lay else (lay, nlay)
            m.__class__ = FusedResNet18
            m.__dict__[_STEM_POOL] = bool(stem_pool)
            switched += 1
    return switched


def uninstall(model: nn.Module) -> None:
    for m in model.modules():
        if type(m) is FusedBasicBlock:
            m.__dict__.pop("_mhaq_next", None)
            m.__dict__.pop("_mhaq_path", None)
            m.__class__ = nets.BasicBlock
        elif type(m) is FusedResNet18:
            m.__dict__.pop(_STEM_POOL, None)
            m.__class__ = nets.ResNet18
