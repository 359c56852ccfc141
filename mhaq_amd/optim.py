"""FusedRAdam: torch.optim.RAdam whose step is ONE HIP launch (mhaq_fq_radam_step, csrc/optim.hip).

torch.optim.RAdam in its foreach form -- what QATTrainer stepped until now -- walks the parameters in 9 op launches per ~24
tensors: 20 launches, 21 tensor-passes and a parameter-sized temporary per ResNet-18 step.  The update itself needs 7 passes
(read p, g, m, v; write p, m, v); the kernel makes those, with the foreach chain's arithmetic line by line, so p, exp_avg and
exp_avg_sq keep the bits torch.optim.RAdam(foreach=True) gives on the same device (tests/test_gpu_fused_radam.py).

Only step() is overridden.  The state is torch's own -- `step` (a CPU tensor), `exp_avg`, `exp_avg_sq`, created by the parent
class's _init_group -- so state_dict() / load_state_dict() are interchangeable with torch.optim.RAdam in both directions.

A parameter takes the fused launch when its group has weight_decay == 0, maximize / capturable / differentiable off and a
Python-float lr, and p, p.grad, exp_avg and exp_avg_sq are dense, non-overlapping float32 tensors on one GPU in the same
memory order (equal strides once the dimensions of size 1 are dropped).  Every other parameter of the group goes through
torch's _multi_tensor_radam in the same step() -- never silently: fused_radam_fallbacks() counts them.  This class is the
foreach form throughout: a group's `foreach` entry is not consulted.
"""
from __future__ import annotations

import os

import torch
from torch.optim.optimizer import _use_grad_for_differentiable
from torch.optim.radam import _multi_tensor_radam, radam as _radam

ENV_SWITCH = "MHAQ_FUSED_RADAM"

_fallbacks = 0


def enabled(configured: bool = True) -> bool:
    """The trainer's switch: `configured` (QATConfig.fused_optimizer) unless MHAQ_FUSED_RADAM is set, which then decides:
    "1" / "true" / "on" / "yes" enable the fused step, anything else disables it."""
    v = os.environ.get(ENV_SWITCH)
    if v is None or not v.strip():
        return bool(configured)
    return v.strip().lower() in ("1", "true", "on", "yes")


def fused_radam_steps() -> int:
    """Launches of mhaq_fq_radam_step so far in this process."""
    from . import _ext
    return int(_ext.ext().fused_radam_steps())


def fused_radam_fallbacks() -> int:
    """Parameter updates that FusedRAdam.step() handed to torch's foreach implementation so far in this process."""
    return _fallbacks


def radam_scalars(step: float, lr: float, beta1: float, beta2: float):
    """(c1, c2) = (unrect_step_size, bias_correction2) of a tensor at step count `step`: Python doubles, operation for
    operation those of _multi_tensor_radam's non-capturable branch.  Up to step 5 (rho_t <= 5) c2 is -0.0."""
    rho_inf = 2 / (1 - beta2) - 1
    rho_t = rho_inf - 2 * step * (beta2 ** step) / (1 - beta2 ** step)
    rect = (((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5
            if rho_t > 5 else 0)
    unrectified = 0 if rect > 0 else 1.0
    bias_correction1 = 1 - beta1 ** step
    c1 = (lr * unrectified / bias_correction1) * -1
    c2 = ((1 - beta2 ** step) ** 0.5) * (lr * rect / bias_correction1) * -1
    return c1, c2


def group_fallback_reason(group):
    """Why a parameter group cannot take the fused launch (None: it can)."""
    if group["weight_decay"] != 0:
        return "weight_decay"
    for flag in ("maximize", "capturable", "differentiable"):
        if group.get(flag, False):
            return flag
    if type(group["lr"]) is not float:
        return "lr"
    return None


def _memory_order(t):
    return tuple((n, s) for n, s in zip(t.shape, t.stride()) if n != 1)


def _dense(order) -> bool:
    expect = 1
    for n, s in sorted(order, key=lambda ns: ns[1]):
        if s != expect:
            return False
        expect *= n
    return True


_dense_orders = {}


def tensor_fallback_reason(p, g, m, v, require_gpu: bool = True):
    """Why one parameter cannot take the fused launch (None: it can).  require_gpu=False leaves the device type out, so
    that the rule can be exercised on CPU tensors."""
    ts = (p, g, m, v)
    for t in ts:
        if t.dtype is not torch.float32:
            return "dtype"
    dev = p.device
    if (require_gpu and dev.type != "cuda") or g.device != dev or m.device != dev or v.device != dev:
        return "device"
    for t in ts:
        if t.layout is not torch.strided:
            return "layout"
    order = _memory_order(p)
    if not (p.shape == g.shape == m.shape == v.shape) or not (order == _memory_order(g) == _memory_order(m)
                                                              == _memory_order(v)):
        return "order"
    ok = _dense_orders.get(order)
    if ok is None:
        if len(_dense_orders) > 4096:
            _dense_orders.clear()
        ok = _dense_orders[order] = p.numel() == 0 or _dense(order)
    return None if ok else "dense"


class FusedRAdam(torch.optim.RAdam):
    """See the module docstring.  Constructor, state and state_dict are torch.optim.RAdam's."""

    _one = None

    @_use_grad_for_differentiable
    def step(self, closure=None):
        global _fallbacks
        self._cuda_graph_capture_health_check()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, steps = [], [], [], [], []
            beta1, beta2 = group["betas"]
            has_complex = self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, steps)
            if not params:
                continue
            if group_fallback_reason(group) is None:
                rest = [i for i in range(len(params))
                        if tensor_fallback_reason(params[i], grads[i], exp_avgs[i], exp_avg_sqs[i]) is not None]
            else:
                rest = list(range(len(params)))
            if rest:
                _fallbacks += len(rest)
                pick = lambda xs: [xs[i] for i in rest]      # noqa: E731
                kw = dict(beta1=beta1, beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"],
                          decoupled_weight_decay=group["decoupled_weight_decay"], differentiable=group["differentiable"],
                          maximize=group["maximize"], capturable=group["capturable"], has_complex=has_complex)
                lists = (pick(params), pick(grads), pick(exp_avgs), pick(exp_avg_sqs), pick(steps))
                if group["differentiable"]:          # the foreach ops do not record a graph: torch's per-tensor form
                    _radam(*lists, foreach=False, **kw)
                else:
                    _multi_tensor_radam(*lists, **kw)
                if len(rest) == len(params):
                    continue
                skip = set(rest)
                keep = [i for i in range(len(params)) if i not in skip]
                params, grads, exp_avgs, exp_avg_sqs, steps = ([xs[i] for i in keep]
                                                               for xs in (params, grads, exp_avgs, exp_avg_sqs, steps))
            self._fused(group, params, grads, exp_avgs, exp_avg_sqs, steps, beta1, beta2)
        return loss

    def _fused(self, group, params, grads, exp_avgs, exp_avg_sqs, steps, beta1, beta2):
        from . import _ext
        if FusedRAdam._one is None:
            FusedRAdam._one = torch.tensor(1.0, device="cpu")
        torch._foreach_add_(steps, FusedRAdam._one, alpha=1.0)       # as _multi_tensor_radam does for CPU step counts
        lr = group["lr"]
        memo, c1s, c2s = {}, [], []
        for s in steps:
            k = s.item()
            c = memo.get(k)
            if c is None:
                c = memo[k] = radam_scalars(k, lr, beta1, beta2)
            c1s.append(c[0])
            c2s.append(c[1])
        by_device = {}
        for i, p in enumerate(params):
            by_device.setdefault(p.device, []).append(i)
        for idx in by_device.values():
            pick = (lambda xs: xs) if len(idx) == len(params) else (lambda xs: [xs[i] for i in idx])
            _ext.ext().radam_step(pick(params), pick(grads), pick(exp_avgs), pick(exp_avg_sqs), pick(c1s), pick(c2s),
                                  beta1, beta2, group["eps"])
