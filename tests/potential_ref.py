"""Checker code for the PotentialLoss kernels (mhaq_fq_potential_loss_fwd / _bwd, mhaq_amd/loss.py: FusedPotentialLoss*):

  ref64(base, las, laq, lws, lwq, a_bits, w_bits, state, p, lossless, g)
        gdnsq_loss.py:47-84 as a high-precision yardstick that keeps the reference's active sets.  Per element it runs the
        reference's own float32 statements on the CPU -- d = lwq - lws, h = d - (bits - 1e-3), max(0, h), .pow(p), > 0: single
        IEEE operations, whose float64 restatement would flip a hinge within an ulp of zero and with it wact / aact and wmul --
        and from there on everything in float64: the counts are exact integers, the means, calib, wmul, amul, ploss, cw, ca, cb
        are float64.  out[11] is the float32 (lwq - lws).max(), NaN-propagating as torch's.  Returns the 12 outputs, the state
        after a training step and the closed-form gradients g_lwq = g cw hinge'(h), g_lws = -g_lwq (activations alike);
        hinge' is 1/2 at h == 0 for p == 1 (torch.max splits there) and p h^(p-1), hence 0 at the tie, for p == 2.
  chain32(...)   the framework's float32 chain where the tensors live: oracle/fq_eager.potential_loss with autograd; the means, the
                 logged statistics and the three multipliers by the same statements as float32 tensor operations
  scalar_bar / grad_bar   the accuracy bars of the GPU tests (distill_ref.MARGIN, ulp32)
  make_inputs / plant_tie seeded inputs on a grid of 2^-10 with magnitude below 16: lwq - lws is exact in float32, so the sign of h is
                 the same in float32 and float64

No kernel is involved in any of them."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests.distill_ref import MARGIN, ulp32

L_EPS = float(np.float32(1e-3))             # the reference's l_eps is a float32 tensor
OUT_NAMES = ["ploss", "wloss", "aloss", "rloss", "cw", "ca", "cb", "-mean lws", "mean lwq", "-mean las", "mean laq",
             "max(lwq-lws)"]
GRAD_NAMES = ["g_las", "g_laq", "g_lws", "g_lwq"]
GRID = 2.0 ** -10


def threshold(bits):
    """float32(bits) - float32(1e-3) in float32: the reference's (bits - l_eps), the kernel's bits - 1e-3f."""
    return torch.tensor(float(bits), dtype=torch.float32) - torch.tensor(1e-3, dtype=torch.float32)


def _f32(v):
    return v.detach().to(torch.float32).cpu().reshape(-1)


def _side(ls, lq, bits, p):
    """One side's hinge by the reference's float32 statements -> (elements, count of active, h in float32, h in float64)."""
    thr = threshold(bits)
    d = lq - ls
    h = d - thr
    e = torch.max(torch.tensor(0), h).pow(torch.tensor(p))
    return e, int((e > 0).sum()), h, d.double() - thr.double()


def _hinge_grad(h32, h64, p):
    """d/dh of max(0, h)^p in float64; the branch is the float32 sign of h (what every float32 evaluation sees)."""
    d = torch.ones_like(h64) if p == 1 else p * h64.clamp_min(0).pow(p - 1)
    out = torch.where(h32 > 0, d, torch.where(h32 == 0, 0.5 * d, torch.zeros_like(d)))
    return torch.where(torch.isnan(h32), torch.full_like(d, math.nan), out)


def ref64(base, las, laq, lws, lwq, a_bits, w_bits, state, p=1, lossless=False, g=1.0):
    """state = (loss_sum, cnt, t) as the call finds it (calib is read before the update).  -> namespace with out (12 floats),
    state (after a training step), g_base (float) and g_las / g_laq / g_lws / g_lwq (float64 tensors)."""
    las, laq, lws, lwq = _f32(las), _f32(laq), _f32(lws), _f32(lwq)
    na, nw = las.numel(), lws.numel()
    b = float(_f32(torch.as_tensor(base))[0])
    loss_sum, cnt, t = float(state[0]), float(state[1]), float(state[2])
    we, wact, wh32, wh64 = _side(lws, lwq, w_bits, p)
    ae, aact, ah32, ah64 = _side(las, laq, a_bits, p)
    wloss, aloss = float(we.double().sum()) / nw, float(ae.double().sum()) / na
    rloss = b ** p
    calib = loss_sum / cnt
    wmul = (wact + L_EPS) / (wact + aact + L_EPS)
    amul = (aact + L_EPS) / (wact + aact + L_EPS)
    l1, l2 = (1.0, t) if lossless else (t, 1.0)
    ploss = calib * l1 * (wmul * wloss + amul * aloss) + l2 * rloss
    cw, ca = calib * l1 * wmul / nw, calib * l1 * amul / na
    cb = l2 * (1.0 if p == 1 else p * b ** (p - 1))
    out = [ploss, wloss, aloss, rloss, cw, ca, cb,
           -float(lws.double().sum()) / nw, float(lwq.double().sum()) / nw,
           -float(las.double().sum()) / na, float(laq.double().sum()) / na,
           float((lwq - lws).max())]
    g = float(g)
    g_lwq, g_laq = g * cw * _hinge_grad(wh32, wh64, p), g * ca * _hinge_grad(ah32, ah64, p)
    return SimpleNamespace(out=out, state=(loss_sum + rloss, cnt + 1.0, t), g_base=g * cb, g_las=-g_laq, g_laq=g_laq,
                           g_lws=-g_lwq, g_lwq=g_lwq, wact=wact, aact=aact, wh=wh32, ah=ah32)


def chain32(base, las, laq, lws, lwq, a_bits, w_bits, state, p=1, lossless=False, g=1.0):
    """The framework's float32 chain on the device of the tensors.  state[0] may be a float32 tensor (a running sum carried
    from call to call) or a float.  Same fields as ref64; out and state hold float32 values."""
    from oracle import fq_eager as O
    leaves = [v.detach().float().reshape(-1).clone().requires_grad_(True) for v in (las, laq, lws, lwq)]
    bl = torch.as_tensor(base).detach().float().reshape(()).to(leaves[0].device).clone().requires_grad_(True)
    loss_sum = torch.as_tensor(state[0], dtype=torch.float32)
    cnt, t = int(state[1]), float(state[2])
    ploss, rloss = O.potential_loss(bl * 1.0, *leaves, a_bits, w_bits, t, loss_sum, cnt, lossless=lossless, p=p)
    grads = torch.autograd.grad(ploss * g, [bl] + leaves)
    with torch.no_grad():
        a, s, w, q = leaves
        # the intermediates of gdnsq_loss.py:47-62 and what it logs next to the loss (:73-84), statement for statement
        l_eps = torch.tensor(1e-3)
        wloss0 = torch.max(torch.tensor(0), (q - w) - (w_bits - l_eps)).pow(torch.tensor(p))
        aloss0 = torch.max(torch.tensor(0), (s - a) - (a_bits - l_eps)).pow(torch.tensor(p))
        wloss, aloss = wloss0.mean(), aloss0.mean()
        wact, aact = (wloss0 > 0).sum().cpu(), (aloss0 > 0).sum().cpu()
        calib = loss_sum.cpu() / cnt
        wmul, amul = (wact + l_eps) / (wact + aact + l_eps), (aact + l_eps) / (wact + aact + l_eps)
        l1, l2 = (1.0, t) if lossless else (t, 1.0)
        cb = torch.tensor(l2, dtype=torch.float32) * (1.0 if p == 1 else p * bl.detach().cpu().pow(p - 1))
        out = [ploss, wloss, aloss, rloss, calib * l1 * wmul / w.numel(), calib * l1 * amul / a.numel(), cb,
               -w.mean(), q.mean(), -a.mean(), s.mean(), (q - w).max()]
        out = [float(v) for v in out]
        new_sum = loss_sum.cpu() + rloss.detach().cpu()
    return SimpleNamespace(out=out, state=(new_sum.float(), cnt + 1.0, t), g_base=float(grads[0]),
                           g_las=grads[1].detach(), g_laq=grads[2].detach(), g_lws=grads[3].detach(),
                           g_lwq=grads[4].detach())


# ------------------------------------------------------------------------------------------------- bars
def scalar_bar(v32, v64, margin=MARGIN):
    """|v - v64| <= margin |v_torch32 - v64| + 8 ulp32(v64)"""
    return margin * abs(float(v32) - float(v64)) + 8 * ulp32(v64)


def grad_bar(g32, g64, margin=MARGIN):
    """max|g - g64| <= margin max|g_torch32 - g64| + 8 2^-24 max|g64|"""
    g64 = g64.double().cpu()
    return margin * float((g32.double().cpu() - g64).abs().max()) + 8 * 2.0 ** -24 * float(g64.abs().max())


def scalar_share(v, v32, v64):
    """-> (ok, error / bar); a NaN or infinite yardstick asks for the same special value."""
    v, v64 = float(v), float(v64)
    if math.isnan(v64):
        return math.isnan(v), 0.0
    if math.isinf(v64):
        return v == v64, 0.0
    err, bar = abs(v - v64), scalar_bar(v32, v64)
    return err <= bar, err / bar


def grad_share(gx, g32, g64):
    err = float((gx.double().cpu().reshape(-1) - g64.double().cpu()).abs().max())
    bar = grad_bar(g32.reshape(-1), g64)
    return (err <= bar), (err / bar if bar else (0.0 if err == 0 else math.inf))


# ------------------------------------------------------------------------------------------------- inputs
def on_grid(v):
    """Rounded to the grid of 2^-10 and kept below 16 in magnitude."""
    return (torch.round(v.float() / GRID) * GRID).clamp(-16 + GRID, 16 - GRID)


def make_inputs(na, nw, a_bits, w_bits, seed, spread=1.5, a_shift=0.0, w_shift=0.0):
    """(las, laq, lws, lwq) on the grid, float32 on the CPU.  Each side's laq - las / lwq - lws is centred on its own threshold
    (+ shift), so about half of its hinges are active at shift 0; a shift of -12 / +12 leaves none / all active."""
    gen = torch.Generator().manual_seed(seed)
    las = on_grid(-5 + torch.randn(na, generator=gen))
    laq = on_grid(las + (a_bits + a_shift) + spread * torch.randn(na, generator=gen))
    lws = on_grid(-6 + torch.randn(nw, generator=gen))
    lwq = on_grid(lws + (w_bits + w_shift) + spread * torch.randn(nw, generator=gen))
    return las, laq, lws, lwq


def plant_tie(ls, lq, bits, idx):
    """Exact ties h == 0 at idx (in place): ls = -6, lq = fl32(-6 + threshold), so that (lq - ls) - threshold == 0 in float32."""
    thr = threshold(bits)
    ls[idx] = -6.0
    lq[idx] = torch.tensor(-6.0) + thr
    assert bool((((lq[idx] - ls[idx]) - thr) == 0).all())
    return ls, lq
