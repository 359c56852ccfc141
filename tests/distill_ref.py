"""Checker code for the fused distillation losses (mhaq_fq_distill_loss_fwd / _bwd, mhaq_amd/loss.py: FusedDistillLoss):

  torch_loss(kind, x, t)      the six losses with torch ops, as the reference's modules state them (src/aux/loss:
                              distill_ce.py, symm_ce_loss.py, kl_loss.py, symm_kl_loss.py, jsdloss.py, hellinger.py)
  closed_form(kind, x, t)     the table of include/mhaq_fq.h -- loss and d loss / d x -- as a torch function of any dtype
  autograd64(kind, x, t, g)   float64 autograd through torch_loss on the CPU: the yardstick
  within_bar(...)             the accuracy bar of the GPU tests

No kernel is involved in any of them."""
import math

import torch
import torch.nn.functional as F

CE, SCE, KL, SKL, JSD, HELLINGER = range(6)
KINDS = [CE, SCE, KL, SKL, JSD, HELLINGER]
NAMES = {CE: "Cross-Entropy", SCE: "Symmetrical Cross-Entropy", KL: "KL", SKL: "Symmetrical KL", JSD: "JSD",
         HELLINGER: "Hellinger"}
ZERO_AT_EQUAL = [KL, SKL, JSD, HELLINGER]         # loss and gradient vanish where target == input

# the shapes of the GPU tests: register path (1001: unaligned row bases), its edge at 4096 / 4097, a re-walked row; more row
# partials than the finalize has threads (257: one of them, 600: a third trip); 1028 and 4092 columns: the first 4-element group
# of a thread's second trip over the row and the last group of its fourth
SHAPES = [(3, 1), (1, 2), (5, 37), (16, 1001), (250, 1000), (2, 4096), (4, 4097), (2, 10007), (257, 4), (600, 3), (3, 1028),
          (2, 4092)]
CPU_SHAPES = [(1, 2), (5, 37), (16, 1001)]
MARGIN = 4.0                                     # the issue's factor on the framework chain's own error


def torch_loss(kind, x, t):
    """The reference module's forward, statement for statement (input = the student's logits, target = the teacher's)."""
    if kind == CE:
        return F.cross_entropy(x, t.softmax(-1))
    if kind == SCE:
        return -(torch.sum(F.softmax(t, dim=1) * F.log_softmax(x, dim=1), dim=1).mean()
                 + torch.sum(F.softmax(x, dim=1) * F.log_softmax(t, dim=1), dim=1).mean())
    if kind == KL:
        return F.kl_div(F.log_softmax(x, dim=1), F.log_softmax(t, dim=1), log_target=True)
    if kind == SKL:
        a, b = F.log_softmax(x, dim=1), F.log_softmax(t, dim=1)
        return (F.kl_div(a, b, log_target=True, reduction="batchmean")
                + F.kl_div(b, a, log_target=True, reduction="batchmean"))
    if kind == JSD:
        p, q = x.log_softmax(-1), t.log_softmax(-1)
        m = 0.5 * (p + q)
        return F.kl_div(m, p, log_target=True) + F.kl_div(m, q, log_target=True)
    if kind == HELLINGER:
        return F.mse_loss(x.softmax(-1).sqrt(), t.softmax(-1).sqrt())
    raise NotImplementedError(kind)


def closed_form(kind, x, t):
    """-> (loss, gunit): the table's term sum / denom and r / denom, in the dtype of x and t (sums in that dtype too)."""
    rows, cols = x.shape
    n = rows * cols
    ls, lt = F.log_softmax(x, dim=1), F.log_softmax(t, dim=1)
    ps, pt = F.softmax(x, dim=1), F.softmax(t, dim=1)
    d = ls - lt
    if kind == CE:
        term, denom, r = -pt * ls, rows, ps - pt
    elif kind == SCE:
        m = (ps * lt).sum(1, keepdim=True)
        term, denom, r = -pt * ls - ps * lt, rows, ps - pt - ps * (lt - m)
    elif kind == KL:
        term, denom, r = pt * (lt - ls), n, ps - pt
    elif kind in (SKL, JSD):
        k = (ps * d).sum(1, keepdim=True)
        term, denom, r = (ps - pt) * d, (rows if kind == SKL else 2 * n), ps - pt + ps * (d - k)
    elif kind == HELLINGER:
        h = ps - (ps * pt).sqrt()
        term, denom, r = (ps.sqrt() - pt.sqrt()) ** 2, n, h - ps * h.sum(1, keepdim=True)
    else:
        raise NotImplementedError(kind)
    return term.sum() / denom, r / denom


def autograd64(kind, x, t, g=1.0):
    """float64 CPU autograd through the torch statement from the bits of x and t -> (loss, g * d loss / d x)."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    loss = torch_loss(kind, x64, t.detach().double().cpu())
    (gx,) = torch.autograd.grad(loss * g, x64)
    return loss.detach(), gx


def chain32(kind, x, t, g=1.0):
    """The framework's float32 chain where x lives (the GPU tests run it on the device) -> (loss, gx)."""
    xf = x.detach().float().requires_grad_(True)
    loss = torch_loss(kind, xf, t.detach().float())
    (gx,) = torch.autograd.grad(loss * g, xf)
    return loss.detach(), gx


def ulp32(v):
    v = abs(float(v))
    if v == 0.0 or not math.isfinite(v):
        return 2.0 ** -149
    return max(2.0 ** (math.floor(math.log2(v)) - 23), 2.0 ** -149)


def loss_bar(l_torch, l64, margin=MARGIN):
    return margin * abs(float(l_torch) - float(l64)) + 8 * ulp32(l64)


def grad_bar(g_torch, g64, margin=MARGIN):
    g64 = g64.double().cpu()
    return margin * float((g_torch.double().cpu() - g64).abs().max()) + 8 * 2.0 ** -24 * float(g64.abs().max())


def within_bar(loss, gx, chain, ref, margin=MARGIN):
    """-> (ok, figures): |L - L64| <= margin |L_torch - L64| + 8 ulp32(L64) and
    max|gx - g64| <= margin max|g_torch - g64| + 8 2^-24 max|g64|."""
    (l_t, g_t), (l64, g64) = chain, ref
    el = abs(float(loss) - float(l64))
    eg = float((gx.double().cpu() - g64.double().cpu()).abs().max())
    bl, bg = loss_bar(l_t, l64, margin), grad_bar(g_t, g64, margin)
    fig = dict(loss_err=el, loss_bar=bl, loss_err_torch=abs(float(l_t) - float(l64)), grad_err=eg, grad_bar=bg,
               grad_err_torch=float((g_t.double().cpu() - g64.double().cpu()).abs().max()))
    return (el <= bl and eg <= bg), fig


def logits(shape, scale, seed, noise=0.5, device="cpu"):
    """Seeded normal logits of the given scale and a teacher x + noise, float32."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen) * scale
    t = x + noise * scale * torch.randn(shape, generator=gen)
    return x.to(device), t.to(device)
