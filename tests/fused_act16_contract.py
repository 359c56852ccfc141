"""The arithmetic contract of mhaq_fq_act_relu_*_x16 (include/mhaq_fq.h) restated in torch, on any device (test
infrastructure).  up = the exact conversion to float32, R = round to nearest-even to the 16-bit dtype (NaN stays NaN):

  forward    t = addend ? R(up(z) + up(addend)) : z;   a = relu(t) (NaN passes);   y = R(fwd32(up(a)))
  backward   a = relu(up(z));   gq = R(bwd32(a, up(g_y)));   gs = g_a ? R(up(gq) + up(g_a)) : gq
             gx = (up(z) <= 0) ? +0 : gs                    (a NaN z passes the gradient)

fwd32 / bwd32 are the quantizer's fp32 element functions (any callables on float32 tensors).  gs is rounded twice on
purpose -- the separate launches write a 16-bit gq and add the other consumer's 16-bit gradient with a 16-bit add --;
backward(..., single_rounding=True) is the variant the contract rules out, gs = R(bwd32(..) + up(g_a)).

plant_double_rounding() builds, from the fp32 gradient p of an element, the 16-bit g_a at which the two variants differ."""
import torch

MANTISSA_BITS = {torch.bfloat16: 7, torch.float16: 10}


def forward(z, addend, fwd32):
    dt = z.dtype
    t = (z.float() + addend.float()).to(dt) if addend is not None else z
    a = torch.where(t.float() <= 0, torch.zeros_like(t), t)
    return fwd32(a.float()).to(dt), a


def backward(z, g_y, g_a, bwd32, single_rounding=False):
    dt = z.dtype
    zf = z.float()
    a = torch.where(zf <= 0, torch.zeros_like(zf), zf)
    p = bwd32(a, g_y.float())
    if g_a is None:
        gs = p.to(dt)
    elif single_rounding:
        gs = (p + g_a.float()).to(dt)
    else:
        gs = (p.to(dt).float() + g_a.float()).to(dt)
    return torch.where(zf <= 0, torch.zeros_like(gs), gs)


def plant_double_rounding(p, dtype):
    """For each fp32 p: (g_a, ok).  Where ok, R(R(p) + g_a) != R(p + g_a): g_a is half a unit in the last place of
    q = R(p), signed so that q + g_a is an exact tie which rounds (to even) AWAY from where p + g_a rounds.  ok needs a
    finite, normal q != p."""
    m = MANTISSA_BITS[dtype]
    q = p.to(dtype)
    qf = q.float()
    tiny = torch.finfo(dtype).tiny
    ok = torch.isfinite(p) & torch.isfinite(qf) & (qf != p) & (qf.abs() >= 4 * tiny) & (qf.abs() < torch.finfo(dtype).max / 4)
    safe = torch.where(ok, qf.abs(), torch.ones_like(qf))
    half = torch.exp2(torch.floor(torch.log2(safe)) - (m + 1))
    odd = (q.view(torch.int16) & 1).bool()
    towards_p = torch.sign(p - qf)
    g_a = (torch.where(odd, -towards_p, towards_p) * half).to(dtype)
    differs = (qf + g_a.float()).to(dtype) != (p + g_a.float()).to(dtype)
    return g_a, ok & differs
