"""Inputs and the eager oracle for the ReLU / residual-add forms of the NoisyAct kernels (test infrastructure; CPU only).

build(n, pset, with_add, family, seed) gives z, addend, g_y, g_a as flat fp32 CPU tensors: randn everywhere, and at every
flat index i with (i + first) % stride < len(slots) the planted value of that slot.  The stride is odd, so the planted
values walk through every residue mod 4 and every lane: the head, the float4 body and the n % 4 tail all receive them.

  finite   +-0, lo, hi, lo / hi one ulp to each side, lo + (k + 1/2) s, negatives inside and outside [lo, hi], a value
           far above hi, +-1e-42, +-3e38, an inside value; with an addend: 0 + 0, (-0) + (-0), exact cancellation.
  special  the finite slots, then NaN / +-inf in z, inf + (-inf), NaN / +-inf / +-1e-42 / 3e38 in g_y and in g_a, NaN
           gradients under a masked element (z < 0), and a few special-with-special pairs.

Order of the special slots: a NaN g_y comes before the 3e38 g_y.  A lone 3e38 gradient overflows the reference's g * q
term (STE / LSQ: the kernels sum g * (q - v) instead, csrc/fq_pt.hip bwd_elem), which is a documented difference of the
REDUCED scale gradient, not what these cases are about; with the NaN in the sum both sides are NaN.  Sizes below the
stride start at the first special slot in the special family (`first`), so that the tiny sizes see special values too.

oracle(case, method, ...) is torch eager only: a = relu(z + addend), oracle.fq_eager.act_fake_quant(a, ..., r, method),
torch.autograd.backward([y, a], [g_y, g_a]); the signs r are tests/philox_ref.signs(n, seed, offset)."""
import functools
import math

import numpy as np
import torch

from oracle import fq_closed_form as CF
from oracle import fq_eager as O
from tests import philox_ref

SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 2047, 2048, 2049, 2052, 4099, 3 * 2048 + 1031)
METHODS = ("STE", "LSQ", "EWGS")
METHOD_VALUE = {"STE": 0, "EWGS": 1, "LSQ": 3}          # include/mhaq_fq.h

S_ALL_ONES_BITS = 0x3E7FFFFF                             # 0.24999998: fast_div false (tests/test_gpu_special_values.py)

# name -> (log_s, log_q, b, signed, s_bits): s_bits pins the scale's bits where no fp32 log_s reaches them through exp2
# (the backward entry points take the scale itself; the forward entry points, which take log_s, leave that set out)
PARAM_SETS = {
    "above_zero": (-3.0, 2.0, 0.25, True, None),         # zeros clip to lo
    "holds_zero": (-3.0, 2.0, -1.0, True, None),
    "nonpow2_a": (-4.37, 2.21, -2.3, True, None),
    "nonpow2_b": (-9.913, 0.087, -0.47, True, None),
    "unsigned": (-4.0, 2.5, 0.0, False, None),           # the network's post-ReLU quantizer: a == 0 sits on lo
    "all_ones": (-2.0, 2.0, -0.75, True, S_ALL_ONES_BITS),
    "inverted": (-2.0, -3.0, 0.5, True, None),           # log_q < log_s: hi < lo, every element clamps to hi
}
FORWARD_SETS = tuple(k for k, v in PARAM_SETS.items() if v[4] is None)

_f32 = np.float32


class Quantizer:
    """The fp32 scalars of one parameter set, computed with the oracle's own ops: s, qr, lo = b, hi = (b + qr) - s."""

    def __init__(self, name):
        self.name = name
        self.log_s, self.log_q, self.b, self.signed, self.s_bits = PARAM_SETS[name]
        ls, lq, b = (torch.tensor([v], dtype=torch.float32) for v in (self.log_s, self.log_q, self.b))
        self.s_t = torch.exp2(ls) if self.s_bits is None else torch.from_numpy(
            np.array([self.s_bits], dtype=np.uint32).view(np.float32).copy())
        self.qr_t = torch.exp2(lq)
        self.hi_t = b + self.qr_t - self.s_t
        self.s, self.qr, self.lo, self.hi = (float(t) for t in (self.s_t, self.qr_t, b, self.hi_t))

    def params(self):
        """{s, zp, lo, hi, qr}: what mhaq_fq_act_relu_fwd publishes and the backward entry points read."""
        return torch.tensor([self.s, self.lo, self.lo, self.hi, self.qr], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def quantizer(name):
    return Quantizer(name)


def _ulp(v, direction):
    return float(np.nextafter(_f32(v), _f32(direction)))


def _ties(q):
    """lo + (k + 1/2) s for four k, preferring those whose fp32 value divides back to exactly k + 1/2."""
    lo, s = _f32(q.lo), _f32(q.s)
    exact, other = [], []
    k0 = max(0, int(-q.lo / q.s)) if q.s > 0 else 0        # the first positive ones: ReLU zeroes the rest
    for k in range(k0, k0 + 96):
        t = _f32(lo + _f32(_f32(k + 0.5) * s))
        if not (0 < t < q.hi):
            continue
        (exact if _f32(_f32(t - lo) / s) == _f32(k + 0.5) else other).append(float(t))
    return (exact + other + [0.5, 0.5, 0.5, 0.5])[:4]


def inside_value(q):
    """A positive value strictly inside (lo, hi) and off the grid (0.3 for the inverted set, which has no inside)."""
    if q.lo < q.hi and q.hi > 0:
        return float(_f32(max(q.lo, 0.0) + 0.3 * (q.hi - max(q.lo, 0.0))))
    return 0.3


# a slot: (z, addend, g_y, g_a); None leaves the random value.  `addend` applies only with an addend.
def finite_slots(q):
    lo, hi = q.lo, q.hi
    neg_in = lo * 0.5 if lo < 0 else -0.375
    neg_out = min(lo, 0.0) - 1.3
    pin = inside_value(q)
    S = [(0.0, 0.0), (-0.0, -0.0), (lo, 0.0), (hi, 0.0),
         (_ulp(lo, -np.inf), 0.0), (_ulp(lo, np.inf), 0.0), (_ulp(hi, -np.inf), 0.0), (_ulp(hi, np.inf), 0.0)]
    S += [(t, 0.0) for t in _ties(q)]
    S += [(neg_in, 0.0), (neg_out, 0.0), (hi + 50.0, 0.0), (1e-42, 0.0), (-1e-42, 0.0), (3e38, 0.0), (-3e38, 0.0),
          (pin, "cancel"), (-0.0, 0.0), (pin, 0.0), (pin, None), (neg_in, None)]
    return [(z, a, None, None) for z, a in S]


def special_slots(q):
    nan, inf = float("nan"), float("inf")
    pin = inside_value(q)
    return [
        (nan, None, None, None), (inf, None, None, None), (-inf, None, None, None), (inf, -inf, None, None),
        (pin, 0.0, nan, None), (pin, 0.0, None, nan),
        (-0.5, 0.0, nan, None), (-0.5, 0.0, None, nan), (-0.5, 0.0, nan, nan),      # masked: the gradient is 0, not NaN
        (pin, 0.0, inf, None), (pin, 0.0, -inf, None), (pin, 0.0, None, inf), (pin, 0.0, None, -inf),
        (pin, 0.0, 1e-42, None), (pin, 0.0, -1e-42, None), (pin, 0.0, None, 1e-42), (pin, 0.0, None, -1e-42),
        (pin, 0.0, 3e38, None), (pin, 0.0, None, 3e38), (pin, 0.0, 3e38, 3e38),
        # special with special
        (nan, None, nan, None), (nan, None, None, inf), (nan, nan, inf, nan), (inf, None, inf, None),
        (-inf, None, inf, -inf), (1e-42, 0.0, 1e-42, -1e-42), (q.hi, 0.0, inf, None), (inf, -inf, nan, 1e-42),
        (0.0, 0.0, -inf, nan), (-3e38, -3e38, nan, inf),
    ]


FINITE_STRIDE, SPECIAL_STRIDE = 29, 61


class Case:
    pass


@functools.lru_cache(maxsize=None)
def build(n, pset, with_add, family, seed=0):
    """The inputs of one case (cached: treat them as read-only)."""
    assert family in ("finite", "special")
    q = quantizer(pset)
    gen = torch.Generator().manual_seed(1000 * seed + n)
    span = max(abs(q.lo), abs(q.hi), 1.0)
    z = torch.randn(n, generator=gen) * span
    addend = torch.randn(n, generator=gen) * (0.5 * span) if with_add else None
    gy = torch.randn(n, generator=gen)
    ga = torch.randn(n, generator=gen)
    fin = finite_slots(q)
    slots = fin + (special_slots(q) if family == "special" else [])
    stride = SPECIAL_STRIDE if family == "special" else FINITE_STRIDE
    assert len(slots) <= stride and stride % 2 == 1
    first = len(fin) if (family == "special" and n < stride) else 0
    slot = torch.full((n,), -1, dtype=torch.int64)          # which slot each element took (-1: random)
    for i in range(n):
        k = (i + first) % stride
        if k >= len(slots):
            continue
        slot[i] = k
        vz, va, vgy, vga = slots[k]
        if va == "cancel":
            z[i] = vz if not with_add else z[i]
            if with_add:
                addend[i] = -z[i]
        else:
            z[i] = vz
            if with_add and va is not None:
                addend[i] = va
        if vgy is not None:
            gy[i] = vgy
        if vga is not None:
            ga[i] = vga
    c = Case()
    c.n, c.pset, c.q, c.with_add, c.family = n, pset, q, with_add, family
    c.z, c.addend, c.gy, c.ga, c.slot = z, addend, gy, ga, slot
    return c


def signs(n, seed, offset):
    """+-0.5 fp32: the (seed, offset) sign stream as the oracle's r."""
    return torch.from_numpy(philox_ref.signs(n, seed, offset).astype(np.float32)) * 0.5


class _PinnedExp2(torch.autograd.Function):
    """exp2(log_s) with the result's bits given (the all-ones significand no fp32 log_s reaches); backward as exp2's."""

    @staticmethod
    def forward(ctx, log_s, s):
        ctx.save_for_backward(s)
        return s.clone()

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return g * s * math.log(2.0), None


def leaf_params(q):
    return [torch.tensor([v], dtype=torch.float32, requires_grad=True) for v in (q.log_s, q.log_q, q.b)]


def oracle(case, method, seed=0, offset=0, use_gy=True, use_ga=True):
    """The eager chain on the CPU.  dict: y, a, gx (= z.grad = addend.grad), grads = [d/dlog_s, d/dlog_q, d/db] as fp32
    one-element tensors (zeros when only a received a gradient), r (+-0.5)."""
    assert use_gy or use_ga
    q = case.q
    z = case.z.clone().requires_grad_(True)
    addend = case.addend.clone().requires_grad_(True) if case.with_add else None
    ls, lq, b = leaf_params(q)
    r = signs(case.n, seed, offset)
    a = torch.relu(z + addend if addend is not None else z)
    if q.s_bits is None:
        y, _ = O.act_fake_quant(a, ls, lq, b, r=r, method=method)
    else:                                   # act_fake_quant's two lines with the scale's bits pinned
        s, qr = _PinnedExp2.apply(ls, q.s_t), torch.exp2(lq)
        y = O.dequantize(O.quantize(a, s, b, b, b + qr - s, method, r), s, b)
    outs = ([y] if use_gy else []) + ([a] if use_ga else [])
    gs = ([case.gy] if use_gy else []) + ([case.ga] if use_ga else [])
    torch.autograd.backward(outs, gs)
    if addend is not None:
        same = (z.grad == addend.grad) | (torch.isnan(z.grad) & torch.isnan(addend.grad))
        assert bool(same.all())
    grads = [p.grad if p.grad is not None else torch.zeros(1) for p in (ls, lq, b)]
    return dict(y=y.detach(), a=a.detach(), gx=z.grad, grads=grads, r=r)


def yardsticks(case, a, r, method, use_gy=True):
    """The 1e-6 x sum|terms| bars of (d/dlog_s, d/dlog_q, d/db): tests/test_gpu_act16.yardsticks on (a, g_y)."""
    from tests.test_gpu_act16 import yardsticks as bars
    q = case.q
    ls = torch.log2(q.s_t)                   # (the pinned scale: its own logarithm, 1e-7 off the bar at most)
    gy = case.gy if use_gy else torch.zeros_like(case.gy)
    return bars(a, gy, r, ls, torch.tensor([q.log_q]), torch.tensor([q.b]), method)


def closed_form(case, a, r, method):
    q = case.q
    return CF.per_tensor(a, case.gy, r, q.s_t, q.lo, q.lo, q.hi_t, method)


def regions(case):
    """Which regions of the quantizer the case populates (on a = relu(z + addend))."""
    q = case.q
    a = torch.relu(case.z + case.addend if case.with_add else case.z)
    v = (torch.clamp(a, min=q.lo, max=q.hi) - q.lo) / q.s_t
    return dict(a_zero=bool((a == 0).any()), z_neg=bool((case.z < 0).any()), above_hi=bool((a > q.hi).any()),
                tie=bool(((v - torch.floor(v)) == 0.5).any()), bound=bool(((a == q.lo) | (a == q.hi)).any()),
                inside=bool(((a > max(q.lo, 0.0)) & (a < q.hi)).any()))
