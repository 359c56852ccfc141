"""The contract of the frozen forward on 16-bit tensors (mhaq_fq_bn_infer_act_x16 / mhaq_fq_bn_relu_pool3s2_x16,
include/mhaq_fq.h) restated in torch, on any device (test infrastructure).  Built on tests/teacher_fused_contract.py: the fp32
contract on the exactly upcast inputs, rounded once to nearest-even into the inputs' dtype.

  want() / want_pool()   torch's fp32 ops (K.chain / K.chain_pool on x.float()) and torch's cast: the expected value bit for
                         bit -- never the code under test.  same_values() compares values with NaN positions equal; NaN
                         payloads are not compared (torch's bf16 cast canonicalises a NaN, the hardware convert keeps a payload).
  check16()              |y - y64| <= u |y64| + (1 + u) 1e-6 T + s  against the fp64 formula on the upcast inputs (K.ref64 /
                         K.ref64_pool): the fp32 value lies within 1e-6 T of y64 by the fp32 contract, so its magnitude is at
                         most |y64| + 1e-6 T, and one rounding to nearest adds at most u times that; u = 2^-8 (bf16) or 2^-11
                         (fp16); s = 2^-25, half the spacing of fp16's subnormals, 0 for bf16 (whose exponent range is fp32's).
                         A non-finite y64 must be met in kind.
"""
import torch

from tests import teacher_fused_contract as K

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
S = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]


def _f(t):
    return None if t is None else t.float()


def want(x, k, mode=K.BN_RELU, r=None, x2=None, k2=None):
    """The expected bits on channel-last 16-bit tensors [..., C] with the fp32 slab(s) k [3, C]."""
    return K.chain(x.float(), k, mode, r=_f(r), x2=_f(x2), k2=k2).to(x.dtype)


def want_pool(x, k):
    """The same for the stem, on a 16-bit [N, C, H, W]."""
    return K.chain_pool(x.float(), k).to(x.dtype)


def rounded_twice(x, k, r):
    """BN_ADD_RELU with t rounded to 16 bits before the add, R16(relu(R16(t) + r)): what the contract excludes."""
    t = K._t32(x.float(), k).to(x.dtype).float()
    return torch.relu(t + r.float()).to(x.dtype)


def same_values(got, exp):
    """Asserts equal dtype, shape and values, NaN where and only where the expected value is NaN."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    gn, en = torch.isnan(got), torch.isnan(exp)
    assert torch.equal(gn, en), f"NaN positions differ in {int((gn != en).sum())} elements"
    zero = torch.zeros((), dtype=got.dtype, device=got.device)
    a, b = torch.where(gn, zero, got), torch.where(en, zero, exp)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ from the fp32 chain rounded once"


def check16(y, y64, T):
    """Asserts the bound; returns the largest error in units of the bound over the finite elements."""
    u, s = U[y.dtype], S[y.dtype]
    assert y.shape == y64.shape
    g = y.double()
    fin = torch.isfinite(y64)
    same_kind = torch.where(torch.isnan(y64), torch.isnan(g), g == y64)
    assert bool(same_kind[~fin].all()), "a non-finite fp64 value is not met in kind"
    assert not bool(torch.isnan(g[fin]).any()), "NaN where the fp64 value is finite"
    bounded = fin & torch.isfinite(T)
    err = (g - y64).abs()[bounded]
    tol = u * y64.abs()[bounded] + (1 + u) * K.REL * T[bounded] + s
    over = err > tol
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert not bool(over.any()), f"{int(over.sum())} of {err.numel()} elements off the bound; worst {worst:.3f} of it"
    return worst
