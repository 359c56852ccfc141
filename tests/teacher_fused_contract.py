"""The contract of the frozen forward (mhaq_fq_bn_infer_consts / _act / mhaq_fq_bn_relu_pool3s2, include/mhaq_fq.h) restated
in torch, on any device (test infrastructure).

The yardstick is the fp64 textbook formula, never the code under test:

    invstd = (running_var + eps)^-1/2        t = (x - running_mean) * invstd * gamma + beta
    BN_RELU  y = relu(t)      BN_ADD_RELU  y = relu(t + r)      BN2_ADD_RELU  y = relu(t + t2)      pool  p = max_pool2d(relu(t), 3, 2, 1)

  chain()       the SAME fp32 constants pushed through separate torch ops, torch.relu((x - mean) * a + beta [+ r or + t2]):
                torch rounds after every op, which is where the contract rounds, so the kernels' output equals it bit for bit
                (NaN positions included) and any difference is an indexing or geometry bug.
  check()       |y - y64| <= 1e-6 * T,  T = (|x| + |mean|) * invstd * |gamma| + |beta|  (+ |r|, or + the second branch's T):
                the training forward's bound (tests/bn_fwd_contract.py; six roundings of <= 2^-24 each stay below 4.2e-7 T, the
                add of the second stream adds one more).  ReLU and max are 1-Lipschitz, so the bound carries through them; for
                the pool T is the window's largest.  Where the fp64 value is not finite the result must be of the same kind.
  check_slab()  mean and beta are copies; a lies within one fp32 ulp of the fp32 rounding of the fp64 product.

Tensors are [..., C] with the channel last (the [M, C] view the kernels walk), or [N, C, H, W] for the pool.
"""
import torch
import torch.nn.functional as F

REL = 1e-6
BN_RELU, BN_ADD_RELU, BN2_ADD_RELU = 0, 1, 2


def consts64(rm, rv, gamma, beta, eps):
    """fp64 {mean, invstd, gamma, beta}; gamma / beta None = 1 / 0."""
    c = rm.numel()
    ga = torch.ones(c, dtype=torch.float64, device=rm.device) if gamma is None else gamma.double()
    be = torch.zeros(c, dtype=torch.float64, device=rm.device) if beta is None else beta.double()
    return rm.double(), (rv.double() + eps) ** -0.5, ga, be


def slab(rm, rv, gamma, beta, eps):
    """The [3, C] fp32 slab as the contract states it: a = gamma * invstd in fp64, rounded once."""
    mean, invstd, ga, be = consts64(rm, rv, gamma, beta, eps)
    return torch.stack([mean.float(), (ga * invstd).float(), be.float()])


def check_slab(got, rm, rv, gamma, beta, eps):
    want = slab(rm, rv, gamma, beta, eps)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]), "mean and beta are copies"
    a = want[1]
    lo, hi = torch.nextafter(a, torch.full_like(a, -torch.inf)), torch.nextafter(a, torch.full_like(a, torch.inf))
    assert bool(((got[1] >= lo) & (got[1] <= hi)).all()), "a: more than one ulp from the rounded fp64 product"
    return int((got[1] != a).sum())


def _t32(x, k):
    return (x - k[0]) * k[1] + k[2]


def chain(x, k, mode=BN_RELU, r=None, x2=None, k2=None):
    """Separate fp32 torch ops on channel-last tensors [..., C] with the slab(s) k [3, C]."""
    t = _t32(x, k)
    if mode == BN_ADD_RELU:
        t = t + r
    elif mode == BN2_ADD_RELU:
        t = t + _t32(x2, k2)
    return torch.relu(t)


def _nchw(k):
    return k.reshape(3, 1, -1, 1, 1)


def chain_pool(x, k):
    """The same for the stem, on [N, C, H, W]."""
    k = _nchw(k)
    return F.max_pool2d(torch.relu((x - k[0]) * k[1] + k[2]), 3, 2, 1)


def _t64(x, c64):
    mean, invstd, ga, be = c64
    x = x.double()
    return (x - mean) * invstd * ga + be, (x.abs() + mean.abs()) * invstd * ga.abs() + be.abs()


def ref64(x, c64, mode=BN_RELU, r=None, x2=None, c64_2=None):
    """(y64, T) on channel-last tensors; c64 = consts64(...)."""
    t, T = _t64(x, c64)
    if mode == BN_ADD_RELU:
        t, T = t + r.double(), T + r.double().abs()
    elif mode == BN2_ADD_RELU:
        t2, T2 = _t64(x2, c64_2)
        t, T = t + t2, T + T2
    return torch.relu(t), T


def ref64_pool(x, c64):
    """(p64, T) on [N, C, H, W]: T is the window's largest."""
    mean, invstd, ga, be = (v.reshape(1, -1, 1, 1) for v in c64)
    x = x.double()
    t = (x - mean) * invstd * ga + be
    T = (x.abs() + mean.abs()) * invstd * ga.abs() + be.abs()
    T = torch.where(torch.isnan(T), torch.full_like(T, torch.inf), T)      # (max_pool2d would spread a NaN bound: no bound there)
    return F.max_pool2d(torch.relu(t), 3, 2, 1), F.max_pool2d(T, 3, 2, 1)


def check(y, y64, T):
    """Asserts the bound; returns the largest error in units of T over the finite elements."""
    assert y.dtype == torch.float32 and y.shape == y64.shape
    g = y.double()
    fin = torch.isfinite(y64)
    same_kind = torch.where(torch.isnan(y64), torch.isnan(g), g == y64)
    assert bool(same_kind[~fin].all()), "a non-finite fp64 value is not met in kind"
    assert not bool(torch.isnan(g[fin]).any()), "NaN where the fp64 value is finite"
    bounded = fin & torch.isfinite(T)
    err, tol = (g - y64).abs()[bounded], T[bounded]
    over = err > REL * tol
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert not bool(over.any()), f"{int(over.sum())} of {err.numel()} elements off the bound; worst {worst:.3e} T"
    return worst


def planted(kind, m, c, seed=0, device="cpu"):
    """(x [M, C], rm, rv, gamma, beta, eps) in fp32: the planted cases of the contract."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, c, generator=g) * (0.5 + torch.rand(c, generator=g) * 3) + torch.randn(c, generator=g) * 2
    rm, rv = torch.randn(c, generator=g) * 2, torch.rand(c, generator=g) * 4 + 0.25
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    eps = 1e-5
    if kind == "far_mean":
        sign = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0)
        x = sign * 1e4 + torch.randn(m, c, generator=g)
        rm = sign * 1e4 + torch.randn(c, generator=g) * 0.1
    elif kind in ("zero_var_eps1e-5", "zero_var_eps1e-3"):
        rv = torch.zeros(c)
        eps = 1e-5 if kind.endswith("1e-5") else 1e-3
    elif kind == "gamma_zero":
        gamma[0::2] = 0.0
        gamma[1] = -0.0
    elif kind == "gamma_negative":
        gamma = -gamma.abs() - 0.1
    else:
        assert kind == "plain", kind
    return tuple(t.to(device) if isinstance(t, torch.Tensor) else t for t in (x, rm, rv, gamma, beta, eps))
