"""The arithmetic contract of mhaq_fq_bn_fwd_x16 (include/mhaq_fq.h) restated in torch, on any device (test infrastructure).
up = the exact conversion to float32, R16 = round to nearest-even to the 16-bit dtype.  The contract is mhaq_fq_bn_fwd's on
up(x) -- shifted fp64 sums, float32 statistics rounded once -- with ONE more rounding at the end:

    y = R16((up(x) - mean) * (gamma * invstd) + beta)                                  (fp32, in this order)

The yardstick is bn_fwd_contract.closed_form on rows(x).float(): the fp64 textbook formulas on the exactly upcast input, never
the code under test.  The statistics are fp32 quantities of an exact input: bn_fwd_contract.check_stat / check_running,
unchanged.  y is held to it by bn_bwd16_contract.check_dx16(got, y64, T, dtype):

  bound      |y - y64| <= 1e-6 * T + spacing16(y) / 2,   T = (|x| + |mean64|) * invstd64 * |gamma| + |beta|
  rounding   wherever y64 lies farther than 1e-6 * T from a midpoint between adjacent 16-bit values, y IS its nearest-even
             rounding.  The share of elements nearer than that is capped (EXCLUDED_CAP: 1 % bf16, 4 % fp16) on the ordinary
             inputs with M >= CAP_MIN_ROWS -- a condition on the case, not a measurement (a torch evaluation of the contract
             excludes <= 0.39 % / 2.7 % on them).  NOT capped: constant channels (T ~ |x| / sqrt(eps) puts every element of
             theirs out of the rule; y == R16(beta) bit for bit is asserted instead), tiny_sigma and far_mean (one or two 16-bit
             values per channel: kept for the statistics), and `spread` (below).

planted(): bn_fwd_contract.planted cast to the dtype, plus "spread": 1000 * randn(C) + 64 * randn(M, C), a far mean whose
channels still spread after the rounding to 16 bits (adjacent bf16 values at 1000 are 4 apart) -- the case that tells the
shifted sums from fp32 E[x^2] - E[x]^2.
"""
import torch

from tests import bn_bwd16_contract as B
from tests import bn_fwd_contract as F

EXCLUDED_CAP = B.EXCLUDED_CAP
CAP_MIN_ROWS = 75
CAPPED_KINDS = ("plain", "outlier", "gamma_sign")
rows = F.rows


def capped(kind, m):
    """Whether the excluded-share cap is a condition of this case."""
    return kind in CAPPED_KINDS and m >= CAP_MIN_ROWS


def planted(kind, m, c, dtype, seed=0):
    """[M, C] inputs on the CPU: x in `dtype`, gamma and beta float32."""
    if kind == "spread":
        g = torch.Generator().manual_seed(seed)
        x = 1000 * torch.randn(c, generator=g) + 64 * torch.randn(m, c, generator=g)
        gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    else:
        x, gamma, beta = F.planted(kind, m, c, seed)
    return x.to(dtype), gamma, beta


def closed_form(X16, gamma, beta, eps, rm=None, rv=None, f=0.1, want_y=True):
    """X16: [M, C] in a 16-bit dtype.  bn_fwd_contract.closed_form on its exact upcast."""
    assert X16.dtype in B.MANTISSA_BITS
    return F.closed_form(X16.float(), gamma, beta, eps, rm, rv, f, want_y)


def simulate(X16, gamma, beta, eps, rm=None, rv=None, f=0.1, variant=None):
    """The contract in torch (CPU).  Returns dict(y [16-bit], mean, invstd, rm, rv).  variant: None, "truncated_y" (y cut off
    instead of rounded to nearest-even) or one of bn_fwd_contract.simulate's ("no_beta", "truncated_mean", "unshifted_fp32",
    "biased_running_var")."""
    sim = F.simulate(X16.float(), gamma, beta, eps, rm, rv, f, variant=None if variant == "truncated_y" else variant)
    sim["y"] = B._truncate(sim["y"], X16.dtype) if variant == "truncated_y" else sim["y"].to(X16.dtype)
    return sim


def check_y16(got, cf, dtype, cap=True):
    """Bound and rounding rule on y ([M, C], 16-bit); a channel that holds a non-finite x is NaN everywhere (its y64 is)."""
    bad = cf["bad"]
    assert bool(torch.isnan(cf["y"][:, bad]).all())
    assert bool(torch.isnan(got[:, bad].float()).all()), "a channel with a non-finite x is not NaN everywhere"
    return B.check_dx16(got, cf["y"], cf["T"], dtype, cap=cap)


def check_all(got, cf, dtype, cap=True):
    """got: dict(y, mean, invstd[, rm, rv]) with y as [M, C] (or None); cf: closed_form() of the same inputs."""
    fig = {}
    if got.get("y") is not None:
        fy = check_y16(got["y"], cf, dtype, cap)
        fig["y"], fig["excluded"] = fy["err"], fy["excluded"]
    fig["mean"] = F.check_stat(got["mean"], cf["mean"], cf["bad"], "save_mean", cf["xmax"])
    fig["invstd"] = F.check_stat(got["invstd"], cf["invstd"], cf["bad"], "save_invstd")
    if got.get("rm") is not None:
        fig["rm"] = F.check_running(got["rm"], cf["rm"], cf["rm_abs"], cf["bad"], "running_mean")
        fig["rv"] = F.check_running(got["rv"], cf["rv"], cf["rv_abs"], cf["bad"], "running_var")
    return fig
