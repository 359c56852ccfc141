"""The arithmetic contract of mhaq_fq_bn_fwd (include/mhaq_fq.h) restated in torch, on any device (test infrastructure).

closed_form() is the yardstick, an fp64 evaluation (never the code under test) on the [M, C] view of x:

    mean = sum x / M,   var = sum (x - mean)^2 / M,   invstd = (var + eps)^-1/2,   y = (x - mean) * invstd * gamma + beta
    running_mean' = (1 - f) running_mean + f mean,     running_var' = (1 - f) running_var + f var M / (M - 1)

simulate() evaluates the contract itself in torch -- shifted fp64 sums, every statistic rounded to fp32 once, y in fp32 in the
stated order -- and, on request, one of the variants the contract rules out.  The checkers:

  check_y       |y - y64| <= 1e-6 * T,  T = (|x| + |mean64|) * invstd64 * |gamma| + |beta|  (the project's 1e-6 * sum|terms|; one
                rounding each of mean, invstd, a, the difference, the product and the sum is <= ~4.2e-7 T).  A channel that holds
                a NaN or an infinity is NaN in every element.
  check_stat    save_mean / save_invstd within one fp32 ulp of the fp32 rounding of the fp64 value (non-finite channels: not finite).
                For the mean also BY VALUE: where mean64 lies farther than 2^-30 * max|x| from the nearest midpoint between
                adjacent fp32 values, the result IS the nearest fp32 -- two fixed-order fp64 sums of M <= 2^21 terms differ by at
                most 2^-53 * M * 2 max|x| <= 2^-31 max|x|, so a correctly rounded mean cannot sit on the other side of a midpoint
                that far away; a truncated one sits there in half the channels.
  check_running within 1e-6 * ((1 - f) |old| + f |new term|).
"""
import torch

REL = 1e-6


def rows(t):
    """[N, C, H, W] channels_last -> the [M, C] view the kernels walk."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def closed_form(X, gamma, beta, eps, rm=None, rv=None, f=0.1, want_y=True):
    """X: [M, C].  gamma / beta None = 1 / 0.  Returns fp64 tensors."""
    X = X.double()
    m, c = X.shape
    ga = torch.ones(c, dtype=torch.float64, device=X.device) if gamma is None else gamma.double()
    be = torch.zeros(c, dtype=torch.float64, device=X.device) if beta is None else beta.double()
    mean = X.sum(0) / m
    var = (X - mean).square().sum(0) / m
    invstd = (var + eps) ** -0.5
    out = dict(mean=mean, var=var, invstd=invstd, xmax=X.abs().amax(0), bad=~torch.isfinite(X).all(0))
    if want_y:
        out["y"] = (X - mean) * invstd * ga + be
        out["T"] = (X.abs() + mean.abs()) * invstd * ga.abs() + be.abs()
    if rm is not None:
        unb = var * m / (m - 1)
        out["rm"], out["rm_abs"] = (1 - f) * rm.double() + f * mean, (1 - f) * rm.double().abs() + f * mean.abs()
        out["rv"], out["rv_abs"] = (1 - f) * rv.double() + f * unb, (1 - f) * rv.double().abs() + f * unb.abs()
    return out


def _trunc32(v64):
    """fp64 -> fp32 toward zero: the rounding the contract rules out."""
    r = v64.float()
    over = r.double().abs() > v64.abs()
    return torch.where(over, torch.nextafter(r, torch.zeros_like(r)), r)


def simulate(X, gamma, beta, eps, rm=None, rv=None, f=0.1, variant=None):
    """The contract in torch.  Returns dict(y, mean, invstd, rm, rv) in fp32.  variant: None, "unshifted_fp32" (statistics as
    fp32 E[x^2] - E[x]^2), "no_beta", "truncated_mean", "biased_running_var"."""
    X = X.float()
    m = X.shape[0]
    ga = torch.ones(X.shape[1]) if gamma is None else gamma.float()
    be = torch.zeros(X.shape[1]) if beta is None else beta.float()
    if variant == "unshifted_fp32":
        e1 = X.mean(0)
        var64 = ((X * X).mean(0) - e1 * e1).clamp_min(0).double()
        mean64 = e1.double()
    else:
        k = X[0].double()
        d = X.double() - k
        e1, e2 = d.sum(0) / m, (d * d).sum(0) / m
        var64 = e2 - e1 * e1
        var64 = torch.where(var64 < 0, torch.zeros_like(var64), var64)
        mean64 = k + e1
    mean = _trunc32(mean64) if variant == "truncated_mean" else mean64.float()
    invstd = ((var64 + eps) ** -0.5).float()
    a = ga * invstd
    y = (X - mean) * a
    if variant != "no_beta":
        y = y + be
    out = dict(y=y, mean=mean, invstd=invstd)
    if rm is not None:
        unb = var64 if variant == "biased_running_var" else var64 * m / (m - 1)
        out["rm"] = ((1 - f) * rm.double() + f * mean64).float()
        out["rv"] = ((1 - f) * rv.double() + f * unb).float()
    return out


def check_y(got, cf):
    """Asserts the elementwise bound; returns the largest error in units of T."""
    g, ref, T, bad = got.double(), cf["y"], cf["T"], cf["bad"]
    assert g.shape == ref.shape
    assert bool(torch.isnan(g[:, bad]).all()), "a channel with a non-finite x is not NaN everywhere"
    g, ref, T = g[:, ~bad], ref[:, ~bad], T[:, ~bad]
    assert bool(torch.isfinite(g).all()), "a non-finite y in a finite channel"
    err = (g - ref).abs()
    worst = float((err / T.clamp_min(1e-300)).max()) if err.numel() else 0.0
    over = err > REL * T
    assert not bool(over.any()), f"{int(over.sum())} of {err.numel()} elements off the bound; worst {worst:.3e} T"
    return worst


def check_stat(got, ref64, bad, what, xmax=None):
    """One fp32 ulp around R32(ref64); with xmax (the mean) also the by-value rule of the module docstring.  Returns the largest
    relative error against the fp64 value."""
    assert got.dtype == torch.float32 and got.shape == ref64.shape
    assert not bool(torch.isfinite(got[bad]).any()), f"{what}: finite in a channel with a non-finite x"
    g, r64 = got[~bad], ref64[~bad]
    r32 = r64.float()
    lo, hi = torch.nextafter(r32, torch.full_like(r32, -torch.inf)), torch.nextafter(r32, torch.full_like(r32, torch.inf))
    assert bool(((g >= lo) & (g <= hi)).all()), f"{what}: more than one ulp from the rounded fp64 value"
    if xmax is not None:
        mid_lo, mid_hi = (lo.double() + r32.double()) / 2, (hi.double() + r32.double()) / 2
        dist = torch.minimum((r64 - mid_lo).abs(), (r64 - mid_hi).abs())
        cmp = dist > 2.0 ** -30 * xmax[~bad]
        assert bool((g[cmp] == r32[cmp]).all()), f"{what}: {int((g[cmp] != r32[cmp]).sum())} of {int(cmp.sum())} not the nearest fp32"
    nz = r64 != 0
    return float(((g.double() - r64).abs()[nz] / r64.abs()[nz]).max()) if bool(nz.any()) else 0.0


def check_running(got, ref64, ref_abs, bad, what):
    assert not bool(torch.isfinite(got[bad]).any()), f"{what}: finite in a channel with a non-finite x"
    err = (got.double() - ref64).abs()[~bad]
    tol = REL * ref_abs[~bad]
    assert bool((err <= tol).all()), (what, float((err / ref_abs[~bad].clamp_min(1e-300)).max()))
    return float((err / ref_abs[~bad].clamp_min(1e-300)).max()) if err.numel() else 0.0


def check_all(got, cf, f_given=True):
    """got: dict(y, mean, invstd[, rm, rv]) with y as [M, C] (or None); cf: closed_form() of the same inputs."""
    fig = {}
    if got.get("y") is not None:
        fig["y"] = check_y(got["y"], cf)
    fig["mean"] = check_stat(got["mean"], cf["mean"], cf["bad"], "save_mean", cf["xmax"])
    fig["invstd"] = check_stat(got["invstd"], cf["invstd"], cf["bad"], "save_invstd")
    if got.get("rm") is not None:
        fig["rm"] = check_running(got["rm"], cf["rm"], cf["rm_abs"], cf["bad"], "running_mean")
        fig["rv"] = check_running(got["rv"], cf["rv"], cf["rv_abs"], cf["bad"], "running_var")
    return fig


def planted(kind, m, c, seed=0):
    """[M, C] float32 inputs (x, gamma, beta) on the CPU: the planted cases of the contract."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, c, generator=g) * (0.5 + torch.rand(c, generator=g) * 3) + torch.randn(c, generator=g) * 2
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    if kind == "far_mean":
        sign = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0)
        x = sign * 1e4 + torch.randn(m, c, generator=g)
    elif kind == "constant_channel":
        x[:, 1] = 3.0
        x[:, c - 1] = 0.0
    elif kind == "outlier":
        x[0, :] = 1e4
    elif kind == "tiny_sigma":
        x = 100 + 1e-3 * torch.randn(m, c, generator=g)
    elif kind == "gamma_sign":
        gamma[0], gamma[1], gamma[2] = 0.0, -1.5, -0.0
    else:
        assert kind == "plain", kind
    return x, gamma, beta
