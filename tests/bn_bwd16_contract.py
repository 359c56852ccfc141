"""The arithmetic contract of mhaq_fq_bn_bwd_x16 (include/mhaq_fq.h) restated in torch, on any device (test
infrastructure).  up = the exact conversion to float32, R16 = round to nearest-even to the 16-bit dtype:

    dbeta = sum up(dy),   dgamma = invstd * sum up(dy) * (up(x) - mean)            (fp64 sums, rounded to fp32 once)
    dx = R16((gamma * invstd) * ((up(dy) - dbeta / M) - ((up(x) - mean) * invstd) * (dgamma / M)))        (fp32, this order)

closed_form() is the fp64 evaluation of tests/test_gpu_bn_backward.py from the SAVED fp32 mean and invstd, on x.double()
and dy.double() of the 16-bit tensors; simulate() evaluates the contract itself in fp32 torch operations (and, on request,
one of the variants the contract rules out); check_dx16() holds a 16-bit dx against the closed form:

  bound (every element)   |got - ref| <= 1e-6 * ref_abs + spacing16(got) / 2,
                          ref_abs = |gamma| * invstd * (|dy| + |dbeta| / M + |xhat| * |dgamma| / M);
                          1e-6 * ref_abs bounds the fp32 value before rounding, the second term is the one rounding;
                          spacing16(got) = the larger of the two gaps from got to its 16-bit neighbours.
                          ref_abs == 0: got is exactly zero.  A non-finite ref is matched in kind; an fp16 got may be +-inf
                          where a finite |ref| >= 65504 - spacing16(65504) / 2.
  rounding (by value)     where ref lies farther than 1e-6 * ref_abs from the nearest midpoint between adjacent 16-bit values,
                          got IS the round-to-nearest-even 16-bit value of ref: the value before rounding cannot lie on the
                          other side of a midpoint that far away.  Elements nearer than that are excluded; their share is
                          capped (EXCLUDED_CAP) on every case with M >= 9 -- a condition on the case, not a measurement.
"""
import torch

MANTISSA_BITS = {torch.bfloat16: 7, torch.float16: 10}
MIN_EXPONENT = {torch.bfloat16: -126, torch.float16: -14}
EXCLUDED_CAP = {torch.bfloat16: 0.01, torch.float16: 0.04}
REL = 1e-6


def rows(t):
    """[N, C, H, W] channels_last -> the [M, C] view the kernels walk."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def closed_form(x, dy, gamma, mean, invstd):
    X, G = rows(x).double(), rows(dy).double()
    mu, iv, ga = mean.double(), invstd.double(), gamma.double()
    m = X.shape[0]
    d = X - mu
    db, db_abs = G.sum(0), G.abs().sum(0)
    dg, dg_abs = iv * (G * d).sum(0), iv * (G * d).abs().sum(0)
    xh = d * iv
    dx = ga * iv * (G - db / m - xh * dg / m)
    dx_abs = ga.abs() * iv * (G.abs() + db.abs() / m + xh.abs() * dg.abs() / m)
    return dict(dx=dx, dx_abs=dx_abs, dg=dg, dg_abs=dg_abs, db=db, db_abs=db_abs)


def _truncate(v32, dtype):
    """fp32 -> 16 bits by dropping the low mantissa bits (round toward zero): the rounding the contract rules out."""
    if dtype == torch.bfloat16:
        return (v32.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(dtype)
    r = v32.to(dtype)
    over = r.float().abs() > v32.abs()                       # rounded away from zero: step one value back
    bits = r.view(torch.int16)
    return torch.where(over & torch.isfinite(v32), bits - 1, bits).view(dtype)


def simulate(x, dy, gamma, mean, invstd, variant=None):
    """The contract in torch: fp64 sums, fp32 dx in the stated order, one rounding.  Returns (dx16 [M, C], dgamma, dbeta).
    variant: None, "truncate" (dx cut off instead of rounded to nearest-even), "no_dbias" (the dbeta / M term dropped),
    "folded_mean" (mean folded into an additive constant: xhat * dgamma / M as x * b - mean * b)."""
    dt = x.dtype
    X, G = rows(x).float(), rows(dy).float()
    m = X.shape[0]
    db64 = G.double().sum(0)
    dw64 = invstd.double() * (G.double() * (X.double() - mean.double())).sum(0)
    k2 = gamma.float() * invstd
    k3, k4 = (db64 / m).float(), (dw64 / m).float()
    if variant == "no_dbias":
        k3 = torch.zeros_like(k3)
    if variant == "folded_mean":
        b = invstd * k4
        v = k2 * ((G - k3) - (X * b - mean * b))
    else:
        v = k2 * ((G - k3) - ((X - mean) * invstd) * k4)
    out = _truncate(v, dt) if variant == "truncate" else v.to(dt)
    return out, dw64.float(), db64.float()


def _gaps(a, dtype):
    """For a magnitude a (float64, a 16-bit value): the gaps to the next 16-bit value above and below."""
    mb, emin = MANTISSA_BITS[dtype], MIN_EXPONENT[dtype]
    frac, exp = torch.frexp(torch.where(a > 0, a, torch.ones_like(a)))        # a = frac * 2^exp, frac in [0.5, 1)
    e = torch.where(a > 0, exp - 1, torch.full_like(exp, emin)).clamp_min(emin)
    up = torch.exp2((e - mb).double())
    pow2 = (a > 0) & (frac == 0.5) & (e > emin)
    return up, torch.where(pow2, up / 2, up)


def spacing16(v16):
    """The larger of the two gaps from each (finite) 16-bit value to its neighbours, as float64."""
    return _gaps(v16.double().abs(), v16.dtype)[0]


def check_dx16(got, ref, ref_abs, dtype, cap=True):
    """Asserts the bound and the rounding rule of the module docstring; returns the figures it measured:
    err = the largest |got - ref| - spacing16(got) / 2 in units of ref_abs, excluded = the share left out of the rounding rule."""
    assert got.dtype == dtype and got.shape == ref.shape == ref_abs.shape
    g = got.double()
    zero = ref_abs == 0
    assert bool((g[zero] == 0).all()), "an element whose term sum is 0 is not exactly zero"
    nan = torch.isnan(ref)
    assert bool(torch.isnan(g[nan]).all()), "a NaN of the reference is not a NaN"
    inf = torch.isinf(ref)
    assert bool((g[inf] == ref[inf]).all()), "an infinity of the reference is not matched"
    fin = ~zero & ~nan & ~inf
    fmax = torch.finfo(dtype).max
    half_top = _gaps(torch.tensor(fmax, dtype=torch.float64), dtype)[0].item() / 2
    may_overflow = fin & (ref.abs() >= fmax - half_top) if dtype == torch.float16 else torch.zeros_like(fin)
    g_inf = torch.isinf(g)
    assert bool((g_inf[fin] <= may_overflow[fin]).all()), "an infinity where the reference is finite and in range"
    assert bool((torch.sign(g[fin & g_inf]) == torch.sign(ref[fin & g_inf])).all())
    assert not bool(torch.isnan(g[fin]).any()), "a NaN where the reference is finite"
    b = fin & ~g_inf
    tol = REL * ref_abs[b] + spacing16(got)[b] / 2
    err = (g[b] - ref[b]).abs()
    worst = float(((err - spacing16(got)[b] / 2) / ref_abs[b]).max()) if bool(b.any()) else 0.0
    bad = err > tol
    assert not bool(bad.any()), (f"{int(bad.sum())} of {int(b.sum())} elements off the bound; worst "
                                 f"{worst:.3e} of the term sum beyond the rounding")
    # the rounding rule
    r16 = ref.to(dtype)                                       # via float32: 2^-24 |ref| << 1e-6 ref_abs off a midpoint
    a = r16.double().abs()
    up, dn = _gaps(torch.where(torch.isfinite(a), a, torch.zeros_like(a)), dtype)
    t = ref.abs()
    dist = torch.minimum((t - (a + up / 2)).abs(), (t - (a - dn / 2)).abs())
    cmp = b & ~may_overflow & torch.isfinite(a) & (dist > REL * ref_abs)
    wrong = cmp & (g != r16.double())
    assert not bool(wrong.any()), f"{int(wrong.sum())} of {int(cmp.sum())} elements are not the nearest-even rounding"
    excluded = 1.0 - float(cmp.sum()) / int(fin.sum()) if bool(fin.any()) else 0.0
    if cap:
        assert excluded <= EXCLUDED_CAP[dtype], f"{excluded:.4f} of the elements lie too near a midpoint to be compared"
    return dict(err=worst, excluded=excluded)


def check_sums(got, ref, ref_abs, what):
    """dgamma / dbeta: within 1e-6 * sum |terms| of the closed form, exact where that sum is 0, non-finite in kind."""
    g = got.double()
    bad = ~torch.isfinite(ref)
    assert bool((torch.isnan(g[bad]) == torch.isnan(ref[bad])).all()) and bool((g[bad & ~torch.isnan(ref)] == ref[bad & ~torch.isnan(ref)]).all()), what
    ok = ~bad
    err = (g[ok] - ref[ok]).abs()
    assert bool((err <= REL * ref_abs[ok]).all()), (what, float((err / ref_abs[ok].clamp_min(1e-300)).max()))
    nz = ok & (ref_abs > 0)
    return float(((g[nz] - ref[nz]).abs() / ref_abs[nz]).max()) if bool(nz.any()) else 0.0
