"""Shared by tests/test_fused_radam_cpu.py and tests/test_gpu_fused_radam_edges.py (no GPU needed to import or run):

1. radam_ref: RAdam in float64 written from the algorithm (Liu et al., "On the Variance of the Adaptive Learning Rate and
   Beyond", algorithm 2, with the eps and the bias-corrected second moment of torch.optim.RAdam's docstring) -- NOT from
   torch's foreach op chain and not from csrc/optim.hip.  When a bit comparison against the framework fails, this says which
   side moved.
2. oracle_errors / within_twice: the yardstick that holds an fp32 result to that oracle: its error may be at most twice the
   error of torch's own fp32 foreach result plus one fp32 ulp of the reference value.
3. Slab / banded_streams / plant_state: every one of p, grad, exp_avg and exp_avg_sq as a view into its own
   [band | tensor | band] slab, each stream's start element chosen modulo 4 on its own, the bands filled with a sentinel, and
   the optimizer state planted on those views (torch's _init_group leaves a non-empty state alone).
4. The case lists of the two test files: betas, eps, sizes, alignments, learning rates, planted gradient values.
"""
import math

import torch

CHUNK = 4096                                                       # mhaq_fq_radam_chunk_elements()
LRS = [3e-3, 1e-3, 0.0, 3e-3, 2e-3, 3e-3, 0.0, 4e-3, 1e-4]         # a schedule moves the rate between steps, 0 included
SPECIALS = [0.0, -0.0, 1e-41, float("inf"), float("-inf"), float("nan"), 1e-12, 1e6]

# 1 - beta1 as a float decides lerp's branch: < 0.5 takes m + w (g - m), anything else g - (g - m)(1 - w).
#   0.5, 0.5 + 1e-10 (float(1 - beta1) == 0.5f although 1 - beta1 < 0.5 in double), 0.3, 0.0 -> second branch
#   0.5 - 1e-10 (float(1 - beta1) == 0.5f as well), 0.6 (w = 0.4)                          -> see lerp_branch()
# beta2 in {0.999, 0.99, 0.9}: rho_t > 5 from step 6 on; beta2 in {0.5, 0.0}: rho_inf <= 3, never rectified.
BETAS = [(0.5, 0.999), (0.5 + 1e-10, 0.999), (0.5 - 1e-10, 0.999), (0.3, 0.99), (0.0, 0.9), (0.95, 0.5), (0.6, 0.0)]
EPSS = [1e-8, 1e-3, 0.0]
DEFAULT_BETAS = (0.9, 0.999)


def lerp_branch(beta1):
    """1 or 2: the branch of radam_element's lerp that float(1 - beta1) takes."""
    w1 = torch.tensor(1.0 - beta1, dtype=torch.float64).to(torch.float32).item()
    return 1 if abs(w1) < 0.5 else 2


def first_rectified_step(beta2, upto=64):
    """The first step count with rho_t > 5, or None when there is none up to `upto`."""
    for t in range(1, upto + 1):
        if _rho(beta2, t)[1] > 5:
            return t
    return None


def case_id(betas, eps=None):
    b1, b2 = betas
    s = f"b1={b1!r}-lerp{lerp_branch(b1)}-b2={b2!r}-" + ("rect6" if first_rectified_step(b2) == 6 else "never_rect")
    return s if eps is None else s + f"-eps={eps!r}"


# ---------------------------------------------------------------------------------------------- the float64 oracle
def _rho(beta2, t):
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    b2t = beta2 ** t
    return rho_inf, rho_inf - 2.0 * t * b2t / (1.0 - b2t)


def radam_ref(ps, gs, ms, vs, steps, lr, beta1, beta2, eps):
    """One RAdam step in place on lists of float64 tensors; steps[i] is tensor i's step count t AFTER this step.
        m = beta1 m + (1 - beta1) g          v = beta2 v + (1 - beta2) g^2          m_hat = m / (1 - beta1^t)
        rho_inf = 2 / (1 - beta2) - 1        rho_t = rho_inf - 2 t beta2^t / (1 - beta2^t)
        rho_t > 5:   l = sqrt(1 - beta2^t) / (sqrt(v) + eps)
                     r = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
                     p -= lr m_hat r l
        otherwise:   p -= lr m_hat"""
    for p, g, m, v, t in zip(ps, gs, ms, vs, steps):
        assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float64
        t = int(t)
        m.mul_(beta1).add_(g * (1.0 - beta1))
        v.mul_(beta2).add_(g * g * (1.0 - beta2))
        m_hat = m / (1.0 - beta1 ** t)
        rho_inf, rho_t = _rho(beta2, t)
        if rho_t > 5:
            l = math.sqrt(1.0 - beta2 ** t) / (v.sqrt() + eps)
            r = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t))
            p.sub_(lr * r * m_hat * l)
        else:
            p.sub_(lr * m_hat)


def ulp32(ref):
    """One fp32 unit in the last place of each float64 reference value (2^-149 below the normal range)."""
    _, e = torch.frexp(ref.abs())                                    # |ref| = f 2^e, f in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), (e - 24).clamp(min=-149))


def oracle_errors(got, ref, lr, slack_ulps=0.0):
    """-> {"p", "exp_avg", "exp_avg_sq"}: the error of the fp32 tensors got = (p, m, v) against the float64 ref = (p, m, v):
    max |x - ref| / (|ref| + lr) for p, the maximal relative error for the moments.  slack_ulps fp32 ulps of the reference
    value are taken off every |x - ref| first (not below 0).  Finite inputs only: every element counts."""
    out = {}
    for name, x, r, floor in (("p", got[0], ref[0], lr), ("exp_avg", got[1], ref[1], 0.0), ("exp_avg_sq", got[2], ref[2], 0.0)):
        x = x.detach().to("cpu", torch.float64).reshape(-1)
        r = r.reshape(-1)
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(r).all()), name
        d = ((x - r).abs() - slack_ulps * ulp32(r)).clamp(min=0.0)
        den = r.abs() + floor
        q = torch.where(d == 0, torch.zeros_like(d), d / den)        # an exact value is no error, whatever the reference is
        out[name] = float(q.max()) if q.numel() else 0.0
    return out


def within_twice(candidate, reference, lr):
    """The 2x rule, per quantity.  candidate, reference: ((p, m, v) fp32, (p, m, v) float64 oracle) pairs sharing the oracle.
    -> (ok, {name: (candidate's error net of one ulp, torch's error)}).  The factor 2 allows another valid rounding order of
    the same chain of about ten ops; a wrong coefficient or a missed step is orders of magnitude outside it."""
    e_c = oracle_errors(candidate[0], candidate[1], lr, slack_ulps=1.0)
    e_t = oracle_errors(reference[0], reference[1], lr)
    return all(e_c[k] <= 2.0 * e_t[k] for k in e_c), {k: (e_c[k], e_t[k]) for k in e_c}


ORACLE_SIZES = [5, 1023, CHUNK + 5]
ORACLE_LRS = [3e-3, 1e-3, 2e-3, 3e-3, 4e-3, 1e-4, 3e-3, 2e-3, 1e-3, 3e-3, 5e-4, 3e-3]      # 12 steps, never 0
ORACLE_EPS = 1e-8


def oracle_inputs(seed=31):
    """-> (initial parameters, per step the gradients, per step the learning rate): fp32 on the CPU, finite values only,
    every gradient tensor at a magnitude of its own between 1e-3 and 1e2."""
    gen = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=gen) for n in ORACLE_SIZES]
    grads = [[torch.randn(n, generator=gen) * (10.0 ** float(torch.randint(-3, 3, (1,), generator=gen))) for n in ORACLE_SIZES]
             for _ in ORACLE_LRS]
    return p0, grads, list(ORACLE_LRS)


def oracle_run(opt_class, device, betas, **kw):
    """`opt_class` over oracle_inputs() on `device` -> (p, exp_avg, exp_avg_sq): every step's fp32 values of every tensor,
    concatenated on the CPU in oracle_trajectory()'s order."""
    p0, grads, lrs = oracle_inputs()
    ps = [p.to(device).requires_grad_(True) for p in p0]
    opt = opt_class(ps, lr=lrs[0], betas=betas, eps=ORACLE_EPS, **kw)
    rec = []
    for gs, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        for p, g in zip(ps, gs):
            p.grad = g.to(device)
        opt.step()
        rec.append([torch.cat([p.detach().reshape(-1) for p in ps])] +
                   [torch.cat([opt.state[p][k].reshape(-1) for p in ps]) for k in ("exp_avg", "exp_avg_sq")])
    return tuple(torch.cat([r[j] for r in rec]).cpu() for j in range(3))


def oracle_trajectory(betas):
    """radam_ref over oracle_inputs() -> ((p, m, v) float64, the learning rate of every element's step)."""
    p0, grads, lrs = oracle_inputs()
    ref = [[p.double() for p in p0], [torch.zeros_like(p, dtype=torch.float64) for p in p0],
           [torch.zeros_like(p, dtype=torch.float64) for p in p0]]
    rec, rec_lr = [], []
    for step, (gs, lr) in enumerate(zip(grads, lrs), 1):
        radam_ref(ref[0], [g.double() for g in gs], ref[1], ref[2], [step] * len(gs), lr, betas[0], betas[1], ORACLE_EPS)
        rec.append([torch.cat([x.reshape(-1) for x in ref[j]]) for j in range(3)])
        rec_lr.append(torch.full_like(rec[-1][0], lr))
    return tuple(torch.cat([r[j] for r in rec]) for j in range(3)), torch.cat(rec_lr)


# ---------------------------------------------------------------------------------------------- slabs and guard bands
BAND = 64                                                         # elements on either side, before the mod-4 offset
SENTINEL = 12345.678                                               # finite; no update of these tests produces it
# 1, 3: below one float4        4, 5: one float4 (+ tail)        1020, 1023, 1024, 1028: nv = 255, 255 + tail 3, nv == kBlock
# (the first unroll slot exactly full), 257        4092, 4095: the last float4 of a chunk, tail 3 at its end
# C: e0 >= n for a second chunk        C + 1, C + 4: a second chunk of one dword / one float4        2 C, 2 C + 3
BAND_SIZES = [1, 3, 4, 5, 1020, 1023, 1024, 1028, 4092, 4095, CHUNK, CHUNK + 1, CHUNK + 4, 2 * CHUNK, 2 * CHUNK + 3]
# name -> tensor index -> start element modulo 4 of (p, g, exp_avg, exp_avg_sq).  The kernel ORs the four addresses: one
# misaligned stream sends the whole chunk down the dword path.  The "only" cases walk byte offsets 4, 8 and 12 over the sizes.
ALIGN_CASES = {
    "all_aligned": lambda i: (0, 0, 0, 0),
    "all_plus1_byte4": lambda i: (1, 1, 1, 1),
    "all_plus2_byte8": lambda i: (2, 2, 2, 2),
    "all_plus3_byte12": lambda i: (3, 3, 3, 3),
    "only_g_misaligned": lambda i: (0, 1 + i % 3, 0, 0),
    "only_exp_avg_misaligned": lambda i: (0, 0, 1 + (i + 1) % 3, 0),
    "only_p_misaligned": lambda i: (1 + (i + 2) % 3, 0, 0, 0),
}


class Slab:
    """[band | tensor | band] in one allocation of its own; .view is the tensor, starting at element BAND + offset."""

    def __init__(self, values, offset, device, band=BAND):
        n = values.numel()
        self.start, self.n = band + offset, n
        self.full = torch.full((self.start + n + band,), SENTINEL, dtype=torch.float32, device=device)
        self.view = self.full[self.start:self.start + n].view(values.shape)
        self.view.copy_(values)
        assert self.full.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 4 * (offset % 4)
        self._sentinel = torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()

    def bands_intact(self):
        b = self.full.view(torch.int32)
        return bool((b[:self.start] == self._sentinel).all()) and bool((b[self.start + self.n:] == self._sentinel).all())

    def bits(self):
        return self.full.view(torch.int32).clone()


def banded_streams(case, device, sizes=BAND_SIZES, seed=21):
    """-> per tensor {"p", "g", "m", "v"}: Slabs laid out by ALIGN_CASES[case]; p random, g and the moments zero."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        off = ALIGN_CASES[case](i)
        vals = {"p": torch.randn(n, generator=gen), "g": torch.zeros(n), "m": torch.zeros(n), "v": torch.zeros(n)}
        out.append({k: Slab(vals[k], o, device) for k, o in zip("pgmv", off)})
    return out


def plant_state(opt, params, streams):
    """The state torch's _init_group would create (step = tensor(0.) on the CPU, zeroed moments), on the slabs' views."""
    for p, s in zip(params, streams):
        s["m"].view.zero_()
        s["v"].view.zero_()
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": s["m"].view, "exp_avg_sq": s["v"].view}


def banded_optimizer(opt_class, case, device, sizes=BAND_SIZES, **kw):
    """-> (optimizer, parameters, streams): every parameter a leaf on its slab's view, its .grad the gradient slab's view
    (refilled in place by the caller), the state planted before the first step."""
    streams = banded_streams(case, device, sizes)
    params = [s["p"].view.detach().requires_grad_(True) for s in streams]
    for p, s in zip(params, streams):
        assert p.data_ptr() == s["p"].view.data_ptr()
        p.grad = s["g"].view
    opt = opt_class(params, lr=LRS[0], **kw)
    plant_state(opt, params, streams)
    return opt, params, streams


def planted_gradient(gen, n, plant):
    """n gradient values at a random magnitude 1e-12 .. 1e6; with `plant`, SPECIALS at the head and mirrored at the tail
    (the n % 4 tail lanes see them too)."""
    g = torch.randn(n, generator=gen) * (10.0 ** float(torch.randint(-12, 7, (1,), generator=gen)))
    if plant and n >= 2 * len(SPECIALS):
        g[:len(SPECIALS)] = torch.tensor(SPECIALS)
        g[-len(SPECIALS):] = torch.tensor(SPECIALS)
    return g
