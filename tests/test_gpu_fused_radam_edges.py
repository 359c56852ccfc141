"""GPU (-m gpu): the edges of the one-pass RAdam (mhaq_fq_radam_step, csrc/optim.hip, behind mhaq_amd/optim.py: FusedRAdam)
that tests/test_gpu_fused_radam.py leaves out.  The yardstick is torch.optim.RAdam(foreach=True) on the same device and
inputs, EQUAL BITS in p, exp_avg, exp_avg_sq and step after every step (C = one chunk, 4096 elements):

    hyper-parameters   the SECOND branch of radam_element's lerp (float(1 - beta1) >= 0.5: beta1 0.5, 0.5 +- 1e-10, 0.3, 0.0)
                       beside the first (0.95, 0.6); beta2 rectified from step 6 (0.999, 0.99, 0.9) and never (0.5, 0.0);
                       eps 1e-8, 1e-3 and 0 (NaN at the same elements with the same bits)
    guard bands        p, grad, exp_avg and exp_avg_sq each inside its own [band | tensor | band] slab: 15 sizes around the
                       float4, unroll-slot and chunk edges x 7 alignments (all four streams at +0 / +1 / +2 / +3 elements;
                       only g, only exp_avg, only p misaligned, at byte offsets 4, 8 and 12); no band and no gradient written
    table states       6 parameter groups of 64, 65, 129, 3, 10 and 1 tensors plus a second optimizer, interleaved for 20 steps
                       without a host synchronisation: 7 work lists through a cache of 4 (evicted while earlier launches are
                       queued), descriptor rings of 8 that wrap several times; a non-default stream
    the C ABI          work entries whose chunk lies past the tensor's end touch no memory
    float64 oracle     tests/radam_ref.py, independent of the framework's op chain: the kernel's error is at most twice
                       torch's own plus one fp32 ulp
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import radam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = R.CHUNK


def _bits(ts):
    """Every element of the listed tensors, in logical order, as one int32 vector on the device."""
    return torch.cat([t.detach().reshape(-1) for t in ts]).view(torch.int32)


def _assert_same_bits(got, want, sizes, what):
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero().view(-1)
    first, ends = int(bad[0]), np.cumsum(sizes)
    i = int(np.searchsorted(ends, first, side="right"))
    raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} elements differ, first in tensor {i} ({sizes[i]} elements) at "
                         f"{first - (int(ends[i - 1]) if i else 0)}: {int(got[first]) & 0xffffffff:08x} != "
                         f"{int(want[first]) & 0xffffffff:08x}")


def _counters():
    from mhaq_amd import optim
    return optim.fused_radam_steps(), optim.fused_radam_fallbacks()


# ---------------------------------------------------------------------------------------------- hyper-parameters
# about a dozen tensors: 1, 3, 4, 5, 64, 1023 (planted), C, C + 5, 2 C + 3, [8,4,3,3] channels_last, two offset views
HYPER_SPECS = [("plain", (1,)), ("plain", (3,)), ("plain", (4,)), ("plain", (5,)), ("plain", (64,)), ("plain", (1023,)),
               ("plain", (CHUNK,)), ("plain", (CHUNK + 5,)), ("plain", (2 * CHUNK + 3,)), ("channels_last", (8, 4, 3, 3)),
               ("offset_view", (1023,)), ("offset_view", (CHUNK + 7,))]
PLANTED, ZEROED = 5, 4       # indices into HYPER_SPECS


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _make(kind, shape, vals):
    if kind == "plain":
        return vals.reshape(shape).to(DEV)
    if kind == "channels_last":
        return vals.reshape(shape).to(DEV).contiguous(memory_format=torch.channels_last)
    if kind == "offset_view":              # 4-byte aligned, 16-byte misaligned
        base = torch.zeros(vals.numel() + 1, device=DEV)
        base[1:] = vals.to(DEV)
        v = base[1:].view(shape)
        assert v.data_ptr() % 16 == 4
        return v
    raise AssertionError(kind)


@pytest.fixture(scope="module")
def hyper_inputs():
    """Initial values and nine steps of planted gradients (zeros, -0.0, a subnormal, +-inf, NaN, 1e-12 .. 1e6), made once."""
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(_numel(s), generator=gen) for _, s in HYPER_SPECS]
    grads = []
    for step in range(1, 10):
        gs = []
        for i, (_, s) in enumerate(HYPER_SPECS):
            g = torch.randn(_numel(s), generator=gen) * (10.0 ** float(torch.randint(-12, 7, (1,), generator=gen)))
            if i == PLANTED:
                g[:len(R.SPECIALS)] = torch.tensor(R.SPECIALS)
            if i == ZEROED and step == 3:
                g.zero_()
            if i == ZEROED and step == 4:
                g.zero_().neg_()                                       # all -0.0
            gs.append(g.to(DEV))
        grads.append(gs)
    return p0, grads


def _run_hyper(opt_class, inputs, betas, eps, **kw):
    """-> per step (bits of p, exp_avg, exp_avg_sq of every tensor; the step counts), all still on the device."""
    p0, grads = inputs
    ps = [_make(kind, shape, v).requires_grad_(True) for (kind, shape), v in zip(HYPER_SPECS, p0)]
    opt = opt_class(ps, lr=1e-3, betas=betas, eps=eps, **kw)
    out = []
    for step in range(1, 10):
        opt.param_groups[0]["lr"] = R.LRS[step - 1]
        for p, g in zip(ps, grads[step - 1]):
            p.grad = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g.view(p.shape))
        opt.step()
        out.append((_bits(ps), _bits([opt.state[p]["exp_avg"] for p in ps]), _bits([opt.state[p]["exp_avg_sq"] for p in ps]),
                    [float(opt.state[p]["step"]) for p in ps]))          # (the step counts live on the CPU)
    return out


_torch_hyper = {}


def _torch_hyper_run(inputs, betas, eps):
    key = (betas, eps)
    if key not in _torch_hyper:
        _torch_hyper[key] = _run_hyper(torch.optim.RAdam, inputs, betas, eps, foreach=True)
    return _torch_hyper[key]


def _assert_hyper_equal(got, want, what):
    sizes = [_numel(s) for _, s in HYPER_SPECS]
    for step, (g, w) in enumerate(zip(got, want), 1):
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), g, w):
            _assert_same_bits(a, b, sizes, f"{what}, step {step}, {name}")
        assert g[3] == w[3] == [float(step)] * len(sizes)


@pytest.mark.parametrize("eps", R.EPSS, ids=lambda e: f"eps={e!r}")
@pytest.mark.parametrize("betas", R.BETAS, ids=R.case_id)
def test_betas_and_eps_matrix_equals_torch_foreach_radam_bit_for_bit(betas, eps, hyper_inputs):
    """The test id names the lerp branch (lerp1: fmaf(w1, g - m, m); lerp2: fmaf(g - m, -(1 - w1), g)) and whether beta2
    rectifies from step 6 or never.  Every lerp2 case failed against the branch's first form, fmaf(-(g - m), 1 - w1, g): the
    element whose gradient is NaN had the other sign in p from step 1 on (MHAQ_RADAM_FORM bit 4)."""
    from mhaq_amd import optim
    steps0, fb0 = _counters()
    got = _run_hyper(optim.FusedRAdam, hyper_inputs, betas, eps)
    assert _counters() == (steps0 + 9, fb0)                                   # one launch per step, nothing handed to torch
    _assert_hyper_equal(got, _torch_hyper_run(hyper_inputs, betas, eps), R.case_id(betas, eps))
    # elements 0-2 of the planted tensor never see a non-zero g * g: with eps = 0 they are 0 / c2 -> NaN from step 1 on,
    # NaN on both sides with the same bits (the comparison above); with eps > 0 they stay finite
    first = sum(_numel(s) for _, s in HYPER_SPECS[:PLANTED])
    p_last = got[-1][0][first:first + 3].view(torch.float32)
    assert bool(torch.isnan(p_last).all()) == (eps == 0.0) and bool(torch.isfinite(p_last).all()) == (eps != 0.0)


# +-0, two finite values, a subnormal, +-inf, quiet NaNs of both signs without and with a payload, a signalling NaN
PAIR_BITS = [0x00000000, 0x80000000, 0x3fc00000, 0xc0100000, 0x00001234, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000,
             0x7fc00001, 0xffc12345, 0x7fa00000]


def _from_bits(bits):
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.int32)).view(torch.float32)


@pytest.mark.parametrize("betas", [R.DEFAULT_BETAS, (0.5, 0.999), (0.3, 0.99), (0.0, 0.9)], ids=R.case_id)
def test_every_pair_of_special_exp_avg_and_gradient_values_equals_torch_bit_for_bit(betas):
    """All 144 (exp_avg, gradient) pairs of PAIR_BITS, planted as the state, on the float4 and on the dword path, two steps.
    Where g - m is NaN the lerp's instruction decides whose sign and payload survive: the written forms of its second branch
    that round every finite value alike differ in 97 of these pairs."""
    from mhaq_amd import optim
    m0 = _from_bits([a for a in PAIR_BITS for _ in PAIR_BITS])
    g0 = _from_bits([b for _ in PAIR_BITS for b in PAIR_BITS])
    n = m0.numel()

    def run(opt_class, **kw):
        def at(off, vals):
            base = torch.zeros(off + n, device=DEV)
            base[off:].copy_(vals)
            assert base[off:].data_ptr() % 16 == 4 * off
            return base[off:]
        ps = [at(off, torch.linspace(-1.0, 1.0, n)).requires_grad_(True) for off in (0, 1)]
        opt = opt_class(ps, lr=3e-3, betas=betas, **kw)
        for off, p in zip((0, 1), ps):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": at(off, m0), "exp_avg_sq": at(off, torch.zeros(n))}
            p.grad = at(off, g0)
        assert torch.equal(_bits([opt.state[ps[1]]["exp_avg"]]).cpu(), m0.view(torch.int32))      # the bits arrived
        out = []
        for _ in range(2):
            opt.step()
            out.append(tuple(_bits([x(p) for p in ps]) for x in
                             (lambda p: p, lambda p: opt.state[p]["exp_avg"], lambda p: opt.state[p]["exp_avg_sq"])))
        return out

    steps0, fb0 = _counters()
    got = run(optim.FusedRAdam)
    assert _counters() == (steps0 + 2, fb0)
    want = run(torch.optim.RAdam, foreach=True)
    for step, (g, w) in enumerate(zip(got, want), 1):
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), g, w):
            _assert_same_bits(a, b, [n, n], f"{R.case_id(betas)}, step {step}, {name}")


# ---------------------------------------------------------------------------------------------- guard bands
@pytest.fixture(scope="module")
def band_gradients():
    gen = torch.Generator().manual_seed(22)
    return [[R.planted_gradient(gen, n, plant=True).to(DEV) for n in R.BAND_SIZES] for _ in range(9)]


def _run_banded(opt_class, case, gradients, **kw):
    """Nine steps on the slabs of `case`; after each: every band and the whole gradient slab bit-unchanged.
    -> per step the bits of (p, exp_avg, exp_avg_sq) of every tensor."""
    opt, ps, streams = R.banded_optimizer(opt_class, case, DEV, **kw)
    out = []
    for step in range(1, 10):
        opt.param_groups[0]["lr"] = R.LRS[step - 1]
        for s, g in zip(streams, gradients[step - 1]):
            s["g"].view.copy_(g)
        before = [s["g"].bits() for s in streams]
        opt.step()
        for i, (p, s) in enumerate(zip(ps, streams)):
            for k in "pgmv":
                assert s[k].bands_intact(), f"{case}, step {step}, {R.BAND_SIZES[i]} elements: a band of {k} was written"
            assert torch.equal(s["g"].bits(), before[i]), f"{case}, step {step}, {R.BAND_SIZES[i]} elements: g was written"
            st = opt.state[p]
            assert st["exp_avg"].data_ptr() == s["m"].view.data_ptr() and st["exp_avg_sq"].data_ptr() == s["v"].view.data_ptr()
            assert float(st["step"]) == step
        out.append(tuple(_bits([s[k].view for s in streams]) for k in "pmv"))
    return out


@pytest.mark.parametrize("case", list(R.ALIGN_CASES))
def test_guard_bands_stay_intact_at_every_size_and_alignment(case, band_gradients):
    """R.BAND_SIZES (1, 3, 4, 5, 1020, 1023, 1024, 1028, 4092, 4095, C, C + 1, C + 4, 2 C, 2 C + 3) in the alignment the test
    id names (R.ALIGN_CASES): a tail overrun, a float4 one vector too far or a write to the gradient lands in a band."""
    from mhaq_amd import optim
    steps0, fb0 = _counters()
    got = _run_banded(optim.FusedRAdam, case, band_gradients)
    assert _counters() == (steps0 + 9, fb0)              # every layout took the launch: a fallback would make this vacuous
    want = _run_banded(torch.optim.RAdam, case, band_gradients, foreach=True)
    for step, (g, w) in enumerate(zip(got, want), 1):
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), g, w):
            _assert_same_bits(a, b, R.BAND_SIZES, f"{case}, step {step}, {name}")
    assert not torch.equal(got[0][0], got[-1][0])


# ---------------------------------------------------------------------------------------------- table states
# Work lists are cached per size list, 4 per device (TableCache); descriptor tables come from rings of 8 per capacity of 64,
# 128, 192 ... descriptors (TablePool), shared by every group of that capacity.  Seven distinct size lists per step evict a
# work list at every launch; the capacity-64 ring takes 5 tables per step (groups of 64, 3, 10 and 1 tensors and the second
# optimizer) and wraps 12 times in 20 steps, the rings of the 65- and the 129-tensor group twice.
GROUP_SIZES = [[1 + (7 * i) % 61 for i in range(64)],                 # exactly 64 tensors: one full grain
               [1 + (5 * i) % 53 for i in range(65)],                 # 65: the second grain begins
               [1 + (3 * i) % 47 for i in range(129)],                # 129: the third
               [CHUNK, 2 * CHUNK + 3, 5],
               [1 + (11 * i) % 29 for i in range(10)],
               [1023]]
SECOND_SIZES = [CHUNK + 1, 7, 64, 3, 1028]
# steps 7 and 8 at rate 0 with step 8's gradients refilled in place: c1 = c2 = -0.0 twice over the same pointers, so the
# ring is asked for a table it still holds
LRS20 = [3e-3, 1e-3, 0.0, 3e-3, 2e-3, 3e-3, 0.0, 0.0, 4e-3, 1e-4, 3e-3, 1e-3, 2e-3, 0.0, 3e-3, 1e-3, 2e-3, 3e-3, 4e-3, 1e-3]


@pytest.fixture(scope="module")
def table_inputs():
    sizes = [n for g in GROUP_SIZES for n in g] + SECOND_SIZES
    gen = torch.Generator().manual_seed(41)
    p0 = torch.randn(sum(sizes), generator=gen)
    scale = torch.cat([torch.full((n,), 10.0 ** float(torch.randint(-6, 4, (1,), generator=gen))) for n in sizes])
    flats = [(torch.randn(sum(sizes), generator=gen) * scale).to(DEV) for _ in LRS20]
    return sizes, p0, flats


def _run_tables(first_class, second_class, inputs, **kw):
    """20 interleaved steps of one optimizer over GROUP_SIZES' six groups and a second one over SECOND_SIZES, with no host
    read-back and no synchronisation inside the loop -> per step the bits of (p, exp_avg, exp_avg_sq), the final step counts."""
    sizes, p0, flats = inputs
    ps = [v.clone().to(DEV).requires_grad_(True) for v in p0.split(sizes)]
    spans, o = [], 0
    for n in sizes:
        spans.append((o, n))
        o += n
    groups, at = [], 0
    for g in GROUP_SIZES:
        groups.append({"params": ps[at:at + len(g)]})
        at += len(g)
    first = first_class(groups, lr=1e-3, **kw)
    second = second_class(ps[at:], lr=1e-3, **kw)
    state = lambda p: (first if any(p is q for q in ps[:at]) else second).state[p]      # noqa: E731
    snaps = []
    torch.cuda.synchronize()
    for step, lr in enumerate(LRS20, 1):
        for grp in first.param_groups + second.param_groups:
            grp["lr"] = lr
        flat = flats[step - 1]
        for p, (o, n) in zip(ps, spans):
            if step % 2 == 1:
                p.grad = flat[o:o + n].clone()                         # a fresh tensor, as after zero_grad(set_to_none=True)
            else:
                p.grad.copy_(flat[o:o + n])                            # refilled in place
        first.step()
        second.step()
        owner = [first.state[p] for p in ps[:at]] + [second.state[p] for p in ps[at:]]
        snaps.append((_bits(ps), _bits([s["exp_avg"] for s in owner]), _bits([s["exp_avg_sq"] for s in owner])))
    torch.cuda.synchronize()
    return snaps, [float(state(p)["step"]) for p in ps]


def test_six_groups_and_a_second_optimizer_interleaved_for_twenty_steps_without_a_sync(table_inputs):
    """Groups of exactly 64, 65 and 129 tensors; more than 4 work lists, each evicted while earlier launches are queued; the
    descriptor rings wrapped; two optimizers stepped alternately; fresh gradients on odd steps, refilled ones on even steps."""
    from mhaq_amd import optim
    assert [len(g) for g in GROUP_SIZES] == [64, 65, 129, 3, 10, 1]
    assert len({tuple(g) for g in GROUP_SIZES + [SECOND_SIZES]}) == 7 > 4
    steps0, fb0 = _counters()
    got, got_steps = _run_tables(optim.FusedRAdam, optim.FusedRAdam, table_inputs)
    assert _counters() == (steps0 + 7 * len(LRS20), fb0)                 # 6 groups + the second optimizer, every step
    want, want_steps = _run_tables(torch.optim.RAdam, torch.optim.RAdam, table_inputs, foreach=True)
    assert got_steps == want_steps == [float(len(LRS20))] * len(got_steps)
    for step, (g, w) in enumerate(zip(got, want), 1):
        for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), g, w):
            _assert_same_bits(a, b, table_inputs[0], f"step {step}, {name}")
    assert not torch.equal(got[0][0], got[-1][0])


def test_nine_steps_on_a_non_default_stream_give_the_same_bits(hyper_inputs):
    from mhaq_amd import optim
    betas, eps = (0.5, 0.999), 1e-8
    want = _torch_hyper_run(hyper_inputs, betas, eps)                         # on the default stream
    side = torch.cuda.Stream(device=DEV)
    steps0, fb0 = _counters()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream(DEV) == side
        got = _run_hyper(optim.FusedRAdam, hyper_inputs, betas, eps)
    side.synchronize()
    torch.cuda.synchronize()
    assert _counters() == (steps0 + 9, fb0)
    _assert_hyper_equal(got, want, "side stream")


# ---------------------------------------------------------------------------------------------- the C ABI, directly
DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("c1", "<f4"), ("c2", "<f4")])
WORK = np.dtype([("tensor", "<i4"), ("chunk", "<i4")])
ABI_SIZES = [5, 1023, CHUNK, CHUNK + 5, 2 * CHUNK, 2 * CHUNK + 3]
ABI_BAND = 3 * CHUNK         # trailing: the two chunks past a tensor's end that the extra entries name lie inside it


def _abi_buffers(start):
    """Per tensor {"p","g","m","v"} -> (whole buffer [start | n | ABI_BAND] filled with the sentinel, n)."""
    gen = torch.Generator().manual_seed(51)
    out = []
    for n in ABI_SIZES:
        t = {}
        for k in "pgmv":
            full = torch.full((start + n + ABI_BAND,), R.SENTINEL, dtype=torch.float32)
            x = torch.randn(n, generator=gen)
            full[start:start + n] = x * x if k == "v" else x             # exp_avg_sq is never negative
            t[k] = full.to(DEV)
        out.append((t, n))
    return out


def _abi_launch(bufs, start, work, scalars):
    from mhaq_amd import _lib, optim
    L = _lib.lib()
    descs = np.zeros(len(bufs), DESC)
    for i, (t, n) in enumerate(bufs):
        for k in "pgmv":
            descs[i][k] = t[k].data_ptr() + 4 * start
        descs[i]["n"] = n
    wl = np.array(work, WORK)
    for step, lr, betas, eps in scalars:
        c1, c2 = optim.radam_scalars(float(step), lr, *betas)
        descs["c1"], descs["c2"] = c1, c2
        dtab = torch.from_numpy(descs.view(np.uint8).copy()).to(DEV)
        wtab = torch.from_numpy(wl.view(np.uint8).copy()).to(DEV)
        assert dtab.numel() == 48 * len(bufs) and wtab.numel() == 8 * len(work)
        torch.cuda.synchronize()
        rc = L.mhaq_fq_radam_step(ctypes.c_void_p(dtab.data_ptr()), len(bufs), ctypes.c_void_p(wtab.data_ptr()), len(work),
                                  1.0 - betas[0], betas[1], 1.0 - betas[1], eps, None)
        assert rc == 0
        torch.cuda.synchronize()


@pytest.mark.parametrize("start", [0, 1], ids=["float4_path", "dword_path"])
def test_work_entries_past_a_tensors_end_touch_no_memory(start):
    """Hand-built tables through _lib: besides every real (tensor, chunk) the list names, per tensor, the two chunks behind
    its last one -- for n = C and 2 C the first of them begins exactly at the end (e0 == n).  Every buffer ends in 3 C
    sentinels, so even a kernel that did not skip them would stay inside allocated memory, and show."""
    real, extra = [], []
    for i, n in enumerate(ABI_SIZES):
        c0 = (n + CHUNK - 1) // CHUNK
        real += [(i, c) for c in range(c0)]
        extra += [(i, c0), (i, c0 + 1)]
        assert (c0 + 2) * CHUNK <= n + ABI_BAND
    mixed = []
    for j, w in enumerate(real):                   # the extras between the real entries, not behind them
        mixed.append(w)
        if j < len(extra):
            mixed.append(extra[j])
    mixed = extra[len(real):] + mixed
    assert sorted(mixed) == sorted(real + extra)
    # step 3: c2 = -0.0, unrectified; step 7: rectified; the second branch of the lerp once
    scalars = [(3, 3e-3, R.DEFAULT_BETAS, 1e-8), (7, 2e-3, R.DEFAULT_BETAS, 1e-8), (7, 1e-3, (0.3, 0.99), 1e-3)]
    plain, with_extras, untouched = _abi_buffers(start), _abi_buffers(start), _abi_buffers(start)
    _abi_launch(plain, start, real, scalars)
    _abi_launch(with_extras, start, mixed, scalars)
    sentinel = torch.tensor(R.SENTINEL).view(torch.int32).item()
    for (a, n), (b, _), (u, _) in zip(plain, with_extras, untouched):
        for k in "pgmv":
            ab, bb = a[k].view(torch.int32), b[k].view(torch.int32)
            for bits in (ab, bb):
                assert bool((bits[:start] == sentinel).all()) and bool((bits[start + n:] == sentinel).all()), (n, k)
            assert torch.equal(ab, bb), (n, k)                             # the real chunks: as without the extra entries
            assert torch.equal(bb, u[k].view(torch.int32)) == (k == "g"), (n, k)      # g read-only; p, m and v did move
        assert not bool((a["p"][start:start + n] == u["p"][start:start + n]).any())      # every element of every chunk ran


# ---------------------------------------------------------------------------------------------- float64 oracle
@pytest.mark.parametrize("betas", [R.DEFAULT_BETAS, (0.3, 0.99)], ids=R.case_id)
def test_the_kernels_error_against_the_float64_oracle_is_within_twice_torchs(betas):
    """12 steps, finite gradients, every element compared.  The figures printed are torch's own (the reference's), in units of
    2^-24: DESIGN section 14 has them."""
    from mhaq_amd import optim
    steps0, fb0 = _counters()
    fused = R.oracle_run(optim.FusedRAdam, DEV, betas)
    assert _counters() == (steps0 + len(R.ORACLE_LRS), fb0)
    framework = R.oracle_run(torch.optim.RAdam, DEV, betas, foreach=True)
    ref, lr = R.oracle_trajectory(betas)
    ok, errs = R.within_twice((fused, ref), (framework, ref), lr)
    for name, (e_k, e_t) in errs.items():
        print(f"oracle {R.case_id(betas)} {name}: torch {e_t * 2 ** 24:.2f} x 2^-24, kernel net of one ulp {e_k * 2 ** 24:.2f} x 2^-24")
    assert ok, errs
