"""GPU (-m gpu): the ReLU / residual-add forms of the NoisyAct kernels (pt_fwd_relu_kernel / pt_bwd_relu_kernel behind
mhaq_fq_act_relu_fwd / _bwd / _bwd_partials, the ActReluFn node, ops.act_relu_layer, NoisyAct.forward_fused) against an
INDEPENDENT oracle: torch eager on the CPU -- relu(z + addend), oracle/fq_eager.act_fake_quant, autograd -- with the signs
of tests/philox_ref.  tests/test_gpu_fused_act.py compares these kernels with the project's own unfused ones, which share
their element bodies; here nothing is shared.  Cases: tests/fused_act_cases.py (checked by test_fused_act_cases_cpu.py).

Elementwise outputs (y, a, gx) must be the oracle's VALUES, NaN where it is NaN.  The one allowance is the existing one
of tests/test_gpu_special_values.py (its helper is used): where |g_y| * s < 2^-126, gx may differ by 8 subnormal ulps
(DESIGN.md section 8).  Those elements (the +-1e-42 gradients of the special family) are held to that rule in ONE place,
test_gx_where_g_times_s_underflows_is_within_8_subnormal_ulps, over every case the other tests use -- the other tests
compare every remaining element for equality: the distance grows as 1 / (2 s), and the
parameter sets here go down to s = 2^-9.9 (see that test's docstring).
Parameter gradients: within 1e-6 x sum|terms| (tests/test_gpu_act16.yardsticks on (a, g_y)) in
the finite family; in the special family NaN exactly where the oracle's are, equal where they are +-inf, finite elsewhere.
Every output lives inside a larger buffer filled with a sentinel: no byte outside [0, n) may change."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import fused_act_cases as C  # noqa: E402
from tests.test_gpu_special_values import _same_values  # noqa: E402

DEV = "cuda:0"
SEED, OFFSET = 1234, 7
GUARD = 64                                   # sentinel elements on each side of every output
SENTINEL = 0x7FA5C3C3                        # a NaN no kernel produces, compared by its bits
# (z input / output, g_a) x addend: with an addend the backward reads the ReLU's output (ActReluFn saves a)
BWD_FORMS = [(False, "z", False), (False, "z", True), (False, "a", False), (False, "a", True),
             (True, "a", False), (True, "a", True)]


@functools.lru_cache(maxsize=None)
def _oracle(n, pset, with_add, family, method, use_gy=True, use_ga=True, seed=SEED, offset=OFFSET):
    return C.oracle(C.build(n, pset, with_add, family), method, seed, offset, use_gy, use_ga)


def _lib_ops():
    from mhaq_amd import _lib, ops
    return _lib, _lib.lib(), ops


def _buf(n, shift=0, src=None):
    """n floats `shift` elements past a 16-byte boundary inside a sentinel-filled buffer: (whole buffer, the view)."""
    raw = torch.full((2 * GUARD + 4 + n,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    assert raw.data_ptr() % 16 == 0
    view = raw[GUARD + shift:GUARD + shift + n]
    assert view.data_ptr() % 16 == 4 * shift
    if src is not None:
        view.copy_(src)
    return raw, view


def _untouched(raw, shift, n):
    bits = raw.view(torch.int32)
    return bool((bits[:GUARD + shift] == SENTINEL).all()) and bool((bits[GUARD + shift + n:] == SENTINEL).all())


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _dev1(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _forward(case, want_a, shifts=(0, 0, 0, 0)):
    """mhaq_fq_act_relu_fwd; shifts = element offsets of (z, addend, y, a_out).  (y, a or None, params_out) on the CPU."""
    _lib, L, ops = _lib_ops()
    q, n = case.q, case.n
    _, z = _buf(n, shifts[0], case.z)
    add = _buf(n, shifts[1], case.addend)[1] if case.with_add else None
    y_raw, y = _buf(n, shifts[2])
    a_raw, a = _buf(n, shifts[3]) if want_a else (None, None)
    ls, lq, b = _dev1(q.log_s), _dev1(q.log_q), _dev1(q.b)
    pout = torch.full((5,), float("nan"), device=DEV)
    _lib.check(L.mhaq_fq_act_relu_fwd(z.data_ptr(), _ptr(add), y.data_ptr(), _ptr(a), n, ls.data_ptr(), lq.data_ptr(),
                                      b.data_ptr(), pout.data_ptr(), ops._stream()), "mhaq_fq_act_relu_fwd")
    torch.cuda.synchronize()
    assert _untouched(y_raw, shifts[2], n), ("y wrote outside [0, n)", n, shifts)
    if want_a:
        assert _untouched(a_raw, shifts[3], n), ("a_out wrote outside [0, n)", n, shifts)
    return y.cpu(), (a.cpu() if want_a else None), pout.cpu()


def _backward(q, src, gy, ga, method, shifts=(0, 0, 0, 0), seed=SEED, offset=OFFSET, offset_dev=None, partials=False):
    """mhaq_fq_act_relu_bwd (or, `partials`, _bwd_partials: the row count instead of the gradients); shifts = element
    offsets of (z, g_y, g_a, gx).  (gx, the three parameter gradients | nparts) on the CPU."""
    _lib, L, ops = _lib_ops()
    n = src.numel()
    _, z = _buf(n, shifts[0], src)
    _, g = _buf(n, shifts[1], gy)
    g_a = _buf(n, shifts[2], ga)[1] if ga is not None else None
    gx_raw, gx = _buf(n, shifts[3])
    params = q.params().to(DEV)
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    m = C.METHOD_VALUE[method]
    if partials:
        nparts = ctypes.c_int32(-1)
        _lib.check(L.mhaq_fq_act_relu_bwd_partials(z.data_ptr(), g.data_ptr(), _ptr(g_a), gx.data_ptr(), n,
                                                   params.data_ptr(), m, seed, offset, _ptr(offset_dev), ws.data_ptr(), nb,
                                                   ctypes.byref(nparts), ops._stream()), "mhaq_fq_act_relu_bwd_partials")
        out = nparts
    else:
        grads = torch.full((3,), float("nan"), device=DEV)
        _lib.check(L.mhaq_fq_act_relu_bwd(z.data_ptr(), g.data_ptr(), _ptr(g_a), gx.data_ptr(), n, params.data_ptr(), m,
                                          seed, offset, _ptr(offset_dev), grads.data_ptr(), ws.data_ptr(), nb,
                                          ops._stream()), "mhaq_fq_act_relu_bwd")
        out = grads
    torch.cuda.synchronize()
    assert _untouched(gx_raw, shifts[3], n), ("gx wrote outside [0, n)", n, shifts)
    return gx.cpu(), (out.value if partials else out.cpu())


def _tiny(gy, s):
    """The elements of the one allowance: g_y * s underflows (tests/test_gpu_special_values.py)."""
    g = gy.numpy().astype(np.float64)
    return (np.abs(g) * s < 2.0 ** -126) & (g != 0)


def _check_gx(gx, o, case, what, use_gy=True):
    """Equal values, NaN as NaN, on every element whose g_y * s does not underflow; those that do belong to
    test_gx_where_g_times_s_underflows_is_within_8_subnormal_ulps, which runs every case that comes through here."""
    keep = ~_tiny(case.gy, case.q.s) if use_gy else np.ones(case.n, dtype=bool)
    assert gx.shape == o["gx"].shape
    assert _same_values(gx.numpy()[keep], o["gx"].numpy()[keep]), ("gx", what)


def _check_grads(got, o, case, method, what, use_gy=True):
    """got: three floats (d/dlog_act_s, d/dlog_act_q, d/dact_b) against the oracle's."""
    ref = [float(g) for g in o["grads"]]
    got = [float(g) for g in got]
    if case.family == "finite":
        bars = C.yardsticks(case, o["a"], o["r"], method, use_gy)
        for name, a, r_, bar in zip(("log_act_s", "log_act_q", "act_b"), got, ref, bars):
            assert math.isfinite(r_) and math.isfinite(bar), (name, what, r_, bar)     # never skipped (CPU test)
            assert abs(a - r_) <= bar, (name, what, a, r_, abs(a - r_), bar)
        return
    for name, a, r_ in zip(("log_act_s", "log_act_q", "act_b"), got, ref):
        if math.isnan(r_):
            assert math.isnan(a), (name, what, a, r_)
        elif math.isinf(r_):
            assert a == r_, (name, what, a, r_)
        else:
            assert math.isfinite(a), (name, what, a, r_)


# ------------------------------------------------------------------------------------------------ C ABI: forward
@pytest.mark.parametrize("family", ["finite", "special"])
@pytest.mark.parametrize("pset", C.FORWARD_SETS)
def test_forward_equals_the_oracle(pset, family):
    """y, a_out and params_out at every size, with and without an addend and a_out (the forward has no method)."""
    q = C.quantizer(pset)
    for n in C.SIZES:
        for with_add in (False, True):
            case = C.build(n, pset, with_add, family)
            o = _oracle(n, pset, with_add, family, "LSQ")
            for want_a in (False, True):
                what = (pset, family, n, with_add, want_a)
                y, a, pout = _forward(case, want_a)
                assert _same_values(y.numpy(), o["y"].numpy()), ("y", what)
                if want_a:
                    assert _same_values(a.numpy(), o["a"].numpy()), ("a", what)     # (CPU relu(-0.0) is -0.0: by value)
                assert torch.equal(pout, q.params()), ("params_out", what, pout.tolist(), q.params().tolist())


# ------------------------------------------------------------------------------------------------ C ABI: backward
@pytest.mark.parametrize("family", ["finite", "special"])
@pytest.mark.parametrize("pset", list(C.PARAM_SETS))
@pytest.mark.parametrize("method", C.METHODS)
def test_backward_equals_the_oracle(method, pset, family):
    """gx and the three parameter gradients at every size: z the ReLU's input or its output, with and without g_a, with
    and without an addend in front of the ReLU."""
    q = C.quantizer(pset)
    for n in C.SIZES:
        for with_add, src_kind, has_ga in BWD_FORMS:
            case = C.build(n, pset, with_add, family)
            o = _oracle(n, pset, with_add, family, method, True, has_ga)
            src = case.z if src_kind == "z" else o["a"]
            what = (method, pset, family, n, with_add, src_kind, has_ga)
            gx, grads = _backward(q, src, case.gy, case.ga if has_ga else None, method)
            _check_gx(gx, o, case, what)
            _check_grads(grads, o, case, method, what)


@pytest.mark.parametrize("pset", list(C.PARAM_SETS))
@pytest.mark.parametrize("method", C.METHODS)
def test_gx_where_g_times_s_underflows_is_within_8_subnormal_ulps(method, pset):
    """The elements the other tests leave to this one: |g_y| * s < 2^-126 (the +-1e-42 gradients of the special family),
    at every size that holds them and the 1155 elements of the autograd tests, in every backward form.  The rule is the
    existing helper's: at most 8 subnormal ulps (2^-149) from the oracle.

    The reference rounds g_y * s to the subnormal grid first and the division by s magnifies that half ulp to 1 / (2 s)
    ulps of g_y: 2.1 at s = 0.2371, 8 at 2^-4, 10.3 at 2^-4.37, 482 at 2^-9.913.  The exact-quotient correction of the
    STE / LSQ element used to return g_y itself there (10 and 250 ulps from the oracle at the two smallest scales of
    this file, measured); such elements now take the IEEE division (csrc/fq_pt.hip product_underflowed)."""
    q = C.quantizer(pset)
    worst, seen = 0.0, 0
    for n in [n for n in C.SIZES if n >= C.SPECIAL_STRIDE] + [N4]:
        for with_add, src_kind, has_ga in BWD_FORMS:
            case = C.build(n, pset, with_add, "special")
            o = _oracle(n, pset, with_add, "special", method, True, has_ga)
            tiny = _tiny(case.gy, q.s)
            seen += int(tiny.sum())
            src = case.z if src_kind == "z" else o["a"]
            gx, _ = _backward(q, src, case.gy, case.ga if has_ga else None, method)
            got, ref = gx.numpy()[tiny].astype(np.float64), o["gx"].numpy()[tiny].astype(np.float64)
            assert np.isfinite(got).all() and np.isfinite(ref).all()
            worst = max(worst, float(np.abs(got - ref).max()) / 2.0 ** -149)
    print(f"{method} {pset} s={q.s!r}: {seen} underflowing elements, worst |gx - oracle| = {worst:g} subnormal ulps")
    assert seen > 0
    assert worst <= 8, (method, pset, q.s, worst)


def test_backward_cases_reach_the_generic_and_the_fast_element():
    """What the parameter sets are for: fast = fast_div && lo < hi && s > 0 (pt_bwd_relu_kernel) holds for some, fails on
    fast_div for the all-ones significand and on lo < hi for the inverted bounds."""
    def fast_div(s):
        bits = np.float32(s).view(np.uint32)
        rbits = (np.float32(1.0) / np.float32(s)).view(np.uint32)
        return 0 < ((bits >> 23) & 0xff) < 255 and 0 < ((rbits >> 23) & 0xff) < 255 and (bits & 0x7FFFFF) != 0x7FFFFF
    fast = {k: fast_div(C.quantizer(k).s) and C.quantizer(k).lo < C.quantizer(k).hi for k in C.PARAM_SETS}
    assert not fast["all_ones"] and not fast["inverted"]
    assert fast["unsigned"] and fast["nonpow2_a"] and fast["nonpow2_b"] and fast["above_zero"]
    assert C.quantizer("inverted").s > 0 and fast_div(C.quantizer("inverted").s)


# ------------------------------------------------------------------------------------------------ C ABI: alignment
ALL_SHIFTS = [(1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3)]


@pytest.mark.parametrize("pset", ["unsigned", "nonpow2_b"])
def test_forward_with_misaligned_pointers_gives_the_same_values(pset):
    """All pointers 1, 2, 3 elements off a 16-byte boundary; then exactly one of addend, a_out (every other pointer
    aligned): one misaligned pointer sends the whole launch to the dword form."""
    for n in C.SIZES:
        case = C.build(n, pset, True, "finite")
        o = _oracle(n, pset, True, "finite", "LSQ")
        for shifts in ALL_SHIFTS + [(0, 1, 0, 0), (0, 0, 0, 1), (0, 0, 0, 3), (0, 2, 0, 0)]:
            y, a, pout = _forward(case, True, shifts)
            assert _same_values(y.numpy(), o["y"].numpy()), ("y", pset, n, shifts)
            assert _same_values(a.numpy(), o["a"].numpy()), ("a", pset, n, shifts)
            assert torch.equal(pout, case.q.params())


def _unfused_nparts(n, aligned, method):
    """nparts_out of mhaq_fq_act_bwd_partials for n elements in the same alignment class."""
    _lib, L, ops = _lib_ops()
    sh = 0 if aligned else 1
    x, g, gx = (_buf(n, sh, torch.ones(n))[1] for _ in range(3))
    params = C.quantizer("unsigned").params().to(DEV)
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    nparts = ctypes.c_int32(-1)
    _lib.check(L.mhaq_fq_act_bwd_partials(x.data_ptr(), g.data_ptr(), gx.data_ptr(), n, params.data_ptr(),
                                          C.METHOD_VALUE[method], None, SEED, OFFSET, None, ws.data_ptr(), nb,
                                          ctypes.byref(nparts), ops._stream()), "mhaq_fq_act_bwd_partials")
    torch.cuda.synchronize()
    return nparts.value


@pytest.mark.parametrize("pset", ["unsigned", "nonpow2_b"])
@pytest.mark.parametrize("method", C.METHODS)
def test_backward_with_misaligned_pointers_gives_the_same_values(method, pset):
    """All pointers shifted by 1, 2, 3 elements; then exactly one of g_a, gx (and of z, g_y).  Same values as the aligned
    launch, and the row count mhaq_fq_act_bwd_partials reports for the same n in the same alignment class."""
    q = C.quantizer(pset)
    for n in C.SIZES:
        case = C.build(n, pset, False, "finite")
        o = _oracle(n, pset, False, "finite", method)
        for shifts in [(0, 0, 0, 0)] + ALL_SHIFTS + [(0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 3, 0), (0, 0, 0, 2), (1, 0, 0, 0),
                                                      (0, 1, 0, 0)]:
            what = (method, pset, n, shifts)
            gx, grads = _backward(q, case.z, case.gy, case.ga, method, shifts)
            _check_gx(gx, o, case, what)
            _check_grads(grads, o, case, method, what)
            gx2, nparts = _backward(q, case.z, case.gy, case.ga, method, shifts, partials=True)
            _check_gx(gx2, o, case, what)
            aligned = n >= 4 and not any(shifts)
            assert nparts == _unfused_nparts(n, aligned, method), ("nparts_out", what, nparts)
        # without g_a its alignment does not count
        gx, grads = _backward(q, case.z, case.gy, None, method, (0, 0, 1, 0))
        _check_gx(gx, _oracle(n, pset, False, "finite", method, True, False), case, (method, pset, n, "no g_a"))


def test_device_offset_word_is_added_to_the_host_offset():
    """(offset, *offset_dev = k) gives the bits of (offset + k, NULL)."""
    n, k = 4099, 3
    q = C.quantizer("nonpow2_a")
    case = C.build(n, "nonpow2_a", False, "finite")
    word = torch.tensor([k], dtype=torch.int64, device=DEV)
    for method in ("STE", "EWGS"):
        gx_a, gr_a = _backward(q, case.z, case.gy, case.ga, method, offset=5, offset_dev=word)
        gx_b, gr_b = _backward(q, case.z, case.gy, case.ga, method, offset=5 + k)
        gx_c, gr_c = _backward(q, case.z, case.gy, case.ga, method, offset=5)
        assert torch.equal(gx_a.view(torch.int32), gx_b.view(torch.int32))
        assert torch.equal(gr_a.view(torch.int32), gr_b.view(torch.int32)), (method, gr_a.tolist(), gr_b.tolist())
        assert float(gr_a[0]) != float(gr_c[0])              # and the word was not ignored
        _check_grads(gr_a, _oracle(n, "nonpow2_a", False, "finite", method, True, True, SEED, 5 + k), case, method,
                     (method, "offset_dev"))


# ------------------------------------------------------------------------------------------------ autograd node, module
SHAPE = (3, 5, 7, 11)                        # 1155 elements: n % 4 == 3
N4 = 3 * 5 * 7 * 11


def _shaped(flat, layout):
    """A flat (memory-order) CPU tensor as a SHAPE device tensor in `layout`."""
    t = flat.to(DEV)
    if layout == "channels_last":
        n_, c_, h_, w_ = SHAPE
        return t.view(n_, h_, w_, c_).permute(0, 3, 1, 2)
    return t.view(SHAPE)


def _flat(t):
    """The memory-order flat values of a dense 4-D tensor, on the CPU."""
    if t.is_contiguous():
        return t.detach().reshape(-1).cpu()
    assert t.is_contiguous(memory_format=torch.channels_last)
    return t.detach().permute(0, 2, 3, 1).reshape(-1).cpu()


def _module(pset, method):
    import mhaq_amd as M
    q = C.quantizer(pset)
    m = M.NoisyAct(init_s=q.log_s, init_q=q.log_q, signed=q.signed).to(DEV).train()
    with torch.no_grad():
        m.act_b.fill_(q.b)
    m.Q.qnmethod = M.QNMethod[method]
    assert m.act_b.requires_grad == q.signed
    return m


@pytest.mark.parametrize("use_hub", [False, True], ids=["nohub", "hub"])
@pytest.mark.parametrize("family", ["finite", "special"])
@pytest.mark.parametrize("pset", ["unsigned", "nonpow2_a"])
@pytest.mark.parametrize("method", C.METHODS)
def test_forward_fused_equals_the_oracle_chain(method, pset, family, use_hub):
    """NoisyAct.forward_fused on the network's unsigned post-ReLU quantizer and on a non-power-of-two signed one, relu ->
    quantizer (y only) and add -> relu -> quantizer (y and a), both layouts, with and without an ActGradHub."""
    from mhaq_amd import ops
    from mhaq_amd.act_hub import ActGradHub
    signed = C.quantizer(pset).signed
    for with_add in (False, True):
        for layout in ("nchw", "channels_last"):
            case = C.build(N4, pset, with_add, family)
            mod, other = _module(pset, method), _module(pset, method)
            holder = torch.nn.ModuleList([other, mod])
            hub = ActGradHub(holder) if use_hub else None
            z = _shaped(case.z, layout).requires_grad_(True)
            add = _shaped(case.addend, layout).requires_grad_(True) if with_add else None
            ops.manual_seed(SEED)
            if hub is not None:
                hub.begin()
            try:
                assert mod.can_fuse_relu(z, add)
                y, a = mod.forward_fused(z, add)
                assert (a is not None) == with_add
                offset = ops.rng.drawn() + 1             # the stream pre-increments: the k-th draw uses offset k
                outs, gs = [y], [_shaped(case.gy, layout)]
                if with_add:
                    outs.append(a)
                    gs.append(_shaped(case.ga, layout))
                torch.autograd.backward(outs, gs)
            finally:
                if hub is not None:
                    hub.end()
                    for m_ in holder:
                        m_.__dict__.pop("_hub", None)
            torch.cuda.synchronize()
            o = _oracle(N4, pset, with_add, family, method, True, with_add, SEED, offset)
            what = (method, pset, family, use_hub, with_add, layout)
            assert _same_values(_flat(y).numpy(), o["y"].numpy()), ("y", what)
            assert y.stride() == z.stride() and z.grad.stride() == z.stride()
            if with_add:
                assert _same_values(_flat(a).numpy(), o["a"].numpy()), ("a", what)
                _check_gx(_flat(add.grad), o, case, ("addend.grad",) + what)
            _check_gx(_flat(z.grad), o, case, ("z.grad",) + what)
            if not signed:
                assert mod.act_b.grad is None            # the unsigned quantizer's zero point is not learnt
            got = [mod.log_act_s.grad, mod.log_act_q.grad, mod.act_b.grad if signed else o["grads"][2]]
            _check_grads([g.detach().cpu() for g in got], o, case, method, what)


@pytest.mark.parametrize("used", ["y", "a", "both"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("method", C.METHODS)
def test_want_act_backward_of_y_only_a_only_and_both(method, with_add, used):
    """ops.act_relu_layer(want_act=True): z.grad, addend.grad and the parameter gradients when only y, only a, or both
    received a gradient (HAS_GA false / a zero g_y / both).

    a only: the oracle's backward([a], [g_a]) leaves the quantizer's parameters without a gradient, and so must the node
    -- zeros, also where z holds NaN / inf (the quantizer's terms on a zero g_y would be 0 * NaN there), with and
    without an ActGradHub."""
    from mhaq_amd import ops
    for pset, family in (("unsigned", "finite"), ("nonpow2_a", "special"), ("inverted", "finite")):
        case = C.build(N4, pset, with_add, family)
        q = case.q
        z = _shaped(case.z, "nchw").requires_grad_(True)
        add = _shaped(case.addend, "nchw").requires_grad_(True) if with_add else None
        ls, lq, b = (_dev1(v).requires_grad_(True) for v in (q.log_s, q.log_q, q.b))
        ops.manual_seed(SEED)
        y, a = ops.act_relu_layer(z, add, ls, lq, b, C.METHOD_VALUE[method], True)[:2]
        offset = ops.rng.drawn() + 1
        use_gy, use_ga = used in ("y", "both"), used in ("a", "both")
        outs = ([y] if use_gy else []) + ([a] if use_ga else [])
        gs = ([_shaped(case.gy, "nchw")] if use_gy else []) + ([_shaped(case.ga, "nchw")] if use_ga else [])
        torch.autograd.backward(outs, gs)
        torch.cuda.synchronize()
        o = _oracle(N4, pset, with_add, family, method, use_gy, use_ga, SEED, offset)
        what = (method, with_add, used, pset, family)
        assert _same_values(_flat(y).numpy(), o["y"].numpy()) and _same_values(_flat(a).numpy(), o["a"].numpy()), what
        _check_gx(_flat(z.grad), o, case, ("z.grad",) + what, use_gy)
        if with_add:
            _check_gx(_flat(add.grad), o, case, ("addend.grad",) + what, use_gy)
        _check_grads([p.grad.cpu() for p in (ls, lq, b)], o, case, method, what, use_gy)


@pytest.mark.parametrize("method", C.METHODS)
def test_a_only_backward_under_a_hub_gives_the_quantizer_no_gradient(method):
    """forward_fused under an ActGradHub, only a used, z with NaN / inf: the hub's finalize must deliver zeros for this
    quantizer (its partial rows are empty), and z.grad / addend.grad are the oracle's."""
    from mhaq_amd import ops
    from mhaq_amd.act_hub import ActGradHub
    pset = "nonpow2_a"
    case = C.build(N4, pset, True, "special")
    mod, other = _module(pset, method), _module(pset, method)
    holder = torch.nn.ModuleList([other, mod])
    hub = ActGradHub(holder)
    z = _shaped(case.z, "nchw").requires_grad_(True)
    add = _shaped(case.addend, "nchw").requires_grad_(True)
    ops.manual_seed(SEED)
    hub.begin()
    try:
        y, a = mod.forward_fused(z, add)
        a.backward(_shaped(case.ga, "nchw"))
    finally:
        hub.end()
        for m_ in holder:
            m_.__dict__.pop("_hub", None)
    torch.cuda.synchronize()
    o = _oracle(N4, pset, True, "special", method, False, True)
    _check_gx(_flat(z.grad), o, case, ("z.grad", method), use_gy=False)
    _check_gx(_flat(add.grad), o, case, ("addend.grad", method), use_gy=False)
    for p in (mod.log_act_s, mod.log_act_q, mod.act_b):
        assert p.grad is None or float(p.grad) == 0.0, (method, float(p.grad))


@pytest.mark.parametrize("z_layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("method", C.METHODS)
def test_gradients_arriving_in_another_layout_are_re_laid(method, z_layout):
    """z channels_last with g_y / g_a arriving contiguous, and the reverse: like_layout re-lays them, the gradients keep
    z's strides and are the oracle's values."""
    from mhaq_amd import ops
    pset = "nonpow2_a"
    case = C.build(N4, pset, True, "finite")
    q = case.q
    z = _shaped(case.z, z_layout).requires_grad_(True)
    add = _shaped(case.addend, z_layout).requires_grad_(True)
    other = torch.contiguous_format if z_layout == "channels_last" else torch.channels_last
    gy = _shaped(case.gy, z_layout).contiguous(memory_format=other)          # the same logical values, other strides
    ga = _shaped(case.ga, z_layout).contiguous(memory_format=other)
    assert gy.stride() != z.stride() and ga.stride() != z.stride()
    ls, lq, b = (_dev1(v).requires_grad_(True) for v in (q.log_s, q.log_q, q.b))
    ops.manual_seed(SEED)
    y, a = ops.act_relu_layer(z, add, ls, lq, b, C.METHOD_VALUE[method], True)[:2]
    offset = ops.rng.drawn() + 1
    torch.autograd.backward([y, a], [gy, ga])
    torch.cuda.synchronize()
    o = _oracle(N4, pset, True, "finite", method, True, True, SEED, offset)
    assert y.stride() == z.stride() and a.stride() == z.stride()
    assert z.grad.stride() == z.stride() and add.grad.stride() == z.stride()
    _check_gx(_flat(z.grad), o, case, ("z.grad", method, z_layout))
    _check_gx(_flat(add.grad), o, case, ("addend.grad", method, z_layout))
    _check_grads([p.grad.cpu() for p in (ls, lq, b)], o, case, method, (method, z_layout))


@pytest.mark.parametrize("method", C.METHODS)
def test_a_backward_draws_the_next_offset_of_the_seeded_stream(method):
    """The backward after k earlier draws uses (seed, k + 1); ops.fill_r materialises that stream and it is the numpy
    restatement's.  gx does not depend on the signs; the log_act_s gradient of STE / EWGS does, and is the oracle's for
    exactly that offset."""
    from mhaq_amd import ops
    # s = 1/8, q <= 32: the sign term, ~ s / sqrt(12) * |g| * sqrt(n) = 1 in the sum, stands ~90 bars (1e-6 * sum|g q| =
    # 0.011) above the yardstick; at the 2^-9.9 scale of nonpow2_b it would drown in it and the last check could not bite
    pset = "holds_zero"
    case = C.build(N4, pset, False, "finite")
    q = case.q
    results = []
    for seed, burn in ((SEED, 0), (SEED, 2), (99, 0)):
        z = _shaped(case.z, "nchw").requires_grad_(True)
        ls, lq, b = (_dev1(v).requires_grad_(True) for v in (q.log_s, q.log_q, q.b))
        ops.manual_seed(seed)
        for _ in range(burn):
            ops.rng.next()
        y, a = ops.act_relu_layer(z, None, ls, lq, b, C.METHOD_VALUE[method], True)[:2]
        before = ops.rng.drawn()
        assert before == burn
        torch.autograd.backward([y, a], [_shaped(case.gy, "nchw"), _shaped(case.ga, "nchw")])
        torch.cuda.synchronize()
        assert ops.rng.drawn() - before == (0 if method == "LSQ" else 1)
        offset = before + 1
        r8 = ops.fill_r(N4, seed, offset, DEV).cpu()
        o = _oracle(N4, pset, False, "finite", method, True, True, seed, offset)
        assert torch.equal(r8.float() * 0.5, o["r"])
        _check_gx(_flat(z.grad), o, case, (method, seed, burn))
        _check_grads([p.grad.cpu() for p in (ls, lq, b)], o, case, method, (method, seed, burn))
        results.append((_flat(z.grad), float(ls.grad), o))
    for gx, _, _ in results[1:]:
        assert torch.equal(gx.view(torch.int32), results[0][0].view(torch.int32))      # gx: no sign in it
    if method != "LSQ":
        bar = C.yardsticks(case, results[0][2]["a"], results[0][2]["r"], method)[0]
        for _, g_s, _ in results[1:]:
            assert abs(g_s - results[0][1]) > 10 * bar        # another offset / seed is another gradient: the check bites
