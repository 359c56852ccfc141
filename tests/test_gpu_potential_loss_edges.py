"""GPU (-m gpu): the PotentialLoss kernels (mhaq_fq_potential_loss_fwd / _bwd, csrc/fq_pc.hip) at unequal bit widths, at the
edges of the forward's four-loads-in-flight loop and of the backward's 64-block grid, at the corners of the active sets and
under inf / NaN -- through the C ABI (every output poisoned between bands of ones) and through ops.potential_loss /
FusedPotentialLossNoPred (autograd through the compiled node).  The yardstick is tests/potential_ref.ref64, the bar the
framework's own float32 chain on the device, never the kernel:
    |v - v64| <= 4 |v_torch32 - v64| + 8 ulp32(v64) per scalar,   max|g - g64| <= 4 max|g_torch32 - g64| + 8 2^-24 max|g64|.
Exact: out[11] (one float32 subtraction), out[6] for p = 1, cnt, g_lws = -g_lwq bit for bit, the zero gradients of inactive
hinges, the halves at ties.  Every case is at most 16641 + 3 floats per vector pair."""
import ctypes
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import potential_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 64                                  # elements of ones planted before and after every output
POISON = -7.0
G_UP = 0.375                               # a non-trivial upstream gradient
f32 = lambda v: float(np.float32(v))       # noqa: E731
BASE = f32(1.7)
STATE = (f32(3.3), 3.0, f32(0.35))
FAMILY = ["ploss", "hinge mean", "hinge mean", "rloss", "multiplier", "multiplier", "multiplier", "mean", "mean", "mean",
          "mean", "max"]
SHARES = {}                                # largest error / bar per output family over the module's tests


@pytest.fixture(scope="module", autouse=True)
def _report_shares():
    yield
    print("\nbar shares, largest per output family:", {k: round(v, 4) for k, v in sorted(SHARES.items())})


def _share(family, s):
    SHARES[family] = max(SHARES.get(family, 0.0), s)
    return s


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().contiguous().reshape(-1).cpu().view(torch.int32)


class Banded:
    """n poisoned float32 elements between two bands of ones."""

    def __init__(self, n):
        self.buf = torch.ones(BAND + n + BAND, dtype=torch.float32, device=DEV)
        self.n = n
        self.view = self.buf[BAND:BAND + n]
        self.view.fill_(POISON)

    def intact(self):
        return bool((self.buf[:BAND] == 1).all()) and bool((self.buf[BAND + self.n:] == 1).all())

    def written(self):
        return bool((self.view != POISON).all())


def capi(base, vecs, a_bits, w_bits, state, p=1, lossless=False, update=0, g=G_UP, backward=True):
    """Both launches through the C ABI -> out [12], state [3] and the gradients, on the CPU.  Asserts that every output element
    was written, that nothing around an output was, and that the state keeps its bits when update == 0."""
    from mhaq_amd import _lib
    lib = _lib.lib()
    las, laq, lws, lwq = vecs
    na, nw = las.numel(), lws.numel()
    b = torch.tensor([base], dtype=torch.float32, device=DEV)
    out, st = Banded(12), Banded(3)
    st.view.copy_(torch.as_tensor(state, dtype=torch.float32))
    before = _bits(st.view)
    _lib.check(lib.mhaq_fq_potential_loss_fwd(_ptr(b), _ptr(las), _ptr(laq), na, _ptr(lws), _ptr(lwq), nw, float(a_bits),
                                              float(w_bits), float(p), int(lossless), _ptr(st.view), int(update),
                                              _ptr(out.view), _stream()), "mhaq_fq_potential_loss_fwd")
    torch.cuda.synchronize()
    assert out.intact() and st.intact() and out.written()
    if not update:
        assert torch.equal(_bits(st.view), before)
    res = SimpleNamespace(out=out.view.cpu(), state=st.view.cpu())
    if backward:
        gb, outs = Banded(1), [Banded(na), Banded(na), Banded(nw), Banded(nw)]
        gdev = torch.tensor([g], dtype=torch.float32, device=DEV)
        _lib.check(lib.mhaq_fq_potential_loss_bwd(_ptr(gdev), _ptr(out.view), _ptr(las), _ptr(laq), na, _ptr(lws), _ptr(lwq),
                                                  nw, float(a_bits), float(w_bits), float(p), _ptr(gb.view),
                                                  *[_ptr(o.view) for o in outs], _stream()), "mhaq_fq_potential_loss_bwd")
        torch.cuda.synchronize()
        assert gb.intact() and gb.written() and all(o.intact() and o.written() for o in outs)
        assert out.intact() and torch.equal(_bits(out.view), _bits(res.out))         # the backward only reads `out`
        res.g_base = float(gb.view.cpu())
        res.g_las, res.g_laq, res.g_lws, res.g_lwq = (o.view.cpu() for o in outs)
    return res


def node(base, vecs, a_bits, w_bits, state, p=1, lossless=False, update=False, g=G_UP):
    """ops.potential_loss with autograd through the compiled node."""
    from mhaq_amd import ops
    leaves = [v.clone().requires_grad_(True) for v in vecs]
    b = torch.tensor(base, dtype=torch.float32, device=DEV, requires_grad=True)
    st = torch.tensor(state, dtype=torch.float32, device=DEV)
    ploss, stats = ops.potential_loss(b * 1.0, *leaves, st, a_bits, w_bits, p=p, lossless=lossless, update_state=update)
    (ploss * g).backward()
    assert torch.equal(_bits(ploss), _bits(stats[0]))
    return SimpleNamespace(out=stats.cpu(), state=st.cpu(), g_base=float(b.grad),
                           **{n: leaf.grad.cpu() for n, leaf in zip(R.GRAD_NAMES, leaves)})


def module(base, vecs, a_bits, w_bits, state, p=1, lossless=False, update=False, g=G_UP):
    """FusedPotentialLossNoPred in training (update) or evaluation mode -> the same fields, and the module."""
    from mhaq_amd.loss import FusedPotentialLossNoPred
    L = FusedPotentialLossNoPred(None, p=p, a=a_bits, w=w_bits, lossless=lossless).to(DEV).train(bool(update))
    L.loss_sum, L.cnt, L.t = state
    leaves = [v.clone().requires_grad_(True) for v in vecs]
    b = torch.tensor(base, dtype=torch.float32, device=DEV, requires_grad=True)
    ploss = L((b * 1.0, *leaves))
    (ploss * g).backward()
    assert torch.equal(_bits(ploss), _bits(L._stats[0]))
    return SimpleNamespace(out=L._stats.cpu(), state=L._state.cpu(), g_base=float(b.grad), module=L,
                           **{n: leaf.grad.cpu() for n, leaf in zip(R.GRAD_NAMES, leaves)})


def refs(base, vecs, a_bits, w_bits, state, p=1, lossless=False, g=G_UP):
    """-> (ref64 on the CPU, the framework's float32 chain on the device)."""
    cpu = [v.cpu() for v in vecs]
    return (R.ref64(base, *cpu, a_bits, w_bits, state, p, lossless, g),
            R.chain32(base, *vecs, a_bits, w_bits, state, p, lossless, g))


def check_out(tag, got, ref, c32, p):
    """All twelve outputs against ref64: out[11] exact, out[6] exact for p == 1, the rest within the bar."""
    shares = {}
    for k in range(12):
        v, want = float(got.out[k]), ref.out[k]
        what = (tag, R.OUT_NAMES[k], v, c32.out[k], want)
        if k == 11 or (k == 6 and p == 1):
            assert (math.isnan(v) and math.isnan(want)) or v == want, what
            continue
        ok, s = R.scalar_share(v, c32.out[k], want)
        assert ok, what + (s,)
        shares[FAMILY[k]] = max(shares.get(FAMILY[k], 0.0), _share(FAMILY[k], s))
    return shares


def check_grads(tag, got, ref, c32):
    shares = {}
    for n in R.GRAD_NAMES:
        ok, s = R.grad_share(getattr(got, n), getattr(c32, n), getattr(ref, n))
        assert ok, (tag, n, s)
        shares["gradient"] = max(shares.get("gradient", 0.0), _share("gradient", s))
    ok, s = R.scalar_share(got.g_base, c32.g_base, ref.g_base)
    assert ok, (tag, "g_base", got.g_base, c32.g_base, ref.g_base, s)
    shares["g_base"] = _share("g_base", s)
    assert torch.equal(_bits(got.g_lws), _bits(-got.g_lwq)) and torch.equal(_bits(got.g_las), _bits(-got.g_laq)), tag
    return shares


def check(tag, got, ref, c32, p=1):
    shares = check_out(tag, got, ref, c32, p)
    shares.update(check_grads(tag, got, ref, c32))
    print("bar shares", tag, {k: round(v, 4) for k, v in shares.items()})


@functools.lru_cache(maxsize=None)
def _inputs(na, nw, a_bits, w_bits, seed=0, a_shift=0.0, w_shift=0.0):
    """Grid inputs on the device, shared and never modified."""
    return tuple(v.to(DEV) for v in R.make_inputs(na, nw, a_bits, w_bits, 1000 * na + nw + seed, a_shift=a_shift,
                                                  w_shift=w_shift))


def _changed(vecs, which, idx, value):
    out = list(vecs)
    out[which] = vecs[which].clone()
    out[which][idx] = value
    return tuple(out)


# ---------------------------------------------------------------------------------------------- unequal bit widths
@pytest.mark.parametrize("na,nw", [(21, 300), (300, 21)])
@pytest.mark.parametrize("a_bits,w_bits", [(8, 4), (3, 6)])
def test_unequal_bit_widths_through_the_c_abi_the_node_and_the_module(a_bits, w_bits, na, nw):
    """Each side's inputs are centred on its own threshold, so a swap of at and wt anywhere -- forward kernel, backward kernel,
    the node's argument order, ops.potential_loss -- leaves one side all active and the other all inactive."""
    vecs = _inputs(na, nw, a_bits, w_bits)
    ref, c32 = refs(BASE, vecs, a_bits, w_bits, STATE)
    assert 0 < ref.wact < nw and 0 < ref.aact < na
    got = capi(BASE, vecs, a_bits, w_bits, STATE)
    check(("capi", a_bits, w_bits, na, nw), got, ref, c32)
    # the case does not degenerate: the swapped widths give another loss and other gradients, in the yardstick and in the kernel
    swapped, ref_sw = capi(BASE, vecs, w_bits, a_bits, STATE), R.ref64(BASE, *[v.cpu() for v in vecs], w_bits, a_bits, STATE,
                                                                       g=G_UP)
    for r in (got, ref):
        o = swapped if r is got else ref_sw
        assert float(r.out[0]) != float(o.out[0])
        assert not torch.equal(r.g_lwq, o.g_lwq) and not torch.equal(r.g_laq, o.g_laq)
        assert not torch.equal(r.g_lws, o.g_lws) and not torch.equal(r.g_las, o.g_las)
    check(("ops", a_bits, w_bits, na, nw), node(BASE, vecs, a_bits, w_bits, STATE), ref, c32)
    m = module(BASE, vecs, a_bits, w_bits, STATE, update=True)
    check(("module", a_bits, w_bits, na, nw), m, ref, c32)
    assert m.module.at == a_bits and m.module.wt == w_bits and m.module.cnt == 4


# ---------------------------------------------------------------------------------------------- all twelve outputs
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("lossless", [False, True])
def test_all_twelve_outputs_and_the_modules_attribute_views(p, lossless):
    vecs = _inputs(21, 300, 8, 4)
    ref, c32 = refs(BASE, vecs, 8, 4, STATE, p, lossless)
    got = capi(BASE, vecs, 8, 4, STATE, p, lossless)
    check(("capi", p, lossless), got, ref, c32, p)
    m = module(BASE, vecs, 8, 4, STATE, p, lossless)
    check(("module", p, lossless), m, ref, c32, p)
    views = dict(wloss=1, aloss=2, rloss=3, s_weight_loss=7, q_weight_loss=8, s_act_loss=9, q_act_loss=10, weight_reg_loss=11)
    for name, k in views.items():
        assert torch.equal(_bits(getattr(m.module, name)), _bits(m.out[k])), name
    assert torch.equal(_bits(m.state), _bits(torch.tensor(STATE)))                  # evaluation mode: the state is left alone


# ---------------------------------------------------------------------------------------------- loop edges
EDGE_SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 2049]     # one thread's four loads are i0, i0 + 256, i0 + 512, i0 + 768


def _positions(n):
    """First, last, the first lane of the last partial trip -- and the same lane of each other wave (threads 64, 128, 192) in that
    wave's last trip, so that every slot of thread 0's fold over the four wave maxima decides the result once."""
    waves = {64 * w + 256 * ((n - 1 - 64 * w) // 256) for w in (1, 2, 3) if n > 64 * w}
    return sorted({0, n - 1, 256 * ((n - 1) // 256)} | waves)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_forward_loop_edges_weight_side(n):
    """The maximum of lwq - lws planted first, last, in the first lane of the last partial trip and in the first lane of every
    other wave: in a clamped trip, in each of the four waves, beside 256 and 1024 where a thread's second load / second pass
    begins.  It is also that side's largest hinge."""
    base = _inputs(3, n, 8, 4)
    for pos in _positions(n):
        vecs = _changed(_changed(base, 2, pos, -8.0), 3, pos, 15.0)
        ref, c32 = refs(BASE, vecs, 8, 4, STATE)
        assert ref.out[11] == 23.0 and int(torch.argmax(vecs[3] - vecs[2])) == pos
        check(("edge w", n, pos), capi(BASE, vecs, 8, 4, STATE), ref, c32)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_forward_loop_edges_activation_side(n):
    """The same eight sizes for na with nw = 3; the planted element is the activation side's largest hinge by far, so a trip that
    drops it or counts it twice moves aloss and the two means out of the bar."""
    base = _inputs(n, 3, 8, 4)
    for pos in _positions(n):
        vecs = _changed(_changed(base, 0, pos, -8.0), 1, pos, 15.0)
        ref, c32 = refs(BASE, vecs, 8, 4, STATE)
        check(("edge a", n, pos), capi(BASE, vecs, 8, 4, STATE), ref, c32)


# ---------------------------------------------------------------------------------------------- backward past its grid cap
@pytest.mark.parametrize("na,nw", [(3, 16641), (16641, 3)])
@pytest.mark.parametrize("p", [1, 2])
def test_backward_second_trip_of_the_grid_stride_loop(p, na, nw):
    """64 blocks x 256 threads = 16384: elements 16384 .. 16640 are the second trip, active, inactive and tied among them."""
    a_bits, w_bits = 8, 4
    las, laq, lws, lwq = (v.clone() for v in _inputs(na, nw, a_bits, w_bits))
    if nw > na:
        R.plant_tie(lws, lwq, w_bits, slice(16385, None, 7))
        h_tail = R.ref64(BASE, las.cpu(), laq.cpu(), lws.cpu(), lwq.cpu(), a_bits, w_bits, STATE, p).wh[16384:]
    else:
        R.plant_tie(las, laq, a_bits, slice(16385, None, 7))
        h_tail = R.ref64(BASE, las.cpu(), laq.cpu(), lws.cpu(), lwq.cpu(), a_bits, w_bits, STATE, p).ah[16384:]
    assert h_tail.numel() == 257 and bool((h_tail > 0).any()) and bool((h_tail < 0).any()) and bool((h_tail == 0).any())
    vecs = (las, laq, lws, lwq)
    ref, c32 = refs(BASE, vecs, a_bits, w_bits, STATE, p)
    check(("cap capi", p, na, nw), capi(BASE, vecs, a_bits, w_bits, STATE, p), ref, c32, p)      # every element written: capi()
    check(("cap ops", p, na, nw), node(BASE, vecs, a_bits, w_bits, STATE, p), ref, c32, p)


# ---------------------------------------------------------------------------------------------- active-set corners
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("a_shift,w_shift", [(-12.0, -12.0), (-12.0, 0.0), (0.0, -12.0), (12.0, 12.0)],
                         ids=["none", "weights only", "activations only", "all"])
def test_active_set_corners(a_shift, w_shift, p):
    na, nw = 21, 300
    vecs = _inputs(na, nw, 8, 4, a_shift=a_shift, w_shift=w_shift)
    ref, c32 = refs(BASE, vecs, 8, 4, STATE, p)
    want = {-12.0: lambda c, n: c == 0, 0.0: lambda c, n: 0 < c < n, 12.0: lambda c, n: c == n}
    assert want[a_shift](ref.aact, na) and want[w_shift](ref.wact, nw)
    got = capi(BASE, vecs, 8, 4, STATE, p)
    check(("corner", a_shift, w_shift, p), got, ref, c32, p)
    if a_shift < 0:
        assert bool((got.g_las == 0).all()) and bool((got.g_laq == 0).all()) and float(got.out[2]) == 0.0
    if w_shift < 0:
        assert bool((got.g_lws == 0).all()) and bool((got.g_lwq == 0).all()) and float(got.out[1]) == 0.0
    if a_shift < 0 and w_shift < 0:                 # wmul = amul = 1e-3 / 1e-3, both means zero: ploss == l2 * rloss
        ok, s = R.scalar_share(got.out[0], c32.out[3], ref.out[3])
        assert ok and ref.out[0] == ref.out[3], (float(got.out[0]), ref.out[3], s)


@pytest.mark.parametrize("p", [1, 2])
def test_planted_ties_on_both_sides(p):
    """h == 0 exactly: torch.max splits the gradient, so for p = 1 a tie gets exactly half of an active neighbour's g * cw; for
    p = 2 the factor p h^(p-1) is zero."""
    las, laq, lws, lwq = (v.clone() for v in _inputs(21, 300, 8, 4))
    R.plant_tie(lws, lwq, 4, slice(1, None, 5))
    R.plant_tie(las, laq, 8, slice(2, None, 4))
    vecs = (las, laq, lws, lwq)
    ref, c32 = refs(BASE, vecs, 8, 4, STATE, p)
    got = capi(BASE, vecs, 8, 4, STATE, p)
    check(("ties", p), got, ref, c32, p)
    for g_q, h in ((got.g_lwq, ref.wh), (got.g_laq, ref.ah)):
        tie, active = h == 0, h > 0
        assert int(tie.sum()) >= 5 and bool(active.any()) and bool((h < 0).any())
        if p == 1:
            full = g_q[active]
            assert bool((full == full[0]).all()) and float(full[0]) != 0
            assert bool((g_q[tie] == 0.5 * full[0]).all())
        else:
            assert bool((g_q[tie] == 0).all())
        assert bool((g_q[h < 0] == 0).all())


# ---------------------------------------------------------------------------------------------- state
@pytest.mark.parametrize("p", [1, 2])
def test_five_consecutive_training_steps_carry_the_state(p):
    """calib is read before the update.  cnt exact; loss_sum and ploss within the bar of the float32 chain carrying its own
    float32 sum the same way."""
    vecs = _inputs(21, 300, 8, 4)
    cpu = [v.cpu() for v in vecs]
    t = f32(0.35)
    s_dev, s64, s32 = (0.0, 1.0, t), (0.0, 1.0, t), (torch.tensor(0.0), 1.0, t)
    for k, b in enumerate(f32(v) for v in (1.7, 0.9, 2.25, 0.31, 1.1)):
        ref = R.ref64(b, *cpu, 8, 4, s64, p, False, G_UP)
        c32 = R.chain32(b, *vecs, 8, 4, s32, p, False, G_UP)
        got = capi(b, vecs, 8, 4, s_dev, p, update=1)
        check(("state", p, k), got, ref, c32, p)
        assert float(got.state[1]) == k + 2 and float(got.state[2]) == t
        ok, s = R.scalar_share(got.state[0], c32.state[0], ref.state[0])
        assert ok, (k, float(got.state[0]), float(c32.state[0]), ref.state[0], s)
        _share("loss_sum", s)
        s_dev, s64, s32 = tuple(float(v) for v in got.state), ref.state, c32.state


# ---------------------------------------------------------------------------------------------- upstream gradient
def test_upstream_gradient_scales_every_gradient():
    """g = 0.375 through the C ABI and (out * 0.375).backward() through the node (every test above runs with it); here against
    g = 1: g_base == g * out[6] within the bar and the vectors scale with g."""
    vecs = _inputs(21, 300, 8, 4)
    for g in (G_UP, 1.0):
        ref, c32 = refs(BASE, vecs, 8, 4, STATE, 2, True, g)
        got, via = capi(BASE, vecs, 8, 4, STATE, 2, True, g=g), node(BASE, vecs, 8, 4, STATE, 2, True, g=g)
        check(("g capi", g), got, ref, c32, 2)
        check(("g ops", g), via, ref, c32, 2)
        ok, s = R.scalar_share(got.g_base, c32.g_base, g * ref.out[6])
        assert ok and ref.g_base == g * ref.out[6], (got.g_base, g * ref.out[6], s)


# ---------------------------------------------------------------------------------------------- inf and NaN
def _check_special(tag, got, ref, c32, p=1):
    """Where the yardstick is NaN or infinite the output is the same special value, elsewhere it is within the bar."""
    for k in range(12):
        v, want = float(got.out[k]), ref.out[k]
        if k in (4, 5):
            continue                 # the multipliers follow the counts alone: checked in the clean runs
        if math.isnan(want):
            assert math.isnan(v), (tag, R.OUT_NAMES[k], v)
        elif math.isinf(want) or k == 11:
            assert v == want, (tag, R.OUT_NAMES[k], v, want)
        else:
            ok, s = R.scalar_share(v, c32.out[k], want)
            assert ok, (tag, R.OUT_NAMES[k], v, c32.out[k], want, s)


def test_infinity_as_the_reference():
    base = _inputs(21, 300, 8, 4)
    i = 150
    vecs = _changed(base, 3, i, math.inf)                                     # lwq[i] = +inf: ploss = +inf, max = +inf
    ref, c32 = refs(BASE, vecs, 8, 4, STATE)
    assert ref.out[0] == math.inf and ref.out[11] == math.inf and ref.out[1] == math.inf and ref.out[8] == math.inf
    got = capi(BASE, vecs, 8, 4, STATE)
    _check_special(("lwq inf",), got, ref, c32)
    assert float(got.out[0]) == math.inf and float(got.out[11]) == math.inf
    vecs = _changed(vecs, 2, i, math.inf)                                     # lws[i] = lwq[i] = +inf: inf - inf = NaN
    ref, c32 = refs(BASE, vecs, 8, 4, STATE)
    assert math.isnan(ref.out[0]) and math.isnan(ref.out[11]) and math.isnan(c32.out[0]) and math.isnan(c32.out[11])
    got = capi(BASE, vecs, 8, 4, STATE)
    _check_special(("lws lwq inf",), got, ref, c32)
    assert math.isnan(float(got.out[0])) and math.isnan(float(got.out[11])) and math.isnan(float(got.out[1]))


@pytest.mark.parametrize("na,nw", [(21, 300), (3, 1025), (1025, 3)])
@pytest.mark.parametrize("which", range(4), ids=["las", "laq", "lws", "lwq"])
def test_nan_propagates_as_the_references(which, na, nw):
    """No NaN screening, plain IEEE: the reference's torch.max(0, h), .mean() and (lwq - lws).max() hand a NaN on.  One NaN in
    the middle of a vector -- at 1025 elements the middle, 512, is a thread's third load of a pass whose fourth is clamped --
    makes ploss, that side's mean hinge, that vector's mean and, for lws / lwq, max(lwq - lws) NaN.  The other side's mean
    hinge and means keep the bits of the run without the NaN.  The backward runs, writes every element and nothing else (capi());
    its values under NaN are not pinned."""
    base = _inputs(na, nw, 8, 4)
    clean = capi(BASE, base, 8, 4, STATE)
    vecs = _changed(base, which, base[which].numel() // 2, math.nan)
    ref, c32 = refs(BASE, vecs, 8, 4, STATE)
    assert math.isnan(c32.out[0]) and math.isnan(ref.out[0])                 # the framework's own float32 chain says NaN
    weight_side = which >= 2
    own_mean = {0: 9, 1: 10, 2: 7, 3: 8}[which]
    nan_out = {0, 1 if weight_side else 2, own_mean} | ({11} if weight_side else set())
    assert {k for k in range(12) if math.isnan(ref.out[k])} == nan_out
    for face in (capi, node):
        got = face(BASE, vecs, 8, 4, STATE)
        for k in sorted(nan_out):
            assert math.isnan(float(got.out[k])), (face.__name__, R.OUT_NAMES[k], float(got.out[k]))
        other = [2, 9, 10] if weight_side else [1, 7, 8, 11]
        for k in other + [3, 6]:
            assert torch.equal(_bits(got.out[k]), _bits(clean.out[k])), (face.__name__, R.OUT_NAMES[k])
        _check_special(("nan", which, na, nw, face.__name__), got, ref, c32)
