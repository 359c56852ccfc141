"""GPU (-m gpu): the ReLU / residual-add forms of the 16-bit NoisyAct kernels (mhaq_fq_act_relu_*_x16, NoisyAct.forward_fused
under torch.autocast) against today's composition -- torch's 16-bit add / relu + the 16-bit NoisyAct op + autograd.  The
contract (include/mhaq_fq.h) is the BITS of that composition, the double rounding of the accumulated gradient included,
so everything is compared for equality: y, a and the input gradients value for value with NaNs at the same positions, the
three parameter gradients bit for bit (with and without an ActGradHub), and -- at the C ABI -- the partial rows.

Kernel forms as in tests/test_gpu_fused_act.py: one partial row per block from 20 Mi elements, one per wave below, the
element kernel for pointers off a 16-byte boundary and for n < 8.  Where the fused backward reads an unaligned z (the form
without a), the reference quantizer is fed an equally misaligned copy of a, so that both sides sum in the element kernel's
order.

Inputs: the fp32 test's planted zeros, -0.0, exact cancellations, values below / inside / above the range; pairs whose sum
needs rounding to 16 bits; in the `special` family NaN and +-inf in z and in both gradients (the parameter gradients are
then NaN on both sides, so the `finite` family carries their comparison); and g_a values built from the fp32 gradient p of
their element so that R(R(p) + g_a) != R(p + g_a) (tests/fused_act16_contract.plant_double_rounding).  The scale is not
a power of two: with one, the STE / LSQ gradient inside the range is g_y itself, a 16-bit number, and nothing is ever
rounded twice.  For the same reason the n = 5 case can hold such an element only with EWGS."""
import ctypes

import pytest
import torch

from tests import fused_act16_contract as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
FORMS = ("relu_fq", "add_relu_fq_a", "relu_fq_a")
SHAPES = {
    "big": (40, 64, 96, 96),       # 23.6 M elements >= 20 Mi: one partial row per block
    "mid": (8, 64, 14, 14),        # 100 352 elements: 49 blocks, one partial row per wave
    "ragged": (3, 5, 7, 11),       # 1155 elements, n % 8 == 3
    "tiny": (1, 1, 1, 5),          # n < 8: the element kernel
    "unaligned": (6, 16, 9, 13),   # a view 2 bytes into its buffer: the element kernel
}
LOG_S, LOG_Q = -3.17, 2.0           # s = 0.1111..., qr = 4: [b, b + 4 - s]
# (dtype, size): the 23.6 M-element case runs in one dtype
DT_SIZES = [(dt, size) for dt in DTYPES for size in SHAPES if size != "big" or dt == "bf16"]


def _flat(t, layout):
    """A flat alias of t in memory order."""
    f = t.permute(0, 2, 3, 1).reshape(-1) if layout == "channels_last" else t.reshape(-1)
    assert f.data_ptr() == t.data_ptr()
    return f


def _tensor(shape, layout, gen, dtype, unaligned=False, scale=3.0):
    """A dense 16-bit tensor of `shape` in `layout` memory order; `unaligned`: a view one element into a larger buffer."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.empty(n + 8, device=DEV, dtype=dtype)
    flat = buf[1:n + 1] if unaligned else buf[:n]
    flat.copy_(torch.randn(n, device=DEV, generator=gen) * scale)
    if layout == "channels_last":
        N, C, H, W = shape
        return flat.view(N, H, W, C).permute(0, 3, 1, 2)
    return flat.view(shape)


def _misaligned_copy(t):
    """The values of t in t's own strides, 2 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, device=t.device, dtype=t.dtype)
    out = buf[1:t.numel() + 1].as_strided(t.shape, t.stride())
    out.copy_(t)
    assert out.data_ptr() % 16 == 2
    return out


def _quantizer(method, b):
    import mhaq_amd as M
    q = M.NoisyAct(init_s=-3, init_q=2, signed=True).to(DEV).train()
    with torch.no_grad():
        q.log_act_s.fill_(LOG_S)
        q.log_act_q.fill_(LOG_Q)
        q.act_b.fill_(b)
    q.Q.qnmethod = method
    return q


def _fp32_gradient(q, a, gy):
    """p = the fp32 gx of the quantizer on (up(a), up(g_y)) -- what the 16-bit backward rounds (it does not depend on the
    random signs)."""
    from mhaq_amd import ops
    ops.manual_seed(1)
    a32 = a.float().requires_grad_(True)
    q(a32).backward(gy.float())
    for p in q.parameters():
        p.grad = None
    return a32.grad


def _inputs(q, shape, layout, dtype, unaligned, with_add, b, special):
    gen = torch.Generator(device=DEV).manual_seed(1234)
    z = _tensor(shape, layout, gen, dtype, unaligned)
    add = _tensor(shape, layout, gen, dtype, unaligned) if with_add else None
    gy = _tensor(shape, layout, gen, dtype, scale=1.0)
    ga = _tensor(shape, layout, gen, dtype, scale=1.0)
    zf, gyf, gaf = _flat(z, layout), _flat(gy, layout), _flat(ga, layout)
    n = zf.numel()
    nan, inf = float("nan"), float("inf")
    zf[0::7] = 0.0
    zf[1::11] = -0.0
    zf[2::13] = b - 0.5                              # below the clamp range
    zf[3::17] = b + 0.25                             # inside it
    zf[4::19] = 50.0                                 # above it
    if n < 8:
        zf[3] = 0.625                                # positive and inside the range for every b used here
    if with_add:
        af = _flat(add, layout)
        af[0::7] = 0.0                               # 0 + 0
        af[5::23] = -zf[5::23]                       # exact cancellation: z + addend == 0
        af[2::13] = 0.0
        af[3::17] = 0.0
        af[4::19] = 0.0
        zf[6::29] = 1.0                              # 1 + half a unit in the last place: the sum is a tie
        af[6::29] = 2.0 ** -(K.MANTISSA_BITS[dtype] + 1)
    if special:
        zf[8::31] = nan
        zf[9::37] = inf
        zf[10::41] = -inf
        gyf[11::43] = nan
        gyf[12::47] = inf
        gyf[13::53] = -inf
        gaf[14::59] = nan
        gaf[15::61] = inf
        gaf[16::67] = -inf
        if with_add:
            af[9::74] = -inf                         # inf + (-inf)
    # g_a at which the second rounding of gs changes the result, on every third element that admits one
    a = torch.relu(z + add if add is not None else z)
    p = _fp32_gradient(q, a, gy)
    plant, ok = K.plant_double_rounding(p, dtype)
    idx = torch.empty_like(ga, dtype=torch.int64)    # the flat index of every element, in ga's memory order
    _flat(idx, layout).copy_(torch.arange(n, device=DEV))
    ga.copy_(torch.where(ok & (idx % 3 == 0), plant, ga))
    single = (p + ga.float()).to(dtype)
    double = (p.to(dtype).float() + ga.float()).to(dtype)
    twice = int(((single != double) & ~(torch.isnan(single) & torch.isnan(double)) & (a > 0)).sum())
    return z, add, gy, ga, twice


def _run(q, hub, fused, form, dtype, z0, add0, gy, ga, seed, use=("y", "a")):
    from mhaq_amd import ops
    ops.manual_seed(seed)                            # the same (seed, offset) for both sides
    for p in q.parameters():
        p.grad = None
    z = z0.detach().requires_grad_(True)
    add = add0.detach().requires_grad_(True) if add0 is not None else None
    want_a = form != "relu_fq"

    def backward(y, a):
        outs, gs = [], []
        if "y" in use:
            outs.append(y); gs.append(gy)
        if want_a and "a" in use:
            outs.append(a); gs.append(ga)
        torch.autograd.backward(outs, gs)

    if hub is not None:
        hub.begin()
    try:
        with torch.autocast("cuda", dtype=dtype):
            if fused:
                assert q.can_fuse_relu(z, add)
                y, a = q.forward_fused(z, add, want_act=want_a)
                assert (a is not None) == want_a
                backward(y, a)
            else:
                a = torch.relu(torch.add(z, add) if add is not None else z)
                assert a.dtype == dtype
                if not want_a and z.data_ptr() % 16 != 0:
                    # (module docstring) the reference quantizer on a misaligned copy of a: the element kernel on both sides
                    a_u = _misaligned_copy(a.detach()).requires_grad_(True)
                    y = q(a_u)
                    y.backward(gy)
                    a.backward(a_u.grad)
                else:
                    y = q(a)
                    backward(y, a)
    finally:
        if hub is not None:
            hub.end()
    torch.cuda.synchronize()
    grads = [p.grad.detach().clone() if p.grad is not None else None for p in (q.log_act_s, q.log_act_q, q.act_b)]
    return (y.detach(), a.detach() if want_a else None, z.grad, add.grad if add is not None else None, grads)


def _same(a, b):
    """Equal values, NaNs at the same positions, same dtype."""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _assert_run_equal(got, ref, what):
    assert _same(got[0], ref[0]), ("y", what)
    if ref[1] is not None:
        assert _same(got[1], ref[1]), ("a", what)
    assert _same(got[2], ref[2]), ("gx", what)
    if ref[3] is not None:
        assert _same(got[3], ref[3]), ("g_addend", what)
    for name, g_f, g_r in zip(("log_act_s", "log_act_q", "act_b"), got[4], ref[4]):
        assert (g_f is None) == (g_r is None), (name, what)
        if g_f is not None:
            assert g_f.shape == g_r.shape and g_f.dtype == torch.float32
            assert torch.equal(g_f.view(torch.int32), g_r.view(torch.int32)), (name, what, float(g_f), float(g_r))


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("method", ["STE", "LSQ", "EWGS"])
@pytest.mark.parametrize("dt,size", DT_SIZES)
def test_fused_forms_equal_todays_composition(dt, size, method, layout):
    import mhaq_amd as M
    from mhaq_amd.act_hub import ActGradHub
    dtype = DTYPES[dt]
    shape, unaligned = SHAPES[size], size == "unaligned"
    for b in (0.25, -1.0):                           # a range above zero (zeros clip to lo) and one that holds zero
        if size == "big" and b != 0.25:
            continue                                 # (one pass over the 23.6 M-element case)
        q = _quantizer(M.QNMethod[method], b)
        other = _quantizer(M.QNMethod[method], b)    # a second quantizer: the hub finalizes several in one launch
        holder = torch.nn.ModuleList([other, q])
        for form in FORMS:
            for special in (False, True):
                z, add, gy, ga, twice = _inputs(q, shape, layout, dtype, unaligned, form == "add_relu_fq_a", b, special)
                assert (z.data_ptr() % 16 != 0) == unaligned
                n = z.numel()
                if form != "relu_fq" and (n >= 8 or method == "EWGS"):
                    assert twice > 0, (dt, method, layout, size, b, form, special)      # the second rounding matters
                for use_hub in (False, True):
                    hub = ActGradHub(holder) if use_hub else None
                    ref = _run(q, hub, False, form, dtype, z, add, gy, ga, seed=77)
                    got = _run(q, hub, True, form, dtype, z, add, gy, ga, seed=77)
                    if hub is not None:
                        for m in holder:
                            m.__dict__.pop("_hub", None)
                    what = (dt, method, layout, size, b, form, special, use_hub)
                    _assert_run_equal(got, ref, what)
                    if ref[1] is not None:
                        assert got[1].stride() == z.stride()
                    if not special:
                        assert all(bool(torch.isfinite(g)) for g in ref[4]), what
                # the zeros, the negatives, the clipped values and the rounded sums are really there
                zf32 = z.float()
                a_all = torch.relu(z + add if add is not None else z)
                assert bool((a_all == 0).any()) and bool((zf32 < b - 0.25).any()) and bool((a_all > b + 3.9).any())
                if add is not None and n > 100:
                    assert bool(((zf32 + add.float()) != (z + add).float()).any())
                if special and n > 100:
                    assert bool(torch.isnan(zf32).any()) and bool(torch.isinf(gy.float()).any())
                    assert bool(torch.isnan(ga.float()).any())
                del z, add, gy, ga
        torch.cuda.empty_cache()


@pytest.mark.parametrize("use", [("y",), ("a",), ("y", "a")])
@pytest.mark.parametrize("method", ["STE", "LSQ", "EWGS"])
def test_only_y_only_a_or_both_used(method, use):
    """Whichever outputs receive a gradient, the op returns the composition's gradients (an unused y gives its quantizer no
    gradient: zeros, as the composition's parameters get None / zeros)."""
    import mhaq_amd as M
    from mhaq_amd.act_hub import ActGradHub
    dtype = torch.bfloat16
    q = _quantizer(M.QNMethod[method], -1.0)
    for form in ("add_relu_fq_a", "relu_fq_a"):
        z, add, gy, ga, _ = _inputs(q, SHAPES["mid"], "channels_last", dtype, False, form == "add_relu_fq_a", -1.0, True)
        for use_hub in (False, True):
            hub = ActGradHub(torch.nn.ModuleList([q])) if use_hub else None
            ref = _run(q, hub, False, form, dtype, z, add, gy, ga, seed=5, use=use)
            got = _run(q, hub, True, form, dtype, z, add, gy, ga, seed=5, use=use)
            q.__dict__.pop("_hub", None)
            for k in (0, 1, 2, 3):
                if ref[k] is not None:
                    assert _same(got[k], ref[k]), (k, method, use, form, use_hub)
            if "y" in use:
                for g_f, g_r in zip(got[4], ref[4]):
                    assert torch.equal(g_f.view(torch.int32), g_r.view(torch.int32)), (method, use, form, use_hub)
            else:
                for g_f in got[4]:
                    assert g_f is None or float(g_f) == 0.0


@pytest.mark.parametrize("method", [0, 1, 3])        # STE, EWGS, LSQ (include/mhaq_fq.h)
@pytest.mark.parametrize("dt,size", DT_SIZES)
def test_partial_rows_equal_the_unfused_16bit_kernels(dt, size, method):
    """C ABI: mhaq_fq_act_relu_bwd_partials_x16 leaves the bytes mhaq_fq_act_bwd_partials_x16 leaves for (relu(z), g_y) --
    row count, layout, values, {s, qr} behind them -- with z the ReLU's input or its output, with and without g_a, in
    every kernel form (both sides get the same pointer alignment); gx = threshold_backward(R(gx_unfused + g_a), a); the
    forward gives mhaq_fq_act_fwd_x16's y on a."""
    import mhaq_amd as M
    from mhaq_amd import _lib, ops
    L = _lib.lib()
    dtype, code = DTYPES[dt], {"bf16": _lib.DT_BF16, "fp16": _lib.DT_F16}[dt]
    shape, unaligned = SHAPES[size], size == "unaligned"
    name = {0: "STE", 1: "EWGS", 3: "LSQ"}[method]
    z, _, gy, ga, _ = _inputs(_quantizer(M.QNMethod[name], 0.25), shape, "nchw", dtype, unaligned, False, 0.25, False)
    n = z.numel()
    a = _misaligned_copy(torch.relu(z)) if unaligned else torch.relu(z)
    ls, lq, bb = (torch.tensor([v], device=DEV) for v in (LOG_S, LOG_Q, 0.25))
    params = torch.empty(5, device=DEV)
    y_ref, y, a_out = torch.empty_like(a), torch.empty_like(z), torch.empty_like(z)
    _lib.check(L.mhaq_fq_act_fwd_x16(a.data_ptr(), y_ref.data_ptr(), n, code, ls.data_ptr(), lq.data_ptr(), bb.data_ptr(),
                                     params.data_ptr(), None, None, None, 0, ops._stream()), "mhaq_fq_act_fwd_x16")
    p2 = torch.empty(5, device=DEV)
    _lib.check(L.mhaq_fq_act_relu_fwd_x16(z.data_ptr(), None, y.data_ptr(), a_out.data_ptr(), n, code, ls.data_ptr(),
                                          lq.data_ptr(), bb.data_ptr(), p2.data_ptr(), ops._stream()),
               "mhaq_fq_act_relu_fwd_x16")
    assert torch.equal(y, y_ref) and torch.equal(p2, params) and torch.equal(a_out, a)
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    ws_ref = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    gx_ref = torch.empty_like(a)
    np_ref = ctypes.c_int32(0)
    _lib.check(L.mhaq_fq_act_bwd_partials_x16(a.data_ptr(), gy.data_ptr(), gx_ref.data_ptr(), n, code, params.data_ptr(),
                                              method, None, 99, 5, None, ws_ref.data_ptr(), nb, ctypes.byref(np_ref),
                                              ops._stream()), "mhaq_fq_act_bwd_partials_x16")
    used = (3 * np_ref.value + 2) * 4
    for src in (z, a):                               # the ReLU's input (mid-block) or its output (block end, stem)
        for g_a in (None, ga):
            ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
            gx = torch.empty_like(src)
            np_f = ctypes.c_int32(0)
            _lib.check(L.mhaq_fq_act_relu_bwd_partials_x16(src.data_ptr(), gy.data_ptr(),
                                                           g_a.data_ptr() if g_a is not None else None, gx.data_ptr(),
                                                           n, code, params.data_ptr(), method, 99, 5, None,
                                                           ws.data_ptr(), nb, ctypes.byref(np_f), ops._stream()),
                       "mhaq_fq_act_relu_bwd_partials_x16")
            torch.cuda.synchronize()
            assert np_f.value == np_ref.value
            assert torch.equal(ws[:used], ws_ref[:used]), (dt, method, size, src is z, g_a is not None)
            total = gx_ref + g_a if g_a is not None else gx_ref          # a 16-bit add: the second rounding
            assert total.dtype == dtype
            want = torch.ops.aten.threshold_backward(total.contiguous(), a.contiguous(), 0)
            assert _same(gx.contiguous(), want), (dt, method, size, src is z, g_a is not None)


def test_error_codes_are_the_existing_ones():
    from mhaq_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros(64, device=DEV, dtype=torch.bfloat16)
    p = torch.ones(5, device=DEV)
    ws = torch.zeros(L.mhaq_fq_act_bwd_workspace_bytes(64), dtype=torch.uint8, device=DEV)
    npo = ctypes.c_int32(0)
    P = L.mhaq_fq_act_relu_bwd_partials_x16
    args = (x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 64, _lib.DT_BF16, p.data_ptr())
    tail = (0, 0, None, ws.data_ptr(), ws.numel(), ctypes.byref(npo), ops._stream())
    assert P(*args, 2, *tail) == -4                  # AEWGS: MHAQ_FQ_EUNSUPPORTED
    assert P(*args, 7, *tail) == -1                  # MHAQ_FQ_EINVAL
    assert P(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 64, 0, p.data_ptr(), 0, *tail) == -1       # dtype
    assert P(*args, 0, 0, 0, None, ws.data_ptr(), 8, ctypes.byref(npo), ops._stream()) == -2             # EWORKSPACE
    assert P(x.data_ptr() + 1, x.data_ptr(), None, x.data_ptr(), 60, _lib.DT_BF16, p.data_ptr(), 0, *tail) == -3   # EALIGN
    assert L.mhaq_fq_act_relu_fwd_x16(None, None, x.data_ptr(), None, 64, _lib.DT_BF16, p.data_ptr(), p.data_ptr(),
                                      p.data_ptr(), p.data_ptr(), ops._stream()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("use_hub", [False, True])
def test_a_backward_draws_one_sign_stream_offset_or_none(use_hub):
    """Host side only: a 16-bit backward that launches a random estimator (STE, EWGS) takes exactly ONE offset of the sign
    stream -- whichever of y and a were used --, LSQ takes none; with and without an ActGradHub."""
    import mhaq_amd as M
    from mhaq_amd import ops
    from mhaq_amd.act_hub import ActGradHub
    z0 = torch.randn(2, 3, 5, 7, device=DEV).bfloat16()
    g = torch.randn(2, 3, 5, 7, device=DEV).bfloat16()
    q = _quantizer(M.QNMethod.STE, 0.25)
    hub = ActGradHub(torch.nn.ModuleList([q])) if use_hub else None
    ops.manual_seed(3)
    try:
        for method, want in (("STE", 1), ("EWGS", 1), ("LSQ", 0)):
            m = M.QNMethod[method].value
            for used in ((0,), (1,), (0, 1)):            # y only, a only, both
                z = z0.clone().requires_grad_(True)
                params = (q.log_act_s, q.log_act_q, q.act_b)
                if hub is not None:
                    hub.begin()
                    params = hub.take(0)
                outs = ops.act_relu_layer(z, None, *params, m, True, hub_slot=(hub, 0) if hub is not None else None)[:2]
                if hub is not None:
                    hub.end()
                assert outs[0].dtype == outs[1].dtype == torch.bfloat16
                before = ops.rng.drawn()
                torch.autograd.backward([outs[i] for i in used], [g] * len(used))
                torch.cuda.synchronize()
                assert z.grad is not None and z.grad.dtype == torch.bfloat16
                assert ops.rng.drawn() - before == want, (method, used)
    finally:
        q.__dict__.pop("_hub", None)


def test_backward_refuses_a_gradient_of_another_dtype():
    import mhaq_amd as M
    from mhaq_amd import ops
    q = _quantizer(M.QNMethod.LSQ, 0.25)
    ops.manual_seed(3)
    z = torch.randn(2, 3, 5, 7, device=DEV).bfloat16().requires_grad_(True)
    y, a = ops.act_relu_layer(z, None, q.log_act_s, q.log_act_q, q.act_b, M.QNMethod.LSQ.value, True)[:2]
    node = y.grad_fn
    with pytest.raises(RuntimeError, match="dtype"):
        node(torch.ones_like(y, dtype=torch.float32), None, torch.ones_like(a, dtype=torch.float32))


def test_16bit_tensors_outside_autocast_are_not_fused():
    """There the module promotes to float32 (the reference's op chain does): forward_fused does not restate that."""
    import mhaq_amd as M
    q = _quantizer(M.QNMethod.STE, 0.25)
    z = torch.randn(2, 3, 5, 7, device=DEV).bfloat16()
    assert not q.can_fuse_relu(z)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert q.can_fuse_relu(z) and q.can_fuse_relu(z, z.clone())
        assert not q.can_fuse_relu(z, z.float()) and not q.can_fuse_relu(z.half())
        assert q.can_fuse_relu(z.float())
    with torch.autocast("cuda", dtype=torch.float16):
        assert q.can_fuse_relu(z.half()) and not q.can_fuse_relu(z)


def test_mixed_hub_finalizes_fp32_plain_16bit_plain_and_16bit_fused_in_one_launch():
    import mhaq_amd as M
    from mhaq_amd import _ext, ops
    from mhaq_amd.act_hub import ActGradHub
    dtype = torch.bfloat16
    qs = [_quantizer(M.QNMethod.STE, -1.0), _quantizer(M.QNMethod.EWGS, 0.25), _quantizer(M.QNMethod.STE, -1.0)]
    holder = torch.nn.ModuleList(qs)
    gen = torch.Generator(device=DEV).manual_seed(8)
    x32 = torch.randn(4, 16, 14, 14, device=DEV, generator=gen) * 2
    x16 = _tensor((8, 64, 14, 14), "channels_last", gen, dtype)
    z, add, gy, ga, _ = _inputs(qs[2], SHAPES["ragged"], "nchw", dtype, False, True, -1.0, False)
    g32, g16 = torch.randn_like(x32), torch.randn_like(x16)

    def run(hub, fused):
        ops.manual_seed(21)
        for q in qs:
            for p in q.parameters():
                p.grad = None
        zz, aa = z.detach().requires_grad_(True), add.detach().requires_grad_(True)
        if hub is not None:
            hub.begin()
        with torch.autocast("cuda", dtype=dtype):
            y0 = qs[0](x32)
            y1 = qs[1](x16)
            if fused:
                y2, a2 = qs[2].forward_fused(zz, aa, want_act=True)
            else:
                a2 = torch.relu(zz + aa)
                y2 = qs[2](a2)
        if hub is not None:
            hub.end()
        assert y0.dtype == torch.float32 and y1.dtype == dtype and y2.dtype == dtype
        _ext.ext().host_timers(True)
        torch.autograd.backward([y0, y1, y2, a2], [g32, g16, gy, ga])
        torch.cuda.synchronize()
        launches = _ext.ext().host_timers(True)["hub_bwd"][0]
        return [p.grad.clone() for q in qs for p in q.parameters()], zz.grad, launches

    try:
        hub = ActGradHub(holder)
        ref, gz_ref, n_ref = run(hub, False)
        got, gz, n_got = run(hub, True)
        assert n_ref == 1 and n_got == 1 and hub.state()["pending"] == 0
    finally:
        for q in qs:
            q.__dict__.pop("_hub", None)
    alone, gz_alone, n_alone = run(None, True)       # per-quantizer finalize launches: the same bits
    assert n_alone == 0
    assert len(got) == 9 and _same(gz, gz_ref) and _same(gz, gz_alone)
    for k, (g, r, s) in enumerate(zip(got, ref, alone)):
        assert bool(torch.isfinite(g).all()) and float(g) != 0.0, k
        assert torch.equal(g.view(torch.int32), r.view(torch.int32)), k
        assert torch.equal(g.view(torch.int32), s.view(torch.int32)), k
