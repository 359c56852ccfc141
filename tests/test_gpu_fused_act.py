"""GPU (-m gpu): the ReLU / residual-add forms of the NoisyAct kernels (mhaq_fq_act_relu_fwd / _bwd, NoisyAct.forward_fused)
against today's composition -- torch.relu / torch.add + the NoisyAct op + autograd.  ReLU, a two-term fp32 add and a mask
are exact elementwise operations, so everything is compared for equality: y, a, the input gradients with torch.equal, the
three parameter gradients bit for bit (with and without an ActGradHub), and -- at the C ABI -- the partial rows themselves.

Kernel forms: the parameter gradients are sums whose order belongs to the kernel form (one row per block from 20 Mi
elements, one per wave below, the dword kernel for unaligned pointers).  The fused backward reads the tensor it saved: the
ReLU output a (a fresh, aligned tensor) when a is an output of the op, the caller's z otherwise.  For an unaligned z in
the form without a, today's path would hand its quantizer the aligned torch.relu(z) and sum in another order; there the
reference quantizer is fed an equally misaligned copy of a, so that both sides run the dword kernel (the elementwise
results do not depend on the form)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

FORMS = ("relu_fq", "add_relu_fq_a", "relu_fq_a")
SHAPES = {
    "big": (40, 64, 96, 96),       # 23.6 M elements >= 20 Mi: one partial row per block
    "mid": (250, 128, 14, 14),     # 6.3 M elements: one partial row per wave
    "ragged": (3, 5, 7, 11),       # 1155 elements, n % 4 == 3
    "unaligned": (6, 16, 9, 13),   # a view 4 bytes into its buffer: the dword kernels
}


def _tensor(shape, layout, gen, unaligned=False, scale=3.0):
    """A dense tensor of `shape` in `layout` memory order; `unaligned`: a view one float into a larger buffer."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.empty(n + 1, device=DEV)
    flat = buf[1:] if unaligned else buf[:n]
    flat.copy_(torch.randn(n, device=DEV, generator=gen) * scale)
    if layout == "channels_last":
        N, C, H, W = shape
        return flat.view(N, H, W, C).permute(0, 3, 1, 2)
    return flat.view(shape)


def _misaligned_copy(t):
    """The values of t in t's own strides, 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device)
    out = buf[1:].as_strided(t.shape, t.stride())
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def _inputs(shape, layout, unaligned, with_add, b):
    """z (and addend) with exact zeros, -0.0, negative values inside and outside [lo, hi] and values beyond hi."""
    gen = torch.Generator(device=DEV).manual_seed(1234)
    z = _tensor(shape, layout, gen, unaligned)
    add = _tensor(shape, layout, gen, unaligned) if with_add else None
    zf = z.permute(0, 2, 3, 1).reshape(-1) if layout == "channels_last" else z.reshape(-1)
    assert zf.data_ptr() == z.data_ptr()            # a flat alias in memory order
    zf[0::7] = 0.0
    zf[1::11] = -0.0
    zf[2::13] = b - 0.5                              # below the clamp range
    zf[3::17] = b + 0.25                             # inside it
    zf[4::19] = 50.0                                 # above it
    if with_add:
        af = add.permute(0, 2, 3, 1).reshape(-1) if layout == "channels_last" else add.reshape(-1)
        af[0::7] = 0.0                               # 0 + 0
        af[5::23] = -zf[5::23]                       # exact cancellation: z + addend == 0
        af[2::13] = 0.0
        af[3::17] = 0.0
        af[4::19] = 0.0
    gy = _tensor(shape, layout, gen)
    ga = _tensor(shape, layout, gen)
    return z, add, gy, ga


def _quantizer(method, b):
    import mhaq_amd as M
    q = M.NoisyAct(init_s=-3, init_q=2, signed=True).to(DEV).train()      # s = 1/8, qr = 4: [b, b + 3.875]
    with torch.no_grad():
        q.act_b.fill_(b)
    q.Q.qnmethod = method
    return q


def _run(q, hub, fused, form, z0, add0, gy, ga, seed):
    from mhaq_amd import ops
    ops.manual_seed(seed)                            # the same (seed, offset) for both sides
    for p in q.parameters():
        p.grad = None
    z = z0.detach().requires_grad_(True)
    add = add0.detach().requires_grad_(True) if add0 is not None else None
    want_a = form != "relu_fq"
    if hub is not None:
        hub.begin()
    try:
        if fused:
            assert q.can_fuse_relu(z, add)
            y, a = q.forward_fused(z, add, want_act=want_a)
            assert (a is not None) == want_a
            outs, gs = ([y, a], [gy, ga]) if want_a else ([y], [gy])
            torch.autograd.backward(outs, gs)
        else:
            a = torch.relu(torch.add(z, add) if add is not None else z)
            if not want_a and z.data_ptr() % 16 != 0:
                # (module docstring) the reference quantizer on a misaligned copy of a: the dword kernel on both sides
                a_u = _misaligned_copy(a.detach()).requires_grad_(True)
                y = q(a_u)
                y.backward(gy)
                a.backward(a_u.grad)
            else:
                y = q(a)
                outs, gs = ([y, a], [gy, ga]) if want_a else ([y], [gy])
                torch.autograd.backward(outs, gs)
    finally:
        if hub is not None:
            hub.end()
    torch.cuda.synchronize()
    grads = [p.grad.detach().clone() for p in (q.log_act_s, q.log_act_q, q.act_b)]
    return (y.detach(), a.detach() if want_a else None, z.grad, add.grad if add is not None else None, grads)


@pytest.mark.parametrize("size", list(SHAPES))
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("method", ["STE", "LSQ", "EWGS"])
def test_fused_forms_equal_todays_composition(method, layout, size):
    import mhaq_amd as M
    from mhaq_amd.act_hub import ActGradHub
    shape, unaligned = SHAPES[size], size == "unaligned"
    for b in (0.25, -1.0):                           # a range above zero (zeros clip to lo) and one that holds zero
        if size == "big" and b != 0.25:
            continue                                 # (one pass over the 23.6 M-element case)
        q = _quantizer(M.QNMethod[method], b)
        other = _quantizer(M.QNMethod[method], b)    # a second quantizer: the hub finalizes several in one launch
        holder = torch.nn.ModuleList([other, q])
        for form in FORMS:
            z, add, gy, ga = _inputs(shape, layout, unaligned, form == "add_relu_fq_a", b)
            assert (z.data_ptr() % 16 != 0) == unaligned
            for use_hub in (False, True):
                hub = ActGradHub(holder) if use_hub else None
                ref = _run(q, hub, False, form, z, add, gy, ga, seed=77)
                got = _run(q, hub, True, form, z, add, gy, ga, seed=77)
                if hub is not None:
                    for m in holder:
                        m.__dict__.pop("_hub", None)
                what = (method, layout, size, b, form, use_hub)
                assert torch.equal(got[0], ref[0]), ("y", what)
                if ref[1] is not None:
                    assert torch.equal(got[1], ref[1]), ("a", what)
                    assert got[1].stride() == z.stride()
                assert torch.equal(got[2], ref[2]), ("gx", what)
                if ref[3] is not None:
                    assert torch.equal(got[3], ref[3]), ("g_addend", what)
                for name, g_f, g_r in zip(("log_act_s", "log_act_q", "act_b"), got[4], ref[4]):
                    assert g_f.shape == g_r.shape
                    assert torch.equal(g_f.view(torch.int32), g_r.view(torch.int32)), (name, what, float(g_f), float(g_r))
                # the zeros, the negatives and the clipped values are really there
                a_all = torch.relu(z + add if add is not None else z)
                assert bool((a_all == 0).any()) and bool((z < b - 0.25).any()) and bool((a_all > b + 3.875).any())
            del z, add, gy, ga
        torch.cuda.empty_cache()


@pytest.mark.parametrize("size", list(SHAPES))
@pytest.mark.parametrize("method", [0, 1, 3])        # STE, EWGS, LSQ (include/mhaq_fq.h)
def test_partial_rows_equal_the_unfused_kernels(method, size):
    """C ABI: mhaq_fq_act_relu_bwd_partials leaves the bytes mhaq_fq_act_bwd_partials leaves for (relu(z), g_y) -- row
    count, layout, values, {s, qr} behind them -- with z the ReLU's input or its output, with and without g_a, in every
    kernel form (here both sides get the same pointer alignment); gx = threshold_backward(gx_unfused + g_a, a)."""
    from mhaq_amd import _lib, ops
    L = _lib.lib()
    shape, unaligned = SHAPES[size], size == "unaligned"
    z, _, gy, ga = _inputs(shape, "nchw", unaligned, False, 0.25)
    n = z.numel()
    a = _misaligned_copy(torch.relu(z)) if unaligned else torch.relu(z)
    ls, lq, bb = (torch.tensor([v], device=DEV) for v in (-3.0, 2.0, 0.25))
    params = torch.empty(5, device=DEV)
    y_ref, y = torch.empty_like(a), torch.empty_like(z)
    _lib.check(L.mhaq_fq_act_fwd(a.data_ptr(), y_ref.data_ptr(), n, ls.data_ptr(), lq.data_ptr(), bb.data_ptr(),
                                 params.data_ptr(), None, None, None, 0, ops._stream()), "mhaq_fq_act_fwd")
    p2 = torch.empty(5, device=DEV)
    _lib.check(L.mhaq_fq_act_relu_fwd(z.data_ptr(), None, y.data_ptr(), None, n, ls.data_ptr(), lq.data_ptr(),
                                      bb.data_ptr(), p2.data_ptr(), ops._stream()), "mhaq_fq_act_relu_fwd")
    assert torch.equal(y, y_ref) and torch.equal(p2, params)
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    ws_ref = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    gx_ref = torch.empty_like(a)
    np_ref = ctypes.c_int32(0)
    _lib.check(L.mhaq_fq_act_bwd_partials(a.data_ptr(), gy.data_ptr(), gx_ref.data_ptr(), n, params.data_ptr(), method,
                                          None, 99, 5, None, ws_ref.data_ptr(), nb, ctypes.byref(np_ref), ops._stream()),
               "mhaq_fq_act_bwd_partials")
    used = (3 * np_ref.value + 2) * 4
    for src in (z, a):                               # the ReLU's input (mid-block) or its output (block end, stem)
        for g_a in (None, ga):
            ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
            gx = torch.empty_like(src)
            np_f = ctypes.c_int32(0)
            _lib.check(L.mhaq_fq_act_relu_bwd_partials(src.data_ptr(), gy.data_ptr(),
                                                       g_a.data_ptr() if g_a is not None else None, gx.data_ptr(), n,
                                                       params.data_ptr(), method, 99, 5, None, ws.data_ptr(), nb,
                                                       ctypes.byref(np_f), ops._stream()),
                       "mhaq_fq_act_relu_bwd_partials")
            torch.cuda.synchronize()
            assert np_f.value == np_ref.value
            assert torch.equal(ws[:used], ws_ref[:used]), (method, size, src is z, g_a is not None)
            total = gx_ref + g_a if g_a is not None else gx_ref
            assert torch.equal(gx, torch.ops.aten.threshold_backward(total.contiguous(), a.contiguous(), 0)), \
                (method, size, src is z, g_a is not None)


def test_error_codes_are_the_existing_ones():
    from mhaq_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros(64, device=DEV)
    p = torch.ones(5, device=DEV)
    ws = torch.zeros(L.mhaq_fq_act_bwd_workspace_bytes(64), dtype=torch.uint8, device=DEV)
    npo = ctypes.c_int32(0)
    args = (x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 64, p.data_ptr())
    tail = (0, 0, None, ws.data_ptr(), ws.numel(), ctypes.byref(npo), ops._stream())
    assert L.mhaq_fq_act_relu_bwd_partials(*args, 2, *tail) == -4        # AEWGS: MHAQ_FQ_EUNSUPPORTED
    assert L.mhaq_fq_act_relu_bwd_partials(*args, 7, *tail) == -1        # MHAQ_FQ_EINVAL
    assert L.mhaq_fq_act_relu_bwd_partials(x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 64, p.data_ptr(), 0, 0, 0, None,
                                           ws.data_ptr(), 8, ctypes.byref(npo), ops._stream()) == -2   # EWORKSPACE
    assert L.mhaq_fq_act_relu_bwd_partials(x.data_ptr() + 2, x.data_ptr(), None, x.data_ptr(), 60, p.data_ptr(), 0, 0, 0,
                                           None, ws.data_ptr(), ws.numel(), ctypes.byref(npo), ops._stream()) == -3  # EALIGN
    assert L.mhaq_fq_act_relu_fwd(None, None, x.data_ptr(), None, 64, p.data_ptr(), p.data_ptr(), p.data_ptr(),
                                  p.data_ptr(), ops._stream()) == -1


@pytest.mark.parametrize("use_hub", [False, True])
def test_a_backward_draws_one_sign_stream_offset_or_none(use_hub):
    """Host side only (any size runs the same host code): a backward that launches a random estimator (STE, EWGS) takes
    exactly ONE offset of the sign stream -- whichever of y and a were used --, LSQ and explicit signs take none; with and
    without an ActGradHub."""
    import mhaq_amd as M
    from mhaq_amd import ops
    from mhaq_amd.act_hub import ActGradHub
    z0 = torch.randn(2, 3, 5, 7, device=DEV)
    g = torch.randn_like(z0)
    q = _quantizer(M.QNMethod.STE, 0.25)
    hub = ActGradHub(torch.nn.ModuleList([q])) if use_hub else None
    ops.manual_seed(3)

    def drawn_by(op, used):
        """Sign-stream offsets taken by the backward of the outputs `used` of op(z, parameters, hub_slot)."""
        z = z0.clone().requires_grad_(True)
        params = (q.log_act_s, q.log_act_q, q.act_b)
        if hub is not None:
            hub.begin()
            params = hub.take(0)
        outs = op(z, params, (hub, 0) if hub is not None else None)
        if hub is not None:
            hub.end()
        before = ops.rng.drawn()
        torch.autograd.backward([outs[i] for i in used], [g] * len(used))
        torch.cuda.synchronize()
        assert z.grad is not None
        return ops.rng.drawn() - before

    try:
        for method, want in (("STE", 1), ("EWGS", 1), ("LSQ", 0)):
            m = M.QNMethod[method].value
            for used in ((0,), (1,), (0, 1)):            # y only, a only, both
                got = drawn_by(lambda z, p, hs: ops.act_relu_layer(z, None, *p, m, True, hub_slot=hs)[:2], used)
                assert got == want, (method, used, got)
        r_sign = torch.ones(z0.shape, dtype=torch.int8, device=DEV)
        for r, want in ((r_sign, 0), (None, 1)):
            got = drawn_by(lambda z, p, hs: ops.fake_quant_act_layer(z, *p, M.QNMethod.STE, r, hub_slot=hs), (0,))
            assert got == want, (r is not None, got)
    finally:
        q.__dict__.pop("_hub", None)
