"""GPU (-m gpu): the stem's max pool with 1-byte argmax codes (mhaq_fq_maxpool3s2_fwd), the BatchNorm backward that gathers
its dy from the pooled gradient and those codes (mhaq_fq_bn_pool_bwd, csrc/bn_bwd.hip), the node over both
(bn_pool_train, csrc/torch_binding.cpp) and the trainer with the switch on and off.

Every comparison is BIT FOR BIT (int32 views: signed zeros and NaNs count): max and select are exact, the at most four
fp32 adds of the pool's backward are done in torch's order (and not done where torch's channels_last kernel assigns: an
element covered by one window), and the BatchNorm sums are the same fp64 code over the same partition.  The yardsticks are torch's own max_pool2d forward / backward on the same device and mhaq_fq_bn_bwd on the
materialized dy.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5

# the smallest shapes at which each part can go wrong (N, C, H, W): one window; even / odd edges; C / 4 = 5 (an idle lane
# in the reduction, a non-zero column step in dx); two row chunks with a ragged end; eight column chunks; the stem's row
# length; the BIG occupancy form with default loads (22.2 M elements) and with non-temporal loads (29.6 M)
SHAPES = [(1, 4, 1, 1), (2, 4, 2, 3), (1, 8, 3, 3), (3, 20, 5, 7), (2, 64, 9, 9), (2, 8, 17, 15), (2, 512, 7, 7),
          (1, 64, 112, 112), (3, 64, 340, 340), (4, 64, 340, 340)]
_ids = lambda s: "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = det


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _out(n):
    return (n - 1) // 2 + 1


def _pool_input(shape, seed=0):
    """Integer-valued data in a small range (ties are plentiful), with planted windows: all equal, all -inf, one holding
    +inf, one holding one NaN and one holding several (each in its own channel, where the tensor is large enough)."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-3, 4, shape, generator=g).float()
    if h >= 3 and w >= 3:
        a, b = (h - 3) // 2, (w - 3) // 2
        t[0, 0, a:a + 3, b:b + 3] = 2.0
        t[0, 1, a:a + 3, b:b + 3] = float("-inf")
        t[0, 2, a + 1, b + 1] = float("inf")
        t[0, 3, a + 1, b + 2] = float("nan")
        t[n - 1, 0, a, b] = float("nan")
        t[n - 1, 0, a + 2, b + 1] = float("nan")
        t[n - 1, 0, a + 1, b + 2] = float("nan")
        t[n - 1, 1, :, :] = float("-inf")               # a whole plane: no window chooses an element
    else:
        t[0, 1] = float("-inf")
        t[0, 2, 0, 0] = float("nan")
        t[0, 3] = 1.0
    return _cl(t)


def _pooled_grad(shape, seed=1):
    """The pooled gradient [N, C, OH, OW]: small integers with +-0 among them; NaN and +-inf planted in channels 1 and 2."""
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-2, 3, (n, c, _out(h), _out(w)), generator=gen).float()
    g[g == 0] = g[g == 0] * torch.where(torch.rand(int((g == 0).sum()), generator=gen) < 0.5, -1.0, 1.0)   # +-0
    g[0, 1, 0, 0] = float("nan")
    g[n - 1, 2, -1, -1] = float("inf")
    if _out(w) > 1:
        g[0, 2, 0, 1] = float("-inf")
    return _cl(g)


def _lib():
    from mhaq_amd import _lib
    return _lib.lib()


_p = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hip_pool(t):
    n, c, h, w = t.shape
    p = torch.empty((n, c, _out(h), _out(w)), device=DEV).contiguous(memory_format=torch.channels_last)
    code = torch.empty((n, c, _out(h), _out(w)), dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    rc = _lib().mhaq_fq_maxpool3s2_fwd(_p(t), _p(p), _p(code), n, h, w, c, _stream())
    assert rc == 0, rc
    return p, code


def _dy_from_codes(g, code, h, w):
    """The test's own statement of the gather.  An input element covered by ONE window takes that window's g where the
    code names it and 0.0 where not (torch's channels_last backward assigns there: -0.0 stays -0.0); one covered by two or
    four starts at 0.0 and adds g of every window whose code names it, in ascending oh, then ascending ow -- for a fixed
    input row that is DEscending kh (kh = ih - 2 oh + 1), likewise kw."""
    n, c, oh, ow = g.shape
    dy = torch.zeros((n, c, h, w), device=g.device)
    r, s = torch.arange(oh, device=g.device), torch.arange(ow, device=g.device)
    ihs, iws = torch.arange(h, device=g.device), torch.arange(w, device=g.device)
    one_h = ~((ihs % 2 == 1) & (ihs // 2 + 1 < oh))                   # rows covered by one row of windows
    one_w = ~((iws % 2 == 1) & (iws // 2 + 1 < ow))
    single = one_h[:, None] & one_w[None, :]
    for kh in (2, 1, 0):
        ih = 2 * r - 1 + kh
        vh = (ih >= 0) & (ih < h)
        for kw in (2, 1, 0):
            iw = 2 * s - 1 + kw
            vw = (iw >= 0) & (iw < w)
            if not bool(vh.any()) or not bool(vw.any()):
                continue
            rows, cols = ih[vh][:, None], iw[vw][None, :]
            gg = g[:, :, vh][:, :, :, vw]
            hit = code[:, :, vh][:, :, :, vw] == kh * 3 + kw
            old = dy[:, :, rows, cols]
            dy[:, :, rows, cols] = torch.where(hit, torch.where(single[rows, cols], gg, old + gg), old)
    return dy.contiguous(memory_format=torch.channels_last)


class _Case:
    """Everything the tests of one shape share, computed once: torch's pool forward and backward on the device, ours, the
    BatchNorm inputs, and mhaq_fq_bn_bwd on torch's dy."""

    def __init__(self, shape):
        n, c, h, w = shape
        self.shape = shape
        self.t = _pool_input(shape)
        tt = self.t.clone().requires_grad_(True)
        self.p_torch, self.idx_torch = F.max_pool2d(tt, 3, 2, 1, return_indices=True)
        self.g = _pooled_grad(shape)
        self.dy_torch, = torch.autograd.grad(self.p_torch, tt, self.g)
        self.p_torch = self.p_torch.detach()
        self.p, self.code = _hip_pool(self.t)
        gen = torch.Generator().manual_seed(7)
        self.x = _cl(torch.randn(shape, generator=gen) * 2 + torch.randn(1, c, 1, 1, generator=gen))
        self.mean = self.x.mean((0, 2, 3))
        self.invstd = (self.x.var((0, 2, 3), unbiased=False) + EPS).rsqrt() if n * h * w > 1 else torch.full((c,), EPS ** -0.5, device=DEV)
        self.gamma = torch.randn(c, generator=gen).to(DEV)
        self.ref = self.bn_bwd()

    def workspace_bytes(self):
        n, c, h, w = self.shape
        L = _lib()
        nb = L.mhaq_fq_bn_pool_bwd_workspace_bytes(n, h, w, c)
        assert nb == L.mhaq_fq_bn_bwd_workspace_bytes(n * h * w, c) and nb > 0
        return nb

    def bn_bwd(self):
        n, c, h, w = self.shape
        nb = self.workspace_bytes()
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        dx, dw, db = torch.empty_like(self.x), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        rc = _lib().mhaq_fq_bn_bwd(_p(self.x), _p(self.dy_torch), _p(self.mean), _p(self.invstd), _p(self.gamma), _p(dx),
                                   _p(dw), _p(db), n * h * w, c, _p(ws), nb, _stream())
        assert rc == 0, rc
        return dx, dw, db, ws

    def bn_pool_bwd(self, want=(True, True, True), gamma=True):
        n, c, h, w = self.shape
        nb = self.workspace_bytes()
        ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        dx = torch.empty_like(self.x) if want[0] else None
        dw = torch.empty(c, device=DEV) if want[1] else None
        db = torch.empty(c, device=DEV) if want[2] else None
        rc = _lib().mhaq_fq_bn_pool_bwd(_p(self.x), _p(self.g), _p(self.code), _p(self.mean), _p(self.invstd),
                                        _p(self.gamma) if gamma else None, _p(dx), _p(dw), _p(db), n, h, w, c, _p(ws), nb,
                                        _stream())
        assert rc == 0, rc
        return dx, dw, db, ws


_cases = {}


def _case(shape):
    if shape not in _cases:
        if len(_cases) and max(map(lambda s: s[0] * s[1] * s[2] * s[3], _cases)) > 1 << 24:
            _cases.clear()                              # one large case resident at a time
            torch.cuda.empty_cache()
        _cases[shape] = _Case(shape)
    return _cases[shape]


# ------------------------------------------------------------------------------------------------ C ABI, forward
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_equals_torch_max_pool2d_values_and_indices(shape):
    k = _case(shape)
    n, c, h, w = shape
    assert _same_bits(k.p, k.p_torch)
    code = k.code.long()
    oh = torch.arange(_out(h), device=DEV)[:, None]
    ow = torch.arange(_out(w), device=DEV)[None, :]
    # code 9: the window chose no element (all -inf); torch's channels_last kernel leaves its initial index 0 there
    assert int(code.max()) <= 9 and (h < 3 or w < 3 or bool((code == 9).any()))
    idx = torch.where(code == 9, 0, (2 * oh - 1 + code // 3) * w + (2 * ow - 1 + code % 3))
    assert torch.equal(idx, k.idx_torch)
    chosen = (2 * oh - 1 + code // 3 >= 0) & (2 * oh - 1 + code // 3 < h) & (2 * ow - 1 + code % 3 >= 0) & (2 * ow - 1 + code % 3 < w)
    assert bool((chosen | (code == 9)).all())                      # a chosen element lies inside the tensor


# ------------------------------------------------------------------------------------------------ C ABI, backward
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gather_restated_in_torch_equals_torch_max_pool2d_backward(shape):
    k = _case(shape)
    assert _same_bits(_dy_from_codes(k.g, k.code, shape[2], shape[3]), k.dy_torch)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_bn_pool_bwd_equals_bn_bwd_on_torchs_dy_partial_rows_included(shape):
    k = _case(shape)
    dx, dw, db, ws = k.bn_pool_bwd()
    rdx, rdw, rdb, rws = k.ref
    assert _same_bits(dx, rdx) and _same_bits(dw, rdw) and _same_bits(db, rdb)
    assert torch.equal(ws, rws)                        # the constants and the fp64 partial rows, byte for byte


def test_outputs_are_optional_and_a_null_weight_is_one():
    k = _case((3, 20, 5, 7))
    full = k.bn_pool_bwd()
    only = k.bn_pool_bwd(want=(False, True, False))
    assert only[0] is None and only[2] is None and _same_bits(only[1], full[1])
    only = k.bn_pool_bwd(want=(True, False, False))
    assert _same_bits(only[0], full[0])
    saved = k.gamma
    one = k.bn_pool_bwd(gamma=False)
    k.gamma = torch.ones_like(saved)
    ones = k.bn_pool_bwd()
    k.gamma = saved
    assert all(_same_bits(a, b) for a, b in zip(one[:3], ones[:3]))


def test_argument_errors_launch_nothing():
    """Misaligned base pointers, a short workspace, C % 4 and n * h * w >= 2^31: the error code, and sentinel-filled
    outputs stay untouched."""
    L = _lib()
    k = _case((2, 64, 9, 9))
    n, c, h, w = k.shape
    sent = 0x5A
    nb = k.workspace_bytes()
    ws = torch.full((nb + 16,), sent, dtype=torch.uint8, device=DEV)
    dx = torch.full((k.x.numel() * 4 + 16,), sent, dtype=torch.uint8, device=DEV)
    dw = torch.full((c * 4,), sent, dtype=torch.uint8, device=DEV)
    db = torch.full((c * 4,), sent, dtype=torch.uint8, device=DEV)
    args = [_p(k.x), _p(k.g), _p(k.code), _p(k.mean), _p(k.invstd), _p(k.gamma), _p(dx), _p(dw), _p(db), n, h, w, c,
            _p(ws), nb, _stream()]
    for pos, off in ((0, 4), (1, 8), (2, 2), (6, 4), (13, 8), (3, 2)):
        bad = list(args)
        bad[pos] = ctypes.c_void_p(args[pos].value + off)
        assert L.mhaq_fq_bn_pool_bwd(*bad) == -3, pos
    short = list(args)
    short[14] = nb - 1
    assert L.mhaq_fq_bn_pool_bwd(*short) == -2
    odd = list(args)
    odd[12] = 62
    assert L.mhaq_fq_bn_pool_bwd(*odd) == -4
    huge = list(args)
    huge[9], huge[14] = (1 << 31) // (h * w) + 1, 1 << 62
    assert L.mhaq_fq_bn_pool_bwd(*huge) == -4
    # the forward
    p = torch.full((k.p.numel() * 4 + 16,), sent, dtype=torch.uint8, device=DEV)
    code = torch.full((k.p.numel() + 16,), sent, dtype=torch.uint8, device=DEV)
    fargs = [_p(k.t), _p(p), _p(code), n, h, w, c, _stream()]
    for pos, off in ((0, 4), (1, 8), (2, 1)):
        bad = list(fargs)
        bad[pos] = ctypes.c_void_p(fargs[pos].value + off)
        assert L.mhaq_fq_maxpool3s2_fwd(*bad) == -3, pos
    bad = list(fargs)
    bad[6] = 62
    assert L.mhaq_fq_maxpool3s2_fwd(*bad) == -4
    bad = list(fargs)
    bad[3] = (1 << 31) // (h * w) + 1
    assert L.mhaq_fq_maxpool3s2_fwd(*bad) == -4
    torch.cuda.synchronize()
    for buf in (ws, dx, dw, db, p, code):
        assert bool((buf == sent).all())


@pytest.mark.parametrize("shape", [(3, 20, 5, 7), (2, 8, 17, 15), (2, 512, 7, 7)], ids=_ids)
def test_sentinel_guards_around_every_output(shape):
    L = _lib()
    k = _case(shape)
    n, c, h, w = shape
    guard, sent = 4096, 0x5A
    nb = k.workspace_bytes()
    buf = lambda body: torch.full((body + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    ws, dx, dw, db = buf(nb), buf(k.x.numel() * 4), buf(c * 4), buf(c * 4)
    p, code = buf(k.p.numel() * 4), buf(k.p.numel())
    assert L.mhaq_fq_maxpool3s2_fwd(_p(k.t), _p(p, guard), _p(code, guard), n, h, w, c, _stream()) == 0
    assert L.mhaq_fq_bn_pool_bwd(_p(k.x), _p(k.g), _p(code, guard), _p(k.mean), _p(k.invstd), _p(k.gamma), _p(dx, guard),
                                 _p(dw, guard), _p(db, guard), n, h, w, c, _p(ws, guard), nb, _stream()) == 0
    torch.cuda.synchronize()
    for b, body in ((ws, nb), (dx, k.x.numel() * 4), (dw, c * 4), (db, c * 4), (p, k.p.numel() * 4), (code, k.p.numel())):
        assert bool((b[:guard] == sent).all()) and bool((b[guard + body:] == sent).all())
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1)
    assert torch.equal(dx[guard:guard + k.x.numel() * 4].view(torch.int32), rows(k.ref[0]).view(torch.int32))
    assert torch.equal(code[guard:guard + k.p.numel()], rows(k.code))
    assert torch.equal(p[guard:guard + k.p.numel() * 4].view(torch.int32), rows(k.p).view(torch.int32))


# ------------------------------------------------------------------------------------------------ the node
def _ext():
    from mhaq_amd import _ext
    return _ext.ext()


def _node_step(entry, x, g, w, b, train_w=True, train_b=True):
    """One forward / backward of `entry`(x, weight, bias, running_mean, running_var, 0.1, eps, True) on fresh leaves."""
    x = x.clone().requires_grad_(True)
    w, b = w.clone().requires_grad_(train_w), b.clone().requires_grad_(train_b)
    c = x.shape[1]
    rm, rv = torch.zeros(c, device=x.device), torch.ones(c, device=x.device)
    p = entry(x, w, b, rm, rv, 0.1, EPS, True)
    p.backward(g)
    return dict(p=p.detach(), dx=x.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv)


def _composition(x, w, b, rm, rv, momentum, eps, cudnn):
    return F.max_pool2d(_ext().bn_train(x, w, b, rm, rv, momentum, eps, cudnn), 3, 2, 1)


def _assert_same_step(a, b):
    for key in a:
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, key
        else:
            assert _same_bits(a[key], b[key]), key


def _node_inputs(shape, seed=3):
    gen = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    # integer-valued inputs make ties in the BatchNorm output plentiful too (equal inputs normalize to equal outputs)
    x = _cl(torch.randint(-3, 4, shape, generator=gen).float())
    g = _cl(torch.randn((n, c, _out(h), _out(w)), generator=gen))
    return x, g, torch.randn(c, generator=gen).to(DEV), torch.randn(c, generator=gen).to(DEV)


@pytest.mark.parametrize("shape", [(2, 4, 2, 3), (3, 20, 5, 7), (2, 64, 9, 9), (2, 8, 17, 15), (1, 64, 112, 112)], ids=_ids)
def test_node_equals_bn_train_then_max_pool2d(shape):
    E = _ext()
    x, g, w, b = _node_inputs(shape)
    n0, m0 = E.bn_pool_hip_backwards(), E.bn_hip_backwards()
    got = _node_step(E.bn_pool_train, x, g, w, b)
    assert E.bn_pool_hip_backwards() == n0 + 1 and E.bn_hip_backwards() == m0          # the kernels were taken
    ref = _node_step(_composition, x, g, w, b)
    assert E.bn_pool_hip_backwards() == n0 + 1 and E.bn_hip_backwards() == m0 + 1
    _assert_same_step(got, ref)


def test_node_frozen_weight_frozen_bias_and_an_nchw_strided_gradient():
    E = _ext()
    x, g, w, b = _node_inputs((3, 20, 5, 7))
    full = _node_step(E.bn_pool_train, x, g, w, b)
    for tw, tb in ((False, True), (True, False), (False, False)):
        n0 = E.bn_pool_hip_backwards()
        got = _node_step(E.bn_pool_train, x, g, w, b, tw, tb)
        assert E.bn_pool_hip_backwards() == n0 + 1
        _assert_same_step(got, _node_step(_composition, x, g, w, b, tw, tb))
        assert (got["dw"] is None) == (not tw) and (got["db"] is None) == (not tb) and _same_bits(got["dx"], full["dx"])
    n0 = E.bn_pool_hip_backwards()
    got = _node_step(E.bn_pool_train, x, g.contiguous(), w, b)                         # the same values, NCHW strides
    assert E.bn_pool_hip_backwards() == n0 + 1
    _assert_same_step(got, full)


@pytest.mark.parametrize("case", ["nchw", "c_not_multiple_of_4", "cpu"])
def test_node_fallback_is_the_composition_and_the_counter_shows_it(case):
    E = _ext()
    if case == "c_not_multiple_of_4":
        x, g, w, b = _node_inputs((2, 6, 5, 4))
    else:
        x, g, w, b = _node_inputs((2, 8, 6, 5))
        x, g = x.contiguous(), g.contiguous()
    if case == "cpu":
        x, g, w, b = x.cpu(), g.cpu(), w.cpu(), b.cpu()
    n0 = E.bn_pool_hip_backwards()
    got = _node_step(E.bn_pool_train, x, g, w, b)
    assert E.bn_pool_hip_backwards() == n0
    _assert_same_step(got, _node_step(_composition, x, g, w, b))


class _Stem(nn.Module):
    """conv -> bn -> pool as the module path runs it: HipBackwardBatchNorm2d.forward_pooled against bn + nn.MaxPool2d."""

    def __init__(self, c, pooled):
        super().__init__()
        self.bn, self.pool, self.pooled = nn.BatchNorm2d(c), nn.MaxPool2d(3, 2, 1), pooled

    def forward(self, x):
        if self.pooled and self.bn.takes_node(x):
            return self.bn.forward_pooled(x)
        return self.pool(self.bn(x))


def test_module_path_statistics_counter_and_eval_mode():
    """Two training steps through forward_pooled against bn + pool: output, running statistics, num_batches_tracked and
    the gradients; in eval mode takes_node() is false and the stock modules run."""
    from mhaq_amd import bn_backward
    E = _ext()
    x, g, w, b = _node_inputs((2, 8, 17, 15))
    torch.manual_seed(5)
    ref = _Stem(8, False).to(DEV)
    with torch.no_grad():
        ref.bn.weight.copy_(w)
        ref.bn.bias.copy_(b)
    assert bn_backward.install(ref) == 1
    mine = copy.deepcopy(ref)
    mine.pooled = True
    for momentum in (0.1, None):
        ref.bn.momentum = mine.bn.momentum = momentum
        for _ in range(2):
            outs = []
            for m in (ref, mine):
                xi = x.clone().requires_grad_(True)
                m.zero_grad(set_to_none=True)
                n0 = E.bn_pool_hip_backwards()
                p = m(xi)
                p.backward(g)
                assert E.bn_pool_hip_backwards() == n0 + (1 if m is mine else 0)
                outs.append([p.detach(), xi.grad, m.bn.weight.grad, m.bn.bias.grad, m.bn.running_mean, m.bn.running_var])
            assert all(_same_bits(a, b) for a, b in zip(*outs))
            assert torch.equal(ref.bn.num_batches_tracked, mine.bn.num_batches_tracked)
    mine.eval()
    ref.eval()
    n0 = E.bn_pool_hip_backwards()
    assert not mine.bn.takes_node(x) and _same_bits(mine(x), ref(x)) and E.bn_pool_hip_backwards() == n0


def test_node_in_a_captured_graph_replays_like_eager():
    E = _ext()
    x, g, w, b = _node_inputs((2, 64, 9, 9))
    eager = _node_step(E.bn_pool_train, x, g, w, b)
    xs = x.clone().requires_grad_(True)
    ws, bs = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rm, rv = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up off the capturing stream
        E.bn_pool_train(xs, ws, bs, rm, rv, 0.1, EPS, True).backward(g)
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = ws.grad = bs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        p = E.bn_pool_train(xs, ws, bs, rm, rv, 0.1, EPS, True)
        p.backward(g)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(p, eager["p"]) and _same_bits(xs.grad, eager["dx"])
        assert _same_bits(ws.grad, eager["dw"]) and _same_bits(bs.grad, eager["db"])


# ------------------------------------------------------------------------------------------------ the trainer
def _trainer_run(stem_pool, capture):
    """The bench configuration (STE activations, AEWGS per-channel weights, distillation, channels_last) in the manner of
    tests/test_gpu_fused_blocks.py: same seeds, calibration batch and input batches for both settings of the switch."""
    import mhaq_amd as M
    from mhaq_amd import fused_blocks, nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    E = _ext()
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(8, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.AEWGS, distillation=True, warmup=2,
                    learning_rate=1e-3, fuse_stem_pool=stem_pool)
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)
    assert type(tr.net) is fused_blocks.FusedResNet18
    for m in tr.net.modules():
        if hasattr(m, "log_act_s"):
            m.Q.qnmethod = M.QNMethod.STE
    gen = torch.Generator().manual_seed(9)
    batches = []
    for _ in range(4):
        x = torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)
        batches.append((x, torch.randint(0, 10, (4,), generator=gen).to(DEV)))
    n0 = E.bn_pool_hip_backwards()
    losses = [float(tr.train_step(x, y)) for x, y in batches]
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in tr.net.parameters()], E.bn_pool_hip_backwards() - n0, tr


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "graph"])
def test_trainer_switch_on_equals_switch_off(capture):
    """Four QATTrainer steps of the quantized ResNet-18, batch 4 at 3x64x64: losses and all parameters equal."""
    l_off, p_off, taken_off, _ = _trainer_run(False, capture)
    l_on, p_on, taken_on, tr = _trainer_run(True, capture)
    assert taken_off == 0
    assert taken_on == 4 if not capture else taken_on >= 1      # (a replayed step does not pass through the node again)
    assert all(v == v for v in l_off), l_off
    assert l_on == l_off
    assert all(torch.equal(a, b) for a, b in zip(p_on, p_off))
    assert list(tr.net.state_dict().keys()) == list(copy.deepcopy(tr.net).state_dict().keys())
