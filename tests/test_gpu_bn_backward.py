"""GPU (-m gpu): the BatchNorm backward kernels (csrc/bn_bwd.hip) through the C ABI and through the module
(mhaq_amd/bn_backward.py), against an fp64 evaluation of the closed form

    dbeta = sum dy,   dgamma = invstd * sum dy * (x - mean),
    dx = gamma * invstd * (dy - dbeta / M - xhat * dgamma / M),   xhat = (x - mean) * invstd

done on the device from the SAVED fp32 mean and invstd, upcast -- the statistics' own rounding is the forward's, not the
backward's.

Bounds.  dgamma, dbeta: 1e-6 * sum|terms|.  dx, elementwise: 1e-6 * |gamma| * invstd * (|dy| +
|dbeta| / M + |xhat| * |dgamma| / M).  Next to each, the same error figure -- the largest error in units of the bound's
term sum -- is taken for the framework's own backward (MIOpen) on the same inputs, and the new one may be at most twice
that plus a floor.  The floor is one fp32 rounding of the result, 2^-24 of the term sum: both implementations round
their result to fp32 once more than the fp64 reference does, so either can land half an ulp off where the other, by
luck, does not.  Measured on MI355X (largest figure over the shapes below, in units of the term sum): see
docs/NOTEBOOK.md section 6, "BatchNorm backward".
"""
import ctypes

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
FLOOR = 2.0 ** -24
TINY = 1e-30          # keeps 0 <= 0 comparisons of an all-zero dy from depending on the sign of a rounding

SHAPES = [(2, 4, 1, 1), (2, 64, 3, 3), (3, 20, 5, 5), (5, 512, 7, 7), (1, 8, 1, 9), (8, 64, 56, 56), (7, 4, 389, 385)]


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = det


def _inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = torch.randn(shape, generator=g) * (0.5 + torch.rand(1, c, 1, 1, generator=g) * 3) + torch.randn(1, c, 1, 1, generator=g) * 2
    dy = torch.randn(shape, generator=g)
    gamma = torch.randn(c, generator=g)
    beta = torch.randn(c, generator=g)
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)
    return cl(x), cl(dy), gamma.to(DEV), beta.to(DEV)


def _forward(x, gamma, beta):
    """The framework's training forward: (y, saved mean, saved invstd, reserve, implementation index)."""
    c = x.shape[1]
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    return torch.ops.aten._batch_norm_impl_index(x, gamma, beta, rm, rv, True, 0.1, EPS, True), rm, rv


def _stock_backward(x, dy, gamma, fwd, rm, rv):
    _, mean, invstd, reserve, impl = fwd
    return torch.ops.aten._batch_norm_impl_index_backward(impl, x, dy, gamma, rm, rv, mean, invstd, True, EPS,
                                                          [True, True, True], reserve)


def _rows(t):
    """[N, C, H, W] channels_last -> the [M, C] view the kernels walk."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _closed_form(x, dy, gamma, mean, invstd):
    X, G = _rows(x).double(), _rows(dy).double()
    mu, iv, ga = mean.double(), invstd.double(), gamma.double()
    m = X.shape[0]
    d = X - mu
    db, db_abs = G.sum(0), G.abs().sum(0)
    dg, dg_abs = iv * (G * d).sum(0), iv * (G * d).abs().sum(0)
    xh = d * iv
    dx = ga * iv * (G - db / m - xh * dg / m)
    dx_abs = ga.abs() * iv * (G.abs() + db.abs() / m + xh.abs() * dg.abs() / m)
    return dict(dx=dx, dx_abs=dx_abs, dg=dg, dg_abs=dg_abs, db=db, db_abs=db_abs)


def _hip_backward(x, dy, mean, invstd, gamma, want=(True, True, True)):
    from mhaq_amd import _lib
    L = _lib.lib()
    c = x.shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_bwd_workspace_bytes(m, c)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dx = torch.empty_like(x) if want[0] else None
    dw = torch.empty(c, device=DEV) if want[1] else None
    db = torch.empty(c, device=DEV) if want[2] else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = L.mhaq_fq_bn_bwd(p(x), p(dy), p(mean), p(invstd), p(gamma), p(dx), p(dw), p(db), m, c, p(ws), nb,
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return dx, dw, db


def _figures(got, ref, ref_abs, exact_zeros=True):
    """Largest error in units of the term sum; entries whose term sum is 0 must be exact (asked of the new kernels only)."""
    err = (got.double() - ref).abs()
    zero = ref_abs == 0
    assert not exact_zeros or bool((err[zero] == 0).all())
    return float((err[~zero] / ref_abs[~zero]).max()) if bool((~zero).any()) else 0.0


def _check(x, dy, gamma, fwd, rm, rv, label):
    _, mean, invstd, _, _ = fwd
    cf = _closed_form(x, dy, gamma, mean, invstd)
    new = _hip_backward(x, dy, mean, invstd, gamma)
    old = _stock_backward(x, dy, gamma, fwd, rm, rv)
    for name, a, b, ref, ref_abs in (("dx", _rows(new[0]), _rows(old[0]), cf["dx"], cf["dx_abs"]),
                                     ("dgamma", new[1], old[1], cf["dg"], cf["dg_abs"]),
                                     ("dbeta", new[2], old[2], cf["db"], cf["db_abs"])):
        f_new, f_old = _figures(a, ref, ref_abs), _figures(b, ref, ref_abs, exact_zeros=False)
        print(f"{label} {name}: new {f_new:.3e}  stock {f_old:.3e}  (units of the term sum)")
        assert f_new <= 1e-6, (label, name, f_new)
        assert f_new <= 2 * f_old + FLOOR, (label, name, f_new, f_old)
    return new, cf


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_c_abi_against_the_fp64_closed_form(shape):
    x, dy, gamma, beta = _inputs(shape)
    fwd, rm, rv = _forward(x, gamma, beta)
    new, _ = _check(x, dy, gamma, fwd, rm, rv, str(shape))
    # a second run gives the same bits; gamma = NULL is gamma = 1; each output is optional
    again = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    assert all(torch.equal(a, b) for a, b in zip(new, again))
    one = _hip_backward(x, dy, fwd[1], fwd[2], None)
    ones = _hip_backward(x, dy, fwd[1], fwd[2], torch.ones_like(gamma))
    assert all(torch.equal(a, b) for a, b in zip(one, ones))
    only = _hip_backward(x, dy, fwd[1], fwd[2], gamma, want=(False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1], new[1])
    only = _hip_backward(x, dy, fwd[1], fwd[2], gamma, want=(True, False, False))
    assert torch.equal(only[0], new[0])


def _planted(kind):
    shape = (3, 20, 5, 5)
    x, dy, gamma, beta = _inputs(shape, seed=5)
    if kind == "constant_channel":
        x[:, 3] = 3.0
        x[:, 7] = 0.0
    elif kind == "gamma_sign":
        gamma[0], gamma[1], gamma[2] = 0.0, -1.5, -0.0
    elif kind == "far_mean":
        x[:, 4] = 1e4 + torch.randn(3, 5, 5, generator=torch.Generator().manual_seed(6)).to(DEV)
        x[:, 9] = -1e4 + torch.randn(3, 5, 5, generator=torch.Generator().manual_seed(7)).to(DEV)
    elif kind == "zero_dy":
        dy.zero_()
    return x, dy, gamma, beta


@pytest.mark.parametrize("kind", ["constant_channel", "gamma_sign", "far_mean", "zero_dy"])
def test_planted_cases(kind):
    x, dy, gamma, beta = _planted(kind)
    fwd, rm, rv = _forward(x, gamma, beta)
    new, cf = _check(x, dy, gamma, fwd, rm, rv, kind)
    if kind == "constant_channel":
        assert float(fwd[2][7]) == pytest.approx(EPS ** -0.5, rel=1e-3)      # variance 0: invstd = eps^-1/2
        assert float(fwd[2][3]) > 100.0
    if kind == "gamma_sign":
        assert bool((new[0][:, 0] == 0).all()) and bool((new[0][:, 2] == 0).all())
    if kind == "zero_dy":
        assert all(bool((t == 0).all()) for t in new)


def test_one_nan_in_dy_poisons_its_own_channel_only():
    x, dy, gamma, beta = _inputs((3, 20, 5, 5), seed=8)
    fwd, rm, rv = _forward(x, gamma, beta)
    clean = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    dy2 = dy.clone()
    dy2[1, 6, 2, 3] = float("nan")
    got = _hip_backward(x, dy2, fwd[1], fwd[2], gamma)
    others = [c for c in range(20) if c != 6]
    assert bool(torch.isnan(got[0][:, 6]).all()) and bool(torch.isnan(got[1][6])) and bool(torch.isnan(got[2][6]))
    assert torch.equal(got[0][:, others], clean[0][:, others])
    assert torch.equal(got[1][others], clean[1][others]) and torch.equal(got[2][others], clean[2][others])


def test_misaligned_pointers_and_a_short_workspace_are_rejected():
    from mhaq_amd import _lib
    L = _lib.lib()
    x, dy, gamma, beta = _inputs((2, 64, 3, 3))
    fwd, _, _ = _forward(x, gamma, beta)
    m, c = 18, 64
    nb = L.mhaq_fq_bn_bwd_workspace_bytes(m, c)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device=DEV)
    dx = torch.empty(x.numel() + 4, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    args = [p(x), p(dy), p(fwd[1]), p(fwd[2]), p(gamma), p(dx), None, None, m, c, p(ws), nb, None]
    for k, off in ((0, 4), (1, 8), (5, 4), (10, 4)):
        bad = list(args)
        bad[k] = ctypes.c_void_p(args[k].value + off)
        assert L.mhaq_fq_bn_bwd(*bad) == -3, k
    short = list(args)
    short[11] = nb - 1
    assert L.mhaq_fq_bn_bwd(*short) == -2


@pytest.mark.parametrize("shape", [(3, 20, 5, 5), (8, 64, 56, 56), (5, 512, 7, 7)], ids=lambda s: "x".join(map(str, s)))
def test_sentinel_guards_around_dx_and_the_workspace(shape):
    from mhaq_amd import _lib
    L = _lib.lib()
    x, dy, gamma, beta = _inputs(shape)
    fwd, _, _ = _forward(x, gamma, beta)
    c = shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_bwd_workspace_bytes(m, c)
    guard = 4096                                               # bytes on either side, a multiple of 16
    sent = 0x5A
    wsbuf = torch.full((nb + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    dxbuf = torch.full((x.numel() * 4 + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    outbuf = torch.full((2 * c * 4 + 3 * 64,), sent, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = L.mhaq_fq_bn_bwd(p(x), p(dy), p(fwd[1]), p(fwd[2]), p(gamma), p(dxbuf, guard), p(outbuf, 64),
                          p(outbuf, 128 + c * 4), m, c, p(wsbuf, guard), nb,
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for buf, body in ((wsbuf, nb), (dxbuf, x.numel() * 4)):
        assert bool((buf[:guard] == sent).all()) and bool((buf[guard + body:] == sent).all())
    assert bool((outbuf[:64] == sent).all()) and bool((outbuf[64 + c * 4:128 + c * 4] == sent).all())
    assert bool((outbuf[128 + 2 * c * 4:] == sent).all())
    ref = _hip_backward(x, dy, fwd[1], fwd[2], gamma)
    assert torch.equal(dxbuf[guard:guard + x.numel() * 4].view(torch.float32), _rows(ref[0]).reshape(-1))
    assert torch.equal(outbuf[64:64 + c * 4].view(torch.float32), ref[1])


# ------------------------------------------------------------------------------------------------ the module
def _pair(c, **kw):
    from mhaq_amd import bn_backward
    torch.manual_seed(4)
    stock = nn.BatchNorm2d(c, **kw).to(DEV)
    with torch.no_grad():
        stock.weight.uniform_(-1.5, 1.5)
        stock.bias.uniform_(-1, 1)
    import copy
    mine = copy.deepcopy(stock)
    assert bn_backward.install(mine) == 1
    return stock, mine


def _step(bn, x, g):
    x = x.clone().requires_grad_(True)
    for p in bn.parameters():
        p.grad = None
    y = bn(x)
    y.backward(g)
    own = lambda t: None if t is None else t.clone()          # a later backward accumulates into .grad in place
    return dict(y=y.detach(), dx=x.grad, dw=own(bn.weight.grad), db=own(bn.bias.grad), rm=bn.running_mean.clone(),
                rv=bn.running_var.clone())


def _hip_count():
    from mhaq_amd import _ext
    return _ext.ext().bn_hip_backwards()


@pytest.mark.parametrize("shape", SHAPES[:6], ids=lambda s: "x".join(map(str, s)))
def test_module_keeps_the_forward_bits_and_runs_the_hip_backward(shape):
    x, dy, _, _ = _inputs(shape, seed=2)
    stock, mine = _pair(shape[1])
    n0 = _hip_count()
    a, b = _step(stock, x, dy), _step(mine, x, dy)
    assert _hip_count() == n0 + 1                               # never a silent fallback
    for k in ("y", "rm", "rv"):
        assert torch.equal(a[k], b[k]), k
    fwd, rm, rv = _forward(x, stock.weight.detach(), stock.bias.detach())
    cf = _closed_form(x, dy, stock.weight.detach(), fwd[1], fwd[2])
    for name, got, old, ref, ref_abs in (("dx", _rows(b["dx"]), _rows(a["dx"]), cf["dx"], cf["dx_abs"]),
                                         ("dw", b["dw"], a["dw"], cf["dg"], cf["dg_abs"]),
                                         ("db", b["db"], a["db"], cf["db"], cf["db_abs"])):
        f_new, f_old = _figures(got, ref, ref_abs), _figures(old, ref, ref_abs, exact_zeros=False)
        assert f_new <= 1e-6 and f_new <= 2 * f_old + FLOOR, (name, f_new, f_old)


@pytest.mark.parametrize("case", ["c_not_multiple_of_4", "nchw"])
def test_fallback_equals_stock_batchnorm_bit_for_bit(case):
    if case == "c_not_multiple_of_4":
        x, dy, _, _ = _inputs((2, 6, 4, 4), seed=3)
    else:
        x, dy, _, _ = _inputs((4, 8, 6, 5), seed=3)
        x, dy = x.contiguous(), dy.contiguous()
    stock, mine = _pair(x.shape[1])
    n0 = _hip_count()
    a, b = _step(stock, x, dy), _step(mine, x, dy)
    assert _hip_count() == n0
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_frozen_weight_frozen_bias_and_an_nchw_strided_dy():
    x, dy, _, _ = _inputs((3, 20, 5, 5), seed=4)
    _, mine = _pair(20)
    full = _step(mine, x, dy)
    mine.weight.requires_grad_(False)
    got = _step(mine, x, dy)
    assert got["dw"] is None and torch.equal(got["dx"], full["dx"]) and torch.equal(got["db"], full["db"])
    mine.weight.requires_grad_(True)
    mine.bias.requires_grad_(False)
    got = _step(mine, x, dy)
    assert got["db"] is None and torch.equal(got["dx"], full["dx"]) and torch.equal(got["dw"], full["dw"])
    mine.bias.requires_grad_(True)
    n0 = _hip_count()
    got = _step(mine, x, dy.contiguous())                       # the same values, NCHW strides
    assert _hip_count() == n0 + 1
    for k in ("dx", "dw", "db"):
        assert torch.equal(got[k], full[k]), k
    # eval mode, autocast's 16-bit input: the stock forward
    n0 = _hip_count()
    mine.eval()
    _step(mine, x, dy)
    mine.train()
    _step(mine, x.bfloat16(), dy.bfloat16())
    assert _hip_count() == n0


def test_forward_and_backward_in_a_captured_graph_replay_like_eager():
    x, dy, _, _ = _inputs((8, 64, 56, 56), seed=6)
    _, mine = _pair(64)
    state = {k: v.clone() for k, v in mine.state_dict().items()}
    eager = [_step(mine, x, dy) for _ in range(3)]
    mine.load_state_dict(state)
    xs = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up off the capturing stream
        mine(xs).backward(dy)
    torch.cuda.current_stream().wait_stream(side)
    mine.load_state_dict(state)
    xs.grad = mine.weight.grad = mine.bias.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = mine(xs)
        ys.backward(dy)
    mine.load_state_dict(state)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e = eager[k]
        assert torch.equal(ys, e["y"]) and torch.equal(xs.grad, e["dx"])
        assert torch.equal(mine.weight.grad, e["dw"]) and torch.equal(mine.bias.grad, e["db"])
        assert torch.equal(mine.running_mean, e["rm"]) and torch.equal(mine.running_var, e["rv"])


def test_small_net_same_loss_and_statistics_gradients_no_further_from_fp64():
    """conv -> BN -> ReLU -> conv -> BN, channels_last, no quantizers (no rounding flips): the forward is the stock one,
    so loss and running statistics are equal; each parameter gradient is no further (L2) from an fp64 run of the same net
    than twice the stock fp32 run is."""
    import copy
    from mhaq_amd import bn_backward
    torch.manual_seed(7)
    # bias-free convolutions, as in the model: a bias in front of a BatchNorm has the gradient 0, and the distance of two
    # fp32 runs from that is the ratio of two rounding noises
    net = nn.Sequential(nn.Conv2d(8, 32, 3, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                        nn.Conv2d(32, 32, 3, padding=1, bias=False), nn.BatchNorm2d(32))
    ref = copy.deepcopy(net).double()
    x = torch.randn(6, 8, 20, 20)
    t = torch.randn(6, 32, 20, 20)
    (ref(x.double()) - t.double()).square().mean().backward()
    g64 = [p.grad for p in ref.parameters()]

    def run(install):
        m = copy.deepcopy(net).to(DEV).to(memory_format=torch.channels_last)
        if install:
            assert bn_backward.install(m) == 2
        loss = (m(x.to(DEV).contiguous(memory_format=torch.channels_last)) - t.to(DEV)).square().mean()
        loss.backward()
        return loss.detach(), m
    n0 = _hip_count()
    l0, stock = run(False)
    assert _hip_count() == n0
    l1, mine = run(True)
    assert _hip_count() == n0 + 2
    assert torch.equal(l0, l1)
    for k in ("1.running_mean", "1.running_var", "4.running_mean", "4.running_var"):
        assert torch.equal(stock.state_dict()[k], mine.state_dict()[k]), k
    for (name, ps), pm, g in zip(stock.named_parameters(), mine.parameters(), g64):
        d_stock = float((ps.grad.double().cpu() - g).norm())
        d_mine = float((pm.grad.double().cpu() - g).norm())
        print(f"{name}: |g - g64| stock {d_stock:.3e}  new {d_mine:.3e}  (|g64| {float(g.norm()):.3e})")
        assert d_mine <= 2 * d_stock + TINY, (name, d_mine, d_stock)


def test_trainer_installs_next_to_the_fused_blocks_and_spares_the_checkers(monkeypatch):
    import mhaq_amd as M
    from mhaq_amd import bn_backward, nets
    from mhaq_amd.qat import QATConfig, QATTrainer
    from oracle.ref_layers import ORACLE_LAYERS

    def trainer(**kw):
        torch.manual_seed(3)
        cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, distillation=True,
                        hip_bn_backward=kw.pop("hip", True))
        return QATTrainer(nets.resnet18(10).to(memory_format=torch.channels_last), cfg, DEV, distributed=False,
                          capture_graph=False, **kw)
    count = lambda tr: sum(type(m) is bn_backward.HipBackwardBatchNorm2d for m in tr.net.modules())
    assert count(trainer()) == 20
    assert count(trainer(hip=False)) == 0
    assert count(trainer(layers=ORACLE_LAYERS)) == 0
    tr = trainer()
    assert all(type(m) is not bn_backward.HipBackwardBatchNorm2d for m in tr.teacher.modules())
    monkeypatch.setenv(bn_backward.ENV_SWITCH, "0")
    assert count(trainer()) == 0
