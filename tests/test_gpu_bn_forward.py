"""GPU (-m gpu): the opt-in HIP BatchNorm training forward (mhaq_fq_bn_fwd, csrc/bn_bwd.hip) through the C ABI, the compiled
nodes (`hip_forward` of bn_train / bn_pool_train), the module and the trainer, against the contract of
tests/bn_fwd_contract.py: an fp64 evaluation on the device of

    mean = sum x / M,  var = sum (x - mean)^2 / M,  invstd = (var + eps)^-1/2,  y = (x - mean) * invstd * gamma + beta

and of the two running-statistics formulas.  y within 1e-6 * T elementwise, T = (|x| + |mean|) * invstd * |gamma| + |beta|; the
saved statistics within one fp32 ulp of the rounded fp64 value; the running statistics within 1e-6 of their term sum.  The
framework's own forward (MIOpen) is run on the same inputs and its figures are printed beside ours; nothing is asserted about it
(docs/NOTEBOOK.md section 6, "BatchNorm forward").
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import bn_fwd_contract as K
from tests.test_gpu_bn_backward import FLOOR, _closed_form as _bwd_closed_form, _figures as _bwd_figures

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
_ids = lambda s: "x".join(map(str, s))

# the backward suite's shapes: M = 2 and one column vector; ...; cv = 5 (an idle lane, constants re-fetched); eight column
# chunks; ...; 56 row chunks; rows per block above the minimum
SHAPES = [(2, 4, 1, 1), (2, 64, 3, 3), (3, 20, 5, 5), (5, 512, 7, 7), (1, 8, 1, 9), (8, 64, 56, 56), (7, 4, 389, 385)]
# one case just above each size threshold of the launcher (csrc/bn_bwd.hip: kBnBigElems = 20 Mi elements for the occupancy of
# the normalisation, kBnFwdReduceNtElems = kBnFwdNormNtElems = 56 Mi for the cache policy): the smallest [1, 64, H, W] there
THRESHOLD_SHAPES = [(1, 64, 640, 512), (1, 64, 896, 1024)]


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = det


def _cl(x_rows, shape):
    """[M, C] rows -> the channels_last [N, C, H, W] tensor on the device with those rows."""
    n, c, h, w = shape
    return x_rows.reshape(n, h, w, c).to(DEV).permute(0, 3, 1, 2)


def _inputs(shape, kind="plain", seed=0):
    n, c, h, w = shape
    x, gamma, beta = K.planted(kind, n * h * w, c, seed)
    g = torch.Generator().manual_seed(seed + 100)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    x = _cl(x, shape)
    assert x.is_contiguous(memory_format=torch.channels_last)
    return x, gamma.to(DEV), beta.to(DEV), rm.to(DEV), rv.to(DEV)


def _hip_forward(x, gamma, beta, rm=None, rv=None, f=0.1, eps=EPS, want_y=True):
    """One call of the C ABI on copies of the running statistics: dict(y, mean, invstd, rm, rv, ws)."""
    from mhaq_amd import _lib
    L = _lib.lib()
    c = x.shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_fwd_workspace_bytes(m, c)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=DEV)
    y = torch.empty_like(x) if want_y else None
    mean, invstd = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    rm, rv = (None, None) if rm is None else (rm.clone(), rv.clone())
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = L.mhaq_fq_bn_fwd(p(x), p(gamma), p(beta), p(y), p(mean), p(invstd), p(rm), p(rv), f, eps, m, c, p(ws), nb,
                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv, ws=ws)


def _rowsed(out):
    return dict(out, y=None if out["y"] is None else K.rows(out["y"]))


def _same(a, b, keys=("y", "mean", "invstd", "rm", "rv", "ws")):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is b[k], k
        else:
            assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k
    return True


def _stock(x, gamma, beta, rm, rv, f=0.1, eps=EPS):
    rm, rv = rm.clone(), rv.clone()
    out = torch.ops.aten._batch_norm_impl_index(x, gamma, beta, rm, rv, True, f, eps, True)
    return dict(y=out[0], mean=out[1], invstd=out[2], rm=rm, rv=rv)


def _check(x, gamma, beta, rm, rv, label, f=0.1, eps=EPS, got=None):
    cf = K.closed_form(K.rows(x), gamma, beta, eps, rm, rv, f)
    got = got if got is not None else _hip_forward(x, gamma, beta, rm, rv, f, eps)
    old = _stock(x, gamma, beta, rm, rv, f, eps)
    ok = ~cf["bad"]
    fy = float(((K.rows(old["y"]).double() - cf["y"]).abs() / cf["T"].clamp_min(1e-300))[:, ok].max()) if bool(ok.any()) else 0.0
    rel = lambda a, r: float(((a.double() - r).abs()[ok] / r.abs()[ok].clamp_min(1e-300)).max()) if bool(ok.any()) else 0.0
    print(f"{label}: miopen  y {fy:.3e} T  mean {rel(old['mean'], cf['mean']):.3e}  invstd {rel(old['invstd'], cf['invstd']):.3e}")
    fig = K.check_all(_rowsed(got), cf)
    print(f"{label}: new     " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    return got, cf


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_c_abi_against_the_fp64_closed_form(shape):
    x, gamma, beta, rm, rv = _inputs(shape)
    got, _ = _check(x, gamma, beta, rm, rv, str(shape))
    # determinism: equal bits in y, the statistics and the whole workspace
    assert _same(got, _hip_forward(x, gamma, beta, rm, rv))
    # weight NULL = 1, bias NULL = 0; no running statistics and no y change nothing else
    assert _same(_hip_forward(x, None, beta, rm, rv), _hip_forward(x, torch.ones_like(gamma), beta, rm, rv))
    assert _same(_hip_forward(x, gamma, None, rm, rv), _hip_forward(x, gamma, torch.zeros_like(beta), rm, rv))
    assert _same(_hip_forward(x, gamma, beta), got, keys=("y", "mean", "invstd", "ws"))
    stats = _hip_forward(x, gamma, beta, rm, rv, want_y=False)
    assert stats["y"] is None and _same(stats, got, keys=("mean", "invstd", "rm", "rv", "ws"))


@pytest.mark.parametrize("shape", THRESHOLD_SHAPES, ids=_ids)
def test_just_above_each_size_threshold(shape):
    n, c, h, w = shape
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(n, h, w, c, device=DEV, generator=gen).mul_(2).add_(1).permute(0, 3, 1, 2)
    gamma, beta = torch.randn(c, device=DEV, generator=gen), torch.randn(c, device=DEV, generator=gen)
    rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
    got = _hip_forward(x, gamma, beta, rm, rv)
    cf = K.closed_form(K.rows(x), gamma, beta, EPS, rm, rv, 0.1)
    print(shape, K.check_all(_rowsed(got), cf))


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("kind", ["far_mean", "constant_channel", "outlier", "tiny_sigma", "gamma_sign"])
@pytest.mark.parametrize("shape", [(3, 20, 5, 5), (8, 64, 56, 56)], ids=_ids)
def test_planted_cases(shape, kind, eps):
    x, gamma, beta, rm, rv = _inputs(shape, kind, seed=5)
    got, cf = _check(x, gamma, beta, rm, rv, f"{shape} {kind} eps={eps}", eps=eps)
    if kind == "constant_channel":
        c = shape[1]
        for ch, val in ((1, 3.0), (c - 1, 0.0)):
            assert float(got["mean"][ch]) == val                                     # the constant exactly
            assert float(got["invstd"][ch]) == float(torch.tensor(eps, dtype=torch.float64).rsqrt().float())   # var == 0
            assert bool((got["y"][:, ch] == beta[ch]).all())                         # y == beta bit for bit
            assert float(got["rv"][ch]) == float((0.9 * rv[ch].double()).float())    # ... and adds 0 to the running variance
    if kind == "gamma_sign":
        assert bool((got["y"][:, 0] == beta[0]).all()) and bool((got["y"][:, 2] == beta[2]).all())


@pytest.mark.parametrize("f", [0.1, 1.0, 0.0, 1.0 / 3], ids=lambda f: f"f={f:.3g}")
def test_running_statistics_follow_the_factor(f):
    x, gamma, beta, rm, rv = _inputs((3, 20, 5, 5), seed=7)
    got, _ = _check(x, gamma, beta, rm, rv, f"f={f}", f=f)
    if f == 0.0:
        assert torch.equal(got["rm"], rm) and torch.equal(got["rv"], rv)
    # M = 2: the unbiased factor M / (M - 1) = 2
    x, gamma, beta, rm, rv = _inputs((2, 4, 1, 1), seed=7)
    _check(x, gamma, beta, rm, rv, f"M=2 f={f}", f=f)


def test_one_nan_in_x_poisons_its_own_channel_only():
    x, gamma, beta, rm, rv = _inputs((3, 20, 5, 5), seed=8)
    clean = _hip_forward(x, gamma, beta, rm, rv)
    # one NaN; then a NaN, an infinity, and an infinity in row 0 (the shift of its channel) in three channels
    for plant in ({(1, 6, 2, 3): float("nan")},
                  {(1, 6, 2, 3): float("nan"), (2, 9, 4, 1): float("inf"), (0, 13, 0, 0): float("-inf")}):
        x2 = x.clone()
        for at, v in plant.items():
            x2[at] = v
        bad = sorted(at[1] for at in plant)
        others = [c for c in range(20) if c not in bad]
        got, _ = _check(x2, gamma, beta, rm, rv, f"non-finite in channels {bad}")
        for ch in bad:
            assert bool(torch.isnan(got["y"][:, ch]).all()) and not bool(torch.isfinite(got["mean"][ch]))
            assert bool(torch.isnan(got["invstd"][ch])) and not bool(torch.isfinite(got["rv"][ch]))
        for k in ("mean", "invstd", "rm", "rv"):
            assert torch.equal(got[k][others], clean[k][others]), k
        assert torch.equal(got["y"][:, others], clean["y"][:, others])


def test_argument_errors_leave_the_outputs_untouched():
    from mhaq_amd import _lib
    L = _lib.lib()
    x, gamma, beta, rm, rv = _inputs((2, 64, 3, 3))
    m, c = 18, 64
    nb = L.mhaq_fq_bn_fwd_workspace_bytes(m, c)
    sent = 0x5A
    ws = torch.full((nb + 16,), sent, dtype=torch.uint8, device=DEV)
    y = torch.full((x.numel() * 4 + 16,), sent, dtype=torch.uint8, device=DEV)
    outs = torch.full((4, c * 4 + 16), sent, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    args = [p(x), p(gamma), p(beta), p(y), p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), 0.1, EPS, m, c, p(ws), nb, None]
    for k, off in ((0, 4), (3, 4), (12, 8), (1, 2), (4, 2), (7, 1)):
        bad = list(args)
        bad[k] = ctypes.c_void_p(args[k].value + off)
        assert L.mhaq_fq_bn_fwd(*bad) == -3, k
    short = list(args)
    short[13] = nb - 1
    assert L.mhaq_fq_bn_fwd(*short) == -2
    one = list(args)
    one[10] = 1
    assert L.mhaq_fq_bn_fwd(*one) == -4
    lone = list(args)
    lone[7] = None
    assert L.mhaq_fq_bn_fwd(*lone) == -1
    torch.cuda.synchronize()
    assert all(bool((t == sent).all()) for t in (ws, y, outs))


@pytest.mark.parametrize("shape", [(3, 20, 5, 5), (8, 64, 56, 56), (5, 512, 7, 7)], ids=_ids)
def test_sentinel_guards_around_every_output_and_the_workspace(shape):
    from mhaq_amd import _lib
    L = _lib.lib()
    x, gamma, beta, rm, rv = _inputs(shape)
    c = shape[1]
    m = x.numel() // c
    nb = L.mhaq_fq_bn_fwd_workspace_bytes(m, c)
    guard, sent = 4096, 0x5A
    wsbuf = torch.full((nb + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    ybuf = torch.full((x.numel() * 4 + 2 * guard,), sent, dtype=torch.uint8, device=DEV)
    out = torch.full((4, c * 4 + 128), sent, dtype=torch.uint8, device=DEV)          # 64 guard bytes around each [c] vector
    out[2, 64:64 + c * 4] = rm.view(torch.uint8)
    out[3, 64:64 + c * 4] = rv.view(torch.uint8)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    rc = L.mhaq_fq_bn_fwd(p(x), p(gamma), p(beta), p(ybuf, guard), p(out[0], 64), p(out[1], 64), p(out[2], 64), p(out[3], 64),
                          0.1, EPS, m, c, p(wsbuf, guard), nb, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for buf, body in ((wsbuf, nb), (ybuf, x.numel() * 4)):
        assert bool((buf[:guard] == sent).all()) and bool((buf[guard + body:] == sent).all())
    assert bool((out[:, :64] == sent).all()) and bool((out[:, 64 + c * 4:] == sent).all())
    ref = _hip_forward(x, gamma, beta, rm, rv)
    assert torch.equal(ybuf[guard:guard + x.numel() * 4].view(torch.float32), K.rows(ref["y"]).reshape(-1))
    for i, k in enumerate(("mean", "invstd", "rm", "rv")):
        assert torch.equal(out[i, 64:64 + c * 4].contiguous().view(torch.float32), ref[k]), k
    assert torch.equal(wsbuf[guard:guard + nb], ref["ws"])


def test_ops_wrapper_is_the_c_abi_call_and_never_falls_back():
    from mhaq_amd import _lib, ops
    x, gamma, beta, rm, rv = _inputs((3, 20, 5, 5), seed=12)
    ref = _hip_forward(x, gamma, beta, rm, rv)
    rm2, rv2 = rm.clone(), rv.clone()
    y, mean, invstd = ops.bn_forward_train(x, gamma, beta, rm2, rv2, 0.1, EPS)
    assert _same(dict(y=y, mean=mean, invstd=invstd, rm=rm2, rv=rv2), ref, keys=("y", "mean", "invstd", "rm", "rv"))
    y, mean, invstd = ops.bn_forward_train(x)
    assert _same(dict(y=y, mean=mean, invstd=invstd), _hip_forward(x, None, None), keys=("y", "mean", "invstd"))
    with pytest.raises(_lib.MhaqFqError):                       # C % 4 != 0: an error, not another implementation
        ops.bn_forward_train(_inputs((2, 6, 4, 4))[0])


# ------------------------------------------------------------------------------------------------ nodes and module
def _E():
    from mhaq_amd import _ext
    return _ext.ext()


def _pair(c, hip_forward=True, **kw):
    from mhaq_amd import bn_backward
    torch.manual_seed(4)
    stock = nn.BatchNorm2d(c, **kw).to(DEV)
    with torch.no_grad():
        stock.weight.uniform_(-1.5, 1.5)
        stock.bias.uniform_(-1, 1)
        stock.running_mean.uniform_(-1, 1)
        stock.running_var.uniform_(0.5, 1.5)
    mine = copy.deepcopy(stock)
    assert bn_backward.install(mine, hip_forward=hip_forward) == 1
    return stock, mine


def _step(bn, x, g):
    x = x.clone().requires_grad_(True)
    for p in bn.parameters():
        p.grad = None
    y = bn(x)
    y.backward(g)
    own = lambda t: None if t is None else t.clone()
    return dict(y=y.detach(), dx=x.grad, dw=own(bn.weight.grad), db=own(bn.bias.grad), rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())


def _dy(shape, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("shape", SHAPES[:6], ids=_ids)
def test_module_with_the_flag_holds_the_contract_and_feeds_the_hip_backward(shape):
    x = _inputs(shape, seed=2)[0]
    dy = _dy(shape)
    stock, mine = _pair(shape[1])
    E = _E()
    n0, b0 = E.bn_hip_forwards(), E.bn_hip_backwards()
    rm, rv = mine.running_mean.clone(), mine.running_var.clone()
    v0 = mine.running_mean._version
    got = _step(mine, x, dy)
    assert E.bn_hip_forwards() == n0 + 1 and E.bn_hip_backwards() == b0 + 1          # never a silent fallback
    assert mine.running_mean._version > v0                                           # the in-place update is visible
    gamma, beta = mine.weight.detach(), mine.bias.detach()
    direct = _hip_forward(x, gamma, beta, rm, rv)
    assert torch.equal(got["y"], direct["y"]) and torch.equal(got["rm"], direct["rm"]) and torch.equal(got["rv"], direct["rv"])
    K.check_all(_rowsed(dict(direct, y=got["y"])), K.closed_form(K.rows(x), gamma, beta, EPS, rm, rv, 0.1))
    # the backward, evaluated from the statistics the HIP forward saved, within the backward suite's bounds
    cf = _bwd_closed_form(x, dy, gamma, direct["mean"], direct["invstd"])
    old = _step(stock, x, dy)
    for name, a, b, ref, ref_abs in (("dx", K.rows(got["dx"]), K.rows(old["dx"]), cf["dx"], cf["dx_abs"]),
                                     ("dw", got["dw"], old["dw"], cf["dg"], cf["dg_abs"]),
                                     ("db", got["db"], old["db"], cf["db"], cf["db_abs"])):
        f_new = _bwd_figures(a, ref, ref_abs)
        assert f_new <= 1e-6, (name, f_new)
    assert torch.equal(got["nbt"], old["nbt"])


@pytest.mark.parametrize("shape", [(3, 20, 5, 5), (8, 64, 56, 56)], ids=_ids)
def test_flag_off_is_todays_module_bit_for_bit(shape):
    x = _inputs(shape, seed=2)[0]
    dy = _dy(shape)
    stock, mine = _pair(shape[1], hip_forward=False)
    E = _E()
    n0 = E.bn_hip_forwards()
    for _ in range(2):
        a, b = _step(stock, x, dy), _step(mine, x, dy)
        for k in ("y", "rm", "rv", "nbt"):
            assert torch.equal(a[k], b[k]), k
    assert E.bn_hip_forwards() == n0
    # ... and the node without the argument is the node with hip_forward=False
    outs = []
    for more in ((), (False, False)):
        xi = x.clone().requires_grad_(True)
        w, bb = stock.weight.detach().clone().requires_grad_(True), stock.bias.detach().clone().requires_grad_(True)
        rm, rv = torch.zeros_like(w), torch.ones_like(w)
        y = E.bn_train(xi, w, bb, rm, rv, 0.1, EPS, True, *more)
        y.backward(dy)
        outs.append((y.detach(), xi.grad, w.grad, bb.grad, rm, rv))
    assert all(torch.equal(p, q) for p, q in zip(*outs)) and E.bn_hip_forwards() == n0


@pytest.mark.parametrize("case", ["nchw", "c_not_multiple_of_4", "bf16"])
def test_fallbacks_equal_the_frameworks_forward_bit_for_bit(case):
    shape = {"nchw": (4, 8, 6, 5), "c_not_multiple_of_4": (2, 6, 4, 4), "bf16": (3, 24, 5, 5)}[case]
    x, dy = _inputs(shape, seed=3)[0], _dy(shape)
    if case == "nchw":
        x, dy = x.contiguous(), dy.contiguous()
    if case == "bf16":
        x, dy = x.bfloat16(), dy.bfloat16()
    stock, mine = _pair(shape[1])
    E = _E()
    n0 = E.bn_hip_forwards()
    a, b = _step(stock, x, dy), _step(mine, x, dy)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert E.bn_hip_forwards() == n0


@pytest.mark.parametrize("momentum", [0.1, 0.3, None])
def test_bookkeeping_equals_the_stock_modules(momentum):
    """num_batches_tracked counts alike, and momentum=None hands the kernels the cumulative factor 1 / n."""
    shape = (3, 20, 5, 5)
    stock, mine = _pair(20, momentum=momentum)
    rm, rv = mine.running_mean.clone(), mine.running_var.clone()
    for i in range(3):
        x, dy = _inputs(shape, seed=20 + i)[0], _dy(shape, seed=30 + i)
        a, b = _step(stock, x, dy), _step(mine, x, dy)
        assert torch.equal(a["nbt"], b["nbt"]) and int(b["nbt"]) == i + 1
        f = 1.0 / (i + 1) if momentum is None else momentum
        cf = K.closed_form(K.rows(x), None, None, EPS, rm, rv, f, want_y=False)
        K.check_running(b["rm"], cf["rm"], cf["rm_abs"], cf["bad"], "running_mean")
        K.check_running(b["rv"], cf["rv"], cf["rv_abs"], cf["bad"], "running_var")
        rm, rv = b["rm"], b["rv"]
    mine.eval()                                                  # eval mode: the stock forward, from the HIP running statistics
    n0 = _E().bn_hip_forwards()
    ye = mine(x)
    assert _E().bn_hip_forwards() == n0
    assert torch.equal(ye, F.batch_norm(x, mine.running_mean, mine.running_var, mine.weight, mine.bias, False, 0.0, EPS))


@pytest.mark.parametrize("shape", [(2, 8, 5, 7), (4, 64, 56, 56), (1, 4, 1, 2)], ids=_ids)
def test_pooled_node_is_max_pool2d_of_the_hip_forward(shape):
    x, gamma, beta, rm0, rv0 = _inputs(shape, seed=4)
    E = _E()
    outs = []
    gp = None
    for fn in (lambda *a: F.max_pool2d(E.bn_train(*a, 0.1, EPS, True, False, True), 3, 2, 1),
               lambda *a: E.bn_pool_train(*a, 0.1, EPS, True, True)):
        xi, w, b = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rm, rv = rm0.clone(), rv0.clone()
        n0, p0 = E.bn_hip_forwards(), E.bn_pool_hip_backwards()
        p = fn(xi, w, b, rm, rv)
        assert E.bn_hip_forwards() == n0 + 1
        gp = _dy(tuple(p.shape), seed=5) if gp is None else gp
        p.backward(gp)
        outs.append((p.detach(), xi.grad, w.grad, b.grad, rm, rv))
    assert E.bn_pool_hip_backwards() == p0 + 1
    direct = _hip_forward(x, gamma, beta, rm0, rv0)
    assert torch.equal(outs[1][0], F.max_pool2d(direct["y"], 3, 2, 1))
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a, b), k


def test_forward_and_backward_in_a_captured_graph_replay_like_eager():
    shape = (8, 64, 56, 56)
    x, dy = _inputs(shape, seed=6)[0], _dy(shape)
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
    n0 = _E().bn_hip_forwards()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = mine(xs)
        ys.backward(dy)
    assert _E().bn_hip_forwards() == n0 + 1
    mine.load_state_dict(state)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e = eager[k]
        assert torch.equal(ys, e["y"]) and torch.equal(xs.grad, e["dx"])
        assert torch.equal(mine.weight.grad, e["dw"]) and torch.equal(mine.bias.grad, e["db"])
        assert torch.equal(mine.running_mean, e["rm"]) and torch.equal(mine.running_var, e["rv"])


# ------------------------------------------------------------------------------------------------ the trainer
STEPS = 4


def _trainer(hip_forward=None, capture=False, **more):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(4, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    kw = {} if hip_forward is None else dict(hip_bn_forward=hip_forward)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, distillation=True, warmup=2,
                    learning_rate=1e-3, **kw)
    return QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture, **more)


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last),
             torch.randint(0, 10, (4,), generator=gen).to(DEV)) for _ in range(n)]


def _run(tr, batches):
    losses = [float(tr.train_step(x, y)) for x, y in batches]
    return losses, [p.detach().clone() for p in tr.net.parameters()]


def _flags(tr):
    return [m.takes_hip_forward() for m in tr.net.modules() if hasattr(m, "takes_hip_forward")]


def test_trainer_default_is_off_and_equals_the_explicit_off(monkeypatch):
    from mhaq_amd import bn_backward
    from oracle.ref_layers import ORACLE_LAYERS
    monkeypatch.delenv(bn_backward.ENV_SWITCH_FORWARD, raising=False)
    batches = _batches(STEPS)
    E = _E()
    n0 = E.bn_hip_forwards()
    tr = _trainer()
    assert len(_flags(tr)) == 20 and not any(_flags(tr))
    default = _run(tr, batches)
    monkeypatch.setenv(bn_backward.ENV_SWITCH_FORWARD, "0")
    off = _run(_trainer(), batches)
    assert E.bn_hip_forwards() == n0
    assert default[0] == off[0] and all(torch.equal(a, b) for a, b in zip(default[1], off[1]))
    # the environment decides when it is set, either way; checker trainers and the teacher are spared
    assert not any(_flags(_trainer(hip_forward=True)))
    monkeypatch.setenv(bn_backward.ENV_SWITCH_FORWARD, "1")
    tr = _trainer()
    assert len(_flags(tr)) == 20 and all(_flags(tr))
    assert not any(hasattr(m, "takes_hip_forward") for m in tr.teacher.modules())
    assert _flags(_trainer(layers=ORACLE_LAYERS)) == []


def test_trainer_with_the_hip_forward(monkeypatch):
    from mhaq_amd import bn_backward
    monkeypatch.delenv(bn_backward.ENV_SWITCH_FORWARD, raising=False)
    batches = _batches(STEPS)
    default = _run(_trainer(), batches)
    tr = _trainer(hip_forward=True)
    assert len(_flags(tr)) == 20 and all(_flags(tr))
    E = _E()
    n0 = E.bn_hip_forwards()
    eager = _run(tr, batches)
    assert E.bn_hip_forwards() == n0 + 20 * STEPS                # every student BatchNorm, the stem's included, every step
    for i, (a, b) in enumerate(zip(eager[0], default[0])):
        print(f"step {i}: loss with the HIP forward {a:.9g}  default {b:.9g}  difference {abs(a - b):.3e}")
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (i, a, b)
    graphed = _run(_trainer(hip_forward=True, capture=True), batches)
    assert eager[0] == graphed[0] and all(torch.equal(a, b) for a, b in zip(eager[1], graphed[1]))
