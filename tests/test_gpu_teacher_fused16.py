"""GPU (-m gpu): the frozen teacher's fused forward on 16-bit tensors (mhaq_fq_bn_infer_act_x16 / mhaq_fq_bn_relu_pool3s2_x16
in csrc/bn_bwd.hip, install(model, x16=True) of mhaq_amd/frozen_blocks.py, QATConfig.fuse_teacher_16bit) through the C ABI, its
ctypes wrappers, the compiled binding, the model and the trainer, against tests/teacher_fused16_contract.py.  Per kernel:

  1. the output equals, value for value and NaN for NaN, torch's fp32 chain on the upcast inputs cast once to the dtype;
  2. |y - y64| <= u |y64| + (1 + u) 1e-6 T + s against the fp64 formula (u = 2^-8 / 2^-11, s = 0 / 2^-25 for bf16 / fp16);
  3. a sentinel-filled guard region around y stays untouched.

The framework's own 16-bit eval chain is run on the same inputs and its figure printed beside ours; nothing is asserted about
it.  Measured on an MI355X: ours at most 0.995 of the bound; the framework's chain up to 2 (bf16,
BN_RELU) and, where the residual cancels, up to 2.8e3 of it.
"""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import teacher_fused16_contract as K16
from tests import teacher_fused_contract as K
from tests.test_gpu_teacher_fused import _batches, _bn_params, _net, _nhwc, _plant

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ids = lambda s: "x".join(map(str, s))

# [M][C]: one vector; cv = 3 (256 % cv != 0: the constants are fetched again for the second vector); a tail block; the layer-1
# and layer-4 widths over several blocks
SHAPES = [(1, 8), (7, 24), (513, 64), (3 * 56 * 56, 64), (2 * 7 * 7, 512)]
# ... and one shape just above each size threshold of the launcher, with the modes that change kernel there: 20 Mi elements
# (the occupancy, every mode), 112 Mi elements of input streams (non-temporal loads: 56 Mi per stream of the two-stream modes,
# 112 Mi of BN_RELU's one)
C_BIG = 64
BIG = [(((20 << 20) // C_BIG + 4, C_BIG), K.BN_RELU), (((20 << 20) // C_BIG + 4, C_BIG), K.BN_ADD_RELU),
       (((20 << 20) // C_BIG + 4, C_BIG), K.BN2_ADD_RELU), (((56 << 20) // C_BIG + 4, C_BIG), K.BN_ADD_RELU),
       (((56 << 20) // C_BIG + 4, C_BIG), K.BN2_ADD_RELU), (((112 << 20) // C_BIG + 4, C_BIG), K.BN_RELU)]
MODES = [K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU]
MODE_IDS = ["bn_relu", "bn_add_relu", "bn2_add_relu"]
POOL_SHAPES = [(1, 1, 1, 8), (2, 2, 3, 24), (3, 7, 5, 64), (2, 112, 112, 64)]      # (N, H, W, C)
GUARD = 4096                                                                        # elements on either side of y
SENTINEL = {torch.bfloat16: 0x7B7B, torch.float16: 0x5B5B}                          # finite values no output of these cases takes

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _deterministic_miopen():
    """For the whole module: the bit-for-bit comparisons of the model and the trainer run convolutions too."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True       # MIOpen's default NHWC / wrw kernels use atomics
    yield
    torch.backends.cudnn.deterministic = det


def _case(shape, dtype):
    """Inputs and constants of one [M][C] and dtype, made once and shared by the modes (one case is held at a time)."""
    if (shape, dtype) not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        from mhaq_amd import ops
        m, c = shape
        gen = torch.Generator().manual_seed(m * 31 + c)
        dgen = torch.Generator(device=DEV).manual_seed(m * 31 + c)
        d = dict(p1=_bn_params(c, gen), p2=_bn_params(c, gen))
        for i in ("1", "2"):
            rm, rv, gamma, beta = d["p" + i]
            d["k" + i] = ops.bn_infer_consts(rm, rv, gamma, beta, 1e-5)
            d["c64_" + i] = K.consts64(rm, rv, gamma, beta, 1e-5)
        for name, at in (("x", (0, 5, 10)), ("x2", (1, 6, 11)), ("r", (2, 7, 12))):
            d[name] = (torch.randn(m, c, device=DEV, generator=dgen) * 3 + 1).to(dtype)
        if shape == (513, 64):
            # rows 64..127: the residual nearly cancels t, so rounding t to 16 bits before the add would change the result
            d["r"][64:128] = (0.37 - K._t32(d["x"][64:128].float(), d["k1"])).to(dtype)
        for name, at in (("x", (0, 5, 10)), ("x2", (1, 6, 11)), ("r", (2, 7, 12))):
            _plant(d[name], at)
        _cache[(shape, dtype)] = d
    return _cache[(shape, dtype)]


def _args(d, mode):
    x2 = d["x2"] if mode == K.BN2_ADD_RELU else None
    return dict(x2=x2, consts2=d["k2"] if mode == K.BN2_ADD_RELU else None, residual=d["r"] if mode == K.BN_ADD_RELU else None)


def _rows(y, shape):
    return y.permute(0, 2, 3, 1).reshape(shape)


def _worst16(got, y64, T):
    """The largest error in units of the bound where everything is finite (a figure to print, not a check)."""
    u, s = K16.U[got.dtype], K16.S[got.dtype]
    g = got.double()
    ok = torch.isfinite(y64) & torch.isfinite(T) & torch.isfinite(g)
    tol = u * y64.abs() + (1 + u) * K.REL * T + s
    return float(((g - y64).abs()[ok] / tol[ok].clamp_min(1e-300)).max()) if bool(ok.any()) else 0.0


def _guarded_call(d, mode, dtype):
    """The C ABI itself on a y inside a sentinel-filled buffer: (y, the two guard regions)."""
    from mhaq_amd import _lib, ops
    x = d["x"]
    m, c = x.shape
    buf = torch.full((x.numel() + 2 * GUARD,), SENTINEL[dtype], dtype=torch.int16, device=DEV)
    y = buf[GUARD:GUARD + x.numel()]
    a = _args(d, mode)
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().mhaq_fq_bn_infer_act_x16(P(x), P(d["k1"]), P(a["x2"]), P(a["consts2"]), P(a["residual"]), P(y), m, c, mode,
                                             ops._X16[dtype], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y.view(dtype).view(m, c), buf[:GUARD], buf[GUARD + x.numel():]


@pytest.mark.parametrize("dtype", K16.DTYPES, ids=K16.DT_IDS)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_elementwise_kernel_is_the_fp32_chain_rounded_once_and_within_the_bound(shape, mode, dtype):
    from mhaq_amd import _ext, ops
    E = _ext.ext()
    d = _case(shape, dtype)
    x, x2, r, k1, k2 = d["x"], d["x2"], d["r"], d["k1"], d["k2"]
    want = K16.want(x, k1, mode, r=r, x2=x2, k2=k2)
    assert bool(torch.isnan(want).any())
    if shape == (513, 64) and mode == K.BN_ADD_RELU:
        twice = K16.rounded_twice(x, k1, r)
        n_twice = int(((twice != want) & ~torch.isnan(want)).sum())
        print(f"{_ids(shape)} {dtype}: {n_twice} elements where rounding t before the add changes the result")
        assert n_twice > 100
    a = {n: None if t is None else (_nhwc(t) if t.dim() == 2 and n != "consts2" else t) for n, t in _args(d, mode).items()}
    # 1. the three routes give the expected values
    n0, n16 = E.teacher_fused_calls(), E.teacher_fused_x16_calls()
    y_ops = _rows(ops.bn_infer_act_x16(_nhwc(x), k1, mode, **a), x.shape)
    assert (E.teacher_fused_calls(), E.teacher_fused_x16_calls()) == (n0, n16)           # (ctypes: not the binding's counters)
    y_ext = E.bn_infer_act(_nhwc(x), k1, mode, x16=True, **a)
    assert y_ext.dtype == dtype and y_ext.is_contiguous(memory_format=torch.channels_last)
    assert (E.teacher_fused_calls(), E.teacher_fused_x16_calls()) == (n0 + 1, n16 + 1)
    y_abi, lo, hi = _guarded_call(d, mode, dtype)
    for y in (y_ops, _rows(y_ext, x.shape), y_abi):
        K16.same_values(y, want)
    # 3. nothing outside y was written
    assert bool((lo == SENTINEL[dtype]).all()) and bool((hi == SENTINEL[dtype]).all())
    del want
    # 2. the fp64 bound
    y64, T = K.ref64(x.float(), d["c64_1"], mode, r=r.float(), x2=x2.float(), c64_2=d["c64_2"])
    worst = K16.check16(y_ops, y64, T)
    # the framework's own 16-bit eval chain on the same inputs: recorded, not asserted
    rm, rv, gamma, beta = d["p1"]
    t = _rows(F.batch_norm(_nhwc(x), rm, rv, gamma, beta, False, 0.1, 1e-5), x.shape)
    if mode == K.BN_ADD_RELU:
        t = t + r
    elif mode == K.BN2_ADD_RELU:
        t = t + _rows(F.batch_norm(_nhwc(x2), *d["p2"], False, 0.1, 1e-5), x.shape)
    print(f"{_ids(shape)} mode {mode} {dtype}: ours {worst:.3f} of the bound, the framework's 16-bit eval chain "
          f"{_worst16(torch.relu(t), y64, T):.3f}")


@pytest.mark.parametrize("shape,mode", BIG, ids=[f"{_ids(s)}-{MODE_IDS[m]}" for s, m in BIG])
def test_elementwise_kernel_above_each_size_threshold(shape, mode):
    """bf16; value equality alone: the kernels above the thresholds differ in cache policy and occupancy, not in arithmetic."""
    from mhaq_amd import ops
    d = _case(shape, torch.bfloat16)
    x, x2, r, k1, k2 = d["x"], d["x2"], d["r"], d["k1"], d["k2"]
    a = {n: None if t is None else (_nhwc(t) if t.dim() == 2 and n != "consts2" else t) for n, t in _args(d, mode).items()}
    y = _rows(ops.bn_infer_act_x16(_nhwc(x), k1, mode, **a), x.shape)
    want = K16.want(x, k1, mode, r=r, x2=x2, k2=k2)
    K16.same_values(y, want)
    assert bool(torch.isnan(want.view(-1)[-64:]).any())                                  # the planted tail was reached


@pytest.mark.parametrize("dtype", K16.DTYPES, ids=K16.DT_IDS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_ids)
def test_pool_kernel_is_the_fp32_chain_rounded_once_and_within_the_bound(shape, dtype):
    from mhaq_amd import _ext, ops
    n, h, w, c = shape
    gen = torch.Generator().manual_seed(h * 13 + c)
    rm, rv, gamma, beta = _bn_params(c, gen)
    gamma[1] = 1.5
    x = (torch.randn(n, h, w, c, generator=gen) * 3 + 1).to(DEV).to(dtype).permute(0, 3, 1, 2)
    x[0, 1, 0:2, 0:2] = float("-inf")                          # the whole window of output (0, 0) in channel 1
    x[n - 1, 2, h - 1, w - 1] = float("nan")
    x[0, 3, h // 2, w // 2] = float("nan")
    x[n - 1, 0, 0, w - 1] = float("inf")
    x[0, 6, h - 1, 0] = float("inf")
    assert x.is_contiguous(memory_format=torch.channels_last)
    k = ops.bn_infer_consts(rm, rv, gamma, beta, 1e-5)
    want = K16.want_pool(x, k)
    p = ops.bn_relu_pool_x16(x, k)
    p_ext = _ext.ext().bn_relu_pool(x, k, x16=True)
    for got in (p, p_ext):
        assert got.dtype == dtype and got.shape == want.shape and got.is_contiguous(memory_format=torch.channels_last)
        K16.same_values(got, want)
    assert bool(torch.isnan(p).any())
    assert float(p[0, 1, 0, 0]) == 0.0                         # relu(-inf) in every position of the window
    c64 = K.consts64(rm, rv, gamma, beta, 1e-5)
    p64, T = K.ref64_pool(x.float(), c64)
    worst = K16.check16(p, p64, T)
    fw = F.max_pool2d(torch.relu(F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5)), 3, 2, 1)
    print(f"{_ids(shape)} {dtype}: ours {worst:.3f} of the bound, the framework's 16-bit eval chain {_worst16(fw, p64, T):.3f}")


def _counts():
    from mhaq_amd import _ext
    E = _ext.ext()
    return E.teacher_fused_calls(), E.teacher_fused_x16_calls()


def test_binding_refuses_what_the_kernels_cannot_take_and_routes_by_dtype():
    """x16 widens what the compiled functions take; it is not a quiet framework path, and fp32 keeps its own entry point."""
    from mhaq_amd import _ext
    E = _ext.ext()
    xf = torch.randn(2, 16, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    x = xf.bfloat16()
    k = torch.zeros(3, 16, device=DEV)
    k[1] = 1.0
    x12 = torch.randn(2, 12, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last).bfloat16()
    k12 = torch.zeros(3, 12, device=DEV)
    n0 = _counts()
    for bad, kk in ((x.contiguous(), k), (x12, k12), (x.cpu(), k), (x, k[:, :8]), (x, k.cpu()), (x[:, :8], k[:, :8].contiguous())):
        with pytest.raises(Exception):
            E.bn_infer_act(bad, kk, K.BN_RELU, x16=True)
        with pytest.raises(Exception):
            E.bn_relu_pool(bad, kk, x16=True)
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN_ADD_RELU, residual=xf, x16=True)                       # an fp32 residual beside a bf16 x
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN_ADD_RELU, residual=x.half(), x16=True)                 # ... and another 16-bit dtype
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN2_ADD_RELU, x2=xf, consts2=k, x16=True)
    with pytest.raises(Exception):
        E.bn_infer_act(xf, k, K.BN_ADD_RELU, residual=x, x16=True)
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN_ADD_RELU, residual=x[:, :, :2], x16=True)
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN_ADD_RELU, x16=True)                                    # the mode's operand is missing
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN_RELU, residual=x, x16=True)                            # ... or foreign
    for dt in (torch.bfloat16, torch.float16):                                           # without x16: refused as before
        with pytest.raises(Exception):
            E.bn_infer_act(xf.to(dt), k, K.BN_RELU)
        with pytest.raises(Exception):
            E.bn_infer_act(xf.to(dt), k, K.BN_RELU, x16=False)
        with pytest.raises(Exception):
            E.bn_relu_pool(xf.to(dt), k)
    assert _counts() == n0
    # an fp32 input with x16=True takes the fp32 entry point: the fp32 bits, and only the common counter moves
    y = E.bn_infer_act(xf, k, K.BN_RELU, x16=True)
    p = E.bn_relu_pool(xf, k, x16=True)
    assert y.dtype == torch.float32 and torch.equal(y, E.bn_infer_act(xf, k, K.BN_RELU))
    assert p.dtype == torch.float32 and torch.equal(p, E.bn_relu_pool(xf, k))
    assert _counts() == (n0[0] + 4, n0[1])
    y = E.bn_infer_act(x.half(), k, K.BN_ADD_RELU, residual=x.half(), x16=True)
    assert y.dtype == torch.float16 and _counts() == (n0[0] + 5, n0[1] + 1)


# ----------------------------------------------------------------------------- the model
def _amp():
    return torch.autocast("cuda", dtype=torch.bfloat16)


@pytest.fixture(scope="module")
def model():
    """(stock net on the device, input, stock bf16-autocast logits, fp64 CPU logits): made once, never modified."""
    from mhaq_amd import _ext
    _ext.ext()
    net = _net()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(7)).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(x.double())
        net = net.to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
        xd = x.to(DEV)
        with _amp():
            stock = net(xd)
    return net, xd, stock, ref


def _fused(net, x16=True):
    from mhaq_amd import frozen_blocks
    net = copy.deepcopy(net)
    assert frozen_blocks.install(net, x16=x16) == 9
    return net


def test_fused_bf16_logits_are_as_near_the_fp64_forward_as_the_stock_bf16_ones(model):
    """Distance = the L2 norm of the difference to the fp64 CPU forward over the 2 x 1000 logits.  Both paths are bf16: the
    reference for the margin is the stock autocast path's own distance, and the factor 2 covers only that the two round at
    different places (the fused path at a subset of the stock path's).
    Measured on an MI355X (|ref| = 173.6): stock bf16 4.945, fused bf16 1.129."""
    net, x, stock, ref = model
    n0 = _counts()
    with torch.no_grad(), _amp():
        _fused(net, x16=False)(x)                              # install(net): the stock modules under autocast, as before
        assert _counts() == n0
        fused = _fused(net)
        got = fused(x)
        assert _counts() == (n0[0] + 17, n0[1] + 17)           # 17 launches per forward, all of them 16-bit
        fused(x)
        assert _counts() == (n0[0] + 34, n0[1] + 34)
    assert got.dtype == stock.dtype
    d_stock = float((stock.double().cpu() - ref).norm())
    d_fused = float((got.double().cpu() - ref).norm())
    print(f"L2 distance to the fp64 forward (|ref| = {float(ref.norm()):.3e}): stock bf16 {d_stock:.3e}, fused bf16 {d_fused:.3e}")
    assert d_fused <= 2 * d_stock


def test_every_fallback_condition_runs_the_stock_modules_under_x16(model):
    from torch.nn.modules import module as nn_module
    net, x, stock, _ = model
    fused = _fused(net)
    n0 = _counts()
    tr = copy.deepcopy(fused).train()                          # train mode (on a copy: it moves the running statistics)
    with torch.no_grad(), _amp():
        tr(x)
    assert _counts() == n0
    g = copy.deepcopy(fused).requires_grad_(True)              # grad enabled with parameters that require it
    with _amp():
        assert g(x).requires_grad and _counts() == n0
    with torch.no_grad(), _amp():
        nchw = copy.deepcopy(fused).to(memory_format=torch.contiguous_format)      # NCHW-dense weights and input
        out = nchw(x.contiguous())
        assert _counts() == n0 and not out.isnan().any()
        h = nn_module.register_module_forward_hook(lambda m, i, o: None)          # a global hook: nothing may be bypassed
        try:
            assert torch.equal(fused(x), stock) and _counts() == n0
        finally:
            h.remove()
        # a hook on a bypassed module: that place alone runs the stock modules, hook included
        blk, stock_blk = fused.layer1[0], net.layer1[0]
        f = torch.randn(2, 64, 16, 16, device=DEV).contiguous(memory_format=torch.channels_last).bfloat16()
        want = stock_blk(f)
        seen = []
        for mod, places_left in ((blk.relu, 0), (blk.bn1, 1), (blk.bn2, 1)):
            h = mod.register_forward_hook(lambda m, i, o: seen.append(m))
            try:
                before = _counts()
                out = blk(f)
            finally:
                h.remove()
            assert _counts() == (before[0] + places_left, before[1] + places_left), type(mod).__name__
            assert seen and seen[-1] is mod
            if not places_left:
                assert torch.equal(out, want)                  # the whole stock block
        h = fused.maxpool.register_forward_pre_hook(lambda m, i: seen.append(m))
        try:
            before = _counts()
            fused(x)
        finally:
            h.remove()
        assert _counts() == (before[0] + 16, before[1] + 16) and seen[-1] is fused.maxpool      # the stem alone fell back
        # mixed dtypes: a 16-bit c2 beside an fp32 identity -- the mid-block place is fused, the block end is not
        before = _counts()
        out = blk(f.float())
        assert _counts() == (before[0] + 1, before[1] + 1) and out.dtype == torch.float32
        before = _counts()
        blk(f)
        fused(x)
        assert _counts() == (before[0] + 2 + 17, before[1] + 2 + 17)


def test_a_width_of_twelve_runs_the_stock_block_in_16_bits():
    """12 is a multiple of 4, not of 8: fused in fp32, stock under autocast."""
    from mhaq_amd import frozen_blocks, nets
    torch.manual_seed(4)
    blk = nets.BasicBlock(12, 12).eval().to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
    x = torch.randn(2, 12, 9, 9, device=DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        with _amp():
            want = blk(x.bfloat16())
        assert frozen_blocks.install(blk, x16=True) == 1
        n0 = _counts()
        with _amp():
            assert torch.equal(blk(x.bfloat16()), want)
        assert _counts() == n0
        blk(x)
        assert _counts() == (n0[0] + 2, n0[1])


def test_outside_autocast_the_flagged_model_takes_the_fp32_route(model):
    net, x, _, _ = model
    with torch.no_grad():
        want = _fused(net, x16=False)(x)
        n0 = _counts()
        got = _fused(net)(x)
    assert _counts() == (n0[0] + 17, n0[1]) and got.dtype == torch.float32 and torch.equal(got, want)


def test_load_state_dict_is_followed_under_x16(model):
    net, x, _, _ = model
    fused = _fused(net)
    other = _net(seed=11).to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
    with torch.no_grad(), _amp():
        first = fused(x)
        fused.load_state_dict(other.state_dict())
        n0 = _counts()
        got = fused(x)
        assert _counts() == (n0[0] + 17, n0[1] + 17)
        want = _fused(other)(x)                                # slabs computed from scratch
    assert torch.equal(got, want) and not torch.equal(got, first)


# ----------------------------------------------------------------------------- the trainer
_runs = {}


def _trainer(fuse16=None, capture=False, amp=True):
    """The small ResNet-18 recipe of tests/test_gpu_teacher_fused.py's _trainer under bf16 autocast; fuse16 None: the default."""
    import mhaq_amd as M
    from mhaq_amd import frozen_blocks, nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(4, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    kw = {} if fuse16 is None else dict(fuse_teacher_16bit=fuse16)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, distillation=True, warmup=2, learning_rate=1e-3,
                    fuse_teacher=True, autocast_dtype=torch.bfloat16 if amp else None, **kw)
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)
    assert type(tr.teacher) is frozen_blocks.FrozenResNet18 and type(tr.net) is not frozen_blocks.FrozenResNet18
    gs = torch.Generator().manual_seed(8)                      # statistics for the teacher to normalise with
    with torch.no_grad():
        for m in tr.teacher.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=gs) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=gs) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=gs) * 0.1)
    for m in tr.net.modules():
        if hasattr(m, "log_act_s"):
            m.Q.qnmethod = M.QNMethod.LSQ
    return tr


def _run(key, steps, **kw):
    """(losses, parameters, (fused launches, 16-bit ones), trainer) of `steps` steps, made once per key."""
    if key not in _runs:
        n0 = _counts()
        tr = _trainer(**kw)
        losses = [float(tr.train_step(x, y)) for x, y in _batches(steps)]
        n1 = _counts()
        _runs[key] = (losses, [p.detach().clone() for p in tr.net.parameters()], (n1[0] - n0[0], n1[1] - n0[1]), tr)
    return _runs[key]


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    assert all(torch.equal(p, q) for p, q in zip(a[1], b[1]))


def test_trainer_default_is_off_and_the_environment_decides(monkeypatch):
    from mhaq_amd import frozen_blocks
    monkeypatch.delenv(frozen_blocks.ENV_SWITCH_X16, raising=False)
    default = _run("stock16", 4)
    explicit = _run("explicit_false", 4, fuse16=False)
    monkeypatch.setenv(frozen_blocks.ENV_SWITCH_X16, "0")
    env_off = _run("env_off", 4, fuse16=True)
    monkeypatch.setenv(frozen_blocks.ENV_SWITCH_X16, "1")
    env_on = _run("env_on", 4, fuse16=False)
    monkeypatch.delenv(frozen_blocks.ENV_SWITCH_X16)
    for r in (default, explicit, env_off):
        assert r[2] == (0, 0) and all(v == v for v in r[0])                              # the stock teacher under autocast
        assert not any(frozen_blocks.takes_x16(m) for m in r[3].teacher.modules())
    _same(default, explicit)
    _same(default, env_off)
    assert env_on[2] == (4 * 17, 4 * 17) and frozen_blocks.takes_x16(env_on[3].teacher)
    on = _run("fused16", 6, fuse16=True)
    assert env_on[0] == on[0][:4]                                                        # the same switch by either way


def test_trainer_fuses_its_bf16_teacher_and_captured_steps_equal_eager_steps(monkeypatch):
    from mhaq_amd import frozen_blocks
    monkeypatch.delenv(frozen_blocks.ENV_SWITCH_X16, raising=False)
    eager = _run("fused16", 6, fuse16=True)
    assert eager[2] == (6 * 17, 6 * 17)                                                  # 17 16-bit launches per eager step
    graphed = _run("fused16_graph", 6, fuse16=True, capture=True)
    tr = graphed[3]
    assert tr._graph is not None
    n = (tr._eager_steps + 1) * 17                             # the settling steps and the capture; replays run no host code
    assert graphed[2] == (n, n)
    assert all(v == v and abs(v) != float("inf") for v in eager[0])
    _same(eager, graphed)


def test_trainer_bf16_loss_stays_as_near_the_fp32_run_as_with_the_stock_teacher(monkeypatch):
    """l32: the fp32 trainer of the same seeds with the fp32 fused teacher.  sum |l_fused16 - l32| <= 2 sum |l_stock16 - l32|
    over 4 steps: both sums are dominated by the student's own bf16 arithmetic, which the switch does not touch; the factor is
    the margin for the teacher's different roundings.
    Measured on an MI355X: l32 [0.42577, 0.41613, 0.39479, 0.36173], stock teacher [0.41262, 0.39531, 0.37529, 0.34695], fused
    teacher [0.42923, 0.41524, 0.39178, 0.36709]; the sums 6.83e-02 (stock) and 1.27e-02 (fused)."""
    from mhaq_amd import frozen_blocks
    monkeypatch.delenv(frozen_blocks.ENV_SWITCH_X16, raising=False)
    l32 = _run("fp32", 4, amp=False)
    assert l32[2] == (4 * 17, 0)
    ls, lf = _run("stock16", 4)[0], _run("fused16", 6, fuse16=True)[0][:4]
    print("loss, fp32 trainer:", l32[0], "bf16 with the stock teacher:", ls, "bf16 with the fused teacher:", lf)
    s_stock = sum(abs(a - b) for a, b in zip(ls, l32[0]))
    s_fused = sum(abs(a - b) for a, b in zip(lf, l32[0]))
    print(f"sum |l16 - l32|: stock teacher {s_stock:.3e}, fused teacher {s_fused:.3e}")
    assert s_fused <= 2 * s_stock
