"""GPU (-m gpu): the frozen teacher's fused forward (mhaq_fq_bn_infer_consts / _act / mhaq_fq_bn_relu_pool3s2 in
csrc/bn_bwd.hip, mhaq_amd/frozen_blocks.py) through the C ABI's ctypes wrappers, the compiled binding, the model and the
trainer, against the contract of tests/teacher_fused_contract.py.  Two properties per kernel:

  1. the output equals, bit for bit and NaN for NaN, the same fp32 constants pushed through separate torch ops;
  2. |y - y64| <= 1e-6 * T against the fp64 textbook formula, T = (|x| + |mean|) * invstd * |gamma| + |beta| (+ |r| or + T2).

The framework's own eval BatchNorm is run on the same inputs and its figure printed beside ours; nothing is asserted about it
(docs/NOTEBOOK.md section 6, "Frozen teacher").
"""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import teacher_fused_contract as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ids = lambda s: "x".join(map(str, s))

# [M][C]: one float4; cv = 3 (256 % cv != 0: the constants are fetched again for the second float4); a tail block;
# the layer-1 and layer-4 widths over several blocks; then one shape just above each size threshold of the launcher
# (kBnBigElems = 20 Mi elements: the occupancy; 56 Mi elements: the non-temporal loads of every mode)
C_BIG = 64
SHAPES = [(1, 4), (7, 12), (513, 64), (3 * 56 * 56, 64), (2 * 7 * 7, 512),
          ((20 << 20) // C_BIG + 4, C_BIG), ((56 << 20) // C_BIG + 4, C_BIG)]
MODES = [K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU]
POOL_SHAPES = [(1, 1, 1, 4), (2, 2, 3, 12), (3, 7, 5, 64), (2, 112, 112, 64)]      # (N, H, W, C)

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _deterministic_miopen():
    """For the whole module (the shared model fixture included): the bit-for-bit comparisons below run convolutions too."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True       # MIOpen's default NHWC / wrw kernels use atomics
    yield
    torch.backends.cudnn.deterministic = det


def _bn_params(c, gen):
    rm, rv = torch.randn(c, generator=gen) * 2, torch.rand(c, generator=gen) * 4 + 0.25
    gamma, beta = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    gamma[0] = 0.0                                             # a channel that BatchNorm switches off
    if c > 4:
        gamma[5] = -abs(gamma[5]) - 0.1
    return [t.to(DEV) for t in (rm, rv, gamma, beta)]


def _plant(t, at):
    """NaN, +inf and -inf into the flat tensor, near both ends."""
    flat = t.view(-1)
    n = flat.numel()
    for i, v in zip(at, (float("nan"), float("inf"), float("-inf"))):
        flat[i % n] = v
        if n > 32:
            flat[n - 1 - i] = v


def _case(shape):
    """Inputs and references of one [M][C], made once and shared by the three modes (one shape is held at a time)."""
    if shape not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        from mhaq_amd import ops
        m, c = shape
        gen = torch.Generator().manual_seed(m * 31 + c)
        dgen = torch.Generator(device=DEV).manual_seed(m * 31 + c)
        d = dict(p1=_bn_params(c, gen), p2=_bn_params(c, gen))
        for name, at in (("x", (0, 5, 10)), ("x2", (1, 6, 11)), ("r", (2, 7, 12))):
            d[name] = torch.randn(m, c, device=DEV, generator=dgen) * 3 + 1
            _plant(d[name], at)
        for i in ("1", "2"):
            rm, rv, gamma, beta = d["p" + i]
            d["k" + i] = ops.bn_infer_consts(rm, rv, gamma, beta, 1e-5)
            K.check_slab(d["k" + i].cpu(), rm.cpu(), rv.cpu(), gamma.cpu(), beta.cpu(), 1e-5)
            d["c64_" + i] = K.consts64(rm, rv, gamma, beta, 1e-5)
        _cache[shape] = d
    return _cache[shape]


def _worst(got, y64, T):
    """The largest error in units of T where everything is finite (a figure to print, not a check)."""
    ok = torch.isfinite(y64) & torch.isfinite(T) & torch.isfinite(got)
    return float(((got - y64).abs()[ok] / T[ok].clamp_min(1e-300)).max()) if bool(ok.any()) else 0.0


def _nhwc(t):
    """[M, C] rows -> a dense channels_last [1, C, M, 1] view of the same memory."""
    v = t.view(1, t.shape[0], 1, t.shape[1]).permute(0, 3, 1, 2)
    assert v.is_contiguous(memory_format=torch.channels_last) and v.data_ptr() == t.data_ptr()
    return v


@pytest.mark.parametrize("mode", MODES, ids=["bn_relu", "bn_add_relu", "bn2_add_relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_elementwise_kernel_is_the_torch_chain_and_within_the_bound(shape, mode):
    from mhaq_amd import ops
    d = _case(shape)
    x, x2, r, k1, k2 = d["x"], d["x2"], d["r"], d["k1"], d["k2"]
    y = ops.bn_infer_act(_nhwc(x), k1, mode, x2=_nhwc(x2) if mode == K.BN2_ADD_RELU else None,
                         consts2=k2 if mode == K.BN2_ADD_RELU else None,
                         residual=_nhwc(r) if mode == K.BN_ADD_RELU else None)
    y = y.permute(0, 2, 3, 1).reshape(x.shape)
    want = K.chain(x, k1, mode, r=r, x2=x2, k2=k2)
    assert torch.equal(torch.isnan(y), torch.isnan(want)) and bool(torch.isnan(y).any())
    assert torch.equal(torch.nan_to_num(y, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), \
        f"{int((torch.nan_to_num(y, nan=-1.0) != torch.nan_to_num(want, nan=-1.0)).sum())} elements differ from the torch chain"
    del want
    y64, T = K.ref64(x, d["c64_1"], mode, r=r, x2=x2, c64_2=d["c64_2"])
    worst = K.check(y, y64, T)
    # the framework's eval BatchNorm on the same inputs: recorded, not asserted
    rm, rv, gamma, beta = d["p1"]
    t = F.batch_norm(_nhwc(x), rm, rv, gamma, beta, False, 0.1, 1e-5).permute(0, 2, 3, 1).reshape(x.shape)
    if mode == K.BN_ADD_RELU:
        t = t + r
    elif mode == K.BN2_ADD_RELU:
        t = t + F.batch_norm(_nhwc(x2), *d["p2"], False, 0.1, 1e-5).permute(0, 2, 3, 1).reshape(x.shape)
    fw = torch.relu(t).double()
    print(f"{_ids(shape)} mode {mode}: ours {worst:.2e} T, the framework's eval chain {_worst(fw, y64, T):.2e} T")


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=_ids)
def test_pool_kernel_is_the_torch_chain_and_within_the_bound(shape):
    from mhaq_amd import ops
    n, h, w, c = shape
    gen = torch.Generator().manual_seed(h * 13 + c)
    rm, rv, gamma, beta = _bn_params(c, gen)
    gamma[1] = 1.5
    x = (torch.randn(n, h, w, c, generator=gen) * 3 + 1).to(DEV).permute(0, 3, 1, 2)
    x[0, 1, 0:2, 0:2] = float("-inf")                          # the whole window of output (0, 0) in channel 1
    x[n - 1, 2, h - 1, w - 1] = float("nan")
    x[0, 3, h // 2, w // 2] = float("nan")
    x[n - 1, 0, 0, w - 1] = float("inf")
    if c > 4:
        x[0, 6, h - 1, 0] = float("inf")
    k = ops.bn_infer_consts(rm, rv, gamma, beta, 1e-5)
    K.check_slab(k.cpu(), rm.cpu(), rv.cpu(), gamma.cpu(), beta.cpu(), 1e-5)
    p = ops.bn_relu_pool(x, k)
    want = K.chain_pool(x, k)
    assert p.shape == want.shape and p.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(torch.isnan(p), torch.isnan(want)) and bool(torch.isnan(p).any())
    assert torch.equal(torch.nan_to_num(p, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert float(p[0, 1, 0, 0]) == 0.0                         # relu(-inf) in every position of the window
    worst = K.check(p, *K.ref64_pool(x, K.consts64(rm, rv, gamma, beta, 1e-5)))
    fw = F.max_pool2d(torch.relu(F.batch_norm(x, rm, rv, gamma, beta, False, 0.1, 1e-5)), 3, 2, 1).double()
    p64, T = K.ref64_pool(x, K.consts64(rm, rv, gamma, beta, 1e-5))
    print(f"{_ids(shape)}: ours {worst:.2e} T, the framework's eval chain {_worst(fw, p64, T):.2e} T")


def test_binding_refuses_what_the_kernels_cannot_take():
    """The compiled functions are not a quiet framework path: an input outside the kernels' domain is an error."""
    from mhaq_amd import _ext
    E = _ext.ext()
    x = torch.randn(2, 8, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    k = torch.zeros(3, 8, device=DEV)
    n0 = E.teacher_fused_calls()
    for bad in (x.contiguous(), x.bfloat16(), x.cpu(), x[:, :6]):
        with pytest.raises(Exception):
            E.bn_infer_act(bad, k, K.BN_RELU)
        with pytest.raises(Exception):
            E.bn_relu_pool(bad, k)
    with pytest.raises(Exception):
        E.bn_infer_act(x, k[:, :4], K.BN_RELU)
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN_ADD_RELU, residual=x[:, :, :2])
    with pytest.raises(Exception):
        E.bn_infer_act(x, k, K.BN_ADD_RELU)                    # the mode's operand is missing: the library's EINVAL
    assert E.teacher_fused_calls() == n0


# ----------------------------------------------------------------------------- the model
def _net(seed=0):
    from mhaq_amd import nets
    torch.manual_seed(seed)
    net = nets.ResNet18().eval()
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            c = m.num_features
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(c, generator=g) * 0.1)
    return net


@pytest.fixture(scope="module")
def model():
    """(stock net on the device, input, stock eval logits, fp64 CPU logits): made once, never modified."""
    from mhaq_amd import _ext
    _ext.ext()
    net = _net()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(7)).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = copy.deepcopy(net).double()(x.double())
        net = net.to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
        xd = x.to(DEV)
        stock = net(xd)
    return net, xd, stock, ref


def _fused(net):
    from mhaq_amd import frozen_blocks
    net = copy.deepcopy(net)
    assert frozen_blocks.install(net) == 9
    return net


def _calls():
    from mhaq_amd import _ext
    return _ext.ext().teacher_fused_calls()


def test_fused_logits_are_as_near_the_fp64_forward_as_the_stock_ones(model):
    """Distance = the L2 norm of the difference to the fp64 CPU forward over the 2 x 1000 logits (an average over 2000 values;
    the largest single difference is one value's luck).  The fused distance may be at most twice the stock path's own: the two
    fp32 paths round differently, and that is all the factor covers."""
    net, x, stock, ref = model
    fused = _fused(net)
    n0 = _calls()
    with torch.no_grad():
        got = fused(x)
        assert _calls() - n0 == 17
        fused(x)
        assert _calls() - n0 == 34
    d_stock = float((stock.double().cpu() - ref).norm())
    d_fused = float((got.double().cpu() - ref).norm())
    print(f"L2 distance to the fp64 forward (|ref| = {float(ref.norm()):.3e}): stock {d_stock:.3e}, fused {d_fused:.3e}; "
          f"largest single difference: stock {float((stock.double().cpu() - ref).abs().max()):.3e}, "
          f"fused {float((got.double().cpu() - ref).abs().max()):.3e}")
    assert d_fused <= 2 * d_stock


def test_every_fallback_condition_runs_the_stock_modules(model):
    from torch.nn.modules import module as nn_module
    net, x, stock, _ = model
    fused = _fused(net)
    n0 = _calls()
    # train mode (on a copy: it moves the running statistics)
    tr = copy.deepcopy(fused).train()
    with torch.no_grad():
        tr(x)
    assert _calls() == n0
    # grad enabled with parameters that require it
    g = copy.deepcopy(fused).requires_grad_(True)
    assert g(x).requires_grad and _calls() == n0
    with torch.no_grad():
        # an NCHW-dense input through NCHW-dense weights
        nchw = copy.deepcopy(fused).to(memory_format=torch.contiguous_format)
        out = nchw(x.contiguous())
        assert _calls() == n0 and not out.isnan().any()
        # 16-bit activations
        with torch.autocast("cuda", dtype=torch.bfloat16):
            fused(x)
        assert _calls() == n0
        # a global hook: nothing may be bypassed
        h = nn_module.register_module_forward_hook(lambda m, i, o: None)
        try:
            assert torch.equal(fused(x), stock) and _calls() == n0
        finally:
            h.remove()
        # a hook on a bypassed module: the decision is per place, and that place runs the stock modules, hook included
        blk, stock_blk = fused.layer1[0], net.layer1[0]
        f = torch.randn(2, 64, 16, 16, device=DEV).contiguous(memory_format=torch.channels_last)
        want = stock_blk(f)
        seen = []
        for mod, places_left in ((blk.relu, 0), (blk.bn1, 1), (blk.bn2, 1)):
            h = mod.register_forward_hook(lambda m, i, o: seen.append(m))
            try:
                before = _calls()
                out = blk(f)
            finally:
                h.remove()
            assert _calls() - before == places_left and seen and seen[-1] is mod, type(mod).__name__
            if not places_left:
                assert torch.equal(out, want)                  # the whole stock block
        h = fused.maxpool.register_forward_pre_hook(lambda m, i: seen.append(m))
        try:
            before = _calls()
            fused(x)
        finally:
            h.remove()
        assert _calls() - before == 16 and seen[-1] is fused.maxpool      # the stem alone fell back
        before = _calls()
        blk(f)
        fused(x)
        assert _calls() - before == 2 + 17


def test_a_width_that_is_no_multiple_of_four_runs_the_stock_block():
    from mhaq_amd import frozen_blocks, nets
    torch.manual_seed(4)
    blk = nets.BasicBlock(6, 6).eval().to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
    x = torch.randn(2, 6, 9, 9, device=DEV).contiguous(memory_format=torch.channels_last)
    n0 = _calls()
    with torch.no_grad():
        want = blk(x)
        assert frozen_blocks.install(blk) == 1
        assert torch.equal(blk(x), want)
    assert _calls() == n0


def test_load_state_dict_is_followed(model):
    net, x, stock, _ = model
    fused = _fused(net)
    other = _net(seed=11).to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
    with torch.no_grad():
        first = fused(x)
        fused.load_state_dict(other.state_dict())
        n0 = _calls()
        got = fused(x)
        assert _calls() - n0 == 17
        want = _fused(other)(x)                                # slabs computed from scratch
        near = other(x)
    assert torch.equal(got, want) and not torch.equal(got, first)
    assert float((got - near).abs().max()) <= 1e-4 * float(near.abs().max())


# ----------------------------------------------------------------------------- the trainer
def _trainer(fuse_teacher, capture=False):
    import mhaq_amd as M
    from mhaq_amd import frozen_blocks, nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(4, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, distillation=True, warmup=2, learning_rate=1e-3,
                    fuse_teacher=fuse_teacher)
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)
    assert (type(tr.teacher) is frozen_blocks.FrozenResNet18) == fuse_teacher
    assert type(tr.net) is not frozen_blocks.FrozenResNet18
    # a fresh BatchNorm (mean 0, variance 1, gamma 1, beta 0) is x * a on either path: give the teacher statistics to normalise with
    gs = torch.Generator().manual_seed(8)
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


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last),
             torch.randint(0, 10, (4,), generator=gen).to(DEV)) for _ in range(n)]


def test_trainer_fuses_its_teacher_and_captured_steps_equal_eager_steps():
    batches = _batches(6)
    n0 = _calls()
    eager = _trainer(True)
    le = [float(eager.train_step(x, y)) for x, y in batches]
    assert _calls() - n0 == 6 * 17
    n1 = _calls()
    graphed = _trainer(True, capture=True)
    lg = [float(graphed.train_step(x, y)) for x, y in batches]
    assert graphed._graph is not None
    assert _calls() - n1 == (graphed._eager_steps + 1) * 17    # the settling steps and the capture; replays run no host code
    assert all(v == v for v in le) and le == lg
    for (n, a), (_, b) in zip(eager.net.named_parameters(), graphed.net.named_parameters()):
        assert torch.equal(a, b), n


def test_trainer_loss_stays_within_the_bound_of_the_stock_teacher():
    batches = _batches(4)
    n0 = _calls()
    stock = _trainer(False)
    ls = [float(stock.train_step(x, y)) for x, y in batches]
    assert _calls() == n0
    fused = _trainer(True)
    lf = [float(fused.train_step(x, y)) for x, y in batches]
    assert _calls() - n0 == 4 * 17
    print("loss, stock teacher:", ls, "fused teacher:", lf)
    assert all(abs(a - b) <= 2e-3 for a, b in zip(ls, lf)), (ls, lf)
