"""GPU (-m gpu): the pooled 16-bit stem node -- bn_pool_train(x16, pool_x16) in csrc/torch_binding.cpp, the module flag of
bn_backward.install(x16=True, pool_x16=True), and QATConfig.fuse_stem_pool_16bit / MHAQ_STEM_POOL_X16 in the trainer.

The yardstick of the node and the module is the composition it replaces, max_pool2d(bn_train(x, .., x16, hip_forward_x16)) with
torch's own pool forward and backward: the pooled tensor, the running statistics, num_batches_tracked, dx, dgamma and dbeta
are compared BIT FOR BIT (int16 / int32 views; NaN payloads and signed zeros count).  The pooled gradient is the one of
tests/test_gpu_stem_pool16.py: +-0, NaN, +-inf, and the sums that tell one rounding of an fp32 sum from a 16-bit add per term.
A fallback must leave the pooled counters still and give the bits of the code path that ran before the flag existed.
"""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import test_gpu_stem_pool16 as SP          # the pooled gradient and its rounding plants (helpers only)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_dt = lambda d: "bf16" if d is BF16 else "fp16"
# one window per image; ragged edges; C / 8 = 3 with odd extents; all rounding plants (7 x 9); several blocks of every kernel
SHAPES = [(2, 8, 2, 3), (3, 24, 5, 7), (2, 16, 7, 9), (3, 64, 13, 12)]
_ids = lambda s: "x".join(map(str, s))


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = det


def _E():
    from mhaq_amd import _ext
    return _ext.ext()


def _counts():
    E = _E()
    return dict(f32=E.bn_hip_forwards(), f16=E.bn_hip_forwards_x16(), b32=E.bn_hip_backwards(), b16=E.bn_hip_backwards_x16(),
                pb32=E.bn_pool_hip_backwards(), pf16=E.bn_pool_hip_forwards_x16(), pb16=E.bn_pool_hip_backwards_x16())


def _moved(before, **by):
    now = _counts()
    return all(now[k] == before[k] + by.get(k, 0) for k in now)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype in DTYPES else t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    for k in a:
        assert (a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and a[k].dtype == b[k].dtype
                                                   and a[k].shape == b[k].shape and torch.equal(_bits(a[k]), _bits(b[k]))), k
    return True


def _x(shape, dtype, seed=0):
    """Small integers (exact in both formats, ties in every window) with the strict maxima the rounding plants of the pooled
    gradient need, in every image: gamma > 0 in those channels (4 .. 7) keeps them the maxima of y."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randint(-3, 4, shape, generator=gen, device=DEV).float()
    for ch, ih, iw, _ in SP._rounding_plants(shape):
        x[:, ch, ih, iw] = 9.0
    return x.to(dtype).contiguous(memory_format=torch.channels_last)


def _params(c, seed=4):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    u = lambda lo, hi: torch.rand(c, generator=gen, device=DEV) * (hi - lo) + lo
    w = u(-1.5, 1.5)
    w[3:8] = w[3:8].abs() + 0.5
    return w, u(-1, 1), u(-1, 1), u(0.5, 1.5)            # weight, bias, running_mean, running_var


def _node_step(fn, x, g, w, b, rm, rv, grad_w=True, grad_b=True):
    x = x.clone().requires_grad_(True)
    w, b = w.clone().requires_grad_(grad_w), b.clone().requires_grad_(grad_b)
    rm, rv = rm.clone(), rv.clone()
    p = fn(x, w, b, rm, rv)
    p.backward(g)
    return dict(p=p.detach(), dx=x.grad, dw=w.grad, db=b.grad, rm=rm, rv=rv)


def _composition(x, w, b, rm, rv):
    return F.max_pool2d(_E().bn_train(x, w, b, rm, rv, 0.1, EPS, True, x16=True, hip_forward=False, hip_forward_x16=True), 3, 2, 1)


def _pooled(x, w, b, rm, rv):
    return _E().bn_pool_train(x, w, b, rm, rv, 0.1, EPS, True, hip_forward=False, x16=True, pool_x16=True)


# ------------------------------------------------------------------------------------------------ the node
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_node_equals_the_composition_bit_for_bit_and_counts_once(shape, dtype):
    x, g = _x(shape, dtype), SP._pooled_grad(shape, dtype)
    w, b, rm, rv = _params(shape[1])
    ref = _node_step(_composition, x, g, w, b, rm, rv)
    n0 = _counts()
    got = _node_step(_pooled, x, g, w, b, rm, rv)
    assert _moved(n0, pf16=1, pb16=1)                  # the pooled 16-bit routes and no other
    assert got["p"].dtype == dtype and got["dx"].dtype == dtype and got["dw"].dtype == torch.float32
    assert got["p"].is_contiguous(memory_format=torch.channels_last)
    assert _same(ref, got)
    assert not torch.equal(got["rm"], rm)              # the running statistics were updated


@pytest.mark.parametrize("frozen", ["weight", "bias", "both", "input"])
def test_node_with_a_frozen_weight_or_bias(frozen):
    shape = (3, 24, 5, 7)
    x, g = _x(shape, BF16), SP._pooled_grad(shape, BF16)
    w, b, rm, rv = _params(shape[1])
    kw = dict(grad_w=frozen not in ("weight", "both"), grad_b=frozen not in ("bias", "both"))
    if frozen == "input":
        def step(fn):
            wl, bl = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            r1, r2 = rm.clone(), rv.clone()
            p = fn(x, wl, bl, r1, r2)
            p.backward(g)
            return dict(p=p.detach(), dw=wl.grad, db=bl.grad, rm=r1, rv=r2)
        ref, n0 = step(_composition), _counts()
        got = step(_pooled)
    else:
        ref, n0 = _node_step(_composition, x, g, w, b, rm, rv, **kw), _counts()
        got = _node_step(_pooled, x, g, w, b, rm, rv, **kw)
    assert _moved(n0, pf16=1, pb16=1) and _same(ref, got)
    if frozen in ("weight", "both"):
        assert got["dw"] is None
    if frozen in ("bias", "both"):
        assert got["db"] is None


def test_node_takes_a_pooled_gradient_of_another_layout_or_dtype():
    """autograd may hand the node a gradient that is not dense NHWC (an expanded one) -- it is copied into the codes' layout."""
    shape = (2, 16, 7, 9)
    x = _x(shape, BF16)
    w, b, rm, rv = _params(shape[1])
    g = SP._pooled_grad(shape, BF16).contiguous()      # NCHW
    ref = _node_step(_composition, x, g, w, b, rm, rv)
    got = _node_step(_pooled, x, g, w, b, rm, rv)
    assert _same(ref, got)


# ------------------------------------------------------------------------------------------------ the module
def _modules(c, mine=dict(x16=True, pool_x16=True), ref=dict(x16=True, hip_forward_x16=True), **kw):
    from mhaq_amd import bn_backward
    torch.manual_seed(4)
    stock = nn.BatchNorm2d(c, **kw).to(DEV)
    with torch.no_grad():
        stock.weight.uniform_(-1.5, 1.5)
        stock.weight[3:8] = stock.weight[3:8].abs() + 0.5
        stock.bias.uniform_(-1, 1)
        stock.running_mean.uniform_(-1, 1)
        stock.running_var.uniform_(0.5, 1.5)
    a, b = copy.deepcopy(stock), copy.deepcopy(stock)
    assert bn_backward.install(a, **ref) == 1 and bn_backward.install(b, **mine) == 1
    return a, b


def _stem(bn, x):
    """What fused_blocks.FusedResNet18.forward does with its bn1 and pool."""
    return bn.forward_pooled(x) if bn.takes_pooled_node(x) else F.max_pool2d(bn(x), 3, 2, 1)


def _module_step(bn, x, g):
    x = x.clone().requires_grad_(True)
    for p in bn.parameters():
        p.grad = None
    p = _stem(bn, x)
    p.backward(g)
    own = lambda t: None if t is None else t.clone()
    return dict(p=p.detach(), dx=x.grad, dw=own(bn.weight.grad), db=own(bn.bias.grad), rm=bn.running_mean.clone(),
                rv=bn.running_var.clone(), nbt=bn.num_batches_tracked.clone())


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape", [(3, 24, 5, 7), (3, 64, 13, 12)], ids=_ids)
def test_module_with_the_flag_equals_the_unpooled_module_and_the_frameworks_pool(shape, dtype):
    x, g = _x(shape, dtype), SP._pooled_grad(shape, dtype)
    ref_bn, mine = _modules(shape[1])
    assert mine.takes_x16() and mine.takes_pool_x16() and mine.takes_pooled_node(x) and not ref_bn.takes_pooled_node(x)
    assert "_mhaq_bn_pool_x16" in mine.__dict__ and "_mhaq_bn_pool_x16" not in dict(mine.named_buffers())
    v0 = mine.running_mean._version
    for i in range(2):                                 # two steps: the second starts from the first one's running statistics
        ref = _module_step(ref_bn, x, g)
        n0 = _counts()
        got = _module_step(mine, x, g)
        assert _moved(n0, pf16=1, pb16=1)
        assert _same(ref, got) and int(got["nbt"]) == i + 1
    assert mine.running_mean._version > v0
    from mhaq_amd import bn_backward
    bn_backward.uninstall(mine)
    assert type(mine) is nn.BatchNorm2d and "_mhaq_bn_pool_x16" not in mine.__dict__


@pytest.mark.parametrize("case", ["nchw", "c_not_multiple_of_8", "fp32_input", "eval", "pool_x16_without_x16"])
def test_fallbacks_leave_the_counters_still_and_match_the_bits_from_before_the_flag(case):
    """Every case but fp32_input ends in the FRAMEWORK's 16-bit BatchNorm forward, on both sides of the comparison.  That
    forward is not fed arbitrary shapes here: on a [3,24,5,7] bf16 NCHW tensor it ended the test process with a host
    segmentation fault inside bn_train of the module WITHOUT the flag (the shape of DESIGN.md section 12c's fault; section 12f
    records two more).  The shapes below are the ones tests/test_gpu_bn_forward16.py already hands it."""
    shape = (2, 12, 4, 4) if case == "c_not_multiple_of_8" else (3, 24, 5, 5)
    x, g = _x(shape, BF16), SP._pooled_grad(shape, BF16)
    if case == "nchw":
        x, g = x.contiguous(), g.contiguous()
    if case == "fp32_input":
        x, g = x.float(), torch.nan_to_num(g.float(), nan=0.5, posinf=2.0, neginf=-2.0)
    x16 = case != "pool_x16_without_x16"
    before, mine = _modules(shape[1], mine=dict(x16=x16, pool_x16=True), ref=dict(x16=x16))
    if case == "eval":
        before, mine = before.eval(), mine.eval()
    assert mine.takes_pool_x16() and mine.takes_pooled_node(x) == (case not in ("eval", "pool_x16_without_x16"))
    ref = _module_step(before, x, g)
    n0 = _counts()
    got = _module_step(mine, x, g)
    now = _counts()
    assert now["pf16"] == n0["pf16"] and now["pb16"] == n0["pb16"] and now["f16"] == n0["f16"]
    assert _same(ref, got)
    if case == "fp32_input":
        assert now["pb32"] == n0["pb32"] + 1           # the fp32 pooled node, as before
    # the node itself under the flags of the case
    w, b, rm, rv = _params(shape[1])
    if case != "eval":
        old = lambda x, w, b, rm, rv: F.max_pool2d(_E().bn_train(x, w, b, rm, rv, 0.1, EPS, True, x16=x16), 3, 2, 1)
        new = lambda x, w, b, rm, rv: _E().bn_pool_train(x, w, b, rm, rv, 0.1, EPS, True, x16=x16, pool_x16=True)
        if case == "fp32_input":
            old = lambda x, w, b, rm, rv: _E().bn_pool_train(x, w, b, rm, rv, 0.1, EPS, True)
        a = _node_step(old, x, g, w, b, rm, rv)
        n0 = _counts()
        c = _node_step(new, x, g, w, b, rm, rv)
        now = _counts()
        assert now["pf16"] == n0["pf16"] and now["pb16"] == n0["pb16"] and _same(a, c)


def test_one_row_falls_back_to_what_ran_before():
    """N * H * W = 1 has no unbiased variance: the pooled node hands the call to the unpooled one, whatever that does with it."""
    E = _E()
    x = torch.randn(1, 8, 1, 1, device=DEV).to(BF16).contiguous(memory_format=torch.channels_last)
    w, b = torch.rand(8, device=DEV) + 0.5, torch.randn(8, device=DEV)
    outs = []
    n0 = _counts()
    for fn in (lambda rm, rv: F.max_pool2d(E.bn_train(x, w, b, rm, rv, 0.1, EPS, True, x16=True), 3, 2, 1),
               lambda rm, rv: E.bn_pool_train(x, w, b, rm, rv, 0.1, EPS, True, x16=True, pool_x16=True)):
        rm, rv = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
        try:
            outs.append((fn(rm, rv).detach(), rm, rv))
        except RuntimeError as e:
            outs.append(type(e))
    assert _counts() == n0
    if isinstance(outs[0], tuple):
        assert isinstance(outs[1], tuple) and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(*outs))
    else:
        assert outs[1] is outs[0]


def test_a_side_stream_gives_the_default_streams_bits():
    shape = (4, 64, 28, 28)
    x, g = _x(shape, BF16, seed=6), SP._pooled_grad(shape, BF16)
    _, mine = _modules(64)
    other = copy.deepcopy(mine)
    ref = _module_step(mine, x, g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    n0 = _counts()
    with torch.cuda.stream(side):
        got = _module_step(other, x, g)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert _moved(n0, pf16=1, pb16=1) and _same(ref, got)


def test_forward_and_backward_in_a_captured_graph_replay_like_eager():
    shape = (4, 64, 28, 28)
    x, g = _x(shape, BF16, seed=6), SP._pooled_grad(shape, BF16)
    _, mine = _modules(64)
    state = {k: v.clone() for k, v in mine.state_dict().items()}
    eager = [_module_step(mine, x, g) for _ in range(3)]
    mine.load_state_dict(state)
    xs = x.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # warm-up off the capturing stream
        mine.forward_pooled(xs).backward(g)
    torch.cuda.current_stream().wait_stream(side)
    mine.load_state_dict(state)
    xs.grad = mine.weight.grad = mine.bias.grad = None
    n0 = _counts()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ps = mine.forward_pooled(xs)
        ps.backward(g)
    assert _moved(n0, pf16=1, pb16=1)
    mine.load_state_dict(state)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        e = eager[k]
        assert torch.equal(_bits(ps), _bits(e["p"])) and torch.equal(_bits(xs.grad), _bits(e["dx"]))
        assert torch.equal(_bits(mine.weight.grad), _bits(e["dw"])) and torch.equal(_bits(mine.bias.grad), _bits(e["db"]))
        assert torch.equal(mine.running_mean, e["rm"]) and torch.equal(mine.running_var, e["rv"])


# ------------------------------------------------------------------------------------------------ the trainer
STEPS = 4


def _trainer(autocast=True, capture=False, **cfg_kw):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    gen = torch.Generator().manual_seed(2)
    calib = torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)
    if autocast:
        cfg_kw = dict(cfg_kw, autocast_dtype=BF16)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, distillation=True, warmup=2,
                    learning_rate=1e-3, **cfg_kw)
    return QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last),
             torch.randint(0, 10, (4,), generator=gen).to(DEV)) for _ in range(n)]


def _run(tr, batches):
    losses = [float(tr.train_step(x, y)) for x, y in batches]
    return losses, [p.detach().clone() for p in tr.net.parameters()]


def _flags(tr):
    return [(m.takes_x16(), m.takes_pool_x16()) for m in tr.net.modules() if hasattr(m, "takes_pool_x16")]


_ENVS = ("ENV_SWITCH", "ENV_SWITCH_X16", "ENV_SWITCH_FORWARD", "ENV_SWITCH_FORWARD_X16", "ENV_SWITCH_POOL_X16")
_runs = {}


def _clear_env(monkeypatch):
    from mhaq_amd import bn_backward
    for v in _ENVS:
        monkeypatch.delenv(getattr(bn_backward, v), raising=False)


def _shared(name, monkeypatch, **kw):
    """One run per configuration for the whole module, with the BatchNorm variables unset: (losses, parameters, what each
    counter moved by during the run, the per-module flags)."""
    _clear_env(monkeypatch)
    if name not in _runs:
        tr = _trainer(**kw)
        n0 = _counts()
        losses, params = _run(tr, _batches(STEPS))
        now = _counts()
        _runs[name] = (losses, params, {k: now[k] - n0[k] for k in now}, _flags(tr))
    return _runs[name]


def _equal_runs(a, b):
    return a[0] == b[0] and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))


def test_trainer_default_zero_and_false_are_one_trainer(monkeypatch):
    from mhaq_amd import bn_backward
    base = _shared("x16", monkeypatch, hip_bn_backward_16bit=True)
    assert len(base[3]) == 20 and all(a and not b for a, b in base[3])
    assert base[2]["pf16"] == 0 and base[2]["pb16"] == 0 and base[2]["b16"] == 20 * STEPS
    n0 = _counts()
    off = _run(_trainer(hip_bn_backward_16bit=True, fuse_stem_pool_16bit=False), _batches(STEPS))
    assert _equal_runs(base, off)
    monkeypatch.setenv(bn_backward.ENV_SWITCH_POOL_X16, "0")       # the variable, when set, decides either way
    tr = _trainer(hip_bn_backward_16bit=True, fuse_stem_pool_16bit=True)
    assert not any(b for _, b in _flags(tr))
    assert _equal_runs(base, _run(tr, _batches(STEPS)))
    now = _counts()
    assert now["pf16"] == n0["pf16"] and now["pb16"] == n0["pb16"]
    monkeypatch.setenv(bn_backward.ENV_SWITCH_POOL_X16, "1")
    assert all(a and b for a, b in _flags(_trainer(hip_bn_backward_16bit=True)))


def test_trainer_with_only_the_pool_switch_changes_nothing(monkeypatch):
    default = _shared("default", monkeypatch)
    only = _shared("pool_only", monkeypatch, fuse_stem_pool_16bit=True)
    assert only[2] == default[2] and only[2]["pf16"] == 0 and only[2]["pb16"] == 0 and only[2]["b16"] == 0
    assert len(only[3]) == 20 and all(b and not a for a, b in only[3])            # the flag is set; nothing takes it
    assert _equal_runs(default, only)


def test_trainer_switched_on_runs_one_pooled_forward_and_backward_per_step_and_captures(monkeypatch):
    from mhaq_amd import fused_blocks
    on = _shared("on", monkeypatch, hip_bn_backward_16bit=True, fuse_stem_pool_16bit=True)
    assert len(on[3]) == 20 and all(a and b for a, b in on[3])
    # the stem and only the stem: its backward leaves the unpooled 16-bit count, the framework's forward runs the other 19
    assert on[2] == dict(f32=0, f16=0, b32=0, b16=19 * STEPS, pb32=0, pf16=STEPS, pb16=STEPS)
    assert all(v == v and abs(v) != float("inf") for v in on[0]), on[0]
    tr = _trainer(hip_bn_backward_16bit=True, fuse_stem_pool_16bit=True, capture=True)
    assert type(tr.net) is fused_blocks.FusedResNet18
    assert not any(hasattr(m, "takes_pool_x16") for m in tr.teacher.modules())
    assert _equal_runs(on, _run(tr, _batches(STEPS)))


def test_trainer_loss_stays_as_near_the_fp32_trainers_as_the_default_bf16_run(monkeypatch):
    """At every step the loss is no farther from the fp32 trainer's on the same batches than twice the largest distance of the
    default bf16 trainer from it, plus 2e-3 (DESIGN.md section 12f's bound): both bf16 runs are one-rounding-per-tensor
    perturbations of the same step, and 2e-3 is the trajectory tolerance of DESIGN.md section 2."""
    fp32 = _shared("fp32", monkeypatch, autocast=False)[0]
    default = _shared("default", monkeypatch)[0]
    new = _shared("on", monkeypatch, hip_bn_backward_16bit=True, fuse_stem_pool_16bit=True)[0]
    d_default = [abs(a - b) for a, b in zip(default, fp32)]
    d_new = [abs(a - b) for a, b in zip(new, fp32)]
    for i in range(STEPS):
        print(f"step {i}: fp32 {fp32[i]:.9g}  default bf16 {default[i]:.9g} (off by {d_default[i]:.3e})  "
              f"pooled 16-bit stem {new[i]:.9g} (off by {d_new[i]:.3e})")
    bound = 2 * max(d_default) + 2e-3
    print(f"bound {bound:.3e}")
    assert all(v == v and abs(v) != float("inf") for v in new), new
    assert all(d <= bound for d in d_new), (d_new, bound)
