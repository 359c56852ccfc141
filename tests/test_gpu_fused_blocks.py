"""GPU (-m gpu): mhaq_amd/fused_blocks.py -- ReLU and residual add of nets.BasicBlock and the nets.ResNet18 stem inside
the activation quantizer's kernels.  The fusions are exact, so a trainer with fuse_blocks=True must leave EXACTLY the
parameters and losses of one with fuse_blocks=False from the same seeds (MIOpen held to its deterministic kernels), in
eager steps and in hipGraph replays; the decision to fuse is per call and per place, and hooks, eval mode and calibration
see the original modules."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True       # MIOpen's default NHWC / wrw kernels use atomics
    yield
    torch.backends.cudnn.deterministic = det


@pytest.fixture
def fused_calls(monkeypatch):
    """How many quantizers took forward_fused, and which."""
    from mhaq_amd.layers import NoisyAct
    calls = []
    inner = NoisyAct.forward_fused

    def counting(self, z, addend=None, want_act=False):
        calls.append((self, addend is not None, want_act))
        return inner(self, z, addend, want_act)
    monkeypatch.setattr(NoisyAct, "forward_fused", counting)
    return calls


def _trainer(fuse, layout, act_method, w_method, distillation, capture=False):
    import mhaq_amd as M
    from mhaq_amd import fused_blocks, nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(8, 3, 64, 64, generator=g).to(DEV)
    if layout == "channels_last":
        net = net.to(memory_format=torch.channels_last)
        calib = calib.contiguous(memory_format=torch.channels_last)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod[w_method], distillation=distillation, warmup=2,
                    learning_rate=1e-3, fuse_blocks=fuse)
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)
    assert (type(tr.net) is fused_blocks.FusedResNet18) == fuse
    for m in tr.net.modules():
        if hasattr(m, "log_act_s"):
            m.Q.qnmethod = M.QNMethod[act_method]
    return tr


def _batches(n, layout):
    gen = torch.Generator().manual_seed(9)
    out = []
    for _ in range(n):
        x = torch.randn(8, 3, 64, 64, generator=gen).to(DEV)
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        out.append((x, torch.randint(0, 10, (8,), generator=gen).to(DEV)))
    return out


@pytest.mark.parametrize("act_method,w_method,distillation,layout", [
    ("STE", "AEWGS", True, "channels_last"),        # the bench configuration
    ("STE", "AEWGS", True, "nchw"),
    ("LSQ", "LSQ", False, "channels_last"),
    ("LSQ", "LSQ", True, "nchw"),
])
def test_fused_trainer_equals_unfused_trainer(act_method, w_method, distillation, layout, fused_calls):
    batches = _batches(4, layout)
    plain = _trainer(False, layout, act_method, w_method, distillation)
    lp = [float(plain.train_step(x, y)) for x, y in batches]
    assert not fused_calls
    fused = _trainer(True, layout, act_method, w_method, distillation)
    lf = [float(fused.train_step(x, y)) for x, y in batches]
    # every one of the 16 quantizers is served by a fused kernel: 8 mid-block, 7 block ends, the stem
    assert len(fused_calls) == 4 * 16
    assert sum(1 for _, add, _ in fused_calls if add) == 4 * 7
    assert sum(1 for _, add, want in fused_calls if want and not add) == 4 * 1
    assert all(v == v for v in lp), lp
    assert lf == lp
    changed = False
    for (n, a), (_, b) in zip(plain.net.named_parameters(), fused.net.named_parameters()):
        assert torch.equal(a, b), n
    for p0, p1 in zip(_trainer(False, layout, act_method, w_method, distillation).net.parameters(),
                      fused.net.parameters()):
        changed = changed or not torch.equal(p0, p1)
    assert changed                                   # (the four steps did train)


def test_replayed_fused_steps_equal_eager_fused_steps(fused_calls):
    from mhaq_amd import ops
    batches = _batches(6, "channels_last")
    eager = _trainer(True, "channels_last", "STE", "AEWGS", True, capture=False)
    le = [float(eager.train_step(x, y)) for x, y in batches]
    n_eager = len(fused_calls)
    graphed = _trainer(True, "channels_last", "STE", "AEWGS", True, capture=True)
    lg = [float(graphed.train_step(x, y)) for x, y in batches]
    assert graphed._graph is not None and graphed._eager_steps == 3
    assert n_eager == 6 * 16 and len(fused_calls) - n_eager == 4 * 16      # 3 settling steps + the capture
    assert le == lg
    for (n, a), (_, b) in zip(eager.net.named_parameters(), graphed.net.named_parameters()):
        assert torch.equal(a, b), n
    assert ops.rng.offset_base is None


def _model(act_method="LSQ", w_method="LSQ"):
    import mhaq_amd as M
    from mhaq_amd import nets, wrap
    torch.manual_seed(21)
    net = nets.resnet18(10).to(DEV).to(memory_format=torch.channels_last)
    wrap.quantize_model(net, M.QScheme.PER_CHANNEL, M.QNMethod[w_method], ("conv1", "fc"), False, 4)
    net.to(DEV)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "log_act_s"):
                m.log_act_s.fill_(-5.3); m.log_act_q.fill_(3.4); m.act_b.fill_(-3.1 if m.signed else 0.0)
                m.Q.qnmethod = M.QNMethod[act_method]
            if hasattr(m, "log_wght_s"):
                m.log_wght_s.fill_(-9.2)
    return net.train()


def _step(net, x, y):
    from mhaq_amd import ops
    ops.manual_seed(31)
    net.zero_grad(set_to_none=True)
    out = net(x)
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    return out.detach(), loss.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


def _assert_same_step(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for n in a[2]:
        assert torch.equal(a[2][n], b[2][n]), n


def _xy():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(8, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    return x, torch.randint(0, 10, (8,), generator=g).to(DEV)


@pytest.mark.parametrize("act_method", ["STE", "LSQ"])
def test_stem_reorder_alone_equals_the_original_order(act_method, fused_calls):
    """maxpool(relu(t)) against relu(maxpool(t)) inside layer1.0's first quantizer, with every other place held unfused
    (a hook on each block's ReLU): logits, loss and every gradient -- conv1 and bn1 of the stem included -- are equal."""
    from mhaq_amd import fused_blocks, nets
    plain = _model(act_method)
    fused = copy.deepcopy(plain)
    assert fused_blocks.install(fused) == 9
    handles = [m.relu.register_forward_hook(lambda mod, inp, out: None) for m in fused.modules()
               if isinstance(m, nets.BasicBlock)]
    x, y = _xy()
    ref = _step(plain, x, y)
    got = _step(fused, x, y)
    assert len(fused_calls) == 1 and fused_calls[0][0] is fused.layer1[0].conv1.activations_quantizer
    _assert_same_step(got, ref)
    assert "conv1.weight" in got[2] and "bn1.weight" in got[2]
    for h in handles:
        h.remove()
    fused_calls.clear()
    _assert_same_step(_step(fused, x, y), ref)       # and with every place fused
    assert len(fused_calls) == 16


def test_hooks_take_their_place_back_to_the_original_modules(fused_calls):
    from mhaq_amd import fused_blocks
    from tests.teacher_forced import Recorder
    plain = _model()
    fused = copy.deepcopy(plain)
    fused_blocks.install(fused)
    x, y = _xy()
    ref = _step(plain, x, y)
    seen = []
    h1 = fused.layer2[0].conv2.activations_quantizer.register_forward_hook(lambda m, i, o: seen.append("act"))
    h2 = fused.layer3[1].relu.register_forward_pre_hook(lambda m, i: seen.append("relu"))
    got = _step(fused, x, y)
    # unfused: layer2.0 mid-block (hooked NoisyAct); layer3.1 mid-block and block end (hooked ReLU, used twice)
    assert len(fused_calls) == 16 - 3
    unfused = {fused.layer2[0].conv2.activations_quantizer, fused.layer3[1].conv2.activations_quantizer,
               fused.layer4[0].conv1.activations_quantizer}
    assert not unfused & {c[0] for c in fused_calls}
    assert seen == ["act", "relu", "relu"]
    _assert_same_step(got, ref)
    h1.remove(); h2.remove()
    # the Recorder hooks every NoisyAct: nothing is fused, and what it recorded checks out against the closed forms
    fused_calls.clear()
    rec = Recorder(fused)
    got = _step(fused, x, y)
    rec.close()
    assert not fused_calls
    assert rec.check(rel=1e-6) == 32                 # 16 activation + 16 weight quantizers
    _assert_same_step(got, ref)
    fused_calls.clear()
    _step(fused, x, y)
    assert len(fused_calls) == 16                    # hooks gone: fused again


def test_eval_mode_and_calibration_are_unfused(fused_calls):
    from mhaq_amd import fused_blocks
    from mhaq_amd.gdnsq import check_model_integrity
    from mhaq_amd.qat import calibrate_activations
    plain = _model()
    fused = copy.deepcopy(plain)
    fused_blocks.install(fused)
    x, _ = _xy()
    plain.eval(); fused.eval()
    with torch.no_grad():
        assert torch.equal(fused(x), plain(x))
    assert not fused_calls
    check_model_integrity(fused)                     # the eval path computed its flag words ...
    bws = [float(m.bw) for m in fused.modules() if hasattr(m, "log_act_s")]
    assert len(bws) == 16 and all(b > 0 for b in bws)            # ... and bw
    fused.train(); plain.train()
    calibrate_activations(fused, [x], 8)
    calibrate_activations(plain, [x], 8)
    assert not fused_calls and fused.training
    for (n, a), (_, b) in zip(plain.named_parameters(), fused.named_parameters()):
        assert torch.equal(a, b), n
    fused_blocks.uninstall(fused)
    assert type(fused) is type(plain) and type(fused.layer1[0]) is type(plain.layer1[0])
