"""GPU (-m gpu): mhaq_amd/fused_blocks.py under bf16 autocast (QATConfig.autocast_dtype) -- the fused places run the 16-bit
ReLU / residual-add kernels (mhaq_fq_act_relu_*_x16), whose contract is the bits of the separate 16-bit modules.  A trainer
with fuse_blocks=True must therefore leave EXACTLY the losses and parameters of one with fuse_blocks=False from the same
seeds (MIOpen held to its deterministic kernels), in eager steps and in hipGraph replays, and a hook sends its place back
to the stock modules.

Precondition: two unfused runs equal each other.  Where MIOpen's bf16 kernels are not reproducible against themselves the
comparison says nothing and the test skips with that reason; it is never loosened."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
STEPS = 4
N_FUSED = 16            # per forward: 8 mid-block, 7 block ends, the stem


@pytest.fixture(autouse=True)
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True       # MIOpen's default NHWC / wrw kernels use atomics
    yield
    torch.backends.cudnn.deterministic = det


@pytest.fixture
def fused_calls(monkeypatch):
    """The quantizers that took forward_fused, with the dtype they were handed."""
    from mhaq_amd.layers import NoisyAct
    calls = []
    inner = NoisyAct.forward_fused

    def counting(self, z, addend=None, want_act=False):
        calls.append((self, z.dtype, addend is not None, want_act))
        return inner(self, z, addend, want_act)
    monkeypatch.setattr(NoisyAct, "forward_fused", counting)
    return calls


def _trainer(fuse, act_method, w_method, distillation, autocast=BF16, capture=False):
    import mhaq_amd as M
    from mhaq_amd import fused_blocks, nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(4, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod[w_method], distillation=distillation, warmup=2,
                    learning_rate=1e-3, fuse_blocks=fuse, autocast_dtype=autocast)
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)
    assert (type(tr.net) is fused_blocks.FusedResNet18) == fuse
    for m in tr.net.modules():
        if hasattr(m, "log_act_s"):
            m.Q.qnmethod = M.QNMethod[act_method]
    return tr


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(4, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last),
             torch.randint(0, 10, (4,), generator=gen).to(DEV)) for _ in range(n)]


def _run(tr, batches):
    losses = [float(tr.train_step(x, y)) for x, y in batches]
    return losses, [p.detach().clone() for p in tr.net.parameters()]


def _equal(a, b):
    return a[0] == b[0] and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))


@pytest.mark.parametrize("act_method,w_method,distillation", [("STE", "AEWGS", True), ("LSQ", "LSQ", False)])
def test_fused_bf16_trainer_equals_unfused_bf16_trainer(act_method, w_method, distillation, fused_calls):
    batches = _batches(STEPS)
    plain = _run(_trainer(False, act_method, w_method, distillation), batches)
    again = _run(_trainer(False, act_method, w_method, distillation), batches)
    assert not fused_calls
    assert all(v == v for v in plain[0]), plain[0]
    if not _equal(plain, again):
        pytest.skip("MIOpen's bf16 kernels are not reproducible against themselves here: two unfused runs differ")
    fused = _run(_trainer(True, act_method, w_method, distillation), batches)
    # the fused path really ran, on bf16 tensors, at every place the fp32 trainer fuses
    n_bf16 = len(fused_calls)
    assert n_bf16 > 0 and all(dt is BF16 for _, dt, _, _ in fused_calls)
    assert sum(1 for _, _, add, _ in fused_calls if add) == STEPS * 7
    assert sum(1 for _, _, add, want in fused_calls if want and not add) == STEPS * 1
    fused_calls.clear()
    _run(_trainer(True, act_method, w_method, distillation, autocast=None), batches)
    assert all(dt is torch.float32 for _, dt, _, _ in fused_calls)
    assert n_bf16 == len(fused_calls) == STEPS * N_FUSED
    assert fused[0] == plain[0], (fused[0], plain[0])
    fresh = _trainer(False, act_method, w_method, distillation).net
    for (n, _), a, b in zip(fresh.named_parameters(), plain[1], fused[1]):
        assert torch.equal(a, b), n
    assert any(not torch.equal(a, b) for a, b in zip(fresh.parameters(), fused[1]))       # (the four steps did train)


def test_replayed_fused_bf16_steps_equal_eager_fused_bf16_steps(fused_calls):
    from mhaq_amd import ops
    batches = _batches(6)
    eager = _run(_trainer(True, "STE", "AEWGS", True), batches)
    n_eager = len(fused_calls)
    tr = _trainer(True, "STE", "AEWGS", True, capture=True)
    graphed = _run(tr, batches)
    assert tr._graph is not None and tr._eager_steps == 3
    assert n_eager == 6 * N_FUSED and len(fused_calls) - n_eager == 4 * N_FUSED     # 3 settling steps + the capture
    assert all(dt is BF16 for _, dt, _, _ in fused_calls)
    assert eager[0] == graphed[0]
    for a, b in zip(eager[1], graphed[1]):
        assert torch.equal(a, b)
    assert ops.rng.offset_base is None


def test_a_hook_takes_its_place_back_to_the_stock_modules(fused_calls):
    """Module level, one forward and backward under autocast: with a hook on one NoisyAct that place runs relu -> the
    module's own forward (bf16 in, bf16 out), the other fifteen stay fused, and logits, loss and every gradient are
    those of the unfused model."""
    import copy

    import mhaq_amd as M
    from mhaq_amd import fused_blocks, nets, ops, wrap
    torch.manual_seed(21)
    net = nets.resnet18(10).to(DEV).to(memory_format=torch.channels_last)
    wrap.quantize_model(net, M.QScheme.PER_CHANNEL, M.QNMethod.LSQ, ("conv1", "fc"), False, 4)
    net.to(DEV)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, "log_act_s"):
                m.log_act_s.fill_(-5.3); m.log_act_q.fill_(3.4); m.act_b.fill_(-3.1 if m.signed else 0.0)
                m.Q.qnmethod = M.QNMethod.STE
            if hasattr(m, "log_wght_s"):
                m.log_wght_s.fill_(-9.2)
    plain = net.train()
    fused = copy.deepcopy(plain)
    assert fused_blocks.install(fused) == 9
    g = torch.Generator().manual_seed(4)
    x = torch.randn(4, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (4,), generator=g).to(DEV)

    def step(model):
        ops.manual_seed(31)
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF16, cache_enabled=False):
            out = model(x)
            loss = torch.nn.functional.cross_entropy(out.float(), y)
        loss.backward()
        return out.detach(), loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()
                                             if p.grad is not None}

    ref, ref2 = step(plain), step(plain)
    if not (torch.equal(ref[0], ref2[0]) and all(torch.equal(ref[2][n], ref2[2][n]) for n in ref[2])):
        pytest.skip("MIOpen's bf16 kernels are not reproducible against themselves here: two unfused steps differ")
    assert not fused_calls
    hooked = fused.layer2[0].conv2.activations_quantizer
    seen = []
    h = hooked.register_forward_hook(lambda m, i, o: seen.append((i[0].dtype, o.dtype)))
    got = step(fused)
    h.remove()
    assert seen == [(BF16, BF16)]
    assert len(fused_calls) == N_FUSED - 1 and hooked not in {c[0] for c in fused_calls}
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and got[2].keys() == ref[2].keys()
    for n in ref[2]:
        assert torch.equal(got[2][n], ref[2][n]), n
    fused_calls.clear()
    got = step(fused)                                # the hook gone: fused again, and still the same step
    assert len(fused_calls) == N_FUSED
    for n in ref[2]:
        assert torch.equal(got[2][n], ref[2][n]), n
