"""GPU (-m gpu): QATTrainer with QATConfig.autocast_dtype = torch.bfloat16 -- mixed-precision QAT, the reference trainer's
`precision = "bf16-mixed"`.  The activation quantizers behind the autocast convolutions take the 16-bit kernels
(mhaq_fq_act_*_x16); weights and quantizer parameters stay float32."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16 = torch.bfloat16


@pytest.fixture
def deterministic_miopen():
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True          # MIOpen's default NHWC / wrw kernels use atomics
    yield
    torch.backends.cudnn.deterministic = prev


def _parity_run(layers, steps, distillation):
    """tests/test_gpu_training_parity.py's run, under bf16 autocast."""
    import mhaq_amd as M
    from mhaq_amd import nets
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(11)
    net = nets.resnet20_cifar(10).to(DEV).train()
    gw = torch.Generator(device=DEV).manual_seed(4)
    warm = torch.randn(32, 3, 32, 32, device=DEV, generator=gw)
    with torch.no_grad():
        for _ in range(40):
            net(warm)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=4, weight_bit=4,
                    excluded_layers=("features.init_block.conv", "output"), distillation=distillation,
                    learning_rate=2e-3, warmup=3, autocast_dtype=BF16)
    g = torch.Generator(device=DEV).manual_seed(5)
    calib = torch.randn(32, 3, 32, 32, device=DEV, generator=g)
    mm = (lambda t: torch.stack(list(t.aminmax()))) if layers is not None else None
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], layers=layers, minmax_fn=mm, distributed=False,
                    capture_graph=False)
    for m in tr.net.modules():
        if hasattr(m, "log_act_s"):
            if hasattr(m, "Q"):
                m.Q.qnmethod = M.QNMethod.LSQ
            else:
                m.qnmethod = "LSQ"
    losses = []
    for _ in range(steps):
        x = torch.randn(32, 3, 32, 32, device=DEV, generator=g)
        y = torch.randint(0, 10, (32,), device=DEV, generator=g)
        losses.append(float(tr.train_step(x, y)))
    params = torch.cat([p.detach().flatten() for p in tr.net.parameters()])
    return losses, params


@pytest.mark.parametrize("distillation", [False, True])
def test_bf16_training_tracks_the_oracle_layers_under_the_same_autocast(deterministic_miopen, distillation):
    """The oracle's NoisyAct returns the fp32 y of the reference's chain, which the next autocast convolution casts to
    bf16; ours returns those bf16 bits directly -- the convolutions see the same tensors, so the first two losses (lr 0
    on the first step) agree, and the trajectory stays within the fp32 parity test's bounds."""
    from oracle.ref_layers import ORACLE_LAYERS
    steps = 12
    l_hip, p_hip = _parity_run(None, steps, distillation)
    l_ref, p_ref = _parity_run(ORACLE_LAYERS, steps, distillation)
    assert all(torch.isfinite(torch.tensor(l_hip)))
    for k in (0, 1):
        assert abs(l_hip[k] - l_ref[k]) <= 1e-6 * abs(l_ref[k]), (k, l_hip[k], l_ref[k])
    for i, (a, b) in enumerate(zip(l_hip, l_ref)):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (i, a, b)
    rel = float((p_hip - p_ref).norm() / p_ref.norm())
    assert rel < 1e-3, rel


def _make(capture, distillation, act_method):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(5)
    ops.manual_seed(5)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=4, weight_bit=4,
                    excluded_layers=("features.init_block.conv", "output"), warmup=3, distillation=distillation,
                    learning_rate=1e-3, autocast_dtype=BF16)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
    factory = lambda params, lr: torch.optim.RAdam(   # noqa: E731
        params, torch.tensor(float(lr), device=DEV), capturable=True)
    tr = QATTrainer(nets.resnet20_cifar(10), cfg, DEV, calib_batches=[calib], distributed=False,
                    optimizer_factory=factory, capture_graph=capture)
    for m in tr.net.modules():
        if hasattr(m, "log_act_s"):
            m.Q.qnmethod = M.QNMethod[act_method]
    return tr


@pytest.mark.parametrize("distillation,act_method", [(False, "LSQ"), (True, "STE")])
def test_captured_bf16_steps_equal_eager_steps_bit_for_bit(deterministic_miopen, distillation, act_method):
    gen = torch.Generator().manual_seed(9)
    batches = [(torch.randn(8, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (8,), generator=gen).to(DEV))
               for _ in range(8)]
    eager = _make(False, distillation, act_method)
    le = [float(eager.train_step(x, y)) for x, y in batches]
    graphed = _make(True, distillation, act_method)
    lg = [float(graphed.train_step(x, y)) for x, y in batches]
    assert graphed._graph is not None and graphed._eager_steps == 3
    assert le == lg
    for (n, a), (_, b) in zip(eager.net.named_parameters(), graphed.net.named_parameters()):
        assert torch.equal(a, b), n
    assert all(torch.isfinite(torch.tensor(le)))


def test_every_noisy_act_takes_the_16bit_kernels():
    """A forward hook on every NoisyAct: bf16 in, bf16 out -- the fused 16-bit path ran, not the fp32 route on x.float()
    (which returns float32).  The base loss reaching PotentialLoss is float32 (ops.potential_loss checks it)."""
    import mhaq_amd as M
    tr = _make(False, True, "STE")
    seen = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: seen.append((inp[0].dtype, out.dtype)))
             for m in tr.net.modules() if isinstance(m, M.NoisyAct)]
    gen = torch.Generator().manual_seed(1)
    x, y = torch.randn(8, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (8,), generator=gen).to(DEV)
    try:
        loss = tr.train_step(x, y)
    finally:
        for h in hooks:
            h.remove()
    n_act = sum(isinstance(m, M.NoisyAct) for m in tr.net.modules())
    assert n_act > 10 and len(seen) == n_act
    assert all(s == (BF16, BF16) for s in seen), seen
    assert torch.isfinite(loss) and loss.dtype == torch.float32
    assert tr.loss.base_loss.dtype == torch.float32
    for p in tr.net.parameters():
        assert p.dtype == torch.float32 and (p.grad is None or p.grad.dtype == torch.float32)


def test_validate_step_under_autocast():
    import mhaq_amd as M
    tr = _make(False, False, "LSQ")
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(16, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (16,), generator=gen).to(DEV)
    for _ in range(2):
        tr.train_step(x, y)
    out = tr.validate_step(x, y)
    assert tr.module.training
    assert out["val_loss"].dtype == torch.float32 and torch.isfinite(out["val_loss"])
    for k in ("mean_weights_bit_width", "mean_activations_bit_width"):
        assert torch.isfinite(out[k]), k
    for k in ("actual_activations_bit_width", "actual_activations_max_bit_width"):
        assert torch.isfinite(torch.as_tensor(out[k])), k
    acts = [m for m in tr.net.modules() if isinstance(m, M.NoisyAct)]
    assert all(torch.isfinite(m.bw) for m in acts)
    bad = x.clone()
    bad[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="Not all elements in the tensor"):
        tr.validate_step(bad, y)
    assert tr.module.training
