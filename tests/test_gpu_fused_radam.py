"""GPU (-m gpu): the one-pass RAdam (mhaq_fq_radam_step behind mhaq_amd/optim.py: FusedRAdam).  The yardstick is
torch.optim.RAdam(foreach=True) on the same device and inputs, never the code under test: EQUAL BITS in every p, exp_avg,
exp_avg_sq and step after each of steps 1-9 -- across the rho_t > 5 switch at step 6, with planted gradients (zeros, -0.0, a
subnormal, +-inf and NaN, magnitudes 1e-12 .. 1e6), a moving learning rate (0 included), parameters whose step count lags, and
every size and layout at which the kernel takes another path (C = one chunk, 4096 elements):
    1, 3, 4, 5, 64, 1023        below one float4, one float4, float4 + tail, part of a block
    C + 1, 3 C + 5              more than one block, a tail in the last chunk
    [8,4,3,3] channels_last, [8,4,1,1] under both stride spellings, a view at a 4-byte-aligned, 16-byte-misaligned offset
    70 tensors in one group
The trainer tests have the shape of tests/test_gpu_fused_blocks.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 4096
LRS = [3e-3, 1e-3, 0.0, 3e-3, 2e-3, 3e-3, 0.0, 4e-3, 1e-4]      # a schedule moves the rate between steps
SPECIALS = [0.0, -0.0, 1e-41, float("inf"), float("-inf"), float("nan"), 1e-12, 1e6]


def _make(kind, shape, gen):
    """One parameter's initial value on the device in the layout `kind` (a fresh tensor per call, same values per gen state)."""
    n = 1
    for s in shape:
        n *= s
    vals = torch.randn(n, generator=gen)
    if kind == "plain":
        return vals.reshape(shape).to(DEV)
    if kind == "channels_last":
        return vals.reshape(shape).to(DEV).contiguous(memory_format=torch.channels_last)
    if kind == "cl_strides_1x1":          # [Co, Ci, 1, 1] spelled with channels_last strides
        return vals.to(DEV).as_strided(shape, (shape[1], 1, shape[1], shape[1]))
    if kind == "offset_view":             # 4-byte aligned, 16-byte misaligned
        base = torch.zeros(n + 1, device=DEV)
        base[1:] = vals.to(DEV)
        v = base[1:].view(shape)
        assert v.data_ptr() % 16 == 4
        return v
    raise AssertionError(kind)


SPECS = [("plain", (1,)), ("plain", (3,)), ("plain", (4,)), ("plain", (5,)), ("plain", (64,)), ("plain", (1023,)),
         ("plain", (CHUNK + 1,)), ("plain", (3 * CHUNK + 5,)), ("channels_last", (8, 4, 3, 3)), ("plain", (8, 4, 1, 1)),
         ("cl_strides_1x1", (8, 4, 1, 1)), ("offset_view", (1023,)), ("offset_view", (CHUNK + 7,))]
SPECS += [("plain", (1 + (7 * i) % 61,)) for i in range(70 - len(SPECS))]      # 70 tensors in one group
PLANTED, LAGGING, OTHER_SPELLING = 5, 6, 9      # indices into SPECS


def _grad(i, p, step, gen):
    """The gradient of tensor i at `step` (1-based), in p's memory order unless the case says otherwise; None: no gradient."""
    if i == LAGGING and step in (2, 5):
        return None
    g = torch.randn(p.shape, generator=gen) * (10.0 ** float(torch.randint(-12, 7, (1,), generator=gen)))
    if i == PLANTED:
        g.view(-1)[:len(SPECIALS)] = torch.tensor(SPECIALS)
    if i == 4 and step == 3:
        g.zero_()
    if i == 4 and step == 4:
        g.zero_().neg_()                                                 # all -0.0
    out = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g.to(DEV))
    if i == OTHER_SPELLING:                                              # the same memory under the other stride spelling
        out = out.as_strided(p.shape, (p.shape[1], 1, p.shape[1], p.shape[1]))
    return out


def _run(opt_class, specs, steps=9, grad_fn=_grad, **kw):
    """-> per step: (p, exp_avg, exp_avg_sq, step) of every parameter, as int32 bit patterns / floats on the host."""
    gen = torch.Generator().manual_seed(11)
    ps = [_make(kind, shape, gen).requires_grad_(True) for kind, shape in specs]
    opt = opt_class(ps, lr=1e-3, **kw)
    ggen = torch.Generator().manual_seed(12)
    bits = lambda t: t.detach().contiguous().view(torch.int32).cpu()      # noqa: E731
    out = []
    for step in range(1, steps + 1):
        for grp in opt.param_groups:
            grp["lr"] = LRS[step - 1]
        for i, p in enumerate(ps):
            p.grad = grad_fn(i, p, step, ggen)
        opt.step()
        rec = []
        for p in ps:
            st = opt.state.get(p, {})
            rec.append((bits(p), bits(st["exp_avg"]) if st else None, bits(st["exp_avg_sq"]) if st else None,
                        float(st["step"]) if st else None))
        out.append(rec)
    return out, opt


@pytest.fixture(scope="module")
def torch_run():
    """The yardstick, computed once: torch's foreach RAdam on the 70 tensors."""
    return _run(torch.optim.RAdam, SPECS, foreach=True)[0]


def _assert_equal_bits(got, want, specs):
    for step, (g_rec, w_rec) in enumerate(zip(got, want), 1):
        for i, (g, w) in enumerate(zip(g_rec, w_rec)):
            for name, a, b in zip(("p", "exp_avg", "exp_avg_sq"), g, w):
                assert (a is None) == (b is None), (step, i, name)
                if a is not None:
                    bad = (a != b).nonzero()
                    assert bad.numel() == 0, f"step {step}, tensor {i} {specs[i]}, {name}: {bad.numel()} of {a.numel()} " \
                                             f"elements differ, first at {bad[0].tolist()}"
            assert g[3] == w[3], (step, i, "step")


def test_seventy_tensors_equal_torch_foreach_radam_bit_for_bit_over_nine_steps(torch_run):
    from mhaq_amd import optim
    steps0, fb0 = optim.fused_radam_steps(), optim.fused_radam_fallbacks()
    got, opt = _run(optim.FusedRAdam, SPECS)
    assert optim.fused_radam_steps() - steps0 == 9 and optim.fused_radam_fallbacks() == fb0      # one launch per step
    _assert_equal_bits(got, torch_run, SPECS)
    assert got[-1][LAGGING][3] == 7.0 and got[-1][0][3] == 9.0            # the lagging parameter is at its own step count
    assert not opt.state[opt.param_groups[0]["params"][0]]["step"].is_cuda
    # the planted values did what IEEE says: NaN and the infinities poison their own elements only
    p_bits = got[-1][PLANTED][0].view(torch.float32)
    assert torch.isnan(p_bits[3:6]).all() and torch.isfinite(p_bits[:3]).all() and torch.isfinite(p_bits[6:]).all()


def test_mixed_groups_take_the_fallback_per_parameter_and_stay_bit_equal():
    from mhaq_amd import optim
    specs = [("plain", (CHUNK + 1,)), ("channels_last", (8, 4, 3, 3)), ("plain", (5,)), ("channels_last", (4, 4, 3, 3))]

    def grad_fn(i, p, step, gen):
        g = torch.randn(p.shape, generator=gen).to(DEV)
        if i == 1:
            return g.contiguous()                                        # a channels_last parameter, a contiguous gradient
        return torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)

    def both(cls, **kw):
        gen = torch.Generator().manual_seed(11)
        ps = [_make(k, s, gen).requires_grad_(True) for k, s in specs]
        opt = cls([{"params": ps[:3]}, {"params": ps[3:], "weight_decay": 1e-2}], lr=1e-3, **kw)
        ggen = torch.Generator().manual_seed(12)
        out = []
        for step in range(1, 10):
            for grp in opt.param_groups:
                grp["lr"] = LRS[step - 1]
            for i, p in enumerate(ps):
                p.grad = grad_fn(i, p, step, ggen)
            opt.step()
            out.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(),
                         float(opt.state[p]["step"])) for p in ps])
        return out

    steps0, fb0 = optim.fused_radam_steps(), optim.fused_radam_fallbacks()
    got = both(optim.FusedRAdam)
    # per step: tensors 0 and 2 fused in one launch; tensor 1 (stride mismatch) and tensor 3 (its group decays) fall back
    assert optim.fused_radam_steps() - steps0 == 9 and optim.fused_radam_fallbacks() - fb0 == 9 * 2
    want = both(torch.optim.RAdam, foreach=True)
    for step, (gr, wr) in enumerate(zip(got, want), 1):
        for i, (g, w) in enumerate(zip(gr, wr)):
            for a, b in zip(g[:3], w[:3]):
                assert a.stride() == b.stride()
                assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), (step, i)
            assert g[3] == w[3]


# ---------------------------------------------------------------------------------------------- the trainer
@pytest.fixture
def _deterministic_miopen():
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True       # MIOpen's default NHWC / wrw kernels use atomics
    yield
    torch.backends.cudnn.deterministic = det


def _trainer(fused, capture=False):
    import mhaq_amd as M
    from mhaq_amd import nets, ops, optim
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    net = nets.resnet18(10).to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(8, 3, 64, 64, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.AEWGS, distillation=True, warmup=2,
                    learning_rate=1e-3, fused_optimizer=fused)
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=capture)
    assert (type(tr.optimizer) is optim.FusedRAdam) == fused
    assert type(tr.optimizer) is (optim.FusedRAdam if fused else torch.optim.RAdam)
    return tr


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(8, 3, 64, 64, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last),
             torch.randint(0, 10, (8,), generator=gen).to(DEV)) for _ in range(n)]


@pytest.fixture(scope="module")
def eager_fused_run():
    """Four eager steps of the trainer with the fused optimizer, shared by the two trainer tests."""
    from mhaq_amd import optim
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        steps0, fb0 = optim.fused_radam_steps(), optim.fused_radam_fallbacks()
        tr = _trainer(True)
        losses = [float(tr.train_step(x, y)) for x, y in _batches(4)]
        counts = (optim.fused_radam_steps() - steps0, optim.fused_radam_fallbacks() - fb0)
        return losses, [p.detach().clone() for p in tr.net.parameters()], counts
    finally:
        torch.backends.cudnn.deterministic = det


def test_trainer_with_the_fused_optimizer_equals_the_trainer_with_torchs(eager_fused_run, _deterministic_miopen, monkeypatch):
    from mhaq_amd import optim
    monkeypatch.delenv(optim.ENV_SWITCH, raising=False)
    lf, pf, (launches, fallbacks) = eager_fused_run
    assert launches == 4 and fallbacks == 0              # one launch per step, nothing handed back to torch
    plain = _trainer(False)
    lp = [float(plain.train_step(x, y)) for x, y in _batches(4)]
    assert all(v == v for v in lp), lp
    assert lf == lp
    for (n, a), b in zip(plain.net.named_parameters(), pf):
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32)), n
    fresh = _trainer(False)
    assert any(not torch.equal(a, b) for a, b in zip(fresh.net.parameters(), pf))      # (the four steps did train)
    # the environment decides when set; a factory is never replaced
    monkeypatch.setenv(optim.ENV_SWITCH, "0")
    assert type(_env_trainer()) is torch.optim.RAdam


def _env_trainer():
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.AEWGS, warmup=2, fused_optimizer=True)
    tr = QATTrainer(nets.resnet18(10).to(memory_format=torch.channels_last), cfg, DEV, distributed=False, capture_graph=False)
    return tr.optimizer


def test_replayed_steps_with_the_fused_optimizer_equal_eager_steps(eager_fused_run, _deterministic_miopen):
    from mhaq_amd import optim
    le, pe, _ = eager_fused_run
    steps0, fb0 = optim.fused_radam_steps(), optim.fused_radam_fallbacks()
    graphed = _trainer(True, capture=True)
    lg = [float(graphed.train_step(x, y)) for x, y in _batches(4)]
    assert graphed._graph is not None and graphed._eager_steps == 3      # 3 settling steps, then the capture and a replay
    assert optim.fused_radam_steps() - steps0 == 4 and optim.fused_radam_fallbacks() == fb0
    assert lg == le
    for (n, a), b in zip(graphed.net.named_parameters(), pe):
        assert torch.equal(a.detach().view(torch.int32), b.view(torch.int32)), n
