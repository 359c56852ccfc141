"""GPU (-m gpu): the classification head inside QATTrainer -- the validation record with QATConfig.cls_metrics, the unchanged
record without it, and the non-distillation training step with QATConfig.fused_cross_entropy (eager against the framework's
criterion, captured against eager).  The ResNet-20 trainer of tests/test_gpu_validate_step.py."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import cls_head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OLD_KEYS = ["val_loss", "top1", "mean_weights_bit_width", "actual_weights_bit_width", "actual_weights_max_bit_width",
            "mean_activations_bit_width", "actual_activations_bit_width", "actual_activations_max_bit_width", "converged"]
NEW_KEYS = ["Accuracy_top1", "Accuracy_top5", "ns_Accuracy_top1", "ns_Accuracy_top5", "correct", "metric_flags"]


@pytest.fixture(autouse=True)
def _switches_unset(monkeypatch):
    from mhaq_amd import loss as L
    monkeypatch.delenv(L.ENV_SWITCH_CE, raising=False)
    monkeypatch.delenv(L.ENV_SWITCH_CLS_METRICS, raising=False)


def _trainer(**cfg_kw):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(3)
    ops.manual_seed(3)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=4, weight_bit=4,
                    excluded_layers=("features.init_block.conv", "output"), warmup=2, distillation=False, **cfg_kw)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(16, 3, 32, 32, generator=g).to(DEV)
    y = torch.randint(0, 10, (16,), generator=g).to(DEV)
    tr = QATTrainer(nets.resnet20_cifar(10), cfg, DEV, calib_batches=[x], distributed=False)
    return tr, x, y


def _validate(tr, x, y):
    """-> (record, the logits the eval forward returned, host synchronisations of the step)."""
    seen = []
    hook = tr.net.register_forward_hook(lambda m, inp, out: seen.append(out.detach().clone()))
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            rec = tr.validate_step(x, y)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
            hook.remove()
    (logits,) = seen
    return rec, logits, sum("called a synchronizing" in str(w.message) for w in caught)


def _check_record(rec, logits, y):
    from mhaq_amd.cls_metrics import check_cls_flags
    assert list(rec) == OLD_KEYS + NEW_KEYS
    ref = R.head64(logits.float(), y.cpu(), topk=5)                  # counts from the stable sort of the logits on the CPU
    assert rec["correct"].dtype == torch.int64 and rec["correct"].cpu().tolist() == ref["counts"].tolist()
    assert int(ref["counts"][0]) == 16
    l_t = F.cross_entropy(logits.float(), y)
    assert abs(float(rec["val_loss"]) - float(ref["loss"])) <= R.loss_bar(l_t, ref["loss"])
    assert float(rec["top1"]) == float(rec["Accuracy_top1"]) == int(ref["counts"][1]) / 16
    assert float(rec["Accuracy_top5"]) == int(ref["counts"][2]) / 16
    assert float(rec["top1"]) == float((logits.argmax(1) == y).float().mean())
    assert isinstance(rec["converged"], bool)
    for k in ("Accuracy_top1", "Accuracy_top5"):
        assert float(rec["ns_" + k]) == float(rec[k]) * float(rec["converged"])
    assert check_cls_flags(rec["metric_flags"], nonfinite=True) == 0


def test_validation_record_with_cls_metrics_and_the_unchanged_record_without():
    from mhaq_amd.cls_metrics import ClsValidationMeter
    from mhaq_amd.loss import cls_head_launches
    n0 = cls_head_launches()
    off, x, y = _trainer()
    off2, _, _ = _trainer()
    rec_off, logits_off, syncs_off = _validate(off, x, y)
    rec_off2, _, _ = _validate(off2, x, y)
    # switched off: the keys of the record as it was, the framework's ops on the returned logits bit for bit, and the same
    # bits from a second trainer of the same seed
    assert list(rec_off) == OLD_KEYS and off.module.training
    assert torch.equal(rec_off["val_loss"], F.cross_entropy(logits_off.float(), y))
    assert torch.equal(rec_off["top1"], (logits_off.float().argmax(1) == y).float().mean())
    for k in OLD_KEYS:
        a, b = rec_off[k], rec_off2[k]
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b, k
    # switched on: the same step with the head's keys appended, and no further host synchronisation
    on = off2
    on.cfg.cls_metrics = True
    rec_on, logits_on, syncs_on = _validate(on, x, y)
    assert on.module.training and torch.equal(logits_on, logits_off) and syncs_on == syncs_off
    _check_record(rec_on, logits_on, y)
    for k in OLD_KEYS[2:]:
        a, b = rec_on[k], rec_off[k]
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b, k
    assert cls_head_launches() == n0                       # the compiled node never ran: validation takes the ctypes path
    # an epoch of two such batches through the meter
    meter = ClsValidationMeter()
    meter.update(rec_on)
    meter.update(rec_on)
    out = meter.compute()
    assert float(out["Accuracy_top1"]) == int(rec_on["correct"][1]) / 16
    assert float(out["Accuracy_top5"]) == int(rec_on["correct"][2]) / 16
    assert float(out["val_loss"]) == float(rec_on["val_loss"])


def test_environment_switch_and_the_record_under_bf16_autocast(monkeypatch):
    from mhaq_amd import loss as L
    monkeypatch.setenv(L.ENV_SWITCH_CLS_METRICS, "1")
    tr, x, y = _trainer(autocast_dtype=torch.bfloat16)
    rec, logits, _ = _validate(tr, x, y)
    assert tr.module.training
    _check_record(rec, logits, y)
    monkeypatch.setenv(L.ENV_SWITCH_CLS_METRICS, "0")
    tr.cfg.cls_metrics = True
    assert list(tr.validate_step(x, y)) == OLD_KEYS


# ---------------------------------------------------------------------------------------------- training
@pytest.fixture()
def _deterministic():
    from mhaq_amd import ops
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True      # MIOpen's default wrw kernels use atomics: not run-to-run exact
    yield
    torch.backends.cudnn.deterministic = det
    assert ops.rng.offset_base is None


def _make(capture, **cfg_kw):
    import mhaq_amd as M
    from mhaq_amd import nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(5)
    ops.manual_seed(5)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=4, weight_bit=4,
                    excluded_layers=("features.init_block.conv", "output"), warmup=3, distillation=False,
                    learning_rate=1e-3, **cfg_kw)
    g = torch.Generator().manual_seed(2)
    calib = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
    factory = lambda params, lr: torch.optim.RAdam(   # noqa: E731  -- the same capturable optimizer on both sides
        params, torch.tensor(float(lr), device=DEV), capturable=True)
    return QATTrainer(nets.resnet20_cifar(10), cfg, DEV, calib_batches=[calib], distributed=False,
                      optimizer_factory=factory, capture_graph=capture)


def _batches(n):
    gen = torch.Generator().manual_seed(9)
    return [(torch.randn(8, 3, 32, 32, generator=gen).to(DEV), torch.randint(0, 10, (8,), generator=gen).to(DEV))
            for _ in range(n)]


def _trajectory(steps, **cfg_kw):
    """The run of tests/test_gpu_training_parity.py, where the 2e-3 / 1e-3 trajectory bars come from: a ResNet-20 whose
    BatchNorm statistics have settled, batches of 32, 3 warm-up steps, LSQ everywhere -> (losses, parameters, trainer)."""
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
                    excluded_layers=("features.init_block.conv", "output"), distillation=False, learning_rate=2e-3,
                    warmup=3, **cfg_kw)
    g = torch.Generator(device=DEV).manual_seed(5)
    calib = torch.randn(32, 3, 32, 32, device=DEV, generator=g)
    tr = QATTrainer(net, cfg, DEV, calib_batches=[calib], distributed=False, capture_graph=False)
    for m in tr.net.modules():                      # activations: LSQ instead of the default random STE
        if hasattr(m, "log_act_s"):
            m.Q.qnmethod = M.QNMethod.LSQ
    losses = []
    for _ in range(steps):
        x = torch.randn(32, 3, 32, 32, device=DEV, generator=g)
        y = torch.randint(0, 10, (32,), device=DEV, generator=g)
        losses.append(float(tr.train_step(x, y)))
    return losses, torch.cat([p.detach().flatten() for p in tr.net.parameters()]), tr


def test_fused_cross_entropy_trainer_follows_the_default_trainers_loss_curve(_deterministic):
    """12 steps with the switch on against the same trainer with it off, within the bars of the HIP-versus-oracle trajectories
    (tests/test_gpu_training_parity.py: 2e-3 * max(1, |loss|) per step, 1e-3 of the parameters' norm), on that test's run."""
    from mhaq_amd import loss as L
    n0 = L.cls_head_launches()
    l_off, p_off, off = _trajectory(12)
    assert off._train_criterion is off.cfg.criterion and type(off.cfg.criterion) is torch.nn.CrossEntropyLoss
    assert L.cls_head_launches() == n0                           # the defaults never reach the node
    l_on, p_on, on = _trajectory(12, fused_cross_entropy=True)
    assert type(on._train_criterion) is L.FusedCrossEntropy and type(on.cfg.criterion) is torch.nn.CrossEntropyLoss
    assert L.cls_head_launches() - n0 == 3 * 12                  # two launches forward, one backward
    assert all(torch.isfinite(torch.tensor(l_on)))
    rel = float((p_on - p_off).norm() / p_off.norm())
    for i, (a, b) in enumerate(zip(l_on, l_off)):
        print(f"step {i}: loss with the fused cross-entropy {a:.9g}  default {b:.9g}  difference {abs(a - b):.3e}")
    print("relative parameter distance after 12 steps", rel)
    for i, (a, b) in enumerate(zip(l_on, l_off)):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (i, a, b)
    assert rel < 1e-3, rel


def test_captured_fused_cross_entropy_steps_equal_the_eager_ones_bit_for_bit(_deterministic):
    """Three eager steps, then five replays, against eight eager steps (tests/test_gpu_graph_step.py's run)."""
    batches = _batches(8)
    eager = _make(False, fused_cross_entropy=True)
    le = [float(eager.train_step(x, y)) for x, y in batches]
    graphed = _make(True, fused_cross_entropy=True)
    lg = [float(graphed.train_step(x, y)) for x, y in batches]
    assert graphed._graph is not None and graphed._eager_steps == 3
    assert all(torch.isfinite(torch.tensor(lg))) and le == lg
    for (n, a), (_, b) in zip(eager.net.named_parameters(), graphed.net.named_parameters()):
        assert torch.equal(a, b), n


def test_the_switch_follows_the_environment_and_any_other_criterion_is_left_alone(monkeypatch):
    from mhaq_amd import loss as L
    monkeypatch.setenv(L.ENV_SWITCH_CE, "1")
    smooth = torch.nn.CrossEntropyLoss(label_smoothing=0.1)
    assert _make(False, criterion=smooth)._train_criterion is smooth
    monkeypatch.setenv(L.ENV_SWITCH_CE, "0")
    assert type(_make(False, fused_cross_entropy=True)._train_criterion) is torch.nn.CrossEntropyLoss
