"""GPU (-m gpu): the fused distillation losses (mhaq_fq_distill_loss_fwd / _bwd, csrc/distill.hip) through the C ABI and
through mhaq_amd.loss.FusedDistillLoss, against float64 autograd on the CPU through the reference modules' torch statements
(tests/distill_ref.py).  The bar is the framework's own float32 chain on the device, never the kernel:
    |L - L64| <= 4 |L_torch - L64| + 8 ulp32(L64),   max|gx - g64| <= 4 max|g_torch - g64| + 8 2^-24 max|g64|.
Shapes: 3x1, 1x2, 5x37, 16x1001 (odd: unaligned row bases) and 250x1000 in registers, 2x4096 / 4x4097 at the edge of the
register path, 2x10007 re-walked; 257x4 and 600x3 give the finalize more row partials than it has threads, 3x1028 and 2x4092
end in the first group of a thread's second trip over the row and in the last group of its fourth."""
import ctypes
import functools

import pytest
import torch

from tests import distill_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 64                                  # elements of ones planted before and after every output
G_UP = 0.375                               # a non-trivial upstream gradient
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SCALES = {(3, 1): 2.0, (1, 2): 1.0, (5, 37): 8.0, (16, 1001): 4.0, (250, 1000): 4.0, (2, 4096): 2.0, (4, 4097): 8.0,
          (2, 10007): 1.0, (257, 4): 4.0, (600, 3): 2.0, (3, 1028): 4.0, (2, 4092): 2.0}
ids_shape = lambda s: "%dx%d" % s          # noqa: E731
ids_kind = lambda k: R.NAMES[k]            # noqa: E731


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Banded:
    """n elements between two bands of ones, the view 16-byte aligned plus `shift` elements."""

    def __init__(self, n, dtype, shift=0):
        self.buf = torch.ones(BAND + shift + n + BAND, dtype=dtype, device=DEV)
        self.lo, self.n = BAND + shift, n
        self.view = self.buf[self.lo:self.lo + n]
        self.view.fill_(-7.0)

    def intact(self):
        return bool((self.buf[:self.lo] == 1).all()) and bool((self.buf[self.lo + self.n:] == 1).all())


def capi_fwd(x, t, kind, want_grad=True, shift=0):
    """-> (loss [1], gunit [rows, cols] or None); asserts that nothing around loss, gunit and the workspace was written."""
    from mhaq_amd import _lib
    lib = _lib.lib()
    rows, cols = x.shape
    assert x.is_contiguous() and t.is_contiguous()
    wsb = lib.mhaq_fq_distill_loss_workspace_bytes(rows)
    assert wsb == rows * 8
    ws, loss = Banded(rows, torch.float64), Banded(1, torch.float32)
    gunit = Banded(rows * cols, torch.float32, shift) if want_grad else None
    _lib.check(lib.mhaq_fq_distill_loss_fwd(_ptr(x), DT[x.dtype], _ptr(t), DT[t.dtype], rows, cols, kind, _ptr(loss.view),
                                            _ptr(gunit.view) if want_grad else None, _ptr(ws.view), wsb, _stream()),
               "mhaq_fq_distill_loss_fwd")
    torch.cuda.synchronize()
    assert ws.intact() and loss.intact() and (gunit is None or gunit.intact())
    return loss.view.clone(), (gunit.view.reshape(rows, cols) if want_grad else None)


def capi_bwd(gunit, g, dtype, shift=0):
    from mhaq_amd import _lib
    lib = _lib.lib()
    gx = Banded(gunit.numel(), dtype, shift)
    gdev = torch.tensor([g], dtype=torch.float32, device=DEV)
    _lib.check(lib.mhaq_fq_distill_loss_bwd(_ptr(gunit), _ptr(gdev), _ptr(gx.view), DT[dtype], gunit.numel(), _stream()),
               "mhaq_fq_distill_loss_bwd")
    torch.cuda.synchronize()
    assert gx.intact()
    return gx.view.reshape(gunit.shape).clone()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@functools.lru_cache(maxsize=None)
def _case(shape, seed=0):
    """Inputs on the device, shared and never modified: (x, t)."""
    return R.logits(shape, SCALES[shape], seed=1000 * shape[0] + shape[1] + seed, device=DEV)


@functools.lru_cache(maxsize=None)
def _refs(kind, shape):
    """-> (framework float32 chain on the device, float64 autograd on the CPU), computed once per case."""
    x, t = _case(shape)
    return R.chain32(kind, x, t, G_UP), R.autograd64(kind, x, t, G_UP)


# ---------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("shape", R.SHAPES, ids=ids_shape)
@pytest.mark.parametrize("kind", R.KINDS, ids=ids_kind)
def test_loss_and_gradient_through_the_c_abi_and_the_module_meet_the_bar(kind, shape):
    from mhaq_amd.loss import FusedDistillLoss, distill_fused_launches
    x, t = _case(shape)
    chain, ref = _refs(kind, shape)
    loss, gunit = capi_fwd(x, t, kind)
    gx = capi_bwd(gunit, G_UP, torch.float32)
    ok, fig = R.within_bar(loss, gx, chain, ref)
    print("capi", R.NAMES[kind], shape, fig)
    assert ok, fig
    # the same inputs give the same bits, with and without gunit, at another alignment of gunit
    loss2, gunit2 = capi_fwd(x, t, kind, shift=1)
    loss3, _ = capi_fwd(x, t, kind, want_grad=False)
    assert torch.equal(_bits(loss), _bits(loss2)) and torch.equal(_bits(loss), _bits(loss3))
    assert torch.equal(_bits(gunit), _bits(gunit2))
    assert torch.equal(_bits(gx), _bits(capi_bwd(gunit2.contiguous(), G_UP, torch.float32, shift=3)))
    # the module: the same entry points behind autograd
    n0 = distill_fused_launches()
    xm = x.clone().requires_grad_(True)
    lm = FusedDistillLoss(R.NAMES[kind])(xm, t)
    assert lm.dim() == 0 and lm.dtype == torch.float32
    (lm * G_UP).backward()
    assert distill_fused_launches() - n0 == 3
    assert torch.equal(_bits(lm.detach().reshape(1)), _bits(loss)) and torch.equal(_bits(xm.grad), _bits(gx))
    with torch.no_grad():
        assert torch.equal(_bits(FusedDistillLoss(kind)(xm, t).reshape(1)), _bits(loss))


def test_hellinger_gradient_is_finite_where_a_probability_underflows_and_the_frameworks_is_nan():
    """The bar's first term is the error of a float32 chain of the same quantity.  The framework's gradient is NaN here, so
    where it is, that chain is distill_ref's closed form run in float32 on the device (torch ops, no kernel).  Counting a NaN
    entry as an error of zero -- the second term alone, 8 2^-24 max|g64| = 1.35e-13 -- is a bar no float32 evaluation can meet:
    at logits of scale 20 r = h - ps H cancels operands of order 1 down to 0.015; the kernel's error measured 2.94e-13."""
    x, t = R.logits((2, 10007), 20.0, seed=3, device=DEV)
    assert bool((x.softmax(-1) == 0).any())
    l_t, g_t = R.chain32(R.HELLINGER, x, t, G_UP)
    assert bool(torch.isnan(g_t).any())
    l64, g64 = R.closed_form(R.HELLINGER, x.double().cpu(), t.double().cpu())
    g64 = g64 * G_UP
    loss, gunit = capi_fwd(x, t, R.HELLINGER)
    gx = capi_bwd(gunit, G_UP, torch.float32)
    assert bool(torch.isfinite(gx).all())
    g_c32 = R.closed_form(R.HELLINGER, x, t)[1] * G_UP
    assert bool(torch.isfinite(g_c32).all())
    g_t_finite = torch.where(torch.isfinite(g_t), g_t, g_c32).double().cpu()
    ok, fig = R.within_bar(loss, gx, (l_t, g_t_finite), (l64, g64))
    print("hellinger underflow", fig)
    assert ok, fig


# ---------------------------------------------------------------------------------------------- exactness and structure
@pytest.mark.parametrize("shape", [(5, 37), (16, 1001), (250, 1000), (4, 4097)], ids=ids_shape)
@pytest.mark.parametrize("kind", R.ZERO_AT_EQUAL, ids=ids_kind)
def test_a_target_with_the_bits_of_the_input_gives_exactly_zero(kind, shape):
    x, _ = _case(shape)
    loss, gunit = capi_fwd(x, x.clone(), kind)
    assert float(loss) == 0.0
    assert bool((capi_bwd(gunit, G_UP, torch.float32) == 0).all())


@pytest.mark.parametrize("shape", [(5, 37), (8, 1000), (4, 4097)], ids=ids_shape)
@pytest.mark.parametrize("kind", R.KINDS, ids=ids_kind)
def test_a_nan_turns_its_own_row_to_nan_and_leaves_the_other_rows_bits(kind, shape):
    x, t = R.logits(shape, 2.0, seed=11, device=DEV)
    loss0, gunit0 = capi_fwd(x, t, kind)
    gx0 = capi_bwd(gunit0, G_UP, torch.float32)
    for side, val in (("x", float("nan")), ("t", float("nan")), ("x", float("inf"))):
        xn, tn = x.clone(), t.clone()
        (xn if side == "x" else tn)[1, shape[1] // 2] = val
        loss, gunit = capi_fwd(xn, tn, kind)
        gx = capi_bwd(gunit, G_UP, torch.float32)
        assert bool(torch.isnan(loss).all()) and bool(torch.isfinite(loss0).all())
        assert bool(torch.isnan(gx[1]).all()), (side, val)
        keep = [r for r in range(shape[0]) if r != 1]
        assert torch.equal(_bits(gx[keep]), _bits(gx0[keep]))


@pytest.mark.parametrize("kind", R.KINDS, ids=ids_kind)
def test_logits_at_plus_and_minus_1e4_do_not_overflow(kind):
    for base, shape in ((1e4, (5, 37)), (-1e4, (4, 4097))):
        x, t = R.logits(shape, 1.0, seed=5, device=DEV)
        x, t = x + base, t + base
        chain, ref = R.chain32(kind, x, t, G_UP), R.autograd64(kind, x, t, G_UP)
        loss, gunit = capi_fwd(x, t, kind)
        gx = capi_bwd(gunit, G_UP, torch.float32)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gx).all())
        ok, fig = R.within_bar(loss, gx, chain, ref)
        assert ok, fig


# ---------------------------------------------------------------------------------------------- 16-bit
@pytest.mark.parametrize("dts", [(torch.bfloat16, torch.float32), (torch.float32, torch.bfloat16),
                                 (torch.bfloat16, torch.bfloat16), (torch.float16, torch.float32),
                                 (torch.float32, torch.float16), (torch.float16, torch.float16),
                                 (torch.bfloat16, torch.float16)], ids=lambda d: "-".join(str(x)[6:] for x in d))
@pytest.mark.parametrize("kind", R.KINDS, ids=ids_kind)
def test_16_bit_inputs_equal_the_fp32_entry_on_the_upcast_inputs(kind, dts):
    """loss and gunit bit for bit, gx its nearest-even rounding, and the float64 bar on the upcast inputs: 5x37 and 16x1001
    (odd: unaligned 16-bit row bases), 6x100 (16-bit rows at 8-byte bases: the group layout), 4x1000, 2x4100 (walked)."""
    for shape in ((5, 37), (16, 1001), (6, 100), (4, 1000), (2, 4100)):
        x32, t32 = R.logits(shape, 3.0, seed=17 + shape[1], device=DEV)
        x, t = x32.to(dts[0]), t32.to(dts[1])
        xu, tu = x.float(), t.float()
        loss, gunit = capi_fwd(x, t, kind)
        loss_u, gunit_u = capi_fwd(xu, tu, kind)
        assert torch.equal(_bits(loss), _bits(loss_u)) and torch.equal(_bits(gunit), _bits(gunit_u)), shape
        gx = capi_bwd(gunit, G_UP, dts[0], shift=1)
        gx_u = capi_bwd(gunit_u, G_UP, torch.float32)
        assert gx.dtype == dts[0] and torch.equal(_bits(gx), _bits(gx_u.to(dts[0]))), shape
        ok, fig = R.within_bar(loss, gx_u, R.chain32(kind, xu, tu, G_UP), R.autograd64(kind, xu, tu, G_UP))
        assert ok, (shape, fig)


# ---------------------------------------------------------------------------------------------- module
def test_module_under_autocast_behind_a_linear_head_and_on_other_shapes():
    from mhaq_amd._lib import MhaqFqError
    from mhaq_amd.loss import FusedDistillLoss
    torch.manual_seed(3)
    head = torch.nn.Linear(64, 37).to(DEV)
    feat = torch.randn(10, 64, device=DEV)
    teacher = torch.randn(10, 37, device=DEV)
    crit = FusedDistillLoss("Symmetrical KL")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = head(feat)
        out.retain_grad()
        loss = crit(out, teacher.to(torch.bfloat16))
    assert out.dtype == torch.bfloat16 and loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    assert out.grad.dtype == torch.bfloat16 and head.weight.grad.dtype == torch.float32
    assert bool(torch.isfinite(head.weight.grad).all()) and float(head.weight.grad.abs().max()) > 0
    want, gunit = capi_fwd(out.detach(), teacher.to(torch.bfloat16), R.SKL)
    assert torch.equal(_bits(loss.detach().reshape(1)), _bits(want))
    assert torch.equal(_bits(out.grad), _bits(capi_bwd(gunit, 1.0, torch.bfloat16)))
    # any shape is [-1, C] over its last dimension; a non-dense input is made contiguous
    x, t = R.logits((10, 37), 2.0, seed=2, device=DEV)
    flat = crit(x, t)
    assert torch.equal(crit(x.reshape(2, 5, 37), t.reshape(2, 5, 37)), flat)
    xt = x.t().contiguous().t()
    assert not xt.is_contiguous() and torch.equal(crit(xt, t), flat)
    with pytest.raises(MhaqFqError):
        crit(x.cpu(), t.cpu())
    with pytest.raises(MhaqFqError):
        crit(x, t.cpu())


# ---------------------------------------------------------------------------------------------- trainer
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
                    excluded_layers=("features.init_block.conv", "output"), warmup=3, distillation=True,
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


def test_fused_trainer_first_step_counter_and_captured_replays(_deterministic, monkeypatch):
    from mhaq_amd import loss as L
    monkeypatch.delenv(L.ENV_SWITCH_DISTILL, raising=False)
    batches = _batches(6)
    # the default trainer: today's objects, no fused launch
    n0 = L.distill_fused_launches()
    default = _make(False)
    assert type(default.loss.criterion) is L.SymmetricalKL
    seen = []
    hook = default.loss.criterion.register_forward_hook(lambda m, inp, out: seen.append((inp[0].detach().clone(),
                                                                                         inp[1].detach().clone())))
    default.train_step(*batches[0])
    hook.remove()
    l_torch = float(default.loss.base_loss)
    assert L.distill_fused_launches() == n0
    # the fused trainer from the same state: the first step's distillation loss within the bar of the default trainer's
    eager = _make(False, fused_distill_loss=True)
    assert type(eager.loss.criterion) is L.FusedDistillLoss and eager.loss.criterion.kind == R.SKL
    le = [float(eager.train_step(*batches[0]))]
    l_fused = float(eager.loss.base_loss)
    assert L.distill_fused_launches() - n0 == 3                  # two launches forward, one backward
    (logits, target), = seen
    l64, _ = R.autograd64(R.SKL, logits, target)
    print("trainer first step", dict(l_fused=l_fused, l_torch=l_torch, l64=float(l64)))
    assert abs(l_fused - float(l64)) <= R.loss_bar(l_torch, l64)
    le += [float(eager.train_step(x, y)) for x, y in batches[1:]]
    assert L.distill_fused_launches() - n0 == 3 * 6
    # captured: three eager steps, then three replays with the losses of the eager fused run
    graphed = _make(True, fused_distill_loss=True)
    lg = [float(graphed.train_step(x, y)) for x, y in batches]
    assert graphed._graph is not None and graphed._eager_steps == 3
    assert all(torch.isfinite(torch.tensor(lg))) and le == lg
    for (n, a), (_, b) in zip(eager.net.named_parameters(), graphed.net.named_parameters()):
        assert torch.equal(a, b), n


def test_environment_switch_decides_and_an_unknown_name_raises(_deterministic, monkeypatch):
    from mhaq_amd import loss as L
    monkeypatch.setenv(L.ENV_SWITCH_DISTILL, "1")
    assert type(_make(False).loss.criterion) is L.FusedDistillLoss
    monkeypatch.setenv(L.ENV_SWITCH_DISTILL, "0")
    assert type(_make(False, fused_distill_loss=True).loss.criterion) is L.SymmetricalKL
    tr = _make(False, distillation_loss="JSD")                  # the new names are fused either way
    assert type(tr.loss.criterion) is L.FusedDistillLoss and tr.loss.criterion.kind == R.JSD
    assert bool(torch.isfinite(tr.train_step(*_batches(1)[0])))
    with pytest.raises(NotImplementedError):
        _make(False, distillation_loss="Huber")


def test_l1_distillation_on_the_rfdn_model_runs_a_step(monkeypatch):
    import mhaq_amd as M
    from mhaq_amd import loss as L, nets, ops
    from mhaq_amd.qat import QATConfig, QATTrainer
    monkeypatch.delenv(L.ENV_SWITCH_DISTILL, raising=False)
    torch.manual_seed(1)
    ops.manual_seed(1)
    g = torch.Generator().manual_seed(70)
    x = (torch.rand(2, 3, 24, 24, generator=g) * 255.0).to(DEV)
    y = (torch.rand(2, 3, 96, 96, generator=g) * 255.0).to(DEV)
    cfg = QATConfig(qscheme=M.QScheme.PER_CHANNEL, qnmethod=M.QNMethod.LSQ, act_bit=4, weight_bit=4, distillation=True,
                    distillation_loss="L1", excluded_layers=("fea_conv", "upsampler.0"), learning_rate=5e-4, warmup=2)
    n0 = L.distill_fused_launches()
    tr = QATTrainer(nets.RFDN(nf=16), cfg, DEV, calib_batches=[x], capture_graph=False)
    assert type(tr.loss.criterion) is torch.nn.L1Loss
    assert bool(torch.isfinite(tr.train_step(x, y)))
    assert L.distill_fused_launches() == n0
