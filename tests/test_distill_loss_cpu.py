"""CPU: everything about the fused distillation losses (mhaq_fq_distill_loss_fwd / _bwd, mhaq_amd/loss.py:
FusedDistillLoss) that needs no GPU -- the symbols, the argument errors, the closed forms of the header's table against
float64 autograd through the reference modules' torch statements, the routing of the config names, the switch and the
QATConfig defaults.  The kernels are held to the same yardstick on the device by tests/test_gpu_distill_loss.py."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch
from torch import nn

from mhaq_amd import _lib, loss as L
from mhaq_amd.qat import QATConfig
from tests import distill_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES3 = ("mhaq_fq_distill_loss_workspace_bytes", "mhaq_fq_distill_loss_fwd", "mhaq_fq_distill_loss_bwd")


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_exported_and_bound_with_the_headers_arity():
    raw = open(_lib.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.lib()
    for name in NAMES3:
        assert name in _lib.header_functions() and name in _lib.SIGNATURES
        assert hasattr(lib, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1])
    assert lib.mhaq_fq_abi_version() == 4 and re.search(r"#define MHAQ_FQ_ABI_VERSION 4\b", raw)
    assert re.search(r"MHAQ_FQ_DT_F32 = 0\b.*MHAQ_FQ_DT_BF16 = 1, MHAQ_FQ_DT_F16 = 2", src)
    assert (_lib.DT_F32, _lib.DT_BF16, _lib.DT_F16) == (0, 1, 2)
    for i, k in enumerate(("CE", "SCE", "KL", "SKL", "JSD", "HELLINGER")):
        assert re.search(r"MHAQ_FQ_DISTILL_%s = %d\b" % (k, i), src)
    assert [L.DISTILL_KINDS[R.NAMES[k]] for k in R.KINDS] == R.KINDS
    mk = open(os.path.join(ROOT, "mhaq_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRC\s*=.*\bdistill\.hip\b", mk, flags=re.M)
    assert "-ffp-contract=off" in mk and "-fno-gpu-approx-transcendentals" in mk
    binding = open(os.path.join(ROOT, "mhaq_amd", "csrc", "torch_binding.cpp")).read()
    assert 'm.def("distill_loss"' in binding and 'm.def("distill_fused_launches"' in binding
    for name in NAMES3:
        assert "X(%s)" % name in binding


def test_argument_errors_come_before_any_launch():
    lib = _lib.lib()
    fake, odd2, odd1 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002), ctypes.c_void_p(0x1001)
    ws4 = ctypes.c_void_p(0x1004)
    assert lib.mhaq_fq_distill_loss_workspace_bytes(250) == 250 * 8
    f = lib.mhaq_fq_distill_loss_fwd

    def fwd(x=fake, xdt=0, t=fake, tdt=0, rows=4, cols=10, kind=3, loss=fake, gunit=None, ws=fake, wsb=4 * 8):
        return f(x, xdt, t, tdt, rows, cols, kind, loss, gunit, ws, wsb, None)
    for kw in (dict(x=None), dict(t=None), dict(loss=None), dict(ws=None), dict(rows=0), dict(rows=-1), dict(cols=0),
               dict(cols=-5), dict(kind=6), dict(kind=-1), dict(xdt=3), dict(tdt=-1)):
        assert fwd(**kw) == -1, kw
    assert fwd(wsb=4 * 8 - 1) == -2
    assert fwd(x=None, wsb=0) == -1                                  # the library's order: -1 before -2 before -3 before -4
    assert fwd(x=odd2, wsb=0) == -2
    for kw in (dict(x=odd2), dict(t=odd2), dict(x=odd1, xdt=1), dict(t=odd1, tdt=2), dict(loss=odd2), dict(gunit=odd2),
               dict(ws=ws4)):
        assert fwd(**kw) == -3, kw
    big = 1 << 31
    assert fwd(rows=big, wsb=big * 8) == -4
    assert fwd(rows=big, wsb=big * 8, x=odd2) == -3
    assert fwd(rows=big, wsb=8) == -2
    b = lib.mhaq_fq_distill_loss_bwd
    for args in ((None, fake, fake, 0, 8), (fake, None, fake, 0, 8), (fake, fake, None, 0, 8), (fake, fake, fake, 3, 8),
                 (fake, fake, fake, 0, 0), (fake, fake, fake, 0, -1)):
        assert b(*args, None) == -1, args
    for args in ((odd2, fake, fake, 0, 8), (fake, odd2, fake, 0, 8), (fake, fake, odd2, 0, 8), (fake, fake, odd1, 1, 8),
                 (fake, fake, odd1, 2, 8)):
        assert b(*args, None) == -3, args


# ---------------------------------------------------------------------------------------------- the closed forms
@pytest.mark.parametrize("shape", R.CPU_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", R.KINDS, ids=lambda k: R.NAMES[k])
def test_closed_forms_equal_float64_autograd_through_the_torch_statements(kind, shape):
    for scale in (1.0, 8.0):
        x, t = R.logits(shape, scale, seed=100 * kind + shape[1])
        want_l, want_g = R.autograd64(kind, x, t)
        got_l, got_g = R.closed_form(kind, x.double(), t.double())
        assert abs(float(got_l) - float(want_l)) <= 1e-9 * max(abs(float(want_l)), 1e-30)
        assert float((got_g - want_g).abs().max()) <= 1e-9 * float(want_g.abs().max())


@pytest.mark.parametrize("kind", R.KINDS, ids=lambda k: R.NAMES[k])
def test_a_float32_run_of_the_closed_forms_meets_the_bar_of_the_gpu_tests(kind):
    """The yardstick is usable: closed forms in float32 sit within the bar the GPU tests hold the kernels to, and a wrong
    denominator does not.  (5x37 and 16x1001: over the two elements of 1x2 the framework's own error, which the bar
    scales, can be next to nothing by luck.)"""
    for shape in R.CPU_SHAPES[1:]:
        x, t = R.logits(shape, 4.0, seed=7 * kind + shape[0])
        ref = R.autograd64(kind, x, t, 0.37)
        chain = R.chain32(kind, x, t, 0.37)
        l32, g32 = R.closed_form(kind, x, t)
        ok, fig = R.within_bar(l32, g32 * 0.37, chain, ref)
        assert ok, (shape, fig)
        ok, fig = R.within_bar(l32 * 1.001, g32 * 0.37 * 1.001, chain, ref)
        assert not ok, (shape, fig)


def test_hellinger_framework_gradient_is_nan_where_a_probability_underflows_and_the_closed_form_is_finite():
    x, t = R.logits((2, 10007), 20.0, seed=3)
    assert bool((x.softmax(-1) == 0).any())
    _, g = R.chain32(R.HELLINGER, x, t)
    assert bool(torch.isnan(g).any())
    _, g64 = R.closed_form(R.HELLINGER, x.double(), t.double())
    assert bool(torch.isfinite(g64).all())


# ---------------------------------------------------------------------------------------------- routing and switches
@pytest.mark.parametrize("fused", [False, True])
def test_the_eight_config_names_route_and_an_unknown_one_raises(fused):
    assert type(L.distillation_criterion("L1", fused)) is nn.L1Loss
    assert type(L.distillation_criterion("L2", fused)) is nn.MSELoss
    skl = L.distillation_criterion("Symmetrical KL", fused)
    assert type(skl) is (L.FusedDistillLoss if fused else L.SymmetricalKL)
    if fused:
        assert skl.kind == R.SKL
    for kind in (R.CE, R.SCE, R.KL, R.JSD, R.HELLINGER):
        m = L.distillation_criterion(R.NAMES[kind], fused)
        assert type(m) is L.FusedDistillLoss and m.kind == kind and m.name == R.NAMES[kind]
    assert len({"L1", "L2"} | set(L.DISTILL_KINDS)) == 8
    for bad in ("Huber", "", "kl", "symmetrical kl"):
        with pytest.raises(NotImplementedError):
            L.distillation_criterion(bad, fused)
    with pytest.raises(NotImplementedError):
        L.FusedDistillLoss("L1")
    with pytest.raises(NotImplementedError):
        L.FusedDistillLoss(6)
    assert L.FusedDistillLoss(5).name == "Hellinger"


def test_switch_and_config_defaults(monkeypatch):
    fields = {f.name: f for f in dataclasses.fields(QATConfig)}
    assert fields["distillation_loss"].default == "Symmetrical KL"
    assert fields["fused_distill_loss"].default is False
    assert L.ENV_SWITCH_DISTILL == "MHAQ_DISTILL_FUSED"
    monkeypatch.delenv(L.ENV_SWITCH_DISTILL, raising=False)
    assert L.distill_fused_enabled(True) is True and L.distill_fused_enabled(False) is False
    assert L.distill_fused_enabled() is False
    for v, want in (("1", True), ("true", True), ("on", True), ("yes", True), ("0", False), ("off", False), ("no", False)):
        monkeypatch.setenv(L.ENV_SWITCH_DISTILL, v)
        assert L.distill_fused_enabled(True) is want and L.distill_fused_enabled(False) is want
    monkeypatch.setenv(L.ENV_SWITCH_DISTILL, " ")
    assert L.distill_fused_enabled(True) is True and L.distill_fused_enabled(False) is False
    # with the defaults the trainer's criterion is the framework chain it always built
    monkeypatch.delenv(L.ENV_SWITCH_DISTILL, raising=False)
    cfg = QATConfig()
    assert type(L.distillation_criterion(cfg.distillation_loss, L.distill_fused_enabled(cfg.fused_distill_loss))) \
        is L.SymmetricalKL


def test_a_cpu_tensor_raises():
    x, t = R.logits((5, 37), 1.0, seed=1)
    for kind in R.KINDS:
        with pytest.raises(_lib.MhaqFqError):
            L.FusedDistillLoss(R.NAMES[kind])(x, t)
