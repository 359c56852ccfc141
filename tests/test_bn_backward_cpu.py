"""CPU: the BatchNorm backward plumbing (mhaq_amd/bn_backward.py, BatchNormTrainFn in csrc/torch_binding.cpp,
mhaq_fq_bn_bwd in csrc/bn_bwd.hip) as far as it goes without a device: the C ABI exports the entry points and returns
its argument errors before any launch; install / uninstall change no name, no state_dict key and no copy; on CPU tensors
the switched module IS the stock one, and the compiled node's fallback branch equals F.batch_norm bit for bit."""
import copy
import ctypes
import os
import subprocess

import pytest
import torch
from torch import nn

from mhaq_amd import _lib, bn_backward


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbols_are_exported_and_declared(L):
    for name in ("mhaq_fq_bn_bwd_workspace_bytes", "mhaq_fq_bn_bwd"):
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
    assert L.mhaq_fq_abi_version() == 4


def test_workspace_query_keeps_the_partial_rows_below_one_percent(L):
    # the 20 BatchNorm tensors of ResNet-18 at batch 250 and a few odd ones: 5 fp32 constant rows + 2 fp64 rows per row chunk
    for m, c in [(250 * 112 * 112, 64), (250 * 56 * 56, 64), (250 * 28 * 28, 128), (250 * 14 * 14, 256),
                 (250 * 7 * 7, 512), (1 << 20, 4), (1 << 22, 20), (10 ** 9, 8)]:
        nb = L.mhaq_fq_bn_bwd_workspace_bytes(m, c)
        assert nb % (4 * c) == 0 and nb >= (5 * 4 + 2 * 8) * c
        partial_bytes = nb - 5 * 4 * c
        assert partial_bytes < 0.01 * (4 * m * c), (m, c, partial_bytes)
    assert L.mhaq_fq_bn_bwd_workspace_bytes(2, 4) == (5 * 4 + 2 * 8) * 4          # one row chunk
    assert L.mhaq_fq_bn_bwd_workspace_bytes(16, 6) == 0 and L.mhaq_fq_bn_bwd_workspace_bytes(0, 8) == 0


def test_argument_errors_are_returned_before_any_launch(L):
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    nb = L.mhaq_fq_bn_bwd_workspace_bytes(64, 8)
    call = L.mhaq_fq_bn_bwd
    assert call(None, fake, fake, fake, fake, fake, fake, fake, 64, 8, fake, nb, None) == -1
    assert call(fake, None, fake, fake, fake, fake, fake, fake, 64, 8, fake, nb, None) == -1
    assert call(fake, fake, None, fake, fake, fake, fake, fake, 64, 8, fake, nb, None) == -1
    assert call(fake, fake, fake, None, fake, fake, fake, fake, 64, 8, fake, nb, None) == -1
    assert call(fake, fake, fake, fake, fake, fake, fake, fake, 0, 8, fake, nb, None) == -1
    assert call(fake, fake, fake, fake, fake, fake, fake, fake, 64, 0, fake, nb, None) == -1
    assert call(fake, fake, fake, fake, fake, fake, fake, fake, 64, 8, None, nb, None) == -1
    assert call(fake, fake, fake, fake, fake, fake, fake, fake, 64, 8, fake, nb - 1, None) == -2
    assert call(fake, fake, fake, fake, fake, fake, fake, fake, 64, 8, fake, 0, None) == -2
    for k in (0, 1, 5, 10):                       # x, dy, dx, workspace: 16-byte aligned
        args = [fake] * 8 + [64, 8, fake, nb, None]
        args[k] = odd
        assert call(*args) == -3, k
    assert call(fake, fake, ctypes.c_void_p(0x1002), fake, fake, fake, fake, fake, 64, 8, fake, nb, None) == -3
    assert call(fake, fake, fake, fake, fake, fake, fake, fake, 64, 6, fake, 1 << 20, None) == -4       # C % 4
    assert call(fake, fake, fake, fake, fake, fake, fake, fake, 4, 1 << 23, fake, 1 << 40, None) == -4
    # nothing to compute: no launch, no error (weight and every output are optional)
    assert call(fake, fake, fake, fake, None, None, None, None, 64, 8, fake, nb, None) == 0


def test_argument_errors_come_in_a_fixed_order(L):
    """Several things wrong at once: NULL / size first, then the width, then the workspace, then the alignment."""
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    nb = L.mhaq_fq_bn_bwd_workspace_bytes(64, 8)
    call = L.mhaq_fq_bn_bwd

    def with_(x=fake, dy=odd, m=64, c=6, ws=fake, nbytes=0):
        return call(x, dy, fake, fake, fake, fake, fake, fake, m, c, ws, nbytes, None)
    assert with_(x=None) == -1 and with_(m=0) == -1 and with_(ws=None) == -1
    assert with_(c=0) == -1 and with_(c=-4) == -1
    assert with_() == -4                                          # C % 4 before the workspace and the alignment
    assert with_(m=4, c=1 << 23) == -4 and with_(m=1 << 60, c=8) == -4
    assert with_(c=8) == -2                                       # the workspace before the alignment
    assert with_(c=8, nbytes=nb - 1) == -2
    assert with_(c=8, nbytes=nb) == -3


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(),
                         nn.Sequential(nn.Conv2d(8, 8, 3), nn.BatchNorm2d(8, momentum=None)),
                         nn.SyncBatchNorm(8), nn.BatchNorm2d(8, affine=False), nn.BatchNorm1d(8))


def test_install_keeps_names_keys_copies_and_isinstance():
    net = _net()
    names = [(n, type(m).__name__) for n, m in net.named_modules()]
    keys = list(net.state_dict().keys())
    assert bn_backward.install(net) == 3
    after = [(n, type(m).__name__) for n, m in net.named_modules()]
    assert [n for n, _ in after] == [n for n, _ in names]
    assert {(a[1], b[1]) for a, b in zip(names, after) if a[1] != b[1]} == {("BatchNorm2d", "HipBackwardBatchNorm2d")}
    assert list(net.state_dict().keys()) == keys
    assert isinstance(net[1], nn.BatchNorm2d) and type(net[4]) is nn.SyncBatchNorm and type(net[6]) is nn.BatchNorm1d
    assert bn_backward.install(net) == 0             # idempotent
    dup = copy.deepcopy(net)
    assert type(dup[1]) is bn_backward.HipBackwardBatchNorm2d and list(dup.state_dict().keys()) == keys
    assert all(torch.equal(a, b) for a, b in zip(dup.state_dict().values(), net.state_dict().values()))
    bn_backward.uninstall(net)
    assert [(n, type(m).__name__) for n, m in net.named_modules()] == names


def test_env_switch(monkeypatch):
    monkeypatch.delenv(bn_backward.ENV_SWITCH, raising=False)
    assert bn_backward.enabled_by_env()
    for v in ("0", "false", "off"):
        monkeypatch.setenv(bn_backward.ENV_SWITCH, v)
        assert not bn_backward.enabled_by_env()
    monkeypatch.setenv(bn_backward.ENV_SWITCH, "1")
    assert bn_backward.enabled_by_env()
    from mhaq_amd.qat import QATConfig
    assert QATConfig().hip_bn_backward is True


def _run(bn, x, g):
    x = x.clone().requires_grad_(True)
    y = bn(x)
    y.backward(g)
    return [y.detach(), x.grad] + [p.grad for p in bn.parameters()] + [bn.running_mean.clone(), bn.running_var.clone(),
                                                                      bn.num_batches_tracked.clone()]


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("momentum", [0.1, None])
def test_switched_module_equals_stock_on_cpu_tensors(layout, momentum):
    torch.manual_seed(1)
    x, g = torch.randn(3, 8, 5, 4) * 2 + 1, torch.randn(3, 8, 5, 4)
    if layout == "channels_last":
        x, g = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
    stock = nn.BatchNorm2d(8, momentum=momentum)
    with torch.no_grad():
        stock.weight.uniform_(-1, 1)
        stock.bias.uniform_(-1, 1)
    mine = copy.deepcopy(stock)
    assert bn_backward.install(mine) == 1
    for _ in range(2):                               # two steps: the running statistics and the counter move alike
        for a, b in zip(_run(stock, x, g), _run(mine, x, g)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_compiled_node_fallback_equals_f_batch_norm_on_cpu(layout):
    """The node itself on CPU tensors: the framework's forward and, since nothing of the HIP path applies, the backward
    autograd would have run -- y, dx, dgamma, dbeta and both running statistics bit for bit."""
    import torch.nn.functional as F
    from mhaq_amd import _ext
    E = _ext.ext()
    torch.manual_seed(2)
    x, g = torch.randn(4, 8, 3, 5) * 3 - 2, torch.randn(4, 8, 3, 5)
    if layout == "channels_last":
        x, g = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
    outs = []
    for fn in (lambda *a: F.batch_norm(a[0], a[3], a[4], a[1], a[2], True, 0.1, 1e-5),
               lambda *a: E.bn_train(a[0], a[1], a[2], a[3], a[4], 0.1, 1e-5, True)):
        xi = x.clone().requires_grad_(True)
        w, b = torch.linspace(-1, 1, 8).requires_grad_(True), torch.linspace(0, 1, 8).requires_grad_(True)
        rm, rv = torch.zeros(8), torch.ones(8)
        y = fn(xi, w, b, rm, rv)
        y.backward(g)
        outs.append((y.detach(), xi.grad, w.grad, b.grad, rm, rv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # frozen affine parameters: the output mask is honoured
    xi = x.clone().requires_grad_(True)
    w, b = torch.ones(8), torch.zeros(8, requires_grad=True)
    E.bn_train(xi, w, b, torch.zeros(8), torch.ones(8), 0.1, 1e-5, True).backward(g)
    assert w.grad is None and torch.equal(b.grad, outs[0][3]) and xi.grad is not None


def test_syncbatchnorm_eval_and_frozen_modules_are_left_alone(monkeypatch):
    """None of them may reach the compiled node: SyncBatchNorm keeps its class, an eval-mode module (the frozen teacher:
    eval(), requires_grad_(False)) and one without tracked statistics or affine parameters run nn.BatchNorm2d.forward."""
    from mhaq_amd import _ext

    def boom():
        raise AssertionError("the compiled node must not be reached")
    monkeypatch.setattr(_ext, "ext", boom)
    torch.manual_seed(3)
    x = torch.randn(2, 8, 4, 4)
    sync = nn.SyncBatchNorm(8)
    assert bn_backward.install(sync) == 0 and type(sync) is nn.SyncBatchNorm
    for make in (lambda: nn.BatchNorm2d(8).eval().requires_grad_(False),
                 lambda: nn.BatchNorm2d(8, track_running_stats=False),
                 lambda: nn.BatchNorm2d(8, affine=False),
                 lambda: nn.BatchNorm2d(8).requires_grad_(False)):
        stock = make()
        mine = copy.deepcopy(stock)
        bn_backward.install(mine)
        assert type(mine) is bn_backward.HipBackwardBatchNorm2d
        assert torch.equal(stock(x), mine(x))                    # CPU tensor: the stock forward, whatever the mode
        assert all(torch.equal(a, b) for a, b in zip(stock.state_dict().values(), mine.state_dict().values()))
