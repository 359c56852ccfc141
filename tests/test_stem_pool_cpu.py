"""CPU: the stem pool's plumbing as far as it goes without a device (mhaq_amd/fused_blocks.py "Stem pool",
HipBackwardBatchNorm2d.forward_pooled, bn_pool_train in csrc/torch_binding.cpp, mhaq_fq_maxpool3s2_fwd /
mhaq_fq_bn_pool_bwd in csrc/bn_bwd.hip): the C ABI exports the entry points and returns its argument errors before any
launch; the switch; install / uninstall change no name and no state_dict key; on CPU tensors the node IS
max_pool2d(F.batch_norm(..)), bit for bit, and its counter says so."""
import copy
import ctypes
import io
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from mhaq_amd import _lib, bn_backward, fused_blocks

NAMES = ("mhaq_fq_maxpool3s2_fwd", "mhaq_fq_bn_pool_bwd_workspace_bytes", "mhaq_fq_bn_pool_bwd")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbols_are_exported_and_declared(L):
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
    assert L.mhaq_fq_abi_version() == 4


def test_workspace_query_is_the_batchnorm_backwards_own(L):
    for n, h, w, c in [(250, 112, 112, 64), (1, 1, 1, 4), (3, 5, 7, 20), (2, 7, 7, 512)]:
        nb = L.mhaq_fq_bn_pool_bwd_workspace_bytes(n, h, w, c)
        assert nb > 0 and nb == L.mhaq_fq_bn_bwd_workspace_bytes(n * h * w, c)
    assert L.mhaq_fq_bn_pool_bwd_workspace_bytes(2, 4, 4, 6) == 0                 # C % 4
    assert L.mhaq_fq_bn_pool_bwd_workspace_bytes(0, 4, 4, 8) == 0
    assert L.mhaq_fq_bn_pool_bwd_workspace_bytes(1 << 11, 1 << 10, 1 << 10, 8) == 0      # n * h * w = 2^31


def test_argument_errors_are_returned_before_any_launch(L):
    fake, odd, odd2 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1002)
    n, h, w, c = 2, 5, 4, 8
    nb = L.mhaq_fq_bn_pool_bwd_workspace_bytes(n, h, w, c)
    bwd = L.mhaq_fq_bn_pool_bwd
    ok = [fake] * 9 + [n, h, w, c, fake, nb, None]
    for k in (0, 1, 2, 3, 4, 13):                   # x, g, code, mean, invstd, workspace: required
        args = list(ok)
        args[k] = None
        assert bwd(*args) == -1, k
    for k in (9, 10, 11, 12):                       # n, h, w, c: positive
        args = list(ok)
        args[k] = 0
        assert bwd(*args) == -1, k
    args = list(ok)
    args[14] = nb - 1
    assert bwd(*args) == -2
    for k in (0, 1, 6, 13):                         # x, g, dx, workspace: 16-byte aligned
        args = list(ok)
        args[k] = odd
        assert bwd(*args) == -3, k
    for k in (2, 3, 4, 5, 7, 8):                    # code, mean, invstd, weight, dweight, dbias: 4-byte aligned
        args = list(ok)
        args[k] = odd2
        assert bwd(*args) == -3, k
    args = list(ok)
    args[12] = 6
    assert bwd(*args) == -4                         # C % 4
    args = list(ok)
    args[9], args[10], args[11], args[14] = 1 << 11, 1 << 10, 1 << 10, 1 << 62
    assert bwd(*args) == -4                         # n * h * w >= 2^31: the pixel arithmetic is 32-bit
    # nothing to compute: no launch, no error (weight and every output are optional)
    assert bwd(fake, fake, fake, fake, fake, None, None, None, None, n, h, w, c, fake, nb, None) == 0
    fwd = L.mhaq_fq_maxpool3s2_fwd
    ok = [fake, fake, fake, n, h, w, c, None]
    for k in (0, 1, 2):
        args = list(ok)
        args[k] = None
        assert fwd(*args) == -1, k
    for k in (3, 4, 5, 6):
        args = list(ok)
        args[k] = 0
        assert fwd(*args) == -1, k
    for k, bad in ((0, odd), (1, odd), (2, odd2)):
        args = list(ok)
        args[k] = bad
        assert fwd(*args) == -3, k
    assert fwd(fake, fake, fake, n, h, w, 6, None) == -4
    assert fwd(fake, fake, fake, 1 << 11, 1 << 10, 1 << 10, 8, None) == -4


def test_argument_errors_come_in_a_fixed_order(L):
    """Several things wrong at once: NULL first, then the dimensions, then the workspace, then the alignment."""
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    n, h, w = 2, 5, 4
    nb = L.mhaq_fq_bn_pool_bwd_workspace_bytes(n, h, w, 8)

    def bwd(x=fake, g=odd, n=n, c=6, nbytes=0):
        return L.mhaq_fq_bn_pool_bwd(x, g, fake, fake, fake, fake, fake, fake, fake, n, h, w, c, fake, nbytes, None)
    assert bwd(x=None) == -1
    assert bwd(n=0) == -1 and bwd(c=0) == -1                      # a size that is not positive before one that is unsupported
    assert bwd() == -4                                            # C % 4 before the workspace and the alignment
    assert bwd(n=1 << 31, c=8) == -4
    assert bwd(c=8) == -2                                         # the workspace before the alignment
    assert bwd(c=8, nbytes=nb - 1) == -2
    assert bwd(c=8, nbytes=nb) == -3

    def fwd(t=fake, p=odd, n=n, c=6):
        return L.mhaq_fq_maxpool3s2_fwd(t, p, fake, n, h, w, c, None)
    assert fwd(t=None) == -1
    assert fwd(n=0) == -1 and fwd(c=0) == -1
    assert fwd() == -4                                            # C % 4 before the alignment
    assert fwd(n=1 << 31, c=8) == -4
    assert fwd(c=8) == -3


def test_switches(monkeypatch):
    from mhaq_amd.qat import QATConfig
    assert QATConfig().fuse_stem_pool is True
    assert fused_blocks.ENV_SWITCH_STEM_POOL == "MHAQ_STEM_POOL"
    monkeypatch.delenv(fused_blocks.ENV_SWITCH_STEM_POOL, raising=False)
    assert fused_blocks.stem_pool_enabled_by_env()
    for v in ("0", "false", "off"):
        monkeypatch.setenv(fused_blocks.ENV_SWITCH_STEM_POOL, v)
        assert not fused_blocks.stem_pool_enabled_by_env()
    monkeypatch.setenv(fused_blocks.ENV_SWITCH_STEM_POOL, "1")
    assert fused_blocks.stem_pool_enabled_by_env()


def test_only_the_stems_own_pool_geometry_is_taken():
    yes = [nn.MaxPool2d(3, 2, 1), nn.MaxPool2d((3, 3), (2, 2), (1, 1)), nn.MaxPool2d(kernel_size=3, stride=2, padding=1, dilation=1)]
    no = [nn.MaxPool2d(2, 2), nn.MaxPool2d(3, 2), nn.MaxPool2d(3, 1, 1), nn.MaxPool2d(3, 2, 1, dilation=2),
          nn.MaxPool2d(3, 2, 1, ceil_mode=True), nn.MaxPool2d(3, 2, 1, return_indices=True), nn.MaxPool2d((3, 2), 2, 1),
          nn.AvgPool2d(3, 2, 1)]
    assert all(fused_blocks._is_stem_pool(m) for m in yes)
    assert not any(fused_blocks._is_stem_pool(m) for m in no)

    class Sub(nn.MaxPool2d):
        pass
    assert not fused_blocks._is_stem_pool(Sub(3, 2, 1))


def _quantized():
    import mhaq_amd as M
    from mhaq_amd import nets, wrap
    net = nets.resnet18(10)
    wrap.quantize_model(net, M.QScheme.PER_CHANNEL, M.QNMethod.AEWGS, ("conv1", "fc"), False, 4)
    return net


@pytest.mark.parametrize("stem_pool", [True, False])
def test_install_uninstall_keep_names_keys_and_copies(stem_pool):
    net = _quantized()
    names = [(n, type(m).__name__) for n, m in net.named_modules()]
    keys = list(net.state_dict().keys())
    assert fused_blocks.install(net, stem_pool=stem_pool) == 9 and bn_backward.install(net) == 20
    assert net.__dict__["_mhaq_stem_pool"] is stem_pool
    assert [n for n, _ in net.named_modules()] == [n for n, _ in names] and list(net.state_dict().keys()) == keys
    assert "_mhaq_stem_pool" not in dict(net.named_buffers()) and "_mhaq_stem_pool" not in net._modules
    dup = copy.deepcopy(net)
    assert dup.__dict__["_mhaq_stem_pool"] is stem_pool and list(dup.state_dict().keys()) == keys
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert back.__dict__["_mhaq_stem_pool"] is stem_pool and list(back.state_dict().keys()) == keys
    bn_backward.uninstall(net)
    fused_blocks.uninstall(net)
    assert [(n, type(m).__name__) for n, m in net.named_modules()] == names
    assert "_mhaq_stem_pool" not in net.__dict__


def test_cpu_and_eval_calls_never_reach_the_pooled_node(monkeypatch):
    """takes_node() is what FusedResNet18 asks before forward_pooled: false on a CPU tensor, in eval mode, for a 16-bit
    input, without tracked statistics or affine parameters -- and forward() then runs nn.BatchNorm2d.forward."""
    from mhaq_amd import _ext

    def boom():
        raise AssertionError("the compiled node must not be reached")
    monkeypatch.setattr(_ext, "ext", boom)
    x = torch.randn(2, 8, 6, 6)
    for make in (lambda: nn.BatchNorm2d(8), lambda: nn.BatchNorm2d(8).eval(), lambda: nn.BatchNorm2d(8, affine=False),
                 lambda: nn.BatchNorm2d(8, track_running_stats=False)):
        torch.manual_seed(0)
        stock = make()
        mine = copy.deepcopy(stock)
        assert bn_backward.install(mine) == 1
        assert not mine.takes_node(x) and not mine.takes_node(x.bfloat16())
        assert torch.equal(stock(x), mine(x))
        assert all(torch.equal(a, b) for a, b in zip(stock.state_dict().values(), mine.state_dict().values()))


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_compiled_node_on_cpu_is_batch_norm_then_max_pool2d(layout):
    from mhaq_amd import _ext
    E = _ext.ext()
    torch.manual_seed(2)
    x = torch.randint(-3, 4, (3, 8, 7, 6)).float()                 # ties in every window
    g = torch.randn(3, 8, 4, 3)
    if layout == "channels_last":
        x, g = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
    outs = []
    n0 = E.bn_pool_hip_backwards()
    for fn in (lambda *a: F.max_pool2d(F.batch_norm(a[0], a[3], a[4], a[1], a[2], True, 0.1, 1e-5), 3, 2, 1),
               lambda *a: E.bn_pool_train(a[0], a[1], a[2], a[3], a[4], 0.1, 1e-5, True)):
        xi = x.clone().requires_grad_(True)
        w, b = torch.linspace(-1, 1, 8).requires_grad_(True), torch.linspace(0, 1, 8).requires_grad_(True)
        rm, rv = torch.zeros(8), torch.ones(8)
        p = fn(xi, w, b, rm, rv)
        p.backward(g)
        outs.append((p.detach(), xi.grad, w.grad, b.grad, rm, rv))
    assert E.bn_pool_hip_backwards() == n0                         # the fallback, and the counter shows it
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(Exception):
        E.bn_pool_train(x, None, None, torch.zeros(8), torch.ones(8), 0.1, 1e-5, True)
