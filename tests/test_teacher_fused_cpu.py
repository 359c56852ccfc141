"""CPU: the frozen teacher's fused forward (mhaq_fq_bn_infer_consts / _act / mhaq_fq_bn_relu_pool3s2 in csrc/bn_bwd.hip,
mhaq_amd/frozen_blocks.py, QATConfig.fuse_teacher) as far as it goes without a device: the library exports the entry points
and returns its argument errors before any launch, in the documented order; the switch parses; install / uninstall keep names,
state_dict and deepcopy; the refresh key follows the BatchNorm; the contract evaluated in fp32 torch stays inside its bound on
the planted cases; a CPU model runs the stock modules bit for bit."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from mhaq_amd import _lib, frozen_blocks, nets
from tests import teacher_fused_contract as K

NAMES = ("mhaq_fq_bn_infer_consts", "mhaq_fq_bn_infer_act", "mhaq_fq_bn_relu_pool3s2")
FAKE, ODD, ODD4 = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004), ctypes.c_void_p(0x1002)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbols_are_exported_declared_and_of_the_headers_arity(L):
    with open(_lib.HEADER_PATH) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["mhaq_fq_bn_infer_consts"][1][4] is ctypes.c_double
    assert re.search(r"MHAQ_FQ_BN_RELU = 0, MHAQ_FQ_BN_ADD_RELU = 1, MHAQ_FQ_BN2_ADD_RELU = 2", src)
    assert L.mhaq_fq_abi_version() == 4


def _consts(L, **kw):
    a = dict(rm=FAKE, rv=FAKE, weight=FAKE, bias=FAKE, eps=1e-5, c=8, consts=FAKE, stream=None)
    a.update(kw)
    return L.mhaq_fq_bn_infer_consts(*a.values())


def _act(L, mode=K.BN_RELU, **kw):
    a = dict(x=FAKE, consts=FAKE, x2=None, consts2=None, residual=None, y=FAKE, m=64, c=8, mode=mode, stream=None)
    if mode == K.BN_ADD_RELU:
        a["residual"] = FAKE
    if mode == K.BN2_ADD_RELU:
        a["x2"] = a["consts2"] = FAKE
    a.update(kw)
    return L.mhaq_fq_bn_infer_act(*a.values())


def _pool(L, **kw):
    a = dict(x=FAKE, consts=FAKE, p=FAKE, n=2, h=5, w=7, c=8, stream=None)
    a.update(kw)
    return L.mhaq_fq_bn_relu_pool3s2(*a.values())


def test_argument_errors_are_returned_before_any_launch(L):
    for k in ("rm", "rv", "consts"):
        assert _consts(L, **{k: None}) == -1, k
    assert _consts(L, c=0) == -1 and _consts(L, c=-4) == -1
    assert _consts(L, c=6) == -4 and _consts(L, c=1 << 23) == -4
    assert _consts(L, consts=ODD) == -3
    for k in ("rm", "rv", "weight", "bias"):
        assert _consts(L, **{k: ODD4}) == -3, k
    for mode in (K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU):
        for k in ("x", "consts", "y"):
            assert _act(L, mode, **{k: None}) == -1, (mode, k)
        assert _act(L, mode, m=0) == -1 and _act(L, mode, c=0) == -1 and _act(L, mode, m=-1) == -1
        assert _act(L, mode, c=6) == -4 and _act(L, mode, c=1 << 23) == -4 and _act(L, mode, m=1 << 60) == -4
        for k in ("x", "consts", "y"):
            assert _act(L, mode, **{k: ODD}) == -3, (mode, k)
    assert _act(L, 3) == -1 and _act(L, -1) == -1                                        # an unknown mode
    # a mode's own operands are required, the other modes' refused
    assert _act(L, K.BN_RELU, residual=FAKE) == -1 and _act(L, K.BN_RELU, x2=FAKE, consts2=FAKE) == -1
    assert _act(L, K.BN_ADD_RELU, residual=None) == -1 and _act(L, K.BN_ADD_RELU, x2=FAKE, consts2=FAKE) == -1
    assert _act(L, K.BN2_ADD_RELU, x2=None) == -1 and _act(L, K.BN2_ADD_RELU, consts2=None) == -1
    assert _act(L, K.BN2_ADD_RELU, residual=FAKE) == -1
    assert _act(L, K.BN_ADD_RELU, residual=ODD) == -3
    assert _act(L, K.BN2_ADD_RELU, x2=ODD) == -3 and _act(L, K.BN2_ADD_RELU, consts2=ODD) == -3
    for k in ("x", "consts", "p"):
        assert _pool(L, **{k: None}) == -1, k
        assert _pool(L, **{k: ODD}) == -3, k
    for k in ("n", "h", "w", "c"):
        assert _pool(L, **{k: 0}) == -1, k
    assert _pool(L, c=6) == -4 and _pool(L, c=1 << 23) == -4 and _pool(L, n=1 << 20, h=1 << 6, w=1 << 5) == -4


def test_argument_errors_come_in_the_forwards_order(L):
    """Several things wrong at once: NULL / size / mode first, then width and range, then the alignment."""
    assert _consts(L, rm=None, c=6, consts=ODD) == -1 and _consts(L, c=0, consts=ODD, rv=ODD4) == -1
    assert _consts(L, c=6, consts=ODD, weight=ODD4) == -4
    assert _consts(L, c=8, consts=ODD, weight=ODD4) == -3
    for mode in (K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU):
        worst = dict(y=ODD, c=6)
        assert _act(L, mode, **dict(worst, x=None)) == -1 and _act(L, mode, **dict(worst, m=0)) == -1
        assert _act(L, mode, **worst) == -4 and _act(L, mode, **dict(worst, c=8, m=1 << 60)) == -4
        assert _act(L, mode, **dict(worst, c=8)) == -3
    assert _act(L, 7, y=ODD, c=6) == -1
    assert _act(L, K.BN_RELU, residual=ODD, c=6) == -1                                   # a refused operand, misaligned too
    assert _act(L, K.BN2_ADD_RELU, x2=ODD, c=6) == -4
    assert _pool(L, x=None, c=6, p=ODD) == -1 and _pool(L, h=0, c=6, p=ODD) == -1
    assert _pool(L, c=6, p=ODD) == -4 and _pool(L, n=1 << 31, p=ODD) == -4
    assert _pool(L, p=ODD) == -3


def test_default_and_switch_parsing(monkeypatch):
    from mhaq_amd.qat import QATConfig
    assert QATConfig().fuse_teacher is True
    assert frozen_blocks.ENV_SWITCH == "MHAQ_TEACHER_FUSED"
    monkeypatch.delenv(frozen_blocks.ENV_SWITCH, raising=False)
    assert frozen_blocks.enabled_by_env() is True
    for v in ("0", "false", "OFF", " no "):
        monkeypatch.setenv(frozen_blocks.ENV_SWITCH, v)
        assert frozen_blocks.enabled_by_env() is False
    for v in ("1", "true", "on", ""):
        monkeypatch.setenv(frozen_blocks.ENV_SWITCH, v)
        assert frozen_blocks.enabled_by_env() is True


def _net():
    torch.manual_seed(0)
    net = nets.ResNet18(10).eval()
    g = torch.Generator().manual_seed(1)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.5)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return net


def test_install_and_uninstall_keep_names_state_dict_and_deepcopy():
    net = _net()
    names, keys = [n for n, _ in net.named_modules()], list(net.state_dict().keys())
    assert frozen_blocks.install(net) == 9                                               # eight blocks and the net
    assert type(net) is frozen_blocks.FrozenResNet18 and type(net.layer3[1]) is frozen_blocks.FrozenBasicBlock
    assert [n for n, _ in net.named_modules()] == names and list(net.state_dict().keys()) == keys
    assert not any(frozen_blocks._HOLD in k for k, _ in net.named_buffers())
    assert all(frozen_blocks._HOLD not in m.__dict__ for m in net.modules())             # a CPU model gets no slabs
    dup = copy.deepcopy(net)
    assert type(dup) is frozen_blocks.FrozenResNet18 and list(dup.state_dict().keys()) == keys
    assert all(torch.equal(a, b) for a, b in zip(dup.state_dict().values(), net.state_dict().values()))
    frozen_blocks.uninstall(net)
    assert type(net) is nets.ResNet18 and all(type(b) is nets.BasicBlock for lay in (net.layer1, net.layer4) for b in lay)
    assert frozen_blocks.install(nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8))) == 0


def test_the_refresh_key_follows_the_batchnorm():
    bn = nn.BatchNorm2d(8).eval()
    key = frozen_blocks._key(bn)
    assert frozen_blocks._key(bn) == key                                                 # nothing changed: computed once
    with torch.no_grad():
        bn.running_var.mul_(2.0)                                                         # an in-place update: _version
    k2 = frozen_blocks._key(bn)
    assert k2 != key and k2[:3] == key[:3]
    other = nn.BatchNorm2d(8)
    other.running_mean.normal_()
    bn.load_state_dict(other.state_dict())                                               # copy_ into every tensor
    k3 = frozen_blocks._key(bn)
    assert all(a != b for a, b in zip(k3[:4], k2[:4])) and k3[4] == k2[4]
    bn.weight = nn.Parameter(torch.ones(8))                                              # a reassigned tensor: data_ptr
    k4 = frozen_blocks._key(bn)
    assert k4[0] != k3[0] and k4[1:] == k3[1:]
    bn.eps = 1e-3
    k5 = frozen_blocks._key(bn)
    assert k5[4] == 1e-3 and k5[:4] == k4[:4]
    plain = nn.BatchNorm2d(8, affine=False)
    assert frozen_blocks._key(plain)[:2] == (None, None)


KINDS = ["plain", "far_mean", "zero_var_eps1e-5", "zero_var_eps1e-3", "gamma_zero", "gamma_negative"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 4), (7, 12), (513, 64), (98, 512)], ids=lambda s: "x".join(map(str, s)))
def test_contract_in_fp32_stays_inside_its_bound(shape, kind):
    m, c = shape
    x, rm, rv, gamma, beta, eps = K.planted(kind, m, c)
    x2, rm2, rv2, gamma2, beta2, eps2 = K.planted(kind, m, c, seed=5)
    r = torch.randn(m, c, generator=torch.Generator().manual_seed(9)) * 3
    k, k2 = K.slab(rm, rv, gamma, beta, eps), K.slab(rm2, rv2, gamma2, beta2, eps2)
    c64, c64_2 = K.consts64(rm, rv, gamma, beta, eps), K.consts64(rm2, rv2, gamma2, beta2, eps2)
    assert K.check_slab(k, rm, rv, gamma, beta, eps) == 0
    for mode in (K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU):
        y = K.chain(x, k, mode, r=r, x2=x2, k2=k2)
        worst = K.check(y, *K.ref64(x, c64, mode, r=r, x2=x2, c64_2=c64_2))
        print(shape, kind, mode, f"{worst:.2e} T")
    if m >= 4:
        n = 2 if m % 2 == 0 else 1
        h = 7 if (m // n) % 7 == 0 else 1
        x4 = x.reshape(n, h, m // n // h, c).permute(0, 3, 1, 2)
        print(shape, kind, "pool", f"{K.check(K.chain_pool(x4, k), *K.ref64_pool(x4, c64)):.2e} T")


def test_checker_rejects_shifted_constants_and_a_wrong_kind():
    """The checker is not vacuous: constants of the neighbouring channel, or a ReLU that drops a NaN, fail it."""
    x, rm, rv, gamma, beta, eps = K.planted("plain", 513, 64)
    k, c64 = K.slab(rm, rv, gamma, beta, eps), K.consts64(rm, rv, gamma, beta, eps)
    y64, T = K.ref64(x, c64)
    K.check(K.chain(x, k), y64, T)
    with pytest.raises(AssertionError):
        K.check(K.chain(x, k.roll(1, dims=1)), y64, T)
    x[3, 5] = float("nan")
    y64, T = K.ref64(x, c64)
    y = K.chain(x, k)
    K.check(y, y64, T)
    y[3, 5] = 0.0                                                                        # a ReLU that drops the NaN
    with pytest.raises(AssertionError):
        K.check(y, y64, T)


def test_a_cpu_model_runs_the_stock_forward_bit_for_bit():
    net = _net()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = net(x)
        assert frozen_blocks.install(net) == 9
        got = net(x)
    assert torch.equal(got, want)
    train = copy.deepcopy(net).train()
    stock = copy.deepcopy(train)
    frozen_blocks.uninstall(stock)
    assert torch.equal(train(x), stock(x))
