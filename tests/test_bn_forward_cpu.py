"""CPU: the opt-in HIP BatchNorm forward (mhaq_fq_bn_fwd in csrc/bn_bwd.hip, `hip_forward` of the compiled nodes,
mhaq_amd/bn_backward.py, QATConfig.hip_bn_forward) as far as it goes without a device: the library exports the entry points and
returns its argument errors before any launch, in the documented order; the checker of tests/bn_fwd_contract.py accepts an
fp32 torch evaluation of the contract and rejects the variants the contract rules out; the switches parse; install / deepcopy /
uninstall keep or drop the per-module flag and never touch the state_dict."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from mhaq_amd import _lib, bn_backward
from tests import bn_fwd_contract as K

SHAPES = [(2, 4), (18, 64), (75, 20), (245, 512), (25088, 64), (1048355, 4)]
KINDS = ["plain", "far_mean", "constant_channel", "outlier", "tiny_sigma", "gamma_sign"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbols_are_exported_declared_and_of_the_headers_arity(L):
    with open(_lib.HEADER_PATH) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("mhaq_fq_bn_fwd_workspace_bytes", "mhaq_fq_bn_fwd"):
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["mhaq_fq_bn_fwd"][1][8:10] == [ctypes.c_double, ctypes.c_double]
    assert L.mhaq_fq_abi_version() == 4


def test_workspace_query(L):
    q = L.mhaq_fq_bn_fwd_workspace_bytes
    for m, c in [(250 * 112 * 112, 64), (250 * 56 * 56, 64), (250 * 28 * 28, 128), (250 * 14 * 14, 256),
                 (250 * 7 * 7, 512), (1 << 20, 4), (1 << 22, 20), (10 ** 9, 8)]:
        nb = q(m, c)
        assert nb % (4 * c) == 0 and nb >= (4 * 4 + 2 * 8) * c
        assert nb - 4 * 4 * c < 0.01 * (4 * m * c), (m, c)            # the partial rows stay below 1 % of x
        # the partition is the backward's: the same number of fp64 partial rows
        assert nb - 4 * 4 * c == L.mhaq_fq_bn_bwd_workspace_bytes(m, c) - 5 * 4 * c
    assert q(2, 4) == (4 * 4 + 2 * 8) * 4                              # one row chunk: 3 constant rows, the shift, 2 partial rows
    assert q(1, 4) == 0 and q(16, 6) == 0 and q(0, 8) == 0 and q(4, 1 << 23) == 0


def _args(**kw):
    fake = ctypes.c_void_p(0x1000)
    a = dict(x=fake, weight=fake, bias=fake, y=fake, save_mean=fake, save_invstd=fake, running_mean=fake, running_var=fake,
             factor=0.1, eps=1e-5, m=64, c=8, ws=fake, nbytes=None, stream=None)
    a.update(kw)
    return a


def _call(L, **kw):
    a = _args(**kw)
    if a["nbytes"] is None:
        a["nbytes"] = L.mhaq_fq_bn_fwd_workspace_bytes(64, 8)
    return L.mhaq_fq_bn_fwd(*a.values())


def test_argument_errors_are_returned_before_any_launch(L):
    odd = ctypes.c_void_p(0x1004)
    nb = L.mhaq_fq_bn_fwd_workspace_bytes(64, 8)
    for k in ("x", "save_mean", "save_invstd", "ws"):
        assert _call(L, **{k: None}) == -1, k
    assert _call(L, m=0) == -1 and _call(L, c=0) == -1 and _call(L, m=-3) == -1
    assert _call(L, running_mean=None) == -1 and _call(L, running_var=None) == -1          # both or neither
    assert _call(L, m=1) == -4                                                             # no unbiased variance
    assert _call(L, c=6, nbytes=1 << 20) == -4 and _call(L, m=4, c=1 << 23, nbytes=1 << 40) == -4
    assert _call(L, nbytes=nb - 1) == -2 and _call(L, nbytes=0) == -2
    for k in ("x", "y", "ws"):                                                             # 16-byte aligned
        assert _call(L, **{k: odd}) == -3, k
    for k in ("weight", "bias", "save_mean", "save_invstd", "running_mean", "running_var"):
        assert _call(L, **{k: ctypes.c_void_p(0x1002)}) == -3, k


def test_argument_errors_come_in_the_backwards_order(L):
    """Several things wrong at once: NULL / size first, then width and range, then the workspace, then the alignment."""
    odd = ctypes.c_void_p(0x1004)
    nb = L.mhaq_fq_bn_fwd_workspace_bytes(64, 8)
    worst = dict(y=odd, c=6, nbytes=0)
    assert _call(L, **dict(worst, x=None)) == -1 and _call(L, **dict(worst, m=0)) == -1
    assert _call(L, **dict(worst, ws=None)) == -1 and _call(L, **dict(worst, running_var=None)) == -1
    assert _call(L, **worst) == -4
    assert _call(L, **dict(worst, c=8, m=1)) == -4 and _call(L, **dict(worst, c=8, m=1 << 60)) == -4
    assert _call(L, **dict(worst, c=8)) == -2 and _call(L, **dict(worst, c=8, nbytes=nb - 1)) == -2
    assert _call(L, **dict(worst, c=8, nbytes=nb)) == -3


def _case(kind, m, c, seed=0):
    x, gamma, beta = K.planted(kind, m, c, seed)
    g = torch.Generator().manual_seed(seed + 100)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return x, gamma, beta, rm, rv


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_accepts_the_contract_in_fp32(shape, kind):
    m, c = shape
    x, gamma, beta, rm, rv = _case(kind, m, c)
    for eps, f in ((1e-5, 0.1), (1e-3, 1.0)):
        cf = K.closed_form(x, gamma, beta, eps, rm, rv, f)
        fig = K.check_all(K.simulate(x, gamma, beta, eps, rm, rv, f), cf)
        print(shape, kind, eps, f, {k: f"{v:.2e}" for k, v in fig.items()})
    if kind == "constant_channel":
        sim = K.simulate(x, gamma, beta, 1e-5)
        for ch, val in ((1, 3.0), (c - 1, 0.0)):
            assert float(sim["mean"][ch]) == val and float(sim["invstd"][ch]) == float(torch.tensor(1e-5 ** -0.5))
            assert bool((sim["y"][:, ch] == beta[ch]).all())


def test_checker_follows_factor_zero_the_cumulative_factor_and_missing_affine():
    x, gamma, beta, rm, rv = _case("plain", 75, 20)
    for f in (0.0, 1.0 / 3):
        K.check_all(K.simulate(x, gamma, beta, 1e-5, rm, rv, f), K.closed_form(x, gamma, beta, 1e-5, rm, rv, f))
    K.check_all(K.simulate(x, None, None, 1e-5), K.closed_form(x, None, None, 1e-5))


def test_checker_matches_non_finite_channels_in_kind():
    x, gamma, beta, rm, rv = _case("plain", 75, 20)
    x[3, 5], x[7, 9], x[0, 11] = float("nan"), float("inf"), float("-inf")
    cf = K.closed_form(x, gamma, beta, 1e-5, rm, rv)
    assert cf["bad"].nonzero().flatten().tolist() == [5, 9, 11]
    sim = K.simulate(x, gamma, beta, 1e-5, rm, rv)
    K.check_all(sim, cf)
    clean = dict(sim, y=sim["y"].clone())
    clean["y"][:, 9] = 0.0                                           # finite where the channel holds an infinity
    with pytest.raises(AssertionError):
        K.check_all(clean, cf)


@pytest.mark.parametrize("variant,kind", [("unshifted_fp32", "far_mean"), ("no_beta", "plain"), ("truncated_mean", "plain"),
                                          ("biased_running_var", "plain")])
def test_checker_rejects_what_the_contract_rules_out(variant, kind):
    x, gamma, beta, rm, rv = _case(kind, 245, 512)
    cf = K.closed_form(x, gamma, beta, 1e-5, rm, rv)
    K.check_all(K.simulate(x, gamma, beta, 1e-5, rm, rv), cf)
    bad = K.simulate(x, gamma, beta, 1e-5, rm, rv, variant=variant)
    if variant == "unshifted_fp32":
        print("unshifted fp32 statistics on far_mean: y off by", float(((bad["y"].double() - cf["y"]).abs() / cf["T"]).max()), "T")
    with pytest.raises(AssertionError):
        K.check_all(bad, cf)


def test_switches_parse(monkeypatch):
    from mhaq_amd.qat import QATConfig
    assert QATConfig().hip_bn_forward is False
    monkeypatch.delenv(bn_backward.ENV_SWITCH_FORWARD, raising=False)
    assert bn_backward.ENV_SWITCH_FORWARD == "MHAQ_BN_FORWARD"
    assert bn_backward.hip_forward_enabled() is False and bn_backward.hip_forward_enabled(True) is True
    for v in ("1", "true", "ON", " yes "):
        monkeypatch.setenv(bn_backward.ENV_SWITCH_FORWARD, v)
        assert bn_backward.hip_forward_enabled() is True and bn_backward.hip_forward_enabled(False) is True
    for v in ("0", "false", "off", "no", "2"):
        monkeypatch.setenv(bn_backward.ENV_SWITCH_FORWARD, v)
        assert bn_backward.hip_forward_enabled() is False and bn_backward.hip_forward_enabled(True) is False
    monkeypatch.setenv(bn_backward.ENV_SWITCH_FORWARD, "")
    assert bn_backward.hip_forward_enabled(True) is True


def test_install_deepcopy_and_uninstall_keep_or_drop_the_flag():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.SyncBatchNorm(8))
    keys = list(net.state_dict().keys())
    assert bn_backward.install(net, hip_forward=True) == 1
    assert net[1].takes_hip_forward() and not net[1].takes_x16()
    assert list(net.state_dict().keys()) == keys and not any("hip" in k for k, _ in net.named_buffers())
    assert len(list(net[1].parameters())) == 2
    dup = copy.deepcopy(net)
    assert type(dup[1]) is bn_backward.HipBackwardBatchNorm2d and dup[1].takes_hip_forward()
    assert list(dup.state_dict().keys()) == keys
    bn_backward.uninstall(net)
    assert type(net[1]) is nn.BatchNorm2d and bn_backward._HIP_FWD not in net[1].__dict__
    assert bn_backward.install(net) == 1 and not net[1].takes_hip_forward()       # off unless asked for
    bn_backward.uninstall(net)
    assert bn_backward.install(net, x16=True, hip_forward=True) == 1 and net[1].takes_x16() and net[1].takes_hip_forward()


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_flagged_module_and_node_equal_the_stock_forward_on_cpu_tensors(layout):
    """A CPU tensor never takes the HIP forward: module and node with the flag set are F.batch_norm, bit for bit."""
    from mhaq_amd import _ext
    torch.manual_seed(1)
    x, g = torch.randn(3, 8, 5, 4) * 2 + 1, torch.randn(3, 8, 5, 4)
    if layout == "channels_last":
        x, g = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
    stock = nn.BatchNorm2d(8)
    mine = copy.deepcopy(stock)
    assert bn_backward.install(mine, hip_forward=True) == 1
    E = _ext.ext()
    n0 = E.bn_hip_forwards()
    outs = []
    for bn in (stock, mine):
        xi = x.clone().requires_grad_(True)
        y = bn(xi)
        y.backward(g)
        outs.append([y.detach(), xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    rm, rv = torch.zeros(8), torch.ones(8)
    y = E.bn_train(x, stock.weight, stock.bias, rm, rv, 0.1, 1e-5, True, False, True)
    p = E.bn_pool_train(x, stock.weight, stock.bias, torch.zeros(8), torch.ones(8), 0.1, 1e-5, True, hip_forward=True)
    ref = torch.nn.functional.batch_norm(x, torch.zeros(8), torch.ones(8), stock.weight, stock.bias, True, 0.1, 1e-5)
    assert torch.equal(y, ref) and torch.equal(p, torch.nn.functional.max_pool2d(ref, 3, 2, 1))
    assert E.bn_hip_forwards() == n0
