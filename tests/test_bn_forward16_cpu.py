"""CPU: the opt-in 16-bit HIP BatchNorm forward (mhaq_fq_bn_fwd_x16 in csrc/bn_bwd.hip, `hip_forward_x16` of bn_train,
mhaq_amd/bn_backward.py, QATConfig.hip_bn_forward_16bit) as far as it goes without a device: the library exports the entry points
and returns its argument errors before any launch, in the documented order, the dtype included; the checkers of
tests/bn_fwd16_contract.py accept a torch evaluation of the contract in both dtypes and reject what the contract rules out; the
switches parse; install / deepcopy / uninstall keep or drop the per-module flag and never touch the state_dict."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from mhaq_amd import _lib, bn_backward
from tests import bn_fwd16_contract as K
from tests import bn_fwd_contract as K32

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
_dt = lambda d: "bf16" if d is BF16 else "fp16"
SHAPES = [(75, 24), (1029, 136), (4099, 8)]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbols_are_exported_declared_and_of_the_headers_arity(L):
    with open(_lib.HEADER_PATH) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in ("mhaq_fq_bn_fwd_x16_workspace_bytes", "mhaq_fq_bn_fwd_x16"):
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
    sig = _lib.SIGNATURES["mhaq_fq_bn_fwd_x16"][1]
    assert sig[8:10] == [ctypes.c_double, ctypes.c_double] and sig[12] is ctypes.c_int
    # mhaq_fq_bn_fwd's arguments with `dtype` after c
    assert sig[:12] + sig[13:] == _lib.SIGNATURES["mhaq_fq_bn_fwd"][1]
    assert L.mhaq_fq_abi_version() == 4


def test_workspace_query(L):
    q = L.mhaq_fq_bn_fwd_x16_workspace_bytes
    for m, c in [(250 * 112 * 112, 64), (250 * 56 * 56, 64), (250 * 28 * 28, 128), (250 * 14 * 14, 256),
                 (250 * 7 * 7, 512), (1 << 20, 8), (1 << 22, 24), (10 ** 9, 8)]:
        nb = q(m, c)
        assert nb % (4 * c) == 0 and nb >= (4 * 4 + 2 * 8) * c
        assert nb - 4 * 4 * c < 0.01 * (2 * m * c), (m, c)            # the partial rows stay below 1 % of the 16-bit x
        # the partition is the 16-bit backward's: the same number of fp64 partial rows
        assert nb - 4 * 4 * c == L.mhaq_fq_bn_bwd_x16_workspace_bytes(m, c) - 5 * 4 * c
    assert q(2, 8) == (4 * 4 + 2 * 8) * 8                              # one row chunk: 3 constant rows, the shift, 2 partial rows
    assert q(1, 8) == 0                                                # M = 1
    assert q(16, 4) == 0 and q(16, 12) == 0                            # C % 8 != 0
    assert q(4, 1 << 23) == 0 and q(4, (1 << 22) + 8) == 0             # C over the limit
    assert q(0, 8) == 0 and q(4, 1 << 22) > 0


def _args(**kw):
    fake = ctypes.c_void_p(0x1000)
    a = dict(x=fake, weight=fake, bias=fake, y=fake, save_mean=fake, save_invstd=fake, running_mean=fake, running_var=fake,
             factor=0.1, eps=1e-5, m=64, c=8, dtype=_lib.DT_BF16, ws=fake, nbytes=None, stream=None)
    a.update(kw)
    return a


def _call(L, **kw):
    a = _args(**kw)
    if a["nbytes"] is None:
        a["nbytes"] = L.mhaq_fq_bn_fwd_x16_workspace_bytes(64, 8)
    return L.mhaq_fq_bn_fwd_x16(*a.values())


def test_argument_errors_are_returned_before_any_launch(L):
    odd = ctypes.c_void_p(0x1004)
    nb = L.mhaq_fq_bn_fwd_x16_workspace_bytes(64, 8)
    for k in ("x", "save_mean", "save_invstd", "ws"):
        assert _call(L, **{k: None}) == -1, k
    assert _call(L, m=0) == -1 and _call(L, c=0) == -1 and _call(L, m=-3) == -1
    assert _call(L, running_mean=None) == -1 and _call(L, running_var=None) == -1          # both or neither
    assert {_lib.DT_BF16, _lib.DT_F16} == {1, 2}
    for dt in (0, 3, -1, 16):                                                              # fp32 has its own entry point
        assert _call(L, dtype=dt) == -1, dt
    assert _call(L, m=1) == -4                                                             # no unbiased variance
    assert _call(L, c=4, nbytes=1 << 20) == -4 and _call(L, c=12, nbytes=1 << 20) == -4    # C % 8
    assert _call(L, m=4, c=1 << 23, nbytes=1 << 40) == -4
    assert _call(L, nbytes=nb - 1) == -2 and _call(L, nbytes=0) == -2
    for k in ("x", "y", "ws"):                                                             # 16-byte aligned
        assert _call(L, **{k: odd}) == -3, k
        assert _call(L, **{k: ctypes.c_void_p(0x1008)}) == -3, k
    for k in ("weight", "bias", "save_mean", "save_invstd", "running_mean", "running_var"):
        assert _call(L, **{k: ctypes.c_void_p(0x1002)}) == -3, k


def test_argument_errors_come_in_the_documented_order(L):
    """Several things wrong at once: NULL / size first, then the dtype, then width and range, then the workspace, then the
    alignment."""
    odd = ctypes.c_void_p(0x1004)
    nb = L.mhaq_fq_bn_fwd_x16_workspace_bytes(64, 8)
    worst = dict(y=odd, c=12, nbytes=0)
    assert _call(L, **dict(worst, x=None)) == -1 and _call(L, **dict(worst, m=0)) == -1
    assert _call(L, **dict(worst, ws=None)) == -1 and _call(L, **dict(worst, running_var=None)) == -1
    assert _call(L, **dict(worst, dtype=0)) == -1 and _call(L, **dict(worst, c=8, m=1, dtype=7)) == -1      # before the width
    assert _call(L, **worst) == -4
    assert _call(L, **dict(worst, c=8, m=1)) == -4 and _call(L, **dict(worst, c=8, m=1 << 60)) == -4
    assert _call(L, **dict(worst, c=8)) == -2 and _call(L, **dict(worst, c=8, nbytes=nb - 1)) == -2
    assert _call(L, **dict(worst, c=8, nbytes=nb)) == -3
    assert _call(L, **dict(worst, c=8, nbytes=nb, dtype=_lib.DT_F16)) == -3


def _case(kind, m, c, dtype, seed=0):
    x, gamma, beta = K.planted(kind, m, c, dtype, seed)
    g = torch.Generator().manual_seed(seed + 100)
    rm, rv = torch.randn(c, generator=g), torch.rand(c, generator=g) + 0.5
    return x, gamma, beta, rm, rv


# every planted case on the three shapes, and the ordinary inputs (the cap's condition) on a fourth
ACCEPT = ([(s, k) for s in SHAPES for k in K.CAPPED_KINDS + ("constant_channel", "tiny_sigma", "far_mean", "spread")]
          + [((3000, 264), k) for k in K.CAPPED_KINDS])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape,kind", ACCEPT, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_checkers_accept_the_contract(shape, kind, dtype):
    m, c = shape
    x, gamma, beta, rm, rv = _case(kind, m, c, dtype)
    for eps, f in ((1e-5, 0.1), (1e-3, 1.0)):
        cf = K.closed_form(x, gamma, beta, eps, rm, rv, f)
        fig = K.check_all(K.simulate(x, gamma, beta, eps, rm, rv, f), cf, dtype, cap=K.capped(kind, m))
        print(shape, kind, _dt(dtype), eps, f, {k: f"{v:.2e}" for k, v in fig.items()})
    sim = K.simulate(x, gamma, beta, 1e-5)
    if kind == "constant_channel":
        for ch, val in ((1, 3.0), (c - 1, 0.0)):
            assert float(sim["mean"][ch]) == val and float(sim["invstd"][ch]) == float(torch.tensor(1e-5 ** -0.5))
            assert bool((sim["y"][:, ch] == beta[ch].to(dtype)).all())                     # R16(beta) bit for bit
    if kind == "tiny_sigma":                                        # 100 + 1e-3 randn rounds to 100: mean by value, var = 0
        assert bool((sim["mean"] == 100.0).all()) and bool((sim["invstd"] == float(torch.tensor(1e-5 ** -0.5))).all())


def test_checkers_accept_missing_affine_and_the_other_factors():
    x, gamma, beta, rm, rv = _case("plain", 75, 24, BF16)
    for f in (0.0, 1.0 / 3):
        K.check_all(K.simulate(x, gamma, beta, 1e-5, rm, rv, f), K.closed_form(x, gamma, beta, 1e-5, rm, rv, f), BF16)
    K.check_all(K.simulate(x, None, None, 1e-5), K.closed_form(x, None, None, 1e-5), BF16)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_checkers_match_non_finite_channels_in_kind(dtype):
    x, gamma, beta, rm, rv = _case("plain", 75, 24, dtype)
    x[3, 5], x[7, 9], x[0, 11] = float("nan"), float("inf"), float("-inf")
    cf = K.closed_form(x, gamma, beta, 1e-5, rm, rv)
    assert cf["bad"].nonzero().flatten().tolist() == [5, 9, 11]
    sim = K.simulate(x, gamma, beta, 1e-5, rm, rv)
    K.check_all(sim, cf, dtype)
    clean = dict(sim, y=sim["y"].clone())
    clean["y"][:, 9] = 0.0                                           # finite where the channel holds an infinity
    with pytest.raises(AssertionError):
        K.check_all(clean, cf, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("variant", ["truncated_y", "no_beta"])
def test_y_checker_rejects_what_the_contract_rules_out(variant, dtype):
    x, gamma, beta, rm, rv = _case("plain", 1029, 136, dtype)
    cf = K.closed_form(x, gamma, beta, 1e-5, rm, rv)
    good = K.simulate(x, gamma, beta, 1e-5, rm, rv)
    K.check_y16(good["y"], cf, dtype)
    with pytest.raises(AssertionError):
        K.check_y16(K.simulate(x, gamma, beta, 1e-5, rm, rv, variant=variant)["y"], cf, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_stat_checker_rejects_a_truncated_mean(dtype):
    x, gamma, beta, rm, rv = _case("plain", 1029, 136, dtype)
    cf = K.closed_form(x, gamma, beta, 1e-5, rm, rv)
    bad = K.simulate(x, gamma, beta, 1e-5, rm, rv, variant="truncated_mean")
    K32.check_stat(K.simulate(x, gamma, beta, 1e-5)["mean"], cf["mean"], cf["bad"], "save_mean", cf["xmax"])
    with pytest.raises(AssertionError):
        K32.check_stat(bad["mean"], cf["mean"], cf["bad"], "save_mean", cf["xmax"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_stat_checker_rejects_unshifted_fp32_statistics_on_the_spread_case(dtype):
    """A channel at ~1000 with sigma 64 keeps its spread in 16 bits; fp32 E[x^2] - E[x]^2 loses invstd there."""
    x, gamma, beta, rm, rv = _case("spread", 1029, 136, dtype)
    assert int((x.float().std(0) > 32).sum()) == 136
    cf = K.closed_form(x, gamma, beta, 1e-5, rm, rv)
    K.check_all(K.simulate(x, gamma, beta, 1e-5, rm, rv), cf, dtype, cap=False)
    bad = K.simulate(x, gamma, beta, 1e-5, rm, rv, variant="unshifted_fp32")
    with pytest.raises(AssertionError):
        K32.check_stat(bad["invstd"], cf["invstd"], cf["bad"], "save_invstd")


def test_switches_parse(monkeypatch):
    from mhaq_amd.qat import QATConfig
    assert QATConfig().hip_bn_forward_16bit is False
    assert QATConfig().hip_bn_forward is False and QATConfig().hip_bn_backward_16bit is False
    name = bn_backward.ENV_SWITCH_FORWARD_X16
    assert name == "MHAQ_BN_FORWARD_X16"
    monkeypatch.delenv(name, raising=False)
    assert bn_backward.hip_forward_x16_enabled() is False and bn_backward.hip_forward_x16_enabled(True) is True
    for v in ("1", "true", "ON", " yes "):
        monkeypatch.setenv(name, v)
        assert bn_backward.hip_forward_x16_enabled() is True and bn_backward.hip_forward_x16_enabled(False) is True
    for v in ("0", "false", "off", "no", "2"):
        monkeypatch.setenv(name, v)
        assert bn_backward.hip_forward_x16_enabled() is False and bn_backward.hip_forward_x16_enabled(True) is False
    monkeypatch.setenv(name, "")
    assert bn_backward.hip_forward_x16_enabled(True) is True
    # its own variable: the other switches do not move with it
    monkeypatch.setenv(name, "1")
    monkeypatch.delenv(bn_backward.ENV_SWITCH_FORWARD, raising=False)
    monkeypatch.delenv(bn_backward.ENV_SWITCH_X16, raising=False)
    assert bn_backward.hip_forward_enabled() is False and bn_backward.x16_enabled() is False


def test_install_deepcopy_and_uninstall_keep_or_drop_the_flag():
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.SyncBatchNorm(8))
    keys = list(net.state_dict().keys())
    assert bn_backward.install(net, x16=True, hip_forward_x16=True) == 1
    assert net[1].takes_hip_forward_x16() and net[1].takes_x16() and not net[1].takes_hip_forward()
    assert list(net.state_dict().keys()) == keys and not any("hip" in k for k, _ in net.named_buffers())
    assert len(list(net[1].parameters())) == 2 and len(list(net[1].buffers())) == 3
    dup = copy.deepcopy(net)
    assert type(dup[1]) is bn_backward.HipBackwardBatchNorm2d and dup[1].takes_hip_forward_x16() and dup[1].takes_x16()
    assert list(dup.state_dict().keys()) == keys
    bn_backward.uninstall(net)
    assert type(net[1]) is nn.BatchNorm2d and bn_backward._HIP_FWD_X16 not in net[1].__dict__
    assert bn_backward.install(net) == 1 and not net[1].takes_hip_forward_x16()          # off unless asked for
    bn_backward.uninstall(net)
    assert bn_backward.install(net, hip_forward=True) == 1 and not net[1].takes_hip_forward_x16()
    bn_backward.uninstall(net)
    assert bn_backward.install(net, hip_forward_x16=True) == 1                            # alone: set, and no error
    assert net[1].takes_hip_forward_x16() and not net[1].takes_x16()


@pytest.mark.parametrize("x16", [False, True])
def test_flagged_module_and_node_equal_the_stock_forward_on_cpu_tensors(x16):
    """A CPU tensor never takes the HIP forward: module and node with the flags set are F.batch_norm, bit for bit."""
    from mhaq_amd import _ext
    torch.manual_seed(1)
    x = (torch.randn(3, 8, 5, 4) * 2 + 1).bfloat16().contiguous(memory_format=torch.channels_last)
    g = torch.randn(3, 8, 5, 4).bfloat16().contiguous(memory_format=torch.channels_last)
    stock = nn.BatchNorm2d(8)
    mine = copy.deepcopy(stock)
    assert bn_backward.install(mine, x16=x16, hip_forward_x16=True) == 1
    E = _ext.ext()
    n0 = (E.bn_hip_forwards(), E.bn_hip_forwards_x16())
    outs = []
    for bn in (stock, mine):
        xi = x.clone().requires_grad_(True)
        y = bn(xi)
        y.backward(g)
        outs.append([y.detach(), xi.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var, bn.num_batches_tracked])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    y = E.bn_train(x, stock.weight, stock.bias, torch.zeros(8), torch.ones(8), 0.1, 1e-5, True, True, True, True)
    y2 = E.bn_train(x, stock.weight, stock.bias, torch.zeros(8), torch.ones(8), 0.1, 1e-5, True, x16=True, hip_forward_x16=True)
    ref = torch.nn.functional.batch_norm(x, torch.zeros(8), torch.ones(8), stock.weight, stock.bias, True, 0.1, 1e-5)
    assert torch.equal(y, ref) and torch.equal(y2, ref)
    # ... and the node's backward hands autograd one gradient per argument, the new flag's included
    xi, w, b = x.clone().requires_grad_(True), stock.weight.detach().clone().requires_grad_(True), stock.bias.detach().clone().requires_grad_(True)
    E.bn_train(xi, w, b, torch.zeros(8), torch.ones(8), 0.1, 1e-5, True, True, True, True).backward(g)
    assert torch.equal(xi.grad, outs[0][1]) and torch.equal(w.grad, outs[0][2]) and torch.equal(b.grad, outs[0][3])
    assert (E.bn_hip_forwards(), E.bn_hip_forwards_x16()) == n0
