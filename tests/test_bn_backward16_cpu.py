"""CPU: the 16-bit BatchNorm backward (mhaq_fq_bn_bwd_x16, csrc/bn_bwd.hip) as far as it goes without a device.  The
checker of tests/bn_bwd16_contract.py accepts an fp32 torch evaluation of the contract and rejects the variants the contract
rules out (so the GPU suite, which holds the kernels to the same checker, can tell them apart); the switches default to off;
the C ABI returns its argument errors before any launch; on CPU tensors the compiled node is F.batch_norm bit for bit
whatever the new flag says."""
import ctypes
import os
import subprocess

import pytest
import torch

from mhaq_amd import _lib, bn_backward
from tests import bn_bwd16_contract as K

EPS = 1e-5
DTYPES = [torch.bfloat16, torch.float16]
SHAPES = [(2, 8, 1, 1), (2, 64, 3, 3), (3, 24, 5, 5), (5, 512, 7, 7), (1, 8, 1, 9), (3, 136, 5, 5), (4, 64, 20, 20)]
_ids = lambda s: "x".join(map(str, s))


def _inputs(shape, dtype, seed=0):
    """The recipe of tests/test_gpu_bn_backward.py::_inputs on the CPU, cast to the dtype; the statistics of the 16-bit x
    (fp64 sums, rounded to fp32 once, as a forward would save them)."""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = torch.randn(shape, generator=g) * (0.5 + torch.rand(1, c, 1, 1, generator=g) * 3) + torch.randn(1, c, 1, 1, generator=g) * 2
    dy = torch.randn(shape, generator=g)
    gamma = torch.randn(c, generator=g)
    cl = lambda t: t.to(dtype).contiguous(memory_format=torch.channels_last)
    return cl(x), cl(dy), gamma


def _stats(x):
    X = K.rows(x).double()
    return X.mean(0).float(), (X.var(0, unbiased=False) + EPS).rsqrt().float()


def _far_mean(dtype):
    """far_mean of the fp32 suite (mean = +-1e4 in channels 4 and 9) in a form that survives 16 bits.  Around 1e4 adjacent
    bf16 values are 64 apart (fp16: 8), so 1e4 + randn rounds to ONE value: a constant channel, on which the folded and the
    unfolded form agree exactly.  Here the two channels spread over 64 * randn, and their dy follows x, so that dgamma / M --
    the factor of the term in which a folded mean cancels -- is of order one instead of M^-1/2."""
    shape = (4, 24, 20, 20)
    x, dy, gamma = _inputs(shape, dtype, seed=5)
    x, dy = x.float(), dy.float()
    for ch, mu, seed in ((4, 1e4, 6), (9, -1e4, 7)):
        z = torch.randn(4, 20, 20, generator=torch.Generator().manual_seed(seed))
        x[:, ch] = mu + 64 * z
        dy[:, ch] = z + 0.5 * dy[:, ch]
    return x.to(dtype), dy.to(dtype), gamma


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_checker_accepts_the_contract_and_stays_inside_the_caps(shape, dtype):
    x, dy, gamma = _inputs(shape, dtype)
    mean, invstd = _stats(x)
    cf = K.closed_form(x, dy, gamma, mean, invstd)
    dx, dw, db = K.simulate(x, dy, gamma, mean, invstd)
    m = x.numel() // x.shape[1]
    fig = K.check_dx16(dx, cf["dx"], cf["dx_abs"], dtype, cap=m >= 9)
    print(f"{shape} {dtype}: err {fig['err']:.3e} of the term sum beyond the rounding, excluded {fig['excluded']:.4f}")
    K.check_sums(dw, cf["dg"], cf["dg_abs"], "dgamma")
    K.check_sums(db, cf["db"], cf["db_abs"], "dbeta")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("variant", ["truncate", "no_dbias", "folded_mean"])
def test_checker_rejects_planted_errors(variant, dtype):
    if variant == "folded_mean":
        x, dy, gamma = _far_mean(dtype)
    else:
        x, dy, gamma = _inputs((4, 64, 20, 20), dtype, seed=3)
    mean, invstd = _stats(x)
    cf = K.closed_form(x, dy, gamma, mean, invstd)
    good, _, _ = K.simulate(x, dy, gamma, mean, invstd)
    K.check_dx16(good, cf["dx"], cf["dx_abs"], dtype)
    bad, _, _ = K.simulate(x, dy, gamma, mean, invstd, variant=variant)
    assert not torch.equal(good.view(torch.int16), bad.view(torch.int16))
    with pytest.raises(AssertionError):
        K.check_dx16(bad, cf["dx"], cf["dx_abs"], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_checker_special_values(dtype):
    """Zero term sums must be exact zeros, a NaN / infinity of the reference is matched in kind, and only fp16 may
    overflow, and only at the top of its range."""
    ref = torch.tensor([0.0, float("nan"), float("inf"), 1.0, 65519.0], dtype=torch.float64)
    ref_abs = torch.tensor([0.0, float("nan"), float("inf"), 1.0, 65519.0], dtype=torch.float64)
    top = float("inf") if dtype == torch.float16 else 65519.0
    good = torch.tensor([0.0, float("nan"), float("inf"), 1.0, top]).to(dtype)
    K.check_dx16(good, ref, ref_abs, dtype, cap=False)
    for k, v in ((0, 6e-8), (1, 0.0), (2, 60000.0), (3, float("inf")), (2, float("-inf"))):
        bad = good.clone()
        bad[k] = v
        with pytest.raises(AssertionError):
            K.check_dx16(bad, ref, ref_abs, dtype, cap=False)
    # spacing16: the larger neighbour gap, subnormals included
    mb = K.MANTISSA_BITS[dtype]
    v = torch.tensor([1.0, 1.5, 2.0, 0.0, -3.0]).to(dtype)
    want = [2.0 ** -mb, 2.0 ** -mb, 2.0 ** (1 - mb), 2.0 ** (K.MIN_EXPONENT[dtype] - mb), 2.0 ** (1 - mb)]
    assert K.spacing16(v).tolist() == want


def test_switches_default_to_off(monkeypatch):
    from mhaq_amd.qat import QATConfig
    assert QATConfig().hip_bn_backward_16bit is False
    monkeypatch.delenv(bn_backward.ENV_SWITCH_X16, raising=False)
    assert bn_backward.x16_enabled() is False and bn_backward.x16_enabled(True) is True
    for v in ("1", "true", "on", " ON "):
        monkeypatch.setenv(bn_backward.ENV_SWITCH_X16, v)
        assert bn_backward.x16_enabled() is True and bn_backward.x16_enabled(False) is True
    for v in ("0", "false", "off", "2"):
        monkeypatch.setenv(bn_backward.ENV_SWITCH_X16, v)
        assert bn_backward.x16_enabled() is False and bn_backward.x16_enabled(True) is False
    monkeypatch.setenv(bn_backward.ENV_SWITCH_X16, "")
    assert bn_backward.x16_enabled(True) is True


def test_install_flag_is_per_module_and_not_state():
    import copy
    from torch import nn
    net = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8))
    keys = list(net.state_dict().keys())
    assert bn_backward.install(net, x16=True) == 1
    assert net[1].takes_x16() and copy.deepcopy(net)[1].takes_x16() and list(net.state_dict().keys()) == keys
    x = torch.randn(2, 8, 4, 4).bfloat16()
    assert not net[1].takes_node(x) and not net[1].takes_pooled_node(x)          # a CPU tensor: the stock forward
    bn_backward.uninstall(net)
    assert type(net[1]) is nn.BatchNorm2d and "_mhaq_bn_x16" not in net[1].__dict__
    assert bn_backward.install(net) == 1 and not net[1].takes_x16()


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_workspace_query_keeps_the_partial_rows_below_one_percent(L):
    q16, q32 = L.mhaq_fq_bn_bwd_x16_workspace_bytes, L.mhaq_fq_bn_bwd_workspace_bytes
    for m, c in [(250 * 112 * 112, 64), (250 * 56 * 56, 64), (250 * 28 * 28, 128), (250 * 14 * 14, 256),
                 (250 * 7 * 7, 512), (1 << 20, 8), (1 << 22, 24), (10 ** 9, 8), (2753000, 24), (1345 * 2048, 24)]:
        nb = q16(m, c)
        assert nb % (4 * c) == 0 and nb >= (5 * 4 + 2 * 8) * c
        chunks = (nb - 5 * 4 * c) // (2 * 8 * c)
        # at least 896 rows per block: 16 C bytes of partial rows per 896 * 2 C bytes of ONE 16-bit tensor, 4 / 448 = 0.9 %
        # (a ragged last chunk aside, as in the fp32 geometry)
        assert chunks <= -(-m // 896) and nb - 5 * 4 * c < 0.01 * (2 * m * c), (m, c)
        assert nb <= q32(m, c), (m, c)                                   # never fewer rows per block than the fp32 kernels
    assert q16(2, 8) == (5 * 4 + 2 * 8) * 8                              # one row chunk
    assert q16(16, 12) == 0 and q16(0, 8) == 0 and q16(16, 1 << 23) == 0


def test_argument_errors_are_returned_before_any_launch(L):
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008)
    nb = L.mhaq_fq_bn_bwd_x16_workspace_bytes(64, 8)
    call = L.mhaq_fq_bn_bwd_x16
    base = [fake] * 8 + [64, 8, _lib.DT_BF16, fake, nb, None]

    def with_(**kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for k in (0, 1, 2, 3, 11):                     # x, dy, mean, invstd, workspace
        assert with_(**{f"a{k}": None}) == -1, k
    assert with_(a8=0) == -1 and with_(a9=0) == -1
    for dt in (0, 3, -1):
        assert with_(a10=dt) == -1, dt
    assert with_(a10=_lib.DT_F16, a12=nb - 1) == -2 and with_(a12=0) == -2
    for k in (0, 1, 5, 11):                        # x, dy, dx, workspace: 16-byte aligned
        assert with_(**{f"a{k}": odd}) == -3, k
    assert with_(a2=ctypes.c_void_p(0x1002)) == -3
    assert with_(a9=12, a12=1 << 20) == -4 and with_(a9=4, a12=1 << 20) == -4          # C % 8
    assert with_(a8=4, a9=1 << 23, a12=1 << 40) == -4
    # the order of mhaq_fq_bn_bwd: a bad dtype before an unsupported width, that before the workspace, that before alignment
    assert with_(a10=0, a9=12) == -1 and with_(a9=12, a12=0) == -4 and with_(a12=0, a0=odd) == -2
    # nothing to compute: no launch, no error
    assert with_(a4=None, a5=None, a6=None, a7=None) == 0


@pytest.mark.parametrize("x16", [False, True])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_compiled_node_equals_f_batch_norm_on_cpu_bf16_whatever_the_flag(layout, x16):
    import torch.nn.functional as F
    from mhaq_amd import _ext
    E = _ext.ext()
    torch.manual_seed(2)
    x, g = (torch.randn(4, 8, 3, 5) * 3 - 2).bfloat16(), torch.randn(4, 8, 3, 5).bfloat16()
    if layout == "channels_last":
        x, g = x.contiguous(memory_format=torch.channels_last), g.contiguous(memory_format=torch.channels_last)
    n0 = (E.bn_hip_backwards(), E.bn_hip_backwards_x16())
    outs = []
    for fn in (lambda *a: F.batch_norm(a[0], a[3], a[4], a[1], a[2], True, 0.1, 1e-5),
               lambda *a: E.bn_train(a[0], a[1], a[2], a[3], a[4], 0.1, 1e-5, True, x16)):
        xi = x.clone().requires_grad_(True)
        w, b = torch.linspace(-1, 1, 8).requires_grad_(True), torch.linspace(0, 1, 8).requires_grad_(True)
        rm, rv = torch.zeros(8), torch.ones(8)
        y = fn(xi, w, b, rm, rv)
        y.backward(g)
        outs.append((y.detach(), xi.grad, w.grad, b.grad, rm, rv))
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert (E.bn_hip_backwards(), E.bn_hip_backwards_x16()) == n0
