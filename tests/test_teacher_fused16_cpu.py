"""CPU: the frozen teacher's fused forward on 16-bit tensors (mhaq_fq_bn_infer_act_x16 / mhaq_fq_bn_relu_pool3s2_x16 in
csrc/bn_bwd.hip, install(model, x16=True) of mhaq_amd/frozen_blocks.py, QATConfig.fuse_teacher_16bit) as far as it goes without a
device: the library exports the entry points and returns its argument errors before any launch, in the documented order; the
switches parse; the flag of install(x16=True) is a per-instance attribute that deepcopy keeps and uninstall drops; the contract
evaluated by torch in fp32 and cast once stays inside its bound on the planted cases, and the checker is not vacuous."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

from mhaq_amd import _lib, frozen_blocks, nets
from tests import teacher_fused16_contract as K16
from tests import teacher_fused_contract as K
from tests.test_teacher_fused_cpu import KINDS, _net

NAMES = ("mhaq_fq_bn_infer_act_x16", "mhaq_fq_bn_relu_pool3s2_x16")
FAKE, ODD = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
BF16, F16 = _lib.DT_BF16, _lib.DT_F16


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbols_are_exported_declared_bound_and_of_the_headers_arity(L):
    with open(_lib.HEADER_PATH) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "torch_binding.cpp")) as f:
        binding = f.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert re.search(r"X\(" + name + r"\)", binding), name                          # in the loader's list
    assert _lib.SIGNATURES["mhaq_fq_bn_infer_act_x16"][1][-2] is ctypes.c_int           # dtype, in front of the stream
    assert _lib.SIGNATURES["mhaq_fq_bn_relu_pool3s2_x16"][1][-2] is ctypes.c_int
    assert L.mhaq_fq_abi_version() == 4


def _act(L, mode=K.BN_RELU, **kw):
    a = dict(x=FAKE, consts=FAKE, x2=None, consts2=None, residual=None, y=FAKE, m=64, c=8, mode=mode, dtype=BF16, stream=None)
    if mode == K.BN_ADD_RELU:
        a["residual"] = FAKE
    if mode == K.BN2_ADD_RELU:
        a["x2"] = a["consts2"] = FAKE
    a.update(kw)
    return L.mhaq_fq_bn_infer_act_x16(*a.values())


def _pool(L, **kw):
    a = dict(x=FAKE, consts=FAKE, p=FAKE, n=2, h=5, w=7, c=8, dtype=BF16, stream=None)
    a.update(kw)
    return L.mhaq_fq_bn_relu_pool3s2_x16(*a.values())


def test_argument_errors_are_returned_before_any_launch(L):
    for dt in (BF16, F16):
        for mode in (K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU):
            for k in ("x", "consts", "y"):
                assert _act(L, mode, dtype=dt, **{k: None}) == -1, (mode, k)
                assert _act(L, mode, dtype=dt, **{k: ODD}) == -3, (mode, k)
            assert _act(L, mode, dtype=dt, m=0) == -1 and _act(L, mode, dtype=dt, c=0) == -1
            assert _act(L, mode, dtype=dt, m=-1) == -1
            # c = 12: a multiple of 4, which the fp32 entry point takes, but not of 8
            assert _act(L, mode, dtype=dt, c=12) == -4 and _act(L, mode, dtype=dt, c=4) == -4
            assert _act(L, mode, dtype=dt, c=1 << 23) == -4 and _act(L, mode, dtype=dt, m=1 << 60) == -4
        for k in ("x", "consts", "p"):
            assert _pool(L, dtype=dt, **{k: None}) == -1, k
            assert _pool(L, dtype=dt, **{k: ODD}) == -3, k
        for k in ("n", "h", "w", "c"):
            assert _pool(L, dtype=dt, **{k: 0}) == -1, k
        assert _pool(L, dtype=dt, c=12) == -4 and _pool(L, dtype=dt, c=1 << 23) == -4
        assert _pool(L, dtype=dt, n=1 << 20, h=1 << 6, w=1 << 5) == -4                   # n * h * w = 2^31
    for dt in (0, 3, -1):                                                                # an unknown dtype
        assert _act(L, dtype=dt) == -1 and _pool(L, dtype=dt) == -1
    assert _act(L, 3) == -1 and _act(L, -1) == -1                                        # an unknown mode
    # a mode's own operands are required, the other modes' refused
    assert _act(L, K.BN_RELU, residual=FAKE) == -1 and _act(L, K.BN_RELU, x2=FAKE, consts2=FAKE) == -1
    assert _act(L, K.BN_ADD_RELU, residual=None) == -1 and _act(L, K.BN_ADD_RELU, x2=FAKE, consts2=FAKE) == -1
    assert _act(L, K.BN2_ADD_RELU, x2=None) == -1 and _act(L, K.BN2_ADD_RELU, consts2=None) == -1
    assert _act(L, K.BN2_ADD_RELU, residual=FAKE) == -1
    assert _act(L, K.BN_ADD_RELU, residual=ODD) == -3
    assert _act(L, K.BN2_ADD_RELU, x2=ODD) == -3 and _act(L, K.BN2_ADD_RELU, consts2=ODD) == -3


def test_argument_errors_come_in_the_documented_order(L):
    """Several things wrong at once: NULL / size / mode / operands, then the dtype (all EINVAL, in front of everything else),
    then width and range, then the alignment."""
    for mode in (K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU):
        worst = dict(y=ODD, c=12)
        assert _act(L, mode, **dict(worst, x=None)) == -1 and _act(L, mode, **dict(worst, m=0)) == -1
        assert _act(L, mode, **dict(worst, dtype=7)) == -1                               # the dtype before width and alignment
        assert _act(L, mode, **worst) == -4 and _act(L, mode, **dict(worst, c=8, m=1 << 60)) == -4
        assert _act(L, mode, **dict(worst, c=8)) == -3
        assert _act(L, mode, y=ODD, dtype=0) == -1
    assert _act(L, 7, y=ODD, c=12) == -1 and _act(L, 7, dtype=9) == -1
    assert _act(L, K.BN_RELU, residual=ODD, c=12) == -1                                  # a refused operand, misaligned too
    assert _act(L, K.BN2_ADD_RELU, x2=ODD, c=12) == -4
    assert _pool(L, x=None, c=12, p=ODD) == -1 and _pool(L, h=0, c=12, p=ODD) == -1
    assert _pool(L, dtype=0, c=12, p=ODD) == -1 and _pool(L, dtype=0, n=1 << 31) == -1
    assert _pool(L, c=12, p=ODD) == -4 and _pool(L, n=1 << 31, p=ODD) == -4
    assert _pool(L, p=ODD) == -3


def test_default_and_switch_parsing(monkeypatch):
    from mhaq_amd.qat import QATConfig
    assert QATConfig().fuse_teacher_16bit is False and QATConfig().fuse_teacher is True
    assert frozen_blocks.ENV_SWITCH_X16 == "MHAQ_TEACHER_FUSED_X16"
    monkeypatch.delenv(frozen_blocks.ENV_SWITCH_X16, raising=False)
    assert frozen_blocks.x16_enabled() is False and frozen_blocks.x16_enabled(False) is False
    assert frozen_blocks.x16_enabled(True) is True
    for v in ("1", "true", "ON", " yes "):                                               # when set it decides, either way
        monkeypatch.setenv(frozen_blocks.ENV_SWITCH_X16, v)
        assert frozen_blocks.x16_enabled(False) is True and frozen_blocks.x16_enabled(True) is True
    for v in ("0", "false", "off", "no", "2"):
        monkeypatch.setenv(frozen_blocks.ENV_SWITCH_X16, v)
        assert frozen_blocks.x16_enabled(True) is False and frozen_blocks.x16_enabled(False) is False
    for v in ("", "  "):                                                                 # empty: not set
        monkeypatch.setenv(frozen_blocks.ENV_SWITCH_X16, v)
        assert frozen_blocks.x16_enabled(True) is True and frozen_blocks.x16_enabled(False) is False
    monkeypatch.setenv(frozen_blocks.ENV_SWITCH_X16, "1")                                # the fp32 switch is its own
    assert frozen_blocks.enabled_by_env() is True


def _switched(net):
    return [m for m in net.modules() if type(m) in (frozen_blocks.FrozenBasicBlock, frozen_blocks.FrozenResNet18)]


def test_install_x16_flags_instances_and_keeps_names_state_dict_and_deepcopy():
    net = _net()
    names, keys = [n for n, _ in net.named_modules()], list(net.state_dict().keys())
    buffers, params = [n for n, _ in net.named_buffers()], [n for n, _ in net.named_parameters()]
    assert frozen_blocks.install(net, x16=True) == 9
    assert [n for n, _ in net.named_modules()] == names and list(net.state_dict().keys()) == keys
    assert [n for n, _ in net.named_buffers()] == buffers and [n for n, _ in net.named_parameters()] == params
    sw = _switched(net)
    assert len(sw) == 9 and all(frozen_blocks.takes_x16(m) for m in sw)
    assert all(frozen_blocks._X16 in m.__dict__ for m in sw)                             # per instance, not on the class
    assert not hasattr(frozen_blocks.FrozenBasicBlock, frozen_blocks._X16)
    assert not any(hasattr(m, "takes_x16") for m in net.modules())                       # no attribute or method of that name
    assert not any(frozen_blocks.takes_x16(m) for m in net.modules() if m not in sw)
    dup = copy.deepcopy(net)
    assert list(dup.state_dict().keys()) == keys and all(frozen_blocks.takes_x16(m) for m in _switched(dup))
    assert len(_switched(dup)) == 9
    frozen_blocks.uninstall(net)
    assert type(net) is nets.ResNet18 and not any(frozen_blocks._X16 in m.__dict__ for m in net.modules())
    assert all(frozen_blocks.takes_x16(m) for m in _switched(dup))                       # the copy is its own
    # the default installs without the flag, and an install without it takes an earlier flag away
    assert frozen_blocks.install(net) == 9 and not any(frozen_blocks.takes_x16(m) for m in net.modules())
    assert frozen_blocks.install(dup) == 9 and not any(frozen_blocks.takes_x16(m) for m in dup.modules())


def test_a_flagged_cpu_model_runs_the_stock_forward_bit_for_bit():
    net = _net()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        want = net(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            want16 = net(x)
        assert frozen_blocks.install(net, x16=True) == 9
        assert torch.equal(net(x), want)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            got16 = net(x)
    assert got16.dtype == want16.dtype and torch.equal(got16, want16)


SHAPES = [(1, 8), (7, 24), (513, 64), (98, 512)]


def _case(kind, m, c, dtype):
    x, rm, rv, gamma, beta, eps = K.planted(kind, m, c)
    x2, rm2, rv2, gamma2, beta2, eps2 = K.planted(kind, m, c, seed=5)
    r = torch.randn(m, c, generator=torch.Generator().manual_seed(9)) * 3
    k, k2 = K.slab(rm, rv, gamma, beta, eps), K.slab(rm2, rv2, gamma2, beta2, eps2)
    c64, c64_2 = K.consts64(rm, rv, gamma, beta, eps), K.consts64(rm2, rv2, gamma2, beta2, eps2)
    return x.to(dtype), x2.to(dtype), r.to(dtype), k, k2, c64, c64_2


@pytest.mark.parametrize("dtype", K16.DTYPES, ids=K16.DT_IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_contract_in_16_bits_stays_inside_its_bound(shape, kind, dtype):
    m, c = shape
    x, x2, r, k, k2, c64, c64_2 = _case(kind, m, c, dtype)
    for mode in (K.BN_RELU, K.BN_ADD_RELU, K.BN2_ADD_RELU):
        y = K16.want(x, k, mode, r=r, x2=x2, k2=k2)
        assert y.dtype == dtype and bool(torch.isfinite(y).all())                        # fp16: far below 65504
        worst = K16.check16(y, *K.ref64(x.float(), c64, mode, r=r.float(), x2=x2.float(), c64_2=c64_2))
        print(shape, kind, mode, f"{worst:.3f} of the bound")
    if m >= 4:
        n = 2 if m % 2 == 0 else 1
        h = 7 if (m // n) % 7 == 0 else 1
        x4 = x.reshape(n, h, m // n // h, c).permute(0, 3, 1, 2)
        print(shape, kind, "pool", f"{K16.check16(K16.want_pool(x4, k), *K.ref64_pool(x4.float(), c64)):.3f} of the bound")


@pytest.mark.parametrize("dtype", K16.DTYPES, ids=K16.DT_IDS)
def test_checker_rejects_a_result_rounded_twice_and_shifted_constants(dtype):
    """The checkers are not vacuous.  t is rounded to 16 bits before the add: wherever that changes the result the bit-level
    comparison fails, and where the residual nearly cancels t (y ~ 0.37 from a |t| of several units: an error of up to u |t| / 2
    against a bound of 0.37 u + 1e-6 T) the fp64 bound fails too.  Constants of the neighbouring channel fail both."""
    m, c = 513, 64
    x, _, r, k, _, c64, _ = _case("plain", m, c, dtype)
    t = K._t32(x.float(), k)
    r[:64] = (0.37 - t[:64]).to(dtype)                                                   # rows 0..63: the residual nearly cancels t
    want = K16.want(x, k, K.BN_ADD_RELU, r=r)
    twice = K16.rounded_twice(x, k, r)
    differs = (want != twice) & ~torch.isnan(want)
    assert int(differs.sum()) > 100, "the case plants nothing"
    y64, T = K.ref64(x.float(), c64, K.BN_ADD_RELU, r=r.float())
    K16.same_values(want, want.clone())
    K16.check16(want, y64, T)
    planted = torch.where(differs, twice, want)
    with pytest.raises(AssertionError):
        K16.same_values(planted, want)
    with pytest.raises(AssertionError):
        K16.check16(planted, y64, T)
    one = want.clone()                                                                   # a single element is enough
    i = tuple(int(v) for v in differs.nonzero()[0])
    one[i] = twice[i]
    with pytest.raises(AssertionError):
        K16.same_values(one, want)
    shifted = K16.want(x, k.roll(1, dims=1), K.BN_ADD_RELU, r=r)
    with pytest.raises(AssertionError):
        K16.same_values(shifted, want)
    with pytest.raises(AssertionError):
        K16.check16(shifted, y64, T)
    nan = want.clone()                                                                   # a ReLU that drops a NaN
    xn = x.clone()
    xn[9, 5] = float("nan")
    wn = K16.want(xn, k, K.BN_ADD_RELU, r=r)
    assert bool(torch.isnan(wn[9, 5]))
    with pytest.raises(AssertionError):
        K16.same_values(nan, wn)
