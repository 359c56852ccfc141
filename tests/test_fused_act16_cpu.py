"""CPU: the ReLU / residual-add forms of the 16-bit activation kernels (mhaq_fq_act_relu_*_x16, include/mhaq_fq.h) are
declared, exported and bound, reject bad arguments with the existing return codes before any launch, and their arithmetic
contract -- restated in torch (tests/fused_act16_contract.py) -- is the composition of 16-bit torch ops it stands in for,
double rounding of the accumulated gradient included."""
import ctypes
import os
import subprocess

import pytest
import torch

from mhaq_amd import _lib
from tests import fused_act16_contract as K

RELU16 = ("mhaq_fq_act_relu_fwd_x16", "mhaq_fq_act_relu_bwd_x16", "mhaq_fq_act_relu_bwd_partials_x16")
EINVAL, EWORKSPACE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4
BF16, F16 = 1, 2


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_the_three_entry_points_are_declared_exported_and_bound(L):
    declared = _lib.header_functions()
    for name in RELU16:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.mhaq_fq_abi_version() == 4          # additive: discovered by symbol, the version stays


def test_the_compiled_binding_resolves_them():
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "torch_binding.cpp")).read()
    api = src[src.index("#define MHAQ_API(X)"):src.index("struct Api")]
    for name in RELU16:
        assert f"X({name})" in api, name


def test_forward_argument_errors(L):
    fake = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x1001)

    def call(z=fake, addend=None, y=fake, a_out=None, n=16, dt=BF16, ls=fake, lq=fake, b=fake, po=fake):
        return L.mhaq_fq_act_relu_fwd_x16(z, addend, y, a_out, n, dt, ls, lq, b, po, None)
    # null data / parameter pointers, negative size (the cases of mhaq_fq_act_fwd_x16 and of mhaq_fq_act_relu_fwd)
    assert call(z=None) == EINVAL and call(y=None) == EINVAL
    assert call(ls=None) == EINVAL and call(lq=None) == EINVAL and call(b=None) == EINVAL and call(po=None) == EINVAL
    assert call(n=-1) == EINVAL
    # unknown element type (0 = float32 is not a 16-bit type; 3 does not exist)
    for dt in (0, 3, -1):
        assert call(dt=dt) == EINVAL
    # 2-byte alignment is the minimum, for every data pointer that is given
    assert call(z=odd, dt=F16) == EALIGN and call(y=odd) == EALIGN
    assert call(addend=odd) == EALIGN and call(a_out=odd, dt=F16) == EALIGN
    # an unknown element type is reported before the alignment, as in mhaq_fq_act_fwd_x16
    assert call(z=odd, dt=0) == EINVAL


def test_backward_argument_errors(L):
    fake = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x1003)
    n = 1 << 16
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    for fn in (L.mhaq_fq_act_relu_bwd_partials_x16, L.mhaq_fq_act_relu_bwd_x16):
        tail = (fake, nb, fake, None) if fn is L.mhaq_fq_act_relu_bwd_partials_x16 else (fake, fake, nb, None)

        def call(z=fake, g=fake, ga=None, gx=fake, n=n, dt=BF16, params=fake, method=0, tail=tail):
            return fn(z, g, ga, gx, n, dt, params, method, 0, 0, None, *tail)
        assert call(z=None) == EINVAL
        assert call(g=None) == EINVAL
        assert call(gx=None) == EINVAL
        assert call(params=None) == EINVAL
        assert call(n=-1) == EINVAL
        assert call(dt=0) == EINVAL and call(dt=7) == EINVAL
        assert call(method=9) == EINVAL and call(method=7) == EINVAL
        assert call(method=2) == EUNSUPPORTED                 # AEWGS activations take the fp32 route
        assert call(z=odd) == EALIGN and call(g=odd, dt=F16) == EALIGN and call(gx=odd) == EALIGN
        assert call(ga=odd) == EALIGN
        # order: method before alignment before workspace (mhaq_fq_act_relu_bwd_partials, mhaq_fq_act_bwd_partials_x16)
        assert call(z=odd, method=9) == EINVAL
    P = L.mhaq_fq_act_relu_bwd_partials_x16
    # short / missing workspace
    assert P(fake, fake, None, fake, n, BF16, fake, 0, 0, 0, None, fake, nb - 1, fake, None) == EWORKSPACE
    assert P(fake, fake, fake, fake, n, BF16, fake, 0, 0, 0, None, None, nb, fake, None) == EWORKSPACE
    assert P(fake, fake, None, fake, 64, BF16, fake, 0, 0, 0, None, fake, 8, fake, None) == EWORKSPACE
    assert P(odd, fake, None, fake, n, BF16, fake, 0, 0, 0, None, fake, 8, fake, None) == EALIGN
    B = L.mhaq_fq_act_relu_bwd_x16
    assert B(fake, fake, None, fake, n, F16, fake, 3, 0, 0, None, fake, fake, 16, None) == EWORKSPACE
    assert B(fake, fake, None, fake, n, F16, fake, 3, 0, 0, None, None, fake, nb, None) == EINVAL       # grads


def test_header_states_the_double_rounding():
    src = open(_lib.HEADER_PATH).read()
    sec = src[src.index("NoisyAct behind a ReLU under torch.autocast"):src.index("int mhaq_fq_act_relu_fwd_x16")]
    assert "rounded TWICE" in sec and "R(up(gq) + up(g_a))" in sec and "R(up(z) + up(addend))" in sec


# ----------------------------------------------------------------------------- the contract, in torch on the CPU
class _Quant16(torch.autograd.Function):
    """A stand-in for the 16-bit quantizer launches: 16-bit in, fp32 inside, rounded once on the way out -- forward and
    backward (the contract of mhaq_fq_act_fwd_x16 / _bwd_x16 around arbitrary fp32 element functions)."""

    @staticmethod
    def forward(ctx, a, fwd32, bwd32):
        ctx.save_for_backward(a)
        ctx.bwd32 = bwd32
        return fwd32(a.float()).to(a.dtype)

    @staticmethod
    def backward(ctx, g):
        (a,) = ctx.saved_tensors
        return ctx.bwd32(a.float(), g.float()).to(g.dtype), None, None


def _composition(z0, add0, gy, ga, fwd32, bwd32):
    """Today's unfused chain in 16-bit torch ops: add, relu, the quantizer, autograd's accumulation, threshold_backward."""
    z = z0.clone().requires_grad_(True)
    add = add0.clone().requires_grad_(True) if add0 is not None else None
    a = torch.relu(z + add if add is not None else z)
    y = _Quant16.apply(a, fwd32, bwd32)
    outs, gs = ([y, a], [gy, ga]) if ga is not None else ([y], [gy])
    torch.autograd.backward(outs, gs)
    if add is not None:
        assert _same(add.grad, z.grad)
    return y.detach(), a.detach(), z.grad


def _same(a, b):
    """Bit-equal up to the sign of zero and NaN payloads: equal values, NaNs at the same positions."""
    return a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_contract_on_a_constructed_pair_needs_the_double_rounding(dtype):
    m = K.MANTISSA_BITS[dtype]
    eps = 2.0 ** -(m + 1)                              # half a unit in the last place at 1.0
    fwd32 = lambda a: a * 0.5                          # noqa: E731
    bwd32 = lambda a, g: g * (1.0 + eps)               # noqa: E731   g = 1: p = 1 + eps, a tie: R(p) = 1
    z = torch.tensor([2.0, 2.0, -1.0, 0.0], dtype=dtype)
    gy = torch.ones(4, dtype=dtype)
    ga = torch.tensor([eps, 0.25, eps, eps], dtype=dtype)
    # element 0: R(p) + g_a = 1 + eps is a tie again -> 1;  p + g_a = 1 + 2 eps is a 16-bit number
    double = K.backward(z, gy, ga, bwd32)
    single = K.backward(z, gy, ga, bwd32, single_rounding=True)
    assert float(double[0]) == 1.0 and float(single[0]) == 1.0 + 2 * eps
    assert float(double[1]) == float(single[1]) == 1.25
    assert float(double[2]) == 0.0 and float(double[3]) == 0.0          # masked: z <= 0
    y, a, gx = _composition(z, None, gy, ga, fwd32, bwd32)
    assert torch.equal(gx, double) and not torch.equal(gx, single)
    yk, ak = K.forward(z, None, fwd32)
    assert torch.equal(y, yk) and torch.equal(a, ak)
    # and the planted gradient of the GPU tests finds such a g_a for an arbitrary p
    p = torch.tensor([1.0 + eps / 2, -3.3, 0.0078125 * (1 + eps / 4), 7.0])
    g_a, ok = K.plant_double_rounding(p, dtype)
    assert ok.tolist() == [True, True, True, False]                      # 7.0 is a 16-bit number: nothing to round twice
    assert bool(((p.to(dtype).float() + g_a.float()).to(dtype) != (p + g_a.float()).to(dtype))[:3].all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_add", [False, True])
def test_contract_equals_the_16bit_torch_composition(dtype, with_add):
    """Random and special values through a clamp-and-scale stand-in quantizer: the restated contract gives the bits of
    torch's 16-bit add / relu / threshold_backward / gradient accumulation; the single-rounding variant does not."""
    gen = torch.Generator().manual_seed(5)
    n = 4099
    z = (torch.randn(n, generator=gen) * 2).to(dtype)
    add = (torch.randn(n, generator=gen)).to(dtype) if with_add else None
    gy = torch.randn(n, generator=gen).to(dtype)
    ga = torch.randn(n, generator=gen).to(dtype)
    nan, inf = float("nan"), float("inf")
    z[0::97] = 0.0
    z[1::97] = -0.0
    z[2::97] = nan
    z[3::97] = inf
    z[4::97] = -inf
    gy[5::97] = nan
    ga[6::97] = inf
    ga[7::97] = nan
    gy[8::97] = -inf
    if with_add:
        add[9::97] = -z[9::97]                           # exact cancellation
        add[3::97] = -inf                                # inf + (-inf)
        z[10::97] = 1.0
        add[10::97] = 2.0 ** -(K.MANTISSA_BITS[dtype] + 1)          # z + addend needs rounding (a tie)
    fwd32 = lambda a: torch.round(torch.clamp(a, 0.25, 3.0) * 7.3) / 7.3                # noqa: E731
    bwd32 = lambda a, g: torch.where((a >= 0.25) & (a <= 3.0), g * 1.0371, g * 0.0)      # noqa: E731
    y, a, gx = _composition(z, add, gy, ga, fwd32, bwd32)
    yk, ak = K.forward(z, add, fwd32)
    assert _same(y, yk) and _same(a, ak)
    gk = K.backward(a, gy, ga, bwd32)                    # from the ReLU's output ...
    assert _same(gx, gk)
    if not with_add:
        assert _same(gx, K.backward(z, gy, ga, bwd32))   # ... or from its input
    assert not _same(gx, K.backward(a, gy, ga, bwd32, single_rounding=True))
    assert _same(_composition(z, add, gy, None, fwd32, bwd32)[2], K.backward(a, gy, None, bwd32))
