"""CPU: the pooled 16-bit stem forward's C ABI as far as it goes without a device (mhaq_fq_bn_norm_pool3s2_fwd_x16 in
csrc/bn_bwd.hip): the library exports the entry point, the ctypes table and the header declare it, and every argument error is
returned before any launch, in mhaq_fq_maxpool3s2_fwd_x16's order with the statistics among the required pointers."""
import ctypes
import os
import subprocess

import pytest

from mhaq_amd import _lib

NAME = "mhaq_fq_bn_norm_pool3s2_fwd_x16"
DTYPES = (_lib.DT_BF16, _lib.DT_F16)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbol_is_exported_declared_and_bound(L):
    assert NAME in _lib.SIGNATURES and NAME in _lib.header_functions() and hasattr(L, NAME)
    res, args = _lib.SIGNATURES[NAME]
    #             x mean invstd weight bias p code | n h w c | dtype | stream
    assert res is ctypes.c_int and args == [ctypes.c_void_p] * 7 + [ctypes.c_int64] * 4 + [ctypes.c_int, ctypes.c_void_p]
    assert L.mhaq_fq_abi_version() == 4               # additive: the ABI version stays


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_errors_are_returned_before_any_launch_in_the_documented_order(L, dt):
    """Every pointer is a fake host-side number: a call that got as far as a launch could not return these codes."""
    fake, odd8, odd4, odd2 = (ctypes.c_void_p(v) for v in (0x1000, 0x1008, 0x1004, 0x1002))
    n, h, w, c = 2, 5, 4, 8
    fwd = getattr(L, NAME)
    ok = [fake] * 7 + [n, h, w, c, dt, None]
    assert len(ok) == len(_lib.SIGNATURES[NAME][1])

    def call(**bad):
        args = list(ok)
        for k, v in bad.items():
            args[int(k[1:])] = v
        return fwd(*args)
    for k in (0, 1, 2, 5, 6):                       # x, mean, invstd, p, code: required (weight and bias are not)
        assert call(**{f"a{k}": None}) == -1, k
    for bad in (0, 3, -1, 7):                       # dtype: bf16 or fp16
        assert call(a11=bad) == -1, bad
    for k in (7, 8, 9, 10):                         # n, h, w, c: positive
        assert call(**{f"a{k}": 0}) == -1, k
        assert call(**{f"a{k}": -1}) == -1, k
    assert call(a10=12) == -4                       # C % 8 (a multiple of 4 is not enough)
    assert call(a10=(1 << 22) + 8) == -4            # C <= 2^22
    assert call(a7=1 << 11, a8=1 << 10, a9=1 << 10) == -4      # n * h * w >= 2^31: the pixel arithmetic is 32-bit
    for k in (0, 5):                                # x, p: 16-byte aligned
        assert call(**{f"a{k}": odd8}) == -3, k
    assert call(a6=odd4) == -3                      # code: 8-byte aligned
    for k in (1, 2, 3, 4):                          # mean, invstd, weight, bias: 4-byte aligned
        assert call(**{f"a{k}": odd2}) == -3, k
    # the order: NULL, then dtype, then the sizes, then width and range, then the alignment
    assert call(a1=None, a11=0, a10=12, a0=odd8) == -1
    assert call(a11=0, a10=12, a0=odd8) == -1
    assert call(a7=0, a10=12, a0=odd8) == -1
    assert call(a10=12, a0=odd8) == -4
    assert call(a10=12, a1=odd2) == -4
    assert call(a0=odd8, a1=odd2) == -3
