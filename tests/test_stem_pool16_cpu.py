"""CPU: the 16-bit stem pool's C ABI as far as it goes without a device (mhaq_fq_maxpool3s2_fwd_x16 /
mhaq_fq_bn_pool_bwd_x16 in csrc/bn_bwd.hip): the library exports the entry points, returns its argument errors before any
launch, in the documented order, and sizes the workspace as mhaq_fq_bn_bwd_x16 does."""
import ctypes
import os
import subprocess

import pytest

from mhaq_amd import _lib

NAMES = ("mhaq_fq_maxpool3s2_fwd_x16", "mhaq_fq_bn_pool_bwd_x16_workspace_bytes", "mhaq_fq_bn_pool_bwd_x16")
DTYPES = (_lib.DT_BF16, _lib.DT_F16)


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_symbols_are_exported_and_declared(L):
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(L, name)
    assert L.mhaq_fq_abi_version() == 4


def test_workspace_query_is_the_16_bit_batchnorm_backwards_own(L):
    for n, h, w, c in [(250, 112, 112, 64), (1, 1, 1, 8), (3, 5, 7, 24), (2, 7, 7, 512)]:
        nb = L.mhaq_fq_bn_pool_bwd_x16_workspace_bytes(n, h, w, c)
        assert nb > 0 and nb == L.mhaq_fq_bn_bwd_x16_workspace_bytes(n * h * w, c)
    assert L.mhaq_fq_bn_pool_bwd_x16_workspace_bytes(2, 4, 4, 12) == 0                # C % 8
    assert L.mhaq_fq_bn_pool_bwd_x16_workspace_bytes(0, 4, 4, 8) == 0
    assert L.mhaq_fq_bn_pool_bwd_x16_workspace_bytes(1 << 11, 1 << 10, 1 << 10, 8) == 0      # n * h * w = 2^31


@pytest.mark.parametrize("dt", DTYPES)
def test_argument_errors_are_returned_before_any_launch_in_the_documented_order(L, dt):
    fake, odd8, odd4, odd2 = (ctypes.c_void_p(v) for v in (0x1000, 0x1008, 0x1004, 0x1002))
    n, h, w, c = 2, 5, 4, 8
    nb = L.mhaq_fq_bn_pool_bwd_x16_workspace_bytes(n, h, w, c)
    bwd = L.mhaq_fq_bn_pool_bwd_x16
    #     x g code mean invstd weight dx dweight dbias | n h w c dtype | workspace bytes stream
    ok = [fake] * 9 + [n, h, w, c, dt, fake, nb, None]
    assert len(ok) == len(_lib.SIGNATURES["mhaq_fq_bn_pool_bwd_x16"][1])

    def call(**bad):
        args = list(ok)
        for k, v in bad.items():
            args[int(k[1:])] = v
        return bwd(*args)
    for k in (0, 1, 2, 3, 4, 14):                   # x, g, code, mean, invstd, workspace: required
        assert call(**{f"a{k}": None}) == -1, k
    for bad in (0, 3, -1, 7):                       # dtype: bf16 or fp16
        assert call(a13=bad) == -1, bad
    for k in (9, 10, 11, 12):                       # n, h, w, c: positive
        assert call(**{f"a{k}": 0}) == -1, k
    assert call(a12=12) == -4                       # C % 8 (a multiple of 4 is not enough)
    assert call(a9=1 << 11, a10=1 << 10, a11=1 << 10, a15=1 << 62) == -4      # n * h * w >= 2^31: the pixel arithmetic is 32-bit
    assert call(a15=nb - 1) == -2
    for k in (0, 1, 6, 14):                         # x, g, dx, workspace: 16-byte aligned
        assert call(**{f"a{k}": odd8}) == -3, k
    assert call(a2=odd4) == -3                      # code: 8-byte aligned
    for k in (3, 4, 5, 7, 8):                       # mean, invstd, weight, dweight, dbias: 4-byte aligned
        assert call(**{f"a{k}": odd2}) == -3, k
    # the order: NULL, then dtype, then the dimensions, then the workspace, then the alignment
    assert call(a0=None, a13=0, a12=12, a15=0, a1=odd8) == -1
    assert call(a13=0, a12=12, a15=0, a1=odd8) == -1
    assert call(a12=12, a15=0, a1=odd8) == -4
    assert call(a15=0, a1=odd8) == -2
    # nothing to compute: no launch, no error (weight and every output are optional)
    assert bwd(fake, fake, fake, fake, fake, None, None, None, None, n, h, w, c, dt, fake, nb, None) == 0
    fwd = L.mhaq_fq_maxpool3s2_fwd_x16
    fok = [fake, fake, fake, n, h, w, c, dt, None]

    def fcall(**bad):
        args = list(fok)
        for k, v in bad.items():
            args[int(k[1:])] = v
        return fwd(*args)
    for k in (0, 1, 2):
        assert fcall(**{f"a{k}": None}) == -1, k
    assert fcall(a7=0) == -1 and fcall(a7=3) == -1
    for k in (3, 4, 5, 6):
        assert fcall(**{f"a{k}": 0}) == -1, k
    assert fcall(a6=12) == -4
    assert fcall(a3=1 << 11, a4=1 << 10, a5=1 << 10) == -4
    assert fcall(a0=odd8) == -3 and fcall(a1=odd8) == -3 and fcall(a2=odd4) == -3
    assert fcall(a7=0, a6=12, a0=odd8) == -1 and fcall(a6=12, a0=odd8) == -4
