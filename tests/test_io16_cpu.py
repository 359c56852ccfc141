"""CPU: the 16-bit activation entry points (mhaq_fq_act_*_x16, include/mhaq_fq.h "16-bit activations") are exported and
bound, reject bad arguments with a return code before any launch, and the trainer refuses float16 autocast."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from mhaq_amd import _lib

X16 = ("mhaq_fq_act_fwd_x16", "mhaq_fq_act_bwd_x16", "mhaq_fq_act_bwd_partials_x16")
EINVAL, EWORKSPACE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4
BF16, F16 = 1, 2


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH)], check=True)
    return _lib.lib()


def test_the_three_entry_points_are_declared_exported_and_bound(L):
    declared = _lib.header_functions()
    for name in X16:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.mhaq_fq_abi_version() == 4          # additive: discovered by symbol, the version stays


def test_element_type_enum_matches_the_header():
    src = open(_lib.HEADER_PATH).read()
    assert re.search(r"MHAQ_FQ_DT_BF16\s*=\s*1\b", src) and re.search(r"MHAQ_FQ_DT_F16\s*=\s*2\b", src)
    assert (_lib.DT_BF16, _lib.DT_F16) == (BF16, F16)


def test_forward_argument_errors(L):
    fake = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x1001)
    nb = L.mhaq_fq_pt_fwd_workspace_bytes(1 << 16)
    # null data / parameter pointers, negative size
    assert L.mhaq_fq_act_fwd_x16(None, fake, 16, BF16, fake, fake, fake, fake, None, None, None, 0, None) == EINVAL
    assert L.mhaq_fq_act_fwd_x16(fake, fake, 16, BF16, None, fake, fake, fake, None, None, None, 0, None) == EINVAL
    assert L.mhaq_fq_act_fwd_x16(fake, fake, 16, BF16, fake, fake, fake, None, None, None, None, 0, None) == EINVAL
    assert L.mhaq_fq_act_fwd_x16(fake, fake, -1, BF16, fake, fake, fake, fake, None, None, None, 0, None) == EINVAL
    # unknown element type (0 = float32 is not a 16-bit type; 3 does not exist)
    for dt in (0, 3, -1):
        assert L.mhaq_fq_act_fwd_x16(fake, fake, 16, dt, fake, fake, fake, fake, None, None, None, 0, None) == EINVAL
    # 2-byte alignment is the minimum
    assert L.mhaq_fq_act_fwd_x16(odd, fake, 16, F16, fake, fake, fake, fake, None, None, None, 0, None) == EALIGN
    assert L.mhaq_fq_act_fwd_x16(fake, odd, 16, BF16, fake, fake, fake, fake, None, None, None, 0, None) == EALIGN
    # the eval form needs the fp32 query's workspace
    assert L.mhaq_fq_act_fwd_x16(fake, fake, 1 << 16, BF16, fake, fake, fake, fake, fake, fake, None, nb,
                                 None) == EWORKSPACE
    assert L.mhaq_fq_act_fwd_x16(fake, fake, 1 << 16, BF16, fake, fake, fake, fake, fake, None, fake, nb - 4,
                                 None) == EWORKSPACE


def test_backward_argument_errors(L):
    fake = ctypes.c_void_p(0x1000)
    odd = ctypes.c_void_p(0x1003)
    n = 1 << 16
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    for fn in (L.mhaq_fq_act_bwd_partials_x16, L.mhaq_fq_act_bwd_x16):
        tail = (fake, nb, fake, None) if fn is L.mhaq_fq_act_bwd_partials_x16 else (fake, fake, nb, None)

        def call(x=fake, g=fake, gx=fake, n=n, dt=BF16, params=fake, method=0, tail=tail):
            return fn(x, g, gx, n, dt, params, method, None, 0, 0, None, *tail)
        assert call(x=None) == EINVAL
        assert call(gx=None) == EINVAL
        assert call(params=None) == EINVAL
        assert call(n=-1) == EINVAL
        assert call(dt=0) == EINVAL and call(dt=7) == EINVAL
        assert call(method=9) == EINVAL
        assert call(method=2) == EUNSUPPORTED                 # AEWGS activations take the fp32 route
        assert call(x=odd) == EALIGN and call(g=odd, dt=F16) == EALIGN and call(gx=odd) == EALIGN
    # short / missing workspace
    assert L.mhaq_fq_act_bwd_partials_x16(fake, fake, fake, n, BF16, fake, 0, None, 0, 0, None, fake, nb - 1, fake,
                                          None) == EWORKSPACE
    assert L.mhaq_fq_act_bwd_partials_x16(fake, fake, fake, n, BF16, fake, 0, None, 0, 0, None, None, nb, fake,
                                          None) == EWORKSPACE
    assert L.mhaq_fq_act_bwd_x16(fake, fake, fake, n, F16, fake, 3, None, 0, 0, None, fake, fake, 16,
                                 None) == EWORKSPACE
    assert L.mhaq_fq_act_bwd_x16(fake, fake, fake, n, F16, fake, 3, None, 0, 0, None, None, fake, nb, None) == EINVAL


def test_header_documents_the_workspace_rule():
    src = open(_lib.HEADER_PATH).read()
    sec = src[src.index("16-bit activations"):src.index("mhaq_fq_act_bwd_partials_x16")]
    assert "Workspace rule" in sec and "mhaq_fq_act_bwd_workspace_bytes" in sec and "mhaq_fq_pt_fwd_workspace_bytes" in sec


def test_qat_config_autocast_dtype():
    from mhaq_amd.qat import QATConfig, QATTrainer
    assert QATConfig().autocast_dtype is None
    assert QATConfig(autocast_dtype=torch.bfloat16).autocast_dtype is torch.bfloat16
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Flatten())
    for bad in (torch.float16, torch.float64):
        with pytest.raises(ValueError, match="autocast_dtype"):
            QATTrainer(net, QATConfig(autocast_dtype=bad, distillation=False), "cpu")
