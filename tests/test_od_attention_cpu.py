"""CPU: the argument checks of the mhaq_fq_od_attn calls and of psa_attention, which need no GPU, and the parameter names of the
Attention module."""
import ctypes

import pytest
import torch

from mhaq_amd import _lib
from mhaq_amd.od_attention import Attention, psa_attention


def test_argument_errors_are_returned_before_any_launch():
    L = _lib.lib()
    buf = (ctypes.c_double * 64)()                      # host memory: a call that launched anything would not return a code
    p = ctypes.addressof(buf)
    nb = L.mhaq_fq_od_attn_bwd_workspace_bytes(2, 3, 25)
    assert nb == 2 * 3 * 25 * 4 and L.mhaq_fq_od_attn_bwd_workspace_bytes(2, 3, 16385) == 0

    def fwd(qkv=p, out=p, dtype=_lib.DT_F32, n=25, dk=32, dh=64, nh=3):
        return L.mhaq_fq_od_attn_fwd(qkv, None, dtype, 2, nh, n, dk, dh, out, None, None)

    def bwd(qkv=p, go=p, lse=p, dq=p, ws=p, ws_bytes=nb, dtype=_lib.DT_F32, n=25, dk=32, dh=64, nh=3):
        return L.mhaq_fq_od_attn_bwd(qkv, go, lse, dtype, 2, nh, n, dk, dh, dq, ws, ws_bytes, None)

    for call, pointers in ((fwd, ("qkv", "out")), (bwd, ("qkv", "go", "lse", "dq", "ws"))):
        for name in pointers:
            assert call(**{name: None}) == -1, (call.__name__, name)
        assert call(dtype=7) == -1 and call(n=-1) == -1 and call(nh=0) == -1 and call(dk=0) == -1
        assert call(dk=16) == -4 and call(dh=32) == -4 and call(dh=128) == -4
        assert call(n=16385) == -4 and call(nh=1 << 16) == -4
        assert call(qkv=p + 2) == -3
        assert call(n=0) == 0 and call(n=0, qkv=None) == 0          # nothing to launch
    assert bwd(ws_bytes=nb - 1) == -2 and bwd(ws=p + 2) == -3 and bwd(lse=p + 2) == -3


@pytest.mark.parametrize("channels,num_head", [(64, 1), (256, 1), (128, 2), (130, 1)])
def test_unsupported_head_sizes_raise_value_error(channels, num_head):
    with pytest.raises(ValueError):
        psa_attention(torch.zeros(1, channels, 2, 2), num_head)


def test_host_tensors_are_refused():
    with pytest.raises(_lib.MhaqFqError, match="no CPU fallback"):
        psa_attention(torch.zeros(1, 128, 2, 2), 1)
    with torch.no_grad(), pytest.raises(_lib.MhaqFqError, match="no CPU fallback"):
        psa_attention(torch.zeros(1, 256, 2, 2), 2, torch.zeros(1, 128, 2, 2))


def test_state_dict_keys_are_the_reference_modules():
    m = Attention(128, 2)
    assert list(m.state_dict()) == [
        "qkv.conv.weight", "qkv.norm.weight", "qkv.norm.bias", "qkv.norm.running_mean", "qkv.norm.running_var",
        "qkv.norm.num_batches_tracked",
        "conv1.conv.weight", "conv1.norm.weight", "conv1.norm.bias", "conv1.norm.running_mean", "conv1.norm.running_var",
        "conv1.norm.num_batches_tracked",
        "conv2.conv.weight", "conv2.norm.weight", "conv2.norm.bias", "conv2.norm.running_mean", "conv2.norm.running_var",
        "conv2.norm.num_batches_tracked"]
    assert m.qkv.conv.weight.shape == (256, 128, 1, 1) and m.conv1.conv.weight.shape == (128, 1, 3, 3)
    assert (m.qkv.norm.eps, m.qkv.norm.momentum) == (1e-3, 0.03) and isinstance(m.qkv.relu, torch.nn.Identity)
