"""CPU: installing the fused block forwards (mhaq_amd/fused_blocks.py) changes no module name, no named_modules() order
and no state_dict key; copies and pickles keep working; a model wrapped with other layer classes is left alone; and the
C ABI declares and exports the entry points the fused path calls."""
import copy
import io
import os
import subprocess

import torch


def _quantized(layers=None):
    import mhaq_amd as M
    from mhaq_amd import nets, wrap
    net = nets.resnet18(10)
    wrap.quantize_model(net, M.QScheme.PER_CHANNEL, M.QNMethod.AEWGS, ("conv1", "fc"), False, 4, layers=layers)
    return net


def test_install_keeps_names_order_and_state_dict_keys():
    from mhaq_amd import fused_blocks, nets
    net = _quantized()
    names = [(n, type(m).__name__) for n, m in net.named_modules()]
    keys = list(net.state_dict().keys())
    nparams = sum(1 for _ in net.parameters())
    assert fused_blocks.install(net) == 9            # 8 blocks + the net (stem)
    after = [(n, type(m).__name__) for n, m in net.named_modules()]
    assert [n for n, _ in after] == [n for n, _ in names]
    changed = {(a[1], b[1]) for a, b in zip(names, after) if a[1] != b[1]}
    assert changed == {("BasicBlock", "FusedBasicBlock"), ("ResNet18", "FusedResNet18")}
    assert list(net.state_dict().keys()) == keys and sum(1 for _ in net.parameters()) == nparams
    assert isinstance(net, nets.ResNet18) and all(isinstance(b, nets.BasicBlock) for b in net.layer3)
    # every block but the last knows its consumer; nothing of that is a registered submodule
    blocks = [b for lay in (net.layer1, net.layer2, net.layer3, net.layer4) for b in lay]
    assert [b.__dict__.get("_mhaq_next") for b in blocks] == blocks[1:] + [None]
    assert fused_blocks.install(net) == 0            # idempotent
    dup = copy.deepcopy(net)
    assert type(dup) is fused_blocks.FusedResNet18 and dup.layer1[0].__dict__["_mhaq_next"] is dup.layer1[1]
    assert list(dup.state_dict().keys()) == keys
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert type(back.layer2[0]) is fused_blocks.FusedBasicBlock and list(back.state_dict().keys()) == keys
    assert back.layer4[0].__dict__["_mhaq_next"] is back.layer4[1]
    fused_blocks.uninstall(net)
    assert [(n, type(m).__name__) for n, m in net.named_modules()] == names
    assert all("_mhaq_next" not in b.__dict__ for b in blocks)


def test_nothing_is_installed_over_the_oracle_layers_or_an_unquantized_net():
    from mhaq_amd import fused_blocks, nets
    from oracle.ref_layers import ORACLE_LAYERS
    net = _quantized(ORACLE_LAYERS)
    assert fused_blocks.install(net) == 0
    assert type(net) is nets.ResNet18 and all(type(m) is not fused_blocks.FusedBasicBlock for m in net.modules())
    plain = nets.resnet18(10)
    assert fused_blocks.install(plain) == 0 and type(plain) is nets.ResNet18


def test_environment_switch(monkeypatch):
    from mhaq_amd import fused_blocks
    from mhaq_amd.qat import QATConfig
    assert QATConfig().fuse_blocks is True
    monkeypatch.delenv(fused_blocks.ENV_SWITCH, raising=False)
    assert fused_blocks.enabled_by_env()
    monkeypatch.setenv(fused_blocks.ENV_SWITCH, "0")
    assert not fused_blocks.enabled_by_env()
    monkeypatch.setenv(fused_blocks.ENV_SWITCH, "1")
    assert fused_blocks.enabled_by_env()
    assert fused_blocks.ENV_SWITCH == "MHAQ_FUSE_BLOCKS"


def test_header_declares_and_library_exports_the_fused_entry_points():
    from mhaq_amd import _lib
    names = ("mhaq_fq_act_relu_fwd", "mhaq_fq_act_relu_bwd", "mhaq_fq_act_relu_bwd_partials")
    declared = _lib.header_functions()
    for n in names:
        assert n in declared and n in _lib.SIGNATURES
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH), "libmhaq_fq.so"], check=True)
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n
    # argument validation without a GPU: the existing error codes
    assert L.mhaq_fq_act_relu_fwd(None, None, None, None, 16, None, None, None, None, None) == -1
    assert L.mhaq_fq_act_relu_bwd_partials(None, None, None, None, 16, None, 0, 0, 0, None, None, 0, None, None) == -1
    assert L.mhaq_fq_abi_version() == 4
