"""CPU: after mhaq_amd.compat.install() the REFERENCE's own ModelHelper and PotentialLoss modules -- imported
unchanged -- operate on this package's layer classes: isinstance checks, parameter names and shapes line up.
What those reference modules computed on a toy net of this package's layers is recorded in
tests/golden/compat_cases.npz (oracle/gen_compat_fixture.py, run against the reference); here the stand-in modules
are checked to resolve to this package's classes, and the same net reproduces the recorded regulariser inputs (bit for
bit), loss and gradients through the package's gathering (mhaq_amd/wrap.py) and the CPU port of the loss."""
import sys

import numpy as np
import torch

from tests.golden_util import GOLDEN

FIXTURE = f"{GOLDEN}/compat_cases.npz"


def test_reference_model_helper_runs_on_our_layers():
    import mhaq_amd
    from mhaq_amd import compat, layers, ops_generic, wrap
    from mhaq_amd.gdnsq import Quantizer
    from oracle.loss import PotentialLossNoPred
    z = np.load(FIXTURE)
    saved = {k: v for k, v in sys.modules.items() if k == "src" or k.startswith("src.")}
    try:
        compat.install()
        # the four modules the reference imports the path from now hold this package's classes
        mods = sys.modules
        assert mods["src.quantization.gdnsq.layers.gdnsq_conv2d"].NoisyConv2d is mhaq_amd.NoisyConv2d
        assert mods["src.quantization.gdnsq.layers.gdnsq_act"].NoisyAct is layers.NoisyAct
        assert mods["src.quantization.gdnsq.layers.gdnsq_linear"].NoisyLinear is layers.NoisyLinear
        g = mods["src.quantization.gdnsq.gdnsq"]
        assert g.Quantizer is Quantizer and g.QNLSQ is ops_generic.QNLSQ and g.QNAEWGS is ops_generic.QNAEWGS
        qs = mhaq_amd.QScheme.PER_CHANNEL
        net = torch.nn.Sequential(
            mhaq_amd.NoisyAct(signed=True),
            mhaq_amd.NoisyConv2d(3, 6, 3, qscheme=qs, qnmethod=mhaq_amd.QNMethod.LSQ),
            torch.nn.ReLU(),
            mhaq_amd.NoisyAct(signed=False),
            mhaq_amd.NoisyConv2d(6, 4, 3, qscheme=qs, qnmethod=mhaq_amd.QNMethod.LSQ))
        state = {k[len("state__"):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("state__")}
        net.load_state_dict(state, strict=True)
        ref_vals = [torch.from_numpy(z[f"ref_vals__{i}"].copy()) for i in range(4)]
        our_vals = wrap.get_model_values(net, qs)
        assert len(our_vals) == len(ref_vals)
        for a, b in zip(ref_vals, our_vals):
            assert torch.equal(a, b)
        crit = PotentialLossNoPred(None, p=1, a=4, w=4)
        crit.t, crit.loss_sum, crit.cnt = 0.5, torch.tensor(1.0), 1
        loss = crit((torch.tensor(2.0, requires_grad=True) * 1.0, *our_vals))
        assert np.allclose(loss.detach().numpy(), z["loss"], rtol=1e-6, atol=1e-7)
        loss.backward()
        assert net[1].log_wght_s.grad is not None and net[0].log_act_s.grad is not None
        for name, p in net.named_parameters():
            got = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
            assert np.allclose(got, z[f"grad__{name}"], rtol=1e-6, atol=1e-7), name
    finally:
        for k in [k for k in sys.modules if k == "src" or k.startswith("src.")]:
            del sys.modules[k]
        sys.modules.update(saved)
