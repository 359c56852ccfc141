#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: records what the reference's own ModelHelper and PotentialLossNoPred compute on this
package's layer classes once mhaq_amd.compat.install() has redirected the reference's imports to them, as a data
fixture: tests/golden/compat_cases.npz.  tests/test_compat_with_reference_cpu.py checks the package against it
without the reference being present.

The reference's modules are imported unchanged from a checkout of the reference project (the directory that holds
its `src/`), in the order an integration uses: compat.install() first, then the reference's model_helper.py and
gdnsq_loss.py.  Nothing of the reference's source travels: the fixture holds tensors only --
  state__<key>    the toy net's state_dict (a seeded initialisation of mhaq_amd layers)
  ref_vals__<i>   ModelHelper.get_model_values(net, PER_CHANNEL): log_act_s, log_act_q, log_wght_s, log_wght_q
  loss            PotentialLossNoPred(None, p=1, a=4, w=4) with t=0.5, loss_sum=1, cnt=1 over (2 * 1.0, *ref_vals)
  grad__<name>    the gradient that loss leaves on each parameter of the net (zeros where it leaves none)

Usage:  python oracle/gen_compat_fixture.py --reference DIR  [--out tests/golden/compat_cases.npz]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

A_BITS, W_BITS, T, LOSS_SUM, CNT, BASE = 4, 4, 0.5, 1.0, 1, 2.0


def toy_net(qscheme):
    """The two-quantizer-pair net of the compat test, seeded (the test loads the recorded state on top)."""
    import mhaq_amd
    torch.manual_seed(0)
    return torch.nn.Sequential(
        mhaq_amd.NoisyAct(signed=True),
        mhaq_amd.NoisyConv2d(3, 6, 3, qscheme=qscheme, qnmethod=mhaq_amd.QNMethod.LSQ),
        torch.nn.ReLU(),
        mhaq_amd.NoisyAct(signed=False),
        mhaq_amd.NoisyConv2d(6, 4, 3, qscheme=qscheme, qnmethod=mhaq_amd.QNMethod.LSQ))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (the directory holding src/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "compat_cases.npz"))
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    sys.dont_write_bytecode = True            # leave no __pycache__ in the reference tree
    sys.path.insert(0, ref)
    import src  # noqa: F401  (empty package)
    pkg = types.ModuleType("src.quantization")
    pkg.__path__ = [os.path.join(ref, "src/quantization")]
    sys.modules["src.quantization"] = pkg
    from mhaq_amd import compat
    compat.install()
    from src.quantization.gdnsq.utils.model_helper import ModelHelper      # the reference's file, unchanged
    from src.quantization.gdnsq.gdnsq_loss import PotentialLossNoPred      # the reference's file, unchanged
    from src.aux.types import QScheme as RefQScheme

    net = toy_net(RefQScheme.PER_CHANNEL)
    data = {f"state__{k}": v.detach().to(torch.float32).numpy().copy() for k, v in net.state_dict().items()}
    ref_vals = ModelHelper.get_model_values(net, RefQScheme.PER_CHANNEL)
    data.update({f"ref_vals__{i}": v.detach().numpy().copy() for i, v in enumerate(ref_vals)})
    crit = PotentialLossNoPred(None, p=1, a=A_BITS, w=W_BITS)
    crit.t, crit.loss_sum, crit.cnt = T, torch.tensor(LOSS_SUM), CNT
    loss = crit((torch.tensor(BASE, requires_grad=True) * 1.0, *ref_vals))
    loss.backward()
    data["loss"] = loss.detach().numpy().copy()
    for name, p in net.named_parameters():
        data[f"grad__{name}"] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
    np.savez_compressed(args.out, **data)
    print(f"{args.out}: {len(data)} arrays, loss {float(loss.detach()):.9g}, {os.path.getsize(args.out)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
