"""CPU: everything about the one-pass RAdam (mhaq_fq_radam_step, mhaq_amd/optim.py: FusedRAdam) that needs no GPU -- the
symbols, the arithmetic contract restated with torch CPU ops against torch.optim.RAdam(foreach=True), the host scalars, the
switches, the routing of every fallback condition, and the state_dict round trip.  The kernel's bits are held to torch's on
the device by tests/test_gpu_fused_radam.py."""
import copy
import ctypes
import dataclasses
import os
import re

import pytest
import torch

from mhaq_amd import _lib, optim
from mhaq_amd.qat import QATConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


# ---------------------------------------------------------------------------------------------- symbols
def test_symbols_are_declared_exported_and_bound_with_the_headers_arity():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    L = _lib.lib()
    for name in ("mhaq_fq_radam_step", "mhaq_fq_radam_chunk_elements"):
        assert name in _lib.header_functions() and name in _lib.SIGNATURES
        assert hasattr(L, name)
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else len(params.split(","))
        assert n == len(_lib.SIGNATURES[name][1])
    # the two table records: 48 and 8 bytes (the binding and the kernel share the header's structs)
    assert re.search(r"float\* p;.*const float\* g;.*float\* m;.*float\* v;.*int64_t n;.*float c1, c2;.*\} mhaq_radam_desc;",
                     src, flags=re.S)
    assert re.search(r"int32_t tensor;.*int32_t chunk;.*\} mhaq_radam_work;", src, flags=re.S)
    assert "optim.hip" in open(os.path.join(ROOT, "mhaq_amd", "csrc", "Makefile")).read()
    binding = open(os.path.join(ROOT, "mhaq_amd", "csrc", "torch_binding.cpp")).read()
    assert 'm.def("radam_step"' in binding and 'm.def("fused_radam_steps"' in binding


def test_argument_errors_come_before_any_launch():
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    chunk = L.mhaq_fq_radam_chunk_elements()
    assert chunk > 0 and chunk % 4 == 0
    f = L.mhaq_fq_radam_step
    assert f(fake, -1, fake, 1, 0.1, 0.999, 0.001, 1e-8, None) == -1
    assert f(fake, 1, fake, -1, 0.1, 0.999, 0.001, 1e-8, None) == -1
    assert f(None, 0, None, 0, 0.1, 0.999, 0.001, 1e-8, None) == 0            # an empty step
    assert f(None, 1, fake, 1, 0.1, 0.999, 0.001, 1e-8, None) == -1
    assert f(fake, 1, None, 1, 0.1, 0.999, 0.001, 1e-8, None) == -1
    assert f(fake, 0, fake, 1, 0.1, 0.999, 0.001, 1e-8, None) == -1
    assert f(fake, 1, fake, 1 << 31, 0.1, 0.999, 0.001, 1e-8, None) == -4
    assert f(odd, 1, fake, 1, 0.1, 0.999, 0.001, 1e-8, None) == -3
    assert f(fake, 1, odd, 1, 0.1, 0.999, 0.001, 1e-8, None) == -3


# ---------------------------------------------------------------------------------------------- arithmetic contract
def _planted(gen, shape, step):
    g = torch.randn(shape, generator=gen) * (10.0 ** float(torch.randint(-12, 7, (1,), generator=gen)))
    flat = g.view(-1)
    if flat.numel() >= 8:
        flat[:8] = torch.tensor([0.0, -0.0, 1e-41, float("inf"), float("-inf"), float("nan"), 1e-12, 1e6])
    if step == 3:
        g.zero_()
    return g


def _chain(p, g, m, v, c1, c2):
    """The contract's op chain (include/mhaq_fq.h) with torch CPU ops: every line one op, rounded once."""
    m.lerp_(g, 1 - BETA1)
    v.mul_(BETA2)
    v.addcmul_(g, g, value=1 - BETA2)
    b = v.sqrt()
    b.add_(EPS)
    b.div_(c2)
    b.reciprocal_()
    b.add_(c1)
    p.addcmul_(m, b)


def test_op_chain_and_host_scalars_equal_torch_foreach_radam_bit_for_bit_over_nine_steps(monkeypatch):
    gen = torch.Generator().manual_seed(7)
    shapes = [(1,), (5,), (64,), (8, 4, 3, 3), (1023,)]
    ps = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    opt = torch.optim.RAdam(ps, lr=3e-3, betas=(BETA1, BETA2), eps=EPS, foreach=True)
    mine = [(p.detach().clone(), torch.zeros(s), torch.zeros(s)) for p, s in zip(ps, shapes)]
    # torch's own scalar lists, as _multi_tensor_radam hands them to its foreach ops
    seen = {}
    real_div, real_add = torch._foreach_div_, torch._foreach_add_
    monkeypatch.setattr(torch, "_foreach_div_", lambda a, b: (seen.__setitem__("c2", list(b)), real_div(a, b))[1])

    def add(a, b, **kw):
        if isinstance(b, list):
            seen["c1"] = list(b)
        return real_add(a, b, **kw)
    monkeypatch.setattr(torch, "_foreach_add_", add)
    for step in range(1, 10):
        lr = [3e-3, 0.0, 1e-3, 3e-3, 2e-3, 0.0, 3e-3, 4e-3, 1e-4][step - 1]     # a schedule moves it between steps
        opt.param_groups[0]["lr"] = lr
        grads = [_planted(gen, s, step) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        c1, c2 = optim.radam_scalars(float(step), lr, BETA1, BETA2)
        assert seen["c1"] == [c1] * len(ps) and seen["c2"] == [c2] * len(ps)
        assert [str(x) for x in seen["c2"]] == [str(c2)] * len(ps)             # -0.0 is -0.0, not 0.0
        assert (str(c2) == "-0.0") == (step <= 5 or lr == 0.0)                     # rho_t > 5 from step 6 on
        for (p, m, v), g, ref in zip(mine, grads, ps):
            _chain(p, g, m, v, c1, c2)
            st = opt.state[ref]
            for a, b in ((p, ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), step


# ---------------------------------------------------------------------------------------------- switches
def test_switches_and_their_defaults(monkeypatch):
    fields = {f.name: f for f in dataclasses.fields(QATConfig)}
    assert fields["fused_optimizer"].default is True
    monkeypatch.delenv(optim.ENV_SWITCH, raising=False)
    assert optim.ENV_SWITCH == "MHAQ_FUSED_RADAM"
    assert optim.enabled(True) is True and optim.enabled(False) is False
    for v, want in (("1", True), ("true", True), ("on", True), ("0", False), ("off", False), ("no", False)):
        monkeypatch.setenv(optim.ENV_SWITCH, v)
        assert optim.enabled(True) is want and optim.enabled(False) is want      # when set, the environment decides
    monkeypatch.setenv(optim.ENV_SWITCH, " ")
    assert optim.enabled(True) is True and optim.enabled(False) is False
    src = open(os.path.join(ROOT, "mhaq_amd", "qat.py")).read()
    assert "optimizer_factory is None and self.device.type == \"cuda\"" in src      # factories are never replaced


# ---------------------------------------------------------------------------------------------- routing
def _group(**kw):
    g = dict(lr=1e-3, weight_decay=0, maximize=False, capturable=False, differentiable=False)
    g.update(kw)
    return g


def test_group_conditions():
    assert optim.group_fallback_reason(_group()) is None
    assert optim.group_fallback_reason(_group(lr=0.0)) is None
    assert optim.group_fallback_reason(_group(weight_decay=1e-4)) == "weight_decay"
    assert optim.group_fallback_reason(_group(maximize=True)) == "maximize"
    assert optim.group_fallback_reason(_group(capturable=True)) == "capturable"
    assert optim.group_fallback_reason(_group(differentiable=True)) == "differentiable"
    assert optim.group_fallback_reason(_group(lr=torch.tensor(1e-3))) == "lr"
    assert optim.group_fallback_reason(_group(lr=1)) == "lr"


def test_tensor_conditions_on_cpu_tensors():
    why = lambda *ts: optim.tensor_fallback_reason(*ts, require_gpu=False)      # noqa: E731
    z = lambda *s: torch.zeros(*s)                                              # noqa: E731
    assert why(z(7), z(7), z(7), z(7)) is None
    assert why(z(0), z(0), z(0), z(0)) is None
    assert optim.tensor_fallback_reason(z(7), z(7), z(7), z(7)) == "device"     # a CPU tensor never takes the launch
    assert why(z(7).double(), z(7).double(), z(7).double(), z(7).double()) == "dtype"
    assert why(z(7), z(7).half(), z(7), z(7)) == "dtype"
    assert why(z(7), z(7), z(7).to("meta"), z(7)) == "device"
    assert why(z(7), z(7).to_sparse(), z(7), z(7)) == "layout"
    cl = lambda: z(8, 4, 3, 3).contiguous(memory_format=torch.channels_last)    # noqa: E731
    assert why(cl(), cl(), cl(), cl()) is None
    assert why(cl(), z(8, 4, 3, 3), cl(), cl()) == "order"                      # the gradient arrived contiguous
    assert why(cl(), cl(), cl(), z(8, 4, 3, 3)) == "order"
    # [Co, Ci, 1, 1]: one memory order under both stride spellings
    a, b = z(8, 4, 1, 1), z(8, 4, 1, 1).as_strided((8, 4, 1, 1), (4, 1, 4, 4))
    assert a.stride() != b.stride() and why(a, b, a, b) is None
    # strided, overlapping and transposed views
    assert why(z(14)[::2], z(14)[::2], z(14)[::2], z(14)[::2]) == "dense"
    e = z(1).expand(7)
    assert why(e, e, e, e) == "dense"
    t = lambda: z(4, 6).t()                                                     # noqa: E731
    assert why(t(), t(), t(), t()) is None                                      # dense in its own order
    assert why(t(), z(6, 4), t(), t()) == "order"
    assert why(z(9)[1:], z(8), z(8), z(8)) is None                              # an offset view is still dense
    assert why(z(7), z(8), z(7), z(7)) == "order"


def _run(opt_class, steps=7, **kw):
    gen = torch.Generator().manual_seed(3)
    ps = [torch.randn(s, generator=gen).requires_grad_(True) for s in [(5,), (3, 4), (2, 3, 1, 1)]]
    opt = opt_class(ps, lr=2e-3, **kw)
    for step in range(steps):
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and step % 3 == 1) else torch.randn(p.shape, generator=gen)
        opt.step()
    return ps, opt


@pytest.mark.parametrize("kw", [dict(), dict(weight_decay=1e-2), dict(maximize=True),
                                dict(weight_decay=1e-2, decoupled_weight_decay=True)])
def test_cpu_parameters_route_to_the_parent_class_and_keep_its_bits(kw):
    before = optim.fused_radam_fallbacks()
    ps, opt = _run(optim.FusedRAdam, **kw)
    assert optim.fused_radam_fallbacks() - before == 7 * 3 - 2      # every update that had a gradient was counted
    ref, ref_opt = _run(torch.optim.RAdam, foreach=True, **kw)
    for a, b in zip(ps, ref):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[a][k], ref_opt.state[b][k])
    assert float(opt.state[ps[1]]["step"]) == 5.0 and float(opt.state[ps[0]]["step"]) == 7.0      # a lagging step count


def test_state_dict_round_trips_with_torch_radam_in_both_directions():
    ps, fused = _run(optim.FusedRAdam, steps=3)
    ref_ps, ref = _run(torch.optim.RAdam, steps=3, foreach=True)
    sd_f, sd_r = fused.state_dict(), ref.state_dict()
    assert sd_f["state"].keys() == sd_r["state"].keys()
    for k in sd_f["state"]:
        assert sd_f["state"][k].keys() == sd_r["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        assert not sd_f["state"][k]["step"].is_cuda
    assert {k: v for k, v in sd_f["param_groups"][0].items() if k != "foreach"} == \
           {k: v for k, v in sd_r["param_groups"][0].items() if k != "foreach"}
    # torch -> fused and fused -> torch, then four more steps on both sides
    gen = torch.Generator().manual_seed(11)
    a_ps = [p.detach().clone().requires_grad_(True) for p in ps]
    b_ps = [p.detach().clone().requires_grad_(True) for p in ps]
    a = optim.FusedRAdam(a_ps, lr=1.0)
    a.load_state_dict(copy.deepcopy(sd_r))
    b = torch.optim.RAdam(b_ps, lr=1.0)
    sd = copy.deepcopy(sd_f)
    sd["param_groups"][0]["foreach"] = True
    b.load_state_dict(sd)
    assert a.param_groups[0]["lr"] == b.param_groups[0]["lr"] == 2e-3
    for _ in range(4):
        for x, y in zip(a_ps, b_ps):
            x.grad = torch.randn(x.shape, generator=gen)
            y.grad = x.grad.clone()
        a.step()
        b.step()
    for x, y in zip(a_ps, b_ps):
        assert torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))
        assert float(a.state[x]["step"]) == float(b.state[y]["step"])
