"""CPU: everything about the one-pass RAdam (mhaq_fq_radam_step, mhaq_amd/optim.py: FusedRAdam) that needs no GPU -- the
symbols, the arithmetic contract restated with torch CPU ops against torch.optim.RAdam(foreach=True), the host scalars, the
switches, the routing of every fallback condition, and the state_dict round trip.  The kernel's bits are held to torch's on
the device by tests/test_gpu_fused_radam.py."""
import copy
import ctypes
import dataclasses
import os
import re
import struct

import pytest
import torch

from mhaq_amd import _lib, optim
from mhaq_amd.qat import QATConfig
from tests import radam_ref as R

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


def _chain(p, g, m, v, c1, c2, beta1=BETA1, beta2=BETA2, eps=EPS):
    """The contract's op chain (include/mhaq_fq.h) with torch CPU ops: every line one op, rounded once.  lerp_ takes its
    second branch, g - (g - m) (1 - w), when float(1 - beta1) >= 0.5."""
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2)
    v.addcmul_(g, g, value=1 - beta2)
    b = v.sqrt()
    b.add_(eps)
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


def _intercept_scalar_lists(monkeypatch):
    """-> seen: {"c1", "c2"} refilled at every step with torch's own scalar lists, as _multi_tensor_radam hands them to
    _foreach_add_ (unrect_step_size) and _foreach_div_ (bias_correction2)."""
    seen = {}
    real_div, real_add = torch._foreach_div_, torch._foreach_add_
    monkeypatch.setattr(torch, "_foreach_div_", lambda a, b: (seen.__setitem__("c2", list(b)), real_div(a, b))[1])

    def add(a, b, **kw):
        if isinstance(b, list):
            seen["c1"] = list(b)
        return real_add(a, b, **kw)
    monkeypatch.setattr(torch, "_foreach_add_", add)
    return seen


def _double_bits(xs):
    return [struct.pack("<d", float(x)) for x in xs]          # value AND sign of zero


@pytest.mark.parametrize("eps", R.EPSS, ids=lambda e: f"eps={e!r}")
@pytest.mark.parametrize("betas", R.BETAS, ids=R.case_id)
def test_op_chain_equals_torch_foreach_radam_over_the_betas_and_eps_matrix(betas, eps, monkeypatch):
    """The restatement the kernel follows, at both branches of lerp_ (float(1 - beta1) < 0.5 and >= 0.5, 0.5 +- 1e-10
    included), rectified from step 6 (beta2 0.999 / 0.99 / 0.9) and never (0.5 / 0.0), eps 1e-8 / 1e-3 / 0.  With eps = 0 the
    elements whose gradient history is all zero are 0 / -0.0 = NaN: NaN at the same elements with the same bits."""
    beta1, beta2 = betas
    gen = torch.Generator().manual_seed(7)
    shapes = [(1,), (5,), (64,), (8, 4, 3, 3), (1023,)]
    ps = [torch.randn(s, generator=gen).requires_grad_(True) for s in shapes]
    opt = torch.optim.RAdam(ps, lr=3e-3, betas=betas, eps=eps, foreach=True)
    mine = [(p.detach().clone(), torch.zeros(s), torch.zeros(s)) for p, s in zip(ps, shapes)]
    seen = _intercept_scalar_lists(monkeypatch)
    rect0 = R.first_rectified_step(beta2)
    assert rect0 == (6 if beta2 in (0.999, 0.99, 0.9) else None)
    saw_nan = False
    for step in range(1, 10):
        lr = R.LRS[step - 1]
        opt.param_groups[0]["lr"] = lr
        grads = [_planted(gen, s, step) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        c1, c2 = optim.radam_scalars(float(step), lr, beta1, beta2)
        assert _double_bits(seen["c1"]) == _double_bits([c1] * len(ps))
        assert _double_bits(seen["c2"]) == _double_bits([c2] * len(ps))
        assert (str(c2) == "-0.0") == (rect0 is None or step < rect0 or lr == 0.0)
        for (p, m, v), g, ref in zip(mine, grads, ps):
            _chain(p, g, m, v, c1, c2, beta1, beta2, eps)
            st = opt.state[ref]
            for a, b in ((p, ref.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), step
        saw_nan = saw_nan or bool(torch.isnan(mine[-1][0].view(-1)[:3]).all())
    # element 0, 1 and 2 of the planted tensor: gradient 0.0, -0.0 and a subnormal whose square is 0 at every step
    assert saw_nan == (eps == 0.0)


PLANTED_COUNTS = [6, 7, 100, 10 ** 4, 10 ** 6]


@pytest.mark.parametrize("betas", [R.DEFAULT_BETAS] + R.BETAS, ids=R.case_id)
def test_host_scalars_equal_torchs_lists_at_step_counts_planted_through_load_state_dict(betas, monkeypatch):
    """A run resumed from a checkpoint: tensor i steps at PLANTED_COUNTS[i], + 1 and + 2 (the middle one at lr = 0)."""
    beta1, beta2 = betas
    ps = [torch.ones(3).requires_grad_(True) for _ in PLANTED_COUNTS]
    opt = torch.optim.RAdam(ps, lr=3e-3, betas=betas, foreach=True)
    for p in ps:
        p.grad = torch.ones(3)
    opt.step()
    sd = opt.state_dict()
    for i, k in enumerate(PLANTED_COUNTS):
        sd["state"][i]["step"] = torch.tensor(float(k - 1))
    opt.load_state_dict(sd)
    seen = _intercept_scalar_lists(monkeypatch)
    for ahead, lr in enumerate([3e-3, 0.0, 1e-3]):
        opt.param_groups[0]["lr"] = lr
        opt.step()
        counts = [float(k + ahead) for k in PLANTED_COUNTS]
        assert [float(opt.state[p]["step"]) for p in ps] == counts
        mine = [optim.radam_scalars(k, lr, beta1, beta2) for k in counts]
        assert _double_bits(seen["c1"]) == _double_bits([c[0] for c in mine]), (ahead, seen["c1"], mine)
        assert _double_bits(seen["c2"]) == _double_bits([c[1] for c in mine]), (ahead, seen["c2"], mine)
        if lr == 0.0:
            assert all(str(x) == "-0.0" for c in mine for x in c)
        elif R.first_rectified_step(beta2) == 6:
            assert all(str(c[0]) == "-0.0" and c[1] < 0 for c in mine)           # every planted count is rectified
        else:
            assert all(c[0] < 0 and str(c[1]) == "-0.0" for c in mine)


# ---------------------------------------------------------------------------------------------- the float64 oracle
def test_the_float64_oracle_has_the_algorithms_closed_forms():
    """radam_ref against what the algorithm gives by hand, independent of any op chain: step 1 from a zero state is
    p - lr g (m_hat = g, rho_1 <= 5); at t -> inf (beta^t = 0, rho_t = rho_inf, r = 1) it is p - lr m / (sqrt(v) + eps)."""
    gen = torch.Generator().manual_seed(5)
    for beta1, beta2 in [R.DEFAULT_BETAS] + R.BETAS:
        p0, g = torch.randn(33, generator=gen, dtype=torch.float64), torch.randn(33, generator=gen, dtype=torch.float64)
        p, m, v = p0.clone(), torch.zeros(33, dtype=torch.float64), torch.zeros(33, dtype=torch.float64)
        R.radam_ref([p], [g], [m], [v], [1], 3e-3, beta1, beta2, 1e-8)
        assert torch.allclose(p, p0 - 3e-3 * g, rtol=1e-13, atol=1e-15)
        assert torch.allclose(m, (1 - beta1) * g, rtol=1e-13, atol=0) and torch.allclose(v, (1 - beta2) * g * g, rtol=1e-13, atol=0)
        m0, v0 = torch.randn(33, generator=gen, dtype=torch.float64), torch.rand(33, generator=gen, dtype=torch.float64)
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        R.radam_ref([p], [g], [m], [v], [10 ** 6], 3e-3, beta1, beta2, 1e-3)
        m1, v1 = beta1 * m0 + (1 - beta1) * g, beta2 * v0 + (1 - beta2) * g * g
        assert beta1 ** (10 ** 6) == 0.0 and beta2 ** (10 ** 6) == 0.0
        rectified = 2 / (1 - beta2) - 1 > 5                           # rho_inf; <= 3 for beta2 0.5 and 0.0: m_hat = m alone
        assert rectified == (R.first_rectified_step(beta2) is not None)
        want = p0 - 3e-3 * m1 / (v1.sqrt() + 1e-3) if rectified else p0 - 3e-3 * m1
        assert torch.allclose(p, want, rtol=1e-12, atol=1e-15), (beta1, beta2)
        assert torch.allclose(m, m1, rtol=1e-13, atol=1e-16) and torch.allclose(v, v1, rtol=1e-13, atol=1e-16)


def _oracle_case_on_cpu(betas, mutate=None):
    """-> ((p, m, v) fp32 of torch's CPU foreach RAdam, (p, m, v) of the op-chain restatement [mutated], (p, m, v) float64
    oracle, lr per element): every step's values of every tensor, concatenated."""
    beta1, beta2 = betas
    p0, grads, lrs = R.oracle_inputs()
    ps = [p.clone().requires_grad_(True) for p in p0]
    opt = torch.optim.RAdam(ps, lr=lrs[0], betas=betas, eps=R.ORACLE_EPS, foreach=True)
    mine = [(p.clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in p0]
    ref = [[p.double() for p in p0], [torch.zeros_like(p, dtype=torch.float64) for p in p0],
           [torch.zeros_like(p, dtype=torch.float64) for p in p0]]
    rec_t, rec_c, rec_r, rec_lr = [], [], [], []
    for step, (gs, lr) in enumerate(zip(grads, lrs), 1):
        opt.param_groups[0]["lr"] = lr
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.step()
        skip = mutate == "missed_step" and step == 4
        c1, c2 = optim.radam_scalars(float(step), lr * (1.001 if mutate == "lr_coefficient" else 1.0), beta1, beta2)
        for (p, m, v), g in zip(mine, gs):
            if not skip:
                _chain(p, g, m, v, c1, c2, beta1, beta2, R.ORACLE_EPS)
        R.radam_ref(ref[0], [g.double() for g in gs], ref[1], ref[2], [step] * len(gs), lr, beta1, beta2, R.ORACLE_EPS)
        rec_t.append([torch.cat([p.detach().reshape(-1) for p in ps])] +
                     [torch.cat([opt.state[p][k].reshape(-1) for p in ps]) for k in ("exp_avg", "exp_avg_sq")])
        rec_c.append([torch.cat([x[j].reshape(-1) for x in mine]) for j in range(3)])
        rec_r.append([torch.cat([x.reshape(-1) for x in ref[j]]) for j in range(3)])
        rec_lr.append(torch.full_like(rec_r[-1][0], lr))
    join = lambda rec: tuple(torch.cat([r[j] for r in rec]) for j in range(3))      # noqa: E731
    return join(rec_t), join(rec_c), join(rec_r), torch.cat(rec_lr)


@pytest.mark.parametrize("betas", [R.DEFAULT_BETAS] + R.BETAS, ids=R.case_id)
def test_the_float64_oracle_against_torch_cpu_foreach_radam_by_the_2x_rule(betas):
    """The yardstick of the GPU oracle test, run without a GPU: the op-chain restatement (torch's bits) passes it, and the
    rule has teeth -- a learning-rate coefficient off by 0.1 % and one missed step both fail it."""
    torch_run, chain_run, ref, lr = _oracle_case_on_cpu(betas)
    ok, errs = R.within_twice((chain_run, ref), (torch_run, ref), lr)
    assert ok, errs
    # the second moment is a sum of non-negative terms, so its relative error has a bound of its own: per step the fp32
    # casts of beta2 and 1 - beta2 and at most four roundings (v beta2, g g, w2 (g g), the sum), 2^-24 each, not amplified
    assert errs["exp_avg_sq"][1] <= 6 * len(R.ORACLE_LRS) * 2.0 ** -24, errs
    # (exp_avg and p have none: g - m cancels, and the relative error of a cancelled value is unbounded)
    for mutant in ("lr_coefficient", "missed_step"):
        _, bad_run, _, _ = _oracle_case_on_cpu(betas, mutate=mutant)
        ok, errs = R.within_twice((bad_run, ref), (torch_run, ref), lr)
        assert not ok, (mutant, errs)


# ---------------------------------------------------------------------------------------------- slabs and guard bands
@pytest.mark.parametrize("case", list(R.ALIGN_CASES))
def test_banded_slabs_with_a_planted_state_are_accepted_by_both_classes_and_take_the_launch(case):
    """The construction of the GPU guard-band test on the CPU: both classes step the planted state on the offset views and
    leave it there, neither writes a band or the gradient slab, and every layout passes the fused launch's tensor rule."""
    runs = []
    for cls, kw in ((torch.optim.RAdam, dict(foreach=True)), (optim.FusedRAdam, {})):
        opt, ps, streams = R.banded_optimizer(cls, case, "cpu", **kw)
        gen = torch.Generator().manual_seed(22)
        for i, (p, s) in enumerate(zip(ps, streams)):
            off = R.ALIGN_CASES[case](i)
            assert tuple(s[k].view.data_ptr() % 16 for k in "pgmv") == tuple(4 * o for o in off)
            assert optim.tensor_fallback_reason(p, p.grad, s["m"].view, s["v"].view, require_gpu=False) is None, (case, i)
        for step in range(1, 4):
            for s in streams:
                s["g"].view.copy_(R.planted_gradient(gen, s["g"].n, plant=True))
            before = [s["g"].bits() for s in streams]
            opt.step()
            for i, (p, s) in enumerate(zip(ps, streams)):
                assert all(s[k].bands_intact() for k in "pgmv"), (case, step, i)
                assert torch.equal(s["g"].bits(), before[i])
                st = opt.state[p]
                assert float(st["step"]) == step and not st["step"].is_cuda
                assert st["exp_avg"].data_ptr() == s["m"].view.data_ptr() and st["exp_avg_sq"].data_ptr() == s["v"].view.data_ptr()
        assert any(bool(s["m"].view.ne(0).any()) for s in streams)                  # the planted moments were stepped
        runs.append([torch.cat([s[k].bits() for k in "pmv"]) for s in streams])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_the_alignment_cases_cover_every_listed_offset():
    n = len(R.BAND_SIZES)
    offs = {c: {f(i) for i in range(n)} for c, f in R.ALIGN_CASES.items()}
    assert offs["all_aligned"] == {(0, 0, 0, 0)}
    assert [offs[f"all_plus{k}_byte{4 * k}"] for k in (1, 2, 3)] == [{(k,) * 4} for k in (1, 2, 3)]
    for c, j in (("only_p_misaligned", 0), ("only_g_misaligned", 1), ("only_exp_avg_misaligned", 2)):
        assert {o[j] for o in offs[c]} == {1, 2, 3}                                  # byte offsets 4, 8 and 12
        assert all(o[k] == 0 for o in offs[c] for k in range(4) if k != j)
    C = R.CHUNK
    assert R.BAND_SIZES == [1, 3, 4, 5, 1020, 1023, 1024, 1028, 4092, 4095, C, C + 1, C + 4, 2 * C, 2 * C + 3]
    assert C == _lib.lib().mhaq_fq_radam_chunk_elements() and R.BAND >= 64


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
