"""CPU: the case builder of the fused ReLU / add activation tests (tests/fused_act_cases.py) does what the GPU tests
rely on -- so that none of their comparisons is ever skipped for want of a finite reference or a populated region."""
import math

import pytest
import torch

from tests import fused_act_cases as C


@pytest.mark.parametrize("pset", list(C.PARAM_SETS))
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
def test_finite_family_gives_finite_gradients_and_yardsticks_at_every_size(pset, with_add):
    for n in C.SIZES:
        case = C.build(n, pset, with_add, "finite")
        for t in (case.z, case.gy, case.ga) + ((case.addend,) if with_add else ()):
            assert t.shape == (n,) and t.dtype == torch.float32 and bool(torch.isfinite(t).all())
        for method in C.METHODS:
            o = C.oracle(case, method, seed=11, offset=3)
            assert bool(torch.isfinite(o["y"]).all()) and bool(torch.isfinite(o["gx"]).all())
            for g in o["grads"]:
                assert math.isfinite(float(g)), (n, method, float(g))
            cf = C.closed_form(case, o["a"], o["r"], method)
            abs_g, abs_s = float(cf["abs_g"]), float(cf["abs_s"])
            assert math.isfinite(abs_g) and math.isfinite(abs_s) and abs_g > 0, (n, method, abs_g, abs_s)
            if n >= 64:
                assert abs_s > 0, (n, method)
            assert all(math.isfinite(b) and b > 0 for b in C.yardsticks(case, o["a"], o["r"], method))


@pytest.mark.parametrize("pset", list(C.PARAM_SETS))
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("family", ["finite", "special"])
def test_every_region_is_populated_from_64_elements_up(pset, with_add, family):
    q = C.quantizer(pset)
    for n in [64] + [n for n in C.SIZES if n >= 64]:
        reg = C.regions(C.build(n, pset, with_add, family))
        assert reg["a_zero"] and reg["z_neg"] and reg["above_hi"] and reg["bound"], (n, reg)
        if q.lo < q.hi:                      # inverted bounds: every element clamps to hi, nothing is inside
            assert reg["tie"] and reg["inside"], (n, reg)


def test_planted_values_reach_the_head_and_the_tail():
    """Planted slots land on every residue mod 4 (odd stride), and the tiny sizes of the special family start at the
    special slots."""
    case = C.build(4099, "holds_zero", True, "special")
    planted = torch.isnan(case.gy) | torch.isnan(case.ga) | torch.isnan(case.z)
    idx = planted.nonzero().flatten()
    assert {int(i) % 4 for i in idx} == {0, 1, 2, 3}
    assert int(idx.min()) < 64 and int(idx.max()) > 4000
    for family in ("finite", "special"):
        for n in C.SIZES:
            slot = C.build(n, "holds_zero", True, family).slot
            assert int(slot[0]) >= 0                                  # the head ...
            if n % 4:
                assert bool((slot[n - n % 4:] >= 0).any()), (family, n)       # ... and the n % 4 tail
            if n >= 64:
                assert bool((slot[4:n - n % 4] >= 0).any()) and bool((slot < 0).any())
    assert math.isnan(float(C.build(1, "holds_zero", False, "special").z[0]))
    small = C.build(7, "unsigned", True, "special")
    assert bool(torch.isinf(small.z).any()) and bool(torch.isnan(small.gy).any())
    assert float(small.z[3]) == math.inf and float(small.addend[3]) == -math.inf


def test_the_oracle_has_torch_relu_and_threshold_backward_semantics():
    """What the kernels' header promises is what the eager chain does on the CPU: relu(NaN) is NaN and passes its
    gradient, inf + (-inf) is NaN, a NaN gradient under z < 0 is masked to 0."""
    case = C.build(4099, "unsigned", True, "special")
    o = C.oracle(case, "LSQ", use_gy=False, use_ga=True)             # a only: gx = threshold_backward(g_a, a)
    z, ad, a, gx = case.z, case.addend, o["a"], o["gx"]
    assert bool(torch.isnan(a[torch.isnan(z)]).all())
    both = (z == math.inf) & (ad == -math.inf)
    assert bool(both.any()) and bool(torch.isnan(a[both]).all())
    nan_a = torch.isnan(a) & ~torch.isnan(case.ga)
    assert bool(nan_a.any()) and bool((gx[nan_a] == case.ga[nan_a]).all())
    masked = torch.isnan(case.ga) & (z + ad <= 0)
    assert bool(masked.any()) and bool((gx[masked] == 0).all())
    assert all(float(g) == 0 for g in o["grads"])


def test_the_pinned_scale_is_the_all_ones_significand():
    q = C.quantizer("all_ones")
    assert q.s_t.view(torch.int32).item() == C.S_ALL_ONES_BITS and q.lo < 0 < q.hi
    inv = C.quantizer("inverted")
    assert inv.hi < inv.lo
    assert set(C.FORWARD_SETS) == set(C.PARAM_SETS) - {"all_ones"}
