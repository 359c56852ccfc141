"""CPU: the checker of the PotentialLoss GPU tests (tests/potential_ref.py) checked against the eager oracle
(oracle/fq_eager.potential_loss, oracle/loss.py), float64 autograd through it and the reference-recorded model cases.
No kernel is involved."""
import math

import numpy as np
import pytest
import torch

from oracle import fq_eager as O
from tests import potential_ref as R
from tests.golden_util import load_cases, max_ulp

MODEL = load_cases("model_cases.npz")
f32 = lambda v: float(np.float32(v))        # noqa: E731
STATE = (f32(3.3), 3.0, f32(0.35))
BITS = [(8, 4), (3, 6), (4, 4)]


def _tied(na, nw, a_bits, w_bits, seed):
    las, laq, lws, lwq = R.make_inputs(na, nw, a_bits, w_bits, seed)
    R.plant_tie(lws, lwq, w_bits, slice(1, None, 5))
    R.plant_tie(las, laq, a_bits, slice(2, None, 4))
    return las, laq, lws, lwq


@pytest.mark.parametrize("a_bits,w_bits", BITS)
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("lossless", [False, True])
def test_ref64_rounds_to_the_eager_oracle_within_2_ulp(a_bits, w_bits, p, lossless):
    vecs = R.make_inputs(21, 37, a_bits, w_bits, seed=10 * a_bits + w_bits + p)
    base = torch.tensor(1.7)
    ref = R.ref64(base, *vecs, a_bits, w_bits, STATE, p, lossless)
    assert 0 < ref.wact < 37 and 0 < ref.aact < 21                    # both sides have active and inactive hinges
    ploss, rloss = O.potential_loss(base * 1.0, *vecs, a_bits, w_bits, STATE[2], torch.tensor(STATE[0]), int(STATE[1]),
                                    lossless=lossless, p=p)
    assert max_ulp(np.float32(ref.out[0]), ploss.numpy()) <= 2, (ref.out[0], float(ploss))
    assert max_ulp(np.float32(ref.out[3]), rloss.numpy()) <= 2, (ref.out[3], float(rloss))
    # the float32 chain of the bars is that oracle, and its further outputs restate the same float64 quantities
    c32 = R.chain32(base, *vecs, a_bits, w_bits, STATE, p, lossless)
    assert c32.out[0] == float(ploss) and c32.out[3] == float(rloss)
    for k in range(12):
        assert abs(c32.out[k] - ref.out[k]) <= 1e-5 * abs(ref.out[k]) + 1e-9, (R.OUT_NAMES[k], c32.out[k], ref.out[k])
    assert c32.out[11] == ref.out[11]
    assert abs(float(c32.state[0]) - ref.state[0]) <= 1e-6 * ref.state[0] and c32.state[1] == ref.state[1] == 4.0


def test_ref64_tells_the_bit_widths_apart():
    vecs = R.make_inputs(21, 37, 8, 4, seed=5)
    a, b = R.ref64(1.7, *vecs, 8, 4, STATE), R.ref64(1.7, *vecs, 4, 8, STATE)
    assert a.out[0] != b.out[0] and not torch.equal(a.g_lwq, b.g_lwq) and not torch.equal(a.g_laq, b.g_laq)


@pytest.mark.parametrize("name", sorted(MODEL))
def test_ref64_reproduces_the_reference_recorded_model_cases(name):
    c = MODEL[name]
    if name.endswith("nopred"):
        base = torch.tensor(float(c["base"])) * 1.0
    else:
        base = torch.nn.functional.mse_loss(torch.linspace(-1, 1, 12).view(3, 4), torch.linspace(1, -1, 12).view(3, 4) * 0.5)
    vecs = [torch.from_numpy(np.asarray(c[k])) for k in ("las", "laq", "lws", "lwq")]
    state = (f32(c["loss_sum"]), float(c["cnt"]), f32(c["t"]))
    ref = R.ref64(base, *vecs, int(c["a_bits"]), int(c["w_bits"]), state, 1, False)
    assert abs(ref.out[0] - float(c["ploss"])) <= 1e-6 * abs(float(c["ploss"])), (ref.out[0], float(c["ploss"]))


def _autograd64(base, las, laq, lws, lwq, a_bits, w_bits, state, p, lossless, g):
    leaves = [v.double().requires_grad_(True) for v in (las, laq, lws, lwq)]
    bl = torch.tensor(float(base), dtype=torch.float64, requires_grad=True)
    ploss, _ = O.potential_loss(bl * 1.0, *leaves, a_bits, w_bits, state[2], torch.tensor(state[0], dtype=torch.float64),
                                int(state[1]), lossless=lossless, p=p)
    return torch.autograd.grad(ploss * g, [bl] + leaves)


@pytest.mark.parametrize("a_bits,w_bits", BITS)
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("lossless", [False, True])
def test_closed_form_gradients_equal_float64_autograd_through_the_oracle(a_bits, w_bits, p, lossless):
    """On the grid inputs float32 and float64 agree on the sign of every h, so on the active sets.  The oracle's wmul and
    amul are float32 whatever the inputs' type (integer counts + the float32 l_eps), so the two agree to 2^-22 overall; with
    that common factor divided out -- each vector over its own largest element -- they agree to 1e-12."""
    vecs = _tied(21, 37, a_bits, w_bits, seed=7 + p)
    g = 0.375
    ref = R.ref64(f32(1.7), *vecs, a_bits, w_bits, STATE, p, lossless, g)
    gb, g_las, g_laq, g_lws, g_lwq = _autograd64(f32(1.7), *vecs, a_bits, w_bits, STATE, p, lossless, g)
    assert abs(float(gb) - ref.g_base) <= 1e-12 * abs(ref.g_base)
    for name, auto in zip(R.GRAD_NAMES, (g_las, g_laq, g_lws, g_lwq)):
        mine = getattr(ref, name)
        assert float(mine.abs().max()) > 0
        assert float((auto - mine).abs().max()) <= 2.0 ** -22 * float(mine.abs().max()), name
        assert float((auto / auto.abs().max() - mine / mine.abs().max()).abs().max()) <= 1e-12, name
    assert torch.equal(ref.g_lws, -ref.g_lwq) and torch.equal(ref.g_las, -ref.g_laq)
    # the planted ties: half of an active neighbour's g * cw for p = 1, zero for p = 2
    tie_w, tie_a = ref.wh == 0, ref.ah == 0
    assert int(tie_w.sum()) == len(range(1, 37, 5)) and int(tie_a.sum()) == len(range(2, 21, 4))
    want_w, want_a = (0.5 * g * ref.out[4], 0.5 * g * ref.out[5]) if p == 1 else (0.0, 0.0)
    assert bool((ref.g_lwq[tie_w] == want_w).all()) and bool((ref.g_laq[tie_a] == want_a).all())
    assert bool((g_lwq[tie_w] - want_w).abs().max() <= 2.0 ** -22 * abs(g * ref.out[4]))
    if p == 1:
        assert bool((ref.g_lwq[ref.wh > 0] == g * ref.out[4]).all()) and bool((ref.g_lwq[ref.wh < 0] == 0).all())


@pytest.mark.parametrize("p", [1, 2])
def test_ref64_state_sequence_follows_the_oracle_module_over_five_training_steps(p):
    """calib is read before the update: step k uses the sum and the count of the steps before it."""
    from oracle.loss import PotentialLossNoPred
    vecs = R.make_inputs(21, 37, 8, 4, seed=11)
    L = PotentialLossNoPred(None, p=p, a=8, w=4).train()
    L.t = f32(0.35)
    state = (0.0, 1.0, f32(0.35))
    bases = [f32(b) for b in (1.7, 0.9, 2.25, 0.31, 1.1)]
    want_sum, units = 0.0, []
    for k, b in enumerate(bases):
        ref = R.ref64(b, *vecs, 8, 4, state, p, False)
        ploss = L((torch.tensor(b) * 1.0, *vecs))
        assert abs(float(ploss) - ref.out[0]) <= 1e-6 * abs(ref.out[0]), k
        # the hinge part over calib = (sum of the k earlier task losses) / (k + 1) is the same number at every step
        if k == 0:
            assert ref.out[0] == ref.out[3]
        else:
            units.append((ref.out[0] - ref.out[3]) / (want_sum / (k + 1)))
            assert units[-1] > 0 and abs(units[-1] - units[0]) <= 1e-12 * units[0]
        want_sum += b ** p
        state = ref.state
        assert state[1] == L.cnt == k + 2
        assert abs(state[0] - want_sum) <= 1e-12 and abs(float(L.loss_sum) - state[0]) <= 1e-6 * state[0]
        assert abs(float(L.wloss) - ref.out[1]) <= 1e-6 * ref.out[1] and float(L.weight_reg_loss) == ref.out[11]
    assert R.ref64(bases[0], *vecs, 8, 4, (0.0, 1.0, f32(0.35)), p, False).out[0] == bases[0] ** p      # calib == 0 at step 0


@pytest.mark.parametrize("which", range(4), ids=["las", "laq", "lws", "lwq"])
def test_ref64_propagates_nan_as_the_reference_does(which):
    vecs = list(R.make_inputs(21, 37, 8, 4, seed=13))
    clean = R.ref64(1.7, *vecs, 8, 4, STATE)
    vecs[which] = vecs[which].clone()
    vecs[which][vecs[which].numel() // 2] = math.nan
    ref = R.ref64(1.7, *vecs, 8, 4, STATE)
    ploss, _ = O.potential_loss(torch.tensor(1.7), *vecs, 8, 4, STATE[2], torch.tensor(STATE[0]), int(STATE[1]))
    assert math.isnan(float(ploss)) and math.isnan(ref.out[0])
    weight_side = which >= 2
    nan_out = {0, 1 if weight_side else 2, {0: 9, 1: 10, 2: 7, 3: 8}[which]} | ({11} if weight_side else set())
    for k in range(12):
        if k in nan_out:
            assert math.isnan(ref.out[k]), R.OUT_NAMES[k]
        elif k not in (4, 5):          # the multipliers follow the counts, and a NaN hinge counts as inactive
            assert ref.out[k] == clean.out[k], R.OUT_NAMES[k]
    assert math.isnan(float((vecs[3] - vecs[2]).max())) == weight_side
    assert ref.wact + ref.aact in (clean.wact + clean.aact, clean.wact + clean.aact - 1)
