"""GPU (-m gpu): every cell of the launch plan of the model-wide weight launches (mhaq_fq_wlayer_fwd_multi,
mhaq_fq_wlayer_bwd_group; csrc/fq_pc.hip), on both sides of every threshold, with every row body the cell can hold and
every estimator.  The case table is tests/wmulti_cells.py (what it covers: tests/test_wmulti_cells_cpu.py).

a. every layer of a plan against its own fused op, bit for bit, the sign stream replayed at the layer's element offset;
b. the defining layer -- the one whose row selects the cell -- against the eager oracle, at the bars of
   test_gpu_fused_layers.py::test_per_channel_long_rows_every_code_path;
c. for the cells no earlier test selected: through the C ABI on NaN-filled slabs between guard bands -- nothing outside
   written, everything inside written, and the same bits again on slabs filled with -7."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fq_closed_form as CF  # noqa: E402
from oracle import fq_eager as O  # noqa: E402
from tests import wmulti_cells as WC  # noqa: E402
from tests.aewgs_bound import aewgs_weight_slacks  # noqa: E402
from tests.golden_util import exact_off_extremes  # noqa: E402

DEV = "cuda:0"
SEED = 77
METHOD_VALUE = {"STE": 0, "EWGS": 1, "AEWGS": 2, "LSQ": 3}          # include/mhaq_fq.h
GUARD = 64                                                          # floats before and after every output slab

RUNS = [(c.name, m) for c in WC.CASES for m in WC.estimators(c)]
NEW = [(c.name, m) for c in WC.CASES for m in WC.estimators(c)
       if set(WC.Plan.of(c.layers).cells()) & set(WC.NEW_CELLS)]


class _Desc(ctypes.Structure):          # mhaq_wlayer_desc (include/mhaq_fq.h)
    _fields_ = [("w", ctypes.c_void_p), ("log_s", ctypes.c_void_p), ("G", ctypes.c_void_p), ("g_lwq", ctypes.c_void_p),
                ("co", ctypes.c_int64), ("row", ctypes.c_int64), ("elem_offset", ctypes.c_int64),
                ("chan_offset", ctypes.c_int64)]


def _build(case, method):
    """(net, Gs, hs): weights randn * 0.1 with tied minima and tied maxima planted on one row of every layer, log scales
    from the row spans (test_gpu_fused_layers.py::test_weight_layer_with_fused_regulariser), non-trivial upstream gradients."""
    import mhaq_amd as M
    P = WC.Plan.of(case.layers)
    gen = torch.Generator().manual_seed(P.max_row + 7 * P.total_co)
    mods = []
    for kind, q, shape in case.layers:
        kw = dict(qscheme=M.QScheme.PER_CHANNEL if q == "pc" else M.QScheme.PER_TENSOR, log_s_init=-6,
                  qnmethod=M.QNMethod[method])
        mods.append(M.NoisyConv2d(shape[1], shape[0], shape[2], bias=False, **kw) if kind == "conv"
                    else M.NoisyLinear(shape[1], shape[0], **kw))
    Gs, hs = [], []
    with torch.no_grad():
        for m, (kind, q, shape), co, row in zip(mods, case.layers, P.co, P.row):
            w = torch.randn(co, row, generator=gen) * 0.1
            k = min(1, co - 1)
            w[k, [0, 3]] = w[k].min() - 0.01             # tied minima
            w[k, [1, 2, 5]] = w[k].max() + 0.02          # tied maxima
            span = w.amax(1) - w.amin(1)
            ls = torch.log2(span / 15.0) + 0.2 * torch.randn(co, generator=gen)
            m.weight.copy_(w.reshape(shape))
            m.log_wght_s.copy_(ls.reshape(m.log_wght_s.shape))
            Gs.append(torch.randn(shape, generator=gen))
            hs.append(torch.randn(co, generator=gen))
    net = torch.nn.ModuleList(mods).to(DEV)
    Gs, hs = [g.to(DEV) for g in Gs], [h.to(DEV) for h in hs]
    if case.channels_last:
        net = net.to(memory_format=torch.channels_last)
        Gs = [g.contiguous(memory_format=torch.channels_last) if g.dim() == 4 else g for g in Gs]
    return net, Gs, hs


def _rows(t, co):
    """[co][row] in the order the kernels walk the tensor in (its memory order)."""
    if t.dim() == 4 and not t.is_contiguous():
        t = t.permute(0, 2, 3, 1)
    return t.reshape(co, -1)


@functools.lru_cache(maxsize=None)
def _run(name, method):
    """The model-wide forward and ONE grouped backward of a case: computed once, shared by the checks below."""
    from mhaq_amd import ops
    from mhaq_amd.multi import MultiTensorWeightQuant
    case = WC.CASE[name]
    P = WC.Plan.of(case.layers)
    net, Gs, hs = _build(case, method)
    plan = MultiTensorWeightQuant(net, joint_backward=False, backward_group_elems=1 << 30, long_rows=case.long_rows)
    assert (tuple(plan.co), tuple(plan.row), tuple(plan.elem_off)) == (P.co, P.row, P.elem_off)
    assert (plan.total_co, plan.max_row, plan.nlayers) == (P.total_co, P.max_row, P.nlayers)
    assert plan.per_tensor == [layer[1] == "pt" for layer in case.layers]
    assert [(g.first, g.n, g.max_row, g.co) for g in plan.groups] == [(0, P.nlayers, P.max_row, P.total_co)]
    ops.manual_seed(SEED)
    plan.run()
    outs = []
    for m in net:
        wq, _, _ = m._quantized_weight()
        outs.append((wq, m.regulariser_input()))
    assert plan.groups[0].outs is not None                      # every layer took its slot in the group's node
    loss = sum((wq * G).sum() for (wq, _), G in zip(outs, Gs)) + \
        sum((l.reshape(-1) * h).sum() for (_, l), h in zip(outs, hs))
    loss.backward()                                             # ONE backward launch: stream (SEED, 1)
    got = [(m.weight.grad.clone(), m.log_wght_s.grad.clone()) for m in net]
    outs = [(wq.detach().clone(), lwq.detach().clone()) for wq, lwq in outs]
    s_all = plan.cur_aux[0].clone()
    r_all = ops.fill_r(plan.total_elems, SEED, 1, DEV)
    for m in net:
        m.weight.grad = m.log_wght_s.grad = None
    return dict(case=case, P=P, net=net, Gs=Gs, hs=hs, outs=outs, got=got, r_all=r_all, s_all=s_all)


@pytest.mark.parametrize("name,method", RUNS)
def test_every_layer_of_the_plan_has_the_bits_of_its_own_op(name, method):
    from mhaq_amd import ops
    R = _run(name, method)
    case, P, net = R["case"], R["P"], R["net"]
    f_cell, b_cell = P.cells()
    for i, m in enumerate(net):
        where = (name, method, i, f_cell, b_cell, P.bodies()[i])
        m.weight.grad = m.log_wght_s.grad = None
        n = m.weight.numel()
        r = None if method == "LSQ" else R["r_all"][P.elem_off[i]:P.elem_off[i] + n]
        if case.layers[i][1] == "pt":
            # the layer's own kernels walk a contiguous copy: hand them the signs in that (logical) order
            if r is not None and not m.weight.is_contiguous():
                r = torch.as_strided(r, m.weight.shape, m.weight.stride()).contiguous().reshape(-1)
            wq, zp, s, lwq = ops.fake_quant_weight_layer_pt(m.weight, m.log_wght_s, method, r_sign=r)
        else:
            wq, zp, s, lwq = ops.fake_quant_weight_layer(m.weight, m.log_wght_s, method, r_sign=r)
        assert torch.equal(wq, R["outs"][i][0]), where
        assert torch.equal(lwq.reshape(-1), R["outs"][i][1].reshape(-1)), where
        ((wq * R["Gs"][i]).sum() + (lwq.reshape(-1) * R["hs"][i]).sum()).backward()
        gw, gls = R["got"][i]
        assert torch.equal(m.weight.grad, gw), (where, float((m.weight.grad - gw).abs().max()))
        assert torch.equal(m.log_wght_s.grad, gls), (where, float((m.log_wght_s.grad - gls).abs().max()))
        m.weight.grad = m.log_wght_s.grad = None


@pytest.mark.parametrize("name,method", RUNS)
def test_the_defining_layer_matches_the_eager_oracle(name, method):
    """oracle.fq_eager.weight_fake_quant + the log2(max - min + s) line on the defining layer as [co][row] (a PER_TENSOR layer
    is one row: the same minimum, quantizer and sums), the signs the same fill_r slice as +-0.5."""
    R = _run(name, method)
    case, P = R["case"], R["P"]
    i = case.defining
    co, row, e0 = P.co[i], P.row[i], P.elem_off[i]
    m = R["net"][i]
    w = _rows(m.weight.detach(), co).contiguous()
    G = _rows(R["Gs"][i], co).contiguous()
    h = R["hs"][i]
    r = R["r_all"][e0:e0 + co * row].float().reshape(co, row) * 0.5
    ls0 = m.log_wght_s.detach().reshape(co, 1)
    wr, lsr = w.clone().requires_grad_(True), ls0.clone().requires_grad_(True)
    wq_r, _, _ = O.weight_fake_quant(wr, lsr, True, method, r=r)
    lwq_r = torch.log2(wr.amax(1) - wr.amin(1) + torch.exp2(lsr.ravel()))
    ((wq_r * G).sum() + (lwq_r * h).sum()).backward()
    wq, lwq = _rows(R["outs"][i][0], co), R["outs"][i][1].reshape(-1)
    s = R["s_all"][P.chan_off[i]:P.chan_off[i] + co]
    assert torch.equal(s, torch.exp2(ls0).reshape(-1))
    assert torch.equal(wq, wq_r) and torch.equal(lwq, lwq_r), (name, method, P.cells())
    # reduced gradients within 1e-6 * sum|terms| (AEWGS: + the propagated slack of its group means, tests/aewgs_bound.py),
    # the yardsticks of oracle/fq_closed_form.py plus the regulariser's share t = h / (u ln2)
    cf = CF.per_channel(w.cpu(), G.cpu(), r.cpu(), s.cpu(), method)
    u = (w.amax(1) - w.amin(1) + s).cpu().numpy()
    t = np.abs(h.cpu().numpy()) / (u * math.log(2.0))
    sl_gw, sl_ls = aewgs_weight_slacks(w, G, s, True) if method == "AEWGS" else (0.0, 0.0)
    gw, gw_r = _rows(R["got"][i][0], co).cpu().numpy(), wr.grad.cpu().numpy()
    if method != "AEWGS":
        assert exact_off_extremes(gw, gw_r, w.cpu().numpy(), True, also_max=True), (name, method, P.cells())
    abs_g = (cf["abs_g"].numpy() + 4 * t).reshape(-1, 1)
    assert np.all(np.abs(gw - gw_r) <= 1e-6 * (abs_g + np.abs(gw_r)) + sl_gw), (name, method, P.cells())
    yard = (cf["abs_s"].numpy() + 4 * t) * math.log(2.0) * s.cpu().numpy() * 2
    errs = np.abs(R["got"][i][1].cpu().numpy().reshape(-1) - lsr.grad.cpu().numpy().reshape(-1))
    assert np.all(errs <= 1e-6 * yard + sl_ls + 1e-9), (name, method, float((errs / (yard + 1e-30)).max()))


def _guarded(n, fill):
    return torch.full((n + 2 * GUARD,), fill, device=DEV)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _guards_hold(slab, fill):
    ref = torch.full((GUARD,), fill, device=DEV)
    return _same_bits(slab[:GUARD], ref) and _same_bits(slab[-GUARD:], ref)


@pytest.mark.parametrize("name,method", NEW)
def test_the_new_cells_write_their_slabs_and_nothing_else(name, method):
    """mhaq_fq_wlayer_fwd_multi and mhaq_fq_wlayer_bwd_group (the window form: aux_stride > group_co) called directly: the
    output slabs are NaN-filled between 64-float guard bands -- the guards keep their bits, no element inside keeps a NaN
    -- and a second call on slabs filled with -7 gives the same bits."""
    from mhaq_amd import _lib
    L = _lib.lib()
    case = WC.CASE[name]
    P = WC.Plan.of(case.layers)
    net, Gs, hs = _build(case, method)
    n, st = P.nlayers, torch.cuda.current_stream().cuda_stream
    fwd, bwd = (_Desc * n)(), (_Desc * n)()
    for i, m in enumerate(net):
        fwd[i] = _Desc(m.weight.data_ptr(), m.log_wght_s.data_ptr(), None, None, P.co[i], P.row[i], P.elem_off[i],
                       P.chan_off[i])
        bwd[i] = _Desc(m.weight.data_ptr(), None, Gs[i].data_ptr(), hs[i].data_ptr(), P.co[i], P.row[i], P.elem_off[i],
                       P.chan_off[i])
    t_fwd = torch.frombuffer(bytearray(bytes(fwd)), dtype=torch.uint8).to(DEV)
    t_bwd = torch.frombuffer(bytearray(bytes(bwd)), dtype=torch.uint8).to(DEV)
    stride = P.total_co + 3
    res = []
    for fill in (float("nan"), -7.0):
        wq, aux = _guarded(P.total_elems, fill), _guarded(4 * P.total_co, fill)
        assert L.mhaq_fq_wlayer_fwd_multi(t_fwd.data_ptr(), n, P.total_co, P.max_row, wq.data_ptr() + 4 * GUARD,
                                          aux.data_ptr() + 4 * GUARD, st) == 0
        torch.cuda.synchronize()
        assert _guards_hold(wq, fill) and _guards_hold(aux, fill), (name, "forward guards")
        wide = torch.zeros(4, stride, device=DEV)               # the forward's aux slab as a window of a wider one
        wide[:, :P.total_co] = aux[GUARD:-GUARD].view(4, P.total_co)
        gw, gls = _guarded(P.total_elems, fill), _guarded(P.total_co, fill)
        assert L.mhaq_fq_wlayer_bwd_group(t_bwd.data_ptr(), n, P.total_co, P.max_row, wide.data_ptr(), stride,
                                          gw.data_ptr() + 4 * GUARD, gls.data_ptr() + 4 * GUARD, METHOD_VALUE[method],
                                          None, 5, 9, None, st) == 0
        torch.cuda.synchronize()
        assert _guards_hold(gw, fill) and _guards_hold(gls, fill), (name, "backward guards")
        res.append([t[GUARD:-GUARD] for t in (wq, aux, gw, gls)])
    for a, b, what in zip(res[0], res[1], ("wq_all", "aux", "gw_all", "g_log_s")):
        assert not torch.isnan(a).any(), (name, method, what, "an element was not written")
        assert _same_bits(a, b), (name, method, what)
