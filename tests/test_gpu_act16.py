"""GPU (-m gpu): the 16-bit activation path (mhaq_fq_act_*_x16, csrc/fq_io16.hip) behind NoisyAct under torch.autocast.

Contract (include/mhaq_fq.h, "16-bit activations"; mhaq_amd/ops.py autocast_x16): the reference's op chain on a 16-bit x
promotes to fp32 at the clamp against the fp32 bounds, so its y is fp32 and bit-equal to the chain on x.float(), x.grad
is the fp32 gx rounded to nearest-even, and the parameter gradients are the fp32 ones.  Under autocast (x in the
autocast dtype) the fused path returns y in x's dtype with the bits of y_ref.to(dtype); everything else is as the
reference.  NaN is compared as NaN (its payload after rounding is not part of the contract)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import fq_closed_form as CF  # noqa: E402
from oracle import fq_eager as O  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
PARAM_SETS = [((-3.0, 1.0), -1.0, True), ((-4.37, 2.21), -2.3, True), ((-9.913, 0.087), -0.47, True),
              ((-4.0, 2.5), 0.0, False)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from mhaq_amd import _lib, ops
    _lib.lib()
    return ops


def P(v, grad=True):
    return torch.tensor([v], device=DEV, requires_grad=grad)


def same_bits(a, b):
    """Equal 16-bit (or fp32) tensors bit for bit, NaN compared as NaN."""
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = {2: torch.int16, 4: torch.int32}[a.element_size()]
    a, b = a.contiguous().flatten(), b.contiguous().flatten()
    keep = ~na.contiguous().flatten()
    return torch.equal(a.view(iv)[keep], b.view(iv)[keep])


def same_values(a, b):
    """Equal values (+0 == -0), NaN compared as NaN."""
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(torch.isnan(a), torch.isnan(b)) and bool(((a == b) | torch.isnan(a)).all())


def yardsticks(x16, g16, r, ls, lq, b, method):
    """1e-6 x sum |terms| bars of the three parameter gradients (oracle/fq_closed_form.py)."""
    s, qr = torch.exp2(ls.detach()), torch.exp2(lq.detach())
    bb = b.detach()
    hi = (bb + qr) - s
    cf = CF.per_tensor(x16.float(), g16.float(), r, s, bb, bb, hi, method)
    ln2 = math.log(2.0)
    return (1e-6 * (float(cf["abs_s"]) + float(cf["abs_g"])) * float(s) * ln2 + 1e-30,
            1e-6 * float(cf["abs_g"]) * float(qr) * ln2 + 1e-30, 1e-6 * float(cf["abs_g"]) + 1e-30)


def _inputs(shape, dtype, signed, seed, scale=1.5):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=gen) * scale
    if not signed:
        x = x.relu()
    g = torch.randn(*shape, generator=gen)
    r = torch.randint(0, 2, shape, generator=gen).float() - 0.5
    return x.to(dtype).to(DEV), g.to(dtype).to(DEV), r.to(DEV)


def _fused16(ops, x16, g16, logs, b, signed, method, r=None):
    xg = x16.detach().clone().requires_grad_(True)
    ls, lq, bb = P(logs[0]), P(logs[1]), P(b, signed)
    with torch.autocast("cuda", dtype=x16.dtype):
        y, params = ops.fake_quant_act_layer(xg, ls, lq, bb, method,
                                             r_sign=None if r is None else (r * 2).to(torch.int8))
    y.backward(g16)
    return y.detach(), xg.grad, (ls.grad, lq.grad, bb.grad), (ls, lq, bb)


def _oracle(x16, g16, logs, b, signed, method, r):
    """The reference's chain on the 16-bit tensor itself, explicit signs."""
    xr = x16.detach().clone().requires_grad_(True)
    ls, lq, bb = P(logs[0]), P(logs[1]), P(b, signed)
    y, _ = O.act_fake_quant(xr, ls, lq, bb, r=r, method=method)
    assert y.dtype == torch.float32
    y.backward(g16.float())
    assert xr.grad.dtype == x16.dtype
    return y.detach(), xr.grad, (ls.grad, lq.grad, bb.grad)


def _check_params(got, ref, yard, signed):
    for k, (a, r_, t) in enumerate(zip(got, ref, yard)):
        if k == 2 and not signed:
            assert a is None
            continue
        assert abs(float(a) - float(r_)) <= t, (k, float(a), float(r_), t)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("method", ["STE", "LSQ", "EWGS"])
@pytest.mark.parametrize("logs,b,signed", PARAM_SETS)
def test_kernel_matches_the_reference_chain_on_the_16bit_tensor(ops, dtype, method, logs, b, signed):
    x16, g16, r = _inputs((6, 16, 20, 20), dtype, signed, int(abs(logs[0]) * 1000))
    y, gx, pg, (ls, lq, bb) = _fused16(ops, x16, g16, logs, b, signed, method, r)
    y_r, gx_r, pg_r = _oracle(x16, g16, logs, b, signed, method, r)
    assert y.dtype == dtype and gx.dtype == dtype
    assert same_bits(y, y_r.to(dtype))
    assert same_values(gx, gx_r)
    _check_params(pg, pg_r, yardsticks(x16, g16, r, ls, lq, bb, method), signed)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("method", ["STE", "LSQ", "EWGS"])
@pytest.mark.parametrize("logs,b,signed", PARAM_SETS)
def test_in_kernel_signs_equal_the_fp32_kernel_on_the_upcast_tensors(ops, dtype, method, logs, b, signed):
    """Sign stream v3 is a pure function of the element index: the 16-bit backward (one tile byte per lane) draws the
    fp32 backward's signs (a nibble per lane) at the same (seed, offset).  A ragged size: several blocks and a tail."""
    x16, g16, r = _inputs((3, 7, 33, 35), dtype, signed, 7 + int(abs(logs[1]) * 100))
    ops.manual_seed(1234)
    y, gx, pg, (ls, lq, bb) = _fused16(ops, x16, g16, logs, b, signed, method)
    ops.manual_seed(1234)
    x32 = x16.float().requires_grad_(True)
    ls2, lq2, bb2 = P(logs[0]), P(logs[1]), P(b, signed)
    y32, _ = ops.fake_quant_act_layer(x32, ls2, lq2, bb2, method)
    y32.backward(g16.float())
    assert same_bits(y, y32.detach().to(dtype))
    assert same_bits(gx, x32.grad.to(dtype))
    # both within 1e-6 x sum|terms| of the exact value; the sums of |terms| do not depend on the signs' values
    yard = yardsticks(x16, g16, r, ls, lq, bb, method)
    _check_params(pg, (ls2.grad, lq2.grad, bb2.grad), tuple(2 * t for t in yard), signed)


_BIG = (20 << 20) + 4099
# (n, storage offset of the gradient view): the smallest sizes at which the caller's signs are read on another path
_RSIGN_CASES = [pytest.param(dt, n, off, id=f"{name}-{n}+{off}")
                for n, off, dts in [(7, 0, DTYPES), (2053, 0, DTYPES), (5000, 1, DTYPES), (_BIG, 0, DTYPES[:1])]
                for dt, name in zip(DTYPES, ["bf16", "fp16"]) if dt in dts]


@pytest.mark.parametrize("method", ["STE", "EWGS"])           # LSQ reads no signs
@pytest.mark.parametrize("dtype,n,offset", _RSIGN_CASES)
def test_caller_supplied_signs_on_every_backward_path(ops, dtype, n, offset, method):
    """The explicit sign tensor (RSIGN) away from the aligned, tail-free small form of the test above: n = 7 takes the
    element kernel (n < 8); 2053 = one block of 256 vectors and 5 tail elements that read r_sign[t]; a gradient that is
    a view one element into its buffer is 2-byte aligned only and sends the backward to the element kernel, r_sign[i]
    per element; above 20 Mi elements the BIG form reads two 8-byte sign words per lane."""
    xb, gb, rb = _inputs((n + offset,), dtype, True, n % 1000, scale=2.0)
    x16, g16, r = xb[offset:], gb[offset:], rb[offset:]
    assert (g16.data_ptr() % 16 != 0) == bool(offset)
    logs, b, signed = PARAM_SETS[0]
    y, gx, pg, (ls, lq, bb) = _fused16(ops, x16, g16, logs, b, signed, method, r)
    y_r, gx_r, pg_r = _oracle(x16, g16, logs, b, signed, method, r)
    assert y.dtype == dtype and gx.dtype == dtype
    assert same_bits(y, y_r.to(dtype))
    assert same_values(gx, gx_r)
    _check_params(pg, pg_r, yardsticks(x16, g16, r, ls, lq, bb, method), signed)


def _vs_fp32_kernel(ops, x16, g16, logs=(-3.0, 1.0), b=-1.0, method="STE", seed=99):
    """16-bit path against the fp32 kernels on the upcast tensors, in-kernel signs at the same seed."""
    ops.manual_seed(seed)
    y, gx, pg, (ls, lq, bb) = _fused16(ops, x16, g16, logs, b, True, method)
    ops.manual_seed(seed)
    x32 = x16.detach().float().requires_grad_(True)
    ls2, lq2, bb2 = P(logs[0]), P(logs[1]), P(b)
    y32, _ = ops.fake_quant_act_layer(x32, ls2, lq2, bb2, method)
    y32.backward(g16.float())
    assert same_bits(y, y32.detach().to(x16.dtype))
    assert same_bits(gx, x32.grad.to(x16.dtype))
    r = torch.full(x16.shape, 0.5, device=DEV)         # (the bars depend on |r| only)
    _check_params(pg, (ls2.grad, lq2.grad, bb2.grad), tuple(2 * t for t in yardsticks(x16, g16, r, ls, lq, bb, method)),
                  True)
    return y, gx


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2053])
def test_small_and_ragged_sizes(ops, dtype, n):
    x16, g16, _ = _inputs((n,), dtype, True, n)
    _vs_fp32_kernel(ops, x16, g16)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_channels_last_keeps_its_layout(ops, dtype):
    x16, g16, _ = _inputs((4, 24, 13, 11), dtype, True, 5)
    x16 = x16.contiguous(memory_format=torch.channels_last)
    y, gx = _vs_fp32_kernel(ops, x16, g16, method="EWGS")      # g16 arrives contiguous: like_layout re-lays it
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert gx.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("method", ["STE", "LSQ"])
def test_view_with_a_one_element_storage_offset_takes_the_element_kernel(ops, dtype, method):
    n = 5000
    base, g16, _ = _inputs((n + 1,), dtype, True, 17)
    x16 = base[1:]                                 # 2-byte aligned, not 16: the element kernel
    assert x16.data_ptr() % 16 != 0
    _vs_fp32_kernel(ops, x16, g16[1:].clone(), method=method)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_large_ragged_tensor_bandwidth_form(ops, dtype):
    """Above 20 Mi elements the backward switches to one partial row per block (the BIG form, 2 vectors per lane)."""
    n = (20 << 20) + 4099
    x16, g16, _ = _inputs((n,), dtype, True, 3, scale=2.0)
    _vs_fp32_kernel(ops, x16, g16, method="STE")


def _special(dtype):
    tiny = 2.0 ** -130 if dtype is torch.bfloat16 else 2.0 ** -20       # 16-bit subnormals
    s = 2.0 ** -3
    ties = [-1.0 + (k + 0.5) * s for k in range(0, 16)]                  # (x - zp) / s = k + 1/2 exactly
    vals = [float("nan"), float("inf"), -float("inf"), tiny, -tiny, 3 * tiny, 0.0, -0.0, 1e4, -1e4] + ties
    x = torch.tensor(vals * 9, dtype=torch.float32)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("method", ["STE", "LSQ", "EWGS"])
def test_special_values(ops, dtype, method):
    x16 = _special(dtype).to(DEV)
    gen = torch.Generator().manual_seed(2)
    g16 = torch.randn(x16.shape, generator=gen).to(dtype).to(DEV)
    r = (torch.randint(0, 2, x16.shape, generator=gen).float() - 0.5).to(DEV)
    y, gx, _, _ = _fused16(ops, x16, g16, (-3.0, 2.0), -1.0, True, method, r)
    y_r, gx_r, _ = _oracle(x16, g16, (-3.0, 2.0), -1.0, True, method, r)
    assert same_bits(y, y_r.to(dtype))
    assert same_values(gx, gx_r)
    assert torch.isnan(y).any() and not torch.isnan(y[3:]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape,offset", [((3, 8, 9, 9), 0), ((2, 64, 40, 40), 0), ((5000,), 1)])
def test_eval_form_stats_and_flags_equal_the_fp32_kernel(ops, dtype, shape, offset):
    gen = torch.Generator().manual_seed(8)
    n = int(torch.tensor(shape).prod())
    base = (torch.randn(n + offset, generator=gen) * 2).to(dtype).to(DEV)
    x16 = base[offset:].view(shape)
    ls, lq, b = P(-3.0, False), P(2.0, False), P(-2.0, False)
    for poison in (None, float("inf"), float("nan")):
        if poison is not None:
            x16.view(-1)[n // 2] = poison
        with torch.autocast("cuda", dtype=dtype):
            y, params, qstats, flags = ops.fake_quant_act_layer_eval(x16, ls, lq, b)
        y32, params32, qstats32, flags32 = ops.fake_quant_act_layer_eval(x16.float(), ls, lq, b)
        assert y.dtype == dtype and same_bits(y, y32.to(dtype))
        assert torch.equal(params, params32) and torch.equal(qstats, qstats32)
        assert int(flags) == int(flags32)
    assert int(flags) & 4                          # NaN is not an integer (gdnsq.py:216)


@pytest.mark.parametrize("methods", [("LSQ",) * 4, ("STE", "LSQ", "EWGS", "STE")])
def test_act_hub_with_mixed_fp32_and_bf16_quantizers(methods):
    """One finalize_multi launch over fp32 and 16-bit quantizers gives the per-quantizer finalize's bits
    (tests/test_gpu_act_hub.py pattern, under autocast)."""
    from mhaq_amd.act_hub import ActGradHub
    from tests.test_gpu_act_hub import _run, _stack
    gen = torch.Generator().manual_seed(6)
    shapes = [(4, 16, 33, 31), (2, 8, 64, 64), (1000,), (6, 40, 28, 28)]
    dts = [torch.bfloat16, torch.float32, torch.bfloat16, torch.float32]
    xs = [(torch.randn(s, generator=gen) * 2).to(dt).to(DEV) for s, dt in zip(shapes, dts)]
    gs = [torch.randn(s, generator=gen).to(dt).to(DEV) for s, dt in zip(shapes, dts)]
    acts = _stack(methods, (True, False, True, True))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ref_p, ref_x = _run(acts, xs, gs, None)
        hub = ActGradHub(acts)
        for _ in range(2):
            got_p, got_x = _run(acts, xs, gs, hub)
            for a, b in zip(ref_p, got_p):
                assert (a is None and b is None) or torch.equal(a, b)
            for a, b, dt in zip(ref_x, got_x, dts):
                assert a.dtype == dt and torch.equal(a, b)
    assert hub.state()["pending"] == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("method", ["STE", "LSQ", "AEWGS"])
def test_outside_autocast_a_16bit_input_gets_the_references_fp32_y(ops, dtype, method):
    import mhaq_amd as M
    x16, g16, _ = _inputs((2, 8, 10, 10), dtype, True, 12)
    act = M.NoisyAct(init_s=-3, init_q=1, signed=True, qnmethod=M.QNMethod.LSQ).to(DEV).train()
    xg = x16.clone().requires_grad_(True)
    y = act(xg)
    assert y.dtype == torch.float32
    y_r, gx_r, _ = _oracle(x16, g16, (-3.0, 1.0), float(act.act_b), True, "LSQ", None)
    assert same_bits(y.detach(), y_r)
    y.backward(g16.float())
    assert xg.grad.dtype == dtype and same_values(xg.grad, gx_r)
    if method == "AEWGS":                          # the unfused route: same forward bits, fp32 y outside autocast
        act.Q.qnmethod = M.QNMethod.AEWGS
        y2 = act(x16)
        assert y2.dtype == torch.float32 and same_bits(y2.detach(), y_r)
        with torch.autocast("cuda", dtype=dtype):
            y3 = act(x16)
        assert y3.dtype == dtype and same_bits(y3.detach(), y_r.to(dtype))
    with pytest.raises(TypeError):                 # other dtypes are still refused
        act(x16.double())
