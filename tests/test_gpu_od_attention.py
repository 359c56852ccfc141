"""GPU: the PSA attention kernels (csrc/od_attn.hip) against the reference's three statements in fp64 on the exactly upcast inputs.
Bars (tests/distill_ref.grad_bar): MARGIN times the error of the same statements run by the framework on the device in the case's
dtype, plus 8 * 2^-24 * max|fp64| -- for out, d q, d k and d v each -- plus half an ulp of a 16-bit output dtype at max|fp64| for
the one final rounding.  Measured shares: DESIGN section 21."""
import copy
import functools
import math

import pytest
import torch

from mhaq_amd import od_attention as A
from mhaq_amd import ops
from tests.distill_ref import grad_bar

pytestmark = pytest.mark.gpu
F64, F32, BF16, F16, BAND = torch.float64, torch.float32, torch.bfloat16, torch.float16, 64
SHAPES = [(1, 1, 1, 1), (1, 2, 4, 4), (2, 1, 5, 5), (1, 2, 8, 10), (2, 3, 20, 20)]      # (B, nh, H, W)


def statements(qkv, nh, addend=None):
    """The reference's Attention.forward, its three tensor statements (dim_key 32, dim_head 64)."""
    b, _, h, w = qkv.shape
    q, k, v = qkv.view(b, nh, 128, h * w).split([32, 32, 64], dim=2)
    attn = ((q.transpose(-2, -1) @ k) * 32 ** -0.5).softmax(dim=-1)
    x = (v @ attn.transpose(-2, -1)).view(b, nh * 64, h, w)
    return x if addend is None else x + addend


def autograd(qkv, nh, addend, grad_out, dtype):
    """out, d qkv of the statements in `dtype` on the device from the same bits."""
    x = qkv.to(dtype, copy=True).requires_grad_(True)
    out = statements(x, nh, None if addend is None else addend.to(dtype))
    return out.detach(), torch.autograd.grad(out, x, grad_out.to(dtype))[0]


@functools.lru_cache(maxsize=None)
def case(dtype, with_addend, shape, spread=False):
    """Seeded inputs in `dtype` with the fp64 truth and the framework chain's results; made once, never written to."""
    (b, nh, h, w), gen = shape, torch.Generator().manual_seed(1234 + sum(shape))
    n = h * w
    qkv = torch.randn(b, nh, 128, n, generator=gen, dtype=F64)
    if spread:          # scores of about +-60, and row i's largest at the LAST key, 4 above the others, through q[0] and k[0]
        qkv[:, :, :64] *= 20 ** 0.5
        qkv[:, :, 32] = 0
        qkv[:, :, 32, -1] = 8
        s = (qkv[:, :, :32].transpose(-2, -1) @ qkv[:, :, 32:64]) * 32 ** -0.5
        qkv[:, :, 0] += (s[..., :-1].amax(-1) + 4 - s[..., -1]) / (8 * 32 ** -0.5)
    qkv = qkv.view(b, nh * 128, h, w).to(dtype).cuda()
    addend = torch.randn(b, nh * 64, h, w, generator=gen).to(dtype).cuda() if with_addend else None
    grad_out = (torch.randn(b, nh * 64, h, w, generator=gen) * torch.linspace(0.5, 2.0, w)).to(dtype).cuda()
    return dict(qkv=qkv, addend=addend, grad_out=grad_out, nh=nh, ref=autograd(qkv, nh, addend, grad_out, F64),
                chain=autograd(qkv, nh, addend, grad_out, dtype))


def half_ulp(v, dtype):
    """Half an ulp of |v| in a 16-bit `dtype` (0 for float32): the one rounding of a stored result."""
    return 0.0 if dtype is F32 or v == 0 else 2.0 ** (math.floor(math.log2(v)) - (7 if dtype is BF16 else 10) - 1)


def banded(shape, dtype):
    buf = torch.full((math.prod(shape) + 2 * BAND,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[BAND:-BAND].view(shape)


def run_kernels(c):
    """Forward and backward through the ops wrappers into NaN-filled buffers between NaN bands -> out, lse, d qkv."""
    qkv, nh = c["qkv"], c["nh"]
    b, _, h, w = qkv.shape
    bufs, views = zip(banded((b, nh * 64, h, w), qkv.dtype), banded((b, nh, h * w), F32), banded(qkv.shape, qkv.dtype))
    ops.od_attn_fwd(qkv, nh, c["addend"], out=views[0], lse=views[1])
    ops.od_attn_bwd(qkv, c["grad_out"], views[1], nh, out=views[2])
    for buf in bufs:             # no stray write, and every element written
        assert bool(buf[:BAND].isnan().all()) and bool(buf[-BAND:].isnan().all()) and not bool(buf[BAND:-BAND].isnan().any())
    return views


def shares_of_the_bars(out, dqkv, c, dtype):
    """The share of its bar that out and each of d q, d k, d v uses."""
    (o64, g64), (o_t, g_t), nh = c["ref"], c["chain"], c["nh"]
    parts = {"out": (out, o_t, o64)}
    split = lambda t: t.view(t.shape[0], nh, 128, -1).split([32, 32, 64], dim=2)
    parts.update({n: x for n, x in zip(("dq", "dk", "dv"), zip(split(dqkv), split(g_t), split(g64)))})
    return {n: float((got.double() - r).abs().max()) / (grad_bar(t, r) + half_ulp(float(r.abs().max()), dtype) or 1e-300)
            for n, (got, t, r) in parts.items()}


CASES = [(d, a, s, False) for d in (F32, BF16, F16) for a in (False, True) for s in SHAPES] \
    + [(d, True, SHAPES[-1], True) for d in (F32, BF16, F16)]


@pytest.mark.parametrize("dtype,with_addend,shape,spread", CASES, ids=lambda v: str(v).replace("torch.", "").replace(" ", ""))
def test_kernels_against_the_statements(dtype, with_addend, shape, spread):
    c = case(dtype, with_addend, shape, spread)
    out, lse, dqkv = run_kernels(c)
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip((out, lse, dqkv), run_kernels(c)))
    shares = shares_of_the_bars(out, dqkv, c, dtype)
    print(f"bar shares {dtype} addend={with_addend} {shape} spread={spread}: " + ", ".join(f"{n} {v:.3f}" for n, v in shares.items()))
    assert max(shares.values()) <= 1.0, shares
    # the public function: the same bits, and the addend's gradient is grad_out itself
    x = c["qkv"].clone().requires_grad_(True)
    ad = None if c["addend"] is None else c["addend"].clone().requires_grad_(True)
    y = A.psa_attention(x, c["nh"], ad)
    y.backward(c["grad_out"])
    assert torch.equal(y.detach().view(torch.uint8), out.view(torch.uint8)) and torch.equal(x.grad.view(torch.uint8), dqkv.view(torch.uint8))
    assert ad is None or torch.equal(ad.grad.view(torch.uint8), c["grad_out"].view(torch.uint8))
    with torch.no_grad():
        assert torch.equal(A.psa_attention(c["qkv"], c["nh"], c["addend"]).view(torch.uint8), out.view(torch.uint8))


def test_forward_and_backward_replay_in_a_graph():
    c = case(F32, True, SHAPES[2])
    eager = [t.clone() for t in run_kernels(c)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = ops.od_attn_fwd(c["qkv"], c["nh"], c["addend"])
        dqkv = ops.od_attn_bwd(c["qkv"], c["grad_out"], lse, c["nh"])
    for _ in range(3):
        for t in (out, lse, dqkv):
            t.fill_(float("nan"))
        graph.replay()
        assert all(torch.equal(x, y) for x, y in zip(eager, (out, lse, dqkv)))


def test_attention_module_against_its_torch_core():
    """Attention(128, 2) in train mode against the same module with the statements as its core; fp64 copy as the truth."""
    torch.manual_seed(7)
    m = A.Attention(128, 2).cuda().train()
    x = torch.randn(2, 128, 5, 5, device="cuda")
    go = torch.randn(2, 128, 5, 5, device="cuda") * torch.linspace(0.5, 2.0, 5, device="cuda")

    def torch_core(mod, inp):
        b, ch, h, w = inp.shape
        qkv = mod.qkv(inp)
        v = qkv.view(b, mod.num_head, 128, h * w)[:, :, 64:].reshape(b, ch, h, w)
        return mod.conv2(statements(qkv, mod.num_head, mod.conv1(v)))

    def step(mod, fwd, dt):
        mod = copy.deepcopy(mod).to(dt)
        out = fwd(mod, x.to(dt))
        names, params = zip(*mod.named_parameters())
        return dict(out=out.detach(), **dict(zip(names, torch.autograd.grad(out, params, go.to(dt)))))

    got, chain, ref = step(m, lambda mod, inp: mod(inp), F32), step(m, torch_core, F32), step(m, torch_core, F64)
    shares = {n: float((got[n].double() - ref[n]).abs().max()) / grad_bar(chain[n], ref[n]) for n in ref}
    print("bar shares module: " + ", ".join(f"{n} {v:.3f}" for n, v in shares.items()))
    assert len(shares) == 10 and max(shares.values()) <= 1.0, shares
