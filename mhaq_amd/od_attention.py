"""Detection model: the attention of YOLOv11's PSA block with its core -- softmax(q^T k * scale) applied to v, plus the positional
branch -- as fused matrix-instruction HIP kernels on the qkv convolution's output (csrc/od_attn.hip).

The reference's `Attention.forward` runs two batched matmuls, a scale, a softmax and an add, writes a [B, nh, N, N] tensor three
times and keeps one for the backward.  Here the forward is one launch and the backward two; what is kept is `lse` [B, nh, N].
`psa_attention` is the functional form, `Attention` the drop-in for the reference's module (its `state_dict` loads with
`strict=True`).  The three convolutions and their BatchNorm stay with the framework.  include/mhaq_fq.h has the contract and the
deviations, DESIGN section 21 the launch plan.
"""
from __future__ import annotations

import torch

from . import ops


class _PsaAttention(torch.autograd.Function):
    """out = attention(qkv) (+ addend); backward is two launches into d qkv, and d addend is grad_out itself."""

    @staticmethod
    def forward(ctx, qkv, addend, num_head):
        out, lse = ops.od_attn_fwd(qkv, num_head, addend)
        ctx.num_head = num_head
        ctx.save_for_backward(qkv, lse)
        return out

    @staticmethod
    def backward(ctx, grad):
        qkv, lse = ctx.saved_tensors
        grad = grad.contiguous()
        dqkv = ops.od_attn_bwd(qkv, grad, lse, ctx.num_head) if ctx.needs_input_grad[0] else None
        return dqkv, (grad if ctx.needs_input_grad[1] else None), None


def psa_attention(qkv: torch.Tensor, num_head: int, addend: torch.Tensor | None = None) -> torch.Tensor:
    """`qkv` [B, num_head * 128, H, W]: per head 32 rows of q, 32 of k, 64 of v (float32, bfloat16 or float16, on the device).
    Returns [B, num_head * 64, H, W] in the same dtype: v @ softmax(q^T k * 32 ** -0.5)^T per head, plus `addend` (same shape
    and dtype as the result) if given.  Without autograd no `lse` is written."""
    qkv = qkv.contiguous()
    addend = None if addend is None else addend.contiguous()
    if torch.is_grad_enabled():
        return _PsaAttention.apply(qkv, addend, int(num_head))
    return ops.od_attn_fwd(qkv, num_head, addend, want_lse=False)[0]


class _ConvNorm(torch.nn.Module):
    """conv (no bias) + BatchNorm2d(eps=1e-3, momentum=0.03) + activation, with the reference's attribute names."""

    def __init__(self, in_ch, out_ch, activation, k=1, p=0, g=1):
        super().__init__()
        self.conv = torch.nn.Conv2d(in_ch, out_ch, k, 1, p, groups=g, bias=False)
        self.norm = torch.nn.BatchNorm2d(out_ch, eps=1e-3, momentum=0.03)
        self.relu = activation

    def forward(self, x):
        return self.relu(self.norm(self.conv(x)))


class Attention(torch.nn.Module):
    """The reference's `Attention(ch, num_head)`: its constructor, its submodules `qkv`, `conv1` (depthwise 3x3 on v) and `conv2`,
    its forward -- with the attention core as one `psa_attention` call.  ch // num_head must be 64."""

    def __init__(self, ch, num_head):
        super().__init__()
        self.num_head = num_head
        self.dim_head = ch // num_head
        self.dim_key = self.dim_head // 2
        self.scale = self.dim_key ** -0.5
        self.qkv = _ConvNorm(ch, ch + 2 * self.dim_key * num_head, torch.nn.Identity())
        self.conv1 = _ConvNorm(ch, ch, torch.nn.Identity(), k=3, p=1, g=ch)
        self.conv2 = _ConvNorm(ch, ch, torch.nn.Identity())

    def forward(self, x):
        b, c, h, w = x.shape
        qkv = self.qkv(x)
        v = qkv.view(b, self.num_head, 2 * self.dim_key + self.dim_head, h * w)[:, :, 2 * self.dim_key:]
        return self.conv2(psa_attention(qkv, self.num_head, self.conv1(v.reshape(b, c, h, w))))
