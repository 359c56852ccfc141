#!/usr/bin/env python3
"""Stand-alone timing of the stem's pool and BatchNorm backward on one GPU: torch's max_pool2d forward against
mhaq_fq_maxpool3s2_fwd, and torch's max_pool2d backward + mhaq_fq_bn_bwd against mhaq_fq_bn_pool_bwd, on the stem's own
tensor ([250, 64, 112, 112] fp32 channels_last by default).

Method (that of profiles/r10_bn_bwd_micro.txt): before every timed call a 1 GiB buffer is written and the tensor the step's
producer would just have written (t for the forward, the pooled gradient g for the backward) is rewritten; 7 timed calls after
one warm-up, HIP events around the whole call; min and median.  Bytes are algorithmic (every tensor once per pass that reads or
writes it), TB/s is bytes / min.

    python3 tools/stem_pool_bench.py --out profiles/r11_stem_pool_micro.txt [--lib label=/path/to/libmhaq_fq.so ...]

--lib adds builds of the same library (cache policies, rows in flight) as further rows; the product library is always first.
--dtype bf16 / fp16 times the 16-bit forms on the same tensor in that type: torch's 16-bit pool, mhaq_fq_maxpool3s2_fwd_x16,
mhaq_fq_bn_bwd_x16 on torch's 16-bit dy and mhaq_fq_bn_pool_bwd_x16 (profiles/r15_stem_pool16_micro.txt) -- and three rows for
the stem's forward from the convolution's output (x is the rewritten tensor there): the framework's BatchNorm forward + torch's
pool, mhaq_fq_bn_fwd_x16 + mhaq_fq_maxpool3s2_fwd_x16, and mhaq_fq_bn_fwd_x16 without a y + mhaq_fq_bn_norm_pool3s2_fwd_x16
(profiles/r22_stem_pool16_micro.txt).
--step [--steps K] [--warmup W]: not a kernel timing but tools/amp_bench.py's captured ResNet-18 batch-250 bf16 step in this
process's configuration, for A/B runs of MHAQ_STEM_POOL_X16 (profiles/r22_stem_pool16_ab.txt).
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mhaq_amd import _lib  # noqa: E402


def load(path):
    L = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[250, 64, 112, 112], metavar=("N", "C", "H", "W"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH")
    ap.add_argument("--dtype", choices=["fp32", "bf16", "fp16"], default="fp32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.step:
        # tools/amp_bench.py's ResNet-18 batch-250 bf16 step, captured, in THIS process's configuration (MHAQ_BN_BACKWARD_X16 and
        # MHAQ_STEM_POOL_X16 as the environment has them): one JSON line with the step, the pooled node's counters and the peak
        # of allocated device memory over the process
        import json
        from tools import amp_bench                    # (seeds the private MIOpen database before MIOpen is first used)
        from mhaq_amd import _ext, bn_backward
        torch.backends.cudnn.benchmark = False
        rec = {"tool": "stem_pool_bench", "device": torch.cuda.get_device_name(0), "bn_backward_x16": bn_backward.x16_enabled(),
               "stem_pool_x16": bn_backward.pool_x16_enabled()}
        rec["bf16_captured"] = amp_bench.step(torch.device("cuda:0"), True, True, args.steps, max(args.warmup, 4))
        E = _ext.ext()
        rec["pool_x16_forwards_recorded"] = E.bn_pool_hip_forwards_x16()
        rec["pool_x16_backwards_recorded"] = E.bn_pool_hip_backwards_x16()
        rec["x16_backwards_recorded"] = E.bn_hip_backwards_x16()
        rec["peak_allocated_mb"] = round(torch.cuda.max_memory_allocated() / 1e6, 1)
        print(json.dumps(rec), flush=True)
        return
    dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    x16 = args.dtype != "fp32"
    dt = {"bf16": _lib.DT_BF16, "fp16": _lib.DT_F16}.get(args.dtype)
    es = 2 if x16 else 4                               # bytes per element of x, t, g, p, dy and dx
    bits = (lambda a: a.view(torch.int16)) if x16 else (lambda a: a.view(torch.int32))
    dev = "cuda:0"
    n, c, h, w = args.shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    libs = [("product", _lib.lib())] + [(s.split("=", 1)[0], load(s.split("=", 1)[1])) for s in args.lib]
    gen = torch.Generator(device=dev).manual_seed(1)
    cl = torch.channels_last
    x = torch.randn((n, c, h, w), device=dev, generator=gen).to(dtype).contiguous(memory_format=cl)
    # the pool's input (which element wins is data, not a cost: every element is read either way)
    t0 = (torch.randn((n, c, h, w), device=dev, generator=gen) * 2).to(dtype).contiguous(memory_format=cl)
    t = t0.clone(memory_format=torch.preserve_format)
    g0 = torch.randn((n, c, oh, ow), device=dev, generator=gen).to(dtype).contiguous(memory_format=cl)
    g = g0.clone(memory_format=torch.preserve_format)
    mean = x.mean((0, 2, 3), dtype=torch.float32)
    invstd = (x.float().var((0, 2, 3), unbiased=False) + 1e-5).rsqrt()
    gamma = torch.randn(c, device=dev, generator=gen)
    p = torch.empty_like(g)
    code = torch.empty(g.shape, dtype=torch.uint8, device=dev).contiguous(memory_format=cl)
    dx = torch.empty_like(x)
    dw, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
    nb = (libs[0][1].mhaq_fq_bn_bwd_x16_workspace_bytes if x16 else libs[0][1].mhaq_fq_bn_bwd_workspace_bytes)(n * h * w, c)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda a: ctypes.c_void_p(a.data_ptr())
    k3, s2, p1, d1 = [3, 3], [2, 2], [1, 1], [1, 1]

    p_t, idx_t = torch.ops.aten.max_pool2d_with_indices(t, k3, s2, p1, d1, False)
    state = {}

    def torch_fwd():
        torch.ops.aten.max_pool2d_with_indices(t, k3, s2, p1, d1, False)

    def torch_pool_bwd():
        state["dy"] = torch.ops.aten.max_pool2d_with_indices_backward(g, t, k3, s2, p1, d1, False, idx_t)

    def bn_bwd(L):
        if x16:
            assert L.mhaq_fq_bn_bwd_x16(P(x), P(state["dy"]), P(mean), P(invstd), P(gamma), P(dx), P(dw), P(db), n * h * w, c,
                                        dt, P(ws), nb, st) == 0
        else:
            assert L.mhaq_fq_bn_bwd(P(x), P(state["dy"]), P(mean), P(invstd), P(gamma), P(dx), P(dw), P(db), n * h * w, c,
                                    P(ws), nb, st) == 0

    def hip_fwd(L):
        if x16:
            assert L.mhaq_fq_maxpool3s2_fwd_x16(P(t), P(p), P(code), n, h, w, c, dt, st) == 0
        else:
            assert L.mhaq_fq_maxpool3s2_fwd(P(t), P(p), P(code), n, h, w, c, st) == 0

    def hip_bwd(L):
        if x16:
            assert L.mhaq_fq_bn_pool_bwd_x16(P(x), P(g), P(code), P(mean), P(invstd), P(gamma), P(dx), P(dw), P(db), n, h, w,
                                             c, dt, P(ws), nb, st) == 0
        else:
            assert L.mhaq_fq_bn_pool_bwd(P(x), P(g), P(code), P(mean), P(invstd), P(gamma), P(dx), P(dw), P(db), n, h, w, c,
                                         P(ws), nb, st) == 0

    def timed(fn, rewrite):
        out = []
        for i in range(args.reps + 1):
            flush.fill_(float(i))
            rewrite()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if i:
                out.append(a.elapsed_time(e) * 1e3)
        return min(out), statistics.median(out)

    rew_t = lambda: t.copy_(t0)
    rew_g = lambda: g.copy_(g0)
    elems = n * c * h * w
    pel = n * c * oh * ow
    rows = []

    def row(what, variant, mm, nbytes):
        rows.append(f"{what:>38s} {variant:>8s} {mm[0]:8.1f} {mm[1]:8.1f} {nbytes / 1e6:8.0f} {nbytes / mm[0] / 1e6:6.2f}")
        print(rows[-1], flush=True)

    # exactness first: the two forms give the same bits
    hip_fwd(libs[0][1])
    assert torch.equal(bits(p), bits(p_t)), "pool forward differs from torch"
    torch_pool_bwd()
    bn_bwd(libs[0][1])
    ref = (dx.clone(), dw.clone(), db.clone())
    hip_bwd(libs[0][1])
    assert torch.equal(bits(ref[0]), bits(dx)), "backward differs (dx)"
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ref[1:], (dw, db))), "backward differs"
    del ref
    sfx = "_x16" if x16 else ""
    row("pool fwd", "torch", timed(torch_fwd, rew_t), es * elems + es * pel + 8 * pel)
    for label, L in libs:
        row("pool fwd", label, timed(lambda: hip_fwd(L), rew_t), es * elems + es * pel + pel)
    hip_fwd(libs[0][1])
    row("pool bwd (torch)", "torch", timed(torch_pool_bwd, rew_g), 8 * pel + es * pel + es * elems)
    row(f"mhaq_fq_bn_bwd{sfx} on that dy", "product", timed(lambda: bn_bwd(libs[0][1]), lambda: None), 5 * es * elems)
    row(f"pool bwd (torch) + mhaq_fq_bn_bwd{sfx}", "product", timed(lambda: (torch_pool_bwd(), bn_bwd(libs[0][1])), rew_g),
        8 * pel + es * pel + es * elems + 5 * es * elems)
    for label, L in libs:
        row(f"mhaq_fq_bn_pool_bwd{sfx}", label, timed(lambda: hip_bwd(L), rew_g), 2 * (es * elems + es * pel + pel) + es * elems)
    if x16:
        # the stem's forward from the convolution's output x: BatchNorm and pool as the bf16 step runs them (the framework's
        # BatchNorm, torch's pool), as the two HIP entry points one after the other, and as the pooled node runs them
        # (statistics without a y, then normalisation and pool in one launch); x is rewritten before every timed call
        L0 = libs[0][1]
        x0 = x.clone(memory_format=torch.preserve_format)
        rew_x = lambda: x.copy_(x0)
        beta = torch.randn(c, device=dev, generator=gen)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        sm, si = torch.empty(c, device=dev), torch.empty(c, device=dev)
        y = torch.empty_like(x)
        nbf = L0.mhaq_fq_bn_fwd_x16_workspace_bytes(n * h * w, c)
        wsf = torch.empty(nbf, dtype=torch.uint8, device=dev)

        def stock_fwd():
            out = torch.ops.aten._batch_norm_impl_index(x, gamma, beta, rm, rv, True, 0.1, 1e-5, True)
            torch.ops.aten.max_pool2d_with_indices(out[0], k3, s2, p1, d1, False)

        def stats(L, yp):
            assert L.mhaq_fq_bn_fwd_x16(P(x), P(gamma), P(beta), yp, P(sm), P(si), P(rm), P(rv), 0.1, 1e-5, n * h * w, c, dt,
                                        P(wsf), nbf, st) == 0

        def hip_two(L):
            stats(L, P(y))
            assert L.mhaq_fq_maxpool3s2_fwd_x16(P(y), P(p), P(code), n, h, w, c, dt, st) == 0

        def hip_fused(L):
            stats(L, None)
            assert L.mhaq_fq_bn_norm_pool3s2_fwd_x16(P(x), P(sm), P(si), P(gamma), P(beta), P(p), P(code), n, h, w, c, dt,
                                                     st) == 0

        hip_two(L0)
        ref = (p.clone(), code.clone())
        p.zero_()
        code.zero_()
        hip_fused(L0)
        assert torch.equal(bits(ref[0]), bits(p)) and torch.equal(ref[1], code), "pooled forward differs from the two launches"
        del ref
        row("framework BatchNorm fwd + torch pool", "torch", timed(stock_fwd, rew_x),
            3 * es * elems + es * elems + es * pel + 8 * pel)
        for label, L in libs:
            row("bn_fwd_x16 + maxpool3s2_fwd_x16", label, timed(lambda: hip_two(L), rew_x),
                3 * es * elems + es * elems + es * pel + pel)
        for label, L in libs:
            row("bn_fwd_x16(y=NULL) + bn_norm_pool3s2", label, timed(lambda: hip_fused(L), rew_x),
                2 * es * elems + es * pel + pel)
    head = (f"Stem pool and BatchNorm backward stand-alone, {tuple(args.shape)} {args.dtype} channels_last ({elems / 1e6:.1f} M elements), one "
            f"{torch.cuda.get_device_name(0)}.\nBefore every timed call a 1 GiB buffer is written and the producer's tensor (t for the "
            f"forward, the pooled gradient for the backward;\nnothing for the line that times mhaq_fq_bn_bwd alone: its dy stays as the "
            f"flush left it) is rewritten; {args.reps} timed calls after one warm-up,\nHIP events around the whole call.  MB = algorithmic "
            f"bytes, TB/s = MB / min.  Both forms were checked to give the same bits first.\n\n"
            f"{'what':>38s} {'variant':>8s} {'min us':>8s} {'med us':>8s} {'MB':>8s} {'TB/s':>6s}\n")
    text = head + "\n".join(rows) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
