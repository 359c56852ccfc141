#!/usr/bin/env python3
"""The optimizer step on one GPU, stand-alone: torch.optim.RAdam's foreach step against the one launch of mhaq_fq_radam_step,
on the parameter list of the bench model (ResNet-18 for 1000 classes, quantized as bench.py quantizes it, channels_last).

Both run on the same tensors in one call, alternating; before every timed call a 1 GiB buffer is written (the state of the
last step is not left in the caches) and the gradients are rewritten; --reps timed calls after one warm-up, HIP events around
the whole step; min and median.  torch's row is its device work as the trainer steps it (the host part of its 20 launches
runs ahead and is not what the events see unless it is the slower side).  Bytes are algorithmic: 7 passes of 4 B for the fused
launch, 21 for the chain.  --lib LABEL=PATH adds builds of csrc/optim.hip alone with a forced cache policy (g: the gradient
load, l: the loads of p, m, v, s: the stores; n = non-temporal, p = default policy), e.g. for gp_lp_sn:
    hipcc $(make -s -C mhaq_amd/csrc print-flags) -DMHAQ_RADAM_G_NT=0 -DMHAQ_RADAM_ST_NT=1 -shared -o gp_lp_sn.so \\
          mhaq_amd/csrc/optim.hip
Every library's p, exp_avg and exp_avg_sq are first checked to be the bits of torch's step on the same state.
usage: tools/radam_bench.py [--out FILE] [--lib LABEL=PATH ...] [--reps R]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mhaq_amd import _lib, optim  # noqa: E402

NAMES = ("mhaq_fq_radam_chunk_elements", "mhaq_fq_radam_step")
DESC = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("c1", "<f4"), ("c2", "<f4")])
WORK = np.dtype([("tensor", "<i4"), ("chunk", "<i4")])
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def load(path):
    """A build of csrc/optim.hip alone: only the entry points used here."""
    L = ctypes.CDLL(path)
    for name in NAMES:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return L


def tables(L, ps, gs, ms, vs, c1, c2):
    """Device tables of one launch (what mhaq_amd/csrc/torch_binding.cpp radam_step builds): (descs, work, ntensors, nwork)."""
    chunk = L.mhaq_fq_radam_chunk_elements()
    d = np.zeros(len(ps), DESC)
    w = []
    for i, (p, g, m, v) in enumerate(zip(ps, gs, ms, vs)):
        d[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), c1, c2)
        w += [(i, c) for c in range((p.numel() + chunk - 1) // chunk)]
    dev = ps[0].device
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)      # noqa: E731
    return up(d), up(np.array(w, WORK)), len(ps), len(w)


def launch(L, tab, stream=None):
    d, w, n, nw = tab
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    rc = L.mhaq_fq_radam_step(ctypes.c_void_p(d.data_ptr()), n, ctypes.c_void_p(w.data_ptr()), nw,
                              1 - BETA1, BETA2, 1 - BETA2, EPS, st)
    assert rc == 0, rc


def bench_parameters(dev):
    """The student's parameters as bench.py's trainer holds them (same model, quantizer and memory format)."""
    from mhaq_amd import nets
    from mhaq_amd.enums import QNMethod, QScheme
    from mhaq_amd.wrap import quantize_model
    torch.manual_seed(1234)
    net = nets.resnet18(1000).to(dev)
    quantize_model(net, QScheme.PER_CHANNEL, QNMethod.AEWGS, ("conv1", "fc"), False, 1)
    net = net.to(dev).to(memory_format=torch.channels_last)
    return [p for p in net.parameters() if p.requires_grad]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lib", action="append", default=[], metavar="LABEL=PATH")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    libs = [("product", _lib.lib())] + [(s.split("=", 1)[0], load(s.split("=", 1)[1])) for s in args.lib]
    ps = bench_parameters(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    like = lambda p: torch.empty_like(p, memory_format=torch.preserve_format)      # noqa: E731
    g0 = [like(p).copy_(torch.randn(p.shape, device=dev, generator=gen) * 1e-2) for p in ps]
    nelem = sum(p.numel() for p in ps)
    # the state after 7 steps of torch's optimizer: rho_t > 5, the rectified branch every later step takes
    for p, g in zip(ps, g0):
        p.grad = g.clone(memory_format=torch.preserve_format)
    opt = torch.optim.RAdam(ps, lr=3e-4, betas=(BETA1, BETA2), eps=EPS, foreach=True)
    for _ in range(7):
        opt.step()
    c1, c2 = optim.radam_scalars(8.0, 3e-4, BETA1, BETA2)
    snap = lambda ts: [t.detach().clone(memory_format=torch.preserve_format) for t in ts]      # noqa: E731
    ms, vs = [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps]
    s0 = (snap(ps), snap(ms), snap(vs))

    def restore():
        with torch.no_grad():
            for dst, src in zip((ps, ms, vs), s0):
                torch._foreach_copy_(dst, src)

    # step 8 with torch, then with every library from the same state: equal bits
    opt.step()
    want = (snap(ps), snap(ms), snap(vs))
    gs = [p.grad for p in ps]
    notes = []
    for label, L in libs:
        restore()
        launch(L, tables(L, [p.detach() for p in ps], gs, ms, vs, c1, c2))
        torch.cuda.synchronize()
        same = all(torch.equal(a.detach().view(torch.int32), b.view(torch.int32))
                   for got, ref in zip((ps, ms, vs), want) for a, b in zip(got, ref))
        notes.append(f"{label}: p, exp_avg, exp_avg_sq after step 8 are torch's bits: {same}")
        print(notes[-1], flush=True)
        assert same, label
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    tabs = {label: tables(L, [p.detach() for p in ps], gs, ms, vs, c1, c2) for label, L in libs}

    def torch_step():
        for st in opt.state.values():
            st["step"].fill_(7.0)
        opt.step()

    def timed(fn, i, out):
        flush.fill_(float(i))
        with torch.no_grad():
            torch._foreach_copy_(gs, g0)
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(e) * 1e3)

    rows = {"torch foreach": []}
    rows.update({label: [] for label, _ in libs})
    for i in range(args.reps + 1):          # alternating: one call of every variant per round
        timed(torch_step, i, rows["torch foreach"])
        for label, L in libs:
            timed(lambda: launch(L, tabs[label]), i, rows[label])
    small = sum(1 for p in ps if p.numel() <= 512)
    head = (f"The optimizer step of the bench model in fp32 on one {torch.cuda.get_device_name(0)}, one call: {len(ps)} parameter "
            f"tensors ({small} of them of 1-512 elements),\n{nelem / 1e6:.2f} M elements, {tabs['product'][3]} blocks.  "
            f"torch.optim.RAdam(foreach=True).step() against the one launch of mhaq_fq_radam_step\n(product library and forced "
            f"cache policies: g = the gradient load, l = the loads of p / m / v, s = the stores; n = non-temporal,\np = default "
            f"policy), alternating; before every timed call a 1 GiB buffer is written and the gradients are rewritten;\n"
            f"{args.reps} timed calls after one warm-up, HIP events around the whole step.\n\n")
    lines = [f"{'variant':>16s} {'min us':>9s} {'med us':>9s} {'passes':>7s} {'GB':>6s} {'TB/s(min)':>10s}"]
    for label, t in rows.items():
        passes = 21 if label == "torch foreach" else 7
        gb = passes * 4 * nelem / 1e9
        lines.append(f"{label:>16s} {min(t):9.1f} {statistics.median(t):9.1f} {passes:7d} {gb:6.2f} {gb / min(t) * 1e3:10.2f}")
    best = min((min(t), label) for label, t in rows.items() if label != "torch foreach")
    verdict = (f"\nfused (product) < torch: {min(rows['product']) < min(rows['torch foreach'])} "
               f"({min(rows['torch foreach']):.1f} -> {min(rows['product']):.1f} us, "
               f"{min(rows['torch foreach']) - min(rows['product']):.1f} us per step); fastest policy: {best[1]}\n")
    text = head + "\n".join(notes) + "\n\n" + "\n".join(lines) + "\n" + verdict
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
