#!/usr/bin/env python3
"""Mixed-precision (bf16 autocast) figures on one GPU; prints ONE JSON line (profiles/r07_amp.txt holds a run).

  kernels  the 16-bit activation fake-quant (mhaq_fq_act_fwd_x16 / mhaq_fq_act_bwd_partials_x16, STE with in-kernel signs)
           on the dominant ResNet-18 activation [250,64,56,56] channels_last, bf16, timed by HIP events (median of --reps),
           next to the fp32 kernels on the same tensor; fraction of 8 TB/s at 4 B/elem (forward: 2 B read + 2 B written)
           and 6 B/elem (backward: x and g read, gx written)
  step     the ResNet-18 batch-250 QAT step of BASELINE configs[3] (AEWGS weights, STE activations, distillation, RAdam)
           in fp32 and under bf16 autocast (QATConfig.autocast_dtype), eager and captured (hipGraph), in images/s

Convolution algorithms: MIOpen in immediate mode (torch.backends.cudnn.benchmark = False) for every leg, so that no leg
pays MIOpen's per-shape search -- minutes per fresh box for the bf16 shapes, which mhaq_amd/miopen_db/ does not cover.
The fp32 legs read the recorded fp32 winners of that database as bench.py does; the bf16 legs take MIOpen's heuristic
choice.  bench.py stays the headline measurement; this tool does not change it.
usage: tools/amp_bench.py [--steps K] [--warmup W] [--reps R] [--no-step]"""
import argparse
import glob
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seed_miopen_db():
    """A private writable copy of mhaq_amd/miopen_db/ (bench.py seed_miopen_user_db), before torch touches MIOpen."""
    if "MIOPEN_USER_DB_PATH" in os.environ:
        return None
    files = glob.glob(os.path.join(ROOT, "mhaq_amd", "miopen_db", "*.txt"))
    if not files:
        return None
    dst = tempfile.mkdtemp(prefix="mhaq_amp_miopen_")
    for f in files:
        shutil.copy(f, dst)
    os.environ["MIOPEN_USER_DB_PATH"] = dst
    import atexit
    atexit.register(shutil.rmtree, dst, ignore_errors=True)
    return dst


DB = seed_miopen_db()

import torch  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2]


def kernels(dev, reps):
    from mhaq_amd import _lib, ops
    L = _lib.lib()
    st = ops._stream
    shape = (250, 64, 56, 56)
    n = 250 * 64 * 56 * 56
    gen = torch.Generator(device=dev).manual_seed(3)
    x32 = (torch.randn(shape, device=dev, generator=gen) * 2).contiguous(memory_format=torch.channels_last)
    g32 = torch.randn(shape, device=dev, generator=gen).contiguous(memory_format=torch.channels_last)
    ls = torch.tensor([-3.0], device=dev)
    lq = torch.tensor([2.0], device=dev)
    b = torch.tensor([-2.0], device=dev)
    params = torch.empty(5, device=dev)
    nb = L.mhaq_fq_act_bwd_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    npart = _lib.C.c_int32(0)
    out = {"tensor": "[250,64,56,56] channels_last", "elements": n, "reps": reps}
    for name, x, g, dt in (("bf16", x32.bfloat16(), g32.bfloat16(), _lib.DT_BF16), ("fp32", x32, g32, 0)):
        y = torch.empty_like(x)
        gx = torch.empty_like(x)
        if dt:
            fwd = lambda: _lib.check(L.mhaq_fq_act_fwd_x16(  # noqa: E731
                x.data_ptr(), y.data_ptr(), n, dt, ls.data_ptr(), lq.data_ptr(), b.data_ptr(), params.data_ptr(),
                None, None, None, 0, st()), "fwd")
            bwd = lambda: _lib.check(L.mhaq_fq_act_bwd_partials_x16(  # noqa: E731
                x.data_ptr(), g.data_ptr(), gx.data_ptr(), n, dt, params.data_ptr(), 0, None, 7, 1, None,
                ws.data_ptr(), nb, _lib.C.byref(npart), st()), "bwd")
        else:
            fwd = lambda: _lib.check(L.mhaq_fq_act_fwd(  # noqa: E731
                x.data_ptr(), y.data_ptr(), n, ls.data_ptr(), lq.data_ptr(), b.data_ptr(), params.data_ptr(),
                None, None, None, 0, st()), "fwd")
            bwd = lambda: _lib.check(L.mhaq_fq_act_bwd_partials(  # noqa: E731
                x.data_ptr(), g.data_ptr(), gx.data_ptr(), n, params.data_ptr(), 0, None, 7, 1, None,
                ws.data_ptr(), nb, _lib.C.byref(npart), st()), "bwd")
        esz = x.element_size()
        tf, tb = timed(fwd, reps), timed(bwd, reps)
        out[name] = {"fwd_us": round(tf, 2), "bwd_us": round(tb, 2),
                     "fwd_frac_peak": round(2 * esz * n / (tf * 1e-6) / PEAK, 3),
                     "bwd_frac_peak": round(3 * esz * n / (tb * 1e-6) / PEAK, 3),
                     "bytes_per_elem": {"fwd": 2 * esz, "bwd": 3 * esz}}
    return out


def step(dev, autocast, capture, steps, warmup, batch=250, image=224):
    from mhaq_amd import nets, ops
    from mhaq_amd.enums import QNMethod, QScheme
    from mhaq_amd.qat import QATConfig, QATTrainer
    torch.manual_seed(1234)
    ops.manual_seed(1234)
    cfg = QATConfig(qscheme=QScheme.PER_CHANNEL, qnmethod=QNMethod.AEWGS, distillation=True,
                    autocast_dtype=torch.bfloat16 if autocast else None)
    gen = torch.Generator(device=dev).manual_seed(100)
    net = nets.resnet18(1000).to(memory_format=torch.channels_last)
    x = torch.randn(batch, 3, image, image, device=dev, generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (batch,), device=dev, generator=gen)
    calib = torch.randn(64, 3, image, image, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    calib = calib.contiguous(memory_format=torch.channels_last)
    tr = QATTrainer(net, cfg, dev, calib_batches=[calib], capture_graph=capture)
    for _ in range(warmup):
        tr.train_step(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = tr.train_step(x, y)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    res = {"ms_per_step": round(dt * 1e3, 2), "images_per_s": round(batch / dt, 1), "loss": float(loss),
           "captured": tr._graph is not None}
    del tr
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cudnn.benchmark = False
    rec = {"tool": "amp_bench", "device": torch.cuda.get_device_name(0), "miopen": "immediate mode (no search)",
           "kernels": kernels(dev, args.reps)}
    if not args.no_step:
        legs = {}
        for name, ac, cap in (("fp32_eager", False, False), ("bf16_eager", True, False),
                              ("fp32_captured", False, True), ("bf16_captured", True, True)):
            t0 = time.perf_counter()
            legs[name] = step(dev, ac, cap, args.steps, max(args.warmup, 4 if cap else 1))
            print(f"[amp_bench] {name}: {legs[name]} ({time.perf_counter() - t0:.0f} s)", file=sys.stderr, flush=True)
        legs["bf16_over_fp32_eager"] = round(legs["bf16_eager"]["images_per_s"] / legs["fp32_eager"]["images_per_s"], 3)
        legs["bf16_over_fp32_captured"] = round(legs["bf16_captured"]["images_per_s"] /
                                                legs["fp32_captured"]["images_per_s"], 3)
        rec["resnet18_b250_step"] = legs
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
