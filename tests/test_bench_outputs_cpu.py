"""CPU: bench.py offers --full and --dump-outputs, and the writer behind --dump-outputs (bench.dump_outputs) stores the
loss, every parameter and the gradients -- zeros for a parameter without one -- as float32, in parameter order, or a
fixed sample of them in position order beyond its caps.  Run in a child process: importing bench seeds MIOpen's user
find-db into the environment of the importing process."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import os, sys
import torch
sys.path.insert(0, sys.argv[1])
import bench
out, bench.DUMP_PARAM_ELEMS, bench.DUMP_GRAD_ELEMS = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
net = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 5), torch.nn.Linear(5, 3))
n0 = 0
with torch.no_grad():
    for i, p in enumerate(net.parameters()):
        p.copy_(torch.arange(n0, n0 + p.numel(), dtype=torch.float32).view_as(p))   # value = flat position
        if i != 4:                                                                 # net[2].weight: no gradient
            p.grad = -p.detach().clone()
        n0 += p.numel()
for d in ("a", "b"):
    bench.dump_outputs(os.path.join(out, d), net, torch.tensor(1.25))
"""
N = 40 * 30 + 30 + 30 * 5 + 5 + 5 * 3 + 3
NO_GRAD = range(40 * 30 + 30 + 30 * 5 + 5, 40 * 30 + 30 + 30 * 5 + 5 + 5 * 3)


def _dump(tmp_path, kp, kg):
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path), str(kp), str(kg)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    runs = []
    for d in ("a", "b"):
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["grads_sample.npy", "loss.npy", "params.npy"]
        arrays = {f[:-4]: np.load(tmp_path / d / f) for f in files}
        assert all(a.dtype == np.float32 and a.ndim == 1 for a in arrays.values())
        runs.append(arrays)
    for k in runs[0]:                       # the same positions every time
        assert np.array_equal(runs[0][k], runs[1][k]), k
    return runs[0]


def test_bench_offers_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_writes_every_parameter_and_gradient_in_order(tmp_path):
    a = _dump(tmp_path, 10 ** 6, 10 ** 6)
    assert np.array_equal(a["loss"], np.array([1.25], dtype=np.float32))
    assert np.array_equal(a["params"], np.arange(N, dtype=np.float32))
    want = -np.arange(N, dtype=np.float32)
    want[NO_GRAD.start:NO_GRAD.stop] = 0
    assert np.array_equal(a["grads_sample"], want)


def test_dump_outputs_samples_fixed_positions_beyond_the_caps(tmp_path):
    a = _dump(tmp_path, 100, 50)
    p, g = a["params"], a["grads_sample"]
    assert p.size == 100 and g.size == 50
    assert np.all(np.diff(p) > 0) and p[0] >= 0 and p[-1] < N and np.array_equal(p, np.round(p))
    nz = g[g != 0]
    assert np.all(np.diff(nz) < 0) and nz.min() > -N and np.array_equal(nz, np.round(nz))
