"""GPU (-m gpu): a plain `bench.py --gpus 1` run times the training steps and nothing else -- the keys of the --full
legs stay null -- and `--dump-outputs DIR` leaves what its last timed step computed: the loss on the line, every
parameter of the student and a sample of that step's gradients, float32, within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_times_the_steps_alone_and_dumps_the_last_one(tmp_path):
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "8", "--image", "64", "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True,
                       text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "qat_images_per_sec" and out["unit"] == "images/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["steps"] == 3 and out["warmup"] == 1 and out["full"] is False
    assert abs(out["value"] - 8 * 3 / (out["ms_per_step"] * 3e-3)) <= 0.01 * out["value"]
    for k in ("roofline", "roofline_set", "configs", "cpu_baseline", "gpu_eager_baseline"):
        assert out[k] is None, k
    assert "kernel roofline leg" not in r.stderr and "baseline" not in r.stderr
    files = sorted(os.listdir(out_dir))
    assert files == ["grads_sample.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64e6
    a = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["loss"].shape == (1,) and round(float(a["loss"][0]), 5) == out["config"]["final_loss"]
    assert 11_000_000 < a["params"].size <= 12 << 20                 # ResNet-18 + its quantizers, every element
    assert a["grads_sample"].size == 2 << 20 and np.count_nonzero(a["grads_sample"]) > 0
