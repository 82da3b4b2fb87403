"""bench.py without --full: only the headline is timed, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_times_the_headline_and_dumps_outputs(hip_lib, tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "lidar", "--batch", "1",
           "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "samples/s"
    for leg in ("bf16_mixed_precision", "roofline", "roofline_voxelize", "roofline_mfma_f32", "cpu_baseline", "host_enqueue"):
        assert leg not in line, leg
    names = sorted(os.listdir(out_dir))
    assert {"loss.npy", "param_sample.npy", "grad_sample.npy"} <= set(names), names
    total = 0
    for n in names:
        a = np.load(out_dir / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
    assert float(np.load(out_dir / "loss.npy")[0]) == line["config"]["final_loss"]
    assert np.abs(np.load(out_dir / "grad_sample.npy")).max() > 0
