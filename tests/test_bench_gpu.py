"""A plain bench.py run on the GPU: its result line and what --dump-outputs writes.  -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--scenes-per-gpu", "1",
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]          # 1 scene per step
    # a plain run carries no secondary leg
    for k in ("roofline", "cpu_baseline", "psnr_vs_oracle", "targets70", "latency_b1", "fast_path", "f32_path", "train"):
        assert line[k] is None, k
    files = sorted(os.listdir(d))
    assert {"color.npy", "depth.npy", "gaussians_means.npy", "pred_extrins.npy", "raw_gaussians.npy"} <= set(files), files
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    for f in files:
        a = np.load(d / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    c = np.load(d / "color.npy")
    assert c.size == 1 << 18 and c.std() > 0        # a seeded sample of the 12 rendered views
