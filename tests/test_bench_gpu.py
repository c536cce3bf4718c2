"""bench.py at one process on the toy shape (64x64, B=2): a plain run times the steps and prints
the headline figures only, `--dump-outputs` writes the last timed step's outputs as float32
.npy files, and `--full` adds the roofline, CPU-baseline and parity records."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
           "--res", "64", "--batch", "2", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_last_step_outputs(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "out"))
    assert all(k in d for k in HEADLINE)
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "bf16"
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) <= 1e-2 * d["value"]     # images/s = B / step time
    # a plain run measures nothing beside the timed steps
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["parity"] is None
    files = sorted(glob.glob(str(tmp_path / "out" / "*.npy")))
    assert [os.path.basename(f) for f in files] == ["K.npy", "R.npy", "logstd.npy", "mu.npy", "params.npy", "y.npy"]
    arrs = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    assert arrs["y"].size == 2 * 3 * 64 * 64 and 0.0 <= arrs["y"].min() and arrs["y"].max() <= 1.0
    assert arrs["mu"].size == arrs["logstd"].size
    # the line's last loss is the weighted sum of the dumped terms (w_R = w_K = 1)
    assert abs(d["loss_last"] - (arrs["R"][0] + arrs["K"][0])) <= 1e-5 * abs(d["loss_last"])


def test_bench_full_run_adds_roofline_baseline_and_parity():
    d = _bench("--full", "--cpu-seconds", "0.5")
    assert all(k in d for k in HEADLINE)
    assert d["roofline"]["avg_ms"] > 0 and set(d["roofline"]["families_avg_ms"]) == {"fwd", "dgrad", "wgrad"}
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["unit"] == "images/s"
    # bf16 kernels against the fp32 oracle on the first step.  The record must be a comparison of
    # the same step, not a tight gate (that is tests/test_model_gpu.py in fp32 mode): bf16 storage
    # rounds each activation by up to 2^-8 = 3.9e-3 relative, so a few roundings' worth (5 x 2^-8
    # = 2e-2) bounds the image, and the losses, means over >= 24k elements, stay well inside 1e-2
    assert d["parity"]["image_rel_l2"] < 2e-2 and d["parity"]["R_rel"] < 1e-2 and d["parity"]["K_rel"] < 1e-2
