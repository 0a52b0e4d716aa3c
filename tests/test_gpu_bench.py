"""bench.py's plain run (no --full): the headline line alone, what --dump-outputs writes, and at most 30 s of the run
outside its warm-up and timed steps.  Everything else the benchmark measures or checks is --full's."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("mean_nll_nats", "roofline", "kernels_in_step_us", "roofline_whole_step", "inverse", "inverse_samples_per_sec",
             "cpu_baseline", "nll_trained_weights", "nll_check", "nll_rel_err", "other_workloads", "extra")


def test_plain_run_prints_the_headline_alone(tmp_path):
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=240)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert (res["metric"], res["unit"], res["higher_is_better"], res["dtype"]) == ("train_samples_per_sec", "samples/s", True, "f32")
    assert (res["steps"], res["warmup"], res["n_gpus"]) == (steps, warmup, 1)
    assert res["value"] == pytest.approx(4096 * 1e3 / res["ms_per_step"], rel=1e-9)
    assert not set(FULL_ONLY) & set(res), sorted(set(FULL_ONLY) & set(res))
    arrays = {name: np.load(tmp_path / f"{name}.npy") for name in res["dumped_outputs"]["elements"]}
    assert sorted(arrays) == ["loss_terms", "parameters"]
    assert all(a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all() for a in arrays.values())
    outside = wall - (steps + warmup) * res["ms_per_step"] * 1e-3
    assert outside < 30.0, f"{outside:.1f} s outside the warm-up and timed steps"
