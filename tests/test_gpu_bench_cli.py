"""bench.py as it is called: a plain run prints the headline line and nothing it needs extra runs or events for, two plain runs
with the same arguments dump the same outputs bit for bit, and --full still adds the roofline, the boundary legs and the CPU
baseline.  Short loops (4 denoise steps) keep each run to seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
SHORT = ["--gpus", "1", "--warmup", "1", "--denoise-steps", "4"]


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SHORT, *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_runs_dump_identical_outputs(tmp_path):
    lines = [run_bench("--steps", "2", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "clips/s" and line["higher_is_better"] is True
        assert line["metric"].startswith("denoised motion clips/sec") and line["dtype"]
        assert not {"roofline", "boundary", "cpu_baseline"} & set(line), sorted(line)
    a, b = (np.load(tmp_path / d / "sample.npy") for d in ("a", "b"))
    assert a.dtype == np.float32 and a.shape == (64, 263, 1, 196)
    assert np.isfinite(a).all() and np.array_equal(a, b)


def test_full_run_keeps_the_extras():
    line = run_bench("--steps", "1", "--full", "--cpu-sample-steps", "2")
    assert line["roofline"]["families"] and line["roofline"]["kernel"]
    assert line["boundary"]["philox_noise_clips_per_s"] > 0 and line["boundary"]["torch_noise_clips_per_s"] > 0
    assert line["cpu_baseline"]["value"] > 0
