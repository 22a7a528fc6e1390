"""bench.py on the GPU at a small size: a plain run prints the headline alone, `--steps` is the number of timed steps,
and `--dump-outputs` writes what the last timed step computed -- the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("--n", "1000", "--lightcurves", "16", "--walkers", "64", "--steps", "3", "--warmup", "1")


def _bench(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SMALL, *args],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [json.loads(s) for s in res.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_what_it_computed(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path / "a"))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "evals/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["cpu_baseline"] is None
    for side in ("end_to_end", "clock_under_load", "other_configs", "workflow_config3", "config2_raw_kernel"):
        assert side not in line, side
    lnp, status = np.load(tmp_path / "a" / "loglike.npy"), np.load(tmp_path / "a" / "status.npy")
    assert lnp.dtype == np.float64 and status.dtype == np.float32 and lnp.shape == status.shape == (16 * 64,)
    ok = status == 0
    assert ok.sum() >= lnp.size // 2 and np.all(np.isfinite(lnp[ok])) and np.all(lnp[~ok] == -np.inf)
    # the same arguments: the same inputs, the same outputs
    _bench("--dump-outputs", str(tmp_path / "b"))
    for name in ("loglike", "status"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))), name
