"""bench.py's launch contract, the part that can be checked without a GPU: `--gpus N` with no launcher around starts N
ranks of itself only when the box has N devices, and never reports a one-rank run as an N-GPU one.
On a GPU: a plain run does exactly the requested solves, reports only the headline and writes the last solve's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, drop=()):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)


def test_refuses_n_ranks_on_fewer_devices():
    r = _run(["--gpus", "2", "--steps", "1"], drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRIMME_AMD_BENCH_SHARE_GPU"))
    assert r.returncode != 0
    assert "refusing" in r.stderr and "--gpus 2" in r.stderr
    assert r.stdout.strip() == ""               # no JSON line that could be mistaken for a measurement


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "2", "--steps", "1"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    assert r.stdout.strip() == ""


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr
    assert r.stdout.strip() == ""


@pytest.mark.gpu
def test_plain_run_times_the_requested_steps_and_dumps_the_last_solve(built, tmp_path):
    from primme_amd import problems
    out = tmp_path / "outputs"
    r = _run(["--gpus", "1", "--workload", "lap3d_small", "--steps", "2", "--warmup", "0", "--dump-outputs", str(out)],
             drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "PRIMME_AMD_BENCH_DIST"))
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 2 and line["warmup"] == 0 and line["ms_per_step"] > 0
    for key in ("roofline", "configs1", "configs2", "configs3", "configs4", "cpu_baseline"):
        assert key not in line                  # what a plain run does not measure
    evals, res = np.load(out / "evals.npy"), np.load(out / "resNorms.npy")
    assert evals.dtype == np.float64 and res.dtype == np.float64 and evals.shape == res.shape == (10,)
    exact = problems.laplacian_eigenvalues((60, 61, 62), 10)
    assert np.max(np.abs(np.sort(evals) - exact)) <= 1e-6 * 12.0
    assert np.all(res <= 1e-8 * 12.0 * (1 + 1e-12))
