"""bench.py's plain run: the headline figure only, exactly --steps timed steps, and --dump-outputs (what the last timed step returned
to its caller, the same from run to run with the same arguments).  The legs behind --full are exercised by test_gpu_distributed.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
DUMPED = ["done", "done_reason", "episode_length", "episode_return", "obs", "reward", "terminal_obs"]


def _result_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_offers_full_and_dump_outputs():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    steps, warmup, n = 600, 8, 65536          # 600 = one 512-step graph + a remainder graph
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(d)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        runs.append((_result_line(p.stdout), d))
    out = runs[0][0]
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert out["unit"] == "env steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["region_ms"]["device"] == pytest.approx(out["ms_per_step"] * steps, rel=1e-9)
    for leg in ("cpu_baseline", "f64_storage", "large_n", "config4_global_batch_on_one_gpu", "open_loop_multi_step",
                "config1_single_env_gym_object", "policy_rollout", "vecenv_numpy_boundary"):
        assert leg not in out, leg            # --full only
    total = 0
    for name in DUMPED:
        a, b = (np.load(os.path.join(d, name + ".npy")) for _, d in runs)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.testing.assert_array_equal(a, b, err_msg=name)
        total += os.path.getsize(os.path.join(runs[0][1], name + ".npy"))
    assert sorted(f for f in os.listdir(runs[0][1])) == [x + ".npy" for x in DUMPED]
    assert total <= 64 * 10**6
    d = runs[0][1]
    obs, done, term = (np.load(os.path.join(d, x + ".npy")) for x in ("obs", "done", "terminal_obs"))
    assert obs.shape == (n, 17) and np.isfinite(obs).all()
    assert set(np.unique(done)) <= {0.0, 1.0} and done.any()
    assert not term[done == 0].any()
