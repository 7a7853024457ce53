"""bench.py's command line on a box without a GPU: `--gpus N > 1` started plainly becomes its own launcher (one rank per GPU under torch.distributed.run) instead of
exiting on argument checking; the ranks then refuse to run without an MI355X — the product has no CPU path (the GPU twin: tests/test_gpu_parity.py::
test_two_rank_bench_rehearsal_on_one_gpu[plain])."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(torch.cuda.is_available(), reason="the GPU rehearsal covers the launch on a GPU box")
def test_plain_multi_gpu_start_launches_its_own_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GO2_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--num-envs", "64"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode != 0                                                       # no GPU here: every rank refuses
    assert "needs torch.distributed.run" not in r.stderr                           # (round 5's exit on argument checking)
    assert r.stderr.count("bench.py needs an MI355X") >= 2, r.stderr[-3000:]       # two ranks were started and each one said so
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]          # and no number came out of a box without a GPU


def test_help_lists_full_and_dump_outputs():
    """--full (the measurements the headline does not need) and --dump-outputs DIR are part of the command line."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_iteration(tmp_path):
    """A plain run times exactly --steps iterations — counted inside the run by the runner's iteration counter and by the optimizer's Adam-step
    counter (5 epochs x 4 mini-batches per iteration) — measures nothing beyond the headline (no roofline, no cpu_baseline), and --dump-outputs
    writes the last timed iteration's arrays: float32 / float64 .npy files, finite, at most 64 MB in all."""
    import json

    import numpy as np
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "5", "--num-envs", "2048",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 5 and out["ms_per_step"] > 0
    assert out["timed_iterations"] == 3 and out["timed_adam_steps"] == 3 * 5 * 4
    assert abs(out["value"] - 2048 * 24 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert "roofline" not in out and "cpu_baseline" not in out
    files = {f.name: np.load(f) for f in out_dir.glob("*.npy")}
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    k = len(files["env_index.npy"])
    assert k == 1024 and files["storage.actions.npy"].shape == (24, k, 12) and files["env.obs_buf.npy"].shape == (k, 45)
    assert files["policy.actor.0.weight.npy"].shape == (512, 45)
