"""CPU: bench.py's N > 1 launch path exactly as the driver starts it (`python -m torch.distributed.run --nnodes=1
--nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...`), 8 ranks over gloo, before any
GPU call: `--dry-run` swaps PSMNet for a stand-in model (the HIP kernels have no CPU fallback) and keeps everything
else -- rendezvous from the environment, the world-size / backend assertions, per-rank data, DDP wrap, barrier +
max-over-ranks timing, rank 0's single JSON line."""
import json
import os
import socket
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n", [8])
def test_bench_launch_path_eight_ranks_gloo(n):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(REPO, "bench.py"), "--gpus", str(n),
           "--steps", "3", "--warmup", "1", "--dry-run", "--dist-backend", "gloo"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, env=env, timeout=540)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["steps"] == 3 and out["warmup"] == 1
    assert out["config"]["global_batch"] == 4 * n and out["config"]["parallelism"] == f"dp{n}"
    assert out["config"]["dist_backend"] == "gloo" and out["scaling"] == "weak"
    assert out["replicas_in_sync"] and out["ranks_drew_distinct_data"]
    assert out["vs_baseline"] is None and "dry_run" in out and out["value"] > 0


def test_bench_refuses_a_world_size_that_does_not_match_gpus():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--dry-run", "--dist-backend", "gloo"],
                       capture_output=True, text=True, cwd=REPO, env={k: v for k, v in os.environ.items()
                                                                      if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def _dry_run_dump(path, steps=2, warmup=1):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dry-run", "--dist-backend", "gloo", "--dump-outputs", str(path)],
                       capture_output=True, text=True, cwd=REPO, env=dict(env, OMP_NUM_THREADS="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0
    return out


def test_bench_dump_outputs_are_float32_and_repeatable(tmp_path):
    """--dump-outputs: what the last timed step computed, as float32 .npy files, the same from run to run"""
    import numpy as np

    a, b = _dry_run_dump(tmp_path / "a"), _dry_run_dump(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "grads.npy", "out0.npy"} <= set(names)
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
    assert np.load(tmp_path / "a" / "loss.npy")[0] == np.float32(a["loss"])
    assert a["loss"] == b["loss"]


def test_bench_steps_all_start_from_the_initial_state(tmp_path):
    """every warm-up and timed step is the same training step from the same model and optimizer state: the last of
    five steps computes exactly what a single step does"""
    import numpy as np

    one, five = _dry_run_dump(tmp_path / "one", 1, 0), _dry_run_dump(tmp_path / "five", 3, 2)
    assert one["loss"] == five["loss"]
    for n in sorted(os.listdir(tmp_path / "one")):
        np.testing.assert_array_equal(np.load(tmp_path / "one" / n), np.load(tmp_path / "five" / n), err_msg=n)


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    """arrays over the budget are written as a fixed sample of their elements; the small ones whole"""
    import numpy as np
    import torch

    monkeypatch.syspath_prepend(REPO)
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET", 1000)
    arrays = {"small": torch.arange(10.0), "big": torch.arange(5000.0).reshape(50, 100),
              "bigger": torch.arange(8000, dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    small, big, bigger = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("small", "big", "bigger"))
    assert small.dtype == big.dtype == bigger.dtype == np.float32
    np.testing.assert_array_equal(small, np.arange(10.0))
    assert big.size + bigger.size + small.size <= 1000 and big.size == 495 and bigger.size == 495
    assert (np.diff(big) > 0).all() and set(big) <= set(np.arange(5000.0))  # ascending picks of the flat elements
    for n in ("big", "bigger"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy"))
