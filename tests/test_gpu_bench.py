"""bench.py's own launch paths on the GPU box (subprocesses, so the test process's GPU state is
not shared with the ranks):

* `--config C1` -- the reference train.py's Cityscapes default (R50, no pyramid module,
  512 x 1024, batch 2; BASELINE.json configs[0]) runs through the bench's training step and
  prints one JSON line with finite losses and the roofline object (the C1 config
  was never run by a test); the roofline is a `--full` leg;
* a plain run (no `--full`) with `--dump-outputs`: the side legs are left out and the last
  step's outputs are written as .npy files;
* `--gpus 2` without WORLD_SIZE -- bench.py starts its two rank processes itself (VERDICT r4
  item 2); on a one-GPU box the ranks share the device over gloo (SEG_BENCH_BACKEND=gloo), so
  the line must say n_gpus 2, a two-rank process group, and flag the roofline as invalid.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=400):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=env,
                       capture_output=True, text=True, timeout=timeout, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_bench_config_c1(cuda):
    d = _bench(["--config", "C1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
                "--no-train-py", "--no-eval"])
    assert d["n_gpus"] == 1 and d["config"]["image"] == [512, 1024]
    assert d["config"]["per_gpu_batch"] == 2 and "C1" in d["config"]["workload"]
    assert "NONE" in d["config"]["workload"]          # no pyramid module (train.py's default)
    assert all(v == v and abs(v) < 1e3 for v in d["losses_last_step"])
    assert d["value"] > 0 and d["roofline"]["frac"] > 0


@pytest.mark.timeout(600)
def test_bench_plain_run_dumps_outputs(cuda, tmp_path):
    """A plain run (no --full) times --steps steps, leaves every side leg out (their fields are
    null) and --dump-outputs writes the last step's outputs as float32 .npy files, 64 MB at
    the most in all, every value finite, the losses those of the result line."""
    import numpy as np
    out = tmp_path / "dump"
    d = _bench(["--gpus", "1", "--config", "C1", "--steps", "3", "--warmup", "1",
                "--dump-outputs", str(out)])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = images per second of the timed steps: batch 2 per step of ms_per_step
    assert abs(d["value"] * d["ms_per_step"] / 2e3 - 1) < 1e-2
    for leg in ("roofline", "cpu_baseline", "train_py", "eval", "miou_train_summary"):
        assert d[leg] is None, leg
    files = sorted(p.name for p in out.iterdir())
    assert files == ["ema.npy", "logits.npy", "losses.npy", "momentum.npy", "moving.npy",
                     "params.npy", "reg.npy"]
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert sum((out / f).stat().st_size for f in files) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype == np.float32 and a.size > 0 and np.all(np.isfinite(a)), name
    assert arrays["losses"].shape == (10,) and arrays["reg"].shape == (1,)
    np.testing.assert_allclose(arrays["losses"][:4], d["losses_last_step"], atol=1e-5)
    assert np.any(arrays["momentum"] != 0) and np.any(arrays["params"] != arrays["ema"])


@pytest.mark.timeout(900)
def test_bench_self_launches_two_ranks(cuda):
    d = _bench(["--gpus", "2", "--config", "C1", "--steps", "2", "--warmup", "1", "--full",
                "--no-eval", "--no-train-py", "--no-cpu-baseline"], {"SEG_BENCH_BACKEND": "gloo"})
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["comm"]["world_size"] == 2 and d["comm"]["backend"] == "gloo"
    assert d["comm"]["allreduce_bytes_per_step"] > 0 and d["comm"]["buckets"] >= 1
    assert d["roofline"]["frac"] is None and "share" in d["roofline"]["invalid"]
    assert all(v == v for v in d["losses_last_step"])
