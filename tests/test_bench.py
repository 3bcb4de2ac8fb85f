"""``bench.py``'s command line: a plain run prints the headline line only and ``--steps`` steps are timed;
``--dump-outputs`` writes what the last timed step computed; ``--full`` adds the roofline blocks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_hbm", "roofline_hbm_conv", "roofline_hbm_convs", "fp32_reference_arithmetic",
             "cpu_baseline")


def _bench(argv, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + argv, env=env, capture_output=True, text=True,
                       timeout=timeout)
    return r, [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_refuses_zero_steps():
    r, _ = _bench(["--steps", "0", "--dry-launch"])
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_plain_line_and_dump(tmp_path):
    r, lines = _bench(["--config", "C1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(lines) == 1
    out = lines[0]
    assert all(k in out for k in HEADLINE) and out["steps"] == 2 and out["ms_per_step"] > 0
    assert not any(k in out for k in FULL_ONLY)
    files = sorted(os.listdir(tmp_path))
    assert {"G_state.npy", "D_state.npy", "loss_G_total.npy", "loss_D_train_loss.npy"} <= set(files)
    total = 0
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "G_state.npy").size == 1 << 22  # 34.77M weights: the seeded sample


@pytest.mark.gpu
def test_bench_full_adds_rooflines():
    r, lines = _bench(["--config", "C1", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert r.returncode == 0, r.stderr[-3000:]
    out = lines[0]
    assert all(k in out for k in HEADLINE)
    assert out["roofline"]["launches_timed"] > 0 and out["roofline_hbm"]["launches_timed"] > 0
    assert "cpu_baseline" not in out
