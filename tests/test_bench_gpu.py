"""bench.py end to end on the tiny preset: a plain run prints the headline line only and --dump-outputs writes what the
last timed step returned; --full adds the in-situ kernel figures and the CPU baseline and times the same steps; two runs
with the same arguments write the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ("--preset", "tiny", "--batch", "4", "--text-len", "24", "--steps", "3", "--warmup", "1")


def _run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env,
                       timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _dumped(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("loss", "decoded")}


@pytest.mark.timeout(300)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out_dir = str(tmp_path / "out")
    line = _run(*SMALL, "--dump-outputs", out_dir)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - 4 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-2  # 4 trajectories per step
    assert not {"roofline", "kernels", "cpu_baseline"} & set(line)

    d = _dumped(out_dir)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in d.values())
    assert d["decoded"].shape[0] == 4
    assert abs(float(d["loss"]) - line["loss_last_timed_step"]) <= 1e-3 * abs(line["loss_last_timed_step"]) + 1e-3


@pytest.mark.timeout(600)
def test_full_run_adds_its_figures_after_the_same_steps(tmp_path):
    # forward mode: no optimizer in the loop, so the two runs' last timed steps are comparable tightly
    plain_dir, full_dir = str(tmp_path / "plain"), str(tmp_path / "full")
    _run(*SMALL, "--mode", "forward", "--dump-outputs", plain_dir)
    full = _run(*SMALL, "--mode", "forward", "--full", "--cpu-warm", "1", "--cpu-timed", "1", "--dump-outputs", full_dir)
    assert {"roofline", "kernels", "cpu_baseline"} <= set(full)
    assert full["roofline"]["achieved"] > 0 and full["cpu_baseline"]["value"] > 0
    assert full["cpu_baseline"]["parity_full_size"]["decoded_rel_err"] < 1e-2
    p, f = _dumped(plain_dir), _dumped(full_dir)
    assert f["decoded"].shape == p["decoded"].shape
    assert np.linalg.norm(f["decoded"] - p["decoded"]) <= 1e-5 * np.linalg.norm(p["decoded"])
    assert abs(float(f["loss"]) - float(p["loss"])) <= 1e-5 * abs(float(p["loss"]))


@pytest.mark.timeout(600)
def test_same_arguments_give_the_same_outputs(tmp_path):
    # the default train step (MLLM frozen): every reduction of its backward runs in a fixed order, so the optimizer steps
    # (and with them the last timed step's outputs) are bit-identical from run to run
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    _run(*SMALL, "--dump-outputs", a_dir)
    _run(*SMALL, "--dump-outputs", b_dir)
    a, b = _dumped(a_dir), _dumped(b_dir)
    for n in a:
        assert np.array_equal(a[n], b[n]), n
