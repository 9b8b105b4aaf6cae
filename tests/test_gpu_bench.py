"""bench.py as a command: the result line of a plain run and of --full, and --dump-outputs (what the last timed step
computed, identical from run to run for the same arguments). A 3-level 64^2 unet_bn at B=2 keeps each run to the
start-up cost of a process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--levels", "3", "--size", "64", "--batch", "2"]
PLAIN_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus",
              "config", "build", "train_loss"}
FULL_KEYS = {"roofline", "cpu_baseline", "dice_val"}


def _bench(cwd, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], cwd=cwd, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    cwd = tmp_path_factory.mktemp("bench")
    line = _bench(cwd, "--dump-outputs", str(cwd / "out_a"))
    return cwd, line


def test_plain_line_has_the_headline_and_no_extra_leg(plain_run):
    _, line = plain_run
    assert PLAIN_KEYS <= set(line) and not FULL_KEYS & set(line)
    assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == (
        "1024^2 tiles/sec (train)", "tiles/s", True, "bf16")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    # value = tiles of all timed steps / their time, in 1024^2-tile equivalents (both rounded in the line)
    tiles_per_step = 2 * (64 / 1024.0) ** 2
    assert line["value"] == pytest.approx(tiles_per_step / (line["ms_per_step"] * 1e-3), rel=1e-2)


def test_dump_outputs_files(plain_run):
    cwd, line = plain_run
    out = _load(cwd / "out_a")
    assert set(out) == {"main_out.npy", "param_grads.npy", "params.npy", "metrics.npy"}
    assert sum(os.path.getsize(cwd / "out_a" / f) for f in out) <= 64 << 20
    for f, a in out.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
    assert out["main_out.npy"].shape == (2, 64, 64)   # (below the sampling size: the whole head output)
    assert 0.0 <= out["main_out.npy"].min() and out["main_out.npy"].max() <= 1.0
    assert out["params.npy"].shape == out["param_grads.npy"].shape and np.abs(out["param_grads.npy"]).max() > 0
    assert round(float(out["metrics.npy"][0]), 5) == line["train_loss"]


def test_dump_outputs_repeat_for_the_same_arguments(plain_run):
    cwd, _ = plain_run
    _bench(cwd, "--dump-outputs", str(cwd / "out_b"))
    a, b = _load(cwd / "out_a"), _load(cwd / "out_b")
    assert set(a) == set(b)
    for f in a:
        assert np.array_equal(a[f], b[f]), f


def test_full_adds_the_roofline_and_honours_the_leg_switches(tmp_path):
    line = _bench(tmp_path, "--full", "--no-dice", "--no-cpu-baseline")
    assert PLAIN_KEYS | FULL_KEYS <= set(line)
    assert line["dice_val"] is None and line["cpu_baseline"] is None
    roof = line["roofline"]
    assert roof["kernel"] in roof["per_kernel"] and roof["launches"] > 0 and roof["achieved"] > 0
