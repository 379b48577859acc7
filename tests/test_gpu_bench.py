"""bench.py's plain run on the GPU, on the smallest scene: the line's fields, the legs that wait
for --full, and --dump-outputs against the engine driven directly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bh_amd
from bh_amd import scenes
from conftest import bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("x", "y", "vx", "vy", "m")


def test_plain_run_times_the_steps_and_dumps_their_final_state(tmp_path):
    """`--steps 3 --warmup 1 --dump-outputs DIR` on c1_baseline: the line says what it timed and
    carries none of --full's legs; DIR/<field>.npy is, bit for bit, the state after
    bh_step(1) + bh_step(3) of the same seeded scene."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config",
                        "c1_baseline", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "body-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["ms_per_step"] > 0 and line["value"] > 0
    n = line["config"]["n_bodies"]
    # value = bodies x steps / elapsed and ms_per_step = elapsed / steps describe the same interval
    # (the merge rule may remove a few of the n bodies during it; both figures are rounded)
    assert 0.9 < line["value"] * line["ms_per_step"] * 1e-3 / n <= 1.001
    for leg in ("roofline", "cpu_baseline", "verify"):
        assert line[leg] is None, leg
    assert "drop_in" not in line

    eng = bh_amd.Engine(bh_amd.default_params(theta=0.5), device=0)
    eng.reset_bodies(*scenes.config_scene("c1_baseline"))
    eng.step(1)
    eng.step(3)
    want = eng.get_bodies()
    eng.close()
    assert sorted(os.listdir(out)) == sorted(f + ".npy" for f in FIELDS)
    for f, w in zip(FIELDS, want):
        got = np.load(out / (f + ".npy"))
        assert got.dtype == np.float64 and bits_equal(got, w), f
