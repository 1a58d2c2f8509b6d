"""-m gpu: `bench.py` as a command.  A plain run prints the headline line alone and, with --dump-outputs, the arrays of its
last timed step; --full adds the other measurements on top of the same timed run (same inputs, same result)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--nodes", "20000", "--avg_degree", "40"]
FULL_ONLY = ("ms_per_step_events", "roofline", "roofline_step", "cpu_baseline", "micro_f1", "aux")


def _bench(extra):
    env = dict(os.environ, GS_FAULT_DUMP_S="280")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_run_adds_to_it(dev, tmp_path):
    a, b = str(tmp_path / "plain"), str(tmp_path / "full")
    d = _bench(["--dump-outputs", a])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["unit"] == "sampled-edges/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 6 and d["ms_per_step"] > 0
    assert abs(d["value"] - 512 * (10 + 10 * 25) / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(a)) == ["loss.npy", "params.npy", "preds.npy"]
    out = {k: np.load(os.path.join(a, k + ".npy")) for k in ("loss", "params", "preds")}
    assert out["preds"].shape == (512, 41) and out["preds"].dtype == np.float32 and out["params"].dtype == np.float32
    assert float(out["loss"]) == d["config"]["loss_after"] and np.isfinite(out["params"]).all()

    f = _bench(["--dump-outputs", b, "--full", "--no-cpu-baseline", "--no-aux"])
    assert "ms_per_step_events" in f and "roofline" in f and "roofline_step" in f
    assert f["steps"] == 6 and f["warmup_steps_run"] == d["warmup_steps_run"]
    for k in ("loss", "params", "preds"):
        np.testing.assert_allclose(np.load(os.path.join(b, k + ".npy")), out[k], rtol=1e-5, atol=1e-6, err_msg=k)
