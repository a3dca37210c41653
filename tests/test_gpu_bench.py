"""bench.py on one GPU, tiny configuration: a plain run prints the headline line and nothing it does not need, --dump-outputs
writes what the last timed step computed (bit for bit the same in every run), --full adds the measurements a plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--model", "vit_tiny", "--batch", "8", "--img", "64"]
DUMPED = ["grads.npy", "loss.npy", "params.npy", "pred.npy", "targets.npy"]


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_dumps_its_last_timed_step_and_full_adds_the_rest(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    assert a["metric"] == "images_per_sec" and a["unit"] == "images/s" and a["higher_is_better"] is True and a["dtype"] == "bf16"
    assert a["steps"] == 3 and a["warmup"] == 1 and a["ms_per_step"] > 0
    assert abs(a["value"] - 8 * 1e3 / a["ms_per_step"]) <= 1e-3 * a["value"]
    assert a["roofline"] is None and a["cpu_baseline"] is None and "other_configs" not in a
    assert sorted(os.listdir(tmp_path / "a")) == DUMPED
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in DUMPED}
    assert got["loss"].dtype == np.float64 and got["loss"].shape == (1,)
    assert all(got[k].dtype == np.float32 and got[k].size > 0 for k in ("pred", "targets", "params", "grads"))
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert abs(got["loss"][0] - a["final_loss"]) <= 1e-5
    assert got["pred"].shape == got["targets"].shape and np.isfinite(got["params"]).all() and np.isfinite(got["grads"]).all()
    assert abs(float(np.abs(got["pred"] - got["targets"]).mean()) - got["loss"][0]) <= 1e-3 * got["loss"][0]

    b = _bench("--dump-outputs", str(tmp_path / "b"), "--full", "--no-cpu-baseline")
    assert b["roofline"] is not None and b["roofline"]["launches_per_step"] > 0
    for f in DUMPED:                                    # same inputs, and sums in a fixed order: the same bits in every run
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "a" / f)), f
