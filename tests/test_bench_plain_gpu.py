"""A plain bench.py run (no --full) on one GPU: it prints the headline line only -- no roofline, peaks, traffic or
CPU baseline, which need runs of their own -- and --dump-outputs writes what the last timed step computed."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_plain_run_prints_headline_and_dumps_outputs(tmp_path):
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "4", "--dump-outputs", out]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["unit"] == "clips/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["steps"] == 3 and rec["n_gpus"] == 1 and rec["full"] is False
    assert rec["ms_per_step"] > 0 and math.isfinite(rec["loss"])
    # value and ms_per_step are the same measurement: clips per step / seconds per step
    assert rec["value"] == pytest.approx(4 / (rec["ms_per_step"] * 1e-3), rel=1e-2)
    for key in ("roofline", "peaks_measured", "cpu_baseline", "step_hbm_bytes"):
        assert key not in rec, key
    arrays = {n[:-4]: np.load(os.path.join(out, n)) for n in sorted(os.listdir(out))}
    assert set(arrays) == {"loss", "grad", "params", "sample_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    assert arrays["grad"].shape == arrays["params"].shape == arrays["sample_index"].shape
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert float(arrays["loss"][0]) == pytest.approx(rec["loss"], abs=1e-5)
    assert np.count_nonzero(arrays["grad"]) > 0.5 * arrays["grad"].size
