"""bench.py's plain run on the GPU: exactly --steps timed iterations, the headline line only, and --dump-outputs files that two runs
with the same arguments reproduce."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

CLEAN = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=CLEAN)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_reproducible_outputs(tmp_path):
    outs, lines = [], []
    for tag in ("a", "b"):
        d = str(tmp_path / tag)
        lines.append(_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", d]))
        outs.append(_load(d))
    for line in lines:
        assert line["steps"] == 3 and line["reps"] == 1 and len(line["rep_ms_per_step"]) == 1, line
        assert line["dtype"] == "f32" and line["higher_is_better"] is True and line["unit"] == "rollout-steps/s", line
        assert abs(line["value"] - 1024 * 32 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"], line
        assert not {"roofline", "also", "cpu_baseline", "value_screened", "fetch_all_rollouts_ms"} & set(line), sorted(line)
    a, b = outs
    assert a["policy_mu"].shape == (10, 7) and a["rollout_all_traj"].shape == (1024, 32, 7) and a["rollout_qdot"].shape == (1024, 7)
    assert sum(v.nbytes for v in a.values()) <= 64 * 10**6
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == np.float32, k
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.isfinite(a["qdot_weighted"]).all() and np.isfinite(a["q_next"]).all()
