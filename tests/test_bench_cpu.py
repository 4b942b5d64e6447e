"""bench.py's launcher logic on a box without a GPU: it must REFUSE -- never print a line for a rank count it did not run.  And the
host side of --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

BENCH = os.path.join(ROOT, "bench.py")
CLEAN = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}


def _run(args, env=None, timeout=300):
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env or CLEAN)


def _no_result(r):
    return r.returncode != 0 and not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_more_ranks_than_gpus_is_refused_before_anything_runs():
    """`python bench.py --gpus N` without a launcher environment starts its own ranks -- and exits non-zero with a message when the box
    has fewer than N GPUs (64 is more than any box; on this CPU box 2 already is), instead of running one GPU and printing n_gpus: 1."""
    import __graft_entry__ as g
    g.build()
    r = _run(["--gpus", "64", "--steps", "1", "--warmup", "0"])
    assert _no_result(r) and "--gpus 64 needs 64 GPU(s)" in r.stderr and "refusing" in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    from optimalmodulationds_amd import _lib
    if _lib.device_count() < 2:
        r = _run(["--gpus", "2"])
        assert _no_result(r) and "--gpus 2 needs 2 GPU(s)" in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    if _lib.device_count() < 1:
        r = _run([])
        assert _no_result(r) and "needs a GPU" in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]


def test_a_launcher_world_size_that_disagrees_with_gpus_is_refused():
    """The driver's form (torch.distributed.run sets RANK / WORLD_SIZE): --gpus must equal the number of ranks the launcher started;
    a 2-rank run is never filed as 8 GPUs, nor a 1-rank run as 2."""
    env = dict(CLEAN, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = _run(["--gpus", "8"], env=env)
    assert _no_result(r) and "WORLD_SIZE=2" in r.stderr and "--gpus 8" in r.stderr, r.stderr[-2000:]
    env["WORLD_SIZE"] = "1"
    r = _run(["--gpus", "2"], env=env)
    assert _no_result(r) and "WORLD_SIZE=1" in r.stderr, r.stderr[-2000:]


def test_self_launcher_relays_a_failure_of_its_ranks(monkeypatch, capsys):
    """The self-launcher with the GPU pre-check out of the way: it spawns `torch.distributed.run` with two ranks as a CHILD process;
    here every rank fails (no GPU), and the launcher must turn that into its own non-zero exit and print no result line."""
    from optimalmodulationds_amd import _lib
    if _lib.device_count() >= 1:
        pytest.skip("needs a box without a GPU: the ranks are meant to fail")
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "visible_devices", lambda: 2)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    args = type("A", (), {"gpus": 2, "share_gpu": False})()
    with pytest.raises(SystemExit) as e:
        bench.self_launch(args, ["--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-secondary"])
    assert e.value.code not in (0, None) and "2-rank run failed" in str(e.value.code)
    assert not [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]


def test_physical_cores_come_from_cpuinfo_not_from_psutil():
    sys.path.insert(0, ROOT)
    import bench
    n = bench.physical_cores()
    assert 1 <= n <= (os.cpu_count() or 1)


class _RolloutsOnly:
    """The two rollout getters of optimalmodulationds_amd.engine.Engine that bench.dump_outputs calls, on constant data."""
    def __init__(self, N, H, n, K):
        self.N, self.H, self.n, self.K = N, H, n, K
        self.full_fetches = 0

    def _out(self, R):
        H, n, K = self.H, self.n, self.K
        shapes = {"all_traj": (R, H, n), "closest_dist_all": (R, H), "kernel_val_all": (R, H, K), "dot_products": (R, H),
                  "kernel_activations": (R, H), "qdot": (R, n), "normal": (R, H, n)}
        return {k: np.full(s, 0.5, np.float32) for k, s in shapes.items()}

    def get_rollouts(self):
        self.full_fetches += 1
        return self._out(self.N)

    def get_rollout_rows(self, t):
        return self._out(len(t))


def _dump(path, eng):
    import bench
    K, n = 50, eng.n
    bench.dump_outputs(str(path), eng, K, np.ones((K, n), np.float32), np.ones(K, np.float32), np.ones((K, n), np.float32),
                       np.ones(K, bool), np.ones(n, np.float32), np.ones(n, np.float32))
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_are_float_and_within_64_mb(tmp_path):
    """--dump-outputs: float32 files (the sample's row indices float64); rollout tensors past the budget (8192 x 32 rollouts, K = 50:
    ~70 MB) are written for a seeded sample of rollouts -- the same one every run, so two builds compare row for row."""
    sys.path.insert(0, ROOT)
    import bench
    small = _RolloutsOnly(1024, 32, 7, 50)
    got = _dump(tmp_path / "small", small)
    assert small.full_fetches == 1 and "rollout_rows" not in got and got["rollout_all_traj"].shape == (1024, 32, 7)
    assert all(a.dtype == np.float32 for a in got.values()) and got["update_mask"].shape == (50,)
    big = _RolloutsOnly(8192, 32, 7, 50)
    a, b = _dump(tmp_path / "a", big), _dump(tmp_path / "b", big)
    assert big.full_fetches == 0
    rows = a["rollout_rows"]
    assert rows.dtype == np.float64 and np.array_equal(rows, b["rollout_rows"]) and 0 < rows.size < 8192
    assert np.all(np.diff(rows) > 0) and rows[-1] < 8192 and a["rollout_all_traj"].shape == (rows.size, 32, 7)
    assert all(v.dtype == np.float32 for k, v in a.items() if k != "rollout_rows")
    total = sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES, total
