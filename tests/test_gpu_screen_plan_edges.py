"""GPU test of k_screen's launch plan and the candidate selection where they change form (csrc/screen_plan_def.h, screen_select.h): a
screened propagate against the fp32-pass-1 propagate, bit for bit on every returned array, at the obstacle counts where

  * a rollout's values stop fitting the 8 registers per lane of select_rollout's first group / of all groups (O = 64 | 65, 512 | 513),
  * a rollout stops fitting a workgroup's result buffer and the matrix route with k_select takes over (O = 5120 | 5121),

each with N = 20 rollouts -- not a multiple of SEL_WAVES = 8, so that k_select and k_screen's flush phase both run with dead waves --
and at N = 300, O = 33: more rollouts than CUs, chunks of one and of two rollouts, and a partial last tile whose trailing waves own
no pair.  tests/test_screen_plan_cpu.py walks the plan's integers on the host; here the kernels run by them.

A fallback to fp32 would make the comparison trivially true: every case asserts that screening was active and that the fallback
counter did not move during the compared propagate.  The scenes (uniform clouds of small spheres in the robot's workspace) and their
seeds were chosen on the commit before the plan was stated in a header so that that commit satisfies this too."""
import numpy as np
import pytest

from test_gpu_screen import KEYS, _engine, _run

pytestmark = pytest.mark.gpu

CASES = [(20, 64), (20, 65), (20, 512), (20, 513), (20, 5120), (20, 5121), (300, 33)]   # (N, O); H = 2, k = 5


@pytest.mark.parametrize("N,O", CASES, ids=[f"N{N}-O{O}" for N, O in CASES])
def test_screened_propagate_is_bit_identical_where_the_plan_changes_form(N, O):
    rng = np.random.RandomState(8)
    p = rng.uniform([-0.3, -0.8, 0.0], [1.0, 0.8, 1.2], (O, 3))
    obs = np.c_[p, rng.uniform(0.01, 0.04, O)].astype(np.float32)
    H, K = 2, 4
    e, m, obs, q0, qf = _engine(N, H, obs=obs)
    rng = np.random.RandomState(5)
    mu_c = (q0 + 0.2 * rng.standard_normal((K, 7))).astype(np.float32)
    sg_c, al_c = np.ones(K, np.float32), rng.standard_normal((K, 7)).astype(np.float32)
    a = _run(e, q0, 0, K, mu_c, sg_c, al_c, seed=3)
    before = e.screen_stats()
    b = _run(e, q0, 1, K, mu_c, sg_c, al_c, seed=3)
    st = e.screen_stats()
    print(N, O, {k: st[k] for k in ("active", "eps", "max_err_seen", "candidates_per_rollout_step", "fallbacks", "audit_rows_per_rollout_step")})
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (key, float(np.abs(a[key] - b[key]).max()))
    assert st["active"] and st["fallbacks"] == before["fallbacks"] and st["candidates_per_rollout_step"] >= 5, (before, st)
    e.close()
