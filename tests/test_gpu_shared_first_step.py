"""The shared first step of a propagate from ONE state (propagate.hip: enqueue_dense): at horizon step 1 all N rollouts sit at
q_cur, so pass 1 evaluates one rollout's O rows and every rollout's tail selects from that row.  The SAME BITS as the full N x O
launch (OMDS_FLAG_NATURAL_PASS1) and as a per-rollout propagate fed N copies of q_cur: every tensor of get_rollouts() is equal."""
import numpy as np
import pytest

from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

N, H, K_CLOSEST, K_POLICY = 96, 3, 5, 3


def _rollouts(m, obs, samples, q, flags=0):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import Engine
    e = Engine(7, N, H, K_CLOSEST, max_obs=512, flags=flags)
    e.set_mlp(m.W, m.b)
    e.set_obstacles(obs)
    e.params.dt = 0.5
    e.params.dst_thr = 0.01
    e.params.ignored_links = 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_policy_samples(*samples)
    e.prof_enable(1)
    e.prof_reset()
    e.propagate(q)
    got = e.get_rollouts()
    _, launches, rows = e.prof_read()
    e.close()
    return got, launches, rows


def test_shared_first_step_is_bit_identical_to_the_per_rollout_evaluation():
    from optimalmodulationds_amd import _lib as L, scenes
    m = orc.Mlp.from_npz(weights_path("franka"))
    obs = scenes.shelf_scene()
    O = obs.shape[0]
    assert N * O > 24576, "the Dense route (k_pass1 + k_tail) runs above the Emit route's 24 576 pairs"
    rng = np.random.RandomState(11)
    q_cur = (np.asarray(scenes.FRANKA_Q0, np.float32) + 0.1 * rng.standard_normal(7)).astype(np.float32)
    mu = (q_cur + 0.2 * rng.standard_normal((N, K_POLICY, 7))).astype(np.float32)
    samples = (mu, np.ones((N, K_POLICY), np.float32), rng.standard_normal((N, K_POLICY, 7)).astype(np.float32))

    shared, l_s, r_s = _rollouts(m, obs, samples, q_cur)                                   # case 1: default flags
    natural, l_n, r_n = _rollouts(m, obs, samples, q_cur, flags=L.FLAG_NATURAL_PASS1)      # case 2: the opt-out
    per, l_p, r_p = _rollouts(m, obs, samples, np.tile(q_cur, (N, 1)))                     # case 3: per_rollout = 1, N copies
    print("pass-1 launches / rows: shared", l_s, r_s, "natural", l_n, r_n, "per-rollout", l_p, r_p)
    # the bracket of step 1 counts the rows it launched: O at the shared step, N * O everywhere else
    assert (l_s, r_s) == (H, O + (H - 1) * N * O)
    assert (l_n, r_n) == (H, H * N * O) and (l_p, r_p) == (H, H * N * O)
    assert np.ptp(shared["all_traj"][:, 1], axis=0).max() > 0, "the rollouts must part after the first step for steps 2.. to mean anything"
    for name in shared:
        assert np.array_equal(shared[name], natural[name]), f"{name}: the shared first step differs from the full launch"
        assert np.array_equal(shared[name], per[name]), f"{name}: the shared first step differs from the per-rollout propagate"
