"""The two-part propagate (csrc/propagate.hip: enqueue_dense_halves; the plan: csrc/propagate_plan_def.h): the full steps of the Dense
route as the rollouts [0, split) on the context's stream and [split, N) on a second one, in anti-phase.  Another schedule, the SAME
BITS: a context with OMDS_FLAG_PIPELINED_PROPAGATE against one with OMDS_FLAG_SERIAL_PROPAGATE on the same inputs, compared through the
uint32 views of all seven rollout tensors, the cost and the weighted update, and omds_get_pipeline_info reporting the parts each case
expects.

Shapes: 40 spheres (more than the small-scene step takes, and with OMDS_FLAG_TAIL_FORWARD no emitting pass 1: the Dense route) and
N = 32, 33, 48, 70: parts of 16 / 16, 32 / 1 (a part of one rollout: one ragged 8 x 4 block per obstacle block, a tail launch of one
workgroup), 32 / 16 and 48 / 22 (22 is no multiple of the 3 or 4 rollouts of a tail workgroup, 70 none of 16).  The forced form runs the
block-ordered kernel on every part, however small."""
import functools

import numpy as np
import pytest

from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

K_CLOSEST = 5
TENSORS = ("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal")


def _flags():
    from optimalmodulationds_amd import _lib as L
    base = L.FLAG_BLOCK_TILES | L.FLAG_TAIL_FORWARD
    return L.FLAG_SERIAL_PROPAGATE | base, L.FLAG_PIPELINED_PROPAGATE | base


@functools.lru_cache(maxsize=None)
def _mlp(kind):
    return orc.Mlp.from_npz(weights_path(kind))


@functools.lru_cache(maxsize=None)
def _scene40():
    from optimalmodulationds_amd import scenes
    obs = scenes.shelf_scene()
    assert obs.shape[0] == 294
    return np.ascontiguousarray(obs[::7][:40])


def _split(N):
    return ((N + 1) // 2 + 15) // 16 * 16


def _engine(N, H, flags, obs=None, kind="franka", lib=None):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.cost import FRANKA_Q_MAX, FRANKA_Q_MIN
    from optimalmodulationds_amd.engine import Engine
    m = _mlp(kind)
    obs = _scene40() if obs is None else obs
    e = Engine(7, N, H, K_CLOSEST, max_obs=512, flags=flags, lib=lib)
    e.set_mlp(m.W, m.b, act=m.act, skip_after=m.skip_after)
    e.set_obstacles(obs)
    e.params.dt = 0.5
    e.params.dst_thr = 0.01
    e.params.ignored_links = 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_cost(scenes.franka_dh_params(), FRANKA_Q_MIN, FRANKA_Q_MAX)
    return e


def _means(K, seed):
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(seed)
    s = (np.arange(K) + 0.5) / max(K, 1)
    mu = (scenes.FRANKA_Q0 + s[:, None] * (scenes.FRANKA_QF - scenes.FRANKA_Q0) + 0.15 * rng.standard_normal((K, 7))).astype(np.float32)
    return mu, np.ones(K, np.float32), rng.standard_normal((K, 7)).astype(np.float32)


def _q_cur(seed, N=None):
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(seed)
    q = (np.asarray(scenes.FRANKA_Q0, np.float32) + 0.1 * rng.standard_normal(7)).astype(np.float32)
    if N is not None:
        q = (q + 0.3 * rng.standard_normal((N, 7))).astype(np.float32)
    return q


def _iteration(e, q, means, seed):
    """sample, propagate, cost, update: everything a planner iteration reads, as uint32 views"""
    K = means[0].shape[0]
    e.sample_policy(*means, 0.0, 0.0, 3.0, K, seed=seed)
    e.propagate(q)
    out = dict(e.get_rollouts())
    out["cost"] = e.cost()
    if K:
        mu, sg, al, mask, w = e.weighted_update(0.1, 0.1, *means, want_weights=True)
        out.update(upd_mu=mu, upd_sigma=sg, upd_alpha=al, upd_mask=mask.astype(np.float32), upd_w=w)
    return {k: np.ascontiguousarray(v, np.float32).view(np.uint32) for k, v in out.items()}


def _same(a, b, what):
    assert set(TENSORS) <= set(a) and set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differs between the serial and the two-part propagate"


def _pair(N, H, q, K=10, seed=3, prepare=None, what="", expect=None, **kw):
    """the same iteration on a serial and a two-part context; returns the two-part one's tensors"""
    serial_flags, piped_flags = _flags()
    means = _means(K, seed)
    res = []
    for flags in (serial_flags, piped_flags):
        e = _engine(N, H, flags, **kw)
        if prepare:
            prepare(e)
        res.append(_iteration(e, q, means, seed))
        info = e.pipeline_info()
        e.close()
        want = (1, N) if flags == serial_flags else expect
        assert info == want, f"{what}: the propagate reports parts {info}, expected {want}"
    _same(res[0], res[1], what)
    return res[1]


@pytest.mark.parametrize("H", [1, 2, 3, 5])
@pytest.mark.parametrize("N", [32, 33, 48, 70])
def test_same_bits_on_the_smallest_shapes(N, H):
    """From one state: step 1 is the shared step, so H = 1 and H = 2 leave fewer than two full steps and stay serial"""
    expect = (2, _split(N)) if H >= 3 else (1, N)
    assert _split(N) == {32: 16, 33: 32, 48: 32, 70: 48}[N]
    got = _pair(N, H, _q_cur(11), expect=expect, what=f"N = {N}, H = {H}")
    if H >= 2:
        assert np.ptp(got["all_traj"].view(np.float32)[:, 1], axis=0).max() > 0, "the rollouts must part after the first step"


@pytest.mark.parametrize("K", [0, 10])
def test_policy_kernels(K):
    _pair(33, 4, _q_cur(12), K=K, expect=(2, 32), what=f"K = {K}")


@pytest.mark.parametrize("H", [1, 2, 3])
def test_per_rollout_start(H):
    """No shared first step: step 1 is a full step and itself runs in two parts (the key units are picked on the whole batch in front
    of the fork); two full steps from H = 2 on"""
    N = 48
    got = _pair(N, H, _q_cur(13, N), expect=(2, 32) if H >= 2 else (1, N), what=f"per-rollout start, H = {H}")
    assert np.ptp(got["all_traj"].view(np.float32)[:, 0], axis=0).max() > 0


def test_motion_horizon_in_the_moving_frame():
    """Step i reads slab i - 1 of the obstacle horizon in either half; the tail is the moving frame's instantiation"""
    rng = np.random.RandomState(9)
    vel = (0.2 * rng.standard_normal((40, 3))).astype(np.float32)

    def moving(e):
        e.set_obstacle_motion(vel)
        e.set_obstacle_frame(True)

    q = _q_cur(14)
    got = _pair(70, 4, q, prepare=moving, expect=(2, 48), what="motion horizon, moving frame")
    still = _pair(70, 4, q, expect=(2, 48), what="static scene")
    assert not np.array_equal(got["closest_dist_all"], still["closest_dist_all"]), "the motion was meant to change the distances"


def test_three_iterations_back_to_back():
    """The order buffers, the second stream and the events are reused; each iteration samples anew"""
    serial_flags, piped_flags = _flags()
    N, H = 70, 5
    a, b = _engine(N, H, serial_flags), _engine(N, H, piped_flags)
    means = _means(10, 4)
    for it in range(3):
        q = _q_cur(20 + it)
        ra, rb = _iteration(a, q, means, 30 + it), _iteration(b, q, means, 30 + it)
        _same(ra, rb, f"iteration {it}")
        assert a.pipeline_info() == (1, N) and b.pipeline_info() == (2, 48)
    a.close()
    b.close()


def test_profiling_brackets_whole_batch_steps():
    """omds_prof_enable(2): every second launch of pass 1 is bracketed, and a bracketed step runs as ONE launch over the whole batch
    (the halves joined in front of it, forked and seeded again behind it).  Launches and rows are the serial context's."""
    serial_flags, piped_flags = _flags()
    N, H, O = 70, 5, 40
    means, q = _means(10, 5), _q_cur(15)
    res, prof = [], []
    for flags in (serial_flags, piped_flags):
        e = _engine(N, H, flags)
        e.prof_enable(2)
        e.prof_reset()
        res.append(_iteration(e, q, means, 5))
        _, launches, rows = e.prof_read()
        prof.append((launches, rows))
        assert e.pipeline_info() == ((1, N) if flags == serial_flags else (2, 48))
        e.close()
    _same(res[0], res[1], "profiling at stride 2")
    # launches 1 (the shared step: O rows), 3 and 5 (N x O rows each) are bracketed
    assert prof[0] == (3, O + 2 * N * O), prof
    assert prof[1] == prof[0], f"the two-part propagate counted {prof[1]}, the serial one {prof[0]}"


def test_two_pipelined_contexts_alive_at_once():
    serial_flags, piped_flags = _flags()
    N, H = 48, 4
    means, q1, q2 = _means(10, 6), _q_cur(16), _q_cur(17)
    s = _engine(N, H, serial_flags)
    want1, want2 = _iteration(s, q1, means, 6), _iteration(s, q2, means, 7)
    s.close()
    a, b = _engine(N, H, piped_flags), _engine(N, H, piped_flags)
    got1 = _iteration(a, q1, means, 6)
    got2 = _iteration(b, q2, means, 7)
    got1_again = _iteration(a, q1, means, 6)
    assert a.pipeline_info() == (2, 32) and b.pipeline_info() == (2, 32)
    a.close()
    b.close()
    _same(want1, got1, "first context")
    _same(want2, got2, "second context")
    _same(want1, got1_again, "first context, after the second one ran")


def test_tanh_network_stays_on_one_stream():
    """No compacting pass 1 for a tanh network: the plan says one part whatever the flag asks, and the results are equal"""
    _pair(48, 4, _q_cur(18), kind="franka_tanh", expect=(1, 48), what="tanh network")


def test_default_flags_at_1024_rollouts():
    """1024 x 294 x H = 4 under the default flags against OMDS_FLAG_SERIAL_PROPAGATE: 512 x 294 pairs per part reach
    OMDS_BLOCK_TILES_MIN_PAIRS and three full steps follow the shared one, so the default is two parts of 512"""
    from optimalmodulationds_amd import _lib as L, scenes
    N, H = 1024, 4
    obs = scenes.shelf_scene()
    means, q = _means(10, 8), _q_cur(19)
    res = []
    for flags, want in ((L.FLAG_SERIAL_PROPAGATE, (1, N)), (0, (2, 512))):
        e = _engine(N, H, flags, obs=obs)
        res.append(_iteration(e, q, means, 8))
        assert e.pipeline_info() == want, (flags, e.pipeline_info())
        e.close()
    _same(res[0], res[1], "1024 x 294, default flags")
