"""The obstacle focus on the device (include/omds.h: omds_focus_obstacles, omds_get_obstacle_focus, omds_clear_obstacle_focus;
csrc/obstacle_focus_kernels.hip: k_focus_keys, k_focus_select; csrc/cloud_kernels.hip: FocusSrc through the ordered compaction) against
the host definition (omds_obstacle_focus_select, checked on its own in tests/test_obstacle_focus_cpu.py) applied to the mindist row of
omds_dist_grad(q, 1) on the master, and the CONTRACT: a focused context behaves, bit for bit, like one that was given
omds_set_obstacles(master[idx]) (+ omds_set_obstacle_motion(vel[idx])).

Shapes: N = 64, H = 4, the Franka ReLU fixture network, n_closest = 10.  Masters of 10 and 11 spheres (everything kept; one dropped),
65 (two lanes' worth of one wave and a second compaction lane), 1 025 (one sphere past the 1024 lanes of the selecting workgroup and
past one compaction block), 5 000, 65 536 (64 keys per lane) and 70 000 (more than that)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

F32 = np.float32
N, H, K = 64, 4, 10
KEYS = ("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal")
ERR_INVALID_ARG, ERR_NOT_INITIALISED, ERR_UNSUPPORTED = 1, 4, 5
FAR_SHIFT = 0.45      # metres in y between the near and the far cluster of the equality test


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _net():
    return orc.Mlp.from_npz(weights_path("franka"))


def _q0():
    from optimalmodulationds_amd import scenes
    return np.asarray(scenes.FRANKA_Q0, F32)


def _engine(max_obs=512, flags=0, dt=0.5, network=True):
    from optimalmodulationds_amd.engine import Engine
    e = Engine(7, N, H, K, max_obs=max_obs, flags=flags)
    if network:
        m = _net()
        e.set_mlp(m.W, m.b, act=m.act)
    e.params.dt, e.params.dst_thr, e.params.ignored_links = dt, 0.01, 0b111
    e.push_params()
    return e


def _planner(flags=0, dt=0.5, max_obs=512):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.cost import FRANKA_Q_MAX, FRANKA_Q_MIN
    e = _engine(max_obs, flags, dt)
    e.set_ds(scenes.FRANKA_QF)
    e.set_cost(scenes.franka_dh_params(), np.array(FRANKA_Q_MIN, F32), np.array(FRANKA_Q_MAX, F32))
    rng = np.random.RandomState(3)
    mu = (_q0() + 0.2 * rng.standard_normal((N, 3, 7))).astype(F32)
    e.set_policy_samples(mu, np.ones((N, 3), F32), rng.standard_normal((N, 3, 7)).astype(F32))
    return e


def random_master(O, seed=11):
    """O spheres in the arm's workspace"""
    rng = np.random.RandomState(seed)
    xyz = rng.uniform((-0.8, -0.8, 0.0), (0.8, 0.8, 1.1), (O, 3))
    return np.concatenate([xyz, rng.uniform(0.02, 0.05, (O, 1))], 1).astype(F32)


def shelf():
    from optimalmodulationds_amd import scenes
    return np.ascontiguousarray(scenes.shelf_scene(), F32)


def definition(e, q, margin, max_keep=0, lookahead=0.0, vel=None):
    """the definition applied to the mindist row of omds_dist_grad(q, 1) on the scene in force (the master, before the call)"""
    from optimalmodulationds_amd.engine import obstacle_focus_select
    d = e.dist_grad(q, want_mindist=True)[2][0]
    return obstacle_focus_select(d, K, margin, max_keep, lookahead, vel), d


def focus_and_check(e, master, q, margin, max_keep=0, lookahead=0.0, vel=None, what=""):
    """one focus call on a context whose scene in force is ``master`` (+ ``vel``); -> the kept indices"""
    (want, want_passed), d = definition(e, q, margin, max_keep, lookahead, vel)
    kept, passed = e.focus_obstacles(q, margin, max_keep, lookahead)
    idx = e.obstacle_focus()
    assert (kept, passed) == (len(want), want_passed), (what, kept, passed, len(want), want_passed)
    assert np.array_equal(idx, want), f"{what}: the kept indices are not the definition's"
    assert e.n_obs == kept and np.array_equal(bits(e.get_obstacles()), bits(master[idx])), what
    motion, have = e.get_obstacle_motion()
    moves = vel is not None and bool((vel[idx] != 0).any())
    assert have == moves and np.array_equal(bits(motion), bits(vel[idx] if moves else np.zeros((kept, 3), F32))), what
    return idx, d


# ---- (a) the selection against the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [10, 11, 65, 1025, 5000, 65536, 70000])
def test_selection_is_the_definition(O):
    master = random_master(O)
    e = _engine(max_obs=O)
    e.set_obstacles(master)
    q = _q0()
    for margin, max_keep in ((0.1, 0), (0.0, 0), (np.inf, 0), (0.25, max(K, O // 3)), (np.inf, K)):
        idx, d = focus_and_check(e, master, q, margin, max_keep, what=(O, margin, max_keep))
        assert np.isfinite(d).all()
        e.clear_obstacle_focus()
        assert e.obstacle_focus() is None and e.n_obs == O
    if O > 1000:
        assert K < e.focus_obstacles(q, 0.1)[0] < O, "the margin of this test is meant to drop spheres and keep more than n_closest"
    e.close()


def test_tie_groups_cut_by_max_keep():
    """identical spheres have identical distances: 25 distinct spheres, 8 copies of each, shuffled; the cap cuts through a group, and
    the copies with the smallest indices are the ones kept"""
    rng = np.random.RandomState(5)
    master = np.repeat(random_master(25, seed=9), 8, axis=0)[rng.permutation(200)]
    e = _engine()
    e.set_obstacles(master)
    for max_keep in (10, 13, 16, 21, 199):
        idx, d = focus_and_check(e, master, _q0(), np.inf, max_keep, what=max_keep)
        assert len(np.unique(d)) == 25
        last = d[idx].max()
        if max_keep % 8:
            assert 0 < (d[idx] == last).sum() < 8 and np.array_equal(idx[d[idx] == last], np.flatnonzero(d == last)[:(d[idx] == last).sum()])
        e.clear_obstacle_focus()
    e.close()


def test_sphere_with_a_nan_coordinate_and_velocities_that_are_no_numbers():
    """Pass 1 need not hand a NaN on (its ReLU is a maximum with 0, which drops one): whatever distance the two spheres with a NaN
    coordinate get, the selection is the definition on it.  A NaN REACH does arise from a velocity that is no number; such a sphere
    counts as -inf and is always kept."""
    master = random_master(300, seed=4)
    master[[7, 123], [0, 2]] = np.nan
    e = _engine()
    e.set_obstacles(master)
    idx, d = focus_and_check(e, master, _q0(), 0.0, what="NaN coordinate")
    assert set(np.flatnonzero(np.isnan(d))) <= set(idx)
    e.clear_obstacle_focus()
    vel = np.zeros((300, 3), F32)
    far = np.argsort(np.nan_to_num(d, nan=-1.0))[-3:]
    vel[far[0]], vel[far[1]], vel[far[2]] = [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]
    e.set_obstacle_motion(vel)
    for lookahead in (0.0, 1.0):      # fmaf(-inf, 0, d) is a NaN too
        idx, _ = focus_and_check(e, master, _q0(), 0.0, 0, lookahead, vel, "NaN velocity")
        assert set(far) <= set(idx) and len(idx) < 40
        e.clear_obstacle_focus()
    e.close()


def test_moving_master_with_lookahead():
    master = random_master(1500, seed=6)
    rng = np.random.RandomState(8)
    vel = (0.05 * rng.standard_normal((1500, 3))).astype(F32)
    vel[rng.rand(1500) < 0.5] = 0
    e = _engine(max_obs=1500)
    e.set_obstacles(master)
    e.set_obstacle_motion(vel)
    d = e.dist_grad(_q0(), want_mindist=True)[2][0]
    far = int(np.argsort(d)[1200])
    vel[far] = F32([0.0, 0.6, 0.8]) * F32(d[far] / 1.5 + 0.2)          # fast enough to arrive within 1.5 s
    e.set_obstacle_motion(vel)
    idx, _ = focus_and_check(e, master, _q0(), 0.05, 0, 1.5, vel, "lookahead")
    assert far in idx and K < len(idx) < 1500
    e.clear_obstacle_focus()
    idx0, _ = focus_and_check(e, master, _q0(), 0.05, 0, 0.0, vel, "no lookahead")
    assert far not in idx0
    e.close()


# ---- (b) the contract ----------------------------------------------------------------------------------------------------------------
def _same_rollouts(a, b, what):
    ra, rb = a.get_rollouts(), b.get_rollouts()
    for key in KEYS:
        assert np.array_equal(bits(ra[key]), bits(rb[key])), (what, key)
    assert np.isfinite(ra["all_traj"]).all()


def _same_everything(a, b, what):
    rng = np.random.RandomState(12)
    for q in (_q0(), (_q0() + F32(0.05)).astype(F32)):
        a.propagate(q)
        b.propagate(q)
        _same_rollouts(a, b, what)
        assert np.array_equal(bits(a.cost()), bits(b.cost())), (what, "cost")
    qs = (_q0() + 0.3 * rng.standard_normal((8, 7))).astype(F32)
    for x, y in zip(a.dist_grad(qs, True, True), b.dist_grad(qs, True, True)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, "dist_grad")


@pytest.mark.parametrize("route", ["fused", "unfused", "moving-frame", "screened"])
def test_focused_context_is_the_subset_context(route):
    from optimalmodulationds_amd import _lib
    flags = _lib.FLAG_UNFUSED_STEP if route == "unfused" else 0
    master = np.concatenate([shelf(), random_master(400, seed=2)])
    a, b = _planner(flags), _planner(flags)
    vel = None
    if route == "moving-frame":
        vel = (0.1 * np.random.RandomState(1).standard_normal((len(master), 3))).astype(F32)
    for e in (a, b):
        if route == "screened":
            e.set_screening(1, 0.02)
        e.set_obstacle_frame(route == "moving-frame")
    a.set_obstacles(master)
    if vel is not None:
        a.set_obstacle_motion(vel)
    idx, _ = focus_and_check(a, master, _q0(), 0.15, 0, 0.5 if vel is not None else 0.0, vel, route)
    assert 2 * K < len(idx) < len(master)
    b.set_obstacles(master[idx])
    if vel is not None:
        b.set_obstacle_motion(vel[idx])
        assert a.get_obstacle_frame() == b.get_obstacle_frame() and a.get_obstacle_frame()[2]
        assert np.array_equal(bits(a.get_obstacle_horizon()[0]), bits(b.get_obstacle_horizon()[0]))
    _same_everything(a, b, route)
    if route == "screened":
        sa, sb = a.screen_stats(), b.screen_stats()
        assert sa["active"] and sb["active"] and sa["eps"] == sb["eps"] == F32(0.02) and sa["fallbacks"] == sb["fallbacks"]
    a.close()
    b.close()


# ---- (c) the static rule -------------------------------------------------------------------------------------------------------------
def test_moving_master_whose_kept_spheres_stand_still_is_static():
    master = shelf()
    a, b = _planner(), _planner()
    a.set_obstacles(master)
    d = a.dist_grad(_q0(), want_mindist=True)[2][0]
    vel = np.zeros((len(master), 3), F32)
    vel[d > np.sort(d)[150]] = F32([0.0, 0.0, 0.01])          # only the far half moves, and slowly
    a.set_obstacle_motion(vel)
    idx, _ = focus_and_check(a, master, _q0(), np.inf, 100, 1.5, vel, "static rule")
    assert len(idx) == 100 and not vel[idx].any() and a.get_obstacle_horizon()[1] == 0
    b.set_obstacles(master[idx])
    a.prof_enable(1)
    b.prof_enable(1)
    a.propagate(_q0())
    b.propagate(_q0())
    _same_rollouts(a, b, "static")
    assert a.prof_read_ex()[1] == b.prof_read_ex()[1], "another number of launches"
    a.clear_obstacle_focus()
    assert a.get_obstacle_horizon()[1] == 1 and np.array_equal(bits(a.get_obstacle_motion()[0]), bits(vel))
    a.close()
    b.close()


# ---- (d) re-focusing, and clearing -------------------------------------------------------------------------------------------------------
def test_refocus_selects_from_the_master_again():
    master = np.concatenate([shelf(), random_master(700, seed=3)])
    q1, q2 = _q0(), (_q0() + F32([0.4, -0.3, 0.2, 0.3, 0.0, -0.2, 0.1])).astype(F32)
    a, b = _engine(max_obs=1024), _engine(max_obs=1024)
    a.set_obstacles(master)
    b.set_obstacles(master)
    i1, _ = focus_and_check(a, master, q1, 0.1, what="q1")
    assert a.focus_obstacles(q2, 0.1) == b.focus_obstacles(q2, 0.1)
    i2 = a.obstacle_focus()
    assert np.array_equal(i2, b.obstacle_focus()) and not np.array_equal(i1, i2)
    assert np.array_equal(bits(a.get_obstacles()), bits(master[i2]))
    a.clear_obstacle_focus()
    want, _ = definition(a, q2, 0.1)
    assert np.array_equal(want[0], i2), "the second focus is the definition on the MASTER, not on the first subset"
    assert np.array_equal(bits(a.get_obstacles()), bits(master)) and a.obstacle_focus() is None
    a.clear_obstacle_focus()      # a no-op without a focus
    assert a.n_obs == len(master)
    a.close()
    b.close()


# ---- (e) the state rules ---------------------------------------------------------------------------------------------------------------
def test_state_rules():
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import obstacle_focus_spec
    master = shelf()
    e = _engine()
    q = _q0()
    spec = obstacle_focus_spec(0.1)
    assert e.lib.omds_focus_obstacles(e.h, C.byref(spec), q.ctypes.data, None, None) == ERR_NOT_INITIALISED      # no scene yet
    e.set_obstacles(master)
    # a master with an explicit horizon table is refused, the scene intact
    table = np.repeat(master[None], H, 0).copy()
    table[1:, :, 2] += F32(0.01)
    e.set_obstacle_horizon(table)
    assert e.lib.omds_focus_obstacles(e.h, C.byref(spec), q.ctypes.data, None, None) == ERR_UNSUPPORTED
    got, mode = e.get_obstacle_horizon()
    assert mode == 2 and np.array_equal(bits(got), bits(table)) and e.obstacle_focus() is None
    e.set_obstacle_horizon(None)
    # the motion and horizon setters are refused while focused, for every argument
    vel = np.full((len(master), 3), 0.01, F32)
    e.set_obstacle_motion(vel)
    idx, _ = focus_and_check(e, master, q, 0.1, 0, 0.5, vel, "state")
    scene, motion = e.get_obstacles(), e.get_obstacle_motion()[0]

    def unchanged():
        assert np.array_equal(e.obstacle_focus(), idx) and np.array_equal(bits(e.get_obstacles()), bits(scene))
        assert np.array_equal(bits(e.get_obstacle_motion()[0]), bits(motion)) and e.get_obstacle_horizon()[1] == 1

    v, slabs = vel[idx].copy(), np.repeat(scene[None], H, 0).copy()
    for call in (lambda: e.lib.omds_set_obstacle_motion(e.h, None), lambda: e.lib.omds_set_obstacle_motion(e.h, v.ctypes.data),
                 lambda: e.lib.omds_set_obstacle_horizon(e.h, None, 0),
                 lambda: e.lib.omds_set_obstacle_horizon(e.h, slabs.ctypes.data, len(scene))):
        assert call() == ERR_UNSUPPORTED and b"omds_clear_obstacle_focus" in e.lib.omds_last_error(e.h)
        unchanged()
    # argument refusals leave the scene, the master and the focus as they were
    for bad in (obstacle_focus_spec(-0.1), obstacle_focus_spec(np.nan), obstacle_focus_spec(0.1, K - 1), obstacle_focus_spec(0.1, 0, -1.0),
                obstacle_focus_spec(0.1, 0, np.inf)):
        assert e.lib.omds_focus_obstacles(e.h, C.byref(bad), q.ctypes.data, None, None) == ERR_INVALID_ARG
        unchanged()
    assert e.lib.omds_focus_obstacles(e.h, None, q.ctypes.data, None, None) == ERR_INVALID_ARG
    assert e.lib.omds_focus_obstacles(e.h, C.byref(spec), None, None, None) == ERR_INVALID_ARG
    unchanged()
    e.clear_obstacle_focus()      # the master is still the whole one
    assert np.array_equal(bits(e.get_obstacles()), bits(master)) and np.array_equal(bits(e.get_obstacle_motion()[0]), bits(vel))
    # a setter ends the focus, and its scene is the next master
    e.focus_obstacles(q, 0.1)
    other = random_master(50, seed=1)
    e.set_obstacles(other)
    assert e.obstacle_focus() is None and np.array_equal(bits(e.get_obstacles()), bits(other))
    e.set_obstacle_motion(None)      # allowed again
    focus_and_check(e, other, q, 0.05, what="next master")
    e.clear_obstacle_focus()
    assert np.array_equal(bits(e.get_obstacles()), bits(other))
    # no network: not initialised
    bare = _engine(network=False)
    bare.set_obstacles(master)
    assert bare.lib.omds_focus_obstacles(bare.h, C.byref(spec), q.ctypes.data, None, None) == ERR_NOT_INITIALISED
    assert np.array_equal(bits(bare.get_obstacles()), bits(master))
    with pytest.raises(_lib.OmdsError):
        bare.focus_obstacles(q, 0.1)
    bare.close()
    e.close()


# ---- (f) an objects-route master -------------------------------------------------------------------------------------------------------
def test_objects_master_labels_are_gathered_and_tracking_is_untouched():
    from cloud_object_cases import obj_of, track_of
    from optimalmodulationds_amd.engine import cloud_spec
    prev = np.ascontiguousarray(shelf()[:, :3])
    now = (prev + np.array([-0.4, 1.3, 2.0], F32) * F32(0.05)).astype(F32)
    nxt = (now + np.array([-0.4, 1.3, 2.0], F32) * F32(0.05)).astype(F32)
    spec, track, obj = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28)), track_of(3, 0.1), obj_of(1, 4)
    a, c = _engine(), _engine()
    for e in (a, c):
        e.set_obstacles_from_cloud_objects(prev, spec, track, obj)
        e.set_obstacles_from_cloud_objects(now, spec, track, obj)
    master, (vel, have), (label, flag, n_objects) = a.get_obstacles(), a.get_obstacle_motion(), a.cloud_objects()
    assert have and len(master) > 200
    idx, _ = focus_and_check(a, master, _q0(), 0.1, 0, 0.5, vel, "objects master")
    assert K < len(idx) < len(master)
    got_label, got_flag, got_n = a.cloud_objects()
    assert np.array_equal(got_label, label[idx]) and np.array_equal(got_flag, flag[idx]) and got_n == n_objects
    a.clear_obstacle_focus()
    assert np.array_equal(bits(a.get_obstacles()), bits(master)) and np.array_equal(bits(a.get_obstacle_motion()[0]), bits(vel))
    back = a.cloud_objects()
    assert np.array_equal(back[0], label) and np.array_equal(back[1], flag) and back[2] == n_objects
    a.focus_obstacles(_q0(), 0.1, 0, 0.5)
    # the stored frame and table are unchanged: the next objects call matches as if no focus had happened
    assert a.set_obstacles_from_cloud_objects(nxt, spec, track, obj) == c.set_obstacles_from_cloud_objects(nxt, spec, track, obj)
    assert a.obstacle_focus() is None
    assert np.array_equal(bits(a.get_obstacles()), bits(c.get_obstacles()))
    assert np.array_equal(bits(a.get_obstacle_motion()[0]), bits(c.get_obstacle_motion()[0]))
    for x, y in zip(a.cloud_objects(), c.cloud_objects()):
        assert np.array_equal(x, y)
    a.close()
    c.close()


# ---- (g) equality with the full scene where it must hold ----------------------------------------------------------------------------------
def test_focused_propagate_equals_the_full_one_when_no_dropped_sphere_matters():
    """The master is the shelf (the near cluster: the scene the network was trained around) and a copy of it moved 0.45 m away in y
    (the far cluster), with dt = 0.05: a rollout moves at most (H - 1) dt = 0.15 rad.  Chosen with the CPU oracle
    (oracle.pass1_mindist reproduces the network's bits).  The precondition is asserted, not assumed: at EVERY state of the full
    propagate the 10 nearest spheres lie in the kept set, and spheres were dropped."""
    near = shelf()
    far = near.copy()
    far[:, 1] += F32(FAR_SHIFT)
    master = np.concatenate([near, far])
    full, foc = _planner(dt=0.05, max_obs=1024), _planner(dt=0.05, max_obs=1024)
    full.set_obstacles(master)
    foc.set_obstacles(master)
    q = _q0()
    full.propagate(q)
    traj = full.get_rollouts()["all_traj"]
    idx, _ = focus_and_check(foc, master, q, 0.2, what="near + far")
    assert len(idx) < len(master), "precondition: the focus dropped nothing"
    kept = np.zeros(len(master), bool)
    kept[idx] = True
    for h in range(H):
        nearest = full.dist_grad(np.ascontiguousarray(traj[:, h]), want_idx=True)[3]
        assert kept[nearest].all(), f"precondition: a state of step {h} has a dropped sphere among its {K} nearest"
    foc.propagate(q)
    _same_rollouts(foc, full, "focused against full")
    assert np.array_equal(bits(foc.cost()), bits(full.cost()))
    full.close()
    foc.close()


# ---- (h) the facade ----------------------------------------------------------------------------------------------------------------------
def test_facade_focus_obstacles():
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    nn_model.model_jit = nn_model
    nn_model.update_aot_lambda()
    q_0, q_f = torch.tensor(scenes.FRANKA_Q0), torch.tensor(scenes.FRANKA_QF)
    dh = torch.tensor(scenes.franka_dh_params())
    master = np.concatenate([shelf(), random_master(300, seed=2)])
    vel = (0.05 * np.random.RandomState(4).standard_normal((len(master), 3))).astype(F32)
    mppi = MPPI(q_0, q_f, dh, torch.tensor(master), 0.1, H, N, [LinDS(q_f), LinDS(q_0)], dh[:, 2], nn_model, K)
    assert mppi.obs_focus is None
    mppi.update_obstacles(master, velocities=vel)
    mppi._push()
    from optimalmodulationds_amd.engine import obstacle_focus_select
    d = mppi._engine.dist_grad(scenes.FRANKA_Q0, want_mindist=True)[2][0]
    want, want_passed = obstacle_focus_select(d, K, 0.1, 0, (H - 1) * 0.1, vel)
    kept, passed = mppi.focus_obstacles(0.1)
    assert (kept, passed) == (len(want), want_passed) and K < kept < len(master)
    assert np.array_equal(mppi.obs_focus.numpy(), want) and mppi.n_obs == kept
    assert np.array_equal(bits(mppi.obs.numpy()), bits(master[want])) and np.array_equal(bits(mppi.obs_velocities.numpy()), bits(vel[want]))
    mppi.Policy.sample_policy()
    mppi.propagate()
    assert torch.isfinite(mppi.all_traj).all()
    q2 = (scenes.FRANKA_Q0 + F32(0.3)).astype(F32)
    kept2, _ = mppi.focus_obstacles(0.1, max_keep=40, q=q2)
    assert kept2 == 40 and len(mppi.obs_focus) == 40 and mppi.n_obs == 40
    mppi.clear_obstacle_focus()
    assert mppi.obs_focus is None and mppi.n_obs == len(master) and np.array_equal(bits(mppi.obs_velocities.numpy()), bits(vel))
    mppi.focus_obstacles(0.1)
    mppi.update_obstacles(master[:100])
    assert mppi.obs_focus is None and mppi._engine.obstacle_focus() is None
