"""The obstacle focus along a path of joint states on the device (include/omds.h: omds_focus_obstacles_path;
csrc/obstacle_focus_kernels.hip: k_focus_path_keys, k_focus_path_bars, k_focus_path_merge, k_focus_path_words, k_focus_select<true>)
against the host definition (omds_obstacle_focus_select_path, checked on its own in tests/test_obstacle_focus_path_cpu.py) applied to
the mindist rows of omds_dist_grad(q_path) on the master, and the CONTRACT of the single-state call, which the path call takes over.

Shapes: N = 64, H = 4, the Franka ReLU fixture network, n_closest = 10, as in tests/test_gpu_obstacle_focus.py, whose scenes and
comparison helpers are used here.  A path of B states goes through pass 1 in chunks of min(n_traj, B) states."""
import ctypes as C

import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

from helpers import weights_path
from test_gpu_obstacle_focus import (ERR_INVALID_ARG, ERR_NOT_INITIALISED, ERR_UNSUPPORTED, FAR_SHIFT, F32, H, K, N, _net, _planner, _q0,
                                     _same_everything, _same_rollouts, bits, random_master, shelf)

pytestmark = pytest.mark.gpu


def _engine(max_obs=512, n_traj=N, flags=0, network=True):
    from optimalmodulationds_amd.engine import Engine
    e = Engine(7, n_traj, H, K, max_obs=max_obs, flags=flags)
    if network:
        m = _net()
        e.set_mlp(m.W, m.b, act=m.act)
    e.params.dt, e.params.dst_thr, e.params.ignored_links = 0.5, 0.01, 0b111
    e.push_params()
    return e


def path_of(B, seed=21, spread=0.3):
    """B joint states around the start state, the first one the start state itself"""
    rng = np.random.RandomState(seed)
    p = (_q0() + spread * rng.standard_normal((B, 7))).astype(F32)
    p[0] = _q0()
    return p


def rows_of(e, q_path):
    """the mindist matrix of omds_dist_grad(q_path) on the scene in force, in batches the context takes"""
    step = e.N
    return np.concatenate([e.dist_grad(q_path[i:i + step], want_mindist=True)[2] for i in range(0, len(q_path), step)])


def focus_and_check(e, master, q_path, margin, max_keep=0, lookahead=0.0, ahead=None, vel=None, what="", d=None):
    """one path focus on a context whose scene in force is ``master`` (+ ``vel``) against the definition on ``d`` (None: the rows of
    omds_dist_grad on that scene); -> the kept indices, d"""
    from optimalmodulationds_amd.engine import obstacle_focus_select_path
    d = rows_of(e, q_path) if d is None else d
    want, want_passed = obstacle_focus_select_path(d, K, margin, max_keep, lookahead, ahead, vel)
    kept, passed = e.focus_obstacles_path(q_path, margin, max_keep, lookahead, ahead)
    idx = e.obstacle_focus()
    assert (kept, passed) == (len(want), want_passed), (what, kept, passed, len(want), want_passed)
    assert np.array_equal(idx, want), f"{what}: the kept indices are not the definition's"
    assert e.n_obs == kept and np.array_equal(bits(e.get_obstacles()), bits(master[idx])), what
    motion, have = e.get_obstacle_motion()
    moves = vel is not None and bool((vel[idx] != 0).any())
    assert have == moves and np.array_equal(bits(motion), bits(vel[idx] if moves else np.zeros((kept, 3), F32))), what
    return idx, d


# ---- (a) the selection against the definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,O", [(1, 11), (2, 65), (15, 1025), (16, 1025), (17, 1025), (64, 1025), (65, 1025), (33, 5000), (130, 70000)])
def test_selection_is_the_definition(B, O):
    """one chunk (B <= 64) and several, a last chunk of one state (65), a last chunk of two (130), the size classes of pass 1, an odd
    sphere count (one key per lane of the merge) and a multiple of four (four per lane), more keys than lanes"""
    master = random_master(O)
    e = _engine(max_obs=O)
    e.set_obstacles(master)
    q_path = path_of(B)
    d = None
    for margin, max_keep in ((0.1, 0), (0.0, 0), (np.inf, 0), (0.25, max(K, O // 3)), (np.inf, K)):      # a cap below K is refused
        idx, d = focus_and_check(e, master, q_path, margin, max_keep, what=(B, O, margin, max_keep), d=d)
        assert np.isfinite(d).all() and d.shape == (B, O)
        e.clear_obstacle_focus()
        assert e.obstacle_focus() is None and e.n_obs == O
    if O > 1000:
        assert K < e.focus_obstacles_path(q_path, 0.0)[0] < O, "margin 0 is meant to drop spheres and keep more than n_closest"
    e.close()


def test_tie_groups_cut_by_max_keep():
    """identical spheres have identical distances at every state: 25 distinct spheres, 8 copies of each, shuffled; the cap cuts through
    a group of equal nearest keys, and the copies with the smallest indices are the ones kept"""
    rng = np.random.RandomState(5)
    master = np.repeat(random_master(25, seed=9), 8, axis=0)[rng.permutation(200)]
    e = _engine()
    e.set_obstacles(master)
    q_path = path_of(5)
    for max_keep in (10, 13, 16, 21, 199):
        idx, d = focus_and_check(e, master, q_path, np.inf, max_keep, what=max_keep)
        m = d.min(0)
        last = m[idx].max()
        if max_keep % 8:
            assert 0 < (m[idx] == last).sum() < 8 and np.array_equal(idx[m[idx] == last], np.flatnonzero(m == last)[:(m[idx] == last).sum()])
        e.clear_obstacle_focus()
    e.close()


# ---- (b) one state is the single-state call --------------------------------------------------------------------------------------------
def test_one_state_is_the_single_state_call():
    master = np.concatenate([shelf(), random_master(900, seed=3)])
    vel = (0.05 * np.random.RandomState(2).standard_normal((len(master), 3))).astype(F32)
    a, b = _engine(max_obs=2048), _engine(max_obs=2048)
    for e in (a, b):
        e.set_obstacles(master)
        e.set_obstacle_motion(vel)
    q = (_q0() + F32(0.1)).astype(F32)
    for margin, max_keep, lookahead, ahead in ((0.1, 0, 0.5, None), (0.0, 0, 0.0, [0.0]), (0.2, 50, 1.0, [0.0]), (np.inf, 0, 0.0, None)):
        assert a.focus_obstacles_path(q[None], margin, max_keep, lookahead, ahead) == b.focus_obstacles(q, margin, max_keep, lookahead)
        assert np.array_equal(a.obstacle_focus(), b.obstacle_focus())
        assert np.array_equal(bits(a.get_obstacles()), bits(b.get_obstacles()))
        assert np.array_equal(bits(a.get_obstacle_motion()[0]), bits(b.get_obstacle_motion()[0]))
        assert np.array_equal(bits(a.get_obstacle_horizon()[0]), bits(b.get_obstacle_horizon()[0]))
    a.close()
    b.close()


# ---- (c) the chunk size does not show ---------------------------------------------------------------------------------------------------
def test_chunking_does_not_show():
    """contexts of 1, 16 and 64 rollouts take 33 states one at a time, in chunks of 16 + 16 + 1 and in one chunk"""
    master = random_master(1500, seed=6)
    vel = (0.05 * np.random.RandomState(8).standard_normal((1500, 3))).astype(F32)
    q_path, ahead = path_of(33), np.linspace(0.0, 1.5, 33).astype(F32)
    got = []
    for n_traj in (1, 16, 64):
        e = _engine(max_obs=1500, n_traj=n_traj)
        e.set_obstacles(master)
        e.set_obstacle_motion(vel)
        res = []
        for margin, max_keep in ((0.05, 0), (0.0, 0), (0.2, 300), (np.inf, 40)):
            counts = e.focus_obstacles_path(q_path, margin, max_keep, 0.25, ahead)
            res.append((counts, e.obstacle_focus()))
        got.append(res)
        if n_traj == 64:
            e.clear_obstacle_focus()
            focus_and_check(e, master, q_path, 0.05, 0, 0.25, ahead, vel, "64 rollouts")
        e.close()
    for res in got[1:]:
        for (c0, i0), (c1, i1) in zip(got[0], res):
            assert c0 == c1 and np.array_equal(i0, i1)
    assert K < got[0][0][0][0] < 1500


# ---- (d) moving masters and inputs that are no numbers ---------------------------------------------------------------------------------
def test_sphere_kept_only_through_a_late_states_ahead():
    master = random_master(1500, seed=6)
    e = _engine(max_obs=1500)
    e.set_obstacles(master)
    q_path = path_of(6, spread=0.05)
    d = rows_of(e, q_path)
    far = int(np.argsort(d.min(0))[1200])
    vel = np.zeros((1500, 3), F32)
    t = np.sort(d, 1)[:, K - 1]
    speed = F32((d[5, far] - t[5]) / 1.5 + 0.02)          # after the last state's 1.5 s it is 0.03 m inside that state's threshold ...
    vel[far] = F32([0.0, 0.6, 0.8]) * speed
    assert (d[:, far] - 1.0 * speed).min() > t.max() + 0.05 + 0.01          # ... and after 1 s it is outside every state's bar
    e.set_obstacle_motion(vel)
    late = np.array([0.0, 0.2, 0.4, 0.6, 0.8, 1.5], F32)
    idx, _ = focus_and_check(e, master, q_path, 0.05, 0, 0.0, late, vel, "late ahead", d)
    assert far in idx and K < len(idx) < 1500
    e.clear_obstacle_focus()
    idx, _ = focus_and_check(e, master, q_path, 0.05, 0, 0.0, np.minimum(late, F32(1.0)), vel, "ahead too short", d)
    assert far not in idx
    e.clear_obstacle_focus()
    idx, _ = focus_and_check(e, master, q_path, 0.05, 0, 0.0, None, vel, "no ahead", d)
    assert far not in idx
    e.close()


def test_sphere_with_a_nan_coordinate_and_velocities_that_are_no_numbers():
    master = random_master(300, seed=4)
    master[[7, 123], [0, 2]] = np.nan
    e = _engine()
    e.set_obstacles(master)
    q_path = path_of(5)
    idx, d = focus_and_check(e, master, q_path, 0.0, what="NaN coordinate")
    assert set(np.flatnonzero(np.isnan(d).any(0))) <= set(idx)
    e.clear_obstacle_focus()
    vel = np.zeros((300, 3), F32)
    far = np.argsort(np.nan_to_num(d, nan=-1.0).min(0))[-3:]
    vel[far[0]], vel[far[1]], vel[far[2]] = [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]
    e.set_obstacle_motion(vel)
    for lookahead, ahead in ((0.0, None), (1.0, None), (0.0, np.array([0, 0, 0.5, 0, 0], F32))):      # fmaf(-inf, 0, d) is a NaN too
        idx, _ = focus_and_check(e, master, q_path, 0.0, 0, lookahead, ahead, vel, "NaN velocity")
        assert set(far) <= set(idx) and len(idx) < 150
        e.clear_obstacle_focus()
    e.close()


# ---- (e) the contract ------------------------------------------------------------------------------------------------------------------
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
    q_path = path_of(70, spread=0.1)
    ahead = np.linspace(0.0, 1.0, 70).astype(F32) if vel is not None else None
    idx, _ = focus_and_check(a, master, q_path, 0.05, 0, 0.25 if vel is not None else 0.0, ahead, vel, route)
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


def test_moving_master_whose_kept_spheres_stand_still_is_static():
    master = shelf()
    a, b = _planner(), _planner()
    a.set_obstacles(master)
    q_path = path_of(4, spread=0.02)
    d = rows_of(a, q_path).min(0)
    vel = np.zeros((len(master), 3), F32)
    vel[d > np.sort(d)[150]] = F32([0.0, 0.0, 0.01])          # only the far half moves, and slowly
    a.set_obstacle_motion(vel)
    idx, _ = focus_and_check(a, master, q_path, np.inf, 100, 1.0, np.array([0, 0.5, 0.5, 0.5], F32), vel, "static rule")
    assert len(idx) == 100 and not vel[idx].any() and a.get_obstacle_horizon()[1] == 0
    b.set_obstacles(master[idx])
    a.propagate(_q0())
    b.propagate(_q0())
    _same_rollouts(a, b, "static")
    a.clear_obstacle_focus()
    assert a.get_obstacle_horizon()[1] == 1 and np.array_equal(bits(a.get_obstacle_motion()[0]), bits(vel))
    assert np.array_equal(bits(a.get_obstacles()), bits(master)) and a.obstacle_focus() is None
    a.close()
    b.close()


def test_refocus_selects_from_the_master_again():
    master = np.concatenate([shelf(), random_master(700, seed=3)])
    p1, p2 = path_of(20, seed=1, spread=0.1), (path_of(20, seed=2, spread=0.1) + F32([0.4, -0.3, 0.2, 0.3, 0.0, -0.2, 0.1])).astype(F32)
    a = _engine(max_obs=1024)
    a.set_obstacles(master)
    i1, _ = focus_and_check(a, master, p1, 0.05, what="p1")
    a.focus_obstacles_path(p2, 0.05)
    i2 = a.obstacle_focus()
    assert not np.array_equal(i1, i2) and np.array_equal(bits(a.get_obstacles()), bits(master[i2]))
    a.focus_obstacles(_q0(), 0.05)          # the single-state call selects from the same master, and the path call after it again
    assert np.array_equal(bits(a.get_obstacles()), bits(master[a.obstacle_focus()]))
    a.focus_obstacles_path(p2, 0.05)
    assert np.array_equal(a.obstacle_focus(), i2)
    a.clear_obstacle_focus()
    i3, _ = focus_and_check(a, master, p2, 0.05, what="p2 on the master")
    assert np.array_equal(i3, i2), "the second focus is the definition on the MASTER, not on the first subset"
    a.clear_obstacle_focus()
    assert np.array_equal(bits(a.get_obstacles()), bits(master)) and a.obstacle_focus() is None
    a.close()


def test_state_rules_through_the_path_call():
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import obstacle_focus_spec
    master = shelf()
    e = _engine()
    q_path = path_of(3, spread=0.05)
    spec = obstacle_focus_spec(0.1)

    def raw(spec=spec, path=q_path, ahead=None, n=3):
        return e.lib.omds_focus_obstacles_path(e.h, None if spec is None else C.byref(spec), None if path is None else path.ctypes.data,
                                               None if ahead is None else ahead.ctypes.data, n, None, None)

    assert raw() == ERR_NOT_INITIALISED      # no scene yet
    e.set_obstacles(master)
    table = np.repeat(master[None], H, 0).copy()
    table[1:, :, 2] += F32(0.01)
    e.set_obstacle_horizon(table)      # a master with an explicit horizon table is refused, the scene intact
    assert raw() == ERR_UNSUPPORTED
    got, mode = e.get_obstacle_horizon()
    assert mode == 2 and np.array_equal(bits(got), bits(table)) and e.obstacle_focus() is None
    e.set_obstacle_horizon(None)
    vel = np.full((len(master), 3), 0.01, F32)
    e.set_obstacle_motion(vel)
    idx, _ = focus_and_check(e, master, q_path, 0.1, 0, 0.5, np.array([0, 0.5, 1.0], F32), vel, "state")
    scene, motion = e.get_obstacles(), e.get_obstacle_motion()[0]

    def unchanged():
        assert np.array_equal(e.obstacle_focus(), idx) and np.array_equal(bits(e.get_obstacles()), bits(scene))
        assert np.array_equal(bits(e.get_obstacle_motion()[0]), bits(motion)) and e.get_obstacle_horizon()[1] == 1

    v = vel[idx].copy()
    for call in (lambda: e.lib.omds_set_obstacle_motion(e.h, None), lambda: e.lib.omds_set_obstacle_motion(e.h, v.ctypes.data),
                 lambda: e.lib.omds_set_obstacle_horizon(e.h, None, 0)):
        assert call() == ERR_UNSUPPORTED and b"omds_clear_obstacle_focus" in e.lib.omds_last_error(e.h)
        unchanged()
    # argument refusals leave the scene, the master and the focus as they were
    for bad in (obstacle_focus_spec(-0.1), obstacle_focus_spec(np.nan), obstacle_focus_spec(0.1, K - 1), obstacle_focus_spec(0.1, 0, -1.0),
                obstacle_focus_spec(0.1, 0, np.inf), None):
        assert raw(spec=bad) == ERR_INVALID_ARG
        unchanged()
    assert raw(path=None) == ERR_INVALID_ARG
    for n in (0, -1, 65537):
        assert raw(n=n) == ERR_INVALID_ARG
    for bad in (-0.5, np.nan, np.inf):
        assert raw(ahead=np.array([0.0, 0.0, bad], F32)) == ERR_INVALID_ARG and b"ahead" in e.lib.omds_last_error(e.h)
    unchanged()
    e.clear_obstacle_focus()      # the master is still the whole one
    assert np.array_equal(bits(e.get_obstacles()), bits(master)) and np.array_equal(bits(e.get_obstacle_motion()[0]), bits(vel))
    # a setter ends the focus, and its scene is the next master
    e.focus_obstacles_path(q_path, 0.1)
    other = random_master(50, seed=1)
    e.set_obstacles(other)
    assert e.obstacle_focus() is None and np.array_equal(bits(e.get_obstacles()), bits(other))
    focus_and_check(e, other, q_path, 0.05, what="next master")
    e.clear_obstacle_focus()
    assert np.array_equal(bits(e.get_obstacles()), bits(other))
    bare = _engine(network=False)      # no network: not initialised
    bare.set_obstacles(master)
    assert bare.lib.omds_focus_obstacles_path(bare.h, C.byref(spec), q_path.ctypes.data, None, 3, None, None) == ERR_NOT_INITIALISED
    assert np.array_equal(bits(bare.get_obstacles()), bits(master))
    with pytest.raises(_lib.OmdsError):
        bare.focus_obstacles_path(q_path, 0.1)
    bare.close()
    e.close()


def test_objects_master_labels_are_gathered():
    from cloud_object_cases import obj_of, track_of
    from optimalmodulationds_amd.engine import cloud_spec
    prev = np.ascontiguousarray(shelf()[:, :3])
    now = (prev + np.array([-0.4, 1.3, 2.0], F32) * F32(0.05)).astype(F32)
    spec, track, obj = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28)), track_of(3, 0.1), obj_of(1, 4)
    a = _engine()
    a.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    a.set_obstacles_from_cloud_objects(now, spec, track, obj)
    master, (vel, have), (label, flag, n_objects) = a.get_obstacles(), a.get_obstacle_motion(), a.cloud_objects()
    assert have and len(master) > 200
    q_path = path_of(9, spread=0.05)
    idx, _ = focus_and_check(a, master, q_path, 0.05, 0, 0.25, np.linspace(0, 1, 9).astype(F32), vel, "objects master")
    assert K < len(idx) < len(master)
    got_label, got_flag, got_n = a.cloud_objects()
    assert np.array_equal(got_label, label[idx]) and np.array_equal(got_flag, flag[idx]) and got_n == n_objects
    a.clear_obstacle_focus()
    back = a.cloud_objects()
    assert np.array_equal(back[0], label) and np.array_equal(back[1], flag) and back[2] == n_objects
    a.close()


# ---- (f) equality with the full scene where it must hold -------------------------------------------------------------------------------
def test_focus_along_all_states_at_margin_zero_is_the_full_propagate():
    """The master is the shelf and a copy of it moved 0.45 m in y, 588 spheres, with dt = 0.5: a rollout travels up to 0.91 rad.  A
    focus along all N H = 256 states of the full propagate at margin 0 keeps exactly the spheres that are among some state's 10
    nearest (59 on the device; the CPU oracle's own propagate counts 60), so the focused propagate IS the full one.  The
    single-state focus at the start state with margin 0.2 (86 kept, on the device and by the oracle) lacks 9 of them: the difference
    the path focus exists for."""
    near = shelf()
    far = near.copy()
    far[:, 1] += F32(FAR_SHIFT)
    master = np.concatenate([near, far])
    assert len(master) == 588
    full, foc, one = _planner(dt=0.5, max_obs=1024), _planner(dt=0.5, max_obs=1024), _planner(dt=0.5, max_obs=1024)
    for e in (full, foc, one):
        e.set_obstacles(master)
    q = _q0()
    full.propagate(q)
    traj = full.get_rollouts()["all_traj"]
    q_path = np.ascontiguousarray(traj.reshape(N * H, 7))
    idx, _ = focus_and_check(foc, master, q_path, 0.0, what="all states")
    print("kept along all states at margin 0:", len(idx))
    assert K < len(idx) < 588
    nearest = np.concatenate([full.dist_grad(np.ascontiguousarray(traj[:, h]), want_idx=True)[3] for h in range(H)])
    kept = np.zeros(len(master), bool)
    kept[idx] = True
    assert kept[nearest].all(), f"a state has a dropped sphere among its {K} nearest"
    foc.propagate(q)
    _same_rollouts(foc, full, "focused against full")
    assert np.array_equal(bits(foc.cost()), bits(full.cost()))
    n_one = one.focus_obstacles(q, 0.2)[0]
    single = np.zeros(len(master), bool)
    single[one.obstacle_focus()] = True
    print("kept at q0 with margin 0.2:", n_one, "needed spheres it lacks:", int((~single[np.unique(nearest)]).sum()))
    assert not single[nearest].all(), "the single-state focus at margin 0.2 was expected not to cover every state's nearest"
    for e in (full, foc, one):
        e.close()


# ---- (g) the facade ----------------------------------------------------------------------------------------------------------------------
def _mppi(master, vel, lazy):
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    nn_model.model_jit = nn_model
    nn_model.update_aot_lambda()
    q_0, q_f = torch.tensor(scenes.FRANKA_Q0), torch.tensor(scenes.FRANKA_QF)
    dh = torch.tensor(scenes.franka_dh_params())
    mppi = MPPI(q_0, q_f, dh, torch.tensor(master), 0.1, H, N, [LinDS(q_f), LinDS(q_0)], dh[:, 2], nn_model, K, lazy_rollouts=lazy)
    mppi.update_obstacles(master, velocities=vel)
    mppi._push()
    return mppi


@pytest.mark.parametrize("lazy", [False, True])
def test_facade_focus_obstacles_along(lazy):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import obstacle_focus_select, obstacle_focus_select_path
    master = np.concatenate([shelf(), random_master(300, seed=2)])
    vel = (0.05 * np.random.RandomState(4).standard_normal((len(master), 3))).astype(F32)
    mppi = _mppi(master, vel, lazy)
    q0, dt = np.asarray(scenes.FRANKA_Q0, F32), 0.1

    def check(out, want):
        assert out == (len(want[0]), want[1]) and K < out[0] < len(master)
        assert np.array_equal(mppi.obs_focus.numpy(), want[0]) and mppi.n_obs == out[0]
        assert np.array_equal(bits(mppi.obs.numpy()), bits(master[want[0]]))
        assert np.array_equal(bits(mppi.obs_velocities.numpy()), bits(vel[want[0]]))

    # along=None is the single-state call
    d0 = mppi._engine.dist_grad(q0, want_mindist=True)[2][0]
    check(mppi.focus_obstacles(0.1), obstacle_focus_select(d0, K, 0.1, 0, (H - 1) * dt, vel))
    mppi.clear_obstacle_focus()
    # an array of states: q and those states, each with the whole horizon
    states = path_of(12, seed=7, spread=0.2)[1:]
    path = np.concatenate([q0[None], states])
    d = rows_of(mppi._engine, path)
    want = obstacle_focus_select_path(d, K, 0.05, 0, (H - 1) * dt, None, vel)
    check(mppi.focus_obstacles(0.05, along=torch.tensor(states)), want)
    mppi.clear_obstacle_focus()
    check(mppi.focus_obstacles(0.05, along=states), want)
    mppi.clear_obstacle_focus()
    # rollout indices of the last propagate, every step and every second one
    mppi.Policy.sample_policy()
    mppi.propagate()
    traj = mppi._engine.get_rollouts()["all_traj"]
    rows = [5, 0, 63]
    for stride in (1, 2):
        steps = np.arange(0, H, stride)
        path = np.concatenate([q0[None], traj[rows][:, steps].reshape(-1, 7)])
        ahead = np.concatenate([[0.0], np.tile(steps * dt, len(rows))]).astype(F32)
        d = rows_of(mppi._engine, path)
        want = obstacle_focus_select_path(d, K, 0.05, 40, (stride - 1) * dt, ahead, vel)
        out = mppi.focus_obstacles(0.05, max_keep=40, along=rows, stride=stride)
        assert out == (len(want[0]), want[1]) and K <= out[0] <= 40
        assert np.array_equal(mppi.obs_focus.numpy(), want[0]) and np.array_equal(bits(mppi.obs.numpy()), bits(master[want[0]]))
        mppi.clear_obstacle_focus()
    with pytest.raises(ValueError):
        mppi.focus_obstacles(0.05, along=[N])
    mppi.focus_obstacles(0.05, along=rows)
    mppi.propagate()
    assert np.isfinite(mppi._engine.get_rollouts()["all_traj"]).all()
    mppi.update_obstacles(master[:100])
    assert mppi.obs_focus is None and mppi._engine.obstacle_focus() is None
