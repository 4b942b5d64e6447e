"""Sphere velocities from successive point clouds on the device (include/omds.h: omds_set_obstacles_from_cloud_tracked;
csrc/cloud_kernels.hip: k_cloud_count_rec, the cell indices through both compactions; csrc/cloud_track_kernels.hip: k_cloud_flow) against the host definition
(omds_point_cloud_flow, checked on its own in tests/test_cloud_flow_cpu.py) -- all bit for bit: the records are integer sums, the
window search is integer, and the fp32 lines are one source for host and kernel.

Shapes: k_cloud_flow runs one wave per final sphere, four per workgroup: 1, 3 and 5 spheres are partial workgroups, 35 (the slab) and
the thousands of the random cloud whole ones plus a rest.  reach 1 .. 4 gives windows of 27 .. 729 cells (less or more than the 64
lanes of a wave); corner cells and grids thinner than the window clip it."""
import functools

import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import cloud_flow_cases as cases
from cloud_cases import F32, spec_of
from cloud_flow_cases import track_of
from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

K = 5
PAD = (10.0, 10.0, 10.0, 0.0)      # cloud_spec's default pad sphere
KEYS = ("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal")
ERR_INVALID_ARG = 1


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def flow(prev, now, spec, track):
    from optimalmodulationds_amd.engine import point_cloud_flow
    return point_cloud_flow(prev, now, spec, track, cap=65536)


@functools.lru_cache(maxsize=None)
def _net(kind):
    return orc.Mlp.from_npz(weights_path(kind))


def _q0():
    from optimalmodulationds_amd import scenes
    return np.asarray(scenes.FRANKA_Q0, F32)


def _engine(kind="franka", N=32, H=3, k=K, max_obs=64, ignored=0b111):
    from optimalmodulationds_amd.engine import Engine
    e = Engine(7, N, H, k, max_obs=max_obs)
    if kind is not None:
        m = _net(kind)
        e.set_mlp(m.W, m.b, act=m.act)
    e.params.dt, e.params.dst_thr, e.params.ignored_links = 0.5, 0.01, ignored
    e.push_params()
    return e


def padded(vel, n_obs):
    return np.concatenate([vel, np.zeros((n_obs - len(vel), 3), F32)])


def assert_scene_is_the_definition(e, got, spec, track, prev, now, what=""):
    """the scene and the velocities in force are omds_point_cloud_flow(prev, now), padding spheres at rest"""
    spheres, vel, matched = flow(prev, now, spec, track)
    assert got == (len(spheres), len(spheres), matched), (what, got, len(spheres), matched)
    scene, (motion, have) = e.get_obstacles(), e.get_obstacle_motion()
    assert e.n_obs == max(len(spheres), e.k) and scene.shape == (e.n_obs, 4) and motion.shape == (e.n_obs, 3)
    assert np.array_equal(bits(scene[:len(spheres)]), bits(spheres)) and (scene[len(spheres):] == F32(PAD)).all(), what
    assert np.array_equal(bits(motion), bits(padded(vel, e.n_obs))), f"{what}: the device velocities are not the definition's"
    assert have == bool((vel != 0).any()), what
    if e.C or not have:      # (the tables of a motion horizon need the network)
        assert e.get_obstacle_horizon()[1] == (1 if have else 0), what
    return spheres, vel, matched


# ---- 1. device against the definition ---------------------------------------------------------------------------------------------
def _pair(name):
    if name == "slab":
        return (*cases.slab(), 3)
    if name == "slab-reach1":
        return (*cases.slab(), 1)
    if name == "corners":
        return (*cases.corners(), 1)
    if name == "corners-reach4":
        return (*cases.corners(), 4)
    if name == "faces":
        return (*cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7), 2)
    if name == "37x29x1":
        return (*cases.random_pair(5, (37, 29, 1), 400, 400, shift=(1.6, -0.7, 0.0), fill=0.8), 3)
    if name == "thin-reach4":
        return (*cases.random_pair(6, (3, 2, 5), 12, 25, shift=(0.0, 0.0, 0.0)), 4)
    if name.startswith("spheres-"):
        return (*cases.few_spheres(int(name[-1])), 2)
    if name.startswith("ties-"):
        return (*cases.ties(int(name[-1])), 2)
    if name == "heavy":
        return (*cases.heavy(), 1)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["slab", "slab-reach1", "corners", "corners-reach4", "faces", "37x29x1", "thin-reach4", "spheres-1", "spheres-3",
                                  "spheres-5", "ties-2", "ties-4", "ties-8", "heavy"])
def test_device_velocities_are_the_definition(name):
    spec, prev, now, reach = _pair(name)
    track = track_of(reach, 0.125)
    e = _engine(None)
    first = e.set_obstacles_from_cloud_tracked(prev, spec, track)
    assert first[2] == -1 and not e.get_obstacle_motion()[1]
    got = e.set_obstacles_from_cloud_tracked(now, spec, track)
    spheres, vel, matched = assert_scene_is_the_definition(e, got, spec, track, prev, now, name)
    if name == "slab":
        assert matched == 35 and (vel == F32([1.125, 0, 0])).all()
    if name == "slab-reach1":
        assert matched == 0 and len(spheres) == 35
    e.close()


def test_random_cloud_shuffled_and_device_resident():
    """20 000 points in 24 x 24 x 24 cells that moved by (0.4, -1.3, 2.0) cells: thousands of final spheres (several compaction blocks,
    many workgroups of k_cloud_flow), windows of 125 cells; then the same pair shuffled, and passed as device tensors"""
    spec, prev, now = cases.random_pair(8, (24, 24, 24), 20000, 20000, voxel=0.05, origin=(-0.6, -0.6, 0.0))
    track = track_of(2, 0.1, still=0.2)
    e = _engine(None)
    e.set_obstacles_from_cloud_tracked(prev, spec, track)
    got = e.set_obstacles_from_cloud_tracked(now, spec, track)
    spheres, vel, matched = assert_scene_is_the_definition(e, got, spec, track, prev, now, "random")
    assert len(spheres) > 5000 and matched > 0.9 * len(spheres) and (vel == 0).all(1).any() and (vel != 0).any(1).sum() > 1000
    rng = np.random.RandomState(5)
    prev_s, now_s = prev[rng.permutation(len(prev))], now[rng.permutation(len(now))]
    e.set_obstacles_from_cloud_tracked(prev_s, spec, track)      # the grid is the stored one: this frame is matched against `now`
    got = e.set_obstacles_from_cloud_tracked(now_s, spec, track)
    assert_scene_is_the_definition(e, got, spec, track, prev, now, "shuffled")
    dev = f"cuda:{e.device}"
    e.set_obstacles_from_cloud_tracked(torch.from_numpy(prev_s).to(dev), spec, track)
    got = e.set_obstacles_from_cloud_tracked(torch.from_numpy(now_s).to(dev), spec, track)
    assert_scene_is_the_definition(e, got, spec, track, prev, now, "device tensors")
    e.close()


# ---- 2. first call, grid change, reset --------------------------------------------------------------------------------------------
def test_no_previous_frame_on_first_call_grid_change_and_reset():
    spec, prev, now = cases.slab()
    track = track_of(3, 0.125)
    e = _engine("franka")

    def stands_still(got):
        assert got == (35, 35, -1) and e.get_obstacle_horizon()[1] == 0 and e.get_obstacle_motion()[1] is False
        assert not e.get_obstacle_motion()[0].any()

    stands_still(e.set_obstacles_from_cloud_tracked(prev, spec, track))
    assert e.set_obstacles_from_cloud_tracked(now, spec, track) == (35, 35, 35) and e.get_obstacle_horizon()[1] == 1
    ulp = spec_of((0.0, 0.0, 0.0), np.nextafter(F32(0.0625), F32(1)), (16, 12, 8))
    assert ulp.voxel != spec.voxel
    stands_still(e.set_obstacles_from_cloud_tracked(prev, ulp, track))
    assert e.set_obstacles_from_cloud_tracked(prev, ulp, track)[2] == 35            # the same cloud on the new grid: matched, at rest
    for other in (spec_of((0.0, 0.0, 0.0), 0.0625, (16, 12, 9)), spec_of((0.0, 0.0, -0.0), 0.0625, (16, 12, 9)),
                  spec_of((0.0, 0.0, -0.0), 0.0625, (16, 12, 9), min_points=2)):
        stands_still(e.set_obstacles_from_cloud_tracked(prev, other, track))
    stands_still(e.set_obstacles_from_cloud_tracked(prev, spec, track))
    assert e.set_obstacles_from_cloud_tracked(now, spec, track) == (35, 35, 35)
    e.cloud_track_reset()
    stands_still(e.set_obstacles_from_cloud_tracked(now, spec, track))
    e.close()


# ---- 3. the installed horizon -----------------------------------------------------------------------------------------------------
def test_installed_horizon_is_the_prediction_of_the_definition():
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    spec, prev, now = cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7)
    track = track_of(2, 0.1)
    e = _engine("franka", H=4)
    e.set_obstacles_from_cloud_tracked(prev, spec, track)
    got = e.set_obstacles_from_cloud_tracked(now, spec, track)
    spheres, vel, _ = assert_scene_is_the_definition(e, got, spec, track, prev, now)
    table, mode = e.get_obstacle_horizon()
    assert mode == 1 and np.array_equal(bits(table), bits(predict_obstacle_horizon(spheres, vel, 4, 0.5)))
    e.close()


# ---- 4. / 5. the propagate that follows -------------------------------------------------------------------------------------------
def _samples(N, seed=3, Kp=3):
    rng = np.random.RandomState(seed)
    mu = (_q0() + 0.2 * rng.standard_normal((N, Kp, 7))).astype(F32)
    return mu, np.ones((N, Kp), F32), rng.standard_normal((N, Kp, 7)).astype(F32)


def _planner(N=64, H=4):
    from optimalmodulationds_amd import scenes
    e = _engine("franka", N=N, H=H, max_obs=512)
    e.set_ds(scenes.FRANKA_QF)
    e.set_policy_samples(*_samples(N))
    return e


def _shelf_clouds():
    """the shelf's 294 sphere centres as a cloud, and the same cloud (-0.4, 1.3, 2.0) cells further: about 300 spheres in front of the arm"""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import cloud_spec
    prev = np.ascontiguousarray(scenes.shelf_scene()[:, :3])
    now = (prev + np.array([-0.4, 1.3, 2.0], F32) * F32(0.05)).astype(F32)
    return cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28)), prev, now


def _same_rollouts(a, b, what):
    ra, rb = a.get_rollouts(), b.get_rollouts()
    for key in KEYS:
        assert np.array_equal(bits(ra[key]), bits(rb[key])), (what, key)
    assert np.isfinite(ra["all_traj"]).all()


def test_static_scene_keeps_the_static_propagate():
    spec, prev, _ = _shelf_clouds()
    a, b = _planner(), _planner()
    track = track_of(2, 0.1)
    a.set_obstacles_from_cloud_tracked(prev, spec, track)
    n, occ, matched = a.set_obstacles_from_cloud_tracked(prev, spec, track)
    assert n == occ == matched > 200 and a.get_obstacle_horizon()[1] == 0 and not a.get_obstacle_motion()[1]
    assert b.set_obstacles_from_cloud(prev, spec) == (n, occ)
    a.prof_enable(1)
    b.prof_enable(1)
    a.propagate(_q0())
    b.propagate(_q0())
    _same_rollouts(a, b, "static")
    assert a.prof_read_ex()[1] == b.prof_read_ex()[1], "another number of launches"
    a.close()
    b.close()


@pytest.mark.parametrize("screen", [False, True])
@pytest.mark.parametrize("frame", [False, True])
def test_propagate_equals_set_obstacles_plus_motion(frame, screen):
    spec, prev, now = _shelf_clouds()
    track = track_of(3, 0.1)
    spheres, vel, matched = flow(prev, now, spec, track)
    assert 250 <= len(spheres) <= 300 and matched == len(spheres) and (vel != 0).any(1).all()
    a, b = _planner(), _planner()
    for e in (a, b):
        e.set_screening(1 if screen else 0)
        e.set_screening_horizon(screen)
        e.set_obstacle_frame(frame)
    a.set_obstacles_from_cloud_tracked(prev, spec, track)
    assert a.set_obstacles_from_cloud_tracked(now, spec, track) == (len(spheres), len(spheres), matched)
    b.set_obstacles(spheres)
    b.set_obstacle_motion(vel)
    assert a.get_obstacle_frame() == b.get_obstacle_frame() and a.get_obstacle_frame()[2] == frame
    for q in (_q0(), (_q0() + F32(0.05)).astype(F32)):
        a.propagate(q)
        b.propagate(q)
        _same_rollouts(a, b, (frame, screen))
    sa, sb = a.screen_stats(), b.screen_stats()
    assert sa["active"] == sb["active"] == screen and sa["eps"] == sb["eps"] and sa["fallbacks"] == sb["fallbacks"]
    a.close()
    b.close()


# ---- 6. self-filter on ------------------------------------------------------------------------------------------------------------
def _rows_of(spheres, kept):
    """row of every kept sphere in the definition's list (the definition has no filter): by sphere equality"""
    index = {s.tobytes(): i for i, s in enumerate(spheres)}
    return np.array([index[s.tobytes()] for s in kept], np.int64)


def test_self_filter_keeps_the_untracked_list_and_the_definitions_rows():
    from optimalmodulationds_amd.engine import cloud_spec
    spec = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), max_spheres=8192, self_margin=0.03)
    lo, ext = np.array((-0.8, -0.8, -0.1), F32), np.array((32, 32, 28)) * 0.05
    rng = np.random.RandomState(7)
    prev = (lo + rng.uniform(0, 1, (6000, 3)) * ext).astype(F32)
    now = (prev + np.array([0.4, -1.3, 2.0], F32) * F32(0.05)).astype(F32)
    track = track_of(2, 0.1)
    spheres, vel, _ = flow(prev, now, spec, track)
    a, b = _engine("franka"), _engine("franka")
    n_b, occ_b = b.set_obstacles_from_cloud(now, spec, q=_q0())
    a.set_obstacles_from_cloud_tracked(prev, spec, track, q=_q0())
    n, occ, matched = a.set_obstacles_from_cloud_tracked(now, spec, track, q=_q0())
    assert (n, occ) == (n_b, occ_b) and occ == len(spheres) and 10 <= occ - n, "the filter must have dropped some"
    kept = a.get_obstacles()
    assert np.array_equal(bits(kept), bits(b.get_obstacles())) and len(kept) == n
    rows = _rows_of(spheres, kept)
    assert (np.diff(rows) > 0).all()
    motion, have = a.get_obstacle_motion()
    assert have and np.array_equal(bits(motion), bits(vel[rows]))
    mask = cases.restate_flow(spec, track, prev, now, with_mask=True)[4]
    assert matched == int(mask[rows].sum()) < int(mask.sum()), "n_matched counts the kept spheres with a non-empty window"
    a.close()
    b.close()


def test_self_filter_with_padding():
    """three spheres survive the filter (one point sits on the arm), n_closest is 5: two pad spheres, at rest"""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import cloud_spec
    ends = orc.link_endpoints(_q0(), scenes.franka_dh_params())
    on_arm = (0.5 * (ends[3] + ends[4])).astype(F32)
    far = np.array([[0.6, 0.6, 1.2], [-0.7, 0.5, 0.2], [0.1, -0.75, 1.0]], F32)
    now = np.concatenate([far, on_arm[None]])
    prev = (now - np.array([0.06, 0.0, -0.03], F32)).astype(F32)
    pad = (3.0, -2.0, 1.5, 0.25)
    spec = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), self_margin=0.03, pad=pad)
    track = track_of(2, 0.1)
    spheres, vel, _ = flow(prev, now, spec, track)
    e = _engine("franka", k=5)
    e.set_obstacles_from_cloud_tracked(prev, spec, track, q=_q0())
    assert e.set_obstacles_from_cloud_tracked(now, spec, track, q=_q0()) == (3, 4, 3)
    scene, (motion, have) = e.get_obstacles(), e.get_obstacle_motion()
    rows = _rows_of(spheres, scene[:3])
    assert have and (scene[3:] == F32(pad)).all() and np.array_equal(bits(motion), bits(padded(vel[rows], 5))) and (vel[rows] != 0).any(1).all()
    e.close()


# ---- 7. a refusal changes nothing -------------------------------------------------------------------------------------------------
def test_a_refusal_leaves_the_scene_and_the_stored_frame():
    from optimalmodulationds_amd import _lib as L
    spec, prev, now = cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7)
    other = cases.random_pair(11, (12, 10, 9), 900, 900)[2]
    track = track_of(2, 0.1)
    e = _engine("franka")
    e.set_obstacles_from_cloud_tracked(prev[:300], spec, track)
    got = e.set_obstacles_from_cloud_tracked(prev, spec, track)
    before = assert_scene_is_the_definition(e, got, spec, track, prev[:300], prev)
    assert (before[1] != 0).any()
    scene, motion = e.get_obstacles(), e.get_obstacle_motion()
    small = spec_of(tuple(spec.origin), spec.voxel, tuple(spec.dims), max_spheres=50)          # the same grid, too few spheres allowed
    for refuse in (lambda: e.set_obstacles_from_cloud_tracked(other, small, track), lambda: e.set_obstacles_from_cloud_tracked(other, small, track, q=_q0()),
                   lambda: e.set_obstacles_from_cloud_tracked(other, spec, track_of(0, 0.1)), lambda: e.set_obstacles_from_cloud_tracked(other, spec, track_of(2, 0.0)),
                   lambda: e.set_obstacles_from_cloud_tracked(other, spec_of((0, 0, 0), 0.0, (4, 4, 4)), track)):
        with pytest.raises(L.OmdsError, match=f"omds error {ERR_INVALID_ARG}"):
            refuse()
        assert np.array_equal(bits(e.get_obstacles()), bits(scene)) and e.get_obstacle_horizon()[1] == 1
        assert np.array_equal(bits(e.get_obstacle_motion()[0]), bits(motion[0]))
    got = e.set_obstacles_from_cloud_tracked(now, spec, track)                                  # ... against the frame from before the refusals
    assert_scene_is_the_definition(e, got, spec, track, prev, now)
    e.close()


# ---- 8. the untracked call is untouched -------------------------------------------------------------------------------------------
def test_untracked_call_between_two_tracked_ones():
    from optimalmodulationds_amd.engine import point_cloud_spheres
    spec, prev, now = cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7)
    other_spec, _, other = cases.random_pair(11, (16, 16, 8), 900, 5003)
    track = track_of(2, 0.1)
    e = _engine(None)
    e.set_obstacles_from_cloud_tracked(prev, spec, track)
    for s in (other_spec, spec):
        want = point_cloud_spheres(other, s, cap=65536)
        assert e.set_obstacles_from_cloud(other, s) == (len(want), len(want)) and len(want) > 100
        assert np.array_equal(bits(e.get_obstacles()), bits(want)) and e.get_obstacle_horizon()[1] == 0
    e.set_obstacles(np.array([[1.0, 1.0, 1.0, 0.1]] * K, F32))
    got = e.set_obstacles_from_cloud_tracked(now, spec, track)
    assert_scene_is_the_definition(e, got, spec, track, prev, now)
    e.close()


# ---- the facade -------------------------------------------------------------------------------------------------------------------
def test_facade_takes_the_tracked_route_with_dt_frame():
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    from optimalmodulationds_amd.engine import point_cloud_spheres
    spec, prev, now = _shelf_clouds()
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    mppi = MPPI(torch.tensor(_q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 4, 32, [LinDS(q_f)], dh[:, 2], nn_model, K)
    mppi.dst_thr = 0.01
    lo, hi = (-0.8, -0.8, -0.1), (0.8, 0.8, 1.3)
    spheres, vel, matched = flow(prev, now, spec, track_of(3, 0.1))
    n_prev = len(point_cloud_spheres(prev, spec))
    assert mppi.update_obstacles_from_cloud(prev, 0.05, lo, hi, dt_frame=0.1, reach=3) == (n_prev, n_prev)
    assert mppi.obs_velocities is None and mppi.cloud_matched == -1
    assert mppi.update_obstacles_from_cloud(now, 0.05, lo, hi, dt_frame=0.1, reach=3, moving_frame=True) == (len(spheres), len(spheres))
    assert mppi.cloud_matched == matched and isinstance(mppi.obs_velocities, torch.Tensor) and mppi.obs_velocities.device.type == "cpu"
    assert np.array_equal(bits(mppi.obs_velocities.numpy()), bits(vel)) and np.array_equal(bits(mppi.obs.numpy()), bits(spheres))
    assert mppi._engine.get_obstacle_frame() == (True, 1.0, True) and mppi._engine.get_obstacle_horizon()[1] == 1
    assert np.isfinite(mppi.propagate()[0].numpy()).all()
    assert mppi.update_obstacles_from_cloud(now, 0.05, lo, hi) == (len(spheres), len(spheres))          # without dt_frame: as before
    assert mppi.obs_velocities is None and mppi.cloud_matched is None and mppi._engine.get_obstacle_horizon()[1] == 0
    assert mppi._engine.get_obstacle_frame()[0] is False
    assert mppi.update_obstacles_from_cloud(now, 0.05, lo, hi, dt_frame=0.1, still=1e3)[0] == len(spheres)   # everything under still
    assert mppi.obs_velocities is None and mppi.cloud_matched == len(spheres)
