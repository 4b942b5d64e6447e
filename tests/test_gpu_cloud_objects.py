"""Object velocities from successive point clouds on the device (include/omds.h: omds_set_obstacles_from_cloud_objects;
csrc/cloud_track_kernels.hip: k_obj_slot, k_obj_union, k_obj_flatten, k_obj_sums, the component table through the ordered compaction,
k_obj_match, k_obj_apply) against the host definition (omds_point_cloud_object_flow, checked on its own in
tests/test_cloud_objects_cpu.py) -- all bit for bit: components and their sums are integers, and the fp64 / fp32 lines are one source
for host and kernel.

Shapes: one lane per sphere in workgroups of 256 (1, 4, 16, 27, 36 spheres: part of one wave; 1 008 and thousands: several
workgroups, runs of equal roots that cross waves and workgroups); one wave per component in the match (1, 2, 8 and hundreds of
components; previous tables shorter and longer than the 64 lanes)."""
import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import cloud_object_cases as cases
import test_gpu_cloud_flow as base
from cloud_cases import F32, spec_of
from cloud_object_cases import obj_of, track_of

pytestmark = pytest.mark.gpu

K = base.K
ERR_INVALID_ARG = 1
bits = base.bits


def objflow(prev, now, spec, track, obj, keep_prev=None, keep_now=None):
    from optimalmodulationds_amd.engine import point_cloud_object_flow
    return point_cloud_object_flow(prev, now, spec, track, obj, keep_prev, keep_now, cap=65536)


def assert_scene(e, got, want, what="", pad=base.PAD):
    """scene, velocities, labels and flags in force are ``want`` = objflow(...) (padding: at rest, label -1, no object) and ``got`` the
    call's counts; want[6] None: no previous table was expected"""
    spheres, vel, label, flag, matched, n_obj, n_acc = want
    n = len(spheres)
    assert got[0] == n and got[2:] == (matched, n_obj, -1 if n_acc is None else n_acc), (what, got, want[4:])
    scene, (motion, have) = e.get_obstacles(), e.get_obstacle_motion()
    assert e.n_obs == max(n, e.k) and scene.shape == (e.n_obs, 4)
    assert np.array_equal(bits(scene[:n]), bits(spheres)) and (scene[n:] == F32(pad)).all(), what
    assert np.array_equal(bits(motion), bits(base.padded(vel, e.n_obs))), f"{what}: the device velocities are not the definition's"
    assert have == bool((vel != 0).any()), what
    got_label, got_flag, got_n = e.cloud_objects()
    assert np.array_equal(got_label, np.concatenate([label, np.full(e.n_obs - n, -1, np.int32)])), f"{what}: labels"
    assert np.array_equal(got_flag, np.concatenate([flag, np.zeros(e.n_obs - n, np.int32)])), f"{what}: object flags"
    assert got_n == n_obj, what


def fallback_of(prev, now, spec, track, obj, have_frame=True):
    """what a call without a previous table must give: the definition's list and labels, the tracked call's velocities, no object"""
    spheres, _, label, flag, _, n_obj, _ = objflow(prev, now, spec, track, obj)
    if have_frame:
        _, vel, matched = base.flow(prev, now, spec, track)
    else:
        vel, matched = np.zeros((len(spheres), 3), F32), -1
    return spheres, vel, label, np.zeros_like(flag), matched, n_obj, None


# ---- 1. device against the definition ---------------------------------------------------------------------------------------------
def _pair(name):
    if name == "ball":
        return (*cases.ball(), track_of(2, 0.125), obj_of(1, 4))
    if name == "plate":
        return (*cases.plate(), track_of(1, 0.125), obj_of(1, 4))
    if name == "serpentine":
        return (*cases.serpentine(), track_of(1, 0.1), obj_of(1, 4))
    if name == "corner-touch":
        return (*cases.blobs(-1), track_of(1, 0.1), obj_of(1, 1))
    if name == "gap1-link1":
        return (*cases.blobs(1), track_of(1, 0.1), obj_of(1, 1))
    if name == "gap1-link2":
        return (*cases.blobs(1), track_of(1, 0.1), obj_of(2, 1))
    if name == "gap2-link2":
        return (*cases.blobs(2), track_of(1, 0.1), obj_of(2, 1))
    if name == "corners":
        return (*cases.corner_components(), track_of(2, 0.25), obj_of(1, 2))
    if name == "corners-link2":
        return (*cases.corner_components(), track_of(2, 0.25), obj_of(2, 2))
    if name == "37x29x1":
        return (*cases.random_pair(5, (37, 29, 1), 400, 400, shift=(1.6, -0.7, 0.0), fill=0.8), track_of(3, 0.1), obj_of(2, 3))
    if name == "thin-link2":
        return (*cases.random_pair(6, (3, 2, 5), 12, 25, shift=(0.0, 0.0, 0.0)), track_of(4, 0.1), obj_of(2, 1))
    if name == "mass-2to1":
        return (*cases.line_pair(4, 8), track_of(4, 0.1), obj_of(1, 4))
    if name == "mass-over":
        return (*cases.line_pair(4, 9), track_of(4, 0.1), obj_of(1, 4))
    if name.startswith("reach-"):
        return (*cases.reach_edge(name[6:])[:3], track_of(2, 0.1), obj_of(1, 1))
    if name == "one-sphere":
        return (*cases.equidistant(), track_of(1, 0.5), obj_of(1, 1))
    if name == "heavy":
        return (*cases.heavy(), track_of(1, 0.1), obj_of(1, 4))
    if name == "mixed":
        return (*cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7), track_of(2, 0.1, still=0.3), obj_of(1, 6))
    raise KeyError(name)


@pytest.mark.parametrize("name", ["ball", "plate", "serpentine", "corner-touch", "gap1-link1", "gap1-link2", "gap2-link2", "corners", "corners-link2",
                                  "37x29x1", "thin-link2", "mass-2to1", "mass-over", "reach-below", "reach-at", "reach-above", "one-sphere",
                                  "heavy", "mixed"])
def test_device_objects_are_the_definition(name):
    spec, prev, now, track, obj = _pair(name)
    e = base._engine(None)
    none = np.zeros((0, 3), F32)
    first = e.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    assert_scene(e, first, fallback_of(none, prev, spec, track, obj, have_frame=False), name + ": first call")
    got = e.set_obstacles_from_cloud_objects(now, spec, track, obj)
    want = objflow(prev, now, spec, track, obj)
    assert_scene(e, got, want, name)
    if name == "ball":
        assert want[5:] == (1, 1) and (want[1] == F32([0.5625, 0, 0])).all()
    if name == "plate":
        assert (want[3] == 1).all() and (want[1] == F32([0.25, 0, 0])).all()
    if name == "serpentine":
        assert len(want[0]) == 1008 and (want[2] == 5).all() and want[6] == 1
    if name in ("mass-over", "reach-above"):
        assert want[5:] == (1, 0)
    e.close()


def test_dense_cloud_shuffled_and_device_resident():
    """20 000 points in 24 x 24 x 24 cells: thousands of final spheres in ONE component (every sphere's sums go to the same five words: the
    contended case); then the same pair shuffled, and passed as device tensors"""
    spec, prev, now = cases.dense_pair()
    track, obj = track_of(3, 0.1, still=0.2), obj_of(1, 4)
    want = objflow(prev, now, spec, track, obj)
    counts = np.unique(want[2], return_counts=True)[1]
    assert len(want[0]) > 5000 and counts.max() > 2000 and want[6] >= 1 and (want[3] == 1).sum() > 2000
    e = base._engine(None)
    e.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    assert_scene(e, e.set_obstacles_from_cloud_objects(now, spec, track, obj), want, "dense")
    rng = np.random.RandomState(5)
    prev_s, now_s = prev[rng.permutation(len(prev))], now[rng.permutation(len(now))]
    e.set_obstacles_from_cloud_objects(prev_s, spec, track, obj)
    assert_scene(e, e.set_obstacles_from_cloud_objects(now_s, spec, track, obj), want, "shuffled")
    dev = f"cuda:{e.device}"
    e.set_obstacles_from_cloud_objects(torch.from_numpy(prev_s).to(dev), spec, track, obj)
    assert_scene(e, e.set_obstacles_from_cloud_objects(torch.from_numpy(now_s).to(dev), spec, track, obj), want, "device tensors")
    e.close()


def test_link_two_on_the_dense_cloud():
    spec, prev, now = cases.dense_pair()
    track, obj = track_of(3, 0.1), obj_of(2, 8)
    e = base._engine(None)
    e.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    assert_scene(e, e.set_obstacles_from_cloud_objects(now, spec, track, obj), objflow(prev, now, spec, track, obj), "dense, link 2")
    e.close()


# ---- 2. the previous table --------------------------------------------------------------------------------------------------------
def test_no_previous_table():
    spec, prev, now = cases.ball()
    track, obj = track_of(2, 0.125), obj_of(1, 4)
    none = np.zeros((0, 3), F32)
    e = base._engine(None)
    want = objflow(prev, now, spec, track, obj)

    def fresh(got, a, b, have_frame, o=obj, s=spec):
        assert_scene(e, got, fallback_of(a, b, s, track, o, have_frame), "no table")

    fresh(e.set_obstacles_from_cloud_objects(prev, spec, track, obj), none, prev, False)                       # the first call
    assert_scene(e, e.set_obstacles_from_cloud_objects(now, spec, track, obj), want)
    e.cloud_track_reset()
    fresh(e.set_obstacles_from_cloud_objects(prev, spec, track, obj), none, prev, False)                       # after the reset
    assert_scene(e, e.set_obstacles_from_cloud_objects(now, spec, track, obj), want)
    ulp = spec_of((0.0, 0.0, 0.0), np.nextafter(F32(0.0625), F32(1)), (16, 12, 12))
    fresh(e.set_obstacles_from_cloud_objects(prev, ulp, track, obj), none, prev, False, s=ulp)                 # one ulp of voxel
    fresh(e.set_obstacles_from_cloud_objects(prev, spec, track, obj), none, prev, False)
    for other in (obj_of(2, 4), obj_of(1, 5)):                                                                 # another link / min_cells:
        fresh(e.set_obstacles_from_cloud_objects(now, spec, track, other), prev, now, True, o=other)           # records yes, table no
        fresh(e.set_obstacles_from_cloud_objects(prev, spec, track, obj), now, prev, True)
    assert_scene(e, e.set_obstacles_from_cloud_objects(now, spec, track, obj), want)
    assert e.set_obstacles_from_cloud_tracked(prev, spec, track)[2] >= 0                                      # a plain tracked call in between
    with pytest.raises(Exception, match="omds error"):
        e.cloud_objects()                                                                                      # ... installs no labels
    fresh(e.set_obstacles_from_cloud_objects(now, spec, track, obj), prev, now, True)
    e.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    other_spec, _, other = cases.random_pair(11, (16, 16, 8), 900, 5003)
    e.set_obstacles_from_cloud(other, other_spec)                                                              # an untracked call and a plain
    e.set_obstacles_from_cloud(other, spec)                                                                    # scene in between change nothing
    e.set_obstacles(np.array([[1.0, 1.0, 1.0, 0.1]] * K, F32))
    assert_scene(e, e.set_obstacles_from_cloud_objects(now, spec, track, obj), want, "after untracked calls")
    e.close()


# ---- 3. self-filter ---------------------------------------------------------------------------------------------------------------
def _keep_of(spheres, kept):
    keep = np.zeros(len(spheres), np.uint8)
    keep[base._rows_of(spheres, kept)] = 1
    return keep


def test_self_filter_keeps_the_untracked_list_and_the_definitions_rows():
    from optimalmodulationds_amd.engine import cloud_spec, point_cloud_spheres
    spec = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), max_spheres=8192, self_margin=0.03)
    lo, ext = np.array((-0.8, -0.8, -0.1), F32), np.array((32, 32, 28)) * 0.05
    rng = np.random.RandomState(7)
    prev = (lo + rng.uniform(0, 1, (6000, 3)) * ext).astype(F32)
    now = (prev + np.array([0.4, -1.3, 2.0], F32) * F32(0.05)).astype(F32)
    track, obj = track_of(3, 0.1), obj_of(1, 3)
    q0 = base._q0()
    a, b = base._engine("franka"), base._engine("franka")
    first = a.set_obstacles_from_cloud_objects(prev, spec, track, obj, q=q0)
    kept_prev = a.get_obstacles()[:first[0]]
    n_b, occ_b = b.set_obstacles_from_cloud(now, spec, q=q0)
    got = a.set_obstacles_from_cloud_objects(now, spec, track, obj, q=q0)
    kept = a.get_obstacles()
    assert got[:2] == (n_b, occ_b) and occ_b - n_b >= 10 and first[1] - first[0] >= 10, "the filter must have dropped some in both frames"
    assert np.array_equal(bits(kept), bits(b.get_obstacles()))
    keep_prev, keep_now = _keep_of(point_cloud_spheres(prev, spec, cap=65536), kept_prev), _keep_of(point_cloud_spheres(now, spec, cap=65536), kept)
    want = objflow(prev, now, spec, track, obj, keep_prev, keep_now)
    assert want[6] >= 1 and (want[3] == 1).any() and (want[3] == 0).any()
    assert got[1] == len(keep_now)
    assert_scene(a, (got[0], got[0]) + got[2:], want, "self-filter")
    a.close()
    b.close()


def test_self_filter_with_padding():
    """three spheres survive the filter (one point sits on the arm), n_closest is 5: two pad spheres, at rest, label -1, no object"""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import cloud_spec, point_cloud_spheres
    ends = base.orc.link_endpoints(base._q0(), scenes.franka_dh_params())
    on_arm = (0.5 * (ends[3] + ends[4])).astype(F32)
    far = np.array([[0.6, 0.6, 1.2], [-0.7, 0.5, 0.2], [0.1, -0.75, 1.0]], F32)
    now = np.concatenate([far, on_arm[None]])
    prev = (now - np.array([0.06, 0.0, -0.03], F32)).astype(F32)
    pad = (3.0, -2.0, 1.5, 0.25)
    spec = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), self_margin=0.03, pad=pad)
    track, obj = track_of(2, 0.1), obj_of(1, 1)
    e = base._engine("franka", k=5)
    first = e.set_obstacles_from_cloud_objects(prev, spec, track, obj, q=base._q0())
    keep_prev = _keep_of(point_cloud_spheres(prev, spec), e.get_obstacles()[:first[0]])
    got = e.set_obstacles_from_cloud_objects(now, spec, track, obj, q=base._q0())
    assert got[:2] == (3, 4)
    keep_now = _keep_of(point_cloud_spheres(now, spec), e.get_obstacles()[:3])
    want = objflow(prev, now, spec, track, obj, keep_prev, keep_now)
    assert want[5:] == (3, 3) and (want[1] != 0).any(1).all()
    assert_scene(e, (3, 3) + got[2:], want, "padding", pad=pad)
    e.close()


# ---- 4. a refusal changes nothing -------------------------------------------------------------------------------------------------
def test_a_refusal_leaves_scene_motion_records_and_table():
    from optimalmodulationds_amd import _lib as L
    spec, prev, now = cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7)
    other = cases.random_pair(11, (12, 10, 9), 900, 900)[2]
    track, obj = track_of(3, 0.1), obj_of(1, 6)
    e = base._engine("franka")
    e.set_obstacles_from_cloud_objects(prev[:300], spec, track, obj)
    before = objflow(prev[:300], prev, spec, track, obj)
    assert_scene(e, e.set_obstacles_from_cloud_objects(prev, spec, track, obj), before)
    assert (before[1] != 0).any()
    scene, motion, objects = e.get_obstacles(), e.get_obstacle_motion(), e.cloud_objects()
    small = spec_of(tuple(spec.origin), spec.voxel, tuple(spec.dims), max_spheres=50)          # the same grid, too few spheres allowed
    for refuse in (lambda: e.set_obstacles_from_cloud_objects(other, small, track, obj),
                   lambda: e.set_obstacles_from_cloud_objects(other, small, track, obj, q=base._q0()),
                   lambda: e.set_obstacles_from_cloud_objects(other, spec, track, obj_of(0, 6)),
                   lambda: e.set_obstacles_from_cloud_objects(other, spec, track, obj_of(3, 6)),
                   lambda: e.set_obstacles_from_cloud_objects(other, spec, track_of(0, 0.1), obj),
                   lambda: e.set_obstacles_from_cloud_objects(other, spec_of((0, 0, 0), 0.0, (4, 4, 4)), track, obj)):
        with pytest.raises(L.OmdsError, match=f"omds error {ERR_INVALID_ARG}"):
            refuse()
        assert np.array_equal(bits(e.get_obstacles()), bits(scene)) and e.get_obstacle_horizon()[1] == 1
        assert np.array_equal(bits(e.get_obstacle_motion()[0]), bits(motion[0]))
        now_objects = e.cloud_objects()
        assert np.array_equal(now_objects[0], objects[0]) and np.array_equal(now_objects[1], objects[1]) and now_objects[2] == objects[2]
    want = objflow(prev, now, spec, track, obj)                                                 # ... against the state from before the refusals
    assert want[6] >= 1
    assert_scene(e, e.set_obstacles_from_cloud_objects(now, spec, track, obj), want, "after the refusals")
    e.close()


# ---- 5. the propagate that follows ------------------------------------------------------------------------------------------------
def test_static_scene_keeps_the_static_propagate():
    spec, prev, _ = base._shelf_clouds()
    a, b = base._planner(), base._planner()
    track, obj = track_of(2, 0.1), obj_of(1, 4)
    a.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    n, occ, matched, n_obj, n_acc = a.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    assert n == occ == matched > 200 and n_obj == n_acc >= 1 and a.get_obstacle_horizon()[1] == 0 and not a.get_obstacle_motion()[1]
    assert a.cloud_objects()[1].sum() > 200
    assert b.set_obstacles_from_cloud(prev, spec) == (n, occ)
    a.prof_enable(1)
    b.prof_enable(1)
    a.propagate(base._q0())
    b.propagate(base._q0())
    base._same_rollouts(a, b, "static")
    assert a.prof_read_ex()[1] == b.prof_read_ex()[1], "another number of launches"
    a.close()
    b.close()


def test_propagate_equals_set_obstacles_plus_motion_in_the_moving_frame():
    spec, prev, now = base._shelf_clouds()
    track, obj = track_of(3, 0.1), obj_of(1, 4)
    spheres, vel, label, flag, matched, n_obj, n_acc = objflow(prev, now, spec, track, obj)
    assert 250 <= len(spheres) <= 300 and n_acc >= 10 and flag.sum() > 50 and (flag == 0).any() and (vel != 0).any(1).all()
    a, b = base._planner(), base._planner()
    for e in (a, b):
        e.set_obstacle_frame(True)
    a.set_obstacles_from_cloud_objects(prev, spec, track, obj)
    assert a.set_obstacles_from_cloud_objects(now, spec, track, obj) == (len(spheres), len(spheres), matched, n_obj, n_acc)
    b.set_obstacles(spheres)
    b.set_obstacle_motion(vel)
    assert a.get_obstacle_frame() == b.get_obstacle_frame() and a.get_obstacle_frame()[2] is True
    for q in (base._q0(), (base._q0() + F32(0.05)).astype(F32)):
        a.propagate(q)
        b.propagate(q)
        base._same_rollouts(a, b, "moving frame")
    a.close()
    b.close()


# ---- the facade -------------------------------------------------------------------------------------------------------------------
def test_facade_takes_the_objects_route():
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    spec, prev, now = base._shelf_clouds()
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(base.weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    mppi = MPPI(torch.tensor(base._q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 4, 32, [LinDS(q_f)], dh[:, 2], nn_model, K)
    mppi.dst_thr = 0.01
    lo, hi = (-0.8, -0.8, -0.1), (0.8, 0.8, 1.3)
    spheres, vel, label, flag, matched, n_obj, n_acc = objflow(prev, now, spec, track_of(3, 0.1), obj_of(1, 4))
    with pytest.raises(ValueError, match="dt_frame"):
        mppi.update_obstacles_from_cloud(prev, 0.05, lo, hi, objects=True)
    mppi.update_obstacles_from_cloud(prev, 0.05, lo, hi, dt_frame=0.1, reach=3, objects=True)
    assert mppi.obs_velocities is None and mppi.cloud_matched == -1 and mppi.cloud_objects_matched == -1 and mppi.cloud_objects >= 1
    assert mppi.update_obstacles_from_cloud(now, 0.05, lo, hi, dt_frame=0.1, reach=3, objects=True, moving_frame=True) == (len(spheres), len(spheres))
    assert (mppi.cloud_matched, mppi.cloud_objects, mppi.cloud_objects_matched) == (matched, n_obj, n_acc)
    assert np.array_equal(bits(mppi.obs_velocities.numpy()), bits(vel)) and np.array_equal(bits(mppi.obs.numpy()), bits(spheres))
    assert np.array_equal(mppi._engine.cloud_objects()[1], flag)
    assert np.isfinite(mppi.propagate()[0].numpy()).all()
    mppi.update_obstacles_from_cloud(now, 0.05, lo, hi, dt_frame=0.1, reach=3)                     # the default keeps the tracked route
    assert mppi.cloud_objects is None and mppi.cloud_objects_matched is None and mppi.cloud_matched >= 0
