"""The velocity filter on the device (include/omds.h: THE VELOCITY FILTER) against the host definition and an unfiltered twin.  After
every call of a context with a filter:
  - the installed velocities are bit for bit omds_velocity_filter_step on the state stored before (velocity_filter_state of the
    previous call) and on this call's list (velocity_filter_frame, the cells of the scene, labels and flags of get_cloud_objects);
  - the stored state grid is that step's state_out;
  - a twin without the filter, fed the same frames, has the same scene, labels, counts and stored memory, and its velocities are the
    filtered context's raw ones.
The frames: a plate at 1 m crossing one voxel per frame in front of a wall at 2 m, two cameras of 64 x 48, a grid of 1 287 cells."""
import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import scene_memory_cases as sm
import scene_memory_flow_cases as mf
import test_gpu_cloud_flow as base
from cloud_cases import F32, cells_of, spec_of
from cloud_flow_cases import track_of
from depth_cases import U16

pytestmark = pytest.mark.gpu

bits = base.bits
ROUTES = ("tracked", "objects", "depth", "memory")
FILT = dict(alpha=0.4, alpha_object=0.25, max_jump=1.0)
TRACK = (2, 0.1, 0.05)


def scene(n_frames=6, stop_at=None):
    """(cams, frames [t][camera], clouds [t]): the crossing plate seen by two cameras one cell apart in height; from frame ``stop_at``
    on the plate stands where it was"""
    from optimalmodulationds_amd.engine import depth_points
    cams = [sm.exact_cam(U16, 64, 48, t=(0.25, -0.5, 0.75 - 0.125 * i)) for i in range(2)]
    at = [t if stop_at is None else min(t, stop_at) for t in range(n_frames)]
    per_cam = [mf.crossing(c, n=max(at) + 1) for c in cams]
    frames = [[per_cam[i][t] for i in range(2)] for t in at]
    clouds = [np.concatenate([depth_points(img, c)[0] for img, c in zip(images, cams)]) for images in frames]
    return cams, frames, clouds


def call(e, route, spec, track, cams, images, cloud, mem=None):
    """one scene call of ``route`` -> (n_spheres, n_matched, everything the call returned)"""
    if route == "tracked":
        out = e.set_obstacles_from_cloud_tracked(cloud, spec, track)
    elif route == "objects":
        out = e.set_obstacles_from_cloud_objects(cloud, spec, track, mf.obj_of())
    elif route == "depth":
        out = e.set_obstacles_from_depth(images, cams, spec, None, track, mf.obj_of())
    else:
        out = e.set_obstacles_from_depth_memory_tracked(images, cams, spec, mem, track, mf.obj_of())
    return out[0], out[2], out


def labelled(route):
    return route != "tracked"


def step(e, u, route, spec, track, filt, cams, images, cloud, state_prev, mem=None, what=""):
    """one call on the filtered context ``e`` and its twin ``u``, checked against the definition on ``state_prev`` (the state grid
    stored before, None: empty) -> dict(state, vel, n, live, cells, want_vel, stats, matched)"""
    from optimalmodulationds_amd.engine import velocity_filter_step
    n, n_matched, out = call(e, route, spec, track, cams, images, cloud, mem)
    n_u, matched_u, out_u = call(u, route, spec, track, cams, images, cloud, mem)
    assert out == out_u, f"{what}: the counts are not the unfiltered call's"
    sc = e.get_obstacles()
    assert np.array_equal(bits(sc), bits(u.get_obstacles())), f"{what}: the scene is not the unfiltered call's"
    group = None
    if labelled(route):
        label, flag, n_obj = e.cloud_objects()
        label_u, flag_u, n_obj_u = u.cloud_objects()
        assert np.array_equal(label, label_u) and np.array_equal(flag, flag_u) and n_obj == n_obj_u, f"{what}: labels"
        group = np.where(flag[:n] == 1, label[:n], -1).astype(np.int32)
    if route == "memory":
        (age, words), (age_u, words_u) = e.get_scene_memory(grid=True), u.get_scene_memory(grid=True)
        assert np.array_equal(age, age_u) and np.array_equal(words, words_u), f"{what}: the stored memory"
    raw, live, stats = e.velocity_filter_frame()
    vel_u, have_u = u.get_obstacle_motion()
    assert np.array_equal(bits(raw), bits(vel_u)), f"{what}: the raw velocities are not the unfiltered context's"
    assert not raw[n:].any() and not live[n:].any() and int(live.sum()) == max(n_matched, 0), what
    vel, have = e.get_obstacle_motion()
    state = e.velocity_filter_state()
    cells = cells_of(spec, sc[:n]).astype(np.int32)
    if n_matched == -1:
        assert state is None and not have and not vel.any() and stats == (0, 0, 0), f"{what}: no previous frame, an empty history"
        return dict(state=None, vel=vel, n=n, live=live[:n], cells=cells, want_vel=vel[:n], stats=stats, matched=-1, have=have)
    want_vel, want_state, want_stats = velocity_filter_step(spec, track, filt, state_prev, cells, raw[:n], live[:n], group)
    assert np.array_equal(bits(vel[:n]), bits(want_vel)) and not vel[n:].any(), f"{what}: the installed velocities are not the definition's"
    assert have == bool(want_vel.any()), f"{what}: a motion horizon exactly when some output velocity is not 0"
    assert state is not None and np.array_equal(state, want_state), f"{what}: the stored state is not the definition's state_out"
    assert stats == want_stats, (what, stats, want_stats)
    return dict(state=state, vel=vel, n=n, live=live[:n], cells=cells, want_vel=want_vel, stats=stats, matched=n_matched, have=have, group=group)


def twins(kind=None, filt=FILT, planner=False):
    e, u = (base._planner(), base._planner()) if planner else (base._engine(kind), base._engine(kind))
    e.set_velocity_filter(filt)
    return e, u


def run(routes, frames_of, spec, filt=FILT, track=TRACK, mem=None):
    """the frames through a filtered context and its twin, frame t on routes[t % len(routes)] -> what every call left"""
    cams, frames, clouds = frames_of
    e, u = twins(filt=filt)
    tr, f = track_of(*track), dict(filt)
    state, seen = None, []
    for t, (images, cloud) in enumerate(zip(frames, clouds)):
        r = step(e, u, routes[t % len(routes)], spec, tr, f, cams, images, cloud, state, mem, what=f"{routes[t % len(routes)]} frame {t}")
        state = r["state"]
        seen.append(r)
    e.close()
    u.close()
    return seen


# ---- 1. the four routes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_route_installs_the_definition_on_the_stored_state(route):
    mem = sm.mem_of(0, mf.CROSS_MARGIN, 0) if route == "memory" else None
    seen = run([route], scene(6), sm.grid(max_spheres=8192), mem=mem)
    assert seen[0]["matched"] == -1 and all(r["matched"] > 50 for r in seen[1:])
    assert seen[1]["stats"] == (0, 0, 0) and seen[1]["state"][:, 3].max() == 1, "the first velocities start the history"
    last = seen[-1]
    assert last["stats"][0] > 50 and last["state"][:, 3].max() == 5, "five frames of history behind the wall"
    assert route != "tracked" or sum(r["stats"][1] for r in seen[2:]) > 0, "a wall sphere uncovered beside the plate jumps: a restart"
    assert all(r["have"] for r in seen[1:-1]), "a motion horizon while the plate is whole in view (in the last frame it is half out)"
    if labelled(route):
        assert sum(r["stats"][2] for r in seen[2:]) > 0 and any((r["group"] >= 0).sum() >= 4 for r in seen[2:]), "the plate is an accepted object"
        for r in seen[2:]:
            g = r["group"]
            for lab in np.unique(g[g >= 0]):
                assert len(np.unique(bits(r["vel"][:r["n"]][g == lab]), axis=0)) == 1, "an object stays rigid"


# ---- 2. alpha = 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["tracked", "depth"])
def test_alpha_one_installs_the_unfiltered_velocities(route):
    cams, frames, clouds = scene(4)
    spec, tr = sm.grid(max_spheres=8192), track_of(*TRACK)
    e, u = twins(filt=dict(alpha=1.0))
    moved = 0
    for images, cloud in zip(frames, clouds):
        assert call(e, route, spec, tr, cams, images, cloud)[2] == call(u, route, spec, tr, cams, images, cloud)[2]
        (vel, have), (vel_u, have_u) = e.get_obstacle_motion(), u.get_obstacle_motion()
        assert have == have_u and np.array_equal(bits(vel), bits(vel_u))
        moved += int(vel.any())
    assert moved == 3 and e.velocity_filter_state()[:, 3].max() == 3
    e.close()
    u.close()


# ---- 3. a scene that comes to rest ---------------------------------------------------------------------------------------------------------
def test_static_scene_returns_to_the_static_propagate():
    """the plate stops after frame 2: the raw velocities are 0 from frame 3 on, the filtered ones decay until the still rule zeroes the
    last of them -- in the frame the definition, iterated on the host, says; from there on the propagate is the twin's"""
    from optimalmodulationds_amd.engine import velocity_filter_step
    cams, frames, clouds = scene(8, stop_at=2)
    spec, tr, filt = sm.grid(max_spheres=8192), track_of(2, 0.1, 0.3), dict(alpha=0.5)
    e, u = twins(filt=filt, planner=True)
    host, at_rest, modes = None, None, []
    for t, cloud in enumerate(clouds):
        n, n_matched, _ = call(e, "tracked", spec, tr, cams, None, cloud)
        call(u, "tracked", spec, tr, cams, None, cloud)
        modes.append(e.get_obstacle_horizon()[1])
        if n_matched == -1:
            continue
        raw, live, _ = e.velocity_filter_frame()
        want, host, _ = velocity_filter_step(spec, tr, filt, host, cells_of(spec, e.get_obstacles()[:n]).astype(np.int32), raw[:n], live[:n])
        assert np.array_equal(host, e.velocity_filter_state()) and modes[-1] == int(want.any()), t
        if t >= 3:
            assert not raw.any() and u.get_obstacle_horizon()[1] == 0, "the twin is static as soon as the plate stops"
            if at_rest is None and not want.any():
                at_rest = t
    assert at_rest is not None and at_rest > 3 and modes[1:at_rest] == [1] * (at_rest - 1) and modes[at_rest:] == [0] * (len(modes) - at_rest), modes
    assert (host[:, 3] > 0).any() and (host[:, :3] != 0).any(), "the stored velocities are still decaying: only the output is at rest"
    for x in (e, u):
        x.prof_enable(1)
        x.propagate(base._q0())
    base._same_rollouts(e, u, "at rest")
    assert e.prof_read_ex()[1] == u.prof_read_ex()[1], "another number of launches"
    e.close()
    u.close()


# ---- 4. remembered and uncovered spheres -----------------------------------------------------------------------------------------------------
def test_remembered_and_uncovered_spheres_stand_still_without_history():
    cams, frames, clouds = scene(5)
    spec, tr, mem = sm.grid(max_spheres=8192), track_of(*TRACK), sm.mem_of(0, mf.CROSS_MARGIN, 0)
    e, u = twins()
    state, remembered, uncovered = None, 0, 0
    for t, (images, cloud) in enumerate(zip(frames, clouds)):
        words_before = e.get_scene_memory(grid=True)[1] if t else np.zeros(sm.n_cells_of(spec), np.uint32)
        r = step(e, u, "memory", spec, tr, dict(FILT), cams, images, cloud, state, mem, what=f"frame {t}")
        state = r["state"]
        if state is None:
            continue
        age = e.get_scene_memory()[:r["n"]]
        old = age >= 1
        back = (age == 0) & (words_before[r["cells"]] >= 2)
        for which in (old, back):
            assert not r["live"][which].any() and not r["vel"][:r["n"]][which].any() and not state[r["cells"][which], 3].any()
        remembered, uncovered = remembered + int(old.sum()), uncovered + int(back.sum())
    assert remembered > 5 and uncovered > 0, (remembered, uncovered)
    e.close()
    u.close()


# ---- 5. refused and keyed calls ---------------------------------------------------------------------------------------------------------------
def test_a_refusal_leaves_the_state_and_a_new_key_or_a_reset_empties_it():
    from optimalmodulationds_amd import _lib as L
    cams, frames, clouds = scene(6)
    spec, tr = sm.grid(max_spheres=8192), track_of(*TRACK)
    e, u = twins()
    state = None
    for t in range(3):
        state = step(e, u, "tracked", spec, tr, dict(FILT), cams, frames[t], clouds[t], state, what=f"frame {t}")["state"]
    small = sm.grid(max_spheres=20)
    for x in (e, u):
        with pytest.raises(L.OmdsError, match="omds error 1"):
            x.set_obstacles_from_cloud_tracked(clouds[3], small, tr)
    with pytest.raises(L.OmdsError, match="alpha"):
        e.set_velocity_filter(dict(alpha=0.0))
    assert np.array_equal(e.velocity_filter_state(), state) and e.velocity_filter.alpha == F32(FILT["alpha"]), "a refusal leaves state and filter"
    state = step(e, u, "tracked", spec, tr, dict(FILT), cams, frames[3], clouds[3], state, what="behind the refusals")["state"]
    assert state[:, 3].max() == 3
    # another filter spec: the frame is still there, the history is not
    other = dict(FILT, alpha=0.5)
    e.set_velocity_filter(other)
    r = step(e, u, "tracked", spec, tr, other, cams, frames[4], clouds[4], None, what="another filter spec")
    assert r["matched"] > 50 and r["stats"] == (0, 0, 0) and r["state"][:, 3].max() == 1
    # the reset
    for x in (e, u):
        x.cloud_track_reset()
    assert e.velocity_filter_state() is None
    assert step(e, u, "tracked", spec, tr, other, cams, frames[5], clouds[5], None, what="behind the reset")["matched"] == -1
    state = step(e, u, "tracked", spec, tr, other, cams, frames[4], clouds[4], None, what="a first velocity again")["state"]
    assert state[:, 3].max() == 1
    # another grid (min_points is part of the key): no previous frame on it, and an empty history after it
    dense = sm.grid(max_spheres=8192, min_points=2)
    assert step(e, u, "tracked", dense, tr, other, cams, frames[5], clouds[5], state, what="another grid")["matched"] == -1
    r = step(e, u, "tracked", dense, tr, other, cams, frames[4], clouds[4], None, what="the second frame on it")
    assert r["matched"] > 50 and r["stats"] == (0, 0, 0)
    # clearing the filter empties the history and ends the frame report
    e.set_velocity_filter(None)
    assert e.velocity_filter_state() is None and e.velocity_filter is None
    e.set_obstacles_from_cloud_tracked(clouds[5], dense, tr)
    with pytest.raises(L.OmdsError, match="omds error"):
        e.velocity_filter_frame()
    e.close()
    u.close()


# ---- 6. the routes share the state ------------------------------------------------------------------------------------------------------------
def test_alternating_routes_share_the_state():
    seen = run(["objects", "depth", "tracked", "depth"], scene(6), sm.grid(max_spheres=8192))
    assert seen[0]["matched"] == -1 and all(r["matched"] > 50 for r in seen[1:]) and seen[-1]["state"][:, 3].max() == 5
    assert sum(r["stats"][2] for r in seen[2:]) > 0, "a depth frame blends the plate against the history a cloud frame left"


def test_facade_sets_the_filter_and_reports_its_counts():
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    from helpers import weights_path
    cams, frames, clouds = scene(4)
    g = sm.GRID_SMALL
    lo = np.array(g["origin"], F32)
    hi = lo + F32(g["voxel"]) * np.array(g["dims"], F32)
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    mppi = MPPI(torch.tensor(base._q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 4, 32, [LinDS(q_f)], dh[:, 2], nn_model, base.K)
    with pytest.raises(ValueError, match="dt_frame"):
        mppi.update_obstacles_from_cloud(clouds[0], g["voxel"], lo, hi, smooth=dict(alpha=0.3))
    raw = []
    for t in range(3):
        mppi.update_obstacles_from_cloud(clouds[t], g["voxel"], lo, hi, max_spheres=8192, dt_frame=0.1, smooth=dict(alpha=0.3))
        raw.append(mppi._engine.velocity_filter_frame()[0])
    assert mppi.vel_filter_stats[0] > 50 and mppi._engine.velocity_filter.alpha == F32(0.3)
    assert not np.array_equal(bits(mppi.obs_velocities.numpy()), bits(raw[-1])), "the installed velocities are the smoothed ones"
    mppi.update_obstacles_from_depth(frames[3], cams, g["voxel"], lo, hi, max_spheres=8192, dt_frame=0.1)      # smooth=None: the filter stays
    assert mppi.vel_filter_stats[0] > 50 and mppi._engine.velocity_filter_state()[:, 3].max() == 3
    mppi.update_obstacles_from_depth(frames[3], cams, g["voxel"], lo, hi, max_spheres=8192, dt_frame=0.1, smooth=False)
    assert mppi.vel_filter_stats is None and mppi._engine.velocity_filter is None and mppi._engine.velocity_filter_state() is None
