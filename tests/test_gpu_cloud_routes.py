"""ONE context through all four routes of the scene from a point cloud, in every cyclic order, on two grids (include/omds.h:
omds_set_obstacles_from_cloud, _tracked, _objects, omds_set_obstacles_from_depth; csrc/scene_cloud.hip).  The buffers of a route are
reserved at that route's first call and grown with the spec (scene_cloud.hip: reserve_base / reserve_tracked / reserve_objects), and
the stored frame and the stored component table pass from one route to the next: the other device tests mostly start a fresh context
per route, so a buffer one route forgets to reserve, or reserves too small after another route's call, shows here and not there.

Eight calls cycle through plain, tracked, objects and depth-with-objects; the first four on an 8 x 8 x 8 grid with max_spheres = 64
and about 300 points, the last four on a 12 x 10 x 9 grid with max_spheres = 512 and about 650 points (the context's obstacle capacity
of 64 grows there, too).  Every frame is a 67 x 49 depth image of one sphere of radius 8 cm a metre in front of the camera that moves
12 mm per frame: the depth call takes the image, the cloud calls every 4th (2nd) of its points.  After every call the scene, the
velocities and the labels in force are compared bit for bit with the host definitions (point_cloud_spheres, point_cloud_flow,
point_cloud_object_flow; for depth on the points of depth_points).

What "previous frame" and "previous table" are for a call follows from omds.h and is computed here (plan): a frame is stored by every
tracked, objects or depth call and holds for calls on the same grid; a table is stored by an objects or depth call and dropped by a
plain tracked call.  With depth first no objects call ever has a table (depth A, tracked A, objects A | depth B, tracked B,
objects B: each objects call follows a tracked one, each depth call opens a grid); in the other three orders the depth call follows
the objects call of its grid.

The memory routes (omds_set_obstacles_from_depth_memory, _memory_tracked; reserve_memory / reserve_memory_flow) join in the second
half of this file: twelve calls through six routes, see plan_six."""
import functools

import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it  # noqa: F401

import depth_cases as dc
import scene_memory_cases as sm
import scene_memory_flow_cases as mf
import test_gpu_cloud_flow as base
import test_gpu_cloud_objects as objs
import test_gpu_depth as depth
import test_gpu_scene_memory as gm
import test_gpu_scene_memory_flow as gmf
from cloud_cases import F32, spec_of
from cloud_flow_cases import track_of
from cloud_object_cases import obj_of

pytestmark = pytest.mark.gpu

bits = base.bits
ROUTES = ("plain", "tracked", "objects", "depth")
NONE = np.zeros((0, 3), F32)
ERR_INVALID_ARG = 1


def halves():
    """(spec, every n-th point of a frame goes to a cloud call) of the first and the last four calls"""
    return [(spec_of((-0.2, -0.2, 0.8), 0.05, (8, 8, 8), max_spheres=64), 4),
            (spec_of((-0.18, -0.15, 0.8), 0.03, (12, 10, 9), max_spheres=512), 2)]


def frame(f):
    """(image, camera, its points with NaN rows, the valid ones) of frame f"""
    cam = dc.cam_of(67, 49, 250.0, 250.0, 33.0, 24.0, dc.pose_of(np.eye(3), (0.0, 0.0, 0.0)), dc.U16, 0.001, 0.3, 4.0)
    image = dc.to_u16(dc.render(cam, spheres=[(-0.04 + 0.012 * f, 0.0, 1.0, 0.08)]))
    full = depth.points_of([image], [cam])[0]
    return image, cam, full, full[~np.isnan(full).any(1)]


def plan(first):
    """the eight calls as (route, spec, image, cam, points, want, prev, have_table) -- prev: the points of the stored frame this call
    is matched against, or None; want: the spheres (plain), point_cloud_flow's triple with matched = -1 without a previous frame
    (tracked), test_gpu_cloud_objects' 7-tuple (objects, depth).  The conditions on the inputs are asserted here, on the host
    definitions alone"""
    from optimalmodulationds_amd.engine import point_cloud_spheres
    track, obj = track_of(2, 0.1), obj_of(1, 4)
    order = ROUTES[ROUTES.index(first):] + ROUTES[:ROUTES.index(first)]
    stored = None      # (half, points, a table was stored with it) of the last tracked, objects or depth call
    calls = []
    for i in range(8):
        half, route = i // 4, order[i % 4]
        spec, every = halves()[half]
        image, cam, full, valid = frame(i)
        pts = full if route == "depth" else valid[::every]
        have_prev = stored is not None and stored[0] == half
        have_table = have_prev and stored[2]
        prev = stored[1] if have_prev else NONE
        if route == "plain":
            want, have_prev, have_table = point_cloud_spheres(pts, spec, cap=65536), False, False
            n = len(want)
        elif route == "tracked":
            spheres, vel, matched = base.flow(prev, pts, spec, track)
            want, have_table, n = (spheres, vel, matched if have_prev else -1), False, len(spheres)
            stored = (half, pts, False)
        else:
            want = objs.objflow(prev, pts, spec, track, obj) if have_table else objs.fallback_of(prev, pts, spec, track, obj, have_frame=have_prev)
            n = len(want[0])
            stored = (half, pts, True)
        assert n >= 1 and (half == 1 or n <= 64), (i, route, n)
        assert route == "depth" or abs(len(pts) - (300, 650)[half]) < 60, (i, route, len(pts))
        calls.append((route, spec, image, cam, pts, want, prev if have_prev else None, have_table))
    for half in (0, 1):
        assert any(r != "plain" and p is not None and w[2 if r == "tracked" else 4] > 0 and (w[1] != 0).any()
                   for r, _, _, _, _, w, p, _ in calls[4 * half:4 * half + 4]), f"half {half}: no call with a previous frame, a match and a velocity"
    with_table = [w for r, _, _, _, _, w, _, ht in calls if ht]
    assert bool(with_table) == (first != "depth"), "see the module's text"
    assert first == "depth" or any(w[6] >= 1 and (w[3] == 1).any() for w in with_table), "no accepted object"
    return calls, track, obj


def assert_scene(e, spheres, vel, what):
    n = len(spheres)
    scene, (motion, have) = e.get_obstacles(), e.get_obstacle_motion()
    assert e.n_obs == max(n, e.k) and scene.shape == (e.n_obs, 4) and motion.shape == (e.n_obs, 3), what
    assert np.array_equal(bits(scene[:n]), bits(spheres)) and (scene[n:] == F32(base.PAD)).all(), what
    assert np.array_equal(bits(motion), bits(base.padded(vel, e.n_obs))), f"{what}: the device velocities are not the definition's"
    assert have == bool((vel != 0).any()), what
    if not have:      # (the tables of a motion horizon need the network)
        assert e.get_obstacle_horizon()[1] == 0, what


@pytest.mark.parametrize("first", ROUTES)
def test_one_context_through_every_route(first):
    from optimalmodulationds_amd import _lib as L
    calls, track, obj = plan(first)
    e = base._engine(None)
    for i, (route, spec, image, cam, pts, want, prev, _) in enumerate(calls):
        what = f"call {i} ({route})"
        if route == "plain":
            got = e.set_obstacles_from_cloud(pts, spec)
            assert got == (len(want), len(want)), (what, got)
            assert_scene(e, want, np.zeros((len(want), 3), F32), what)
        elif route == "tracked":
            got = e.set_obstacles_from_cloud_tracked(pts, spec, track)
            if prev is not None:
                base.assert_scene_is_the_definition(e, got, spec, track, prev, pts, what)
            assert got == (len(want[0]), len(want[0]), want[2]), (what, got)
            assert_scene(e, want[0], want[1], what)
        else:
            if route == "objects":
                got = e.set_obstacles_from_cloud_objects(pts, spec, track, obj)
            else:
                got = e.set_obstacles_from_depth(image, cam, spec, None, track, obj)
            assert got[1] == len(want[0]), (what, got)
            objs.assert_scene(e, got, want, what)
        if route in ("plain", "tracked"):      # the labels belong to the objects call that installed the scene
            with pytest.raises(L.OmdsError):
                e.cloud_objects()
    e.close()


def test_a_refusal_for_too_many_cells_leaves_the_stored_frame():
    """tracked frame 4; frame 5 refused under max_spheres = 8 on the same grid (its records were counted into the buffer that is not
    the stored frame); then frame 5 tracked again: matched against frame 4, the scene and the velocities of the definition"""
    from optimalmodulationds_amd import _lib as L
    spec, every = halves()[1]
    small = spec_of(tuple(spec.origin), spec.voxel, tuple(spec.dims), max_spheres=8)
    track = track_of(2, 0.1)
    prev, now = frame(4)[3][::every], frame(5)[3][::every]
    spheres, vel, matched = base.flow(prev, now, spec, track)
    assert len(spheres) > 8 and matched > 0 and (vel != 0).any()
    e = base._engine(None)
    assert e.set_obstacles_from_cloud_tracked(prev, spec, track)[2] == -1
    scene = e.get_obstacles()
    with pytest.raises(L.OmdsError, match=f"omds error {ERR_INVALID_ARG}") as err:
        e.set_obstacles_from_cloud_tracked(now, small, track)
    assert err.value.n_occupied == len(spheres) and np.array_equal(bits(e.get_obstacles()), bits(scene))
    got = e.set_obstacles_from_cloud_tracked(now, spec, track)
    base.assert_scene_is_the_definition(e, got, spec, track, prev, now, "after the refusal")
    e.close()


# ---- the memory routes join in: six routes, twelve calls -------------------------------------------------------------------------------
ROUTES6 = ROUTES + ("memory", "memory_tracked")
MAX_AGE = 1      # a grid sees two memory calls, so nothing expires; what half 0 holds then is bounded in plan_six, on the definition


@functools.lru_cache(maxsize=None)
def frames12():
    return [frame(i) for i in range(12)]


def flow_want(image, cam, spec, mem, track, obj, prev, have_table, m_in):
    """(what the definition gives for a memory-tracked call with an object spec, whether all of it holds): without a stored frame, or
    with a frame and a table, everything of depth_scene_memory_flow; with a frame and no table (a plain tracked call stored it) the
    definition has no such state, and the velocities and n_matched are those it gives without objects, n_objects_matched is -1"""
    from optimalmodulationds_amd.engine import depth_scene_memory_flow
    whole = prev is None or have_table
    before = None if prev is None else ([prev[0]], [prev[1]])
    return depth_scene_memory_flow([image], [cam], spec, mem, track, obj if whole else None, before, m_in, cap=65536), whole


def plan_six(first):
    """the twelve calls as dicts: six on the 8 x 8 x 8 grid with max_spheres = 64, six on the 12 x 10 x 9 grid with 512, cycling through
    ROUTES6 from ``first``; every route takes ALL valid points of its frame (the cloud calls depth_points of the image, no subsample),
    so the stored frame is the same set of points whichever route stored it, and the definition of the memory-tracked route can be
    given the previous IMAGE.  No self-filter.  prev: the frame() of the stored record frame, or None; have_table: a table is stored
    with it (objects, depth and memory-tracked store one, a plain tracked call drops it); the words of a grid pass between the two
    memory routes, and a plain memory call leaves frame and table alone.  The conditions on the inputs are asserted here, on the host
    definitions alone.

    Two of them need a reading.  "A memory call with a remembered cell" is a call of either memory route: in five of the six orders
    the plain memory call comes before the memory-tracked one on both grids and starts from empty memory.  "A memory-tracked call
    with a match and a velocity" cannot exist when ``first`` is memory or memory_tracked: the memory-tracked call is then the first
    on each grid to store a frame.  That is asserted as such; in those two orders the tracked call behind it matches ITS frame."""
    from optimalmodulationds_amd.engine import depth_scene_memory, point_cloud_spheres
    track, obj, mem = track_of(2, 0.1), obj_of(1, 4), sm.mem_of(MAX_AGE)
    order = ROUTES6[ROUTES6.index(first):] + ROUTES6[:ROUTES6.index(first)]
    stored, words = None, None      # (half, frame index, with a table) of the last call that stored a frame; (half, words) of the last memory call
    calls = []
    for i in range(12):
        half, route = i // 6, order[i % 6]
        spec = halves()[half][0]
        image, cam, full, valid = frames12()[i]
        have_prev = stored is not None and stored[0] == half
        have_table = have_prev and stored[2]
        prev = frames12()[stored[1]] if have_prev else None
        prev_pts = prev[3] if have_prev else NONE
        m_in = words[1] if words is not None and words[0] == half else None
        call = dict(route=route, spec=spec, image=image, cam=cam, pts=valid, prev=prev, have_table=have_table, remembered=0, flowed=False)
        if route == "plain":
            call["want"] = point_cloud_spheres(valid, spec, cap=65536)
            n = len(call["want"])
        elif route == "tracked":
            spheres, vel, matched = base.flow(prev_pts, valid, spec, track)
            call["want"], n = (spheres, vel, matched if have_prev else -1), len(spheres)
            stored = (half, i, False)
        elif route in ("objects", "depth"):
            call["want"] = (objs.objflow(prev_pts, valid, spec, track, obj) if have_table else
                            objs.fallback_of(prev_pts, valid, spec, track, obj, have_frame=have_prev))
            n = len(call["want"][0])
            stored = (half, i, True)
        else:
            if route == "memory":
                w, counts = depth_scene_memory([image], [cam], spec, mem, m_in)
            else:
                want, _ = flow_want(image, cam, spec, mem, track, obj, prev, have_table, m_in)
                w, counts = want["words"], want["counts"]
                call["flowed"] = want["n_matched"] > 0 and bool((want["vel"] != 0).any())
                stored = (half, i, True)
            words, n = (half, w), counts[0] + counts[1]
            call["remembered"] = counts[1]
        assert n >= 1 and (half == 1 or n <= 64), (i, route, n)
        calls.append(call)
    assert any(c["remembered"] > 0 for c in calls), "no call of a memory route with a remembered cell"
    assert any(c["flowed"] for c in calls) == (first not in ("memory", "memory_tracked")), "see plan_six's text"
    return calls, track, obj, mem


@pytest.mark.parametrize("first", ROUTES6)
def test_one_context_through_the_memory_routes_too(first):
    """the first four routes are checked as in test_one_context_through_every_route; the memory route against depth_scene_memory and
    the memory-tracked one against depth_scene_memory_flow (flow_want), both on the words read back from the context after the last
    call of a memory route on this grid"""
    from optimalmodulationds_amd import _lib as L
    calls, track, obj, mem = plan_six(first)      # every condition on the inputs, before anything goes to the device
    e = base._engine(None)
    words = None      # (half, the words read back)
    for i, c in enumerate(calls):
        route, spec, image, cam, pts, want, prev = (c.get(k) for k in ("route", "spec", "image", "cam", "pts", "want", "prev"))
        what = f"call {i} ({route})"
        m_in = words[1] if words is not None and words[0] == i // 6 else None
        if route == "plain":
            got = e.set_obstacles_from_cloud(pts, spec)
            assert got == (len(want), len(want)), (what, got)
            assert_scene(e, want, np.zeros((len(want), 3), F32), what)
        elif route == "tracked":
            got = e.set_obstacles_from_cloud_tracked(pts, spec, track)
            if prev is not None:
                base.assert_scene_is_the_definition(e, got, spec, track, prev[3], pts, what)
            assert got == (len(want[0]), len(want[0]), want[2]), (what, got)
            assert_scene(e, want[0], want[1], what)
        elif route in ("objects", "depth"):
            if route == "objects":
                got = e.set_obstacles_from_cloud_objects(pts, spec, track, obj)
            else:
                got = e.set_obstacles_from_depth(image, cam, spec, None, track, obj)
            assert got[1] == len(want[0]), (what, got)
            objs.assert_scene(e, got, want, what)
        elif route == "memory":
            words = (i // 6, gm.step(e, spec, mem, [cam], [image], m_in, what=what)[0])
            assert not e.get_obstacle_motion()[1], f"{what}: a static scene"
        else:
            n, counts, n_matched, n_objects, n_acc = gmf.new_call(e, [image], [cam], spec, mem, track, obj)
            s = gmf.state_of(e, n, obj)
            want, whole = flow_want(image, cam, spec, mem, track, obj, prev, c["have_table"], m_in)
            got = dict(words=s["words"], counts=counts, spheres=s["scene"][:n], vel=s["vel"][:n], age=s["age"][:n], label=s["label"][:n],
                       object=s["flag"][:n], n_matched=n_matched, n_objects=n_objects, n_objects_matched=n_acc)
            if not whole:
                assert n_acc == -1 and not s["flag"].any(), f"{what}: a frame without a table gives no object a velocity"
                got = {k: (v if k in ("words", "counts", "spheres", "vel", "age", "n_matched") else want[k]) for k, v in got.items()}
            mf.same(got, want, what)
            assert (s["age"][n:] == -1).all() and (s["label"][n:] == -1).all() and not s["vel"][n:].any(), what
            assert np.array_equal(bits(s["scene"][n:]), bits(np.tile(gm.PAD, (e.n_obs - n, 1)))), what
            assert s["have"] == bool(s["vel"].any()), what
            words = (i // 6, s["words"])
        if route in ("plain", "tracked", "memory"):      # the labels belong to the objects call that installed the scene
            with pytest.raises(L.OmdsError):
                e.cloud_objects()
    e.close()


def test_a_refused_memory_tracked_call_leaves_the_stored_frame():
    """tracked frame 4; frame 5 through the memory-tracked route refused under max_spheres = 8 on the same grid (it counted into the
    record buffer that is not the stored frame); then frame 5 tracked: matched against frame 4, the scene and the velocities of the
    definition"""
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.engine import depth_scene_memory
    spec, every = halves()[1]
    small = spec_of(tuple(spec.origin), spec.voxel, tuple(spec.dims), max_spheres=8)
    track, obj, mem = track_of(2, 0.1), obj_of(1, 4), sm.mem_of(MAX_AGE)
    image, cam = frame(5)[:2]
    prev, now = frame(4)[3][::every], frame(5)[3][::every]
    spheres, vel, matched = base.flow(prev, now, spec, track)
    counts = depth_scene_memory([image], [cam], small, mem)[1]
    assert counts[0] > 8 and counts[1] == 0 and matched > 0 and (vel != 0).any()
    e = base._engine(None)
    assert e.set_obstacles_from_cloud_tracked(prev, spec, track)[2] == -1
    scene = e.get_obstacles()
    with pytest.raises(L.OmdsError, match=f"omds error {ERR_INVALID_ARG}") as err:
        gmf.new_call(e, [image], [cam], small, mem, track, obj)
    assert err.value.counts == counts + (0,) and err.value.n_occupied == counts[0]
    assert np.array_equal(bits(e.get_obstacles()), bits(scene)) and e.get_scene_memory(grid=True)[1].size == 0
    got = e.set_obstacles_from_cloud_tracked(now, spec, track)
    base.assert_scene_is_the_definition(e, got, spec, track, prev, now, "after the refusal")
    e.close()
