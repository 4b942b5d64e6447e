"""Memory and velocities in one depth call on the device (include/omds.h: omds_set_obstacles_from_depth_memory_tracked) against two
twin engines and the host definition.  After every call:
  - the stored words, the counts, the scene and the ages are bit for bit those of a twin making omds_set_obstacles_from_depth_memory
    calls on the same frames;
  - on the seen spheres, velocities, labels and flags are bit for bit those of a second twin making omds_set_obstacles_from_depth
    (track[, obj]) calls, except where step 4 overrides (the stored word was >= 2): there, and on every remembered sphere, velocity 0;
  - everything is bit for bit omds_depth_scene_memory_flow on the words stored before and the previous frame's images.
Grids of 1 287 and 64 000 cells, images of at most 64 x 48 (96 x 72 where a scene around the arm is rendered)."""
import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import depth_cases as dc
import scene_memory_cases as sm
import scene_memory_flow_cases as mf
import test_gpu_cloud_flow as base
import test_gpu_scene_memory as gm
from cloud_cases import F32, cells_of, spec_of
from cloud_flow_cases import track_of
from depth_cases import FLT, U16

pytestmark = pytest.mark.gpu

bits = base.bits


def new_call(e, images, cams, spec, mem, track, obj, q=None):
    return e.set_obstacles_from_depth_memory_tracked(images, cams, spec, mem, track, obj, q)


def state_of(e, n, obj):
    """what the engine reports of the scene in force: spheres, velocities (zeros without a horizon), ages, words, labels, flags"""
    age, words = e.get_scene_memory(grid=True)
    vel, have = e.get_obstacle_motion()
    label, flag, n_obj = e.cloud_objects() if obj is not None else (np.full(e.n_obs, -1, np.int32), np.zeros(e.n_obs, np.int32), 0)
    return dict(scene=e.get_obstacles(), vel=vel, have=have, age=age, words=words, label=label, flag=flag, n_obj=n_obj, n=n)


def step(e, tm, tt, st, spec, mem, track, obj, cams, images, q=None, src=None, filt=None, what=""):
    """one call of the new route on ``e`` against the memory twin ``tm``, the tracked twin ``tt`` and the host definition; ``st``
    carries the words stored before, the previous images and the previous final cells.  -> what the call covered"""
    from optimalmodulationds_amd.engine import depth_scene_memory, depth_scene_memory_flow
    given = images if src is None else src
    m_in, prev = st.get("m"), st.get("prev")
    n, counts, n_matched, n_objects, n_objects_matched = new_call(e, given, cams, spec, mem, track, obj, q)
    s = state_of(e, n, obj)
    # --- the memory twin
    n1, counts1 = tm.set_obstacles_from_depth_memory(given, cams, spec, mem, q)
    age1, words1 = tm.get_scene_memory(grid=True)
    assert (n, counts) == (n1, counts1) and e.n_obs == tm.n_obs, (what, counts, counts1)
    assert np.array_equal(s["words"], words1) and np.array_equal(s["age"], age1), f"{what}: words / ages are not the memory route's"
    assert np.array_equal(bits(s["scene"]), bits(tm.get_obstacles())), f"{what}: the scene is not the memory route's"
    final = cells_of(spec, s["scene"][:n])
    # --- the tracked twin, on the seen spheres
    out2 = tt.set_obstacles_from_depth(given, cams, spec, q, track, obj)
    n2 = out2[0]
    seen = cells_of(spec, tt.get_obstacles()[:n2])
    at = np.searchsorted(final, seen)
    assert len(seen) == 0 or (at.max() < n and np.array_equal(final[at], seen)), f"{what}: a seen sphere of the tracked twin is missing"
    stored = np.zeros(sm.n_cells_of(spec), np.uint32) if m_in is None else m_in
    moves = stored[seen] < 2
    rest = np.setdiff1d(np.arange(e.n_obs), at[moves])
    vel2 = tt.get_obstacle_motion()[0][:n2]
    assert np.array_equal(bits(s["vel"][at[moves]]), bits(vel2[moves])), f"{what}: velocities on the seen spheres"
    assert not bits(s["vel"][rest]).any(), f"{what}: a remembered, overridden or padding sphere moves"
    assert s["have"] == bool(s["vel"].any()), f"{what}: a motion horizon exactly when some sphere moves"
    assert (n_objects, n_objects_matched) == ((out2[3], out2[4]) if obj is not None else (0, -1)), what
    if obj is not None:
        label2, flag2, n_obj2 = tt.cloud_objects()
        outside = np.setdiff1d(np.arange(e.n_obs), at)
        assert np.array_equal(s["label"][at], label2[:n2]) and (s["label"][outside] == -1).all() and s["n_obj"] == n_obj2 == n_objects, what
        assert np.array_equal(s["flag"][at[moves]], flag2[:n2][moves]) and not s["flag"][rest].any(), what
    # --- the host definition
    keep_now = keep_prev = None
    if q is not None:
        cand = np.nonzero(depth_scene_memory(images, cams, spec, mem, m_in, filter=filt)[0])[0]
        keep_now = np.isin(cand, final)
        assert counts[4] == int((~keep_now).sum())
        if prev is not None:
            keep_prev = np.isin(mf.occupied_cells(spec, mf.points_of(cams, prev, filt)), st["prev_final"])
    want = depth_scene_memory_flow(images, cams, spec, mem, track, obj, None if prev is None else (prev, cams), m_in, keep_prev, keep_now, filt,
                                   cap=65536)
    got = dict(words=s["words"], counts=counts, spheres=s["scene"][:n], vel=s["vel"][:n], age=s["age"][:n], label=s["label"][:n],
               object=s["flag"][:n], n_matched=n_matched, n_objects=n_objects, n_objects_matched=n_objects_matched)
    mf.same(got, want, what)
    assert (s["age"][n:] == -1).all() and (s["label"][n:] == -1).all() and np.array_equal(bits(s["scene"][n:]), bits(np.tile(gm.PAD, (e.n_obs - n, 1))))
    st.update(m=s["words"], prev=images, prev_final=final)
    moving = (s["vel"][:n] != 0).any(1)
    return dict(seen=counts[0], remembered=counts[1], cleared=counts[2], matched=max(n_matched, 0), accepted=int(s["flag"].sum()),
                overridden=int((~moves).sum()), beside=int(moving.any() and (s["age"][:n] >= 1).any()), forgotten=counts[4])


def run(frames, cams, spec, mem, track, obj, filt=None, where="host", q=None, kind=None):
    """the frames ([t][camera]) through three engines; -> the sums of what the calls covered"""
    engines = [base._engine(kind) for _ in range(3)]
    dev = f"cuda:{engines[0].device}"
    for e in engines:
        e.set_depth_filter(filt)
    st, total = {}, {}
    for t, images in enumerate(frames):
        src = None
        if where != "host":
            src = []
            for img in images:
                a = img.view(np.int16) if img.dtype == np.uint16 else img
                if where == "strided":
                    wide = np.zeros((a.shape[0], a.shape[1] + 5), a.dtype)
                    wide[:, 3:-2] = a
                    src.append(torch.from_numpy(wide).to(dev)[:, 3:-2])
                    assert not src[-1].is_contiguous()
                else:
                    src.append(torch.from_numpy(a).to(dev))
        cover = step(*engines, st, spec, mem, track, obj, cams, images, q, src, filt, what=f"frame {t}")
        for k, v in cover.items():
            total[k] = total.get(k, 0) + v
    for e in engines:
        e.close()
    return total


# ---- 1. sequences against the two twins and the definition -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_cams,fmt,size,large,objects,filt,where", [
    ("exact", 1, U16, (32, 24), False, False, None, "host"),
    ("exact", 3, FLT, (64, 48), True, True, None, "device"),
    ("exact", 8, U16, (64, 48), True, False, dict(radius=1, min_support=3), "strided"),
    ("exact", 3, U16, (32, 24), False, True, dict(radius=2, min_support=6), "host"),
    ("general", 1, U16, (64, 48), False, True, None, "strided"),
    ("general", 3, FLT, (64, 48), True, False, None, "host"),
    ("general", 8, U16, (32, 24), True, True, dict(radius=1, min_support=4), "device")])
def test_sequence_is_both_twins_and_the_definition(kind, n_cams, fmt, size, large, objects, filt, where):
    """wall, a plate in front of its left half, plate gone (the uncovered cells: the override), a blind frame, the wall gone"""
    from optimalmodulationds_amd.engine import depth_points
    cams = (gm.exact_cams if kind == "exact" else gm.general_cams)(n_cams, fmt, *size)
    seqs = [sm.sequence(c) for c in cams]
    if kind == "exact":
        spec = sm.grid(sm.GRID_LARGE if large else sm.GRID_SMALL, max_spheres=8192)
    else:
        spec = sm.grid_around(depth_points(seqs[0][0], cams[0])[0], 0.0625 if large else 0.125, (40, 40, 40) if large else (13, 11, 9), 8192)
    total = run([[s[t] for s in seqs] for t in range(5)], cams, spec, sm.mem_of(3, 0.0, 1 if large else 0), track_of(2, 0.1),
                mf.obj_of() if objects else None, filt, where)
    assert total["seen"] > 10 and total["remembered"] > 5 and total["cleared"] > 5 and total["matched"] > 0 and total["overridden"] > 0, total


@pytest.mark.parametrize("n_cams,objects,fmt", [(1, True, U16), (1, False, FLT), (3, True, FLT)])
def test_crossing_plate_is_both_twins_and_the_definition(n_cams, objects, fmt):
    cams = [sm.exact_cam(fmt, 64, 48, t=(0.25, -0.5, 0.75 - 0.125 * i)) for i in range(n_cams)]
    frames = [[mf.crossing(c)[t] for c in cams] for t in range(4)]
    total = run(frames, cams, sm.grid(max_spheres=8192), sm.mem_of(0, mf.CROSS_MARGIN, 0), track_of(2, 0.1), mf.obj_of() if objects else None)
    assert total["remembered"] > 5 and total["cleared"] > 5 and total["matched"] > 0 and total["beside"] > 0, total
    assert not objects or total["accepted"] > 0, total


def test_the_sequences_cover_every_path():
    """the condition is about the inputs: the five-frame sequence and the crossing plate together see, remember and clear cells, match a
    sphere, accept an object, override an uncovered sphere and put a remembered sphere beside a moving one"""
    cam = sm.exact_cam(U16, 64, 48)
    spec, track, obj = sm.grid(max_spheres=8192), track_of(2, 0.1), mf.obj_of()
    a = run([[f] for f in sm.sequence(cam)], [cam], spec, sm.mem_of(3), track, obj)
    b = run([[f] for f in mf.crossing(cam)], [cam], spec, sm.mem_of(0, mf.CROSS_MARGIN, 0), track, obj)
    total = {k: a[k] + b[k] for k in a}
    assert total["seen"] > 10 and total["remembered"] > 5 and total["cleared"] > 5, total
    assert total["matched"] > 0 and total["accepted"] > 0 and total["overridden"] > 0 and total["beside"] > 0, total


# ---- 2. the self-filter ------------------------------------------------------------------------------------------------------------------
def arm_scene(wall_x=0.62, ball=None):
    """a camera looking at the arm's workspace: balls around the arm's link end points in front of a wall at x = -wall_x, the grid
    around them, and render(wall_x, spheres)"""
    from optimalmodulationds_amd import scenes
    from oracle import omds_oracle as orc
    ends = orc.link_endpoints(base._q0(), scenes.franka_dh_params())
    cam = dc.cam_of(96, 72, 80.0, 80.0, 47.5, 35.5, dc.look_at((1.6, 0.3, 0.7), (0.0, 0.0, 0.5)), U16, 0.001, 0.3, 4.0)
    spheres = [(*e, 0.07) for e in ends] + ([ball] if ball is not None else [])
    spec = spec_of((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), min_points=1, max_spheres=8192)
    return cam, spec, lambda x=wall_x, s=spheres: dc.to_u16(dc.render(cam, spheres=s, planes=[((1.0, 0.0, 0.0), -x)]))


@pytest.mark.parametrize("objects", [False, True])
def test_self_filter_forgets_the_arm_and_gives_it_no_velocity(objects):
    """the arm's balls are stored without the filter; then frames filtered at q: the self-forgotten cells leave the words, and no
    sphere inside the arm is left to carry a velocity -- the wall behind moves and keeps its own"""
    cam, spec, render = arm_scene()
    spec.self_margin = 0.03
    mem, track, obj = sm.mem_of(4), track_of(2, 0.1), mf.obj_of() if objects else None
    engines = [base._engine("franka") for _ in range(3)]
    st = {}
    first = step(*engines, st, spec, mem, track, obj, [cam], [render()], what="unfiltered")
    assert first["seen"] > 200
    q = base._q0()
    before = st["m"].copy()
    cover = step(*engines, st, spec, mem, track, obj, [cam], [render(0.605)], q=q, what="filtered, the wall 15 mm nearer")
    forgotten = (before != 0) & (st["m"] == 0)
    e = engines[0]
    assert cover["forgotten"] > 0 and forgotten.sum() > 0 and cover["matched"] > 50, "the arm's cells left the memory; the wall found itself"
    vel, have = e.get_obstacle_motion()
    cells = cells_of(spec, e.get_obstacles()[:cover["seen"] + cover["remembered"] - cover["forgotten"]])
    assert have and not np.isin(np.nonzero(forgotten)[0], cells).any(), "no sphere of the arm is in the scene: none carries a velocity"
    for x in engines:
        x.close()


# ---- 3. shared state ---------------------------------------------------------------------------------------------------------------------
def wall_frames(cams):
    return [[sm.frame(c, z) for c in cams] for z in (2.0, 2.03, 2.06, 2.09)]


def test_state_is_shared_with_the_tracked_objects_and_memory_routes():
    from optimalmodulationds_amd.engine import depth_points, depth_scene_memory_flow
    cams = gm.general_cams(3, U16, 64, 48)
    f = wall_frames(cams)
    spec = sm.grid_around(depth_points(f[0][0], cams[0])[0], 0.0625, (40, 40, 40), 8192)
    mem, track, obj = sm.mem_of(2), track_of(2, 0.1), mf.obj_of()
    a, tt, tm = (base._engine(None) for _ in range(3))
    # a tracked call, then the new call: it uses the tracked call's frame
    assert a.set_obstacles_from_depth(f[0], cams, spec, track=track)[2] == -1
    n, counts, n_matched, n_objects, n_acc = new_call(a, f[1], cams, spec, mem, track, obj)
    want = depth_scene_memory_flow(f[1], cams, spec, mem, track, None, (f[0], cams), None, cap=65536)      # per-cell flow: no table to match
    assert n_matched == want["n_matched"] > 10 and n_acc == -1, "the stored frame was the tracked call's; it stored no table"
    assert np.array_equal(bits(a.get_obstacle_motion()[0][:n]), bits(want["vel"])) and want["vel"].any()
    # ... then a tracked / objects call behaves as on an engine whose previous call was the twin's
    tt.set_obstacles_from_depth(f[0], cams, spec, track=track)
    tt.set_obstacles_from_depth(f[1], cams, spec, track=track, obj=obj)
    assert a.set_obstacles_from_depth(f[2], cams, spec, track=track, obj=obj) == tt.set_obstacles_from_depth(f[2], cams, spec, track=track, obj=obj)
    assert np.array_equal(bits(a.get_obstacles()), bits(tt.get_obstacles()))
    assert np.array_equal(bits(a.get_obstacle_motion()[0]), bits(tt.get_obstacle_motion()[0]))
    assert all(np.array_equal(x, y) for x, y in zip(a.cloud_objects(), tt.cloud_objects()))
    assert a.cloud_objects()[1].any(), "the objects call after the new call matched against the table the new call stored"
    new_call(a, f[3], cams, spec, mem, track, None)
    tt.set_obstacles_from_depth(f[3], cams, spec, track=track)
    assert a.set_obstacles_from_depth(f[2], cams, spec, track=track, obj=obj)[4] == tt.set_obstacles_from_depth(f[2], cams, spec, track=track, obj=obj)[4] == -1, \
        "without obj the new call invalidates the table as a plain tracked call does"
    # ... and the memory route continues from the new call's words
    for images in (f[1], f[3]):
        tm.set_obstacles_from_depth_memory(images, cams, spec, mem)
    blind = [sm.frame(c, None) for c in cams]
    assert a.set_obstacles_from_depth_memory(blind, cams, spec, mem) == tm.set_obstacles_from_depth_memory(blind, cams, spec, mem)
    assert np.array_equal(a.get_scene_memory(grid=True)[1], tm.get_scene_memory(grid=True)[1]) and a.get_scene_memory().max() >= 1
    for e in (a, tt, tm):
        e.close()


def test_a_refusal_leaves_scene_words_frame_and_table():
    """max_spheres one too small: the call raises; scene, motion, words, ages and labels are as before, and the next call of each
    route equals that of a twin that never made the refused call"""
    from optimalmodulationds_amd import _lib
    cam = sm.exact_cam(U16, 64, 48)
    frames = mf.crossing(cam, 6)
    spec, mem, track, obj = sm.grid(max_spheres=8192), sm.mem_of(0, mf.CROSS_MARGIN, 0), track_of(2, 0.1), mf.obj_of()
    a, b = base._engine(None), base._engine(None)
    for t in range(2):
        outs = [new_call(e, [frames[t]], [cam], spec, mem, track, obj) for e in (a, b)]
        assert outs[0] == outs[1]
    before = state_of(a, outs[0][0], obj)
    want = new_call(b, [frames[2]], [cam], spec, mem, track, obj)
    tight = sm.grid(max_spheres=want[1][0] + want[1][1] - 1)
    with pytest.raises(_lib.OmdsError) as err:
        new_call(a, [frames[2]], [cam], tight, mem, track, obj)
    assert err.value.counts == want[1] and err.value.n_occupied == want[1][0] + want[1][1]
    after = state_of(a, outs[0][0], obj)
    for key in ("scene", "vel", "have", "age", "words", "label", "flag", "n_obj"):
        assert np.array_equal(before[key], after[key]), key
    assert new_call(a, [frames[2]], [cam], spec, mem, track, obj) == want, "the new route reads words, frame and table: all as they were"
    sa, sb = state_of(a, want[0], obj), state_of(b, want[0], obj)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa) and sa["have"] and sa["flag"].any()
    tiny = sm.grid(max_spheres=8)
    with pytest.raises(_lib.OmdsError):
        new_call(a, [frames[3]], [cam], tiny, mem, track, obj)
    assert a.set_obstacles_from_depth([frames[3]], [cam], spec, track=track, obj=obj) == b.set_obstacles_from_depth([frames[3]], [cam], spec, track=track, obj=obj)
    assert np.array_equal(bits(a.get_obstacle_motion()[0]), bits(b.get_obstacle_motion()[0])) and a.cloud_objects()[1].any()
    with pytest.raises(_lib.OmdsError):
        new_call(a, [frames[4]], [cam], tiny, mem, track, obj)
    assert a.set_obstacles_from_depth_memory([frames[4]], [cam], spec, mem) == b.set_obstacles_from_depth_memory([frames[4]], [cam], spec, mem)
    assert np.array_equal(a.get_scene_memory(grid=True)[1], b.get_scene_memory(grid=True)[1])
    a.close()
    b.close()


# ---- 4. the propagate that follows -------------------------------------------------------------------------------------------------------
def test_a_scene_in_which_nothing_moves_keeps_the_static_propagate():
    cam, spec, render = arm_scene()
    a, b = base._planner(), base._planner()
    mem, track = sm.mem_of(3), track_of(2, 0.1)
    wall = render(s=[])
    for e in (a, b):
        e.set_obstacles_from_depth_memory([wall], [cam], spec, mem)
    new_call(a, [wall], [cam], spec, mem, track, mf.obj_of())
    n, counts, n_matched, _, _ = new_call(a, [wall], [cam], spec, mem, track, mf.obj_of())
    assert n_matched == n > 100 and not a.get_obstacle_motion()[1] and a.get_obstacle_horizon()[1] == 0
    for _ in range(2):
        b.set_obstacles_from_depth_memory([wall], [cam], spec, mem)
    a.prof_enable(1)
    b.prof_enable(1)
    a.propagate(base._q0())
    b.propagate(base._q0())
    base._same_rollouts(a, b, "static")
    assert a.prof_read_ex()[1] == b.prof_read_ex()[1], "another number of launches"
    a.close()
    b.close()


@pytest.mark.parametrize("frame", [False, True])
def test_a_moving_scene_propagates_as_set_obstacles_plus_motion(frame):
    """the wall comes 15 mm nearer while a ball occludes part of it: moving seen spheres beside remembered ones that stand still"""
    cam, spec, render = arm_scene()
    a, b = base._planner(), base._planner()
    for e in (a, b):
        e.set_obstacle_frame(frame)
    mem, track = sm.mem_of(3), track_of(2, 0.1)
    new_call(a, [render(0.62, [])], [cam], spec, mem, track, None)
    n, counts, n_matched, _, _ = new_call(a, [render(0.605, [(0.3, 0.3, 0.5, 0.15)])], [cam], spec, mem, track, None)
    spheres, (vel, have), age = a.get_obstacles(), a.get_obstacle_motion(), a.get_scene_memory()
    moving = (vel != 0).any(1)
    assert have and n_matched > 50 and counts[1] > 5 and moving.sum() > 50 and not moving[age >= 1].any() and (age >= 1).sum() == counts[1]
    b.set_obstacles(spheres)
    b.set_obstacle_motion(vel)
    assert a.get_obstacle_frame() == b.get_obstacle_frame() and a.get_obstacle_frame()[2] == frame
    assert np.array_equal(bits(a.get_obstacle_horizon()[0]), bits(b.get_obstacle_horizon()[0]))
    for q in (base._q0(), (base._q0() + F32(0.05)).astype(F32)):
        a.propagate(q)
        b.propagate(q)
        base._same_rollouts(a, b, frame)
    a.close()
    b.close()


# ---- 5. the facade -----------------------------------------------------------------------------------------------------------------------
def test_facade_routes_memory_motion_and_sets_ages_and_velocities():
    from helpers import weights_path
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh, q_f = torch.tensor(scenes.franka_dh_params()), torch.tensor(scenes.FRANKA_QF)
    p = MPPI(torch.tensor(base._q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 3, 32, [LinDS(q_f)], dh[:, 2], nn_model, base.K)
    cam, spec, render = arm_scene()
    lo, hi = (-0.8, -0.8, -0.1), (0.8, 0.8, 1.3)
    kw = dict(memory=dict(max_age=3), dt_frame=0.1, memory_motion=True)
    n1, c1 = p.update_obstacles_from_depth([render(0.62, [])], [cam], 0.05, lo, hi, **kw)
    assert c1[0] == n1 > 100 and c1[1:] == (0, 0, 0, 0) and (p.obs_age.numpy() == 0).all() and p.cloud_matched == -1 and p.obs_velocities is None
    n2, c2 = p.update_obstacles_from_depth([render(0.605, [(0.3, 0.3, 0.5, 0.15)])], [cam], 0.05, lo, hi, moving_frame=True, objects=True, **kw)
    age = p.obs_age.numpy()
    assert c2[1] > 5 and (age >= 1).sum() == c2[1] and p.n_obs == n2 == len(age) and p.cloud_matched > 50
    assert p.obs_velocities is not None and (p.obs_velocities.numpy()[age == 0] != 0).any() and not p.obs_velocities.numpy()[age >= 1].any()
    assert p.cloud_objects >= 1 and p.cloud_objects_matched == -1, "the first call stored no component table"
    assert p._engine.get_obstacle_frame()[2], "moving_frame= is honoured as on the tracked route"
    assert np.isfinite(p.propagate()[0].numpy()).all()
    plain = p.update_obstacles_from_depth([render(0.62, [])], [cam], 0.05, lo, hi)
    assert plain[0] == plain[1] and p.obs_age is None
    for bad in (dict(memory_motion=True), dict(memory_motion=True, memory=dict(max_age=2)), dict(memory_motion=True, dt_frame=0.1),
                dict(memory=dict(max_age=2), dt_frame=0.1), dict(memory=dict(max_age=2), dt_frame=0.1, objects=True)):
        with pytest.raises(ValueError):
            p.update_obstacles_from_depth([render()], [cam], 0.05, lo, hi, **bad)
    with pytest.raises(TypeError):
        p.update_obstacles_from_depth([render()], [cam], 0.05, lo, hi, memory_motoin=True)
