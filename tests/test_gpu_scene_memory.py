"""The depth route with a scene memory on the device (include/omds.h: omds_set_obstacles_from_depth_memory) against the host
definition omds_depth_scene_memory iterated from the same stored memory: the stored words, the installed scene, the counts and the
ages are the definition's, word for word and bit for bit.  On the exact camera of tests/scene_memory_cases.py the numpy restatement
must give the same words too; on general cameras (fx = 615.3, rotations from quaternions) device and host definition are compared with
each other only.

Grids: 13 x 11 x 9 (1 287 cells: two compaction blocks, the second partial, and one workgroup of k_scene_memory with padding) and
40 x 40 x 40 (64 000 cells: 63 workgroups' worth of lanes, the last block partial).  Images 32 x 24 and 64 x 48; 1, 3 and 8 cameras;
uint16 and float32."""
import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import depth_cases as dc
import scene_memory_cases as sm
import test_gpu_cloud_flow as base
from cloud_cases import F32, cells_of
from cloud_flow_cases import track_of
from depth_cases import FLT, U16

pytestmark = pytest.mark.gpu

bits = base.bits
PAD = np.array(base.PAD, F32)


def host(spec, mem, cams, images, m):
    from optimalmodulationds_amd.engine import depth_scene_memory
    return depth_scene_memory(images, cams, spec, mem, m)


def scene_of(spec, words, k=base.K):
    """the scene the definition installs for the words: the spheres of the cells that are not 0 in cell order, padded to n_closest"""
    cells = np.nonzero(words)[0]
    radius = F32(spec.radius) if spec.radius > 0 else F32(0.8660254) * F32(spec.voxel)
    spheres = np.concatenate([sm.centres_of(spec, cells), np.full((len(cells), 1), radius, F32)], 1)
    pad = np.tile(PAD, (max(k - len(cells), 0), 1))
    age = np.concatenate([words[cells].astype(np.int64) - 1, np.full(len(pad), -1)]).astype(np.int32)
    return np.concatenate([spheres, pad]).astype(F32), age, len(cells)


def step(e, spec, mem, cams, images, m, q=None, device_images=None, restated=False, what=""):
    """one memory call on the device against one application of the host definition to the words ``m``; -> the new words"""
    want, want_counts = host(spec, mem, cams, images, m)
    if restated:
        inexact = []
        again, again_counts = sm.restate(spec, mem, cams, images, m, inexact)
        assert not inexact and np.array_equal(again, want) and again_counts == want_counts, f"{what}: the restatement differs from the host definition"
    n_spheres, counts = e.set_obstacles_from_depth_memory(images if device_images is None else device_images, cams, spec, mem, q)
    age, grid = e.get_scene_memory(grid=True)
    assert q is not None or (np.array_equal(grid, want) and counts == want_counts + (0,)), (what, counts, want_counts, int((grid != want).sum()))
    scene, want_age, n = scene_of(spec, grid)
    assert n_spheres == n and e.n_obs == len(scene), what
    assert np.array_equal(bits(e.get_obstacles()), bits(scene)), f"{what}: the scene is not the spheres of the stored words"
    assert np.array_equal(age, want_age), f"{what}: ages"
    return grid, counts, want, want_counts


def exact_cams(n, fmt, width, height):
    return [sm.exact_cam(fmt, width, height, t=(0.25, -0.5 + 0.125 * i, 0.75 - 0.0625 * i)) for i in range(n)]


def general_cams(n, fmt, width, height):
    rng = np.random.RandomState(7)
    return [dc.cam_of(width, height, 615.3 * width / 640, 614.9 * width / 640, width / 2 - 0.37, height / 2 + 0.21,
                      dc.quat_pose(np.array([0.8, 0.1, -0.5, 0.3]) + 0.04 * i * rng.standard_normal(4), (0.31 + 0.05 * i, -0.12, 0.93 - 0.03 * i)),
                      fmt, 0.001, 0.3, 4.0) for i in range(n)]


@pytest.fixture
def engine():
    e = base._engine(None)
    yield e
    e.close()


# ---- 1. sequences --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_cams,fmt,size,large", [("exact", 1, U16, (32, 24), False), ("exact", 3, FLT, (64, 48), True),
                                                         ("exact", 8, U16, (64, 48), True), ("exact", 3, U16, (32, 24), False),
                                                         ("general", 1, U16, (64, 48), False), ("general", 3, FLT, (64, 48), True),
                                                         ("general", 8, U16, (32, 24), True)])
def test_sequence_is_the_definition_iterated(engine, kind, n_cams, fmt, size, large):
    """wall, a plate in front of its left half, plate gone, a blind frame, the wall gone: after every frame the stored words, the
    scene, the counts and the ages are those of the host definition applied to the words stored before"""
    from optimalmodulationds_amd.engine import depth_points
    cams = (exact_cams if kind == "exact" else general_cams)(n_cams, fmt, *size)
    frames = [sm.sequence(c) for c in cams]
    if kind == "exact":
        spec = sm.grid(sm.GRID_LARGE if large else sm.GRID_SMALL, max_spheres=8192)
    else:
        spec = sm.grid_around(depth_points(frames[0][0], cams[0])[0], 0.0625 if large else 0.125, (40, 40, 40) if large else (13, 11, 9), 8192)
    mem = sm.mem_of(max_age=3, clear_margin=0.0, footprint=1 if large else 0)
    m, totals = None, np.zeros(4, np.int64)
    for t in range(5):
        m, counts, _, _ = step(engine, spec, mem, cams, [f[t] for f in frames], m, restated=kind == "exact", what=f"{kind} frame {t}")
        totals += counts[:4]
    assert totals[0] > 10 and totals[1] > 5 and totals[2] > 5, f"the sequence saw, remembered and cleared cells: {totals}"
    m, counts, _, _ = step(engine, spec, mem, cams, [f[0] for f in frames], m, restated=kind == "exact", what=f"{kind} the wall again")
    walls = counts[0]
    for t in range(4):      # blind frames: remembered for max_age = 3 calls, expired at the fourth
        m, counts, _, _ = step(engine, spec, mem, cams, [sm.frame(c, None) for c in cams], m, what=f"{kind} blind {t}")
        assert counts[3 if t == 3 else 1] >= walls > 10, (t, counts)
    assert not m.any(), "what no camera could clear expires after max_age unseen calls"


def test_first_call_is_the_plain_depth_call(engine):
    other = base._engine(None)
    cams = exact_cams(3, U16, 64, 48)
    images = [dc.exact_image(20 + i, 64, 48) for i in range(3)]
    spec = sm.grid(sm.GRID_LARGE, max_spheres=8192)
    n, counts = engine.set_obstacles_from_depth_memory(images, cams, spec, sm.mem_of(2))
    want = other.set_obstacles_from_depth(images, cams, spec)
    assert (n, counts[0]) == want and counts[1:] == (0, 0, 0, 0) and n > 100
    assert np.array_equal(bits(engine.get_obstacles()), bits(other.get_obstacles()))
    assert (engine.get_scene_memory() == 0).all()
    other.close()


# ---- 2. where the images live --------------------------------------------------------------------------------------------------------
def test_host_device_and_strided_images_give_the_same_bits():
    engines = [base._engine(None) for _ in range(3)]
    dev = f"cuda:{engines[0].device}"
    cams = [sm.exact_cam(U16), sm.exact_cam(FLT, t=(0.25, -0.375, 0.6875))]
    frames = [sm.sequence(c) for c in cams]
    spec, mem = sm.grid(), sm.mem_of(2, 0.0, 1)
    m = None
    for t in range(5):
        images = [f[t] for f in frames]
        on_dev, views = [], []
        for img in images:
            as_torch = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
            on_dev.append(as_torch(img))
            wide = np.zeros((img.shape[0], img.shape[1] + 5), img.dtype)
            wide[:, 3:-2] = img
            views.append(as_torch(wide)[:, 3:-2])
            assert views[-1].stride(0) == img.shape[1] + 5 and not views[-1].is_contiguous()
        out = [step(e, spec, mem, cams, images, m, device_images=src, restated=True, what=f"frame {t}")
               for e, src in zip(engines, (None, on_dev, views))]
        assert all(np.array_equal(o[0], out[0][0]) and o[1] == out[0][1] for o in out)
        assert all(np.array_equal(bits(e.get_obstacles()), bits(engines[0].get_obstacles())) for e in engines)
        m = out[0][0]
    for e in engines:
        e.close()


# ---- 3. the self-filter --------------------------------------------------------------------------------------------------------------
def test_self_filter_forgets_the_cells_inside_the_arm():
    """balls around the arm's link end points in front of a wall are stored WITHOUT the filter; the next frame is blind and filtered at
    q: every cell is remembered, the candidates inside the arm are dropped and their words are 0 afterwards.  The kept set is the one
    the cloud call's self-filter keeps on the same candidates (a second engine, the cell centres as its cloud)"""
    from optimalmodulationds_amd import scenes
    from oracle import omds_oracle as orc
    from cloud_cases import spec_of
    q = base._q0()
    ends = orc.link_endpoints(q, scenes.franka_dh_params())
    cam = dc.cam_of(96, 72, 80.0, 80.0, 47.5, 35.5, dc.look_at((1.6, 0.3, 0.7), (0.0, 0.0, 0.5)), U16, 0.001, 0.3, 4.0)
    img = dc.to_u16(dc.render(cam, spheres=[(*e, 0.07) for e in ends], planes=[((1.0, 0.0, 0.0), -0.6)]))
    spec = spec_of((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), min_points=1, max_spheres=8192)
    spec.self_margin = 0.03
    mem = sm.mem_of(4)
    a, b = base._engine("franka"), base._engine("franka")
    m1, counts, _, _ = step(a, spec, mem, [cam], [img], None, what="unfiltered")
    assert counts[0] > 200
    blind = sm.frame(cam, None)
    want, want_counts = host(spec, mem, [cam], [blind], m1)
    cand = np.nonzero(want)[0]
    assert want_counts == (0, len(cand), 0, 0) and np.array_equal(cand, np.nonzero(m1)[0])
    n_kept, n_cand = b.set_obstacles_from_cloud(sm.centres_of(spec, cand), spec, q)
    kept = b.get_obstacles()[:n_kept]
    assert n_cand == len(cand) and 0 < n_kept < n_cand, "the filter drops some candidates and keeps some"
    kept_cells = cells_of(spec, kept)
    final = np.zeros_like(want)
    final[kept_cells] = want[kept_cells]
    m2, counts, _, _ = step(a, spec, mem, [cam], [blind], m1, q=q, what="filtered")
    assert counts == (0, n_cand, 0, 0, n_cand - n_kept) and np.array_equal(m2, final), "the dropped cells must leave the memory"
    assert np.array_equal(bits(a.get_obstacles()), bits(b.get_obstacles()))
    dropped = np.setdiff1d(cand, kept_cells)
    assert len(dropped) and not m2[dropped].any() and (m2[kept_cells] == 2).all()
    m3, counts, _, _ = step(a, spec, mem, [cam], [blind], m2, q=q, what="filtered again")      # nothing left to forget
    assert counts == (0, n_kept, 0, 0, 0) and (m3[kept_cells] == 3).all()
    a.close()
    b.close()


# ---- 4. refusal, reset, another key ----------------------------------------------------------------------------------------------------
def test_too_many_cells_is_refused_with_scene_and_memory_unchanged(engine):
    from optimalmodulationds_amd import _lib
    cam = sm.exact_cam()
    seq = sm.sequence(cam)
    spec, mem = sm.grid(), sm.mem_of(3)
    m = None
    for t in range(2):
        m, _, _, _ = step(engine, spec, mem, [cam], [seq[t]], m, restated=True)
    before = engine.get_obstacles().copy()
    want, want_counts = host(spec, mem, [cam], [seq[2]], m)
    tight = sm.grid(max_spheres=want_counts[0] + want_counts[1] - 1)
    with pytest.raises(_lib.OmdsError) as err:
        engine.set_obstacles_from_depth_memory([seq[2]], [cam], tight, mem)
    assert err.value.counts == want_counts + (0,) and err.value.n_occupied == want_counts[0] + want_counts[1]
    age, grid = engine.get_scene_memory(grid=True)
    assert np.array_equal(grid, m) and np.array_equal(bits(engine.get_obstacles()), bits(before)) and engine.n_obs == len(before)
    assert np.array_equal(age, scene_of(spec, m)[1])
    exact = sm.grid(max_spheres=want_counts[0] + want_counts[1])      # exactly as many as there are: taken
    m3, _, _, _ = step(engine, exact, mem, [cam], [seq[2]], m, restated=True, what="the next good call proceeds from the old memory")
    assert np.array_equal(m3, want)


@pytest.mark.parametrize("change", ["voxel", "max_age", "clear_margin", "footprint", "min_points", "reset"])
def test_another_key_or_a_reset_starts_from_empty_memory(engine, change):
    cam = sm.exact_cam()
    spec, mem = sm.grid(), sm.mem_of(3, 0.25, 0)
    m, _, _, _ = step(engine, spec, mem, [cam], [sm.frame(cam, 2.0, 2)], None)
    kept, _, _, _ = step(engine, spec, mem, [cam], [sm.frame(cam, None)], m, what="the same key remembers")
    assert (kept[m != 0] == 2).all() and m.any()
    if change == "voxel":
        spec = sm.grid(dict(sm.GRID_SMALL, voxel=0.25))
    elif change == "min_points":
        spec = sm.grid(min_points=2)
    elif change == "reset":
        engine.scene_memory_reset()
        assert engine.get_scene_memory(grid=True)[1].size == 0
    else:
        mem = sm.mem_of(**dict(dict(max_age=3, clear_margin=0.25, footprint=0), **{change: dict(max_age=4, clear_margin=0.5, footprint=1)[change]}))
    empty, counts, _, _ = step(engine, spec, mem, [cam], [sm.frame(cam, None)], None, what=change)
    assert counts == (0, 0, 0, 0, 0) and not empty.any() and len(empty) == sm.n_cells_of(spec)
    assert np.array_equal(bits(engine.get_obstacles()), bits(np.tile(PAD, (base.K, 1))))


# ---- 5. interplay with the other routes ------------------------------------------------------------------------------------------------
def test_focus_selects_from_the_remembered_scene_and_clearing_restores_it():
    e = base._engine("franka")
    cam = dc.cam_of(96, 72, 80.0, 80.0, 47.5, 35.5, dc.look_at((1.6, 0.3, 0.7), (0.0, 0.0, 0.5)), U16, 0.001, 0.3, 4.0)
    wall = dc.to_u16(dc.render(cam, planes=[((1.0, 0.0, 0.0), -0.6)]))
    from cloud_cases import spec_of
    spec, mem = spec_of((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), max_spheres=8192), sm.mem_of(5)
    m, _, _, _ = step(e, spec, mem, [cam], [wall], None)
    m, counts, _, _ = step(e, spec, mem, [cam], [sm.frame(cam, None)], m)
    master = e.get_obstacles().copy()
    assert counts[1] == len(master) > 100
    kept, passed = e.focus_obstacles(base._q0(), 0.05)
    idx = e.obstacle_focus()
    assert base.K <= kept < len(master) and np.array_equal(bits(e.get_obstacles()), bits(master[idx]))
    assert (e.get_scene_memory() == -1).all(), "under a focus the scene is another setter's"
    e.clear_obstacle_focus()
    assert np.array_equal(bits(e.get_obstacles()), bits(master)) and e.obstacle_focus() is None
    assert np.array_equal(e.get_scene_memory(grid=True)[1], m), "the focus leaves the stored memory alone"
    e.close()


def test_memory_calls_leave_the_record_frame_and_the_plain_route_alone():
    """a tracked depth frame, memory calls, the next tracked frame: counts, scene and velocities are those of an engine that never made
    a memory call; and the plain depth call gives the same bits before and after memory calls as on a fresh engine"""
    a, b, fresh = (base._engine(None) for _ in range(3))
    cams = general_cams(3, U16, 64, 48)
    from optimalmodulationds_amd.engine import depth_points
    near, far = [sm.frame(c, 2.0) for c in cams], [sm.frame(c, 2.06) for c in cams]
    spec, track = sm.grid_around(depth_points(near[0], cams[0])[0], 0.0625, (40, 40, 40), 8192), track_of(2, 0.1)
    plain = fresh.set_obstacles_from_depth(near, cams, spec)
    plain_scene = fresh.get_obstacles().copy()
    assert a.set_obstacles_from_depth(near, cams, spec) == plain and np.array_equal(bits(a.get_obstacles()), bits(plain_scene))
    first = [e.set_obstacles_from_depth(near, cams, spec, track=track) for e in (a, b)]
    assert first[0] == first[1] and first[0][2] == -1
    m = None
    for images in (near, [sm.frame(c, None) for c in cams], far):
        m, _, _, _ = step(a, spec, sm.mem_of(2), cams, images, m)
    assert not a.get_obstacle_motion()[1], "the memory route installs a static scene"
    assert a.set_obstacles_from_depth(near, cams, spec) == plain and np.array_equal(bits(a.get_obstacles()), bits(plain_scene))
    second = [e.set_obstacles_from_depth(far, cams, spec, track=track) for e in (a, b)]
    assert second[0] == second[1] and second[0][2] > 0
    assert np.array_equal(bits(a.get_obstacles()), bits(b.get_obstacles()))
    (va, ha), (vb, hb) = a.get_obstacle_motion(), b.get_obstacle_motion()
    assert ha == hb and np.array_equal(bits(va), bits(vb))
    assert np.array_equal(a.get_scene_memory(grid=True)[1], m), "and the other routes leave the stored memory alone"
    for e in (a, b, fresh):
        e.close()


# ---- 6. the facade ---------------------------------------------------------------------------------------------------------------------
def test_facade_routes_memory_and_sets_obs_age():
    from helpers import weights_path
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh, q_f = torch.tensor(scenes.franka_dh_params()), torch.tensor(scenes.FRANKA_QF)
    p = MPPI(torch.tensor(base._q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 3, 32, [LinDS(q_f)], dh[:, 2], nn_model, base.K)
    cam = dc.cam_of(96, 72, 80.0, 80.0, 47.5, 35.5, dc.look_at((1.6, 0.3, 0.7), (0.0, 0.0, 0.5)), U16, 0.001, 0.3, 4.0)
    wall = dc.to_u16(dc.render(cam, planes=[((1.0, 0.0, 0.0), -0.6)]))
    lo, hi = (-0.8, -0.8, -0.1), (0.8, 0.8, 1.3)
    n1, c1 = p.update_obstacles_from_depth([wall], [cam], 0.05, lo, hi, memory=dict(max_age=2))
    assert c1[0] == n1 > 100 and (p.obs_age.numpy() == 0).all() and p.n_obs == n1
    n2, c2 = p.update_obstacles_from_depth([sm.frame(cam, None)], [cam], 0.05, lo, hi, memory=sm.mem_of(2))
    assert n2 == n1 and c2 == (0, n1, 0, 0, 0) and (p.obs_age.numpy() == 1).all()
    assert np.isfinite(p.propagate()[0].numpy()).all()
    plain = p.update_obstacles_from_depth([wall], [cam], 0.05, lo, hi)
    assert plain == (n1, n1) and p.obs_age is None
    for kw in (dict(dt_frame=0.1), dict(dt_frame=0.1, objects=True)):
        with pytest.raises(ValueError):
            p.update_obstacles_from_depth([wall], [cam], 0.05, lo, hi, memory=dict(max_age=2), **kw)
    with pytest.raises(TypeError):
        p.update_obstacles_from_depth([wall], [cam], 0.05, lo, hi, memroy=None)
