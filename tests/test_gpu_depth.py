"""The scene straight from depth images on the device (include/omds.h: omds_set_obstacles_from_depth; csrc/depth_kernels.hip:
k_depth_count, k_depth_count_rec in front of the unchanged rest of the cloud calls).  The reference side of every comparison is a
SECOND Engine that is given engine.depth_points(...) of every image, concatenated in camera order, through the existing cloud calls
(checked on their own in tests/test_gpu_cloud*.py); the host definition of the points is checked in tests/test_depth_cpu.py.
Everything is bit for bit: counts and record sums are integers, and the deprojection is one source for host and kernel.

The kernel's mapping: blockIdx.y is the camera; a lane takes a run of 4 consecutive visited pixels of a row; a workgroup has 256
lanes; at most 2048 / n_cams workgroups stride over a camera's runs, so one sweep of the launched grid covers (2048 / n_cams) * 256 * 4
visited pixels per camera (2 097 152 with one camera, 698 368 with three)."""
import ctypes as C

import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import depth_cases as dc
import test_gpu_cloud_flow as base
from cloud_cases import F32, spec_of
from cloud_flow_cases import track_of
from cloud_object_cases import obj_of
from depth_cases import FLT, U16

pytestmark = pytest.mark.gpu

bits = base.bits
ERR_INVALID_ARG = 1
BOX = dict(origin=(-3.2, -3.2, -3.2), voxel=0.05, dims=(128, 128, 128))      # holds every point within 2.9 m of the origin


def points_of(images, cams):
    from optimalmodulationds_amd.engine import depth_points
    got = [depth_points(im, c) for im, c in zip(images, cams)]
    return np.concatenate([g[0] for g in got]), sum(g[1] for g in got)


def cloud_call(e, pts, spec, q=None, track=None, obj=None):
    if track is None:
        return e.set_obstacles_from_cloud(pts, spec, q)
    if obj is None:
        return e.set_obstacles_from_cloud_tracked(pts, spec, track, q)
    return e.set_obstacles_from_cloud_objects(pts, spec, track, obj, q)


def assert_same_state(a, b, what="", objects=False):
    """the scene, the velocities, the horizon mode (and labels and flags) in force on both contexts are the same bits"""
    sa, sb = a.get_obstacles(), b.get_obstacles()
    assert a.n_obs == b.n_obs and sa.shape == sb.shape and np.array_equal(bits(sa), bits(sb)), f"{what}: scene"
    (va, ha), (vb, hb) = a.get_obstacle_motion(), b.get_obstacle_motion()
    assert ha == hb and np.array_equal(bits(va), bits(vb)), f"{what}: velocities"
    if (a.C and b.C) or not ha:      # (the tables of a motion horizon need the network)
        assert a.get_obstacle_horizon()[1] == b.get_obstacle_horizon()[1], f"{what}: horizon mode"
    if objects:
        (la, fa, na), (lb, fb, nb) = a.cloud_objects(), b.cloud_objects()
        assert np.array_equal(la, lb) and np.array_equal(fa, fb) and na == nb, f"{what}: labels / object flags"


def both(e_depth, e_cloud, images, cams, spec, q=None, track=None, obj=None, what="", device_images=None):
    """the depth call on one context, the cloud call on the points of the images on the other: same counts, same state"""
    pts, n_valid = points_of(images, cams)
    got = e_depth.set_obstacles_from_depth(images if device_images is None else device_images, cams, spec, q, track, obj)
    want = cloud_call(e_cloud, pts, spec, q, track, obj)
    assert got == want, (what, got, want)
    assert_same_state(e_depth, e_cloud, what, obj is not None)
    return got, n_valid


def random_image(seed, cam, lo=0.4, hi=2.5, holes=0.1):
    rng = np.random.RandomState(seed)
    metres = rng.uniform(lo, hi, (cam.height, cam.width))
    if cam.format == U16:
        img = dc.to_u16(metres, cam.depth_scale)
        img[rng.rand(cam.height, cam.width) < holes] = 0
        return img
    img = metres.astype(F32)
    img[rng.rand(cam.height, cam.width) < holes] = np.nan
    return img


def camera(width, height, fmt=U16, step=1, seed=0, pitch=0):
    rng = np.random.RandomState(100 + seed)
    return dc.cam_of(width, height, 615.3 * width / 640, 614.9 * width / 640, width / 2 - 0.37, height / 2 + 0.21,
                     dc.quat_pose(rng.standard_normal(4), rng.uniform(-0.3, 0.3, 3)), fmt, 0.001, 0.3, 4.0, step, pitch)


@pytest.fixture
def pair():
    engines = [base._engine(None), base._engine(None)]
    yield engines
    for e in engines:
        e.close()


# ---- 1. image shapes, untracked --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height,step", [(1, 1, 1), (13, 7, 1), (67, 49, 1), (67, 49, 2), (67, 49, 3)])
@pytest.mark.parametrize("fmt", [U16, FLT])
def test_one_image_untracked(pair, width, height, step, fmt):
    """1 x 1; 13 x 7 (fewer pixels than a wave, an odd width: the last run of every row is short); 67 x 49 at step 1, 2, 3"""
    cam = camera(width, height, fmt, step)
    img = random_image(1, cam, holes=0.0 if width == 1 else 0.1)
    spec = spec_of(**BOX, max_spheres=8192)
    got, n_valid = both(*pair, [img], [cam], spec, what=f"{width}x{height}/{step}")
    assert 0 < got[0] <= n_valid and got[0] == got[1]
    if step == 1 and width > 1:
        assert got[0] > 0.6 * n_valid, "random depths: nearly every kept pixel has its own cell"


def test_three_cameras_and_their_order(pair):
    """U16 64 x 48, F32 33 x 17 with pitch 40, U16 1 x 1 in one call; then the same cameras permuted"""
    cams = [camera(64, 48, U16, seed=1), camera(33, 17, FLT, seed=2, pitch=40), camera(1, 1, U16, seed=3)]
    flat = np.full(16 * 40 + 33, np.nan, F32)
    view = np.lib.stride_tricks.as_strided(flat, (17, 33), (160, 4))
    view[:] = random_image(3, cams[1])
    images = [random_image(2, cams[0]), view, np.array([[1500]], np.uint16)]
    spec = spec_of(**BOX, min_points=1, max_spheres=8192)
    got, n_valid = both(*pair, images, cams, spec, what="three cameras")
    assert got[0] > 2000 and n_valid > 64 * 48 * 0.7 + 33 * 17 * 0.7
    for order in ((2, 0, 1), (1, 2, 0)):
        again, _ = both(*pair, [images[i] for i in order], [cams[i] for i in order], spec, what=f"order {order}")
        assert again == got
    flat_again = pair[0].set_obstacles_from_depth([images[0], flat, images[2]], cams, spec)      # a flat buffer laid out by the camera's pitch
    assert flat_again == got


def test_more_pixels_than_one_sweep_of_the_grid(pair):
    """three 1280 x 1024 U16 images: 1 310 720 visited pixels each, against 698 368 per camera in one sweep of the launched grid
    (682 workgroups x 256 lanes x 4 pixels): every workgroup goes round its loop twice, the last round partly empty; 3 932 160
    visited pixels in all, within 2^24.  The images are smooth (a tilted plane with ripples), so that few cells are occupied"""
    cams, images = [], []
    v, u = np.mgrid[0:1024, 0:1280]
    for i in range(3):
        cams.append(camera(1280, 1024, U16, seed=10 + i))
        images.append(dc.to_u16(1.5 + 0.3 * i + 0.0003 * u + 0.0002 * v + 0.02 * np.sin(u / 40.0) * np.cos(v / 55.0)))
    images[1][::7, ::5] = 0
    spec = spec_of((-4.0, -4.0, -4.0), 0.1, (80, 80, 80), min_points=3, max_spheres=65536)
    got, n_valid = both(*pair, images, cams, spec, what="two sweeps")
    assert n_valid > 3_500_000 and 500 < got[0] < 65536


# ---- 2. contention extremes ---------------------------------------------------------------------------------------------------------
def narrow_camera(fmt=U16, t=(0.0, 0.0, 0.0)):
    """67 x 49 pixels within +- 0.4 mm of the optical axis at 1 m: all points of one depth fall in one 5 cm cell"""
    return dc.cam_of(67, 49, 1.0e5, 1.0e5, 33.0, 24.0, dc.pose_of(np.eye(3), t), fmt, 0.001, 0.3, 4.0)


CELL_BOX = dict(origin=(-0.225, -0.225, 0.775), voxel=0.05, dims=(9, 9, 29))      # (0, 0, 1) and (0, 0, 2) are the middles of cells


def one_cell_image():
    return np.full((49, 67), 1000, np.uint16)


def two_cell_image():
    img = np.full((49, 67), 1000, np.uint16)
    img.reshape(-1)[1::2] = 2000          # neighbouring pixels alternate between two depths a metre apart
    return img


def speckle():
    """a wide camera whose neighbouring pixels alternate between 1 m and 2 m: 3 pixels per 5 cm cell at 1 m, so the 256 pixels of a wave
    hold dozens of distinct cells, more than the bounded rounds of the wave aggregation take"""
    cam = dc.cam_of(67, 49, 60.0, 60.0, 33.0, 24.0, dc.pose_of(np.eye(3), (0, 0, 0)), U16, 0.001, 0.3, 4.0)
    img = two_cell_image()
    img[::5, ::3] += 7
    return cam, img


def test_all_points_in_one_cell_counted_through_min_points(pair):
    """the wave aggregation's worst case: 3 283 pixels, one cell.  It is occupied at min_points = n_valid and empty at n_valid + 1"""
    cam, img = narrow_camera(), one_cell_image()
    n = 67 * 49
    for min_points, occupied in ((1, 1), (n, 1), (n + 1, 0)):
        got, n_valid = both(*pair, [img], [cam], spec_of(**CELL_BOX, min_points=min_points), what=f"one cell, min_points {min_points}")
        assert n_valid == n and got == (occupied, occupied)
    img[5, 7], img[20, 1] = 0, 60000      # two pixels fewer
    got, n_valid = both(*pair, [img], [cam], spec_of(**CELL_BOX, min_points=n - 2), what="one cell less two")
    assert n_valid == n - 2 and got == (1, 1)
    assert both(*pair, [img], [cam], spec_of(**CELL_BOX, min_points=n - 1))[0] == (0, 0)


def test_speckle_in_two_cells_counted_through_min_points(pair):
    cam, img = narrow_camera(), two_cell_image()
    near, far = 1642, 1641                # 3 283 pixels, the even ones near
    for min_points, occupied in ((1, 2), (far, 2), (near, 1), (near + 1, 0)):
        got, n_valid = both(*pair, [img], [cam], spec_of(**CELL_BOX, min_points=min_points), what=f"two cells, min_points {min_points}")
        assert n_valid == near + far and got == (occupied, occupied)


@pytest.mark.parametrize("min_points", [1, 2, 3])
def test_speckle_with_more_cells_in_a_wave_than_rounds(pair, min_points):
    cam, img = speckle()
    spec = spec_of((-1.5, -1.5, 0.5), 0.05, (60, 60, 40), min_points=min_points, max_spheres=8192)
    got, _ = both(*pair, [img], [cam], spec, what="speckle")
    assert got[0] > {1: 300, 2: 300, 3: 100}[min_points]


@pytest.mark.parametrize("case", ["one-cell", "two-cell", "speckle"])
def test_contention_extremes_tracked(pair, case):
    """the same extremes through the tracked call; the second frame is the first seen from a camera shifted by (10, -5, 15) mm, less
    than a cell: the velocities come from the sums of the sub-cell offsets and must be the cloud route's bits"""
    if case == "speckle":
        cam, img = speckle()
        spec = spec_of((-1.5, -1.5, 0.5), 0.05, (60, 60, 40), min_points=2, max_spheres=8192)
    else:
        cam, img = narrow_camera(), one_cell_image() if case == "one-cell" else two_cell_image()
        spec = spec_of(**CELL_BOX, min_points=100)
    moved = dc.cam_of(67, 49, cam.fx, cam.fy, 33.0, 24.0, dc.pose_of(np.eye(3), (0.010, -0.005, 0.015)), U16, 0.001, 0.3, 4.0)
    track = track_of(1, 0.1)
    first, _ = both(*pair, [img], [cam], spec, track=track, what=case + " frame 1")
    assert first[2] == -1
    second, _ = both(*pair, [img], [moved], spec, track=track, what=case + " frame 2")
    vel, have = pair[0].get_obstacle_motion()
    assert have and second[2] > 0.9 * second[0] > 0
    if case != "speckle":
        assert second[2] == second[0] == (1 if case == "one-cell" else 2)
        assert np.allclose(vel[:second[0]], [0.1, -0.05, 0.15], atol=0.05), "about 10, -5, 15 mm in 0.1 s (offsets count in 1/256 cell)"


# ---- 3. tracked and objects: a sphere moving in front of a wall, two cameras -----------------------------------------------------
SCENE_BOX = dict(origin=(0.0, -1.0, 0.0), voxel=0.05, dims=(28, 40, 24))


def scene_cameras():
    return [dc.cam_of(64, 48, 60.0, 60.0, 31.5, 23.5, dc.look_at(eye, (0.9, 0.0, 0.5)), U16, 0.001, 0.3, 4.0)
            for eye in ((-0.5, -0.6, 0.6), (-0.5, 0.7, 0.9))]


def scene_frames(n=3):
    """per frame the two rendered U16 images: a sphere of radius 0.15 m moving 4 cm per frame along y, 0.5 m in front of the wall x = 1.2"""
    cams = scene_cameras()
    return cams, [[dc.to_u16(dc.render(c, spheres=[(0.7, -0.2 + 0.04 * f, 0.5, 0.15)], planes=[((1.0, 0.0, 0.0), 1.2)])) for c in cams] for f in range(n)]


@pytest.mark.parametrize("route", ["tracked", "objects"])
def test_moving_sphere_in_front_of_a_wall(pair, route):
    cams, frames = scene_frames()
    spec, track = spec_of(**SCENE_BOX, min_points=2), track_of(2, 0.1)
    obj = obj_of(1, 4) if route == "objects" else None
    seen = []
    for f, images in enumerate(frames):
        got, _ = both(*pair, images, cams, spec, track=track, obj=obj, what=f"{route} frame {f}")
        seen.append(got)
    assert seen[0][2] == -1 and seen[1][2] > 0 and seen[2][2] > 0 and seen[0][0] > 100
    vel, have = pair[0].get_obstacle_motion()
    assert have and (np.abs(vel[:, 1]) > 0.1).sum() >= 4, "the sphere's cells move along y"
    if route == "objects":
        assert seen[0][3] >= 2 and seen[0][4] == -1 and seen[2][4] >= 1, "the wall and the sphere are objects; from frame 1 on they are matched"


@pytest.mark.parametrize("depth_first", [True, False])
def test_frames_may_alternate_between_depth_and_cloud_calls(pair, depth_first):
    """frame 0 through the depth call and frame 1 through omds_set_obstacles_from_cloud_tracked on the same context, and the other way
    round: both share the one stored frame, so both give what the all-cloud sequence gives"""
    cams, frames = scene_frames(2)
    spec, track = spec_of(**SCENE_BOX, min_points=2), track_of(2, 0.1)
    mixed, cloud = pair
    pts = [points_of(images, cams)[0] for images in frames]
    for f in range(2):
        want = cloud.set_obstacles_from_cloud_tracked(pts[f], spec, track)
        if depth_first == (f == 0):
            got = mixed.set_obstacles_from_depth(frames[f], cams, spec, track=track)
        else:
            got = mixed.set_obstacles_from_cloud_tracked(pts[f], spec, track)
        assert got == want
        assert_same_state(mixed, cloud, f"frame {f}")
    assert want[2] > 0 and cloud.get_obstacle_motion()[1]


# ---- 4. the self-filter -----------------------------------------------------------------------------------------------------------
def test_self_filter_keeps_the_cloud_calls_list():
    """the franka network at FRANKA_Q0; the image shows balls around the arm's link end points (a band around the arm) in front of a
    wall: the kept list is the cloud call's, and some candidates are dropped"""
    from optimalmodulationds_amd import scenes
    from oracle import omds_oracle as orc
    ends = orc.link_endpoints(base._q0(), scenes.franka_dh_params())
    cam = dc.cam_of(96, 72, 80.0, 80.0, 47.5, 35.5, dc.look_at((1.6, 0.3, 0.7), (0.0, 0.0, 0.5)), U16, 0.001, 0.3, 4.0)
    img = dc.to_u16(dc.render(cam, spheres=[(*e, 0.07) for e in ends], planes=[((1.0, 0.0, 0.0), -0.6)]))
    spec = spec_of((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), min_points=1, max_spheres=8192)
    spec.self_margin = 0.03
    a, b = base._engine("franka"), base._engine("franka")
    got, _ = both(a, b, [img], [cam], spec, q=base._q0(), what="self-filter")
    assert 0 < got[0] < got[1], "the filter drops some candidates and keeps some"
    got_t, _ = both(a, b, [img], [cam], spec, q=base._q0(), track=track_of(2, 0.1), what="self-filter, tracked")
    assert got_t[:2] == got
    a.close()
    b.close()


# ---- 5. where the images live -------------------------------------------------------------------------------------------------------
def test_host_and_device_images_and_a_sliced_view(pair):
    """host numpy; device int16 (the uint16 bits) and float32 tensors; a device view t[:, 1:], whose base is an odd element offset into
    its allocation and whose pitch is not its width: the dword and 16-byte loads of a lane's run are not available, the short ones are"""
    e, ref = pair
    dev = f"cuda:{e.device}"
    spec = spec_of(**BOX, max_spheres=8192)
    cam_u, cam_f = camera(67, 49, U16, seed=4), camera(67, 49, FLT, seed=5)
    img_u, img_f = random_image(6, cam_u), random_image(7, cam_f)
    want_u, _ = both(e, ref, [img_u], [cam_u], spec, what="host u16")
    t16 = torch.from_numpy(img_u.view(np.int16)).to(dev)
    assert both(e, ref, [img_u], [cam_u], spec, what="device int16", device_images=[t16])[0] == want_u
    if hasattr(torch, "uint16"):
        assert both(e, ref, [img_u], [cam_u], spec, what="device uint16", device_images=[t16.view(torch.uint16)])[0] == want_u
    both(e, ref, [img_f], [cam_f], spec, what="device float32", device_images=[torch.from_numpy(img_f).to(dev)])
    for img, cam in ((img_u, cam_u), (img_f, cam_f)):
        wide = np.zeros((49, 68), img.dtype)
        wide[:, 1:] = img
        t = torch.from_numpy(wide.view(np.int16) if img.dtype == np.uint16 else wide).to(dev)
        view = t[:, 1:]
        assert view.stride(0) == 68 and view.data_ptr() % (2 * img.itemsize) != 0
        both(e, ref, [img], [cam], spec, what=f"device view {img.dtype}", device_images=[view])
    both(e, ref, [img_u, img_f], [cam_u, cam_f], spec, what="two device images",
         device_images=[t16, torch.from_numpy(img_f).to(dev)])
    with pytest.raises(ValueError):
        e.set_obstacles_from_depth([t16, img_f], [cam_u, cam_f], spec)      # one on the device, one on the host
    with pytest.raises(ValueError):
        e.set_obstacles_from_depth([t16.t()], [cam_u], spec)                  # not the camera's shape


# ---- 6. a propagate on the scene ----------------------------------------------------------------------------------------------------
def test_propagate_after_the_depth_scene_is_that_after_the_cloud_scene():
    from optimalmodulationds_amd import scenes
    import test_gpu_cloud as cloud_tests
    cams, frames = scene_frames(2)
    spec, track = spec_of(**SCENE_BOX, min_points=2), track_of(2, 0.1)
    N, q = 32, base._q0()
    ctxs = []
    for _ in range(2):
        e = base._engine("franka", N=N, H=3, max_obs=512)
        e.set_ds(scenes.FRANKA_QF)
        e.set_policy_samples(*cloud_tests._samples(N))
        ctxs.append(e)
    a, b = ctxs
    for images in frames:
        got, _ = both(a, b, images, cams, spec, track=track, what="before the propagate")
    assert got[2] > 0 and a.get_obstacle_horizon()[1] == 1
    a.propagate(q)
    b.propagate(q)
    ra, rb = a.get_rollouts(), b.get_rollouts()
    assert set(ra) == set(rb) and len(ra) >= 6
    for name in ra:
        assert np.array_equal(bits(ra[name]), bits(rb[name])), name
    a.close()
    b.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def _code(err):
    return int(str(err.value).split("omds error ")[1].split(":")[0])


def _raw_depth_call(e, spec, cams, addrs, n_cams, track=None, obj=None, on_device=0):
    from optimalmodulationds_amd import _lib as L
    table = (L.OmdsDepthCamera * max(len(cams), 1))(*cams)
    ptrs = (C.c_void_p * max(len(addrs), 1))(*addrs)
    return e.lib.omds_set_obstacles_from_depth(e.h, C.byref(spec), None if track is None else C.byref(track), None if obj is None else C.byref(obj),
                                               table, ptrs, n_cams, on_device, None, None, None, None, None, None)


def test_eight_cameras_are_taken(pair):
    tiny = [dc.cam_of(1, 1, 60.0, 60.0, 0.0, 0.0, dc.pose_of(np.eye(3), (0.1 * i, 0, 0))) for i in range(8)]
    one = [np.array([[1000 + 100 * i]], np.uint16) for i in range(8)]
    got, n_valid = both(*pair, one, tiny, spec_of((-1, -1, 0), 0.05, (40, 40, 40)), what="eight cameras")
    assert n_valid == 8 and got == (8, 8)


def test_refusals_leave_scene_frame_and_table_alone(pair):
    """every refusal, then the next frame: scene and velocities stay after each refused call, and the objects call that follows gives
    what it gives on a context that never saw them (the stored record frame and component table were left alone)"""
    from optimalmodulationds_amd import _lib as L
    cams, frames = scene_frames(2)
    spec, track, obj = spec_of(**SCENE_BOX, min_points=2), track_of(2, 0.1), obj_of(1, 4)
    e, ref = pair
    both(e, ref, frames[0], cams, spec, track=track, obj=obj, what="frame 0")
    scene, (motion, have) = e.get_obstacles().copy(), e.get_obstacle_motion()

    def refused(what, code=ERR_INVALID_ARG, **kw):
        with pytest.raises(L.OmdsError) as err:
            e.set_obstacles_from_depth(**kw)
        assert _code(err) == code, what
        assert np.array_equal(bits(e.get_obstacles()), bits(scene)), what
        m, h = e.get_obstacle_motion()
        assert h == have and np.array_equal(bits(m), bits(motion)), what
        return err

    small = spec_of(**SCENE_BOX, min_points=2, max_spheres=50)
    for kw in (dict(), dict(track=track), dict(track=track, obj=obj)):
        err = refused("more occupied cells than max_spheres", images=frames[1], cams=cams, spec=small, **kw)
        assert err.value.n_occupied > 100
    refused("no camera", images=[], cams=[], spec=spec, track=track)
    tiny, one = dc.cam_of(1, 1, 60.0, 60.0, 0.0, 0.0), np.array([[1000]], np.uint16)
    refused("nine cameras", images=[one] * 9, cams=[tiny] * 9, spec=spec, track=track)
    assert b"n_cams" in e.lib.omds_last_error(e.h)
    refused("a null image", images=[frames[1][0], None], cams=cams, spec=spec, track=track)
    refused("a bad camera", images=frames[1], cams=[cams[0], dc.cam_of(64, 48, 0.0, 60.0, 31.5, 23.5)], spec=spec, track=track)
    refused("an object spec without a track spec", images=frames[1], cams=cams, spec=spec, obj=obj)
    refused("a bad track spec", images=frames[1], cams=cams, spec=spec, track=track_of(9, 0.1))
    refused("a bad grid", images=frames[1], cams=cams, spec=spec_of((0, 0, 0), 0.0, (4, 4, 4)), track=track)
    # more than 2^24 visited pixels, by the shapes alone: eight cameras of 2048 x 1025 over one element -- refused before anything is read
    huge = [dc.cam_of(2048, 1025, 60.0, 60.0, 0.0, 0.0)] * 8
    assert 8 * 2048 * 1025 > 2 ** 24 >= 8 * 2048 * 1024
    assert _raw_depth_call(e, spec, huge, [one.ctypes.data] * 8, 8, track=track, obj=obj) == ERR_INVALID_ARG
    assert b"16 777 216" in e.lib.omds_last_error(e.h)
    assert np.array_equal(bits(e.get_obstacles()), bits(scene)) and e.get_obstacle_motion()[1] == have
    assert _raw_depth_call(e, spec, huge, [one.ctypes.data] * 8, 8, track=track, obj=obj, on_device=1) == ERR_INVALID_ARG
    # the next frame is what it is without the refused calls
    got, _ = both(e, ref, frames[1], cams, spec, track=track, obj=obj, what="frame 1 after the refusals")
    assert got[2] > 0 and got[4] >= 1 and e.get_obstacle_motion()[1]


# ---- 8. the facade ------------------------------------------------------------------------------------------------------------------
def test_facade_updates_the_scene_from_depth_images():
    """MPPI.update_obstacles_from_depth takes the keyword arguments of update_obstacles_from_cloud, returns what it returns on the points
    of the images and sets the same attributes"""
    import inspect
    from helpers import weights_path
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    keywords = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.default is not inspect.Parameter.empty]
    assert keywords(MPPI.update_obstacles_from_depth) == keywords(MPPI.update_obstacles_from_cloud)
    assert [k for k, _ in keywords(MPPI.update_obstacles_from_depth)] == ["radius", "self_margin", "min_points", "max_spheres", "dt_frame", "reach",
                                                                         "still", "moving_frame", "objects", "link", "min_cells"]
    cams, frames = scene_frames(2)
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    a, b = (MPPI(torch.tensor(base._q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 3, 32, [LinDS(q_f)], dh[:, 2], nn_model, base.K)
            for _ in range(2))
    lo, hi = (0.0, -1.0, 0.0), (1.4, 1.0, 1.2)
    for kw in (dict(), dict(dt_frame=0.1), dict(dt_frame=0.1, objects=True), dict(dt_frame=0.1, objects=True, self_margin=0.03, moving_frame=True)):
        for images in frames:
            got = a.update_obstacles_from_depth(images, cams, 0.05, lo, hi, min_points=2, **kw)
            want = b.update_obstacles_from_cloud(points_of(images, cams)[0], 0.05, lo, hi, min_points=2, **kw)
            assert got == want and a.n_obs == b.n_obs and np.array_equal(bits(a.obs.numpy()), bits(b.obs.numpy())), kw
            assert (a.cloud_matched, a.cloud_objects, a.cloud_objects_matched) == (b.cloud_matched, b.cloud_objects, b.cloud_objects_matched), kw
            assert (a.obs_velocities is None) == (b.obs_velocities is None), kw
            if a.obs_velocities is not None:
                assert np.array_equal(bits(a.obs_velocities.numpy()), bits(b.obs_velocities.numpy())), kw
    assert a.cloud_matched > 0 and a.obs_velocities is not None and a._engine.get_obstacle_frame()[0] is True
    assert np.isfinite(a.propagate()[0].numpy()).all()
