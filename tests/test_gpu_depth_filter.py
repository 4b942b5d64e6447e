"""The depth filter on the device (include/omds.h: omds_set_depth_filter; csrc/depth_kernels.hip: k_depth_count_filt,
k_depth_count_filt_rec in place of the counting kernels of the depth routes).  The reference side of every comparison is a SECOND
Engine that is given engine.depth_points(image, cam, filter=...) of every image, concatenated in camera order, through the cloud
calls -- for the memory route the host definition omds_depth_scene_memory_filtered iterated; the host definition itself is checked
in tests/test_depth_filter_cpu.py.  Everything is array for array and count for count, omds_get_depth_filter_stats included.

The kernel's mapping: blockIdx.y is the camera; a workgroup owns a tile of 32 x 32 visited pixels and stages it with a halo of
``radius`` into LDS; a lane takes a run of 4 pixels of one tile row.  So the shapes here are a tile and one pixel more or less in
each direction, and images that are no multiple of anything.  The images are a band of depths in which neighbours agree by chance:
every test asserts on the host that the filter keeps between 0.2 and 0.8 of the returns, so that a pixel's verdict depends on the
values around it -- across a tile seam on the halo staged from the neighbouring tile, at the border on the NaNs outside the image."""
import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import depth_cases as dc
import depth_filter_cases as fc
import test_gpu_cloud_flow as base
import test_gpu_depth as gd
from cloud_cases import F32, spec_of
from cloud_flow_cases import track_of
from cloud_object_cases import obj_of
from depth_cases import FLT, U16

pytestmark = pytest.mark.gpu

bits = base.bits
ERR_INVALID_ARG = 1
# tolerance 0.0071 + 0.0013 z on a band of 64 mm: a neighbour supports with probability about 1 / 4; min_support about the mean
BAND = {1: dict(radius=1, min_support=2, edge_abs=0.0071, edge_rel=0.0013), 2: dict(radius=2, min_support=6, edge_abs=0.0071, edge_rel=0.0013),
        3: dict(radius=3, min_support=12, edge_abs=0.0071, edge_rel=0.0013)}


# ... and on the 3 x 2 image, whose pixels have at most 5 neighbours: 4 of 6, 3 of 6 and 3 of 5 returns stay at radius 1, 2, 3
TINY_SUPPORT = {1: 1, 2: 1, 3: 2}


def filtered_points(images, cams, filt):
    """(points of all images in camera order, pixels kept, pixels rejected) of the host definition"""
    from optimalmodulationds_amd.engine import depth_points
    got = [depth_points(im, c, filter=filt) for im, c in zip(images, cams)]
    return np.concatenate([g[0] for g in got]), sum(g[1] for g in got), sum(g[2] for g in got)


def both(e_depth, e_cloud, images, cams, spec, filt, q=None, track=None, obj=None, what="", device_images=None, band=True):
    """the depth call under the filter on one context, the cloud call on the filtered points of the images on the other: same counts,
    same state, and the filter's statistics are the host's"""
    pts, kept, rejected = filtered_points(images, cams, filt)
    if band:
        assert 0.2 <= kept / (kept + rejected) <= 0.8, f"{what}: the filter keeps {kept} of {kept + rejected} returns: the images do not test it"
    e_depth.set_depth_filter(filt)
    got = e_depth.set_obstacles_from_depth(images if device_images is None else device_images, cams, spec, q, track, obj)
    want = gd.cloud_call(e_cloud, pts, spec, q, track, obj)
    assert got == want, (what, got, want)
    assert e_depth.depth_filter_stats() == (kept, rejected), (what, e_depth.depth_filter_stats(), kept, rejected)
    gd.assert_same_state(e_depth, e_cloud, what, obj is not None)
    return got, kept, rejected


def band_image(seed, cam):
    if cam.format == U16:
        return fc.band_u16(seed, cam.width, cam.height)
    return fc.band_f32(seed, cam.width, cam.height)


@pytest.fixture
def pair():
    engines = [base._engine(None), base._engine(None)]
    yield engines
    for e in engines:
        e.close()


BOX = gd.BOX


# ---- 1. tile seams and halos -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(37, 29), (33, 33), (31, 31), (3, 2), (70, 65)])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_tile_seams_and_halos(pair, width, height, radius):
    """37 x 29; one pixel more than a tile in each direction (four tiles, three of them a sliver); one pixel less; 3 x 2 (smaller than
    every window); 70 x 65 (three tiles by three: a tile with neighbours on every side)"""
    cam = gd.camera(width, height, U16, seed=radius)
    img = band_image(10 * radius + width, cam)
    spec = spec_of(**BOX, max_spheres=8192)
    filt = fc.spec_of(**(dict(BAND[radius], min_support=TINY_SUPPORT[radius]) if width * height < 50 else BAND[radius]))
    got, kept, rejected = both(*pair, [img], [cam], spec, filt, what=f"{width}x{height} r{radius}")
    assert got[0] > 0 and rejected > 0


@pytest.mark.parametrize("case", ["one-cell", "two-cell", "speckle"])
@pytest.mark.parametrize("tracked", [False, True])
def test_contention_extremes_through_the_filtered_merge(pair, case, tracked):
    """the worst cases of the merge behind the filter (tests/test_gpu_depth.py's images): every surviving pixel in one cell, counted
    through min_points; pixels alternating between two depths a metre apart like a checkerboard, where a pixel's four diagonal
    neighbours support it and the pixels of the border, with fewer, are rejected; and more cells in a wave than it has rounds"""
    if case == "speckle":
        cam, img = gd.speckle()
        spec = spec_of((-1.5, -1.5, 0.5), 0.05, (60, 60, 40), min_points=2, max_spheres=8192)
    else:
        cam, img = gd.narrow_camera(), gd.one_cell_image() if case == "one-cell" else gd.two_cell_image()
        spec = spec_of(**gd.CELL_BOX, min_points=67 * 49 if case == "one-cell" else 47 * 65 // 2)
    filt = fc.spec_of(1, 3 if case == "one-cell" else 4, 0.01, 0.0)
    got, kept, rejected = both(*pair, [img], [cam], spec, filt, track=track_of(1, 0.1) if tracked else None, what=case, band=False)
    if case == "one-cell":
        assert (kept, rejected) == (67 * 49, 0) and got[:2] == (1, 1), "a corner has 3 supporters: nothing is rejected, one cell holds all"
    else:
        assert kept == 65 * 47 and rejected == 67 * 49 - kept and got[0] >= 2, "the interior stays, the border goes"


# ---- 2. strides --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [2, 3])
@pytest.mark.parametrize("fmt", [U16, FLT])
def test_strides(pair, step, fmt):
    """135 x 99 at step 2 (68 x 50 visited) and step 3 (45 x 33): the width is no multiple of step x 4, the visited grid has tile seams in
    both directions, and the window's neighbours are step elements apart"""
    cam = gd.camera(135, 99, fmt, step, seed=step)
    both(*pair, [band_image(20 + step, cam)], [cam], spec_of(**BOX, max_spheres=8192), fc.spec_of(**BAND[2]), what=f"step {step}")


# ---- 3. where the images live ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [U16, FLT])
def test_host_pitch_and_device_views(pair, fmt):
    """a host image with pitch > width; the same on the device; a device view t[:, 3:-2] of a wider tensor, whose first element is at an
    odd element offset (no row of it starts on a 4-byte / 16-byte boundary in step with the others) and whose pitch is odd"""
    e, ref = pair
    dev = f"cuda:{e.device}"
    cam = gd.camera(70, 37, fmt, seed=7)
    img = band_image(31, cam)
    spec, filt = spec_of(**BOX, max_spheres=8192), fc.spec_of(**BAND[3])
    want, kept, rejected = both(e, ref, [img], [cam], spec, filt, what="host")
    wide = np.zeros((37, 75), img.dtype)
    wide[:, 3:-2] = img
    host_view = wide[:, 3:-2]
    assert both(e, ref, [host_view], [cam], spec, filt, what="host view, pitch 75")[0] == want
    as_torch = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
    assert both(e, ref, [img], [cam], spec, filt, what="device", device_images=[as_torch(img)])[0] == want
    view = as_torch(wide)[:, 3:-2]
    assert view.stride(0) == 75 and view.data_ptr() % (2 * img.itemsize) != 0 and not view.is_contiguous()
    assert both(e, ref, [img], [cam], spec, filt, what="device view", device_images=[view])[0] == want
    assert e.depth_filter_stats() == (kept, rejected)


# ---- 4. F32 elements ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 3])
def test_f32_image_with_nan_and_inf_elements(pair, radius):
    cam = gd.camera(67, 49, FLT, seed=8)
    img = band_image(41, cam)
    assert np.isnan(img).sum() > 100 and np.isposinf(img).sum() > 20 and np.isneginf(img).sum() > 20
    both(*pair, [img], [cam], spec_of(**BOX, max_spheres=8192), fc.spec_of(**BAND[radius]), what=f"f32 r{radius}")


# ---- 5. several cameras ------------------------------------------------------------------------------------------------------------------
def test_two_cameras_of_different_size_format_and_step(pair):
    """U16 70 x 37 at step 1 and F32 99 x 80 at step 2 with pitch 104 in one call: blockIdx.y picks the camera, and the smaller camera's
    workgroups run out of tiles first; then the cameras the other way round, and the tracked kernel on the same images"""
    cams = [gd.camera(70, 37, U16, seed=11), gd.camera(99, 80, FLT, step=2, seed=12, pitch=104)]
    flat = np.full(79 * 104 + 99, np.nan, F32)
    view = np.lib.stride_tricks.as_strided(flat, (80, 99), (416, 4))
    view[:] = band_image(52, cams[1])
    images = [band_image(51, cams[0]), view]
    spec, filt = spec_of(**BOX, max_spheres=8192), fc.spec_of(**BAND[2])
    got, kept, rejected = both(*pair, images, cams, spec, filt, what="two cameras")
    again, _, _ = both(*pair, images[::-1], cams[::-1], spec, filt, what="two cameras, swapped")
    assert again == got and got[0] > 500
    tracked, _, _ = both(*pair, images, cams, spec, filt, track=track_of(2, 0.1), what="two cameras, tracked")
    assert tracked[:2] == got


# ---- 6. the routes, through the facade ---------------------------------------------------------------------------------------------------
ROUTE_FILTER = dict(radius=1, min_support=6, edge_abs=0.015, edge_rel=0.0)      # keeps about half of the rendered frames below


def _facades(n):
    from helpers import weights_path
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    return [MPPI(torch.tensor(base._q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 3, 32, [LinDS(q_f)], dh[:, 2], nn_model, base.K)
            for _ in range(n)]


@pytest.mark.parametrize("on_device", [False, True])
def test_routes_through_the_facade(on_device):
    """plain, dt_frame=, objects=True and memory=, each with filter= on the two rendered frames of tests/test_gpu_depth.py (a sphere
    moving in front of a wall, two cameras): what update_obstacles_from_cloud gives on the filtered points; for memory=, the host
    definition iterated.  The keyword is in force for its call only"""
    from optimalmodulationds_amd.engine import depth_scene_memory, scene_memory_spec
    cams, frames = gd.scene_frames(2)
    a, b = _facades(2)
    dev = f"cuda:{a._engine.device}"
    lo, hi = (0.0, -1.0, 0.0), (1.4, 1.0, 1.2)
    src = lambda images: [torch.from_numpy(im.view(np.int16)).to(dev) for im in images] if on_device else images
    for kw in (dict(), dict(dt_frame=0.1), dict(dt_frame=0.1, objects=True)):
        for images in frames:
            pts, kept, rejected = filtered_points(images, cams, ROUTE_FILTER)
            assert 0.2 <= kept / (kept + rejected) <= 0.8
            got = a.update_obstacles_from_depth(src(images), cams, 0.05, lo, hi, min_points=2, filter=ROUTE_FILTER, **kw)
            want = b.update_obstacles_from_cloud(pts, 0.05, lo, hi, min_points=2, **kw)
            assert got == want and a.n_obs == b.n_obs and np.array_equal(bits(a.obs.numpy()), bits(b.obs.numpy())), kw
            assert a.depth_filter_stats == (kept, rejected), kw
            assert (a.cloud_matched, a.cloud_objects, a.cloud_objects_matched) == (b.cloud_matched, b.cloud_objects, b.cloud_objects_matched), kw
            assert (a.obs_velocities is None) == (b.obs_velocities is None), kw
            if a.obs_velocities is not None:
                assert np.array_equal(bits(a.obs_velocities.numpy()), bits(b.obs_velocities.numpy())), kw
        assert not kw or a.cloud_matched > 0, kw
        unfiltered = a.update_obstacles_from_depth(src(frames[1]), cams, 0.05, lo, hi, min_points=2)      # no keyword: no filter
        assert unfiltered[0] > got[0] and a._engine.depth_filter_stats() == (0, 0), kw
        a._engine.cloud_track_reset()
        b._engine.cloud_track_reset()
    from optimalmodulationds_amd.engine import cloud_spec
    dims = np.maximum(np.ceil((np.float32(hi) - np.float32(lo)) / np.float32(0.05) - 1e-4), 1).astype(np.int32)
    spec, mem = cloud_spec(np.float32(lo), 0.05, dims, 0.0, 2, 4096, 0.0), scene_memory_spec(3)
    m = None
    for images in (frames[0], [np.zeros_like(im) for im in frames[0]], frames[1]):
        m, want_counts = depth_scene_memory(images, cams, spec, mem, m, filter=ROUTE_FILTER)
        n, counts = a.update_obstacles_from_depth(src(images), cams, 0.05, lo, hi, min_points=2, memory=mem, filter=ROUTE_FILTER)
        age, words = a._engine.get_scene_memory(grid=True)
        assert counts == want_counts + (0,) and np.array_equal(words, m) and n == int((m != 0).sum())
        assert np.array_equal(a.obs_age.numpy()[:n], m[m != 0].astype(np.int64) - 1)
        assert a.depth_filter_stats == filtered_points(images, cams, ROUTE_FILTER)[1:]
    assert counts[1] > 5 and counts[0] > 100, "the last frame sees cells and remembers occluded ones"
    # a filter the engine had before the call is the engine's again after it (a dict is taken by the engine too)
    a._engine.set_depth_filter(dict(BAND[1]))
    a.update_obstacles_from_depth(src(frames[1]), cams, 0.05, lo, hi, min_points=2, filter=ROUTE_FILTER)
    assert a.depth_filter_stats == filtered_points(frames[1], cams, ROUTE_FILTER)[1:] and bytes(a._engine.depth_filter) == bytes(fc.spec_of(**BAND[1]))
    a.update_obstacles_from_depth(src(frames[1]), cams, 0.05, lo, hi, min_points=2)
    assert a._engine.depth_filter_stats() == filtered_points(frames[1], cams, BAND[1])[1:]


# ---- 7. filter off is today ------------------------------------------------------------------------------------------------------------
def test_filter_off_is_the_unfiltered_call(pair):
    """after a filtered call, omds_set_depth_filter(ctx, NULL): every output of the depth call -- plain, tracked and objects -- is that
    of a context that never had a filter, and the statistics are 0, 0"""
    e, fresh = pair
    cams, frames = gd.scene_frames(2)
    spec, track, obj = spec_of(**gd.SCENE_BOX, min_points=2), track_of(2, 0.1), obj_of(1, 4)
    e.set_depth_filter(fc.spec_of(**ROUTE_FILTER))
    e.set_obstacles_from_depth(frames[0], cams, spec, track=track, obj=obj)
    assert e.depth_filter_stats()[1] > 0
    e.cloud_track_reset()
    e.set_depth_filter(None)
    for kw in (dict(), dict(track=track), dict(track=track, obj=obj)):
        for images in frames:
            assert e.set_obstacles_from_depth(images, cams, spec, **kw) == fresh.set_obstacles_from_depth(images, cams, spec, **kw), kw
            gd.assert_same_state(e, fresh, str(kw), "obj" in kw)
            assert e.depth_filter_stats() == (0, 0)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_a_refused_spec_leaves_the_filter_in_force(pair):
    from optimalmodulationds_amd import _lib as L
    e, ref = pair
    cam = gd.camera(37, 29, U16, seed=1)
    img = band_image(61, cam)
    spec, filt = spec_of(**BOX, max_spheres=8192), fc.spec_of(**BAND[1])
    want, kept, rejected = both(e, ref, [img], [cam], spec, filt, what="before")
    for bad in (dict(radius=0), dict(radius=4), dict(min_support=0), dict(min_support=9), dict(edge_abs=-1.0), dict(edge_abs=np.nan), dict(edge_rel=np.inf)):
        with pytest.raises(L.OmdsError) as err:
            e.set_depth_filter(fc.spec_of(**dict(BAND[1], **bad)))
        assert "omds error 1" in str(err.value) and "depth filter" in str(err.value), bad
        assert e.set_obstacles_from_depth([img], [cam], spec) == want and e.depth_filter_stats() == (kept, rejected), bad
    gd.assert_same_state(e, ref, "after the refused specs")


def test_too_many_cells_under_a_filter_leaves_scene_frame_and_memory_alone(pair):
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.engine import scene_memory_spec
    e, ref = pair
    cams, frames = gd.scene_frames(2)
    spec, track, mem = spec_of(**gd.SCENE_BOX, min_points=2), track_of(2, 0.1), scene_memory_spec(3)
    small = spec_of(**gd.SCENE_BOX, min_points=2, max_spheres=50)
    filt = fc.spec_of(**ROUTE_FILTER)
    e.set_depth_filter(filt)
    e.set_obstacles_from_depth_memory(frames[0], cams, spec, mem)
    words = e.get_scene_memory(grid=True)[1].copy()
    both(e, ref, frames[0], cams, spec, filt, track=track, what="frame 0")
    scene = e.get_obstacles().copy()
    _, kept, rejected = filtered_points(frames[1], cams, filt)
    for call in (lambda: e.set_obstacles_from_depth(frames[1], cams, small), lambda: e.set_obstacles_from_depth(frames[1], cams, small, track=track),
                 lambda: e.set_obstacles_from_depth_memory(frames[1], cams, small, mem)):
        with pytest.raises(L.OmdsError) as err:
            call()
        assert "omds error 1" in str(err.value) and err.value.n_occupied > 50
        assert np.array_equal(bits(e.get_obstacles()), bits(scene)) and np.array_equal(e.get_scene_memory(grid=True)[1], words)
        assert e.depth_filter_stats() == (kept, rejected), "the counting pass ran: its statistics are the refused call's"
    got, _, _ = both(e, ref, frames[1], cams, spec, filt, track=track, what="frame 1 after the refusals")
    assert got[2] > 0, "the stored frame is frame 0's: frame 1 matches against it"
