"""The lens of a depth camera on the device (include/omds.h: omds_set_depth_lenses; csrc/depth_kernels.hip: k_depth_rays, the lens
forms of the counting kernels; csrc/scene_memory_kernels.hip: that of k_scene_memory).  The reference side of every comparison is the host definition, which
tests/test_depth_lens_cpu.py checks: a SECOND Engine is given engine.depth_points(image, cam, filter=, lens=) of every image,
concatenated in camera order, through the cloud calls; for the memory routes the host definitions omds_depth_scene_memory_lens and
omds_depth_scene_memory_flow_lens iterated.  Everything is array for array and count for count.

The kernels' mapping: a lane of the counting pass takes a run of 4 visited pixels of a row and loads their four rays as two 16-byte
pairs where a pair starts at an even table entry inside the row, else entry by entry; the last run of the last row ends the table.
So the shapes (tests/depth_lens_cases.py) have widths that are no multiple of 4 or of the step, odd visited widths (every second row
starts at an odd entry), nu < 4, nv = 1 and 1 x 1, both formats, a pitch, and two cameras of which only the second has a lens."""
import numpy as np
import pytest
import torch      # before the library is loaded: torch brings its own HIP runtime and has to be the first to start it

import depth_cases as dc
import depth_filter_cases as fc
import depth_lens_cases as lc
import lens_ref as lr
import scene_memory_flow_cases as mf
import test_gpu_cloud_flow as base
import test_gpu_depth as gd
from cloud_cases import F32, spec_of
from cloud_flow_cases import track_of
from cloud_object_cases import obj_of
from depth_cases import FLT, U16

pytestmark = pytest.mark.gpu

bits = base.bits
FILTER = dict(radius=1, min_support=3, edge_abs=0.02, edge_rel=0.01)
SPEC = dict(lc.BOX, max_spheres=8192)


@pytest.fixture
def pair():
    engines = [base._engine(None), base._engine(None)]
    yield engines
    for e in engines:
        e.close()


def lens_points(images, cams, lenses, filt=None):
    """(points of all images in camera order, pixels kept, pixels rejected) of the host definition"""
    from optimalmodulationds_amd.engine import depth_points
    pts, kept, rejected = [], 0, 0
    for im, c, l in zip(images, cams, lenses):
        got = depth_points(im, c, filter=filt, lens=l)
        pts.append(got[0])
        kept += got[1]
        rejected += got[2] if len(got) > 2 else 0
    return np.concatenate(pts), kept, rejected


def both(e, ref, images, cams, lenses, spec, filt=None, track=None, obj=None, what="", given=None):
    """the depth call under the lenses (and the filter) on one context, the cloud call on the host's lens points on the other"""
    pts, kept, rejected = lens_points(images, cams, lenses, filt)
    e.set_depth_lenses(lenses)
    e.set_depth_filter(filt)
    got = e.set_obstacles_from_depth(images if given is None else given, cams, spec, None, track, obj)
    want = gd.cloud_call(ref, pts, spec, None, track, obj)
    assert got == want, (what, got, want)
    assert e.depth_filter_stats() == ((kept, rejected) if filt is not None else (0, 0)), (what, e.depth_filter_stats(), kept, rejected)
    gd.assert_same_state(e, ref, what, obj is not None)
    return got


def case(lens_name, shape_name, t=0.0):
    _, k, kw = next(l for l in lc.LENSES if l[0] == lens_name)
    cam = lc.shape_camera(shape_name)
    return cam, lc.lens_of(k, **kw), lc.sphere_scene(cam, lc.lens_of(k), t)


def on_device(e, img):
    return torch.from_numpy(np.ascontiguousarray(img).view(np.int16) if img.dtype == np.uint16 else np.ascontiguousarray(img)).to(f"cuda:{e.device}")


# ---- 1. the table --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_name", ["plumb", "nfov", "partial"])
@pytest.mark.parametrize("shape_name", [s[0] for s in lc.SHAPES])
def test_table_is_the_host_rays_and_the_call_the_cloud_call(pair, lens_name, shape_name):
    """k_depth_rays against omds_depth_lens_rays: every entry, r2_max and the pixels without a ray; the plain and the tracked call on
    the table against the cloud call on the lens points; a changed pose uses the same table"""
    from optimalmodulationds_amd.engine import depth_lens_rays
    e, ref = pair
    cam, lens, img = case(lens_name, shape_name)
    spec = spec_of(**SPEC)
    got = both(e, ref, [img], [cam], [lens], spec, what="plain")
    want_ab, want_r2, want_bad = depth_lens_rays(cam, lens)
    ab, r2_max, bad = e.depth_lens_table(0)
    assert ab.shape == want_ab.shape and np.array_equal(bits(ab), bits(want_ab)) and bits(F32(r2_max)) == bits(F32(want_r2)) and bad == want_bad
    assert e.depth_lens_table(1)[0].shape == (0, 2)
    moved = lc.shape_camera(shape_name)
    moved.pose[:] = list(dc.pose_of(dc.LOOK_ALONG_X, (0.05, -0.1, 0.45)).reshape(-1))
    both(e, ref, [img], [moved], [lens], spec, track=track_of(2, 0.1), what="moved, tracked")
    both(e, ref, [lc.sphere_scene(cam, lens, 0.05)], [moved], [lens], spec, track=track_of(2, 0.1), what="moved, tracked, frame 2")
    again = e.depth_lens_table(0)
    assert np.array_equal(bits(again[0]), bits(want_ab)) and again[1:] == (r2_max, bad)
    if img.size > 100 and lens_name != "partial":
        assert got[0] > 20


# ---- 2. the routes ---------------------------------------------------------------------------------------------------------------------------
def two_cameras(t=0.0):
    """an F32 camera at step 2 without a lens and a U16 camera with the plumb-bob lens, side by side"""
    cam0 = lc.camera(61, 47, FLT, 2, pose=dc.pose_of(dc.LOOK_ALONG_X, (0.0, 0.3, 0.4)))
    cam1 = lc.camera(67, 50, U16)
    lens = lc.lens_of(lc.PLUMB)
    return [cam0, cam1], [None, lens], [lc.sphere_scene(cam0, lc.ZERO, t), lc.sphere_scene(cam1, lens, t)]


@pytest.mark.parametrize("where", ["host", "device", "view"])
@pytest.mark.parametrize("filtered", [False, True])
def test_routes_equal_the_cloud_call_on_the_lens_points(pair, filtered, where):
    """plain, tracked and objects, with and without the depth filter, from host images, device images and strided device views, two
    frames each; only the second camera has a lens"""
    e, ref = pair
    spec, filt = spec_of(**SPEC), fc.spec_of(**FILTER) if filtered else None
    frames = [two_cameras(t) for t in (0.0, 0.05)]

    def src(images):
        if where == "host":
            return None
        if where == "device":
            return [on_device(e, im) for im in images]
        views = []
        for im in images:
            wide = np.zeros((im.shape[0], im.shape[1] + 5), im.dtype)
            wide[:, 3:-2] = im
            views.append(on_device(e, wide)[:, 3:-2])
        return views

    for kw in (dict(), dict(track=track_of(2, 0.1)), dict(track=track_of(2, 0.1), obj=obj_of(1, 4))):
        for cams, lenses, images in frames:
            got = both(e, ref, images, cams, lenses, spec, filt, what=f"{kw} {where}", given=src(images), **kw)
        assert got[0] > 100 and (not kw or got[2] > 0), (kw, got)
        e.cloud_track_reset()
        ref.cloud_track_reset()


# ---- 3. the memory routes --------------------------------------------------------------------------------------------------------------------
def memory_frames(cam, lens):
    wall = [((1.0, 0.0, 0.0), lc.WALL_X)]
    slab = lc.as_image(cam, lr.render(cam, lens, planes=[((1.0, 0.0, 0.0), 0.85)]))       # a surface across the whole image ...
    blind = np.zeros_like(lc.as_image(cam, lr.render(cam, lens, planes=wall)))          # ... then nothing ...
    return [slab, blind, lc.as_image(cam, lr.render(cam, lens, planes=wall))]             # ... then the wall behind it: seen through


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("fmt,step", [(U16, 1), (FLT, 2)])
def test_memory_route_is_the_definition_iterated(pair, fmt, step, filtered):
    from optimalmodulationds_amd.engine import depth_scene_memory, scene_memory_spec
    e, _ = pair
    cam, lens = lc.camera(64, 48, fmt, step), lc.lens_of(lc.PLUMB)
    cam0 = lc.camera(61, 47, FLT, 2, pose=dc.pose_of(dc.LOOK_ALONG_X, (0.0, 0.3, 0.4)))
    spec, mem, filt = spec_of(**SPEC), scene_memory_spec(5, 0.0, 1), FILTER if filtered else None
    e.set_depth_lenses([None, lens])
    e.set_depth_filter(filt)
    m, cleared = None, 0
    for im0, im1 in zip(memory_frames(cam0, lc.ZERO), memory_frames(cam, lens)):
        m, want_counts = depth_scene_memory([im0, im1], [cam0, cam], spec, mem, m, filter=filt, lenses=[None, lens])
        n, counts = e.set_obstacles_from_depth_memory([im0, im1], [cam0, cam], spec, mem)
        age, words = e.get_scene_memory(grid=True)
        assert counts == want_counts + (0,) and np.array_equal(words, m) and n == int((m != 0).sum()), (counts, want_counts)
        assert np.array_equal(age[:n], m[m != 0].astype(np.int64) - 1)
        cleared += counts[2]
    plain = depth_scene_memory([im0, im1], [cam0, cam], spec, mem, None, filter=filt)
    assert cleared > 100 and counts[0] > 100, "the wall is seen and the slab in front of it is cleared"
    assert not np.array_equal(plain[0], depth_scene_memory([im0, im1], [cam0, cam], spec, mem, None, filter=filt, lenses=[None, lens])[0])


@pytest.mark.parametrize("objects", [False, True])
def test_memory_tracked_route_is_the_flow_definition(pair, objects):
    from optimalmodulationds_amd.engine import depth_scene_memory_flow, scene_memory_spec
    e, _ = pair
    spec, mem, track, obj = spec_of(**SPEC), scene_memory_spec(5), track_of(2, 0.1), obj_of(1, 4) if objects else None
    frames = [two_cameras(t) for t in (0.0, 0.05, 0.1)]
    cams, lenses, _ = frames[0]
    e.set_depth_lenses(lenses)
    m, prev, matched = None, None, 0
    for _, _, images in frames:
        want = depth_scene_memory_flow(images, cams, spec, mem, track, obj, None if prev is None else (prev, cams), m, lenses=lenses, cap=8192)
        n, counts, n_matched, n_objects, n_objects_matched = e.set_obstacles_from_depth_memory_tracked(images, cams, spec, mem, track, obj)
        age, words = e.get_scene_memory(grid=True)
        vel, _ = e.get_obstacle_motion()
        label, flag, _ = e.cloud_objects() if objects else (np.full(e.n_obs, -1, np.int32), np.zeros(e.n_obs, np.int32), 0)
        got = dict(words=words, counts=counts, spheres=e.get_obstacles()[:n], vel=vel[:n], age=age[:n], label=label[:n], object=flag[:n],
                   n_matched=n_matched, n_objects=n_objects, n_objects_matched=n_objects_matched)
        mf.same(got, want, f"objects {objects}")
        m, prev, matched = words, images, matched + max(n_matched, 0)
    assert matched > 0 and counts[0] > 100


# ---- 4. nothing existing changes ---------------------------------------------------------------------------------------------------------------
def test_zero_lens_through_the_table_is_the_pinhole_call(pair):
    e, fresh = pair
    cams, _, images = two_cameras()
    spec, track = spec_of(**SPEC), track_of(2, 0.1)
    zero = lc.lens_of(lc.ZERO)
    e.set_depth_lenses([zero, zero])
    for filt in (None, fc.spec_of(**FILTER)):
        e.set_depth_filter(filt)
        fresh.set_depth_filter(filt)
        for kw in (dict(), dict(track=track)):
            assert e.set_obstacles_from_depth(images, cams, spec, **kw) == fresh.set_obstacles_from_depth(images, cams, spec, **kw), kw
            gd.assert_same_state(e, fresh, str(kw))
            assert e.depth_filter_stats() == fresh.depth_filter_stats()
    assert e.depth_lens_table(0)[0].shape[0] == 31 * 24 and e.depth_lens_table(1)[2] == 0, "the zero lens went through the table"


def test_lenses_off_is_a_context_that_never_had_them(pair):
    from optimalmodulationds_amd.engine import scene_memory_spec
    e, fresh = pair
    cams, lenses, images = two_cameras()
    spec, track, obj, mem = spec_of(**SPEC), track_of(2, 0.1), obj_of(1, 4), scene_memory_spec(5)
    e.set_depth_lenses(lenses)
    e.set_obstacles_from_depth(images, cams, spec, track=track, obj=obj)
    e.set_obstacles_from_depth_memory(images, cams, spec, mem)
    e.cloud_track_reset()
    e.scene_memory_reset()
    e.set_depth_lenses(None)
    assert e.depth_lenses is None
    for t in (0.0, 0.05):
        images = two_cameras(t)[2]
        for kw in (dict(), dict(track=track), dict(track=track, obj=obj)):
            assert e.set_obstacles_from_depth(images, cams, spec, **kw) == fresh.set_obstacles_from_depth(images, cams, spec, **kw), kw
            gd.assert_same_state(e, fresh, str(kw), "obj" in kw)
        assert e.set_obstacles_from_depth_memory(images, cams, spec, mem) == fresh.set_obstacles_from_depth_memory(images, cams, spec, mem)
        assert np.array_equal(e.get_scene_memory(grid=True)[1], fresh.get_scene_memory(grid=True)[1])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_scene_memory_frame_table_and_filters(pair):
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.engine import depth_lens, scene_memory_spec
    e, ref = pair
    spec, small, track, mem = spec_of(**SPEC), spec_of(**dict(SPEC, max_spheres=50)), track_of(2, 0.1), scene_memory_spec(5)
    filt = fc.spec_of(**FILTER)
    (cams, lenses, f0), (_, _, f1) = two_cameras(0.0), two_cameras(0.05)
    e.set_depth_lenses(lenses)
    e.set_depth_filter(filt)
    e.set_obstacles_from_depth_memory(f0, cams, spec, mem)
    words = e.get_scene_memory(grid=True)[1].copy()
    both(e, ref, f0, cams, lenses, spec, filt, track=track, what="frame 0")
    scene, table = e.get_obstacles().copy(), e.depth_lens_table(1)
    for bad in (dict(k1=np.nan), dict(iters=65), dict(max_residual=np.inf)):
        with pytest.raises(L.OmdsError) as err:
            e.set_depth_lenses([None, depth_lens(**bad)])
        assert "omds error 1" in str(err.value) and "depth lens" in str(err.value), bad
    with pytest.raises(L.OmdsError):
        e.set_depth_lenses([None] * 9)
    assert bytes(e.depth_lenses[1]) == bytes(lenses[1]), "a refused list leaves the lenses in force"
    _, kept, rejected = lens_points(f1, cams, lenses, filt)
    for call in (lambda: e.set_obstacles_from_depth(f1, cams, small), lambda: e.set_obstacles_from_depth(f1, cams, small, track=track),
                 lambda: e.set_obstacles_from_depth_memory(f1, cams, small, mem)):
        with pytest.raises(L.OmdsError) as err:
            call()
        assert "omds error 1" in str(err.value) and err.value.n_occupied > 50
        assert np.array_equal(bits(e.get_obstacles()), bits(scene)) and np.array_equal(e.get_scene_memory(grid=True)[1], words)
        after = e.depth_lens_table(1)
        assert np.array_equal(bits(after[0]), bits(table[0])) and after[1:] == table[1:]
        assert e.depth_filter_stats() == (kept, rejected) and bytes(e.depth_filter) == bytes(filt)
    got = both(e, ref, f1, cams, lenses, spec, filt, track=track, what="frame 1 after the refusals")
    assert got[2] > 0, "the stored frame is frame 0's: frame 1 matches against it"


# ---- 6. the contention extremes of the counting pass under a lens ------------------------------------------------------------------------------
def contention_case(name):
    """the three extremes of tests/test_gpu_depth.py (67 x 49 pixels: all in one cell, in two cells, more cells in a wave than the merge
    has rounds) with the plumb-bob lens on the camera, so that k_depth_count_lens / k_depth_count_rec_lens read a ray table.  On the
    narrow camera |a|, |b| <= 3.3e-4: the lens leaves every pixel its ray and its cell, so the originals' thresholds hold"""
    from optimalmodulationds_amd.engine import depth_lens_rays
    lens = lc.lens_of(lc.PLUMB)
    if name == "speckle":
        cam, img = gd.speckle()
        box = dict(origin=(-1.5, -1.5, 0.5), voxel=0.05, dims=(60, 60, 40), max_spheres=8192)
    else:
        cam, img, box = gd.narrow_camera(), gd.one_cell_image() if name == "one-cell" else gd.two_cell_image(), gd.CELL_BOX
    assert depth_lens_rays(cam, lens)[2] == 0, "the host definition gives every pixel of this camera a ray"
    return cam, lens, img, box


@pytest.mark.parametrize("name", ["one-cell", "two-cell", "speckle"])
def test_contention_extremes_under_a_lens(pair, name):
    """the cell counts pinned at n_valid and n_valid + 1 through min_points, as the pinhole tests pin them"""
    e, ref = pair
    cam, lens, img, box = contention_case(name)
    n, near, far = 67 * 49, 1642, 1641           # 3 283 pixels; two cells: the even ones near
    expect = {"one-cell": ((1, 1), (n, 1), (n + 1, 0)), "two-cell": ((1, 2), (far, 2), (near, 1), (near + 1, 0)),
              "speckle": ((1, None), (2, None), (3, None))}[name]
    for min_points, occupied in expect:
        got = both(e, ref, [img], [cam], [lens], spec_of(**box, min_points=min_points), what=f"{name}, min_points {min_points}")
        assert lens_points([img], [cam], [lens])[1] == n
        if occupied is not None:
            assert got == (occupied, occupied)
        else:
            assert got[0] > {1: 300, 2: 300, 3: 100}[min_points]
    assert e.depth_lens_table(0)[0].shape == (n, 2) and e.depth_lens_table(0)[2] == 0


@pytest.mark.parametrize("name", ["one-cell", "two-cell", "speckle"])
def test_contention_extremes_under_a_lens_tracked(pair, name):
    """... through the tracked call; the second frame is the first seen from a camera shifted by (10, -5, 15) mm, less than a cell: the
    velocities come from the sums of the sub-cell offsets and must be the cloud route's bits"""
    e, ref = pair
    cam, lens, img, box = contention_case(name)
    spec = spec_of(**box, min_points=2 if name == "speckle" else 100)
    moved = dc.cam_of(67, 49, cam.fx, cam.fy, 33.0, 24.0, dc.pose_of(np.eye(3), (0.010, -0.005, 0.015)), U16, 0.001, 0.3, 4.0)
    track = track_of(1, 0.1)
    first = both(e, ref, [img], [cam], [lens], spec, track=track, what=name + " frame 1")
    assert first[2] == -1
    second = both(e, ref, [img], [moved], [lens], spec, track=track, what=name + " frame 2")
    vel, have = e.get_obstacle_motion()
    assert have and second[2] > 0.9 * second[0] > 0
    if name != "speckle":
        assert second[2] == second[0] == (1 if name == "one-cell" else 2)
        assert np.allclose(vel[:second[0]], [0.1, -0.05, 0.15], atol=0.05), "about 10, -5, 15 mm in 0.1 s (offsets count in 1/256 cell)"


# ---- 7. through the facade ---------------------------------------------------------------------------------------------------------------------
def test_facade_takes_lenses_for_one_call():
    """update_obstacles_from_depth(lenses=) on plain, dt_frame= and memory=: what update_obstacles_from_cloud gives on the lens points,
    the memory definition iterated; the keyword is in force for its call only"""
    from test_gpu_depth_filter import _facades
    from optimalmodulationds_amd.engine import cloud_spec, depth_scene_memory, scene_memory_spec
    a, b = _facades(2)
    lo, hi = lc.BOX["origin"], tuple(o + d * lc.BOX["voxel"] for o, d in zip(lc.BOX["origin"], lc.BOX["dims"]))
    frames = [two_cameras(t) for t in (0.0, 0.05)]
    cams, lenses, _ = frames[0]
    for kw in (dict(), dict(dt_frame=0.1)):
        for _, _, images in frames:
            pts, _, _ = lens_points(images, cams, lenses)
            got = a.update_obstacles_from_depth(images, cams, 0.1, lo, hi, lenses=lenses, **kw)
            want = b.update_obstacles_from_cloud(pts, 0.1, lo, hi, **kw)
            assert got == want and a.n_obs == b.n_obs and np.array_equal(bits(a.obs.numpy()), bits(b.obs.numpy())), kw
            assert a._engine.depth_lenses is None, "the keyword is in force for its call only"
        assert not kw or (a.cloud_matched > 0 and np.array_equal(bits(a.obs_velocities.numpy()), bits(b.obs_velocities.numpy()))), kw
        pinhole = a.update_obstacles_from_depth(frames[1][2], cams, 0.1, lo, hi)
        assert pinhole != got, "no keyword: no lens"
        a._engine.cloud_track_reset()
        b._engine.cloud_track_reset()
    dims = np.maximum(np.ceil((np.float32(hi) - np.float32(lo)) / np.float32(0.1) - 1e-4), 1).astype(np.int32)
    spec, mem = cloud_spec(np.float32(lo), 0.1, dims, 0.0, 1, 4096, 0.0), scene_memory_spec(3)
    m = None
    for _, _, images in frames:
        m, want_counts = depth_scene_memory(images, cams, spec, mem, m, lenses=lenses)
        n, counts = a.update_obstacles_from_depth(images, cams, 0.1, lo, hi, memory=mem, lenses=lenses)
        assert counts == want_counts + (0,) and np.array_equal(a._engine.get_scene_memory(grid=True)[1], m) and n == int((m != 0).sum())
    a._engine.set_depth_lenses(lenses)
    a.update_obstacles_from_depth(frames[0][2], cams, 0.1, lo, hi, lenses=[None, None])
    assert bytes(a._engine.depth_lenses[1]) == bytes(lenses[1]), "the engine's own lenses are back after the call"
