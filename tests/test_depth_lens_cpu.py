"""The lens of a depth camera on the host (include/omds.h: omds_depth_lens_rays, omds_depth_points_lens, omds_depth_scene_memory_lens,
omds_depth_scene_memory_flow_lens; no context, no GPU) against the float64 model of tests/lens_ref.py, on the cases of
tests/depth_lens_cases.py.

THE BOUNDS.  A valid ray's fp32 residual is at most max_residual pixels by the definition's own test; evaluating the forward model in
fp32 instead of float64 adds a few ulp of fx |ad| <= 40 x 1.3 x 6e-8 = 3e-6 pixels, far below the other max_residual that
2 max_residual allows.  The memory verdicts are compared with the float64 mirror on every tested cell except those whose float64
projection lies within 1e-3 visited pixels of a rounding tie or whose depth lies within 1e-5 m of lim; at most 2 % of the cells may be
left out, which is asserted.

The same cases go through a stand-alone build of the definition under AddressSanitizer + UBSan (tests/depth_lens_host.cpp), whose
output must be the library's bit for bit."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import depth_filter_cases as fc
import depth_lens_cases as lc
import lens_ref as lr
from cloud_cases import spec_of
from cloud_flow_cases import track_of
from depth_cases import F32, F64, FLT, U16
from helpers import sanitized_host_program

ERR_INVALID_ARG = 1
FILTER = dict(radius=1, min_support=3, edge_abs=0.02, edge_rel=0.01)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def visited_grid(cam):
    step = max(int(cam.step), 1)
    nu, nv = -(-int(cam.width) // step), -(-int(cam.height) // step)
    i = np.arange(nu * nv)
    return nu, nv, (i % nu) * step, (i // nu) * step


ALL = [(ln, sn) for ln, _, _ in lc.LENSES for sn, *_ in lc.SHAPES]


def case(lens_name, shape_name):
    _, k, kw = next(l for l in lc.LENSES if l[0] == lens_name)
    cam, lens = lc.shape_camera(shape_name), lc.lens_of(k, **kw)
    return cam, lens, lc.sphere_scene(cam, lc.lens_of(k))


# ---- 1. the rays ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens_name,shape_name", ALL)
def test_valid_rays_land_on_their_pixels(lib, lens_name, shape_name):
    """the float64 forward model of every valid fp32 ray lies within 2 max_residual of its pixel centre; r2_max and n_invalid are the
    table's; the Newton inverse agrees with every valid ray to 1e-3 in normalised units"""
    from optimalmodulationds_amd.engine import depth_lens_rays
    cam, lens, _ = case(lens_name, shape_name)
    ab, r2_max, n_invalid = depth_lens_rays(cam, lens)
    nu, nv, u, v = visited_grid(cam)
    ok = ~np.isnan(ab[:, 0])
    assert ab.shape == (nu * nv, 2) and n_invalid == int((~ok).sum()) and np.array_equal(np.isnan(ab[:, 0]), np.isnan(ab[:, 1]))
    if not ok.any():
        assert lens_name == "partial" and nu * nv < 100 and r2_max == 0.0, "only the tiny off-axis images lose every ray to two rounds"
        return
    uf, vf = lr.project(cam, lens, ab[ok, 0].astype(F64), ab[ok, 1].astype(F64))
    err = max(np.abs(uf - u[ok]).max(), np.abs(vf - v[ok]).max())
    print(f"{lens_name} {shape_name}: {int(ok.sum())} of {len(ok)} rays, worst float64 residual {err:.2e} px")
    assert err <= 2 * 0.01
    r2 = (ab[ok, 0].astype(F64) ** 2 + ab[ok, 1].astype(F64) ** 2).max()
    assert abs(r2_max - r2) <= 1e-6 * r2, "r2_max is the largest r2 of a valid ray"
    if lens_name != "partial":
        assert n_invalid == 0
    elif nu * nv > 100:
        centre = (np.abs(u - cam.cx) < 4) & (np.abs(v - cam.cy) < 4)
        assert 0.3 * len(ok) < n_invalid < 0.9 * len(ok) and ok[centre].all() and not ok[0] and not ok[-1], "the outer pixels get no ray"
    a64, b64, ok64 = lr.inverse(lens, (u[ok] - F64(cam.cx)) / F64(cam.fx), (v[ok] - F64(cam.cy)) / F64(cam.fy))
    assert ok64.all() and np.abs(a64 - ab[ok, 0]).max() < 1e-3 and np.abs(b64 - ab[ok, 1]).max() < 1e-3


def test_zero_lens_rays_are_the_pinhole_rays_bit_for_bit(lib):
    from optimalmodulationds_amd.engine import depth_lens_rays
    for sn, *_ in lc.SHAPES:
        cam = lc.shape_camera(sn)
        nu, nv, u, v = visited_grid(cam)
        a = (u.astype(F32) - F32(cam.cx)) * (F32(1) / F32(cam.fx))
        b = (v.astype(F32) - F32(cam.cy)) * (F32(1) / F32(cam.fy))
        for lens in (lc.lens_of(lc.ZERO), None):
            ab, r2_max, n_invalid = depth_lens_rays(cam, lens)
            assert np.array_equal(bits(ab[:, 0]), bits(a)) and np.array_equal(bits(ab[:, 1]), bits(b)) and n_invalid == 0, sn


# ---- 2. the points -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape_name", [s[0] for s in lc.SHAPES])
def test_zero_lens_and_no_lens_give_the_existing_points(lib, shape_name):
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.engine import depth_points
    cam = lc.shape_camera(shape_name)
    img = lc.sphere_scene(cam, lc.lens_of(lc.PLUMB))
    plain, n_plain = depth_points(img, cam)
    zero, n_zero = depth_points(img, cam, lens=lc.lens_of(lc.ZERO))
    assert n_zero == n_plain and np.array_equal(bits(zero), bits(plain)) and (n_plain > 0 or img.size < 4)
    none = L.OmdsDepthLens()      # model 0
    assert depth_points(img, cam, lens=none)[1] == n_plain and np.array_equal(bits(depth_points(img, cam, lens=none)[0]), bits(plain))
    f_plain = depth_points(img, cam, filter=dict(FILTER))
    f_zero = depth_points(img, cam, filter=dict(FILTER), lens=lc.lens_of(lc.ZERO))
    assert f_zero[1:] == f_plain[1:] and np.array_equal(bits(f_zero[0]), bits(f_plain[0]))


@pytest.mark.parametrize("lens_name,shape_name", [c for c in ALL if c[0] != "zero"])
def test_points_lie_on_the_rays(lib, lens_name, shape_name):
    """a kept pixel's point is the pose applied to (a z, b z, z) of its ray; a kept pixel without a ray is three NaNs, neither valid
    nor rejected; with the filter the rejected pixels are those of the pinhole filter (the support test reads depths, never rays)"""
    from optimalmodulationds_amd.engine import depth_lens_rays, depth_points
    cam, lens, img = case(lens_name, shape_name)
    ab, _, n_invalid = depth_lens_rays(cam, lens)
    plain, n_plain = depth_points(img, cam)
    got, n_valid = depth_points(img, cam, lens=lens)
    kept = ~np.isnan(plain[:, 0])
    ray = ~np.isnan(ab[:, 0])
    assert np.array_equal(~np.isnan(got[:, 0]), kept & ray) and n_valid == int((kept & ray).sum())
    nu, nv, u, v = visited_grid(cam)
    z = lc.z_of(cam, img)[v, u]
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    sel = kept & ray
    want = np.stack([ab[sel, 0] * z[sel], ab[sel, 1] * z[sel], z[sel]], 1) @ p[:, :3].T + p[:, 3]
    assert sel.sum() == 0 or np.abs(got[sel] - want).max() < 1e-5
    f_plain = depth_points(img, cam, filter=dict(FILTER))
    f_got = depth_points(img, cam, filter=dict(FILTER), lens=lens)
    f_kept = ~np.isnan(f_plain[0][:, 0])
    assert f_got[2] == f_plain[2] and np.array_equal(~np.isnan(f_got[0][:, 0]), f_kept & ray) and f_got[1] == int((f_kept & ray).sum())
    assert np.array_equal(bits(f_got[0][f_kept & ray]), bits(got[f_kept & ray]))


VOXEL = 0.05


def test_tilted_plane_is_flat_with_the_lens_and_bent_without(lib):
    """a plane rendered through the plumb-bob lens: every sphere of the lens run lies within the sphere radius plus one voxel of the
    plane; on the same image the pinhole run has spheres farther than that (the pixel-to-ray error of 14 % at the image edge is several
    voxels at 1.5 m)"""
    from optimalmodulationds_amd.engine import depth_points, point_cloud_spheres
    cam, lens = lc.camera(), lc.lens_of(lc.PLUMB)
    img = lc.plane_scene(cam, lens)
    n, d = lc.PLANE
    spec = spec_of((0.2, 0.2, -0.3), VOXEL, (32, 32, 32), max_spheres=8192)
    far = {}
    for name, l in (("lens", lens), ("pinhole", None)):
        pts = depth_points(img, cam, lens=l)[0]
        sp = point_cloud_spheres(pts, spec, cap=8192)
        dist = np.abs(sp[:, :3].astype(F64) @ n - d)
        far[name] = (len(sp), dist.max(), int((dist > sp[0, 3] + VOXEL).sum()))
        print(name, far[name])
    assert far["lens"][0] > 300 and far["lens"][2] == 0
    assert far["pinhole"][2] >= 20 and far["pinhole"][1] > 0.12


# ---- 3. the memory ---------------------------------------------------------------------------------------------------------------------------
def memory_case(lens_k=lc.PLUMB, fmt=U16, step=1):
    """a wall behind a slab of remembered cells 0.85 m in front of the camera, across the whole grid: some in the middle of the image,
    some near its edge, some beyond it"""
    cam = lc.camera(64, 48, fmt, step)
    lens = lc.lens_of(lens_k)
    img = lc.as_image(cam, lr.render(cam, lens, planes=[((1.0, 0.0, 0.0), lc.WALL_X)]))
    spec = spec_of(**lc.BOX, max_spheres=32768)
    dx, dy, dz = lc.BOX["dims"]
    m_in = np.zeros(dx * dy * dz, np.uint32)
    cells = np.array([(z * dy + y) * dx + 8 for z in range(dz) for y in range(dy)])
    m_in[cells] = 1
    return cam, lens, img, spec, m_in, cells


def centres(spec, cells):
    dx, dy = int(spec.dims[0]), int(spec.dims[1])
    idx = np.stack([cells % dx, (cells // dx) % dy, cells // (dx * dy)], 1)
    return (idx + 0.5) * F64(spec.voxel) + np.array(list(spec.origin), F64)


@pytest.mark.parametrize("footprint", [0, 1])
@pytest.mark.parametrize("fmt,step", [(U16, 1), (FLT, 2)])
def test_memory_clears_edge_cells_with_the_lens_and_the_mirror_agrees(lib, fmt, step, footprint):
    from optimalmodulationds_amd.engine import depth_lens_rays, depth_scene_memory, scene_memory_spec
    cam, lens, img, spec, m_in, cells = memory_case(fmt=fmt, step=step)
    mem = scene_memory_spec(5, 0.0, footprint)
    with_lens, counts = depth_scene_memory([img], [cam], spec, mem, m_in, lenses=[lens])
    pinhole, counts_pin = depth_scene_memory([img], [cam], spec, mem, m_in)
    r2_max = depth_lens_rays(cam, lens)[1]
    z = lc.z_of(cam, img)
    margin = 0.8660254 * float(spec.voxel)
    left_out, cleared_edge = 0, 0
    for cell, c in zip(cells, centres(spec, cells)):
        free, tie = lr.verdict(cam, lens, r2_max, z, margin, footprint, c)
        if tie:
            left_out += 1
            continue
        assert (with_lens[cell] == 0) == free, (cell, c, with_lens[cell], free)
        free_pin, _ = lr.verdict(cam, None, None, z, margin, footprint, c)
        cleared_edge += free and not free_pin
    print(f"fmt {fmt} step {step} footprint {footprint}: cleared {counts[2]} with the lens, {counts_pin[2]} without; {cleared_edge} edge cells; left out {left_out} of {len(cells)}")
    assert left_out <= 0.02 * len(cells)
    assert cleared_edge >= 20 and counts[2] >= counts_pin[2] + 20, "cells near the image edge are cleared with the lens only"
    assert counts[0] > 50 and counts[1] > 50, "the wall is seen, cells beyond the image are remembered"


def test_two_cameras_of_which_the_second_has_a_lens(lib):
    from optimalmodulationds_amd.engine import depth_points, depth_scene_memory, point_cloud_spheres, scene_memory_spec
    cam, lens, img, spec, m_in, cells = memory_case()
    cam0 = lc.camera(61, 47, FLT, 2, pose=dc.pose_of(dc.LOOK_ALONG_X, (0.0, 0.3, 0.4)))
    img0 = lc.as_image(cam0, lr.render(cam0, lc.ZERO, planes=[((1.0, 0.0, 0.0), lc.WALL_X)]))
    mem = scene_memory_spec(5)
    both, counts = depth_scene_memory([img0, img], [cam0, cam], spec, mem, m_in, lenses=[None, lens])
    none, counts_none = depth_scene_memory([img0, img], [cam0, cam], spec, mem, m_in)
    assert counts[2] > counts_none[2], "the second camera's lens clears more"
    pts = np.concatenate([depth_points(img0, cam0)[0], depth_points(img, cam, lens=lens)[0]])
    seen = np.nonzero(both == 1)[0]
    from cloud_cases import cells_of
    assert np.array_equal(seen, np.sort(cells_of(spec, point_cloud_spheres(pts, spec, cap=32768)))), "the counts are those of the lens points"
    with pytest.raises(ValueError):
        depth_scene_memory([img0, img], [cam0, cam], spec, mem, m_in, lenses=[lens])


def test_no_lens_is_the_existing_memory_and_flow(lib):
    from optimalmodulationds_amd.engine import depth_scene_memory, depth_scene_memory_flow, scene_memory_spec
    cam, lens, img, spec, m_in, cells = memory_case()
    mem, track = scene_memory_spec(5), track_of(2, 0.1)
    img2 = lc.sphere_scene(cam, lens, 0.05)
    for kw in (dict(), dict(filter=dict(FILTER))):
        want = depth_scene_memory([img], [cam], spec, mem, m_in, **kw)
        for lenses in ([None], [lc.lens_of(lc.ZERO)]):
            got = depth_scene_memory([img], [cam], spec, mem, m_in, lenses=lenses, **kw)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        fw = depth_scene_memory_flow([img2], [cam], spec, mem, track, prev=([img], [cam]), mem_in=m_in, **kw)
        for lenses in ([None], [lc.lens_of(lc.ZERO)]):
            fg = depth_scene_memory_flow([img2], [cam], spec, mem, track, prev=([img], [cam]), mem_in=m_in, lenses=lenses, **kw)
            for key in fw:
                a, b = np.asarray(fg[key]), np.asarray(fw[key])
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), key
    with_lens = depth_scene_memory_flow([img2], [cam], spec, mem, track, prev=([img], [cam]), mem_in=m_in, lenses=[lens])
    words = depth_scene_memory([img2], [cam], spec, mem, m_in, lenses=[lens])
    assert np.array_equal(with_lens["words"], words[0]) and with_lens["counts"][:4] == words[1] and with_lens["n_matched"] > 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(lib):
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.engine import depth_lens, depth_lens_rays, depth_points, depth_scene_memory, scene_memory_spec
    cam, lens, img, spec, m_in, cells = memory_case()
    flat = np.ascontiguousarray(img).reshape(-1)
    n = cam.width * cam.height

    def points(lens, null=0, cap=n):
        out, n_valid, n_rej = np.full((n, 3), -7.0, F32), C.c_int64(-5), C.c_int64(-6)
        rc = lib.omds_depth_points_lens(None if null & 1 else C.byref(cam), C.byref(lens), None, None if null & 2 else flat.ctypes.data,
                                        None if null & 4 else out.ctypes.data, cap, None if null & 8 else C.byref(n_valid), C.byref(n_rej))
        if rc != 0:
            assert (out == -7.0).all() and n_valid.value == -5 and n_rej.value == -6, "a refused call must write nothing"
        return rc

    def rays(lens, ab=True):
        out = np.full((n, 2), -7.0, F32)
        rc = lib.omds_depth_lens_rays(C.byref(cam), C.byref(lens), out.ctypes.data if ab else None, None, None)
        assert rc == 0 or (out == -7.0).all()
        return rc

    assert points(lens) == 0 and rays(lens) == 0
    bad = [dict(k1=np.nan), dict(k6=np.inf), dict(p1=-np.inf), dict(iters=65), dict(max_residual=np.nan), dict(max_residual=np.inf)]
    for change in bad:
        b = depth_lens(**change)
        assert points(b) == ERR_INVALID_ARG and rays(b) == ERR_INVALID_ARG, change
        assert b"depth lens" in lib.omds_last_error(None)
        with pytest.raises(L.OmdsError):
            depth_scene_memory([img], [cam], spec, scene_memory_spec(5), m_in, lenses=[b])
    other = depth_lens()
    other.model = 2
    assert points(other) == ERR_INVALID_ARG and rays(other) == ERR_INVALID_ARG
    for good in (dict(iters=64), dict(iters=-3), dict(max_residual=-1.0), dict(iters=1, max_residual=1e-6)):
        assert points(depth_lens(lc.PLUMB, **good)) == 0 and rays(depth_lens(lc.PLUMB, **good)) == 0, good
    for null in (1, 2, 4, 8):
        assert points(lens, null=null) == ERR_INVALID_ARG, null
    assert points(lens, cap=n - 1) == ERR_INVALID_ARG and rays(lens, ab=False) == ERR_INVALID_ARG
    with pytest.raises(L.OmdsError):
        depth_points(img, cam, lens=depth_lens(iters=65))
    with pytest.raises(L.OmdsError):
        depth_lens_rays(cam, depth_lens(k2=np.nan))
    with pytest.raises(ValueError):
        depth_lens([1.0, 2.0, 3.0])
    assert list(depth_lens([1, 2, 3, 4, 5]).k) == [1, 2, 3, 4, 5, 0, 0, 0] and list(depth_lens(lc.NFOV).k) == [F32(v) for v in lc.NFOV]
    d = depth_lens()
    assert (d.model, d.iters, d.max_residual) == (1, 0, 0.0)
    assert bits(depth_lens_rays(cam, depth_lens(lc.PLUMB))[0]).tobytes() == bits(depth_lens_rays(cam, depth_lens(lc.PLUMB, iters=20, max_residual=0.01))[0]).tobytes()


# ---- 5. the stand-alone build ------------------------------------------------------------------------------------------------------------------
def test_library_equals_the_stand_alone_build_bit_for_bit(lib, tmp_path):
    """tests/depth_lens_host.cpp under -fsanitize=address,undefined: every lens on every camera shape, with and without the depth
    filter, the image at exactly (H - 1) pitch + W elements and the outputs at exactly the visited count"""
    from optimalmodulationds_amd.engine import depth_lens, depth_lens_rays, depth_points
    exe = sanitized_host_program("depth_lens_host", tmp_path)
    cases = []
    for ln, sn in ALL:
        cam, lens, img = case(ln, sn)
        for filt in (None, fc.spec_of(**FILTER)):
            cases.append((cam, lens, True, filt, img))
    cam, lens, img = case("plumb", "67x50 f32")
    cases.append((cam, lens, False, None, img))
    n_good = len(cases)
    cases.append((cam, depth_lens(iters=65), True, None, img))
    cases.append((cam, depth_lens(k3=np.nan), True, fc.spec_of(**FILTER), img))

    def pack(cam, lens, have_lens, filt, img):
        flat = np.ascontiguousarray(lc.flat_of(cam, img))
        nu, nv, _, _ = visited_grid(cam)
        return (bytes(cam) + bytes(lens) + struct.pack("<i", 1 if have_lens else 0) + bytes(fc.spec_of() if filt is None else filt)
                + struct.pack("<iqiq", 0 if filt is None else 1, nu * nv, flat.itemsize, flat.size) + flat.tobytes())

    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(cases)) + b"".join(pack(*c) for c in cases))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "depth_lens_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off, n_ok = fout.read_bytes(), 0, 0
    for cam, lens, have_lens, filt, img in cases:
        rc_rays, r2_max, n_invalid, rc_points, n_valid, n_rejected, written = struct.unpack_from("<ifqiqqq", raw, off)
        off += 44
        ab = np.frombuffer(raw, F32, written * 2, off).reshape(-1, 2)
        off += written * 8
        xyz = np.frombuffer(raw, F32, written * 3, off).reshape(-1, 3)
        off += written * 12
        if rc_rays != 0 or rc_points != 0:
            assert (rc_rays, rc_points, written) == (ERR_INVALID_ARG, ERR_INVALID_ARG, 0)
            continue
        want_ab, want_r2, want_invalid = depth_lens_rays(cam, lens if have_lens else None)
        assert np.array_equal(bits(ab), bits(want_ab)) and bits(F32(r2_max)) == bits(F32(want_r2)) and n_invalid == want_invalid
        want = depth_points(img, cam, filter=filt, lens=lens if have_lens else None)
        assert np.array_equal(bits(xyz), bits(want[0])) and n_valid == want[1] and n_rejected == (want[2] if filt is not None else 0)
        n_ok += 1
    assert off == len(raw) and n_ok == n_good
