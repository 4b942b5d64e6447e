"""The definition of the points of a depth image on the host (include/omds.h: omds_depth_points; no context, no GPU) against the numpy
restatement of the header's text in tests/depth_cases.py.

EXACT CASE.  Power-of-two fx, fy, integer cx, cy, depth_scale 2^-10, raw depths <= 4095, width <= 32, R a signed permutation (the
camera looks along world x), t on the 2^-6 lattice: the test restates every intermediate in float64 and asserts that rounding it to
float32 changes nothing -- its own precondition -- and then the library's bits must be the restatement's.

GENERAL CASE.  fx = 615.3, a rotation from a unit quaternion, depth_scale 0.001, both formats.  Everything up to xc, yc, z is one
float32 operation per line, which numpy float32 restates exactly (asserted through the kept set).  The world coordinate is compared
with the float64 restatement (float32 ifx, ify and z as its inputs) within 7 * 2^-24 * S, S = |R_r0 xc| + |R_r1 yc| + |R_r2 z| + |t_r|
in float64: xc and yc each carry at most three relative roundings of 2^-24 (the subtraction, the product with ifx, the product with
z) into their products with R, 3 * 2^-24 (|R_r0 xc| + |R_r1 yc|) <= 3 * 2^-24 S; each of the three fmaf rounds a partial sum that is
at most S (1 + small) in magnitude, 3 * 2^-24 S; one more 2^-24 S covers the second-order terms.  float32 R and t are both sides'.

The same edge cases also go through a stand-alone build of the definition under AddressSanitizer + UBSan (tests/depth_host.cpp, the
image allocated at exactly (H - 1) pitch + W elements and the output at exactly the visited count), whose output must be the
library's bit for bit."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import depth_cases as dc
from cloud_cases import cells_of, restate as cloud_restate, spec_of
from depth_cases import F32, F64, FLT, U16
from helpers import sanitized_host_program

ERR_INVALID_ARG = 1
SENTINEL = F32(-7.0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def pitched(img, pitch):
    """(flat buffer of exactly (H - 1) pitch + W elements, its [H, W] view) holding ``img``"""
    H, W = img.shape
    flat = np.zeros((H - 1) * pitch + W, img.dtype)
    view = np.lib.stride_tricks.as_strided(flat, (H, W), (pitch * img.itemsize, img.itemsize))
    view[:] = img
    return flat, view


def visited_of(cam):
    s = max(int(cam.step), 1)
    return -(-cam.height // s) * -(-cam.width // s)


def call(lib, cam, flat, cap=None, null=0):
    """(rc, n_valid, xyz [cap, 3]) of the raw entry point on a flat buffer laid out by cam.pitch; a refused call must write nothing"""
    cap = visited_of(cam) if cap is None else cap
    out, n_valid = np.full((max(cap, 1), 3), SENTINEL, F32), C.c_int64(-5)
    rc = lib.omds_depth_points(None if null & 1 else C.byref(cam), None if null & 2 else flat.ctypes.data, None if null & 4 else out.ctypes.data,
                               cap, None if null & 8 else C.byref(n_valid))
    if rc != 0:
        assert (out == SENTINEL).all() and n_valid.value == -5, "a refused call must write nothing"
    return rc, int(n_valid.value), out[:cap]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def is_f32(x):
    return np.array_equal(np.asarray(x, F64).astype(F32).astype(F64), np.asarray(x, F64))


# ---- the exact case ----------------------------------------------------------------------------------------------------------------
def assert_exact_precondition(r, cam):
    for name in ("a", "b", "xc", "yc", "z", "t3", "t2", "w"):
        assert is_f32(r[name]), f"exact case: {name} is not a float32 everywhere"
    assert is_f32(F64(1) / F64(cam.fx)) and is_f32(F64(1) / F64(cam.fy))
    assert np.array_equal(r["a32"].astype(F64), r["a"]) and np.array_equal(r["b32"].astype(F64), r["b"])
    assert np.array_equal((r["z32"].astype(F64))[r["keep"]], r["z"][r["keep"]])


@pytest.mark.parametrize("step", [1, 2, 3])
def test_exact_case_matches_the_restatement_bit_for_bit(lib, step):
    cam, img = dc.exact_camera(step=step), dc.exact_image(1)
    r = dc.restate(cam, img)
    assert_exact_precondition(r, cam)
    rc, n_valid, got = call(lib, cam, img.reshape(-1))
    assert rc == 0 and n_valid == int(r["keep"].sum()) and 0 < n_valid < len(got)
    assert np.array_equal(np.isnan(got).all(1), ~r["keep"]) and not np.isnan(got[r["keep"]]).any()
    assert same_bits(got[r["keep"]], r["w"][r["keep"]].astype(F32)), "kept points are not the restatement's bits"
    assert np.isnan(got[~r["keep"]]).all(), "a dropped pixel is three NaNs"


def test_python_wrapper_is_the_raw_call(lib):
    from optimalmodulationds_amd.engine import depth_points
    cam, img = dc.exact_camera(), dc.exact_image(2)
    rc, n_valid, want = call(lib, cam, img.reshape(-1))
    got, n = depth_points(img, cam)
    assert rc == 0 and n == n_valid and same_bits(got, want)
    flat, view = pitched(img, 35)                      # a strided view: the pitch is taken from the row stride
    got2, n2 = depth_points(view, cam)
    assert n2 == n_valid and same_bits(got2, want)
    cam4 = dc.cam_of(32, 24, 64.0, 32.0, 16.0, 8.0, np.concatenate([np.array(list(cam.pose), F32).reshape(3, 4), [[0, 0, 0, 1]]]), U16, 2.0 ** -10,
                     2.0 ** -10, 4.0)
    assert bytes(cam4) == bytes(cam), "a 4 x 4 pose is its upper 3 x 4"


# ---- the general case --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [U16, FLT])
@pytest.mark.parametrize("step", [1, 3])
def test_general_case_within_the_stated_bound(lib, fmt, step):
    cam, img = dc.general_camera(fmt, step=step), dc.general_image(3, fmt)
    r = dc.restate(cam, img)
    rc, n_valid, got = call(lib, cam, img.reshape(-1))
    keep = r["keep"]
    assert rc == 0 and n_valid == int(keep.sum()) and 0.5 * len(keep) < n_valid < len(keep)
    assert np.array_equal(np.isnan(got).all(1), ~keep) and not np.isnan(got[keep]).any(), "the kept set is the float32 gate's"
    err = np.abs(got[keep].astype(F64) - r["w"][keep])
    bound = 7 * 2.0 ** -24 * r["S"][keep]
    worst = float((err / bound).max())
    print(f"general case fmt={fmt} step={step}: worst error / bound = {worst:.3f}")
    assert (err <= bound).all(), worst


# ---- pixel values -------------------------------------------------------------------------------------------------------------------
def test_u16_pixel_values_and_the_gate(lib):
    """raw 0 (no return), 1, 65535; z exactly z_min and z_max (kept) and one raw unit outside each (dropped)"""
    scale = F32(2.0 ** -10)
    cam = dc.cam_of(8, 1, 64.0, 64.0, 4.0, 0.0, None, U16, scale, 100 * scale, 1000 * scale)
    img = np.array([[0, 1, 65535, 100, 99, 1000, 1001, 500]], np.uint16)
    rc, n_valid, got = call(lib, cam, img.reshape(-1))
    assert rc == 0 and n_valid == 3
    assert list(np.isnan(got).all(1)) == [True, True, True, False, True, False, True, False]
    assert same_bits(got[[3, 5, 7], 2], F32([100, 1000, 500]) * scale)
    wide = dc.cam_of(8, 1, 64.0, 64.0, 4.0, 0.0, None, U16, scale, scale, 65535 * scale)      # the gate spans every raw value but 0
    rc, n_valid, got = call(lib, wide, img.reshape(-1))
    assert rc == 0 and n_valid == 7 and np.isnan(got[0]).all() and same_bits(got[1:3, 2], F32([1, 65535]) * scale)


def test_f32_pixel_values_and_the_gate(lib):
    """NaN, +-inf, -0, negative values fail the gate by the comparison; z_min and z_max are kept, one ulp outside each is dropped"""
    z_min, z_max = F32(0.3), F32(4.0)
    cam = dc.cam_of(11, 1, 64.0, 64.0, 4.0, 0.0, None, FLT, 1.0, z_min, z_max)
    img = np.array([[np.nan, np.inf, -np.inf, -0.0, -1.5, z_min, np.nextafter(z_min, F32(0)), z_max, np.nextafter(z_max, F32(9)), 0.0, 1.0]], F32)
    rc, n_valid, got = call(lib, cam, img.reshape(-1))
    assert rc == 0 and n_valid == 3
    assert list(np.isnan(got).all(1)) == [True] * 5 + [False, True, False, True, True, False]
    assert same_bits(got[[5, 7, 10], 2], [z_min, z_max, 1.0])
    assert same_bits(got[10], [(F32(10) - F32(4)) * (F32(1) / F32(64)), F32(0), F32(1)])
    nan_scale = dc.cam_of(11, 1, 64.0, 64.0, 4.0, 0.0, None, FLT, np.nan, z_min, z_max)      # depth_scale is the U16 format's alone
    assert call(lib, nan_scale, img.reshape(-1))[:2] == (0, 3)


# ---- image shapes ------------------------------------------------------------------------------------------------------------------
def test_one_pixel_image(lib):
    cam = dc.exact_camera(width=1, height=1)
    img = np.array([[1024]], np.uint16)
    rc, n_valid, got = call(lib, cam, img.reshape(-1))
    r = dc.restate(cam, img)
    assert rc == 0 and n_valid == 1 and got.shape == (1, 3) and same_bits(got, r["w"].astype(F32))
    assert same_bits(got[0], [0.25 + 1.0, -0.5 + 0.25, 0.75 + 0.25])      # a = -16 / 64, b = -8 / 32 at z = 1: y = t_y - xc, z = t_z - yc


@pytest.mark.parametrize("step,visited", [(1, 91), (2, 28), (3, 15), (20, 1), (0, 91), (-3, 91)])
@pytest.mark.parametrize("pitch", [0, 16])
def test_13x7_steps_and_pitch(lib, step, visited, pitch):
    """13 x 7: ceil(7 / step) * ceil(13 / step) visited pixels in row-major order; pitch = width + 3; step < 1 is 1"""
    img = dc.exact_image(4, 13, 7)
    flat, view = pitched(img, pitch or 13)
    assert len(flat) == 6 * (pitch or 13) + 13
    cam = dc.exact_camera(13, 7, step, pitch)
    r = dc.restate(cam, view)
    rc, n_valid, got = call(lib, cam, flat)
    assert rc == 0 and len(got) == visited == len(r["keep"]) and n_valid == int(r["keep"].sum())
    assert same_bits(got, dc.points_of(r))
    assert call(lib, cam, flat, cap=visited - 1)[0] == ERR_INVALID_ARG
    rc, _, more = call(lib, cam, flat, cap=visited + 2)
    assert rc == 0 and same_bits(more[:visited], got) and (more[visited:] == SENTINEL).all(), "rows past the visited count stay untouched"


# ---- composition with the cloud definition -------------------------------------------------------------------------------------------
def test_composition_with_the_cloud_definition_on_cell_faces(lib):
    """exact case with pixels planted so that their points fall on cell faces (they belong to the cell above) and on the grid's upper
    faces (dropped): omds_point_cloud_spheres(omds_depth_points(...)) occupies exactly the restatement's cells"""
    from optimalmodulationds_amd.engine import depth_points, point_cloud_spheres
    cam, img = dc.exact_camera(t=(0.25, -0.5, 0.75)), dc.exact_image(5)
    img[3, 24] = 512      # a = 1 / 8, z = 1 / 2: xc = 1 / 16, a y face;  world x = 0.75, an x face
    img[8, 24] = 1024     # b = 0: yc = 0, world z = t_z = 0.75, a z face
    img[8, 16] = 2048 - 256    # world x = 0.25 + 1.75 = 2.0 = the grid's upper x face below: dropped
    img[8, 17] = 2047 - 256    # one raw unit nearer: the last cell
    img[0, 16] = 4095
    spec = spec_of((0.25, -1.5, -0.25), 0.0625, (28, 32, 24), max_spheres=65536)
    r = dc.restate(cam, img)
    assert_exact_precondition(r, cam)
    pts = dc.points_of(r)
    on_face = np.isclose((pts[r["keep"]] - np.array(list(spec.origin), F32)) / F32(0.0625) % 1, 0).any(1)
    top = F32(0.25) + F32(0.0625) * 28
    assert on_face.sum() >= 3 and (pts[r["keep"], 0] == top).any() and top == 2.0
    xyz, n_valid = depth_points(img, cam)
    assert same_bits(xyz, pts)
    got = point_cloud_spheres(xyz, spec, cap=65536)
    occ, want, _ = cloud_restate(spec, pts)
    assert len(occ) > 100 and np.array_equal(cells_of(spec, got), occ)
    assert same_bits(got, want)
    inside = ((pts >= np.array(list(spec.origin), F32)) & (pts < np.array(list(spec.origin), F32) + F32(0.0625) * F32([28, 32, 24]))).all(1)
    assert 0 < inside.sum() < n_valid, "some kept pixels fall outside the grid"


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def _bad_cameras():
    ok = dict(width=13, height=7, fx=64.0, fy=32.0, cx=6.0, cy=3.0, pose=None, fmt=U16, depth_scale=2.0 ** -10, z_min=0.1, z_max=4.0, step=1, pitch=0)
    bad = []
    for change in (dict(width=0), dict(height=0), dict(width=-3), dict(pitch=12), dict(pitch=-1), dict(fmt=2), dict(fmt=-1), dict(fx=0.0),
                   dict(fy=0.0), dict(fx=np.nan), dict(fy=np.inf), dict(cx=np.nan), dict(cy=-np.inf), dict(depth_scale=0.0), dict(depth_scale=-1.0),
                   dict(depth_scale=np.nan), dict(depth_scale=np.inf), dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=np.nan), dict(z_max=np.inf),
                   dict(z_min=2.0, z_max=1.0), dict(z_max=np.nan)):
        bad.append(dc.cam_of(**dict(ok, **change)))
    for i in (0, 5, 11):
        pose = np.eye(4, dtype=F32)[:3].copy()
        pose.reshape(-1)[i] = [np.nan, np.inf, -np.inf][i % 3]
        bad.append(dc.cam_of(**dict(ok, pose=pose)))
    return dc.cam_of(**ok), bad


def test_errors_write_nothing(lib):
    ok, bad = _bad_cameras()
    flat = dc.exact_image(6, 13, 7).reshape(-1)
    assert call(lib, ok, flat)[0] == 0
    assert call(lib, dc.cam_of(13, 7, -64.0, -32.0, 6.0, 3.0, None, U16, 2.0 ** -10, 0.1, 0.1), flat)[0] == 0      # negative focal lengths, z_min == z_max
    for cam in bad:
        assert call(lib, cam, flat)[0] == ERR_INVALID_ARG, bytes(cam)
    for null in (1, 2, 4, 8):
        assert call(lib, ok, flat, null=null)[0] == ERR_INVALID_ARG
    assert call(lib, ok, flat, cap=90)[0] == ERR_INVALID_ARG and call(lib, ok, flat, cap=0)[0] == ERR_INVALID_ARG
    assert call(lib, ok, flat, cap=-1)[0] == ERR_INVALID_ARG
    assert b"cap_points" in lib.omds_last_error(None)
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import depth_camera, depth_points
    with pytest.raises(_lib.OmdsError):
        depth_points(dc.exact_image(6, 13, 7), bad[7])
    with pytest.raises(ValueError):
        depth_points(dc.exact_image(6, 13, 7).astype(F32), ok)      # the image's type is not the camera's format
    with pytest.raises(ValueError):
        depth_camera(13, 7, 64.0, 32.0, 6.0, 3.0, pose=np.eye(3))


# ---- the sanitizer leg -------------------------------------------------------------------------------------------------------------
def _pack_case(cam, flat, cap, null):
    flat = np.ascontiguousarray(flat)
    return bytes(cam) + struct.pack("<qiiq", cap, null, flat.itemsize, flat.size) + flat.tobytes()


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    """tests/depth_host.cpp, a stand-alone program around the header both the library and its kernels include, built with
    -fsanitize=address,undefined: the image at exactly (H - 1) pitch + W elements, the output at exactly the visited count; a clean
    exit, and the library's bits."""
    exe = sanitized_host_program("depth_host", tmp_path)
    cases = []
    for step in (1, 2, 3, 20):
        for pitch in (0, 16):
            cases.append((dc.exact_camera(13, 7, step, pitch), pitched(dc.exact_image(4, 13, 7), pitch or 13)[0], None, 0))
    cases.append((dc.exact_camera(1, 1), np.array([1024], np.uint16), None, 0))
    for fmt in (U16, FLT):
        for step in (1, 3):
            cases.append((dc.general_camera(fmt, step=step), dc.general_image(3, fmt).reshape(-1), None, 0))
    cases.append((dc.general_camera(FLT, 33, 17), pitched(dc.general_image(7, FLT, 33, 17), 40)[0], None, 0))
    cases[-1][0].pitch = 40
    z_min, z_max = F32(0.3), F32(4.0)
    cases.append((dc.cam_of(11, 1, 64.0, 64.0, 4.0, 0.0, None, FLT, 1.0, z_min, z_max),
                  np.array([np.nan, np.inf, -np.inf, -0.0, -1.5, z_min, np.nextafter(z_min, F32(0)), z_max, np.nextafter(z_max, F32(9)), 0.0, 1.0], F32), None, 0))
    cases.append((dc.cam_of(8, 1, 64.0, 64.0, 4.0, 0.0, None, U16, 2.0 ** -10, 2.0 ** -10, 64.0), np.array([0, 1, 65535, 100, 99, 1000, 1001, 500], np.uint16),
                  None, 0))
    ok, bad = _bad_cameras()
    flat = dc.exact_image(6, 13, 7).reshape(-1)
    for cam in bad:
        cases.append((cam, flat, 91, 0))
    for null in (1, 2, 4, 8):
        cases.append((ok, flat, 91, null))
    cases.append((ok, flat, 90, 0))                # cap one short of the visited count: nothing written
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(cases)) + b"".join(_pack_case(c, f, visited_of(c) if cap is None else cap, null) for c, f, cap, null in cases))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "depth_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off = fout.read_bytes(), 0
    n_ok = 0
    for cam, f, cap, null in cases:
        rc, n_valid, written = struct.unpack_from("<iqq", raw, off)
        off += 20
        got = np.frombuffer(raw, F32, written * 3, off).reshape(-1, 3)
        off += written * 12
        want_rc, want_valid, want = call(lib, cam, np.ascontiguousarray(f), cap, null)
        assert rc == want_rc and (rc != 0 or n_valid == want_valid)
        if rc == 0:
            assert same_bits(got, want)
            n_ok += 1
        else:
            assert written == 0 and n_valid == -1
    assert off == len(raw) and n_ok == 16
