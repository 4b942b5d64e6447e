"""The definition of the depth filter on the host (include/omds.h: omds_depth_points_filtered, omds_depth_scene_memory_filtered; no
context, no GPU) against the numpy restatement of the header's text in tests/depth_filter_cases.py.

BIT FOR BIT.  Everything the filter adds up to its comparison is one float32 operation per line, which numpy restates exactly; tol is
one fmaf, restated in float64.  EXACT CASE: power-of-two edge_abs, edge_rel and depth_scale and raw depths of 11 bits -- tol's float64
value is a float32 (asserted) -- on the exact camera of tests/depth_cases.py, so kept set, points and n_rejected must be the
restatement's.  GENERAL CASE: the kept set and n_rejected are still exact (tol's rare float32 ties are settled in rational
arithmetic); the points of the kept pixels are those of omds_depth_points, which tests/test_depth_cpu.py bounds.

The images are a BAND of depths in which neighbours agree by chance; every such test asserts that the filter keeps between 0.2 and 0.8
of the returns, so that neither "keeps all" nor "drops all" can pass.

The same edge cases go through a stand-alone build of the definition under AddressSanitizer + UBSan (tests/depth_filter_host.cpp, the
image at exactly (H - 1) pitch + W elements, the output at exactly the visited count, radius 3), whose output must be the library's."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import depth_filter_cases as fc
from cloud_cases import cells_of, spec_of as cloud_spec_of
from depth_cases import F32, F64, FLT, U16
from helpers import sanitized_host_program
from test_depth_cpu import ERR_INVALID_ARG, SENTINEL, call as plain_call, is_f32, pitched, same_bits, visited_of


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def call(lib, cam, filt, flat, cap=None, null=0):
    """(rc, n_valid, n_rejected, xyz [cap, 3]) of the raw entry point; a refused call must write nothing.  null: 1 cam, 2 image,
    4 xyz_out, 8 n_valid_out, 16 n_rejected_out"""
    cap = visited_of(cam) if cap is None else cap
    out, n_valid, n_rejected = np.full((max(cap, 1), 3), SENTINEL, F32), C.c_int64(-5), C.c_int64(-6)
    rc = lib.omds_depth_points_filtered(None if null & 1 else C.byref(cam), None if filt is None else C.byref(filt),
                                        None if null & 2 else flat.ctypes.data, None if null & 4 else out.ctypes.data, cap,
                                        None if null & 8 else C.byref(n_valid), None if null & 16 else C.byref(n_rejected))
    if rc != 0:
        assert (out == SENTINEL).all() and n_valid.value == -5 and n_rejected.value == -6, "a refused call must write nothing"
    return rc, int(n_valid.value), int(n_rejected.value), out[:cap]


def check(lib, cam, filt, view, flat=None, exact=False, band=True):
    """the library against the restatement: kept set, n_valid, n_rejected, the points; -> the restatement"""
    flat = np.ascontiguousarray(view).reshape(-1) if flat is None else flat
    r = fc.restate(cam, view, filt)
    if exact:
        assert r["tol_is_f32"] and r["ambiguous"] == 0, "exact case: tol is not a float32 before rounding"
        for name in ("a", "b", "xc", "yc", "z", "t3", "t2", "w"):
            assert is_f32(r[name]), f"exact case: {name} is not a float32 everywhere"
    if band:
        assert 0.2 <= fc.survival(r) <= 0.8, f"the band does not test the filter: it keeps {fc.survival(r):.3f} of the returns"
    rc, n_valid, n_rejected, got = call(lib, cam, filt, flat)
    assert rc == 0 and n_valid == int(r["keep"].sum()) and n_rejected == int(r["rejected"].sum()), (rc, n_valid, n_rejected)
    assert np.array_equal(np.isnan(got).all(1), ~r["keep"]) and not np.isnan(got[r["keep"]]).any(), "the kept set is not the restatement's"
    rc0, n0, plain = plain_call(lib, cam, flat)
    assert rc0 == 0 and n0 == n_valid + n_rejected and same_bits(got[r["keep"]], plain[r["keep"]]), "a kept pixel keeps omds_depth_points' point"
    if exact:
        assert same_bits(got, dc.points_of(r)), "the points are not the restatement's bits"
    return r


EXACT_FILTER = dict(radius=1, min_support=2, edge_abs=2.0 ** -7, edge_rel=2.0 ** -9)


# ---- 1. bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("pitch", [0, 37])
def test_exact_case_matches_the_restatement_bit_for_bit(lib, step, pitch):
    """U16 1000 + randint(0, 64) with 10 % zeros on the exact camera; step 1, 2, 3 (the window is one of VISITED pixels); pitch > width"""
    img = fc.band_u16(1, 32, 24)
    flat, view = pitched(img, pitch or 32)
    cam = dc.exact_camera(step=step, pitch=pitch)
    r = check(lib, cam, fc.spec_of(**EXACT_FILTER), view, flat, exact=True)
    assert r["rejected"].sum() > 20 and r["keep"].sum() > 20


@pytest.mark.parametrize("radius,min_support,edge_abs", [(2, 6, 2.0 ** -7), (3, 10, 2.0 ** -7)])
def test_exact_case_wider_windows(lib, radius, min_support, edge_abs):
    check(lib, dc.exact_camera(), fc.spec_of(radius, min_support, edge_abs, 2.0 ** -9), fc.band_u16(2, 32, 24), exact=True)


@pytest.mark.parametrize("fmt", [U16, FLT])
@pytest.mark.parametrize("step", [1, 3])
def test_general_case_kept_set_and_counts(lib, fmt, step):
    """fx = 615.3, a rotation from a quaternion, depth_scale 0.001, edge 0.0071 + 0.0013 z; the F32 image has NaN, +inf and -inf elements"""
    cam = dc.general_camera(fmt, step=step)
    img = fc.band_u16(3, 64, 48) if fmt == U16 else fc.band_f32(3, 64, 48)
    r = check(lib, cam, fc.spec_of(1, 2, 0.0071, 0.0013), img)
    if fmt == FLT:
        assert np.isinf(img).sum() > 50 and np.isnan(img).sum() > 100
    print(f"general case fmt={fmt} step={step}: kept {int(r['keep'].sum())} rejected {int(r['rejected'].sum())} tol ties settled exactly {r['ambiguous']}")


def test_neighbours_outside_the_range_gate_support(lib):
    """the gate cuts the band in the middle of both ends: pixels kept only because a neighbour beyond z_max or below z_min supports
    them exist, and the library keeps them (a restatement that gates the neighbours differs)"""
    img = fc.band_u16(4, 32, 24)
    cam = dc.exact_camera(z_min=1016 * 2.0 ** -10, z_max=1047 * 2.0 ** -10)
    filt = fc.spec_of(**EXACT_FILTER)
    r = check(lib, cam, filt, img, exact=True)
    gated = fc.restate(cam, img, filt, gate_neighbours=True)
    only = r["keep"] & ~gated["keep"]
    z = fc.z_n_of(cam, img)
    assert only.sum() > 10 and (z > F32(cam.z_max)).sum() > 50 and (z < F32(cam.z_min)).sum() > 50
    assert 0.3 * (img != 0).sum() < r["unfiltered"].sum() < 0.7 * (img != 0).sum(), "the gate keeps about half of the band"


@pytest.mark.parametrize("radius", [1, 3])
def test_corners_and_borders(lib, radius):
    """a flat image: every pixel is supported by all the others of its window that lie inside the image -- a corner by (r + 1)^2 - 1
    of them, a border pixel away from the corners by (r + 1)(2 r + 1) - 1, an inner pixel by (2 r + 1)^2 - 1"""
    cam, img = dc.exact_camera(13, 9), np.full((9, 13), 1024, np.uint16)
    corner, border, inner = (radius + 1) ** 2 - 1, (radius + 1) * (2 * radius + 1) - 1, (2 * radius + 1) ** 2 - 1
    r = check(lib, cam, fc.spec_of(radius, 1, 0.0, 0.0), img, exact=True, band=False)
    s = r["support"].reshape(9, 13)
    assert s[0, 0] == s[0, 12] == s[8, 0] == s[8, 12] == corner and s[0, 6] == s[4, 0] == s[8, 6] == s[4, 12] == border and s[4, 6] == inner
    for min_support, kept in ((corner, 9 * 13), (corner + 1, 9 * 13 - 4), (inner, (9 - 2 * radius) * (13 - 2 * radius))):
        rr = check(lib, cam, fc.spec_of(radius, min_support, 0.0, 0.0), img, exact=True, band=False)
        assert rr["keep"].sum() == kept, (radius, min_support, int(rr["keep"].sum()))


@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1), (2, 5), (5, 2)])
def test_images_smaller_than_the_window(lib, radius, shape):
    """1 x 1 has no other pixel: min_support >= 1 rejects it; 2 x 5 and 5 x 2 have at most 9 others"""
    W, H = shape
    cam, img = dc.exact_camera(W, H), np.full((H, W), 1024, np.uint16)
    r = check(lib, cam, fc.spec_of(radius, 1, 0.0, 0.0), img, exact=True, band=False)
    assert r["support"].max() == min(W, 2 * radius + 1) * min(H, 2 * radius + 1) - 1
    assert r["keep"].sum() == (0 if W == 1 else W * H) and r["rejected"].sum() == (1 if W == 1 else 0)
    if W > 1:
        img[0, 0] = 2048                   # one pixel off the plane: it alone goes
        rr = check(lib, cam, fc.spec_of(radius, 1, 2.0 ** -7, 0.0), img, exact=True, band=False)
        assert rr["rejected"].sum() == 1 and rr["rejected"][0]


def test_f32_special_elements_as_neighbours_and_centres(lib):
    """NaN, +-inf and -0 neighbours give no support; a finite neighbour within tol does; a pixel that fails the gate is not counted as
    rejected"""
    cam = dc.cam_of(5, 1, 64.0, 64.0, 2.0, 0.0, None, FLT, 1.0, 0.5, 4.0)
    f = fc.spec_of(1, 1, 0.25, 0.0)
    for row, keep, rejected in (([np.nan, 1.0, np.inf, 1.0, -np.inf], 0, 2), ([1.0, 1.25, np.nan, -0.0, 0.2], 2, 0), ([1.0, 1.3, 1.5, 8.0, 7.9], 2, 1),
                                ([0.3, 0.5, np.nan, 4.0, 4.2], 2, 0)):
        img = np.array([row], F32)
        r = check(lib, cam, f, img, band=False)
        assert (int(r["keep"].sum()), int(r["rejected"].sum())) == (keep, rejected), row


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(lib):
    cam, flat = dc.exact_camera(13, 7), fc.band_u16(5, 13, 7).reshape(-1)
    ok = fc.spec_of(**EXACT_FILTER)
    assert call(lib, cam, ok, flat)[0] == 0
    bad = [dict(radius=0), dict(radius=4), dict(radius=-1), dict(min_support=0), dict(min_support=9), dict(radius=2, min_support=25),
           dict(radius=3, min_support=49), dict(edge_abs=-0.01), dict(edge_abs=np.nan), dict(edge_abs=np.inf), dict(edge_rel=-1e-3),
           dict(edge_rel=np.nan), dict(edge_rel=-np.inf)]
    for change in bad:
        assert call(lib, cam, fc.spec_of(**dict(EXACT_FILTER, **change)), flat)[0] == ERR_INVALID_ARG, change
    assert b"depth filter" in lib.omds_last_error(None)
    for good in (dict(min_support=8), dict(radius=2, min_support=24), dict(radius=3, min_support=48), dict(edge_abs=0.0, edge_rel=0.0)):
        assert call(lib, cam, fc.spec_of(**dict(EXACT_FILTER, **good)), flat)[0] == 0, good
    for null in (1, 2, 4, 8, 16):
        assert call(lib, cam, ok, flat, null=null)[0] == ERR_INVALID_ARG, null
    assert call(lib, cam, ok, flat, cap=90)[0] == ERR_INVALID_ARG and call(lib, cam, ok, flat, cap=-1)[0] == ERR_INVALID_ARG
    assert call(lib, dc.exact_camera(13, 7, pitch=12), ok, flat)[0] == ERR_INVALID_ARG      # a bad camera, as omds_depth_points
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import depth_points
    with pytest.raises(_lib.OmdsError):
        depth_points(flat.reshape(7, 13), cam, filter=dict(radius=4))


def test_null_filter_is_the_plain_call(lib):
    for cam, img in ((dc.exact_camera(step=2), fc.band_u16(6, 32, 24)), (dc.general_camera(FLT), fc.band_f32(6, 64, 48))):
        flat = img.reshape(-1)
        rc, n_valid, n_rejected, got = call(lib, cam, None, flat)
        rc0, n0, want = plain_call(lib, cam, flat)
        assert rc == rc0 == 0 and n_valid == n0 and n_rejected == 0 and same_bits(got, want)
        assert call(lib, cam, None, flat, null=16)[:2] == (0, n0), "without a filter n_rejected_out may be null"
    from optimalmodulationds_amd.engine import depth_points
    cam, img = dc.exact_camera(), fc.band_u16(6, 32, 24)
    xyz, n_valid, n_rejected = depth_points(img, cam, filter=dict(EXACT_FILTER))
    r = fc.restate(cam, img, fc.spec_of(**EXACT_FILTER))
    assert (n_valid, n_rejected) == (int(r["keep"].sum()), int(r["rejected"].sum())) and np.array_equal(np.isnan(xyz).all(1), ~r["keep"])


# ---- 3. it does what it is for -----------------------------------------------------------------------------------------------------------
VOXEL = 0.04
SCENE_FILTER = dict(radius=1, min_support=4, edge_abs=0.01, edge_rel=0.01)


def test_phantoms_go_and_surfaces_stay(lib):
    """two spheres in front of a wall, rendered at 640 x 480 and box-averaged to 160 x 120: the mixed pixels on the spheres' outlines
    are phantom cells in free space; the filter removes every one of them and keeps the surfaces"""
    from optimalmodulationds_amd.engine import depth_points
    cam, img = fc.rendered_scene()
    raw, _ = depth_points(img, cam)
    filt, n_valid, n_rejected = depth_points(img, cam, filter=dict(SCENE_FILTER))
    c_raw, c_filt = fc.cells_of_points(raw, VOXEL), fc.cells_of_points(filt, VOXEL)
    p_raw, p_filt = fc.phantom(c_raw, VOXEL), fc.phantom(c_filt, VOXEL)
    true_raw, true_filt = int((~p_raw).sum()), int((~p_filt).sum())
    print(f"unfiltered: {int(p_raw.sum())} phantom cells of {len(c_raw)}; filtered: {int(p_filt.sum())} phantom cells, "
          f"{true_filt} of {true_raw} true cells = {true_filt / true_raw:.3f}; {n_rejected} of {n_valid + n_rejected} pixels rejected")
    assert p_raw.sum() >= 100
    assert p_filt.sum() == 0
    assert true_filt >= 0.97 * true_raw


# ---- 4. the memory definition --------------------------------------------------------------------------------------------------------------
GRID = dict(origin=(0.0, -1.6, -0.72), voxel=VOXEL, dims=(56, 80, 64))


def centres(spec, cells):
    dx, dy = int(spec.dims[0]), int(spec.dims[1])
    idx = np.stack([cells % dx, (cells // dx) % dy, cells // (dx * dy)], 1)
    return (idx + 0.5) * F64(spec.voxel) + np.array(list(spec.origin), F64)


def phantom_cells(spec, words):
    cells = np.nonzero(words)[0]
    return cells[fc.phantom_at(centres(spec, cells), VOXEL)]


def test_phantoms_never_enter_the_memory(lib):
    """frame 1: the rendered scene; frame 2: the sensor returns nothing, so every cell of the memory is remembered.  Without a filter
    the phantom cells of frame 1 are in the scene of frame 2; with it they never entered the memory.  The seen cells of a filtered
    call are the cells of the filtered points"""
    from optimalmodulationds_amd.engine import depth_points, depth_scene_memory, point_cloud_spheres, scene_memory_spec
    cam, img = fc.rendered_scene()
    spec, mem = cloud_spec_of(**GRID, max_spheres=65536), scene_memory_spec(5)
    blind = np.zeros_like(img)
    m1, counts1 = depth_scene_memory([img], [cam], spec, mem)
    ph = phantom_cells(spec, m1)
    assert len(ph) >= 100 and counts1[0] == int((m1 == 1).sum())
    m2, counts2 = depth_scene_memory([blind], [cam], spec, mem, m1)
    assert (m2[ph] == 2).all() and counts2 == (0, counts1[0], 0, 0), "the phantoms of frame 1 are remembered in frame 2"
    f1, fcounts1 = depth_scene_memory([img], [cam], spec, mem, filter=dict(SCENE_FILTER))
    assert len(phantom_cells(spec, f1)) == 0 and not f1[ph].any() and 0.9 * (counts1[0] - len(ph)) < fcounts1[0] < counts1[0]
    f2, fcounts2 = depth_scene_memory([blind], [cam], spec, mem, f1, filter=dict(SCENE_FILTER))
    assert len(phantom_cells(spec, f2)) == 0 and fcounts2 == (0, fcounts1[0], 0, 0)
    xyz = depth_points(img, cam, filter=dict(SCENE_FILTER))[0]
    assert np.array_equal(np.nonzero(f1)[0], np.sort(cells_of(spec, point_cloud_spheres(xyz, spec, cap=65536)))), "n[c] are the counts of the filtered points"


def test_verdicts_read_the_raw_image(lib):
    """a remembered cell 1 m in front of a lone speckle return on an otherwise blind patch of the wall: the filter rejects the speckle
    as a point (its wall cell is not seen), and the speckle still clears the cell -- a flying pixel is still a return"""
    from optimalmodulationds_amd.engine import depth_points, depth_scene_memory, scene_memory_spec
    cam, img = fc.rendered_scene()
    spec, mem = cloud_spec_of(**GRID, max_spheres=65536), scene_memory_spec(5)
    cell = (30 * 80 + 32) * 56 + 25      # centre (1.02, -0.30, 0.50): beside the near sphere, in front of the wall
    c = centres(spec, np.array([cell]))[0]
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    pc = p[:, :3].T @ (c - p[:, 3])
    ju, jv = int(np.rint(pc[0] / pc[2] * cam.fx + cam.cx)), int(np.rint(pc[1] / pc[2] * cam.fy + cam.cy))
    assert 5 < ju < 155 and 5 < jv < 115 and img[jv, ju] > 1900, "the cell projects onto the wall"
    img = img.copy()
    speckle = img[jv, ju]
    img[jv - 4:jv + 5, ju - 4:ju + 5] = 0
    img[jv, ju] = speckle
    m_in = np.zeros(56 * 80 * 64, np.uint32)
    m_in[cell] = 1
    raw, counts_raw = depth_scene_memory([img], [cam], spec, mem, m_in)
    filt, counts_filt = depth_scene_memory([img], [cam], spec, mem, m_in, filter=dict(SCENE_FILTER))
    assert counts_raw[2] == 1 and counts_filt[2] == 1 and raw[cell] == 0 and filt[cell] == 0, "the speckle clears the cell with and without the filter"
    at = np.floor((depth_points(img, cam)[0][jv * 160 + ju].astype(F64) - np.array(list(spec.origin), F64)) / VOXEL).astype(int)
    wall_cell = (at[2] * 80 + at[1]) * 56 + at[0]
    assert at[0] in (49, 50) and raw[wall_cell] == 1 and filt[wall_cell] == 0, "... and is no point under the filter"
    img[jv, ju] = 0
    assert depth_scene_memory([img], [cam], spec, mem, m_in, filter=dict(SCENE_FILTER))[0][cell] == 2, "without the speckle the cell is remembered"


def test_filtered_memory_with_a_null_filter_is_the_plain_definition(lib):
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.engine import scene_memory_spec
    cam, img = fc.rendered_scene()
    spec, mem = cloud_spec_of(**GRID, max_spheres=65536), scene_memory_spec(5)
    table, addrs = (L.OmdsDepthCamera * 1)(cam), (C.c_void_p * 1)(img.ctypes.data)
    cells = 56 * 80 * 64
    outs = []
    for filtered in (False, True):
        out, counts = np.full(cells, 0xA5A5A5A5, np.uint32), np.full(4, -7, np.int32)
        if filtered:
            rc = lib.omds_depth_scene_memory_filtered(C.byref(spec), C.byref(mem), None, table, addrs, 1, None, out.ctypes.data, counts.ctypes.data)
        else:
            rc = lib.omds_depth_scene_memory(C.byref(spec), C.byref(mem), table, addrs, 1, None, out.ctypes.data, counts.ctypes.data)
        assert rc == 0
        outs.append((out, counts))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][1][0] > 2000
    out, counts = np.full(cells, 0xA5A5A5A5, np.uint32), np.full(4, -7, np.int32)
    bad = fc.spec_of(radius=4)
    rc = lib.omds_depth_scene_memory_filtered(C.byref(spec), C.byref(mem), C.byref(bad), table, addrs, 1, None, out.ctypes.data, counts.ctypes.data)
    assert rc == ERR_INVALID_ARG and (out == 0xA5A5A5A5).all() and (counts == -7).all(), "a refused spec writes nothing"


# ---- 5. the sanitizer leg --------------------------------------------------------------------------------------------------------------
def _pack_case(cam, filt, flat, cap, null):
    flat = np.ascontiguousarray(flat)
    return (bytes(cam) + bytes(fc.spec_of() if filt is None else filt) + struct.pack("<iqiiq", 0 if filt is None else 1, cap, null, flat.itemsize, flat.size)
            + flat.tobytes())


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    """tests/depth_filter_host.cpp, a stand-alone program around the header both the library and its kernels include, built with
    -fsanitize=address,undefined: the image at exactly (H - 1) pitch + W elements, the output at exactly the visited count, windows of
    radius 3 that leave the image on every side; a clean exit, and the library's bits"""
    exe = sanitized_host_program("depth_filter_host", tmp_path)
    wide = fc.spec_of(3, 10, 2.0 ** -7, 2.0 ** -9)
    cases = []
    for step in (1, 2, 3):
        for pitch in (0, 37):
            cases.append((dc.exact_camera(step=step, pitch=pitch), wide, pitched(fc.band_u16(1, 32, 24), pitch or 32)[0], None, 0))
    for W, H in ((1, 1), (2, 5), (5, 2), (13, 9)):
        cases.append((dc.exact_camera(W, H), fc.spec_of(3, 1, 0.0, 0.0), np.full(W * H, 1024, np.uint16), None, 0))
    for fmt in (U16, FLT):
        img = fc.band_u16(3, 64, 48) if fmt == U16 else fc.band_f32(3, 64, 48)
        cases.append((dc.general_camera(fmt, step=3), fc.spec_of(3, 12, 0.0071, 0.0013), img.reshape(-1), None, 0))
        cases.append((dc.general_camera(fmt), fc.spec_of(1, 2, 0.0071, 0.0013), img.reshape(-1), None, 0))
    cases.append((dc.exact_camera(z_min=1016 * 2.0 ** -10, z_max=1047 * 2.0 ** -10), wide, fc.band_u16(4, 32, 24).reshape(-1), None, 0))
    cases.append((dc.exact_camera(), None, fc.band_u16(6, 32, 24).reshape(-1), None, 0))
    n_good = len(cases)
    cam, flat = dc.exact_camera(13, 7), fc.band_u16(5, 13, 7).reshape(-1)
    for change in (dict(radius=0), dict(radius=4), dict(min_support=0), dict(radius=3, min_support=49), dict(edge_abs=np.nan), dict(edge_rel=-1.0)):
        cases.append((cam, fc.spec_of(**dict(EXACT_FILTER, **change)), flat, 91, 0))
    for null in (1, 2, 4, 8, 16):
        cases.append((cam, wide, flat, 91, null))
    cases.append((cam, wide, flat, 90, 0))
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(cases)) + b"".join(_pack_case(c, f, im, visited_of(c) if cap is None else cap, null) for c, f, im, cap, null in cases))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "depth_filter_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off, n_ok = fout.read_bytes(), 0, 0
    for cam, filt, im, cap, null in cases:
        rc, n_valid, n_rejected, written = struct.unpack_from("<iqqq", raw, off)
        off += 28
        got = np.frombuffer(raw, F32, written * 3, off).reshape(-1, 3)
        off += written * 12
        want_rc, want_valid, want_rejected, want = call(lib, cam, filt, np.ascontiguousarray(im), cap, null)
        assert rc == want_rc
        if rc == 0:
            assert (n_valid, n_rejected) == (want_valid, 0 if filt is None else want_rejected) and same_bits(got, want)
            n_ok += 1
        else:
            assert written == 0 and n_valid == -1 and n_rejected == -1
    assert off == len(raw) and n_ok == n_good
