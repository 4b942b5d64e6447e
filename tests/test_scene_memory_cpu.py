"""The definition of the scene memory of the depth route on the host (include/omds.h: omds_depth_scene_memory; no context, no GPU)
against the numpy restatement of the header's text in tests/scene_memory_cases.py.

Every case runs on the EXACT camera of tests/depth_cases.py (power-of-two fx, fy, integer cx, cy, R a signed permutation, t and the
grids on a binary lattice, depths on the 2^-10 lattice).  There the rotated coordinates xc, yc, zc and the cell centres are float32
values before any rounding (asserted: the restatement reports every fmaf whose float64 value was not), every other line of step 3 is
one float32 operation that numpy restates, and uf, vf are one rounding of an exact float64 sum -- so the library's words must be the
restatement's, bit for bit, and the counts equal.  Each case also asserts what it is about in plain terms.

The same cases go through a stand-alone build of the definition under AddressSanitizer + UBSan (tests/scene_memory_host.cpp; every
image at exactly (H - 1) pitch + W elements, both word arrays at exactly the grid's cells), whose output must be the library's."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import scene_memory_cases as sm
from depth_cases import F32, FLT, U16
from helpers import sanitized_host_program

ERR_INVALID_ARG = 1
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def call(lib, spec, mem, cams, images, mem_in=None, n_cams=None, null=0):
    """(rc, words [cells], counts) of the raw entry point; a refused call must write nothing.  null: 1 mem_spec, 2 mem_out, 4 counts"""
    from optimalmodulationds_amd import _lib as L
    n = len(cams)
    table = (L.OmdsDepthCamera * max(n, 1))(*cams)
    keep = [np.ascontiguousarray(im) for im in images]
    addrs = (C.c_void_p * max(n, 1))(*[k.ctypes.data for k in keep])
    cells = sm.n_cells_of(spec)
    out, counts = np.full(cells, SENTINEL, np.uint32), np.full(4, -7, np.int32)
    src = None if mem_in is None else np.ascontiguousarray(mem_in, np.uint32)
    rc = lib.omds_depth_scene_memory(C.byref(spec), None if null & 1 else C.byref(mem), table, addrs, n if n_cams is None else n_cams,
                                     None if src is None else src.ctypes.data, None if null & 2 else out.ctypes.data,
                                     None if null & 4 else counts.ctypes.data)
    if rc != 0:
        assert (out == SENTINEL).all() and (counts == -7).all(), "a refused call must write nothing"
    return rc, out, tuple(int(v) for v in counts)


def check(lib, spec, mem, cams, images, mem_in=None):
    """the library against the restatement, with the exact case's precondition; -> (words, counts)"""
    inexact = []
    want, want_counts = sm.restate(spec, mem, cams, images, mem_in, inexact)
    assert not inexact, f"exact case: {sorted(set(inexact))} are not float32 everywhere"
    cells = np.nonzero(want != 0)[0] if mem_in is None else np.nonzero((want != 0) | (np.asarray(mem_in) != 0))[0]
    assert sm.is_f32((np.stack([cells % spec.dims[0], (cells // spec.dims[0]) % spec.dims[1], cells // (spec.dims[0] * spec.dims[1])], 1) + 0.5)
                     * np.float64(spec.voxel) + np.array(list(spec.origin), np.float64)), "exact case: a cell centre is not a float32"
    for c in cams:
        assert all(np.frexp(abs(v))[0] == 0.5 for v in (c.fx, c.fy)) and float(c.cx).is_integer() and float(c.cy).is_integer()
    rc, got, counts = call(lib, spec, mem, cams, images, mem_in)
    assert rc == 0 and np.array_equal(got, want), f"{int((got != want).sum())} words differ from the restatement"
    assert counts == want_counts, (counts, want_counts)
    return got, counts


def wall_memory(lib, spec, mem, cam, border=2):
    """the memory after one frame of the wall at 2 m: every wall cell seen"""
    m, counts = check(lib, spec, mem, [cam], [sm.frame(cam, 2.0, border)])
    assert counts[0] == int((m == 1).sum()) > 20 and counts[1:] == (0, 0, 0)
    return m


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [U16, FLT])
def test_occluded_wall_cells_are_remembered(lib, fmt):
    spec, mem, cam = sm.grid(), sm.mem_of(), sm.exact_cam(fmt)
    m1 = wall_memory(lib, spec, mem, cam)
    wall = sm.frame(cam, 2.0, 2)
    m2, counts = check(lib, spec, mem, [cam], [sm.put(wall, cam, 1.0, slice(None), slice(0, 16))], m1)
    was = m1 != 0
    assert counts[2] == 0 and counts[3] == 0 and counts[1] > 5, counts
    assert ((m2[was] == 1) | (m2[was] == 2)).all(), "a wall cell is either seen or remembered with age 1"
    assert (m2[was] == 2).sum() == counts[1] and 0 < (m2[was] == 1).sum()
    p = sm.project(cam, sm.centres_of(spec, np.nonzero(was & (m2 == 2))[0]))
    assert (p["ju"] < 17).all(), "the remembered cells lie behind the plate (columns 0 .. 15, give or take the cell's width)"
    plate = (m2 != 0) & ~was
    assert plate.any() and (m2[plate] == 1).all(), "the plate's own cells are seen"


@pytest.mark.parametrize("fmt,blind", [(U16, 0), (FLT, np.nan), (FLT, np.inf)])
def test_no_return_keeps_everything(lib, fmt, blind):
    spec, mem, cam = sm.grid(), sm.mem_of(), sm.exact_cam(fmt)
    m1 = wall_memory(lib, spec, mem, cam)
    img = np.full((cam.height, cam.width), blind, np.uint16 if fmt == U16 else F32)
    m2, counts = check(lib, spec, mem, [cam], [img], m1)
    assert counts == (0, int((m1 != 0).sum()), 0, 0) and np.array_equal(m2, np.where(m1 != 0, 2, 0))


@pytest.mark.parametrize("far", [3.0, 4.5])
def test_seen_through_clears_every_wall_cell(lib, far):
    """a return at 3 m, and one beyond z_max = 4 m (not gated: still a return from behind the cell)"""
    spec, mem, cam = sm.grid(), sm.mem_of(), sm.exact_cam()
    m1 = wall_memory(lib, spec, mem, cam)
    m2, counts = check(lib, spec, mem, [cam], [sm.frame(cam, far)], m1)
    assert counts == (0, 0, int((m1 != 0).sum()), 0) and not m2.any()


def one_cell(spec, cell, word=1):
    m = np.zeros(sm.n_cells_of(spec), np.uint32)
    m[cell] = word
    return m


def test_clear_margin_boundary(lib):
    """a return exactly at lim = zc + clear_margin keeps the cell, one ulp farther clears it"""
    spec, mem, cam = sm.grid(), sm.mem_of(clear_margin=0.4375), sm.exact_cam(FLT)
    cell = sm.cell_index(spec, 9, 5, 4)
    zc = sm.project(cam, sm.centres_of(spec, [cell]))["zc"][0]
    lim = F32(zc + F32(0.4375))
    assert zc == F32(2.0625) and lim == F32(2.5)
    m = one_cell(spec, cell)
    at, _ = check(lib, spec, mem, [cam], [sm.frame(cam, lim)], m)
    beyond, counts = check(lib, spec, mem, [cam], [sm.frame(cam, np.nextafter(lim, F32(9)))], m)
    assert at[cell] == 2 and beyond[cell] == 0 and counts[2] == 1
    default = sm.mem_of()                      # <= 0: the grid's sphere radius
    r = F32(0.8660254) * F32(0.125)
    at, _ = check(lib, spec, default, [cam], [sm.frame(cam, F32(zc + r))], m)
    beyond, _ = check(lib, spec, default, [cam], [sm.frame(cam, np.nextafter(F32(zc + r), F32(9)))], m)
    assert at[cell] == 2 and beyond[cell] == 0


def test_out_of_view_cells_are_kept(lib):
    """behind the camera, beyond z_max, projecting to ju == nu exactly: SILENT, although every pixel returns from far behind"""
    spec = sm.grid(dict(origin=(-0.75, -1.125, -0.25), voxel=0.125, dims=(48, 11, 9)))
    mem, cam = sm.mem_of(), sm.exact_cam()
    every = np.arange(sm.n_cells_of(spec))
    p = sm.project(cam, sm.centres_of(spec, every))
    behind = every[(p["zc"] < 0) & (np.abs(p["xc"]) < 0.1)][0]
    beyond = every[(p["zc"] > 4.0) & (np.abs(p["xc"]) < 0.1) & (np.abs(p["yc"]) < 0.1)][0]
    rim = every[p["gate"] & (p["ju"] == 32) & (p["jv"] >= 0) & (p["jv"] < 24)][0]
    control = every[p["gate"] & p["inside"] & (p["zc"] < 3.0)][0]
    m = np.zeros(len(every), np.uint32)
    m[[behind, beyond, rim, control]] = [1, 5, 7, 3]
    out, counts = check(lib, spec, mem, [cam], [sm.frame(cam, 3.5)], m)
    seen = out == 1
    assert not seen[[behind, beyond, rim, control]].any()
    assert list(out[[behind, beyond, rim, control]]) == [2, 6, 8, 0] and counts[1:] == (3, 1, 0)


@pytest.mark.parametrize("step,cell_yz,pixel", [(1, (1, 0), (30, 22)), (1, (2, 1), (26, 20)), (3, (5, 3), (4, 6)), (3, (2, 6), (8, 4))])
def test_rint_ties_go_to_the_even_pixel(lib, step, cell_yz, pixel):
    """uf * istep and vf * istep land on k + 0.5 exactly; the even pixel is read: it alone returns from behind, its neighbours block"""
    spec = sm.grid(dict(origin=(1.1875, -1.125 + 1 / 64, -0.25 + 1 / 32), voxel=0.125, dims=(13, 11, 9)))
    mem, cam = sm.mem_of(), sm.exact_cam(step=step)
    cell = sm.cell_index(spec, 8, *cell_yz)
    p = sm.project(cam, sm.centres_of(spec, [cell]))
    assert p["zc"][0] == 2.0 and p["us"][0] % 1 == 0.5 and p["vs"][0] % 1 == 0.5, (p["us"], p["vs"])
    assert (p["ju"][0], p["jv"][0]) == pixel and pixel[0] % 2 == 0 and pixel[1] % 2 == 0
    assert {np.floor(p["us"][0]), np.floor(p["vs"][0])} <= {pixel[0], pixel[0] - 1, pixel[1], pixel[1] - 1}
    img = sm.frame(cam, 1.0)
    img[pixel[1] * step, pixel[0] * step] = 3584
    out, counts = check(lib, spec, mem, [cam], [img], one_cell(spec, cell))
    assert out[cell] == 0 and counts[2] == 1, "the even pixel was not the one read"
    for du, dv in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        img = sm.frame(cam, 1.0)
        img[(pixel[1] + dv) * step, (pixel[0] + du) * step] = 3584
        out, _ = check(lib, spec, mem, [cam], [img], one_cell(spec, cell))
        assert out[cell] == 2, (du, dv)


def test_two_cameras_one_free_verdict_clears(lib):
    spec, mem, cam = sm.grid(), sm.mem_of(), sm.exact_cam()
    m1 = wall_memory(lib, spec, mem, cam)
    occluded, through = sm.frame(cam, 1.0), sm.frame(cam, 3.0)
    a, ca = check(lib, spec, mem, [cam, cam], [occluded, through], m1)
    b, cb = check(lib, spec, mem, [cam, cam], [through, occluded], m1)
    was = m1 != 0
    assert np.array_equal(a, b) and ca == cb and ca[2] == int(was.sum()) and not a[was].any()
    only, c1 = check(lib, spec, mem, [cam], [occluded], m1)
    assert c1[2] == 0 and (only[was] == 2).all()


def test_footprint(lib):
    """one nearer pixel on the window's rim keeps the cell that footprint 0 clears; a window over the image edge uses its inside pixels"""
    spec, cam = sm.grid(), sm.exact_cam()
    cell = sm.cell_index(spec, 9, 5, 4)
    p = sm.project(cam, sm.centres_of(spec, [cell]))
    ju, jv = int(p["ju"][0]), int(p["jv"][0])
    assert 2 <= ju < 30 and 2 <= jv < 22
    m = one_cell(spec, cell)
    img = sm.frame(cam, 3.5)
    img[jv + 1, ju - 1] = 1024                    # a corner of the 3 x 3 window
    out0, _ = check(lib, spec, sm.mem_of(footprint=0), [cam], [img], m)
    out1, _ = check(lib, spec, sm.mem_of(footprint=1), [cam], [img], m)
    assert out0[cell] == 0 and out1[cell] == 2
    img[jv + 1, ju - 1] = 3584
    img[jv + 2, ju] = 1024                        # outside the 3 x 3 window, inside the 5 x 5
    out1, _ = check(lib, spec, sm.mem_of(footprint=1), [cam], [img], m)
    out2, _ = check(lib, spec, sm.mem_of(footprint=2), [cam], [img], m)
    assert out1[cell] == 0 and out2[cell] == 2
    every = np.arange(sm.n_cells_of(spec))
    q = sm.project(cam, sm.centres_of(spec, every))
    corner = every[q["gate"] & (q["ju"] == 0) & (q["jv"] >= 0) & (q["jv"] < 24)]
    assert len(corner), "no cell projects to the first column"
    edge = corner[0]
    out3, c3 = check(lib, spec, sm.mem_of(footprint=3), [cam], [sm.frame(cam, 3.9)], one_cell(spec, edge))
    assert out3[edge] == 0 and c3[2] == 1, "the part of the window past the image edge is not a verdict against the cell"


def test_expiry(lib):
    spec, cam = sm.grid(), sm.exact_cam()
    blind = sm.frame(cam, None)
    m = wall_memory(lib, spec, sm.mem_of(max_age=2), cam)
    n = int((m != 0).sum())
    for unseen, want in ((1, 2), (2, 3), (3, 0)):
        m, counts = check(lib, spec, sm.mem_of(max_age=2), [cam], [blind], m)
        assert counts == ((0, n, 0, 0) if want else (0, 0, 0, n)) and int((m == want).sum()) == (n if want else sm.n_cells_of(spec)), unseen
    m = wall_memory(lib, spec, sm.mem_of(max_age=0), cam)
    for word in (2, 3, 4, 5):
        m, counts = check(lib, spec, sm.mem_of(max_age=0), [cam], [blind], m)
        assert counts == (0, n, 0, 0) and int((m == word).sum()) == n
    top = one_cell(spec, 5, 0xFFFFFFFF)
    m, _ = check(lib, spec, sm.mem_of(max_age=-3), [cam], [blind], top)
    assert m[5] == 0xFFFFFFFF, "the word saturates"
    m, counts = check(lib, spec, sm.mem_of(max_age=1), [cam], [blind], one_cell(spec, 5, 1))
    assert m[5] == 2 and counts[1] == 1
    m, counts = check(lib, spec, sm.mem_of(max_age=1), [cam], [blind], m)
    assert m[5] == 0 and counts[3] == 1


def test_min_points_and_in_place(lib):
    """a cell with fewer than min_points points is not seen: it is asked like any remembered cell; mem_out may be mem_in"""
    cam = sm.exact_cam()
    spec1, spec9 = sm.grid(), sm.grid(min_points=8)      # 4 columns x 2 rows of pixels per interior wall cell, fewer at the rim
    m1 = wall_memory(lib, spec1, sm.mem_of(), cam)
    wall = sm.frame(cam, 2.0, 2)
    m9, counts = check(lib, spec9, sm.mem_of(), [cam], [wall], m1)
    assert 0 < counts[0] < int((m1 != 0).sum()) and counts[2] == 0 and counts[1] == int((m1 != 0).sum()) - counts[0]
    from optimalmodulationds_amd import _lib as L
    buf = m1.copy()
    table, addrs = (L.OmdsDepthCamera * 1)(cam), (C.c_void_p * 1)(wall.ctypes.data)
    assert lib.omds_depth_scene_memory(C.byref(spec9), C.byref(sm.mem_of()), table, addrs, 1, buf.ctypes.data, buf.ctypes.data, None) == 0
    assert np.array_equal(buf, m9)


def test_python_wrapper_is_the_raw_call(lib):
    from optimalmodulationds_amd.engine import depth_scene_memory
    spec, mem, cam = sm.grid(), sm.mem_of(2, 0.2, 1), sm.exact_cam()
    seq = sm.sequence(cam)
    m = None
    for img in seq:
        rc, want, counts = call(lib, spec, mem, [cam], [img], m)
        got, got_counts = depth_scene_memory(img, cam, spec, mem, m)
        assert rc == 0 and np.array_equal(got, want) and got_counts == counts and got.dtype == np.uint32
        m = want
    with pytest.raises(ValueError):
        depth_scene_memory(seq[0], cam, spec, mem, np.zeros(5, np.uint32))


def _refusals():
    spec, cam = sm.grid(), sm.exact_cam()
    img = sm.frame(cam, 2.0)
    ok = dict(spec=spec, mem=sm.mem_of(), cams=[cam], images=[img], mem_in=None, n_cams=None, null=0)
    bad_spec = sm.grid(dict(sm.GRID_SMALL, voxel=0.0))
    bad_cam = sm.exact_cam()
    bad_cam.fx = 0.0
    return ok, [dict(ok, mem=sm.mem_of(footprint=4)), dict(ok, mem=sm.mem_of(footprint=-1)), dict(ok, mem=sm.mem_of(clear_margin=np.nan)),
                dict(ok, null=2), dict(ok, null=1), dict(ok, n_cams=0), dict(ok, n_cams=9), dict(ok, spec=bad_spec), dict(ok, cams=[bad_cam])]


def test_refusals_write_nothing(lib):
    ok, bad = _refusals()
    assert call(lib, **ok)[0] == 0 and call(lib, **dict(ok, null=4))[0] == 0      # counts_out may be NULL
    for case in bad:
        assert call(lib, **case)[0] == ERR_INVALID_ARG, case
    assert b"depth image" in lib.omds_last_error(None)
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import depth_scene_memory
    with pytest.raises(_lib.OmdsError):
        depth_scene_memory(ok["images"][0], ok["cams"][0], ok["spec"], sm.mem_of(footprint=4))


# ---- the sanitizer leg -------------------------------------------------------------------------------------------------------------
def _pack(case):
    spec, cams, images = case["spec"], case["cams"], case["images"]
    cells = sm.n_cells_of(spec)
    m = case.get("mem_in")
    raw = bytes(spec) + bytes(case["mem"]) + struct.pack("<iiiqi", len(cams) if case.get("n_cams") is None else case["n_cams"], len(cams),
                                                         case.get("null", 0), cells, 0 if m is None else 1)
    if m is not None:
        raw += np.ascontiguousarray(m, np.uint32).tobytes()
    for cam, img in zip(cams, images):
        flat = np.ascontiguousarray(img).reshape(-1)
        raw += bytes(cam) + struct.pack("<iq", flat.itemsize, flat.size) + flat.tobytes()
    return raw


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    exe = sanitized_host_program("scene_memory_host", tmp_path)
    cases = []
    for fmt in (U16, FLT):
        spec, cam = sm.grid(), sm.exact_cam(fmt)
        for mem in (sm.mem_of(), sm.mem_of(2, 0.3, 1), sm.mem_of(1, 0.0, 3)):
            m = None
            for img in sm.sequence(cam) + [sm.frame(cam, None)] * 2:
                cases.append(dict(spec=spec, mem=mem, cams=[cam], images=[img], mem_in=m))
                m = call(lib, spec, mem, [cam], [img], m)[1]
    spec = sm.grid(dict(origin=(-0.75, -1.125, -0.25), voxel=0.125, dims=(48, 11, 9)))       # cells behind the camera and past its range
    cam3 = sm.exact_cam(step=3)
    cases.append(dict(spec=spec, mem=sm.mem_of(footprint=3), cams=[sm.exact_cam(), cam3], images=[sm.frame(cam3, 3.5), sm.frame(cam3, 3.9)],
                      mem_in=np.full(sm.n_cells_of(spec), 3, np.uint32)))
    import depth_cases as dc
    from optimalmodulationds_amd.engine import depth_points
    gen = dc.general_camera(FLT, 33, 17)                  # a general camera: not restated, but the two builds must agree on it too
    img = dc.general_image(7, FLT, 33, 17)
    gspec = sm.grid_around(depth_points(img, gen)[0], 0.125, (13, 11, 9))
    cases.append(dict(spec=gspec, mem=sm.mem_of(footprint=2), cams=[gen], images=[img], mem_in=np.full(sm.n_cells_of(gspec), 1, np.uint32)))
    ok, bad = _refusals()
    cases += bad
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(cases)) + b"".join(_pack(c) for c in cases))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scene_memory_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off, n_ok = fout.read_bytes(), 0, 0
    for case in cases:
        rc, c0, c1, c2, c3, written = struct.unpack_from("<iiiiiq", raw, off)
        off += 28
        got = np.frombuffer(raw, np.uint32, written, off)
        off += written * 4
        want_rc, want, want_counts = call(lib, case["spec"], case["mem"], case["cams"], case["images"], case.get("mem_in"), case.get("n_cams"),
                                          case.get("null", 0))
        assert rc == want_rc
        if rc == 0:
            assert np.array_equal(got, want) and (c0, c1, c2, c3) == want_counts
            n_ok += 1
        else:
            assert written == 0 and (c0, c1, c2, c3) == (-7, -7, -7, -7)
    assert off == len(raw) and n_ok == len(cases) - len(bad) == 44
