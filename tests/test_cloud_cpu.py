"""The definition of the obstacle spheres of a point cloud on the host (include/omds.h: omds_point_cloud_spheres; no context, no
GPU) against a numpy restatement of the header's text: crop by floorf((p - origin) * inv) compared as floats, count per cell, the
occupied cells in ascending cell order, centres (i + 0.5) * voxel + origin.

Where the arithmetic is exact (voxel = 2^-4, origin a multiple of it, points on a 2^-10 lattice) everything matches bit for bit.
With voxel = 0.05 the cells and their order are still exact (both sides round p - origin, then the product, then floor); the centres
are compared within 1 ulp, because numpy has no fused multiply-add.  Within 1 ulp of WHAT matters there: float32 numpy rounds
(i + 0.5) * voxel before it adds origin, and where the sum cancels (a centre near 0 in a box that starts at -0.8) that half ulp of
the product is tens of ulps of the centre -- the two-rounding float32 form is itself that far from the header's fmaf.  So the
restatement forms the centre in float64 (the product of two float32 is exact there, the sum is rounded at 2^-53) and the library's
float32 centre must lie within 1 float32 ulp of it.

The same edge cases also go through a stand-alone build of the definition under AddressSanitizer + UBSan (tests/cloud_host.cpp, its
buffers allocated at exactly the sizes passed), whose output must be the library's bit for bit."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

from cloud_cases import F32, cells_of, edge_points, lattice_cloud, restate, spec_of
from helpers import sanitized_host_program

ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def call(lib, spec, pts, cap=None):
    """(rc, count, spheres [min(count, cap) if rc == 0 else 0, 4]) of the raw entry point"""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
    cap = 4096 if cap is None else cap
    out, cnt = np.full((max(cap, 1), 4), -7.0, F32), np.full(1, -1, np.int32)
    rc = lib.omds_point_cloud_spheres(C.byref(spec), pts.ctypes.data if pts.size else None, pts.shape[0], out.ctypes.data, cap,
                                      cnt.ctypes.data)
    if rc != 0:
        assert (out == F32(-7)).all(), "a refused call must write no sphere"
    return rc, int(cnt[0]), out[:int(cnt[0])].copy() if rc == 0 else out[:0]


def test_exact_arithmetic_case_matches_the_restatement_bit_for_bit(lib):
    spec = spec_of((-0.5, -0.25, 0.0), 0.0625, (16, 12, 8))
    pts = np.concatenate([lattice_cloud(1, 3000, -0.7, 1.1), edge_points(spec)])
    rc, count, got = call(lib, spec, pts)
    occ, want, _ = restate(spec, pts)
    assert rc == 0 and count == len(occ) and 100 < count <= 16 * 12 * 8
    assert np.array_equal(cells_of(spec, got), occ), "cells or their order"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "centres / radii are not the restatement's bits"
    assert (got[:, 3] == F32(0.8660254) * F32(0.0625)).all()


def test_non_dyadic_case_cells_exact_centres_within_one_ulp(lib):
    spec = spec_of((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), radius=0.04, max_spheres=8192)
    rng = np.random.RandomState(2)
    pts = np.concatenate([rng.uniform(-1.0, 1.0, (5000, 3)).astype(F32), edge_points(spec)])
    rc, count, got = call(lib, spec, pts, cap=8192)
    occ, _, want64 = restate(spec, pts)
    assert rc == 0 and count == len(occ) > 1000
    assert np.array_equal(cells_of(spec, got), occ), "cells or their order"
    ulp = np.spacing(np.abs(got[:, :3])).astype(np.float64)
    assert (np.abs(got[:, :3].astype(np.float64) - want64) <= ulp).all(), "a centre is more than 1 ulp from (i + 0.5) * voxel + origin"
    assert (got[:, 3] == F32(0.04)).all()


@pytest.mark.parametrize("dims", [(6, 5, 4), (37, 29, 1)])
@pytest.mark.parametrize("min_points", [1, 3])
def test_edge_cases(lib, dims, min_points):
    """faces, upper faces, non-finite coordinates, points outside, duplicates -- counted by hand and against the restatement"""
    spec = spec_of((-0.5, 0.25, 1.0), 0.0625, dims, radius=-1.0, min_points=min_points)
    pts = edge_points(spec)
    rc, count, got = call(lib, spec, pts)
    occ, want, _ = restate(spec, pts)
    assert rc == 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert int(np.prod(dims)) - 1 in occ, "three copies of one point occupy the last cell at either threshold"
    if min_points == 1:
        assert 0 in occ and count >= 3
    else:
        assert count < call(lib, spec_of((-0.5, 0.25, 1.0), 0.0625, dims, radius=-1.0, min_points=1), pts)[1]
    assert (got[:, 3] == F32(0.8660254) * F32(0.0625)).all(), "radius <= 0 selects the circumsphere"
    # no sphere outside the box
    o, top = np.array(list(spec.origin), F32), np.array(list(spec.origin), F32) + F32(0.0625) * np.array(dims, F32)
    assert (got[:, :3] > o).all() and (got[:, :3] < top).all()
    # any order of the input gives the identical list
    rc2, _, got2 = call(lib, spec, pts[np.random.RandomState(5).permutation(len(pts))])
    assert rc2 == 0 and np.array_equal(got2.view(np.uint32), got.view(np.uint32))


def test_upper_faces_and_non_finite_points_alone_give_nothing(lib):
    spec = spec_of((0.0, 0.0, 0.0), 0.25, (4, 4, 4))
    pts = np.array([[1.0, 0.1, 0.1], [0.1, 1.0, 0.1], [0.1, 0.1, 1.0], [np.inf, 0.1, 0.1], [0.1, -np.inf, 0.1], [0.1, 0.1, np.nan],
                    [-1e-30, 0.1, 0.1], [5.0, 5.0, 5.0]], F32)
    assert call(lib, spec, pts)[:2] == (0, 0)
    pts[0, 0] = np.nextafter(F32(1.0), F32(0))          # the last float below the upper face: cell (3, 0, 0)
    rc, count, got = call(lib, spec, pts)
    assert (rc, count) == (0, 1) and np.array_equal(got[0], np.array([0.875, 0.125, 0.125, 0.8660254 * 0.25], F32))


def test_duplicates_and_min_points(lib):
    pts = np.array([[0.1, 0.1, 0.1]] * 3 + [[0.6, 0.1, 0.1]] * 2 + [[0.1, 0.6, 0.1]], F32)
    for mp, cells in ((1, [0, 1, 2]), (3, [0]), (0, [0, 1, 2]), (-4, [0, 1, 2]), (4, [])):
        spec = spec_of((0.0, 0.0, 0.0), 0.5, (2, 2, 2), min_points=mp)
        rc, count, got = call(lib, spec, pts)
        assert rc == 0 and list(cells_of(spec, got)) == cells, mp


def test_no_points(lib):
    spec = spec_of((0.0, 0.0, 0.0), 0.5, (2, 2, 2))
    assert call(lib, spec, np.zeros((0, 3), F32))[:2] == (0, 0)


def test_errors(lib):
    spec = spec_of((0.0, 0.0, 0.0), 0.0625, (16, 16, 16), max_spheres=50)
    pts = lattice_cloud(3, 2000, 0.0, 1.0)
    occ, _, _ = restate(spec, pts)
    assert len(occ) > 1000
    rc, count, got = call(lib, spec, pts)                            # occupied > max_spheres
    assert rc == ERR_INVALID_ARG and count == len(occ) and len(got) == 0
    assert b"max_spheres" in lib.omds_last_error(None)
    big = spec_of((0.0, 0.0, 0.0), 0.0625, (16, 16, 16), max_spheres=65536)
    rc, count, _ = call(lib, big, pts, cap=len(occ) - 1)              # occupied > cap
    assert rc == ERR_INVALID_ARG and count == len(occ)
    rc, count, got = call(lib, big, pts, cap=len(occ))                # ... and exactly cap fits
    assert rc == 0 and count == len(occ) == len(got)
    # null pointers
    out, cnt = np.zeros((8, 4), F32), np.zeros(1, np.int32)
    p8 = np.ascontiguousarray(pts[:8])
    assert lib.omds_point_cloud_spheres(None, p8.ctypes.data, 8, out.ctypes.data, 8, cnt.ctypes.data) == ERR_INVALID_ARG
    assert lib.omds_point_cloud_spheres(C.byref(big), None, 8, out.ctypes.data, 8, cnt.ctypes.data) == ERR_INVALID_ARG
    assert lib.omds_point_cloud_spheres(C.byref(big), p8.ctypes.data, 8, None, 8, cnt.ctypes.data) == ERR_INVALID_ARG
    assert lib.omds_point_cloud_spheres(C.byref(big), p8.ctypes.data, 8, out.ctypes.data, 8, None) == ERR_INVALID_ARG
    assert lib.omds_point_cloud_spheres(C.byref(big), p8.ctypes.data, -1, out.ctypes.data, 8, cnt.ctypes.data) == ERR_INVALID_ARG
    # the spec
    for bad in (spec_of((0, 0, 0), 0.0, (4, 4, 4)), spec_of((0, 0, 0), -0.1, (4, 4, 4)), spec_of((0, 0, 0), np.nan, (4, 4, 4)),
                spec_of((0, 0, 0), 0.1, (2048, 2048, 2)), spec_of((0, 0, 0), 0.1, (4, 0, 4)), spec_of((0, 0, 0), 0.1, (4, 4, 4), max_spheres=65537),
                spec_of((np.inf, 0, 0), 0.1, (4, 4, 4))):
        assert call(lib, bad, p8, cap=8)[0] == ERR_INVALID_ARG
    assert call(lib, spec_of((0, 0, 0), 0.1, (2048, 2048, 1), max_spheres=65536), p8, cap=8)[0] == 0      # exactly 2^22 cells


def test_python_wrapper_raises_with_the_count(lib):
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import point_cloud_spheres
    pts = lattice_cloud(3, 500, 0.0, 1.0)
    got = point_cloud_spheres(pts, spec_of((0.0, 0.0, 0.0), 0.25, (4, 4, 4)))
    assert got.shape == (64, 4)
    with pytest.raises(_lib.OmdsError) as e:
        point_cloud_spheres(pts, spec_of((0.0, 0.0, 0.0), 0.25, (4, 4, 4), max_spheres=10))
    assert e.value.n_occupied == 64


def _pack_case(spec, pts, cap, null_mask=0):
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
    return bytes(spec) + struct.pack("<qii", pts.shape[0], cap, null_mask) + pts.tobytes()


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    """tests/cloud_host.cpp, a stand-alone program around the header both the library and its kernels include, built with
    -fsanitize=address,undefined and run on the edge cases above: a clean exit, and the library's bits."""
    exe = sanitized_host_program("cloud_host", tmp_path)
    cases = []
    for dims in ((6, 5, 4), (37, 29, 1)):
        for mp in (1, 3):
            s = spec_of((-0.5, 0.25, 1.0), 0.0625, dims, radius=-1.0, min_points=mp)
            cases.append((s, edge_points(s), 4096, 0))
    s = spec_of((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), max_spheres=8192)
    cloud = np.concatenate([np.random.RandomState(2).uniform(-1.0, 1.0, (5000, 3)).astype(F32), edge_points(s)])
    cases.append((s, cloud, 8192, 0))
    cases.append((s, cloud[::-1], len(restate(s, cloud)[0]), 0))                   # exactly cap: the last sphere ends the buffer
    cases.append((s, cloud, 100, 0))                                               # occupied > cap: nothing written
    cases.append((spec_of((0, 0, 0), 0.0625, (16, 16, 16), max_spheres=50), lattice_cloud(3, 2000, 0.0, 1.0), 4096, 0))
    cases.append((s, np.zeros((0, 3), F32), 0, 0))                                 # no points, no room
    for mask in (1, 2, 4, 8):
        cases.append((s, cloud[:16], 16, mask))
    cases.append((spec_of((0, 0, 0), 0.1, (2048, 2048, 2)), cloud[:16], 16, 0))
    cases.append((spec_of((0, 0, 0), 0.1, (2048, 2048, 1), max_spheres=65536), cloud[:16], 16, 0))
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(cases)) + b"".join(_pack_case(*c) for c in cases))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cloud_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off = fout.read_bytes(), 0
    for spec, pts, cap, mask in cases:
        rc, count, written = struct.unpack_from("<iii", raw, off)
        off += 12
        got = np.frombuffer(raw, F32, written * 4, off).reshape(-1, 4)
        off += written * 16
        if mask:
            assert rc == ERR_INVALID_ARG
            continue
        want_rc, want_count, want = call(lib, spec, pts, cap)
        assert (rc, count) == (want_rc, want_count)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert off == len(raw)
