"""The definition of the object velocities of two successive point clouds on the host (include/omds.h: omds_point_cloud_object_flow;
no context, no GPU) against the numpy restatement of the header's text in tests/cloud_object_cases.py: labels, flags and counts
exactly, velocities bit for bit, the fallback that of omds_point_cloud_flow.

The same cases also go through a stand-alone build of the definition under AddressSanitizer + UBSan (tests/cloud_objects_host.cpp,
its buffers allocated at exactly the sizes passed), whose output must be the library's bit for bit."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import cloud_object_cases as cases
from cloud_cases import F32, spec_of
from cloud_object_cases import obj_of, restate_objects, track_of
from helpers import sanitized_host_program

ERR_INVALID_ARG = 1
SENTINEL = F32(-7)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _u8(k):
    return None if k is None else np.ascontiguousarray(np.asarray(k) != 0, np.uint8)


def call(lib, spec, track, obj, prev, now, keep_prev=None, keep_now=None, cap=65536):
    """(rc, count, matched, n_objects, n_accepted, spheres, vel, label, object) of the raw entry point; a refused call must have
    written nothing but the count"""
    prev, now = (np.ascontiguousarray(p, F32).reshape(-1, 3) for p in (prev, now))
    kp, kn = _u8(keep_prev), _u8(keep_now)
    n = max(cap, 1)
    out, vel = np.full((n, 4), SENTINEL, F32), np.full((n, 3), SENTINEL, F32)
    label, flag = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    cnt, matched, n_obj, n_acc = (np.full(1, -1, np.int32) for _ in range(4))
    rc = lib.omds_point_cloud_object_flow(C.byref(spec), C.byref(track), C.byref(obj), prev.ctypes.data if prev.size else None, prev.shape[0],
                                          kp.ctypes.data if kp is not None and kp.size else None, now.ctypes.data if now.size else None,
                                          now.shape[0], kn.ctypes.data if kn is not None and kn.size else None, out.ctypes.data,
                                          vel.ctypes.data, label.ctypes.data, flag.ctypes.data, cap, cnt.ctypes.data, matched.ctypes.data,
                                          n_obj.ctypes.data, n_acc.ctypes.data)
    if rc != 0:
        assert (out == SENTINEL).all() and (vel == SENTINEL).all() and (label == -7).all() and (flag == -7).all(), "a refused call must write nothing"
        assert matched[0] == -1 and n_obj[0] == -1 and n_acc[0] == -1
        return rc, int(cnt[0]), -1, -1, -1, out[:0], vel[:0], label[:0], flag[:0]
    w = int(cnt[0]) if kn is None else int(kn.sum())
    assert (out[w:] == SENTINEL).all() and (vel[w:] == SENTINEL).all() and (label[w:] == -7).all() and (flag[w:] == -7).all()
    return rc, int(cnt[0]), int(matched[0]), int(n_obj[0]), int(n_acc[0]), out[:w].copy(), vel[:w].copy(), label[:w].copy(), flag[:w].copy()


def check(lib, spec, track, obj, prev, now, keep_prev=None, keep_now=None):
    """the definition equals the restatement -> the restatement's dict"""
    from optimalmodulationds_amd.engine import point_cloud_spheres
    rc, count, matched, n_obj, n_acc, spheres, vel, label, flag = call(lib, spec, track, obj, prev, now, keep_prev, keep_now)
    want = restate_objects(spec, track, obj, prev, now, keep_prev, keep_now)
    assert rc == 0 and count == want["occupied"]
    all_spheres = point_cloud_spheres(now, spec, cap=65536)
    rows = np.arange(count) if keep_now is None else np.nonzero(np.asarray(keep_now) != 0)[0]
    assert np.array_equal(bits(spheres), bits(all_spheres[rows])), "the list is not the kept rows of omds_point_cloud_spheres(now)"
    assert np.array_equal(label, want["label"]), "labels"
    assert np.array_equal(flag, want["object"]), "object flags"
    assert (matched, n_obj, n_acc) == (want["matched"], want["n_objects"], want["n_accepted"])
    assert np.array_equal(bits(vel), bits(want["vel"])), "velocities are not the restatement's bits"
    want["spheres"] = spheres
    return want


def flow_vel(spec, track, prev, now):
    from optimalmodulationds_amd.engine import point_cloud_flow
    return point_cloud_flow(prev, now, spec, track, cap=65536)[1]


# ---- exact translation and the sliding plate -------------------------------------------------------------------------------------
def test_exact_translation_of_a_ball(lib):
    spec, prev, now = cases.ball()
    track = track_of(2, 0.125)
    r = check(lib, spec, track, obj_of(1, 4), prev, now)
    assert len(r["cells"]) == 27 and r["n_objects"] == r["n_accepted"] == 1 and r["matched"] == 27 and (r["object"] == 1).all()
    assert np.array_equal(bits(r["vel"]), bits(np.tile(np.array([1.125 * 0.0625 / 0.125, 0.0, 0.0], F32), (27, 1))))
    interior = list(r["cells"]).index((5 * 12 + 5) * 16 + 6)
    assert np.array_equal(bits(flow_vel(spec, track, prev, now)[interior]), np.zeros(3, np.uint32)), "the per-cell flow sees nothing in the interior"


def test_sliding_plate(lib):
    spec, prev, now = cases.plate()
    track = track_of(1, 0.125)
    r = check(lib, spec, track, obj_of(1, 4), prev, now)
    assert len(r["cells"]) == 36 and (r["object"] == 1).all() and len(set(r["label"])) == 1
    assert np.array_equal(bits(r["vel"]), bits(np.tile(np.array([0.5 * 0.0625 / 0.125, 0.0, 0.0], F32), (36, 1))))
    today = flow_vel(spec, track, prev, now)
    ix, iy = r["cells"] % 16, (r["cells"] // 16) % 12
    inner = (ix >= 4) & (ix <= 7) & (iy >= 4) & (iy <= 7)
    assert inner.sum() == 16 and not today[inner].any(), "motion along the plate is invisible to the per-cell flow"


# ---- connectivity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap,link,n_comp", [(-1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 2, 2), (0, 1, 1), (2, 1, 2)])
def test_connectivity(lib, gap, link, n_comp):
    spec, prev, now = cases.blobs(gap)
    r = check(lib, spec, track_of(1, 0.1), obj_of(link, 1), prev, now)
    assert len(r["cells"]) == 16 and len(set(r["label"])) == n_comp == r["n_objects"] == r["n_accepted"]
    assert r["label"].min() == r["cells"][0] and (r["object"] == 1).all()


def test_long_component(lib):
    spec, prev, now = cases.serpentine()
    r = check(lib, spec, track_of(1, 0.1), obj_of(1, 4), prev, now)
    assert len(r["cells"]) == 1008 and (r["label"] == 5).all() and r["cells"][0] == 5
    assert r["n_accepted"] == 1 and (r["object"] == 1).all() and not r["vel"].any()


# ---- grid faces ------------------------------------------------------------------------------------------------------------------
def test_components_in_all_eight_corners(lib):
    spec, prev, now = cases.corner_components()
    r = check(lib, spec, track_of(2, 0.25), obj_of(1, 2), prev, now)
    assert len(r["cells"]) == 16 and r["n_objects"] == 8 and len(set(r["label"])) == 8
    r2 = check(lib, spec, track_of(2, 0.25), obj_of(2, 2), prev, now)      # windows of 5 cells on axes of 6, 5 and 4: clipped everywhere
    assert r2["n_objects"] == 8, "the corners are three cells apart: no link of 2 joins them"


def test_flat_grid(lib):
    spec, prev, now = cases.random_pair(5, (37, 29, 1), 400, 400, shift=(1.6, -0.7, 0.0), fill=0.8)
    for link in (1, 2):
        r = check(lib, spec, track_of(3, 0.1), obj_of(link, 3), prev, now)
        assert r["n_objects"] >= 1 and len(r["cells"]) > 100


def test_window_wider_than_the_grid(lib):
    spec, prev, now = cases.random_pair(6, (3, 2, 5), 12, 25, shift=(0.0, 0.0, 0.0))
    r = check(lib, spec, track_of(4, 0.1), obj_of(2, 1), prev, now)
    assert r["n_objects"] >= 1
    spec, prev, now = cases.random_pair(6, (1, 1, 2), 6, 6, shift=(0.0, 0.0, 0.0))
    check(lib, spec, track_of(4, 0.1), obj_of(2, 1), prev, now)


# ---- the gates -------------------------------------------------------------------------------------------------------------------
def test_mass_gate_at_two_to_one(lib):
    r = check(lib, *cases.line_pair(4, 8)[:1], track_of(4, 0.1), obj_of(1, 4), *cases.line_pair(4, 8)[1:])
    assert r["n_objects"] == r["n_accepted"] == 1 and (r["object"] == 1).all() and (r["vel"][:, 0] > 0).all()
    r = check(lib, *cases.line_pair(4, 9)[:1], track_of(4, 0.1), obj_of(1, 4), *cases.line_pair(4, 9)[1:])
    assert r["n_objects"] == 1 and r["n_accepted"] == 0 and not r["object"].any()
    r = check(lib, *cases.line_pair(8, 4)[:1], track_of(4, 0.1), obj_of(1, 4), *cases.line_pair(8, 4)[1:])
    assert r["n_accepted"] == 1
    r = check(lib, *cases.line_pair(9, 4)[:1], track_of(4, 0.1), obj_of(1, 4), *cases.line_pair(9, 4)[1:])
    assert r["n_accepted"] == 0


def test_min_cells_one_below_and_at_the_size(lib):
    spec, prev, now = cases.line_pair(5, 5)
    now = (now + np.array([0.25 * 0.0625, 0, 0], F32)).astype(F32)
    r = check(lib, spec, track_of(1, 0.1), obj_of(1, 5), prev, now)
    assert r["n_objects"] == r["n_accepted"] == 1 and (r["object"] == 1).all()
    r = check(lib, spec, track_of(1, 0.1), obj_of(1, 6), prev, now)
    assert r["n_objects"] == 0 and not r["object"].any()
    spec, prev, _ = cases.line_pair(4, 5)              # the PREVIOUS component is one cell too small to be a candidate
    r = check(lib, spec, track_of(1, 0.1), obj_of(1, 5), prev, now)
    assert r["n_objects"] == 1 and r["n_accepted"] == 0
    for mc in (0, -3):                                  # < 1 -> 1
        assert check(lib, spec, track_of(1, 0.1), obj_of(1, mc), prev, now)["n_objects"] == 1


@pytest.mark.parametrize("kind,accepted", [("below", 1), ("at", 1), ("above", 0)])
def test_reach_gate_one_float64_step_either_side(lib, kind, accepted):
    spec, prev, now, dx = cases.reach_edge(kind)
    r = check(lib, spec, track_of(2, 0.1), obj_of(1, 1), prev, now)
    (_, N, Q), = r["tab_now"].values()
    (_, Np, Qp), = r["tab_prev"].values()
    assert np.float64(Q[0]) / np.float64(N) - np.float64(Qp[0]) / np.float64(Np) == dx and Q[1:] == Qp[1:]
    assert {"below": dx < 512, "at": dx == 512, "above": dx > 512}[kind] and abs(dx - 512) < 2e-13
    assert r["n_objects"] == 1 and r["n_accepted"] == accepted


def test_equidistant_candidates_the_smaller_label_wins(lib):
    spec, prev, now = cases.equidistant()
    r = check(lib, spec, track_of(1, 0.5), obj_of(1, 1), prev, now)
    assert r["n_accepted"] == 1 and np.array_equal(r["vel"][0], np.array([0.0625 / 0.5, 0, 0], F32)), "from the cell at x = 4: +x"


# ---- the fallback ----------------------------------------------------------------------------------------------------------------
def test_fallback_carries_the_per_cell_flow(lib):
    """a rejected match (mass gate), a small component, an object without any candidate and no previous cloud: omds_point_cloud_flow's bits"""
    for spec, prev, now, track, obj in ((*cases.line_pair(4, 9), track_of(4, 0.1), obj_of(1, 4)),
                                        (*cases.line_pair(4, 3), track_of(2, 0.1), obj_of(1, 4)),
                                        (*cases.reach_edge("above")[:3], track_of(2, 0.1), obj_of(1, 1)),
                                        (*cases.ball()[:2], np.zeros((0, 3), F32), track_of(2, 0.1), obj_of(1, 4))):
        prev, now = (now, prev) if len(now) == 0 else (prev, now)          # (the last case: no PREVIOUS cloud)
        r = check(lib, spec, track, obj, prev, now)
        assert not r["object"].any() and r["n_accepted"] == 0
        assert np.array_equal(bits(r["vel"]), bits(flow_vel(spec, track, prev, now)))
    spec, prev, now = cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7)
    r = check(lib, spec, track_of(2, 0.1), obj_of(1, 6), prev, now)          # a mixed scene: some of each
    today = flow_vel(spec, track_of(2, 0.1), prev, now)
    rest = r["object"] == 0
    assert rest.any() and np.array_equal(bits(r["vel"][rest]), bits(today[rest]))


# ---- other inputs and outputs ----------------------------------------------------------------------------------------------------
def test_still_applies_to_the_object_velocity(lib):
    spec, prev, now = cases.ball()
    v = F32(1.125 * 0.0625 / 0.125)
    r = check(lib, spec, track_of(2, 0.125, still=float(np.nextafter(v, F32(1)))), obj_of(1, 4), prev, now)
    assert r["n_accepted"] == 1 and r["matched"] == 27 and np.array_equal(bits(r["vel"]), np.zeros((27, 3), np.uint32))
    r = check(lib, spec, track_of(2, 0.125, still=float(v)), obj_of(1, 4), prev, now)
    assert (r["vel"][:, 0] == v).all()


def test_keep_now_cuts_a_bridge(lib):
    spec, prev, now = cases.bridge()
    whole = check(lib, spec, track_of(1, 0.1), obj_of(1, 4), prev, now)
    assert len(whole["cells"]) == 9 and len(set(whole["label"])) == 1
    keep = np.ones(9, np.uint8)
    keep[cases.bridge_row(spec)] = 0
    cut = check(lib, spec, track_of(1, 0.1), obj_of(1, 4), prev, now, keep_prev=keep, keep_now=keep)
    assert len(cut["cells"]) == 8 and len(set(cut["label"])) == 2 and cut["n_accepted"] == 2 and cut["occupied"] == 9
    half = check(lib, spec, track_of(1, 0.1), obj_of(1, 4), prev, now, keep_now=keep)       # two halves against the whole: 4 of 9 cells
    assert half["n_objects"] == 2 and half["n_accepted"] == 0


def test_keep_prev_removes_the_candidate_but_not_the_fallback(lib):
    spec, prev, now = cases.ball()
    track = track_of(2, 0.125)
    r = check(lib, spec, track, obj_of(1, 4), prev, now, keep_prev=np.zeros(27, np.uint8))
    assert r["n_objects"] == 1 and r["n_accepted"] == 0
    assert np.array_equal(bits(r["vel"]), bits(flow_vel(spec, track, prev, now))), "the fallback looks at the unmasked records"
    keep = np.ones(27, np.uint8)
    keep[:9] = 0                                                                             # the lowest layer: the centroid moves in z too
    r = check(lib, spec, track, obj_of(1, 4), prev, now, keep_prev=keep)
    assert r["n_accepted"] == 1 and (r["vel"][:, 2] < 0).all()


def test_empty_clouds_and_a_single_sphere(lib):
    spec, prev, now = cases.ball()
    none = np.zeros((0, 3), F32)
    tr, ob = track_of(2, 0.125), obj_of(1, 4)
    assert call(lib, spec, tr, ob, prev, none)[:5] == (0, 0, 0, 0, 0)
    assert call(lib, spec, tr, ob, none, none, cap=0)[:5] == (0, 0, 0, 0, 0)
    r = check(lib, spec, tr, ob, none, now)
    assert r["n_objects"] == 1 and r["n_accepted"] == 0 and r["matched"] == 0 and not r["vel"].any()
    r = check(lib, spec, tr, ob, prev, now, keep_now=np.zeros(27, np.uint8))
    assert len(r["cells"]) == 0 and r["occupied"] == 27
    spec, prev, now = cases.equidistant()
    r = check(lib, spec, track_of(1, 0.5), obj_of(1, 1), prev[:1], now)
    assert len(r["cells"]) == 1 and r["n_accepted"] == 1 and r["label"][0] == r["cells"][0]
    assert check(lib, spec, track_of(1, 0.5), obj_of(1, 2), prev[:1], now)["n_objects"] == 0


def test_heavy_component_sums_pass_two_to_the_32(lib):
    spec, prev, now = cases.heavy()
    r = check(lib, spec, track_of(1, 0.1), obj_of(1, 4), prev, now)
    (m, N, Q), = r["tab_now"].values()
    assert (m, N) == (4, 280000) and Q[0] > 2 ** 32 and r["cells"][-1] == 64 * 64 * 48 - 1
    assert r["n_accepted"] == 1 and np.array_equal(r["vel"], np.tile(np.array([0, 0.0625 / 0.1, 0], F32), (4, 1)).astype(F32))


def test_order_of_the_points_changes_nothing(lib):
    spec, prev, now = cases.random_pair(3, (12, 10, 9), 700, 600, fill=0.7)
    tr, ob = track_of(2, 0.1), obj_of(1, 4)
    want = call(lib, spec, tr, ob, prev, now)
    rng = np.random.RandomState(9)
    got = call(lib, spec, tr, ob, prev[rng.permutation(len(prev))], now[rng.permutation(len(now))])
    assert got[:5] == want[:5] and all(np.array_equal(bits(a) if a.dtype == F32 else a, bits(b) if b.dtype == F32 else b) for a, b in zip(got[5:], want[5:]))


def test_errors_write_nothing(lib):
    spec, prev, now = cases.bridge()
    tr, ob = track_of(1, 0.1), obj_of(1, 4)
    assert call(lib, spec, tr, ob, prev, now)[:2] == (0, 9)
    for link in (0, 3, -1):
        assert call(lib, spec, tr, obj_of(link, 4), prev, now)[0] == ERR_INVALID_ARG
    assert b"link" in lib.omds_last_error(None)
    for bad in (track_of(0, 0.1), track_of(5, 0.1), track_of(1, 0.0), track_of(1, np.nan), track_of(1, 0.1, np.inf)):
        assert call(lib, spec, bad, ob, prev, now)[0] == ERR_INVALID_ARG
    assert call(lib, spec_of((0, 0, 0), 0.0, (4, 4, 4)), tr, ob, prev, now)[0] == ERR_INVALID_ARG
    assert call(lib, spec, tr, ob, prev, now, cap=8)[:2] == (ERR_INVALID_ARG, 9)
    assert call(lib, spec_of((0.0, 0.0, 0.0), 0.0625, (12, 6, 4), max_spheres=8), tr, ob, prev, now)[:2] == (ERR_INVALID_ARG, 9)
    assert call(lib, spec, tr, ob, prev, now, cap=9)[:2] == (0, 9)
    n = 16
    out, vel = np.full((n, 4), SENTINEL, F32), np.full((n, 3), SENTINEL, F32)
    label, flag = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    outs = [np.full(1, -1, np.int32) for _ in range(4)]
    args = [C.byref(spec), C.byref(tr), C.byref(ob), prev.ctypes.data, len(prev), None, now.ctypes.data, len(now), None, out.ctypes.data,
            vel.ctypes.data, label.ctypes.data, flag.ctypes.data, n] + [o.ctypes.data for o in outs]

    def untouched():
        return (out == SENTINEL).all() and (vel == SENTINEL).all() and (label == -7).all() and (flag == -7).all() and all(o[0] == -1 for o in outs)

    for i, v in [(i, None) for i in (0, 1, 2, 3, 6, 9, 10, 11, 12, 14, 15)] + [(4, -1), (7, -1), (4, 2 ** 24 + 1), (13, -1)]:
        bad = list(args)
        bad[i] = v
        assert lib.omds_point_cloud_object_flow(*bad) == ERR_INVALID_ARG, (i, v)
        assert untouched(), (i, v)
    skip = list(args)
    skip[16] = skip[17] = None                      # the two object counts may be skipped
    assert lib.omds_point_cloud_object_flow(*skip) == 0 and outs[0][0] == 9 and outs[2][0] == -1


def test_python_wrappers(lib):
    import inspect
    from optimalmodulationds_amd import MPPI, _lib
    from optimalmodulationds_amd.engine import Engine, cloud_object_spec, point_cloud_object_flow
    spec, prev, now = cases.ball()
    spheres, vel, label, flag, matched, n_obj, n_acc = point_cloud_object_flow(prev, now, spec, track_of(2, 0.125), cloud_object_spec())
    assert spheres.shape == (27, 4) and (vel == F32([0.5625, 0, 0])).all() and (flag == 1).all() and (matched, n_obj, n_acc) == (27, 1, 1)
    assert len(set(label)) == 1 and (cloud_object_spec().link, cloud_object_spec().min_cells) == (1, 4)
    keep = np.arange(27) % 2
    assert point_cloud_object_flow(prev, now, spec, track_of(2, 0.125), cloud_object_spec(), keep_now=keep)[0].shape == (13, 4)
    with pytest.raises(_lib.OmdsError) as e:
        point_cloud_object_flow(prev, now, spec, track_of(2, 0.125), cloud_object_spec(), cap=10)
    assert e.value.n_occupied == 27
    ob = cloud_object_spec()
    assert lib.omds_set_obstacles_from_cloud_objects(None, C.byref(spec), C.byref(track_of(2, 0.1)), C.byref(ob), None, 0, 0, None, None, None,
                                                     None, None, None) == ERR_INVALID_ARG
    assert lib.omds_get_cloud_objects(None, None, None, None) == ERR_INVALID_ARG
    assert list(inspect.signature(Engine.set_obstacles_from_cloud_objects).parameters) == ["self", "points", "spec", "track", "obj", "q"]
    assert hasattr(Engine, "cloud_objects")
    p = inspect.signature(MPPI.update_obstacles_from_cloud).parameters
    assert [(k, p[k].default) for k in ("objects", "link", "min_cells")] == [("objects", False), ("link", 1), ("min_cells", 4)]


# ---- the definition under the sanitizers -----------------------------------------------------------------------------------------
def _pack_case(spec, track, obj, prev, now, kp, kn, cap, null_mask):
    prev, now = (np.ascontiguousarray(p, F32).reshape(-1, 3) for p in (prev, now))
    kp, kn = _u8(kp), _u8(kn)
    return (bytes(spec) + bytes(track) + bytes(obj) +
            struct.pack("<qqqqii", prev.shape[0], now.shape[0], -1 if kp is None else kp.size, -1 if kn is None else kn.size, cap, null_mask) +
            prev.tobytes() + now.tobytes() + (b"" if kp is None else kp.tobytes()) + (b"" if kn is None else kn.tobytes()))


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    """tests/cloud_objects_host.cpp, a stand-alone program around the header both the library and its kernels include, built with
    -fsanitize=address,undefined and run on the cases above: a clean exit, and the library's bits."""
    exe = sanitized_host_program("cloud_objects_host", tmp_path)
    none = np.zeros((0, 3), F32)
    todo = []

    def add(spec, track, obj, prev, now, kp=None, kn=None, cap=None, mask=0):
        if cap is None:                                  # exactly the occupied cells: the last row ends all four buffers
            cap = restate_objects(spec, track, obj, prev, now, kp, kn)["occupied"]
        todo.append((spec, track, obj, prev, now, kp, kn, cap, mask))

    s, p, q = cases.ball()
    add(s, track_of(2, 0.125), obj_of(1, 4), p, q)
    add(s, track_of(2, 0.125, still=0.6), obj_of(1, 4), p, q)
    add(s, track_of(2, 0.125), obj_of(1, 4), p, q, kp=np.zeros(27), kn=np.arange(27) % 3)
    add(s, track_of(2, 0.125), obj_of(1, 4), none, q)
    add(s, track_of(2, 0.125), obj_of(1, 4), p, none)
    add(s, track_of(2, 0.125), obj_of(1, 4), p, q, cap=7)                                # too many cells: nothing written
    s, p, q = cases.plate()
    add(s, track_of(1, 0.125), obj_of(1, 4), p, q)
    for gap, link in ((-1, 1), (1, 1), (1, 2), (2, 2)):
        s, p, q = cases.blobs(gap)
        add(s, track_of(1, 0.1), obj_of(link, 1), p, q)
    s, p, q = cases.serpentine()
    add(s, track_of(1, 0.1), obj_of(1, 4), p, q)
    s, p, q = cases.corner_components()
    add(s, track_of(2, 0.25), obj_of(1, 2), p, q)
    add(s, track_of(2, 0.25), obj_of(2, 2), p, q)
    s, p, q = cases.random_pair(5, (37, 29, 1), 400, 400, shift=(1.6, -0.7, 0.0), fill=0.8)
    add(s, track_of(3, 0.1), obj_of(2, 3), p[::-1], q[::-1])
    s, p, q = cases.random_pair(6, (3, 2, 5), 12, 25, shift=(0.0, 0.0, 0.0))
    add(s, track_of(4, 0.1), obj_of(2, 1), p, q)
    for a, b in ((4, 8), (4, 9)):
        s, p, q = cases.line_pair(a, b)
        add(s, track_of(4, 0.1), obj_of(1, 4), p, q)
    for kind in ("below", "at", "above"):
        s, p, q, _ = cases.reach_edge(kind)
        add(s, track_of(2, 0.1), obj_of(1, 1), p, q)
    s, p, q = cases.equidistant()
    add(s, track_of(1, 0.5), obj_of(1, 1), p, q)
    s, p, q = cases.bridge()
    keep = np.ones(9)
    keep[cases.bridge_row(s)] = 0
    add(s, track_of(1, 0.1), obj_of(1, 4), p, q, kp=keep, kn=keep)
    s, p, q = cases.heavy()
    add(s, track_of(1, 0.1), obj_of(1, 4), p, q)
    s, p, q = cases.bridge()
    for bit in range(13):
        add(s, track_of(1, 0.1), obj_of(1, 4), p, q, cap=9, mask=1 << bit)
    add(s, track_of(1, 0.1), obj_of(3, 4), p, q, cap=9)
    add(s, track_of(1, np.nan), obj_of(1, 4), p, q, cap=9)
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(todo)) + b"".join(_pack_case(*c) for c in todo))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cloud_objects_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off = fout.read_bytes(), 0
    for spec, track, obj, prev, now, kp, kn, cap, mask in todo:
        rc, count, matched, n_obj, n_acc, written = struct.unpack_from("<iiiiii", raw, off)
        off += 24
        got = np.frombuffer(raw, F32, written * 4, off).reshape(-1, 4)
        off += written * 16
        got_vel = np.frombuffer(raw, F32, written * 3, off).reshape(-1, 3)
        off += written * 12
        got_label = np.frombuffer(raw, np.int32, written, off)
        off += written * 4
        got_flag = np.frombuffer(raw, np.int32, written, off)
        off += written * 4
        if mask:
            assert (rc == ERR_INVALID_ARG) == (mask < 1 << 11), mask       # the two object counts may be NULL
            continue
        want = call(lib, spec, track, obj, prev, now, kp, kn, cap)
        assert (rc, count, matched, n_obj, n_acc) == want[:5]
        assert np.array_equal(bits(got), bits(want[5])) and np.array_equal(bits(got_vel), bits(want[6]))
        assert np.array_equal(got_label, want[7]) and np.array_equal(got_flag, want[8])
    assert off == len(raw)
