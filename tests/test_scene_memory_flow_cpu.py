"""The definition of memory and velocities in one depth call on the host (include/omds.h: omds_depth_scene_memory_flow; no context, no
GPU) against an independent composition of the three existing host definitions plus step 4 in numpy (tests/scene_memory_flow_cases.py:
compose), every output as bits; the disocclusion artefact it is there to remove, asserted on both definitions; a plate crossing in
front of a wall; the refusals; and the same cases through a stand-alone build of the header under AddressSanitizer + UBSan
(tests/scene_memory_flow_host.cpp), whose output must be the library's."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import scene_memory_cases as sm
import scene_memory_flow_cases as mf
from cloud_cases import F32, cells_of
from cloud_flow_cases import track_of
from depth_cases import FLT, U16
from helpers import sanitized_host_program

ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def define(spec, mem, track, obj, cams, images, prev_images, m_in, **kw):
    from optimalmodulationds_amd.engine import depth_scene_memory_flow
    return depth_scene_memory_flow(images, cams, spec, mem, track, obj, None if prev_images is None else (prev_images, cams), m_in, **kw)


def run_sequence(spec, mem, track, obj, cams, frames, filt=None, keep=None):
    """the definition iterated over ``frames`` ([t][camera]) against the composition; -> the outputs of every frame"""
    m, prev, outs = None, None, []
    for t, images in enumerate(frames):
        keep_now = None
        if keep is not None:
            from optimalmodulationds_amd.engine import depth_scene_memory
            keep_now = keep(np.nonzero(depth_scene_memory(images, cams, spec, mem, m, filter=filt)[0])[0])
        got = define(spec, mem, track, obj, cams, images, prev, m, keep_now=keep_now, filter=filt)
        want = mf.compose(spec, mem, track, obj, cams, images, prev, m, keep_now, filt)
        mf.same(got, want, f"frame {t}")
        outs.append(dict(got, seen=want["seen"], stored=want["stored"]))
        m, prev = got["words"], images
    return outs


# ---- 1. the definition against the composition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("objects", [False, True])
@pytest.mark.parametrize("fmt,size,large", [(U16, (32, 24), False), (FLT, (32, 24), False), (U16, (64, 48), True), (FLT, (64, 48), False)])
def test_definition_is_the_composition_of_the_three(lib, fmt, size, large, objects):
    cam = sm.exact_cam(fmt, *size)
    spec = sm.grid(sm.GRID_LARGE if large else sm.GRID_SMALL, max_spheres=8192)
    mem, track = sm.mem_of(3, 0.0, 1 if large else 0), track_of(2, 0.1)
    outs = run_sequence(spec, mem, track, mf.obj_of() if objects else None, [cam], [[f] for f in sm.sequence(cam)])
    totals = np.sum([o["counts"] for o in outs], 0)
    assert totals[0] > 10 and totals[1] > 5 and totals[2] > 5, totals
    assert outs[0]["n_matched"] == -1 and outs[0]["n_objects_matched"] == -1 and not outs[0]["vel"].any()
    assert outs[1]["n_matched"] > 0, "the wall's visible half finds itself in the previous frame"
    assert any((o["stored"][o["seen"]] >= 2).any() for o in outs), "a seen sphere that was occluded: the override"
    assert (outs[3]["age"] >= 1).all() and not outs[3]["vel"].any() and len(outs[3]["seen"]) == 0, "the blind frame: everything remembered"
    if objects:
        assert max(o["n_objects"] for o in outs) >= 1 and (outs[1]["label"][outs[1]["seen"]] >= 0).all()
        assert all((o["label"][np.setdiff1d(np.arange(len(o["label"])), o["seen"])] == -1).all() for o in outs)


def test_keep_now_and_the_filter_go_through(lib):
    """a stand-in self-filter that drops every third candidate (they leave the words) and the depth filter on both frames"""
    cam = sm.exact_cam(U16, 64, 48)
    spec, mem, track = sm.grid(max_spheres=8192), sm.mem_of(3, 0.0, 0), track_of(2, 0.1)
    outs = run_sequence(spec, mem, track, mf.obj_of(), [cam], [[f] for f in sm.sequence(cam)], filt=dict(radius=1, min_support=4),
                        keep=lambda cand: (np.arange(len(cand)) % 3) != 0)
    assert outs[0]["counts"][4] > 5 and outs[1]["counts"][4] > 0


# ---- 2. the disocclusion --------------------------------------------------------------------------------------------------------------
def test_uncovered_wall_cells_stand_still_where_the_tracked_definition_moves_them(lib):
    from optimalmodulationds_amd.engine import point_cloud_flow
    cam = sm.exact_cam(U16, 32, 24)
    spec, mem, track = sm.grid(max_spheres=8192), sm.mem_of(0), track_of(2, 0.1)
    seq = sm.sequence(cam)
    outs = run_sequence(spec, mem, track, None, [cam], [[f] for f in seq[:3]])
    stored = outs[1]["words"]                                  # after the plate's frame: the wall behind it is remembered
    spheres, vel, _ = point_cloud_flow(mf.points_of([cam], [seq[1]]), mf.points_of([cam], [seq[2]]), spec, track, cap=65536)
    cells = cells_of(spec, spheres)
    uncovered = stored[cells] >= 2
    assert uncovered.sum() > 5, "frame 2 uncovers wall cells that frame 1 had occluded"
    moved = uncovered & (vel != 0).any(1)
    assert moved.any(), "the tracked definition gives an uncovered wall cell a velocity it does not have"
    out = outs[2]
    mine = np.isin(cells_of(spec, out["spheres"]), cells[uncovered])
    assert mine.sum() == uncovered.sum() and not out["vel"][mine].any() and (np.signbit(out["vel"][mine]) == 0).all()
    assert (out["age"][mine] == 0).all(), "they are seen spheres"
    kept = np.isin(cells_of(spec, out["spheres"]), cells[~uncovered])
    assert np.array_equal(out["vel"][kept].view(np.uint32), vel[~uncovered].view(np.uint32)), "every other seen sphere keeps the tracked velocity"


# ---- 3. a crossing plate -----------------------------------------------------------------------------------------------------------------
def test_a_plate_crossing_in_front_of_a_wall(lib):
    cam = sm.exact_cam(U16, 64, 48)
    spec, mem, track = sm.grid(max_spheres=8192), sm.mem_of(0, mf.CROSS_MARGIN, 0), track_of(2, 0.1)
    frames = mf.crossing(cam)
    outs = run_sequence(spec, mem, track, mf.obj_of(1, 4), [cam], [[f] for f in frames])
    dims = np.array(list(spec.dims))
    want_v = F32(F32(-1.0) * F32(spec.voxel)) / F32(0.1)
    for t in range(1, len(frames)):
        out, before = outs[t], outs[t - 1]
        cells = cells_of(spec, out["spheres"])
        ix = cells % dims[0]
        plate = ix == 1                                         # the plate's layer: x = 0.25 + 1 m
        assert plate.sum() >= 8 and (out["age"][plate] == 0).all(), t
        assert (out["object"][plate] == 1).all() and (out["vel"][plate] == np.array([0, want_v, 0], F32)).all(), (t, out["vel"][plate][:3])
        remembered = out["age"] >= 1
        assert remembered.sum() > 5 and (ix[remembered] == 9).all() and not out["vel"][remembered].any(), "the wall behind the plate"
        assert (out["label"][remembered] == -1).all() and (out["object"][remembered] == 0).all()
        was = cells_of(spec, before["spheres"])
        left = np.setdiff1d(was[was % dims[0] == 1], cells[plate])
        assert len(left) >= 4 and out["counts"][2] >= len(left), "the cells the plate left are cleared"
        assert not out["words"][left].any() and not np.isin(left, cells).any(), "and no sphere remains in them"


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def raw_call(lib, case):
    """(rc, every output array) of the raw entry point on a packed-style case; outputs are filled with sentinels first"""
    from optimalmodulationds_amd import _lib as L
    spec, cams, images = case["spec"], case["cams"], case["images"]
    null = case.get("null", 0)
    keepalive = []

    def frame(cs, ims):
        table = (L.OmdsDepthCamera * max(len(cs), 1))(*cs)
        arrs = [np.ascontiguousarray(im) for im in ims]
        keepalive.extend(arrs)
        return table, (C.c_void_p * max(len(cs), 1))(*[a.ctypes.data for a in arrs])
    table, addrs = frame(cams, images)
    prev = case.get("prev")
    ptable, paddrs = frame(cams, prev) if prev is not None else (None, None)
    cells, cap = sm.n_cells_of(spec), case.get("cap", 4096)
    room = max(cap, 1)
    words, counts = np.full(cells, 0xA5A5A5A5, np.uint32), np.full(5, -7, np.int32)
    xyzr, vel = np.full((room, 4), np.nan, F32), np.full((room, 3), np.nan, F32)
    age, label, flag = (np.full(room, -7, np.int32) for _ in range(3))
    cnt, nm, no, na = (np.full(1, -7, np.int32) for _ in range(4))
    m = case.get("mem_in")
    src = None if m is None else np.ascontiguousarray(m, np.uint32)
    obj, filt = case.get("obj"), case.get("filt")
    rc = lib.omds_depth_scene_memory_flow(
        C.byref(spec), None if null & 1 else C.byref(case["mem"]), None if null & 4 else C.byref(case["track"]), None if obj is None else C.byref(obj),
        None if filt is None else C.byref(filt), ptable, paddrs, 0 if prev is None else len(cams), None, table, addrs,
        len(cams) if case.get("n_cams") is None else case["n_cams"], None, None if src is None else src.ctypes.data,
        None if null & 2 else words.ctypes.data, L.iptr(counts), L.fptr(xyzr), None if null & 16 else L.fptr(vel), L.iptr(age), L.iptr(label),
        L.iptr(flag), cap, None if null & 8 else L.iptr(cnt), L.iptr(nm), L.iptr(no), L.iptr(na))
    return rc, dict(words=words, counts=counts, xyzr=xyzr, vel=vel, age=age, label=label, flag=flag, count=cnt, n=(nm, no, na))


def untouched(out, but_counts=False):
    ok = (out["words"] == 0xA5A5A5A5).all() and np.isnan(out["xyzr"]).all() and np.isnan(out["vel"]).all()
    ok &= all((out[k] == -7).all() for k in ("age", "label", "flag")) and all((v == -7).all() for v in out["n"])
    return ok and (but_counts or ((out["counts"] == -7).all() and (out["count"] == -7).all()))


def _refusals():
    from optimalmodulationds_amd.engine import depth_filter_spec
    cam = sm.exact_cam()
    seq = sm.sequence(cam)
    ok = dict(spec=sm.grid(), mem=sm.mem_of(), track=track_of(2, 0.1), obj=mf.obj_of(), cams=[cam], images=[seq[1]], prev=[seq[0]])
    bad_cam = sm.exact_cam()
    bad_cam.fx = 0.0
    bad = [dict(ok, mem=sm.mem_of(footprint=4)), dict(ok, null=1), dict(ok, null=2), dict(ok, null=4), dict(ok, null=8), dict(ok, null=16),
           dict(ok, track=track_of(5, 0.1)), dict(ok, track=track_of(2, 0.0)), dict(ok, obj=mf.obj_of(3, 4)), dict(ok, filt=depth_filter_spec(radius=4)),
           dict(ok, n_cams=0), dict(ok, n_cams=9), dict(ok, cams=[bad_cam]), dict(ok, cap=-1), dict(ok, spec=sm.grid(dict(sm.GRID_SMALL, voxel=0.0)))]
    return ok, bad


def test_refusals_write_nothing(lib):
    ok, bad = _refusals()
    rc, out = raw_call(lib, ok)
    assert rc == 0 and out["count"][0] > 20 and not untouched(out)
    for case in bad:
        rc, out = raw_call(lib, case)
        assert rc == ERR_INVALID_ARG and untouched(out), {k: v for k, v in case.items() if k in ("null", "n_cams", "cap")}
    want = define(ok["spec"], ok["mem"], ok["track"], ok["obj"], ok["cams"], ok["images"], ok["prev"], None)
    n = len(want["spheres"])
    rc, out = raw_call(lib, dict(ok, spec=sm.grid(max_spheres=n - 1)))
    assert rc == ERR_INVALID_ARG and untouched(out, but_counts=True) and out["count"][0] == n and tuple(out["counts"]) == want["counts"]
    rc, out = raw_call(lib, dict(ok, cap=n - 1))
    assert rc == ERR_INVALID_ARG and untouched(out, but_counts=True) and out["count"][0] == n
    rc, out = raw_call(lib, dict(ok, cap=n))
    assert rc == 0 and out["count"][0] == n, "exactly as many as there are: taken"
    from optimalmodulationds_amd import _lib
    with pytest.raises(_lib.OmdsError) as err:
        define(sm.grid(max_spheres=n - 1), ok["mem"], ok["track"], ok["obj"], ok["cams"], ok["images"], ok["prev"], None)
    assert err.value.n_occupied == n and err.value.counts == want["counts"]


# ---- 5. the sanitizer leg ------------------------------------------------------------------------------------------------------------------
def _pack_frame(cams, images, n_cams, keep):
    raw = struct.pack("<ii", n_cams, len(images))
    for cam, img in zip(cams, images):
        flat = np.ascontiguousarray(img).reshape(-1)
        raw += bytes(cam) + struct.pack("<iq", flat.itemsize, flat.size) + flat.tobytes()
    if keep is None:
        return raw + struct.pack("<i", -1)
    k = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
    return raw + struct.pack("<i", k.size) + k.tobytes()


def _pack(case):
    from optimalmodulationds_amd import _lib as L
    spec, cams = case["spec"], case["cams"]
    obj, filt, m, prev = case.get("obj"), case.get("filt"), case.get("mem_in"), case.get("prev")
    raw = bytes(spec) + bytes(case["mem"]) + bytes(case["track"])
    raw += struct.pack("<i", obj is not None) + bytes(obj if obj is not None else L.OmdsCloudObjectSpec())
    raw += struct.pack("<i", filt is not None) + bytes(filt if filt is not None else L.OmdsDepthFilterSpec())
    raw += struct.pack("<iiqi", case.get("null", 0), case.get("cap", 4096), sm.n_cells_of(spec), 0 if m is None else 1)
    if m is not None:
        raw += np.ascontiguousarray(m, np.uint32).tobytes()
    raw += _pack_frame(cams, prev or [], 0 if prev is None else len(cams), None)
    raw += _pack_frame(cams, case["images"], len(cams) if case.get("n_cams") is None else case["n_cams"], case.get("keep_now"))
    return raw


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    from optimalmodulationds_amd.engine import depth_filter_spec
    exe = sanitized_host_program("scene_memory_flow_host", tmp_path)
    cases = []
    for fmt, obj, filt in ((U16, None, None), (FLT, mf.obj_of(), None), (U16, mf.obj_of(2, 2), depth_filter_spec(1, 4))):
        cam = sm.exact_cam(fmt)
        spec, mem, track = sm.grid(), sm.mem_of(2, 0.3, 1), track_of(2, 0.1)
        m, prev = None, None
        for img in sm.sequence(cam) + [sm.frame(cam, 2.0, 2)]:
            case = dict(spec=spec, mem=mem, track=track, obj=obj, filt=filt, cams=[cam], images=[img], prev=prev, mem_in=m)
            n_cand = len(define(spec, mem, track, obj, [cam], [img], prev, m, filter=filt)["spheres"])
            cases.append(case)
            cases.append(dict(case, keep_now=(np.arange(n_cand) % 4) != 1, cap=n_cand))      # the output arrays at exactly the candidates
            m, prev = define(spec, mem, track, obj, [cam], [img], prev, m, filter=filt)["words"], [img]
    wide = sm.exact_cam(U16, 64, 48)
    m, prev = None, None
    for img in mf.crossing(wide):
        cases.append(dict(spec=sm.grid(), mem=sm.mem_of(0, mf.CROSS_MARGIN, 0), track=track_of(2, 0.1), obj=mf.obj_of(), cams=[wide, wide],
                          images=[img, img], prev=prev, mem_in=m))
        m, prev = define(sm.grid(), sm.mem_of(0, mf.CROSS_MARGIN, 0), track_of(2, 0.1), mf.obj_of(), [wide, wide], [img, img], prev, m)["words"], [img, img]
    ok, bad = _refusals()
    n = len(define(ok["spec"], ok["mem"], ok["track"], ok["obj"], ok["cams"], ok["images"], ok["prev"], None)["spheres"])
    bad = bad + [dict(ok, spec=sm.grid(max_spheres=n - 1)), dict(ok, cap=n - 1)]
    cases += bad
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(cases)) + b"".join(_pack(c) for c in cases))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scene_memory_flow_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off, n_ok = fout.read_bytes(), 0, 0
    for i, case in enumerate(cases):
        head = struct.unpack_from("<10iq", raw, off)
        off += 48
        rc, counts, count, rest, cells = head[0], head[1:6], head[6], head[7:10], head[10]
        words = np.frombuffer(raw, np.uint32, cells, off)
        off += cells * 4
        (k,) = struct.unpack_from("<q", raw, off)
        off += 8
        got = {}
        for key, dtype, width in (("spheres", F32, 4), ("vel", F32, 3), ("age", np.int32, 1), ("label", np.int32, 1), ("object", np.int32, 1)):
            got[key] = np.frombuffer(raw, dtype, k * width, off).reshape((k, width) if width > 1 else (k,))
            off += k * width * 4
        if i >= len(cases) - len(bad):
            assert rc == ERR_INVALID_ARG and cells == 0 and k == 0, i
            continue
        want = define(case["spec"], case["mem"], case["track"], case.get("obj"), case["cams"], case["images"], case.get("prev"), case.get("mem_in"),
                      keep_now=case.get("keep_now"), filter=case.get("filt"), cap=case.get("cap"))
        got.update(words=words, counts=tuple(counts), n_matched=rest[0], n_objects=rest[1], n_objects_matched=rest[2])
        assert rc == 0 and count == k
        mf.same(got, want, f"case {i}")
        n_ok += 1
    assert off == len(raw) and n_ok == len(cases) - len(bad) == 40
