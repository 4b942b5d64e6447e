"""The definition of the velocity filter on the host (include/omds.h: omds_velocity_filter_step; no context, no GPU) against the numpy
restatement of the header's text in tests/velocity_filter_cases.py: velocities and state records bit for bit, the counts exactly.

The same cases also go through a stand-alone build of the definition under AddressSanitizer + UBSan (tests/velocity_filter_host.cpp,
its buffers allocated at exactly the sizes passed), whose output must be the library's bit for bit."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import velocity_filter_cases as cases
from cloud_cases import F32
from cloud_flow_cases import fmaf, track_of
from helpers import sanitized_host_program
from velocity_filter_cases import GRIDS, cell_of, filt_of, restate_step

ERR_INVALID_ARG = 1
VEL_MARK, MARK = F32(-7), -77


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def n_cells(spec):
    return int(spec.dims[0]) * int(spec.dims[1]) * int(spec.dims[2])


def call(lib, c, null=()):
    """(rc, vel, state_out, stats) of the raw entry point on the case ``c``; a refused call must have written nothing.  ``null``: the
    names of the arguments passed as NULL"""
    n, cells = len(c["cell"]), n_cells(c["spec"])
    vel, out, stats = np.full((max(n, 1), 3), VEL_MARK, F32), np.full((max(cells, 1), 4), MARK, np.int32), np.full(3, MARK, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data
    args = dict(spec=C.byref(c["spec"]), track=C.byref(c["track"]), filt=C.byref(c["filt"]), state_in=ptr(c["state_in"]), cell=ptr(c["cell"]),
                raw=ptr(c["raw"]), live=ptr(c["live"]), group=ptr(c["group"]), n=n, vel_out=vel.ctypes.data, state_out=out.ctypes.data,
                stats_out=stats.ctypes.data)
    for name in null:
        args[name] = None
    rc = lib.omds_velocity_filter_step(*args.values())
    if rc != 0:
        assert (vel == VEL_MARK).all() and (out == MARK).all() and (stats == MARK).all(), "a refused call must write nothing"
        return rc, None, None, None
    return rc, vel[:n].copy(), out[:cells].copy(), tuple(int(v) for v in stats)


def check(lib, c):
    """the definition equals the restatement -> (vel, state_out, stats)"""
    rc, vel, out, stats = call(lib, c)
    want_vel, want_out, want_stats = restate_step(c["spec"], c["track"], c["filt"], c["state_in"], c["cell"], c["raw"], c["live"], c["group"])
    assert rc == 0 and stats == want_stats, (rc, stats, want_stats)
    assert np.array_equal(out, want_out), "the state records are not the restatement's"
    assert np.array_equal(bits(vel), bits(want_vel)), "velocities are not the restatement's bits"
    return vel, out, stats


# ---- 1. random states, windows clipped at every face ------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", GRIDS)
@pytest.mark.parametrize("reach", [1, 2, 4])
def test_random_states_match_the_restatement(lib, dims, reach):
    c = cases.random_case(10 + reach, dims, reach, fill=0.12 if reach < 4 else 0.03, max_jump=3.0, still=1.2, groups=3)
    vel, out, stats = check(lib, c)
    assert stats[0] > 10 and stats[1] > 0 and stats[2] > 0 and (out[:, 3] > 0).sum() == int(c["live"].sum())
    assert set(cases.face_cells(dims)) <= set(c["cell"].tolist())
    assert (vel[c["live"] == 0] == 0).all() and (vel == 0).all(1).sum() > int((c["live"] == 0).sum()), "some live sphere is under the still bar"


def test_empty_state_and_empty_list(lib):
    c = cases.random_case(3, GRIDS[1], 2)
    c["state_in"] = None
    vel, out, stats = check(lib, c)
    assert stats == (0, 0, 0) and np.array_equal(bits(vel), bits(c["raw"])) and set(out[out[:, 3] > 0, 3]) == {1}
    c = cases.case(GRIDS[1], track_of(2, 0.1), filt_of(), cases.random_state(np.random.RandomState(1), GRIDS[1], 0.5), [], np.zeros((0, 3)))
    _, out, stats = check(lib, c)
    assert stats == (0, 0, 0) and not out.any(), "every cell not written is empty in state_out"


def test_state_in_may_be_state_out(lib):
    c = cases.random_case(5, GRIDS[0], 2, groups=2)
    _, want, _ = check(lib, c)
    state = c["state_in"].copy()
    vel, stats = np.zeros((len(c["cell"]), 3), F32), np.zeros(3, np.int32)
    rc = lib.omds_velocity_filter_step(C.byref(c["spec"]), C.byref(c["track"]), C.byref(c["filt"]), state.ctypes.data, c["cell"].ctypes.data,
                                       c["raw"].ctypes.data, c["live"].ctypes.data, c["group"].ctypes.data, len(c["cell"]), vel.ctypes.data,
                                       state.ctypes.data, stats.ctypes.data)
    assert rc == 0 and np.array_equal(state, want)


# ---- 2. the predecessor -----------------------------------------------------------------------------------------------------------
def test_a_tie_is_averaged(lib):
    c = cases.tie()
    vel, out, stats = check(lib, c)
    p = (np.array([2 * 65536, 0, 80001], np.int64).astype(F32) / F32(2)) * cases.SCALE      # the two cells at d2 = 1; the one at d2 = 4 stays out
    a = max(F32(0.3), F32(1.0) / F32(4))                                                    # h = min(3, 7): alpha has passed the running mean
    want = np.array([fmaf(a, c["raw"][0, k] - p[k], p[k]) for k in range(3)], F32)
    assert np.array_equal(bits(vel[0]), bits(want)) and out[c["cell"][0], 3] == 4 and stats == (1, 0, 0)


def test_the_own_cell_is_the_predecessor(lib):
    c = cases.own_cell()
    vel, out, _ = check(lib, c)
    p = np.array([65536, 0, -32768], np.int64).astype(F32) * cases.SCALE
    want = np.array([fmaf(F32(0.3), c["raw"][0, k] - p[k], p[k]) for k in range(3)], F32)
    assert np.array_equal(bits(vel[0]), bits(want)) and out[c["cell"][0], 3] == 5


# ---- 3. hits: the running mean and the saturation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("h, hits, a", [(0, 1, None), (1, 2, 0.5), (2, 3, 1.0 / 3.0), (254, 255, 0.25), (255, 255, 0.25)])
def test_hits_lead_from_a_running_mean_to_alpha(lib, h, hits, a):
    c = cases.hits_case(h, alpha=0.25)
    vel, out, stats = check(lib, c)
    assert out[c["cell"][0], 3] == hits and stats == (int(h > 0), 0, 0)
    if h == 0:
        assert np.array_equal(bits(vel[0]), bits(c["raw"][0]))
        return
    a = F32(1.0) / F32(h + 1) if h < 3 else F32(a)
    p = np.array([65536 + 7, -3 * 65536 + 1, 11], np.int64).astype(F32) * cases.SCALE
    want = np.array([fmaf(a, c["raw"][0, k] - p[k], p[k]) for k in range(3)], F32)
    assert np.array_equal(bits(vel[0]), bits(want))


@pytest.mark.parametrize("h", [1, 2, 254, 255])
def test_alpha_one_is_the_raw_velocity(lib, h):
    c = cases.hits_case(h, alpha=1.0)
    vel, out, _ = check(lib, c)
    assert np.array_equal(bits(vel[0]), bits(c["raw"][0])) and out[c["cell"][0], 3] == min(h + 1, 255)
    c = cases.random_case(8, GRIDS[0], 2, alpha=1.0, alpha_object=1.0, groups=2)
    vel, _, stats = check(lib, c)
    assert stats[0] > 10 and np.array_equal(bits(vel), bits(c["raw"]))


# ---- 4. the jump test -------------------------------------------------------------------------------------------------------------
def test_jump_exactly_at_the_bar_and_one_ulp_above(lib):
    at, above = cases.jump_case(False), cases.jump_case(True)
    bar = F32(0.75) * F32(0.75)
    j2 = lambda c: fmaf(c["raw"][0, 2], c["raw"][0, 2], fmaf(c["raw"][0, 1], c["raw"][0, 1], c["raw"][0, 0] * c["raw"][0, 0]))
    assert j2(at) == bar and j2(above) == np.nextafter(bar, F32(np.inf))
    vel, out, stats = check(lib, at)
    assert stats == (1, 0, 0) and out[at["cell"][0], 3] == 6 and vel[0, 0] == fmaf(F32(0.3), F32(0.75), F32(0)), "at the bar: no restart"
    vel, out, stats = check(lib, above)
    assert stats == (1, 1, 0) and out[above["cell"][0], 3] == 1 and np.array_equal(bits(vel[0]), bits(above["raw"][0])), "one ulp above: a restart"
    above["filt"] = filt_of(max_jump=0.0)
    assert check(lib, above)[2] == (1, 0, 0), "max_jump <= 0 switches the test off"
    above["filt"] = filt_of(max_jump=-1.0)
    assert check(lib, above)[2] == (1, 0, 0)


# ---- 5. the record ----------------------------------------------------------------------------------------------------------------
def test_clamp_and_ties_to_even(lib):
    c = cases.clamp_and_ties()
    vel, out, _ = check(lib, c)
    q = out[c["cell"], :3]
    top = 1024 * 65536
    assert q[0].tolist() == [top, -top, top] and q[3].tolist() == [top, -top, -top]
    assert q[1].tolist() == [0, 2, 2] and q[2].tolist() == [0, -2, -2] and q[4, 2] == 4
    assert np.array_equal(bits(vel), bits(c["raw"])), "the clamp is the record's: the output is not clamped"


def test_a_dead_sphere_outputs_zero_and_stores_nothing(lib):
    c = cases.own_cell()
    c["live"] = np.zeros(1, np.int32)
    vel, out, stats = check(lib, c)
    assert stats == (0, 0, 0) and np.array_equal(bits(vel), np.zeros((1, 3), np.uint32)) and not out.any()


def test_still_zeroes_the_output_and_not_the_record(lib):
    c = cases.still_case()
    vel, out, _ = check(lib, c)
    assert np.array_equal(bits(vel[0]), np.zeros(3, np.uint32)) and out[c["cell"][0]].tolist()[0] > 0 and out[c["cell"][0], 3] == 201
    c["track"] = track_of(2, 0.1, 0.0)
    assert check(lib, c)[0][0, 0] > 0.1


# ---- 6. groups --------------------------------------------------------------------------------------------------------------------
def test_a_group_blends_against_one_predecessor(lib):
    c = cases.group_case()
    vel, out, stats = check(lib, c)
    assert stats == (6, 0, 1), "the member with an empty window has the group's history"
    m = c["group"] >= 0
    assert m.sum() == 5 and (bits(vel[m]) == bits(vel[0])).all(), "every member receives one velocity"
    assert (out[c["cell"][m]] == out[c["cell"][0]]).all() and out[c["cell"][0], 3] == 3, "Gh = min(3, 9, min(9, 2), 3) = 2"
    # the predecessors: (2,2,2) and (3,2,2) their own cells, (4,2,2) the tie of (3,2,2) and (5,2,2), (2,3,2) the cell (2,2,2), (9,8,7) none
    G = np.array([65536 + 2 * 65536 + (2 * 65536 - 65536) + 65536, 100 - 100 + (-100 + 65536 // 3) + 100, -7 + 9 + (9 + 1) - 7], np.int64)
    p = (G.astype(F32) / F32(5)) * cases.SCALE
    want = np.array([fmaf(F32(0.6), c["raw"][0, k] - p[k], p[k]) for k in range(3)], F32)
    assert np.array_equal(bits(vel[0]), bits(want)), "alpha_object, against the sums over all members' predecessors"
    alone = dict(c, group=None)
    assert not (bits(check(lib, alone)[0][m]) == bits(vel[0])).all(1).any(), "ungrouped, each member blends against its own"


def test_a_group_without_history_starts_from_raw(lib):
    c = cases.group_case(history=False)
    vel, out, stats = check(lib, c)
    assert stats == (0, 0, 0) and np.array_equal(bits(vel), bits(c["raw"])) and (out[c["cell"], 3] == 1).all()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_writes_nothing(lib):
    good = cases.group_case()
    assert call(lib, good)[0] == 0
    for alpha in (0.0, -0.1, 1.0001, np.nan, np.inf):
        assert call(lib, dict(good, filt=filt_of(alpha=alpha)))[0] == ERR_INVALID_ARG, alpha
    assert b"alpha" in lib.omds_last_error(None)
    for ao in (1.5, np.nan, np.inf):
        assert call(lib, dict(good, filt=filt_of(alpha_object=ao)))[0] == ERR_INVALID_ARG, ao
    for ao in (0.0, -3.0, -np.inf, 1.0):
        assert call(lib, dict(good, filt=filt_of(alpha_object=ao)))[0] == 0, ao
    assert call(lib, dict(good, filt=filt_of(max_jump=np.nan)))[0] == ERR_INVALID_ARG
    for mj in (np.inf, -np.inf, -1.0):
        assert call(lib, dict(good, filt=filt_of(max_jump=mj)))[0] == 0, mj
    for reach in (0, 5):
        assert call(lib, dict(good, track=track_of(reach, 0.1)))[0] == ERR_INVALID_ARG
    assert call(lib, dict(good, spec=cases.grid_spec(GRIDS[0], voxel=0.0)))[0] == ERR_INVALID_ARG
    cells = n_cells(good["spec"])
    for bad in ([5, 5], [7, 5], [-1, 3], [3, cells]):
        c = dict(good, cell=np.array(bad, np.int32), raw=good["raw"][:2], live=None, group=None)
        assert call(lib, c)[0] == ERR_INVALID_ARG, bad
    assert b"ascending" in lib.omds_last_error(None)
    for bad in (-2, cells):
        g = good["group"].copy()
        g[1] = bad
        assert call(lib, dict(good, group=g))[0] == ERR_INVALID_ARG, bad
    for name in ("spec", "track", "filt", "cell", "raw", "vel_out", "state_out"):
        assert call(lib, good, null=(name,))[0] == ERR_INVALID_ARG, name
    for name in ("state_in", "live", "group", "stats_out"):      # the optional ones
        assert call(lib, good, null=(name,))[0] == 0, name
    out = np.full((cells, 4), MARK, np.int32)
    rc = lib.omds_velocity_filter_step(C.byref(good["spec"]), C.byref(good["track"]), C.byref(good["filt"]), None, None, None, None, None, -1, None,
                                       out.ctypes.data, None)
    assert rc == ERR_INVALID_ARG and (out == MARK).all(), "n < 0"


def test_python_wrappers(lib):
    import inspect
    from optimalmodulationds_amd import MPPI, _lib
    from optimalmodulationds_amd.engine import Engine, velocity_filter_spec, velocity_filter_step
    c = cases.group_case()
    vel, out, stats = velocity_filter_step(c["spec"], c["track"], dict(alpha=0.3, alpha_object=0.6), c["state_in"], c["cell"], c["raw"], c["live"],
                                           c["group"])
    want = call(lib, c)
    assert np.array_equal(bits(vel), bits(want[1])) and np.array_equal(out, want[2]) and stats == want[3]
    with pytest.raises(_lib.OmdsError):
        velocity_filter_step(c["spec"], c["track"], velocity_filter_spec(alpha=2.0), None, c["cell"], c["raw"])
    d = velocity_filter_spec()
    assert (d.alpha, d.alpha_object, d.max_jump) == (F32(0.3), 0.0, 0.0)
    for name in ("set_velocity_filter", "velocity_filter_frame", "velocity_filter_state"):
        assert hasattr(Engine, name)
    assert lib.omds_set_velocity_filter(None, None) == ERR_INVALID_ARG and lib.omds_get_velocity_filter(None, None, None) == ERR_INVALID_ARG
    assert lib.omds_get_velocity_filter_frame(None, None, None, None) == ERR_INVALID_ARG
    assert lib.omds_get_velocity_filter_state(None, None, None) == ERR_INVALID_ARG
    for f in (MPPI.update_obstacles_from_cloud, MPPI.update_obstacles_from_depth):      # smooth= goes through **route on both: the named keywords stay
        assert "route" in inspect.signature(f).parameters and "smooth" not in inspect.signature(f).parameters and "smooth" in f.__doc__


# ---- 8. the definition under the sanitizers ---------------------------------------------------------------------------------------
def _pack_case(c, null_mask=0):
    n, cells = len(c["cell"]), n_cells(c["spec"])
    have = (1 if c["state_in"] is not None else 0) | (2 if c["live"] is not None else 0) | (4 if c["group"] is not None else 0)
    parts = [bytes(c["spec"]), bytes(c["track"]), bytes(c["filt"]), struct.pack("<iiii", n, cells, have, null_mask)]
    parts += [a.tobytes() for a in (c["state_in"], c["cell"], c["raw"], c["live"], c["group"]) if a is not None]
    return b"".join(parts)


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    """tests/velocity_filter_host.cpp, a stand-alone program around the header both the library and its kernels include, built with
    -fsanitize=address,undefined and run on the cases above: a clean exit, and the library's bits."""
    exe = sanitized_host_program("velocity_filter_host", tmp_path)
    todo = []
    for dims in GRIDS:
        for reach in (1, 2, 4):
            todo.append((cases.random_case(10 + reach, dims, reach, fill=0.12 if reach < 4 else 0.03, max_jump=3.0, still=1.2, groups=3), 0))
    todo += [(c, 0) for c in (cases.tie(), cases.own_cell(), cases.jump_case(False), cases.jump_case(True), cases.clamp_and_ties(),
                              cases.group_case(), cases.group_case(history=False), cases.still_case())]
    todo += [(cases.hits_case(h, alpha), 0) for h in (0, 1, 2, 254, 255) for alpha in (0.25, 1.0)]
    empty = cases.random_case(3, GRIDS[1], 2)
    empty["state_in"] = None
    todo.append((empty, 0))
    todo.append((cases.case(GRIDS[1], track_of(2, 0.1), filt_of(), None, [], np.zeros((0, 3))), 0))
    good = cases.group_case()
    todo += [(good, mask) for mask in (1, 2, 4, 8, 16, 32, 64)]
    todo += [(dict(good, filt=filt_of(alpha=np.nan)), 0), (dict(good, track=track_of(5, 0.1)), 0),
             (dict(good, cell=good["cell"][::-1].copy()), 0)]
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(todo)) + b"".join(_pack_case(c, m) for c, m in todo))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "velocity_filter_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off = fout.read_bytes(), 0
    for c, mask in todo:
        rc, s0, s1, s2, written = struct.unpack_from("<iiiii", raw, off)
        off += 20
        if mask:
            assert rc == ERR_INVALID_ARG and written == 0
            continue
        want_rc, want_vel, want_out, want_stats = call(lib, c)
        assert rc == want_rc
        if rc != 0:
            continue
        cells = n_cells(c["spec"])
        got_vel = np.frombuffer(raw, F32, written * 3, off).reshape(-1, 3)
        off += written * 12
        got_out = np.frombuffer(raw, np.int32, cells * 4, off).reshape(-1, 4)
        off += cells * 16
        assert (s0, s1, s2) == want_stats and np.array_equal(bits(got_vel), bits(want_vel)) and np.array_equal(got_out, want_out)
    assert off == len(raw)
