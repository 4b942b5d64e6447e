"""The definition of the obstacle focus along a path on the host (include/omds.h: omds_obstacle_focus_select_path; no context, no GPU)
against a numpy restatement in the header's operation order (tests/obstacle_focus_path_cases.py): the kept indices and both counts must
match exactly.  Its properties: one state is omds_obstacle_focus_select, and neither the order of the states nor a state given twice
changes anything.  The same cases also go through a stand-alone build of the definition under AddressSanitizer + UBSan
(tests/obstacle_focus_path_host.cpp, its buffers allocated at exactly the sizes passed), whose output must be the library's."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from helpers import ROOT, sanitized_host_program
from obstacle_focus_cases import F32, INF, cases, restate
from obstacle_focus_path_cases import path_cases, restate_path

ERR_INVALID_ARG = 1
NAMES = ["omds_obstacle_focus_select_path", "omds_focus_obstacles_path"]
CASES = path_cases()
SINGLE = cases()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def spec_of(margin, max_keep=0, lookahead=0.0):
    from optimalmodulationds_amd.engine import obstacle_focus_spec
    return obstacle_focus_spec(margin, max_keep, lookahead)


def call(lib, d, ahead, vel, k, margin, max_keep, lookahead, cap=None, n_states=None):
    """(rc, kept, passed, idx [kept if rc == 0 else 0]) of the raw entry point; a refused call must leave idx_out alone"""
    d = np.ascontiguousarray(d, F32)
    B, O = d.shape
    a = None if ahead is None else np.ascontiguousarray(ahead, F32).reshape(-1)
    v = None if vel is None else np.ascontiguousarray(vel, F32).reshape(-1, 3)
    cap = O if cap is None else cap
    idx, kept, passed = np.full(max(cap, 1), -7, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    spec = spec_of(margin, max_keep, lookahead)
    rc = lib.omds_obstacle_focus_select_path(C.byref(spec), d.ctypes.data, None if a is None else a.ctypes.data, None if v is None else v.ctypes.data,
                                             B if n_states is None else n_states, O, k, idx.ctypes.data, cap, kept.ctypes.data, passed.ctypes.data)
    if rc != 0:
        assert (idx == -7).all(), "a refused call must write no index"
    return rc, int(kept[0]), int(passed[0]), idx[:int(kept[0])].copy() if rc == 0 else idx[:0]


def test_symbols_declared_exported_and_bound(lib):
    from optimalmodulationds_amd import _lib
    header = open(os.path.join(ROOT, "include", "omds.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"OMDS_API\s+int\s+" + name + r"\s*\(", header), f"{name} is not declared in omds.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert C.sizeof(_lib.OmdsObstacleFocusSpec) == 12
    assert lib.omds_version() == _lib.ABI_VERSION == 512


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_definition_matches_the_restatement(lib, case):
    name, d, ahead, vel, k, margin, max_keep, lookahead = case
    rc, kept, passed, idx = call(lib, d, ahead, vel, k, margin, max_keep, lookahead)
    want, want_passed = restate_path(d, k, margin, max_keep, lookahead, ahead, vel)
    assert rc == 0 and passed == want_passed and kept == len(want), (rc, kept, passed, len(want), want_passed)
    assert np.array_equal(idx, want)
    assert k <= kept <= passed <= d.shape[1] and (max_keep < 1 or kept <= max_keep)
    assert (np.diff(idx) > 0).all()


def test_cases_cover_what_they_name():
    by = {c[0]: c for c in CASES}

    def got(name, **over):
        _, d, ahead, vel, k, margin, max_keep, lookahead = by[name]
        a = dict(d=d, k=k, margin=margin, max_keep=max_keep, lookahead=lookahead, ahead=ahead, vel=vel)
        a.update(over)
        return restate_path(**a)

    d = by["passes_at_one_state"][1]
    assert 30 in got("passes_at_one_state")[0]
    for b in range(4):
        assert (30 in restate(d[b], 10, 0.0)[0]) == (b == 2)
    # row 0 passes all 40 at margin 0.5, row 1 its 10 nearest only, and those are the LAST ten indices; at 1e-4 row 0 passes few
    assert got("thresholds_far_apart")[1] == 40 and restate(by["thresholds_far_apart"][1][1], 10, 0.5)[1] == 10
    assert 10 < got("thresholds_far_apart_small_margin")[1] < 40
    g = {n: got(n)[1] for n in by if n.startswith("margin_")}
    assert g["margin_zero"] == g["margin_below_gap"] == 20 and g["margin_gap"] == g["margin_above_gap"] == 21 and g["margin_inf"] == 41
    d = by["ties_keep15"][1]
    idx, passed = got("ties_keep15")
    m = d.min(0)
    assert passed == 24 and len(idx) == 15 and 0 < (m[idx] == F32(0.5)).sum() < (m == F32(0.5)).sum() == 12
    assert len({int(np.argmin(d[:, o])) for o in np.flatnonzero(m == F32(0.5))}) == 3, "the tie group is reached in different rows"
    assert got("cap_with_inf_margin")[1] == 44 and len(got("cap_with_inf_margin")[0]) == 20
    assert 41 in got("nan_in_one_row")[0] and 41 in got("nan_in_one_row_cap")[0] and len(got("nan_in_one_row_cap")[0]) == 10
    assert 41 not in restate_path(np.delete(by["nan_in_one_row"][1], 3, 0), 10, 0.0)[0]
    assert got("threshold_is_inf")[1] == 50 and len(got("threshold_is_inf_cap")[0]) == 30
    assert list(got("zeros_cut")[0]) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 17]           # -0.5 first, then the zeros by index
    assert 12 in got("late_ahead_pulls_in")[0] and 12 not in got("ahead_too_short")[0] and 12 in got("ahead_and_lookahead")[0]
    assert 12 not in got("ahead_without_velocities")[0]
    assert {14, 15} <= set(got("velocity_not_finite")[0]) and {14, 15} <= set(got("velocity_not_finite_no_time")[0])


@pytest.mark.parametrize("case", SINGLE, ids=[c[0] for c in SINGLE])
def test_one_state_is_the_single_state_definition(lib, case):
    from optimalmodulationds_amd.engine import obstacle_focus_select
    name, d, vel, k, margin, max_keep, lookahead = case
    want, want_passed = obstacle_focus_select(d, k, margin, max_keep, lookahead, vel)
    assert np.array_equal(want, restate(d, k, margin, max_keep, lookahead, vel)[0])
    for ahead in (None, np.zeros(1, F32)):
        rc, kept, passed, idx = call(lib, d.reshape(1, -1), ahead, vel, k, margin, max_keep, lookahead)
        assert rc == 0 and (kept, passed) == (len(want), want_passed) and np.array_equal(idx, want), (name, ahead)


@pytest.mark.parametrize("case", [c for c in CASES if c[1].shape[0] > 1], ids=lambda c: c[0])
def test_order_and_repetition_of_the_states_change_nothing(lib, case):
    name, d, ahead, vel, k, margin, max_keep, lookahead = case
    rng = np.random.RandomState(5)
    want = call(lib, d, ahead, vel, k, margin, max_keep, lookahead)
    assert want[0] == 0
    p = rng.permutation(d.shape[0])
    twice = np.concatenate([np.arange(d.shape[0]), rng.randint(0, d.shape[0], 3)])
    for rows in (p, p[::-1], twice):
        got = call(lib, d[rows], None if ahead is None else ahead[rows], vel, k, margin, max_keep, lookahead)
        assert got[:3] == want[:3] and np.array_equal(got[3], want[3]), (name, rows)


def test_argument_checks_write_nothing(lib):
    d = np.stack([np.linspace(0.1, 1.0, 40), np.linspace(1.0, 0.1, 40)]).astype(F32)
    for margin, max_keep, lookahead in ((-0.1, 0, 0.0), (np.nan, 0, 0.0), (-np.inf, 0, 0.0), (0.1, 0, -1.0), (0.1, 0, np.inf), (0.1, 0, np.nan),
                                        (0.1, 9, 0.0), (0.1, 1, 0.0)):
        assert call(lib, d, None, None, 10, margin, max_keep, lookahead)[:3] == (ERR_INVALID_ARG, -1, -1), (margin, max_keep, lookahead)
    assert call(lib, d, None, None, 10, 0.1, 10, 0.0)[:2] == (0, 10)
    assert call(lib, d, None, None, 10, INF, -5, 0.0)[:3] == (0, 40, 40)
    assert call(lib, d[:, :9], None, None, 10, 0.1, 0, 0.0)[:3] == (ERR_INVALID_ARG, -1, -1)      # n_obs < n_closest
    assert call(lib, d, None, None, 0, 0.1, 0, 0.0)[:3] == (ERR_INVALID_ARG, -1, -1)              # n_closest < 1
    for n_states in (0, -1):
        assert call(lib, d, None, None, 10, 0.1, 0, 0.0, n_states=n_states)[:3] == (ERR_INVALID_ARG, -1, -1)
    assert b"n_states" in lib.omds_last_error(None)
    vel = np.zeros((40, 3), F32)
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        for v in (None, vel):      # checked without velocities too
            for at in (0, 1):
                ahead = np.zeros(2, F32)
                ahead[at] = bad
                assert call(lib, d, ahead, v, 10, 0.1, 0, 0.0)[:3] == (ERR_INVALID_ARG, -1, -1), (bad, at)
    assert b"ahead" in lib.omds_last_error(None)
    assert call(lib, d, np.array([-0.0, 3.0], F32), vel, 10, 0.1, 0, 0.0)[0] == 0
    spec = spec_of(0.1)
    idx, kept, passed = np.full(40, -7, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    args = [C.byref(spec), d.ctypes.data, None, None, 2, 40, 10, idx.ctypes.data, 40, kept.ctypes.data, passed.ctypes.data]
    for null in (0, 1, 7, 9, 10):
        a = list(args)
        a[null] = None
        assert lib.omds_obstacle_focus_select_path(*a) == ERR_INVALID_ARG
        assert (idx == -7).all() and kept[0] == -1 and passed[0] == -1
    assert lib.omds_obstacle_focus_select_path(*args) == 0 and kept[0] >= 10


def test_cap_below_kept_sets_the_counts_only(lib):
    d = np.stack([np.linspace(0.1, 1.0, 40), np.linspace(1.0, 0.1, 40)]).astype(F32)
    want, want_passed = restate_path(d, 10, 0.2)
    assert len(want) > 20
    rc, kept, passed, idx = call(lib, d, None, None, 10, 0.2, 0, 0.0, cap=len(want) - 1)
    assert rc == ERR_INVALID_ARG and (kept, passed) == (len(want), want_passed) and len(idx) == 0
    rc, kept, passed, idx = call(lib, d, None, None, 10, 0.2, 0, 0.0, cap=len(want))          # exactly cap fits
    assert rc == 0 and np.array_equal(idx, want)


def test_python_wrapper(lib):
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import obstacle_focus_select_path
    d = np.stack([np.linspace(1.0, 0.1, 40), np.linspace(0.1, 1.0, 40)])
    idx, passed = obstacle_focus_select_path(d, 10, 0.2, max_keep=22, ahead=[0.0, 0.5])
    want, want_passed = restate_path(d, 10, 0.2, 22, ahead=np.array([0.0, 0.5], F32))
    assert idx.dtype == np.int32 and np.array_equal(idx, want) and passed == want_passed
    with pytest.raises(_lib.OmdsError, match="ahead"):
        obstacle_focus_select_path(d, 10, 0.2, ahead=[0.0, -1.0])
    with pytest.raises(ValueError):
        obstacle_focus_select_path(d, 10, 0.2, ahead=[0.0])
    with pytest.raises(ValueError):
        obstacle_focus_select_path(d[0], 10, 0.2)


def _pack_case(d, ahead, vel, k, margin, max_keep, lookahead, cap, null_mask=0, n_states=None):
    d = np.ascontiguousarray(d, F32)
    B = d.shape[0] if n_states is None else n_states
    raw = bytes(spec_of(margin, max_keep, lookahead)) + struct.pack("<iiiiiii", B, d.shape[1], k, cap, 0 if ahead is None else 1,
                                                                    0 if vel is None else 1, null_mask)
    raw += d[:max(B, 0)].tobytes()
    if ahead is not None:
        raw += np.ascontiguousarray(ahead, F32).tobytes()
    return raw if vel is None else raw + np.ascontiguousarray(vel, F32).tobytes()


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    """tests/obstacle_focus_path_host.cpp, a stand-alone program around the header both the library and its kernels include, built with
    -fsanitize=address,undefined and run on the cases above: a clean exit, and the library's answers."""
    exe = sanitized_host_program("obstacle_focus_path_host", tmp_path)
    runs = []
    for name, d, ahead, vel, k, margin, max_keep, lookahead in CASES:
        kept = len(restate_path(d, k, margin, max_keep, lookahead, ahead, vel)[0])
        runs.append((d, ahead, vel, k, margin, max_keep, lookahead, kept, 0, None))          # exactly cap: the last index ends the buffer
    for name, d, vel, k, margin, max_keep, lookahead in SINGLE:
        kept = len(restate(d, k, margin, max_keep, lookahead, vel)[0])
        runs.append((d.reshape(1, -1), None, vel, k, margin, max_keep, lookahead, kept, 0, None))
    d = np.stack([np.linspace(0.1, 1.0, 40), np.linspace(1.0, 0.1, 40)]).astype(F32)
    runs.append((d, None, None, 10, 0.2, 0, 0.0, 3, 0, None))                                # cap < kept: counts only
    runs.append((d, None, None, 10, 0.2, 0, 0.0, 0, 0, None))
    runs.append((d[:, :9], None, None, 10, 0.2, 0, 0.0, 9, 0, None))                         # n_obs < n_closest
    runs.append((d, None, None, 10, -1.0, 0, 0.0, 40, 0, None))
    runs.append((d, None, None, 10, 0.1, 5, 0.0, 40, 0, None))
    runs.append((d, None, None, 10, 0.1, 0, 0.0, 40, 0, 0))                                  # n_states 0: nothing is read
    runs.append((d, np.array([0.0, -1.0], F32), None, 10, 0.1, 0, 0.0, 40, 0, None))
    runs.append((d, np.array([np.nan, 0.0], F32), np.zeros((40, 3), F32), 10, 0.1, 0, 0.0, 40, 0, None))
    for mask in (1, 2, 4, 8, 16):
        runs.append((d, None, None, 10, 0.2, 0, 0.0, 40, mask, None))
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(runs)) + b"".join(_pack_case(*r) for r in runs))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "obstacle_focus_path_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off = fout.read_bytes(), 0
    for d, ahead, vel, k, margin, max_keep, lookahead, cap, mask, n_states in runs:
        rc, kept, passed, written = struct.unpack_from("<iiii", raw, off)
        off += 16
        got = np.frombuffer(raw, np.int32, written, off)
        off += written * 4
        if mask:
            assert rc == ERR_INVALID_ARG and written == 0
            continue
        want_rc, want_kept, want_passed, want = call(lib, d, ahead, vel, k, margin, max_keep, lookahead, cap=cap, n_states=n_states)
        assert (rc, kept, passed) == (want_rc, want_kept, want_passed)
        assert np.array_equal(got, want)
    assert off == len(raw)
