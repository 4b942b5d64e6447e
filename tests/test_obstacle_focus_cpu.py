"""The definition of the obstacle focus on the host (include/omds.h: omds_obstacle_focus_select; no context, no GPU) against a numpy
restatement in the header's operation order (tests/obstacle_focus_cases.py: fmaf from libm, float32 sqrt, lexsort on (r, o)): the kept
indices and both counts must match exactly.  The same cases also go through a stand-alone build of the definition under
AddressSanitizer + UBSan (tests/obstacle_focus_host.cpp, its buffers allocated at exactly the sizes passed), whose output must be the
library's."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from helpers import ROOT, sanitized_host_program
from obstacle_focus_cases import F32, INF, cases, restate

ERR_INVALID_ARG = 1
NAMES = ["omds_obstacle_focus_select", "omds_focus_obstacles", "omds_get_obstacle_focus", "omds_clear_obstacle_focus"]
CASES = cases()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def spec_of(margin, max_keep=0, lookahead=0.0):
    from optimalmodulationds_amd.engine import obstacle_focus_spec
    return obstacle_focus_spec(margin, max_keep, lookahead)


def call(lib, d, vel, k, margin, max_keep, lookahead, cap=None, n_obs=None):
    """(rc, kept, passed, idx [kept if rc == 0 else 0]) of the raw entry point; a refused call must leave idx_out alone"""
    d = np.ascontiguousarray(d, F32).reshape(-1)
    v = None if vel is None else np.ascontiguousarray(vel, F32).reshape(-1, 3)
    cap = d.size if cap is None else cap
    idx, kept, passed = np.full(max(cap, 1), -7, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    spec = spec_of(margin, max_keep, lookahead)
    rc = lib.omds_obstacle_focus_select(C.byref(spec), d.ctypes.data, None if v is None else v.ctypes.data, d.size if n_obs is None else n_obs,
                                        k, idx.ctypes.data, cap, kept.ctypes.data, passed.ctypes.data)
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
    assert "omds_obstacle_focus_spec" in header
    assert [f[0] for f in _lib.OmdsObstacleFocusSpec._fields_] == ["margin", "lookahead", "max_keep"] and C.sizeof(_lib.OmdsObstacleFocusSpec) == 12
    assert lib.omds_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_definition_matches_the_restatement(lib, case):
    name, d, vel, k, margin, max_keep, lookahead = case
    rc, kept, passed, idx = call(lib, d, vel, k, margin, max_keep, lookahead)
    want, want_passed = restate(d, k, margin, max_keep, lookahead, vel)
    assert rc == 0 and passed == want_passed and kept == len(want), (rc, kept, passed, len(want), want_passed)
    assert np.array_equal(idx, want)
    assert k <= kept <= passed <= d.size and (max_keep < 1 or kept <= max_keep)
    assert (np.diff(idx) > 0).all()


def test_cases_cover_what_they_name():
    """the cases do what their names say: a cap that cuts a tie group, NaNs below and above k, a far sphere pulled in"""
    by = {c[0]: c for c in CASES}
    _, d, _, k, m, _, _ = by["ties_keep15"]
    idx, passed = restate(d, k, m, 15)
    assert passed == 24 and len(idx) == 15 and 0 < (d[idx] == F32(0.5)).sum() < (d == F32(0.5)).sum()
    assert np.isnan(by["nan_few"][1]).sum() < 10 <= np.isnan(by["nan_many"][1]).sum()
    assert set(np.flatnonzero(np.isnan(by["nan_many"][1]))) <= set(restate(by["nan_many"][1], 10, 0.1)[0])
    _, d, vel, k, m, mk, la = by["lookahead_pulls_in"]
    assert 12 in restate(d, k, m, mk, la, vel)[0] and 12 not in restate(d, k, m, mk, 0.0, vel)[0]
    assert {14, 15} <= set(restate(*[by["velocity_not_finite"][i] for i in (1, 3, 4, 5, 6, 2)])[0])
    g = {n: restate(c[1], c[3], c[4])[1] for n, c in by.items() if n.startswith("margin_")}
    assert g["margin_zero"] == g["margin_below_gap"] == 10 and g["margin_gap"] == g["margin_above_gap"] == 11 and g["margin_inf"] == 41
    z = by["zeros_cut"]
    assert list(restate(z[1], z[3], z[4], z[5])[0]) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 17]     # -0.5 first, then the zeros by index


def test_shuffled_input_gives_the_same_set(lib):
    rng = np.random.RandomState(3)
    d = rng.uniform(0.0, 1.0, 700).astype(F32)              # distinct values: the set is a set of values
    assert len(np.unique(d)) == d.size
    vel = (0.2 * rng.standard_normal((700, 3))).astype(F32)
    _, _, _, idx = call(lib, d, vel, 10, 0.15, 120, 0.5)
    p = rng.permutation(d.size)
    rc, kept, _, idx2 = call(lib, d[p], vel[p], 10, 0.15, 120, 0.5)
    assert rc == 0 and kept == len(idx) and np.array_equal(np.sort(p[idx2]), idx)


def test_argument_checks_write_nothing(lib):
    d = np.linspace(0.1, 1.0, 40).astype(F32)
    for margin, max_keep, lookahead in ((-0.1, 0, 0.0), (np.nan, 0, 0.0), (-np.inf, 0, 0.0), (0.1, 0, -1.0), (0.1, 0, np.inf), (0.1, 0, np.nan),
                                        (0.1, 9, 0.0), (0.1, 1, 0.0)):
        rc, kept, passed, _ = call(lib, d, None, 10, margin, max_keep, lookahead)
        assert (rc, kept, passed) == (ERR_INVALID_ARG, -1, -1), (margin, max_keep, lookahead)
    assert call(lib, d, None, 10, 0.1, 10, 0.0)[:2] == (0, 10)          # max_keep = n_closest is allowed, and < 1 is no cap
    assert call(lib, d, None, 10, INF, -5, 0.0)[:3] == (0, 40, 40)
    assert call(lib, d[:9], None, 10, 0.1, 0, 0.0)[:3] == (ERR_INVALID_ARG, -1, -1)      # n_obs < n_closest
    assert call(lib, d, None, 0, 0.1, 0, 0.0)[:3] == (ERR_INVALID_ARG, -1, -1)           # n_closest < 1
    assert b"obstacle" in lib.omds_last_error(None)
    spec = spec_of(0.1)
    idx, kept, passed = np.full(40, -7, np.int32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    args = [C.byref(spec), d.ctypes.data, None, 40, 10, idx.ctypes.data, 40, kept.ctypes.data, passed.ctypes.data]
    for null in (0, 1, 5, 7, 8):
        a = list(args)
        a[null] = None
        assert lib.omds_obstacle_focus_select(*a) == ERR_INVALID_ARG
        assert (idx == -7).all() and kept[0] == -1 and passed[0] == -1
    assert lib.omds_obstacle_focus_select(*args) == 0 and kept[0] >= 10


def test_cap_below_kept_sets_the_counts_only(lib):
    d = np.linspace(0.1, 1.0, 40).astype(F32)
    want, want_passed = restate(d, 10, 0.2)
    rc, kept, passed, idx = call(lib, d, None, 10, 0.2, 0, 0.0, cap=len(want) - 1)
    assert rc == ERR_INVALID_ARG and (kept, passed) == (len(want), want_passed) and len(idx) == 0
    rc, kept, passed, idx = call(lib, d, None, 10, 0.2, 0, 0.0, cap=len(want))          # exactly cap fits
    assert rc == 0 and np.array_equal(idx, want)


def test_python_wrapper(lib):
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import obstacle_focus_select
    d = np.linspace(1.0, 0.1, 40)
    idx, passed = obstacle_focus_select(d, 10, 0.2, max_keep=12)
    want, want_passed = restate(d, 10, 0.2, 12)
    assert idx.dtype == np.int32 and np.array_equal(idx, want) and passed == want_passed
    with pytest.raises(_lib.OmdsError, match="margin"):
        obstacle_focus_select(d, 10, -1.0)


def _pack_case(d, vel, k, margin, max_keep, lookahead, cap, null_mask=0):
    d = np.ascontiguousarray(d, F32).reshape(-1)
    raw = bytes(spec_of(margin, max_keep, lookahead)) + struct.pack("<iiiii", d.size, k, cap, 0 if vel is None else 1, null_mask) + d.tobytes()
    return raw if vel is None else raw + np.ascontiguousarray(vel, F32).tobytes()


def test_definition_under_address_and_ub_sanitizer(lib, tmp_path):
    """tests/obstacle_focus_host.cpp, a stand-alone program around the header both the library and its kernels include, built with
    -fsanitize=address,undefined and run on the cases above: a clean exit, and the library's answers."""
    exe = sanitized_host_program("obstacle_focus_host", tmp_path)
    runs = []
    for name, d, vel, k, margin, max_keep, lookahead in CASES:
        kept = len(restate(d, k, margin, max_keep, lookahead, vel)[0])
        runs.append((d, vel, k, margin, max_keep, lookahead, kept, 0))              # exactly cap: the last index ends the buffer
    d = np.linspace(0.1, 1.0, 40).astype(F32)
    runs.append((d, None, 10, 0.2, 0, 0.0, 3, 0))                                   # cap < kept: counts only
    runs.append((d, None, 10, 0.2, 0, 0.0, 0, 0))
    runs.append((d[:9], None, 10, 0.2, 0, 0.0, 9, 0))                               # n_obs < n_closest
    runs.append((d, None, 10, -1.0, 0, 0.0, 40, 0))
    runs.append((d, None, 10, 0.1, 5, 0.0, 40, 0))
    for mask in (1, 2, 4, 8, 16):
        runs.append((d, None, 10, 0.2, 0, 0.0, 40, mask))
    fin, fout = tmp_path / "cases.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<i", len(runs)) + b"".join(_pack_case(*r) for r in runs))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "obstacle_focus_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw, off = fout.read_bytes(), 0
    for d, vel, k, margin, max_keep, lookahead, cap, mask in runs:
        rc, kept, passed, written = struct.unpack_from("<iiii", raw, off)
        off += 16
        got = np.frombuffer(raw, np.int32, written, off)
        off += written * 4
        if mask:
            assert rc == ERR_INVALID_ARG and written == 0
            continue
        want_rc, want_kept, want_passed, want = call(lib, d, vel, k, margin, max_keep, lookahead, cap=cap)
        assert (rc, kept, passed) == (want_rc, want_kept, want_passed)
        assert np.array_equal(got, want)
    assert off == len(raw)
