"""The fused tails' plan (optimalmodulationds_amd/csrc/tail_plan_def.h: the tile height of a launch of k_tail / k_tail_sel, the table of
their instantiations, the key a launch looks up, the size of their LDS block) on the host: no library, no GPU.
tests/tail_plan_host.cpp, a stand-alone program around the header tail_kernel.hip includes, is built under AddressSanitizer + UBSan
and answers every case here in one run.

(a) totality: over the whole grid the key either launcher looks up is in the table, and the table is exactly the 18 kernels;
(b) the choosers are the functions they were before the header existed: `restate_*` below are written from tail_kernel.hip as it
    stood then (EXPERIMENTS.md R25), compared over the grid, and the literals their comments name are pinned;
(c) the LDS size is the literal expression of the former tail_lds_bytes, the block offsets are the former pointer chain, and the
    carve ends inside the size;
(d) the tanh scratch covers every tile height either chooser can return."""
import itertools
import struct
import subprocess

import pytest

from helpers import sanitized_host_program

RELU, TANH = 0, 1                                     # OMDS_ACT_*
N_DOF, ACTS, FORCED, NCU = (2, 7), (RELU, TANH), (0, 4, 16, 32), (64, 256)
NS = (1, 40, 83, 128, 129, 300, 512, 768, 769, 1024, 1500, 4096, 8192)
KS = tuple(range(1, 33))
MAX_NHID = 8 + 1                                      # OMDS_MAX_HIDDEN + 1

# k_tail<n_dof, act, rows, frame> / k_tail_sel<n_dof, rows, act, frame>: what the launch ladders instantiated
KERNELS = {(nd, act, rows, frame) for nd in N_DOF for act, rows, frame in
           [(RELU, 4, 0), (RELU, 16, 0), (RELU, 32, 0), (TANH, 16, 0), (TANH, 32, 0), (RELU, 16, 1), (RELU, 32, 1), (TANH, 16, 1), (TANH, 32, 1)]}


def restate_frame_rows(rows, k):
    return rows if rows != 4 else (16 if k <= 16 else 32)


def restate_tail_rows(N, k, g4_ok, ncu, forced):
    if k > 16:
        return 32
    if forced == 4 and g4_ok and k <= 20:
        return 4
    if forced in (16, 32):
        return forced
    rw32 = 32 // k
    if (N + rw32 - 1) // rw32 <= 128:
        return 16
    if forced == 0 and g4_ok and k <= 10:
        rw4 = 20 // k
        if (N + rw4 - 1) // rw4 <= ncu:
            return 4
    return 32


def restate_sel_rows(N, k, g4_ok, ncu, forced):
    if k > 16:
        return 32
    if forced == 4 and g4_ok and k <= 20:
        return 4
    if forced in (16, 32):
        return forced
    rw16 = 16 // k
    wg16 = (N + rw16 - 1) // rw16
    if forced == 0 and g4_ok and k <= 10:
        rw4 = 20 // k
        wg4 = (N + rw4 - 1) // rw4
        cost16, cost4 = ((wg16 + ncu - 1) // ncu) * 8192, ((wg4 + ncu - 1) // ncu) * (5 * 2048 * 11 // 10)
        if wg16 > ncu and cost4 < cost16:
            return 4
    return 16 if wg16 <= 512 else 32


def restate_keys(nd, act, plain, frame, N, k, ncu, forced):
    """the (n_dof, act, rows, frame) omds_launch_tail and omds_launch_tail_sel launched, as their ladders chose them"""
    rows = restate_tail_rows(N, k, act == RELU and plain, ncu, forced)
    if frame:
        rows = restate_frame_rows(rows, k)
    if frame:
        srows = restate_frame_rows(restate_sel_rows(N, k, False, ncu, forced), k)
    elif act == TANH:
        srows = restate_sel_rows(N, k, False, ncu, forced)
    else:
        srows = restate_sel_rows(N, k, bool(plain), ncu, forced)
    return (nd, act, rows, frame), (nd, act, srows, frame)


def restate_scratch_rows(N, k):
    rw32 = 32 // k
    rows = (N + rw32 - 1) // rw32 * 32
    if k <= 16:
        rw16 = 16 // k
        rows = max(rows, (N + rw16 - 1) // rw16 * 16)
    return rows


GRID = list(itertools.product(N_DOF, ACTS, (1, 0), (0, 1), FORCED, NCU, KS, NS))   # n_dof, act, plain, frame, forced, ncu, k, N
# (256 CUs, ReLU without skips, no frame, nothing forced) for the pinned literals, beside the grid's own points
PIN_POINTS = [(7, act, 1, 0, 0, 256, k, N) for act in ACTS for k in (5, 17) for N in NS]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """ask(kind, n_dof, act, plain, frame, forced, ncu, k, N) -> the program's eight numbers, from ONE run over everything this module asks"""
    tmp = tmp_path_factory.mktemp("tail_plan")
    exe = sanitized_host_program("tail_plan_host", tmp)
    asks = sorted({(0, *g) for g in GRID + PIN_POINTS} | {(1, 0, 0, 0, 0, 0, 0, 0, nhid) for nhid in range(1, MAX_NHID + 1)} |
                  {(2, 0, 0, 0, 0, 0, 0, 0, i) for i in range(0, 40)})
    fin, fout = tmp / "cases.bin", tmp / "out.bin"
    fin.write_bytes(struct.pack("<i", len(asks)) + b"".join(struct.pack("<9i", *a) for a in asks))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tail_plan_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw = fout.read_bytes()
    assert len(raw) == 32 * len(asks)
    table = {a: struct.unpack_from("<8i", raw, 32 * i) for i, a in enumerate(asks)}
    return lambda *a: table[tuple(a)]


def _table(plan):
    n = plan(2, 0, 0, 0, 0, 0, 0, 0, 0)[0]
    return [plan(2, 0, 0, 0, 0, 0, 0, 0, i)[1:5] for i in range(n)]


def test_the_table_is_the_eighteen_kernels(plan):
    keys = _table(plan)
    assert len(keys) == 18 and len(set(keys)) == 18, "a key is stated once"
    assert set(keys) == KERNELS
    assert plan(2, 0, 0, 0, 0, 0, 0, 0, 18)[1:5] == (-1, -1, -1, -1)


def test_every_launch_of_the_grid_finds_its_kernel(plan):
    keys = _table(plan)
    for g in GRID:
        nd, act, plain, frame, forced, ncu, k, N = g
        it, rows_t, isel, rows_s = plan(0, *g)[:4]
        want_t, want_s = restate_keys(nd, act, plain, frame, N, k, ncu, forced)
        assert it >= 0 and keys[it] == (nd, act, rows_t, frame) == want_t, g
        assert isel >= 0 and keys[isel] == (nd, act, rows_s, frame) == want_s, g


def test_the_choosers_are_the_functions_they_were(plan):
    for g in GRID:
        nd, act, plain, frame, forced, ncu, k, N = g
        got = plan(0, *g)
        g4_ok = act == RELU and bool(plain)
        assert got[4] == restate_tail_rows(N, k, g4_ok, ncu, forced), g
        assert got[5] == restate_sel_rows(N, k, g4_ok, ncu, forced), g
        assert got[6] == restate_scratch_rows(N, k), g
        assert got[7] == restate_frame_rows(4, k), g


# the literals of the choosers' own comments, at 256 CUs, ReLU without skips, k = 5: (field 4 omds_tail_rows | 5 tail_sel_rows, N, rows)
PINS = [(4, 768, 16),      # 128 workgroups of 32 rows
        (4, 769, 4), (4, 1024, 4), (4, 4096, 32), (5, 1024, 4), (5, 4096, 4), (5, 1500, 16)]


@pytest.mark.parametrize("field,N,rows", PINS, ids=[f"{'tail' if f == 4 else 'sel'}-N{N}" for f, N, _ in PINS])
def test_pinned_tile_heights(plan, field, N, rows):
    assert plan(0, 7, RELU, 1, 0, 0, 256, 5, N)[field] == rows


def test_pinned_edges(plan):
    for N in NS:
        assert plan(0, 7, RELU, 1, 0, 0, 256, 17, N)[4:6] == (32, 32)                   # k = 17: 32 rows from both
    for forced, ncu in itertools.product(FORCED, NCU):                                  # tanh at N = 1024 never gives 4
        got = plan(0, 7, TANH, 1, 0, forced, ncu, 5, 1024)
        assert 4 not in (got[1], got[3], got[4], got[5])
    assert plan(0, 7, RELU, 1, 0, 0, 256, 5, 1024)[7] == 16 and plan(0, 7, RELU, 1, 0, 0, 256, 17, 1024)[7] == 32   # frame_rows(4, k)
    assert all(plan(0, 7, RELU, 1, 1, forced, 256, 5, 1024)[1] != 4 and plan(0, 7, RELU, 1, 1, forced, 256, 5, 1024)[3] != 4 for forced in FORCED)


def test_lds_bytes_are_the_former_expression(plan):
    """the launch's size is the literal expression of the former tail_lds_bytes (+ 128 bytes of sel for k_tail_sel); the carve's offsets
    are the former pointer chain of the two kernels, restated here in bytes, and the carve ends inside the launch's size"""
    P2_MT, P2_NT, LDH, OMDS_MAX_DOF = 32, 512, 260, 7
    for nhid in range(1, MAX_NHID + 1):
        former = (P2_MT * LDH + 32 * 33) * 4 + nhid * P2_NT * 4 + 3 * P2_MT * 4 + (32 * 12 + 32 + 32 * 3 * OMDS_MAX_DOF) * 4   # tail_lds_bytes(nhid)
        got = plan(1, 0, 0, 0, 0, 0, 0, 0, nhid)
        assert got[:2] == (former, former + 32 * 4), nhid
        maskL = (P2_MT * LDH + 32 * 33) * 4                          # sm.maskL = sm.gf + 32 * 33 floats behind the tile
        rowT = maskL + ((nhid - 1 + 2) // 2 * 2) * P2_NT * 2         # + ((m.nhh + 2) / 2 * 2) * P2_NT halfwords
        gx = rowT + 3 * P2_MT * 4                                    # rowT, rowO, rowMin
        sel = gx + (32 * 12 + 32 + 32 * 3 * OMDS_MAX_DOF) * 4        # gx, dr, feat
        assert got[2:8] == (maskL, rowT, gx, sel, sel + 32 * 4, sel), nhid
        assert got[6] <= got[1] and got[7] <= got[0], nhid


def test_the_tanh_scratch_covers_every_tile_height(plan):
    for g in GRID:
        k, N = g[6], g[7]
        got = plan(0, *g)
        for rows in {got[1], got[3], got[4], got[5]} - {4}:     # (4-row groups are ReLU's: no derivative scratch)
            rw = rows // k
            assert rows * ((N + rw - 1) // rw) <= got[6], (g, rows)
