"""The screened step's launch plan (optimalmodulationds_amd/csrc/screen_plan_def.h: who owns which pairs of a k_screen launch, how many
workgroups and result tiles, how much LDS; the rounds of the audit kernels; the LDS of the k_exact / k_audit launches) on the host: no
library, no GPU.  tests/screen_plan_host.cpp, a stand-alone program around the header the kernels and their launchers include, is built
under AddressSanitizer + UBSan and answers every case here in one run.

(a) the plan is the launcher's former inline text (`restate_plan` below, written from omds_launch_screen as it stood before the header
    existed, EXPERIMENTS.md R26), field by field;
(b) the workgroups' chunks tile [0, B O) exactly once, in order, none empty, whole rollouts in select mode;
(c) the result buffer holds the largest chunk and never exceeds SC_MAX_TILES;
(d) the LDS sizes are the former expressions and fit the configured maximum;
(e) the flush phase selects exactly when asked and O <= 5120;
(f) the audit rounds cover the list once, with the former 64- / 32-row choice, on the former grid;
(g) the k_exact / k_audit LDS bytes are the former literals."""
import itertools
import struct
import subprocess

import pytest

from helpers import sanitized_host_program

BS = (1, 7, 8, 9, 96, 255, 256, 257, 300, 1024, 4096)
OS = (1, 31, 32, 33, 64, 65, 255, 256, 257, 512, 513, 600, 5119, 5120, 5121, 6000)
GRID = list(itertools.product(BS, OS, (1, 2, 3, 4), (64, 256), (0, 1)))   # B, O, nhh, ncu, want_select
# the literals of csrc/screen_kernel.hip before the header: 8 waves x 32 pairs, a ring of 4 slices of 16 KB, 20 result tiles
ROWS, MAX_TILES, RING, SLICE, WIDTH, LDH = 256, 20, 4, 16384, 256, 260


def audit_ns(G):
    return (0, 1, 63, 64, 65, 32 * G, 32 * G + 1, 64 * G, 64 * G + 1, int(2.2 * 64 * G))


AUDIT = [(n, G, cap) for G in (1, 512) for n in audit_ns(G) for cap in (n,)] + [(0, 1, cap) for cap in (1, 63, 64, 65, 32767, 32768, 32769, 10 ** 6)]


def restate_plan(B, O, nhh, ncu, want):
    """omds_launch_screen's inline plan: (selects, unit, units_base, units_rem, grid, res_tiles, lds, lds_max)"""
    total = B * O
    lds0 = lambda n: RING * SLICE + (n + 2) * WIDTH * 4   # noqa: E731  omds_screen_lds_bytes
    selects = bool(want) and O <= MAX_TILES * ROWS
    if selects:
        rmax = max(1, MAX_TILES * ROWS // O)
        gl = max(min(B, ncu), (B + rmax - 1) // rmax)
        unit, base, rem = O, B // gl, B % gl
        tiles = ((base + (1 if rem else 0)) * O + ROWS - 1) // ROWS
    else:
        ntiles = (total + ROWS - 1) // ROWS
        gl = max(min(ntiles, ncu), (ntiles + MAX_TILES - 1) // MAX_TILES)
        tiles = (ntiles + gl - 1) // gl
        unit, base, rem = ROWS, ntiles // gl, ntiles % gl
    return (int(selects), unit, base, rem, gl, tiles, lds0(nhh) + tiles * ROWS * 4, lds0(4) + MAX_TILES * ROWS * 4)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """ask(kind, a, b, c, d, e) -> the program's words for that case, from ONE run over everything this module asks"""
    tmp = tmp_path_factory.mktemp("screen_plan")
    exe = sanitized_host_program("screen_plan_host", tmp)
    asks = [(0, *g) for g in GRID] + [(1, n, G, cap, 0, 0) for n, G, cap in AUDIT] + [(2, nhh, 0, 0, 0, 0) for nhh in range(1, 9)]
    fin, fout = tmp / "cases.bin", tmp / "out.bin"
    fin.write_bytes(struct.pack("<i", len(asks)) + b"".join(struct.pack("<6i", *a) for a in asks))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "screen_plan_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw = fout.read_bytes()
    words = struct.unpack(f"<{len(raw) // 8}q", raw)
    table, at = {}, 0
    for a in asks:
        n = 10 + 3 * words[at + 4] if a[0] == 0 else 5 + 2 * a[2] if a[0] == 1 else 13
        table[a] = words[at:at + n]
        at += n
    assert at == len(words)
    return lambda *a: table[tuple(a)]


def chunks(got):
    return [got[10 + 3 * w:13 + 3 * w] for w in range(got[4])]


def test_the_plan_is_the_launchers_former_text(plan):
    for g in GRID:
        got = plan(0, *g)
        assert got[:8] == restate_plan(*g), g
        assert got[8] == g[0] * g[1]


def test_the_chunks_tile_the_pair_space_once_and_in_order(plan):
    for g in GRID:
        B, O = g[0], g[1]
        got = plan(0, *g)
        end = 0
        for p0, p1, tiles in chunks(got):
            assert p0 == end and p1 > p0, (g, p0, p1, end)                    # in order, no gap, no overlap, at least one pair
            assert tiles == (p1 - p0 + ROWS - 1) // ROWS
            if got[0]:
                assert p0 % O == 0 and p1 % O == 0, (g, p0, p1)               # whole rollouts
            end = p1
        assert end == B * O, g


def test_the_result_buffer_holds_the_largest_chunk(plan):
    for g in GRID:
        got = plan(0, *g)
        assert 1 <= got[5] <= MAX_TILES, g
        assert got[5] * ROWS >= max(p1 - p0 for p0, p1, _ in chunks(got)), g
        assert got[5] == max(t for _, _, t in chunks(got)), g                 # ... and not a tile more


def test_the_lds_fits_the_configured_maximum(plan):
    for g in GRID:
        got = plan(0, *g)
        assert got[6] <= got[7] == RING * SLICE + 6 * WIDTH * 4 + MAX_TILES * ROWS * 4 <= 160 * 1024, g
        assert got[6] == RING * SLICE + (g[2] + 2) * WIDTH * 4 + got[5] * ROWS * 4, g
    for nhh in range(1, 9):
        assert plan(2, nhh, 0, 0, 0, 0)[2] == RING * SLICE + (nhh + 2) * WIDTH * 4


def test_the_flush_phase_selects_when_asked_and_rows_fit(plan):
    for g in GRID:
        got = plan(0, *g)
        assert got[0] == int(bool(g[4]) and g[1] <= 5120), g
        assert got[9] == int(g[1] <= 5120), g
    assert plan(0, 96, 5120, 4, 256, 1)[9] == 1 and plan(0, 96, 5121, 4, 256, 1)[9] == 0


def test_the_geometry_is_the_former_literals(plan):
    assert plan(2, 1, 0, 0, 0, 0)[3:] == (8, 512, ROWS, SLICE, RING, 3, 2, MAX_TILES, 8, 3)


@pytest.mark.parametrize("G", (1, 512))
def test_the_audit_rounds_cover_the_list_once(plan, G):
    for n in audit_ns(G):
        got = plan(1, n, G, n, 0, 0)
        grid, full, rest0, rest, last64 = got[:5]
        # the former kernel text: full = n / (64 G) rounds of 64-row tiles, then 64-row tiles when more than 32 G entries are left
        assert (full, rest0, rest, last64) == (n // (64 * G), n // (64 * G) * 64 * G, n - n // (64 * G) * 64 * G, int(n - n // (64 * G) * 64 * G > 32 * G)), (n, G)
        rows = 64 if last64 else 32
        seen = [0] * n
        for r in range(full):
            for w in range(G):
                for e in range((r * G + w) * 64, (r * G + w) * 64 + 64):
                    seen[e] += 1                                              # a full round lies below n: an IndexError is a finding
        for w in range(G):
            in_last, row0 = got[5 + 2 * w], got[6 + 2 * w]
            assert row0 == rest0 + w * rows and in_last == int(w * rows < rest), (n, G, w)
            if in_last:
                for e in range(row0, min(row0 + rows, n)):                    # pass1_tile stops at the list's end
                    seen[e] += 1
        assert all(s == 1 for s in seen), (n, G)


def test_the_audit_grid_is_the_former_expression(plan):
    for n, G, cap in AUDIT:
        assert plan(1, n, G, cap, 0, 0)[0] == min((cap + 63) // 64, 512), cap


def test_exact_and_audit_lds_are_the_former_literals(plan):
    for nhh in range(1, 9):
        got = plan(2, nhh, 0, 0, 0, 0)
        assert got[0] == 16 * LDH * 4 + 16 * 4 + 16 * 4 + 16 * (nhh + 1) * 8 * 4, nhh   # omds_launch_exact
        assert got[1] == 64 * LDH * 4 + 64 * 4 + 64 * 4, nhh                            # omds_launch_audit
