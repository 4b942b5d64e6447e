"""The propagate's schedule (optimalmodulationds_amd/csrc/propagate_plan_def.h: omds_pipeline_plan -- one stream, or the full steps of
the Dense route as two halves of the batch on two streams) on the host: no library, no GPU.  tests/propagate_plan_host.cpp, a stand-alone
program around the header propagate.hip includes, is built under AddressSanitizer + UBSan and answers every case here in one run.

(a) over a grid of (N, O, H, shared, route, flags, blocks_ok) the plan is the rule restated below from the header's comment;
(b) both sides of every threshold: the pair floor per part, the size class of the smaller part, the full steps, the order limits;
(c) split is a multiple of 16 and both parts are non-empty wherever the plan says two parts;
(d) each flag on its own, both together (serial), and every route but Dense (one part)."""
import itertools
import struct
import subprocess

import pytest

from helpers import sanitized_host_program

UNFUSED, SMALL_SCENE, DENSE, EMIT, SCREEN_LIST, SCREEN_MATRIX = range(6)      # StepRoute
BLOCK_TILES, SERIAL, PIPELINED = 64, 128, 256                                 # OMDS_FLAG_*
MIN_PAIRS = 131072                                                            # OMDS_BLOCK_TILES_MIN_PAIRS
MAX_N, MAX_O = 8192, 4096                                                     # OMDS_ORDER_MAX_ROLLOUTS / _OBS
MIN_STEPS, MIN_STEPS_FORCED = 3, 2

NS = (1, 2, 16, 17, 31, 32, 33, 48, 70, 128, 129, 300, 512, 892, 893, 894, 896, 1024, 1029, 4096, 8191, 8192, 8193)
OS = (1, 32, 40, 294, 500, 4096, 4097)
HS = (1, 2, 3, 4, 5, 32)
FLAGS = (0, BLOCK_TILES, SERIAL, PIPELINED, SERIAL | PIPELINED, PIPELINED | BLOCK_TILES, SERIAL | BLOCK_TILES, 4 | 8)
GRID = list(itertools.product(NS, OS, HS, (0, 1), range(6), FLAGS, (0, 1)))
EXTRA = [(N, 294, H, sh, DENSE, fl, 1) for N in range(880, 900) for H in (3, 4) for sh in (0, 1) for fl in (0, BLOCK_TILES)]


def restate_split(N):
    return ((N + 1) // 2 + 15) // 16 * 16


def restate(N, O, H, shared, route, flags, blocks_ok):
    serial = (1, N)
    if route != DENSE or not blocks_ok or flags & SERIAL:
        return serial
    if N < 2 or O < 1 or N > MAX_N or O > MAX_O:
        return serial
    split, full = restate_split(N), H - (1 if shared else 0)
    if split >= N:
        return serial
    if flags & PIPELINED:
        return (2, split) if full >= MIN_STEPS_FORCED else serial
    rest = N - split
    if full < MIN_STEPS or rest * O <= 32 * 128 or rest * O < MIN_PAIRS:
        return serial
    return (2, split)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("propagate_plan")
    exe = sanitized_host_program("propagate_plan_host", tmp)
    asks = sorted(set(GRID + EXTRA))
    fin, fout = tmp / "cases.bin", tmp / "out.bin"
    fin.write_bytes(struct.pack("<i", len(asks)) + b"".join(struct.pack("<7i", *a) for a in asks))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "propagate_plan_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    raw = fout.read_bytes()
    assert len(raw) == 16 * len(asks)
    table = {a: struct.unpack_from("<4i", raw, 16 * i) for i, a in enumerate(asks)}
    return lambda *a: table[tuple(a)]


def test_the_plan_is_the_rule_over_the_grid(plan):
    two = 0
    for g in GRID + EXTRA:
        parts, split, split_of_n, _ = plan(*g)
        assert (parts, split) == restate(*g), g
        assert split_of_n == restate_split(g[0])
        two += parts == 2
    assert 0 < two < len(GRID), "the grid must hold both answers"


def test_two_parts_are_whole_blocks_and_non_empty(plan):
    for g in GRID + EXTRA:
        parts, split, _, _ = plan(*g)
        N = g[0]
        if parts == 2:
            assert split % 16 == 0 and 0 < split < N and split >= N - split, g
        else:
            assert split == N, g
    assert plan(32, 40, 3, 1, DENSE, PIPELINED, 1)[:2] == (2, 16)      # parts of 16 / 16
    assert plan(33, 40, 3, 1, DENSE, PIPELINED, 1)[:2] == (2, 32)      # ... of 32 / 1
    assert plan(48, 40, 3, 1, DENSE, PIPELINED, 1)[:2] == (2, 32)
    assert plan(70, 40, 3, 1, DENSE, PIPELINED, 1)[:2] == (2, 48)
    assert plan(16, 40, 3, 1, DENSE, PIPELINED, 1)[:2] == (1, 16)      # one block: nothing to part
    assert plan(17, 40, 3, 1, DENSE, PIPELINED, 1)[:2] == (2, 16)


def test_both_sides_of_the_thresholds(plan):
    # the pair floor per part at 294 obstacles: the smaller part of 894 rollouts is 446 (131 124 pairs), of 893 it is 445 (130 830)
    assert 446 * 294 >= MIN_PAIRS > 445 * 294
    assert plan(894, 294, 4, 1, DENSE, 0, 1)[:2] == (2, 448)
    assert plan(893, 294, 4, 1, DENSE, 0, 1)[:2] == (1, 893)
    assert plan(893, 294, 4, 1, DENSE, BLOCK_TILES, 1)[:2] == (1, 893), "OMDS_FLAG_BLOCK_TILES does not lower the floor of the parts"
    # full steps: three by default (the shared first step is none), two when forced
    assert plan(1024, 294, 4, 1, DENSE, 0, 1)[:2] == (2, 512) and plan(1024, 294, 3, 1, DENSE, 0, 1)[0] == 1
    assert plan(1024, 294, 3, 0, DENSE, 0, 1)[0] == 2 and plan(1024, 294, 2, 0, DENSE, 0, 1)[0] == 1
    assert plan(1024, 294, 3, 1, DENSE, PIPELINED, 1)[0] == 2 and plan(1024, 294, 2, 1, DENSE, PIPELINED, 1)[0] == 1
    assert plan(1024, 294, 2, 0, DENSE, PIPELINED, 1)[0] == 2 and plan(1024, 294, 1, 0, DENSE, PIPELINED, 1)[0] == 1
    # the order limits
    assert plan(8192, 294, 32, 1, DENSE, 0, 1)[:2] == (2, 4096) and plan(8193, 294, 32, 1, DENSE, 0, 1)[0] == 1
    assert plan(8192, 4096, 32, 1, DENSE, 0, 1)[0] == 2 and plan(8192, 4097, 32, 1, DENSE, 0, 1)[0] == 1
    assert plan(8193, 294, 32, 1, DENSE, PIPELINED, 1)[0] == 1 and plan(8192, 4097, 32, 1, DENSE, PIPELINED, 1)[0] == 1
    # the size class the block-ordered kernel serves by itself: more than 4096 pairs
    assert plan(129, 32, 1, 0, DENSE, 0, 1)[3] == 1 and plan(128, 32, 1, 0, DENSE, 0, 1)[3] == 0


def test_flags(plan):
    at = (1024, 294, 32, 1, DENSE)
    assert plan(*at, 0, 1)[:2] == (2, 512)
    assert plan(*at, SERIAL, 1)[:2] == (1, 1024)
    assert plan(*at, PIPELINED, 1)[:2] == (2, 512)
    assert plan(*at, SERIAL | PIPELINED, 1)[:2] == (1, 1024), "both flags: serial"
    small = (300, 294, 32, 1, DENSE)
    assert plan(*small, 0, 1)[0] == 1 and plan(*small, BLOCK_TILES, 1)[0] == 1
    assert plan(*small, PIPELINED, 1)[:2] == (2, 160)
    assert plan(*small, PIPELINED | SERIAL, 1)[0] == 1
    assert plan(*at, PIPELINED, 0)[0] == 1, "no block-ordered kernel for this context (tanh, skip connections, the natural order asked for)"


def test_every_other_route_is_one_part(plan):
    for route in (UNFUSED, SMALL_SCENE, EMIT, SCREEN_LIST, SCREEN_MATRIX):
        for flags in FLAGS:
            for N, O, H in ((1024, 294, 32), (8192, 294, 32), (70, 40, 5)):
                assert plan(N, O, H, 1, route, flags, 1)[:2] == (1, N), (route, flags, N)
