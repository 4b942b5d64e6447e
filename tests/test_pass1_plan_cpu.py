"""Pass 1's launch plan (optimalmodulationds_amd/csrc/pass1_plan_def.h: the size class of a launch, the natural-order and the block grid
and which rows a workgroup owns, the LDS blocks pass1_tile / pass1_tile_dyn carve and the LDS size of every launch that runs them, the
pair limit of the emitting launch, the small scene's tile choice; and pass 2's carve and size of tail_plan_def.h) on the host: no
library, no GPU.  tests/pass1_plan_host.cpp, a stand-alone program around the headers the kernels and their launchers include, is built
under AddressSanitizer + UBSan and answers every case here in one run.

The expected values are the launchers' and kernels' text as it stood before the header existed (EXPERIMENTS.md R31), restated below
with the lines of that text each one restates; none is read back from the header.

(a) the grid of every (total, compact) is the former expressions;
(b) under the inverse rule the tiles cover [0, total) once, in order, none empty;
(c) the block grid is the former expressions and its blocks cover N x O once;
(d) every byte count is the former literal for nhid 1 .. 9, at most its configured maximum and at most 160 KB;
(e) the carves' offsets are the former pointer chains in words, no block overlaps the next, the slot arrays end inside rowRad;
(f) the address k_step_small computed for maskS is the carve's;
(g) the emit predicate is true exactly up to 24 576 pairs, and every total it admits is Tiny or Small;
(h) k_pass2's carve is TailLdsPlan's first six blocks and its size the former expression;
and the small scene's rollouts per workgroup and tile height are the former functions."""
import itertools
import struct
import subprocess

import numpy as np
import pytest

from helpers import sanitized_host_program

LDH, WIDTH, IDS, MAX_NHID, MAX_DOF, SS_RK = 260, 256, 256 + 64, 9, 7, 4      # mfma_gemm.h, omds_internal.h, pass1_tile_dyn.h:34, omds.h, step_small.hip:30
TINY, SMALL, MEDIUM, LARGE = 0, 1, 2, 3
NEAR_2_31 = 2 ** 31 - 1 - 294                                                # "the launcher keeps total_rows below 2^31" (pass1_tile.h)
TOTALS = (1, 16, 17, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536, 65537) + tuple(N * 294 for N in (8, 40, 96, 129, 230, 448, 1024, 4096)) + (NEAR_2_31,)
BLOCK_NS, BLOCK_OS = (1, 7, 8, 9, 15, 16, 17, 129, 230, 8192), (1, 3, 4, 5, 294, 4096)
NHIDS = range(1, 10)
SMALL_SCENES = list(itertools.product((0, 1), (2, 3, 7), (0, 1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33), (0, 1, 2, 3, 4, 5)))   # plain_relu, n_dof, O, k


def size_class(total):
    """mlp_kernels.hip:347-352 pass1_size"""
    if total >= 64 * 1024:
        return LARGE
    if total >= 64 * 512:
        return MEDIUM
    if total > 32 * 128:
        return SMALL
    return TINY


def big_tiles(total):
    """mlp_kernels.hip:354 pass1_big_tiles"""
    return max(total // 64 - 256, 0)


def restate_grid(total, compact):
    """(big_rows, small_rows, n_big, n_small) of omds_launch_pass1: the compacting branch mlp_kernels.hip:375-383, the dense switch :386-394 with
    launch_pass1_a's tile count :328 and launch_pass1_mixed's :364-365; a launch of one tile height counts its tiles as big ones"""
    size = size_class(total)
    if compact and size != TINY:
        n_big = big_tiles(total) if size == LARGE else total // 64 if size == MEDIUM else 0
        return 64, 32, n_big, (total - n_big * 64 + 31) // 32
    if size == LARGE:
        n_big = big_tiles(total)
        return 64, 32, n_big, (total - n_big * 64 + 31) // 32
    mt = {MEDIUM: 64, SMALL: 32, TINY: 16}[size]
    return mt, mt, (total + mt - 1) // mt, 0


def restate_row0(b, n_big):
    """k_pass1_mixed mlp_kernels.hip:124-129, k_pass1_dyn :139-140"""
    return (64, b * 64) if b < n_big else (32, n_big * 64 + (b - n_big) * 32)


def restate_block_grid(N, O):
    """omds_launch_pass1_blocks mlp_kernels.hip:408-412: (ncb, nrb16, n_big, n_small)"""
    size = size_class(N * O)
    ncb = (O + 3) // 4
    nrb16 = max(N // 16 - (256 + ncb - 1) // ncb, 0) if size == LARGE else N // 16 if size == MEDIUM else 0
    return ncb, nrb16, nrb16 * ncb, (N - nrb16 * 16 + 7) // 8 * ncb


def restate_blocks(N, O):
    """k_pass1_dyn_blk mlp_kernels.hip:150-161 for every workgroup of the launch: rows (big, r0, o0, nr, no)"""
    ncb, nrb16, n_big, n_small = restate_block_grid(N, O)
    wg = np.arange(n_big + n_small, dtype=np.int64)
    big = wg < n_big
    b = np.where(big, wg, wg - n_big)
    rbk, cbk = b // ncb, b % ncb
    r0 = np.where(big, rbk * 16, nrb16 * 16 + rbk * 8)
    return np.stack([big.astype(np.int64), r0, cbk * 4, np.minimum(np.where(big, 16, 8), N - r0), np.minimum(4, O - cbk * 4)], axis=1)


def restate_small_lds(nhid, TR):
    """step_small.hip:228-229 small_lds_bytes"""
    return (TR * LDH + 2 * TR + TR * nhid * 8) * 4 + (32 * 3 + SS_RK * 3) * 4 + (SS_RK + SS_RK * 12 + 16 * 33 + SS_RK * 3 * MAX_DOF + 4) * 4 + 16 + (16 * LDH * 4 if TR == 16 else 0)


def restate_small_rollouts(plain, n_dof, O, k, rows):
    """step_small.hip:233-237 small_rollouts, `plain` standing for m.act == ReLU and no skip_mask"""
    if not plain or n_dof not in (7, 2):
        return 0
    if O < 1 or O > rows or k < 1 or k > SS_RK or k > O:
        return 0
    return max(1, min(rows // O, SS_RK // k))


def tile_queries(total, compact):
    """the (n_big, b0, count) runs of workgroups the test looks at: all of them, or -- the total near 2^31 -- both ends and the seam"""
    _, _, n_big, n_small = restate_grid(total, compact)
    n = n_big + n_small
    if n <= 100000:
        return [(n_big, 0, n)]
    return [(n_big, 0, 8), (n_big, max(n_big - 4, 0), min(8, n - max(n_big - 4, 0))), (n_big, n - 8, 8)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """ask(kind, a, b, c, d, e) -> the program's words for that case, from ONE run over everything this module asks"""
    tmp = tmp_path_factory.mktemp("pass1_plan")
    exe = sanitized_host_program("pass1_plan_host", tmp)
    asks = [(0, t, c, 0, 0, 0) for t in TOTALS for c in (0, 1)]
    asks += sorted({(1, *q, 0, 0) for t in TOTALS for c in (0, 1) for q in tile_queries(t, c)})
    asks += [(2, N, O, 0, 0, 0) for N in BLOCK_NS for O in BLOCK_OS]
    asks += [(3, nhid, 0, 0, 0, 0) for nhid in NHIDS]
    asks += [(4, MT, nhid, 0, 0, 0) for MT in (16, 32, 64) for nhid in NHIDS]
    asks += [(5, t, 0, 0, 0, 0) for t in (1, 4096, 4097, 24575, 24576, 24577, 32767, 32768, 65536, NEAR_2_31)]
    asks += [(6, nhid, 0, 0, 0, 0) for nhid in NHIDS]
    asks += [(7, *s, 0) for s in SMALL_SCENES]
    fin, fout = tmp / "cases.bin", tmp / "out.bin"
    fin.write_bytes(struct.pack("<i", len(asks)) + b"".join(struct.pack("<6i", *a) for a in asks))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pass1_plan_host: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    words = np.frombuffer(fout.read_bytes(), dtype="<i8")
    table, at = {}, 0
    for a in asks:
        n = {0: 6, 1: 2 * a[3], 2: 4, 3: 17, 4: 12, 5: 3, 6: 7, 7: 3}[a[0]]
        if a[0] == 2:
            n += 5 * int(words[at + 2] + words[at + 3])
        table[a] = words[at:at + n]
        at += n
    assert at == len(words)
    return lambda *a: table[tuple(a)]


def test_the_grid_is_the_launchers_former_text(plan):
    for total in TOTALS:
        for compact in (0, 1):
            got = [int(v) for v in plan(0, total, compact, 0, 0, 0)]
            assert got[0] == size_class(total) and got[1] == big_tiles(total), total
            assert tuple(got[2:]) == restate_grid(total, compact), (total, compact)
    # Tiny ends at 32 x 128 rows, Medium starts at 64 x 512, Large at 64 x 1024; the Medium class is where the two launches differ
    assert [size_class(t) for t in (4096, 4097, 32767, 32768, 65535, 65536)] == [TINY, SMALL, SMALL, MEDIUM, MEDIUM, LARGE]
    assert restate_grid(129 * 294, 0) == (64, 64, 593, 0) and restate_grid(129 * 294, 1) == (64, 32, 592, 2)


def test_the_tiles_cover_the_rows_once_and_in_order(plan):
    for total in TOTALS:
        for compact in (0, 1):
            big_rows, small_rows, n_big, n_small = restate_grid(total, compact)
            n = n_big + n_small
            if (big_rows, small_rows) != (64, 32):   # one tile height: k_pass1<MT> / k_pass1e<MT> take row0 = blockIdx.x * MT (mlp_kernels.hip:109, :173)
                assert n_small == 0 and (n - 1) * big_rows < total <= n * big_rows, (total, compact)
                continue
            end = 0
            for q in tile_queries(total, compact):
                got = plan(1, *q, 0, 0).reshape(-1, 2)
                if q[1] != 0:
                    end = restate_row0(q[1], n_big)[1]      # a sampled run: it starts where the former rule says
                for i, (rows, row0) in enumerate(got.tolist()):
                    assert (rows, row0) == restate_row0(q[1] + i, n_big), (total, compact, q, i)
                    assert row0 == end and row0 < total, (total, compact, q, i)       # in order, no gap, no overlap, none empty
                    end = row0 + rows
            assert end >= total > end - 32, (total, compact)                          # the last tile holds the last row


def test_the_block_grid_is_the_former_text_and_covers_every_pair_once(plan):
    clamped = 0
    for N in BLOCK_NS:
        for O in BLOCK_OS:
            got = plan(2, N, O, 0, 0, 0)
            ncb, nrb16, n_big, n_small = restate_block_grid(N, O)
            assert tuple(int(v) for v in got[:4]) == (ncb, nrb16, n_big, n_small), (N, O)
            clamped += size_class(N * O) == LARGE and N // 16 - (256 + ncb - 1) // ncb <= 0
            blocks = got[4:].reshape(-1, 5)
            assert len(blocks) == n_big + n_small
            assert (blocks == restate_blocks(N, O)).all(), (N, O)
            big, r0, o0, nr, no = blocks.T
            assert (big[:n_big] == 1).all() and (big[n_big:] == 0).all() and (nr >= 1).all() and (no >= 1).all(), (N, O)   # none empty
            assert (nr <= np.where(big == 1, 16, 8)).all() and (no <= 4).all(), (N, O)
            assert (r0 >= 0).all() and (r0 + nr <= N).all() and (o0 >= 0).all() and (o0 + no <= O).all(), (N, O)   # no slot past either order
            corners = np.zeros((N + 1, O + 1), np.int32)      # how often each pair is covered: the blocks' corners, summed along both axes
            for rr, oo, sign in ((r0, o0, 1), (r0 + nr, o0, -1), (r0, o0 + no, -1), (r0 + nr, o0 + no, 1)):
                np.add.at(corners, (rr, oo), sign)
            assert (corners.cumsum(0).cumsum(1)[:N, :O] == 1).all(), (N, O)
    assert clamped >= 2                                                               # N = 16 | 17 at O = 4096: Large, and no 16-rollout block is left


def test_every_lds_size_is_the_former_literal(plan):
    for nhid in NHIDS:
        got = [int(v) for v in plan(3, nhid, 0, 0, 0, 0)]
        dmin = [MT * LDH * 4 + MT * 4 for MT in (16, 32, 64)]                                    # launch_pass1_a mlp_kernels.hip:322
        mixed = 64 * LDH * 4 + 64 * 4                                                            # launch_pass1_mixed :359
        dyn = 64 * LDH * 4 + 64 * 4 + 32 + IDS * 4                                               # omds_launch_pass1 :376, omds_launch_pass1_blocks :404
        emit = [MT * LDH * 4 + MT * 8 + MT * nhid * 32 for MT in (16, 32)]                       # launch_pass1e_t :423
        emit_max = [MT * LDH * 4 + MT * 8 + MT * MAX_NHID * 32 for MT in (16, 32)]               # :427
        exact = 16 * LDH * 4 + 16 * 4 + 16 * 4 + 16 * nhid * 8 * 4                               # omds_launch_exact (screen_plan_def.h:116)
        audit = 64 * LDH * 4 + 64 * 4 + 64 * 4                                                   # omds_launch_audit (screen_plan_def.h:117)
        small = [restate_small_lds(nhid, 16), restate_small_lds(nhid, 32), restate_small_lds(MAX_NHID, 16), restate_small_lds(MAX_NHID, 32)]
        pass2 = [(32 * LDH + 32 * 33) * 4 + n * 512 * 4 + 3 * 32 * 4 for n in (nhid, MAX_NHID)]  # omds_launch_pass2 :467-468
        assert got == dmin + [mixed, dyn] + emit + emit_max + [exact, audit] + small + pass2, nhid
        assert all(v <= 160 * 1024 for v in got), nhid
        assert got[5] <= got[7] and got[6] <= got[8] and got[11] <= got[13] and got[12] <= got[14] and got[15] <= got[16], nhid   # launch <= configured maximum


def test_the_carves_are_the_former_pointer_chains(plan):
    for MT in (16, 32, 64):
        for nhid in NHIDS:
            got = [int(v) for v in plan(4, MT, nhid, 0, 0, 0)]
            # pass1_tile.h:83-86: Hs = smem, rowRad = smem + MT * LDH, rowIdx = rowRad + MT, maskS = rowIdx + MT; [MT][nhid][8] masks
            assert got[:5] == [0, MT * LDH, MT * LDH + MT, MT * LDH + 2 * MT, MT * LDH + 2 * MT + MT * nhid * 8], (MT, nhid)
            assert got[0] < got[1] < got[2] < got[3] < got[4]
            assert got[3] == MT * LDH + 2 * MT                                        # (f) step_small.hip:69: smem + TR * LDH + 2 * TR
            if MT == 16:
                continue
            # pass1_tile_dyn.h:150-153: rowRad = smem + MT * LDH, aliveS = rowRad + MT, idsS = aliveS + 8; :187-188: slotT = rowRad + 4, slotO = slotT + MT / 4
            Hs, rowRad, slotT, slotO, aliveS, idsS, end = got[5:]
            assert (Hs, rowRad, slotT, slotO, aliveS, idsS, end) == (0, MT * LDH, MT * LDH + 4, MT * LDH + 4 + MT // 4, MT * LDH + MT, MT * LDH + MT + 8, MT * LDH + MT + 8 + IDS)
            assert Hs < rowRad < aliveS < idsS < end
            assert rowRad + 4 <= slotT and slotT + MT // 4 <= slotO and slotO + 4 <= aliveS   # four radii, the rollout slots, four obstacle slots: inside rowRad


def test_the_launches_reserve_what_their_modes_touch(plan):
    """the sizes against the carve: a mode that keeps the masks reserves the carve's end, the Dmin launches stop in front of rowIdx"""
    for nhid in NHIDS:
        got = [int(v) for v in plan(3, nhid, 0, 0, 0, 0)]
        for i, MT in enumerate((16, 32, 64)):
            assert got[i] == MT * LDH * 4 + MT * 4                                    # rowRad's end
        assert got[5] == (16 * LDH + 2 * 16 + 16 * nhid * 8) * 4 and got[6] == (32 * LDH + 2 * 32 + 32 * nhid * 8) * 4
        assert got[4] == (64 * LDH + 64 + 8 + IDS) * 4 >= (32 * LDH + 32 + 8 + IDS) * 4   # the 32-row tiles of a compacting launch fit inside


def test_the_emit_limit_lies_below_the_medium_class(plan):
    for t in (1, 4096, 4097, 24575, 24576, 24577, 32767, 32768, 65536, NEAR_2_31):
        ok, size, limit = (int(v) for v in plan(5, t, 0, 0, 0, 0))
        assert limit == 24576                                                         # choose_route, propagate.hip:91
        assert ok == int(t <= 24576) and size == size_class(t), t
        assert not ok or size in (TINY, SMALL), t
    assert size_class(24576) == SMALL and all(size_class(t) in (TINY, SMALL) for t in range(1, 24577, 97))


def test_pass2_carves_the_tails_first_six_blocks(plan):
    for nhid in NHIDS:
        got = [int(v) for v in plan(6, nhid, 0, 0, 0, 0)]
        # k_pass2 mlp_kernels.hip:216-222, in words: gf = Hs + 32 * LDH, maskL = gf + 32 * 33, rowT = maskL + ((nhh + 2) / 2 * 2) * 512 halfwords, rowO, rowMin 32 each
        gf = 32 * LDH
        maskL = gf + 32 * 33
        rowT = maskL + (nhid + 1) // 2 * 2 * 512 // 2
        assert got == [0, gf, maskL, rowT, rowT + 32, rowT + 64, rowT + 96], nhid
        assert got[6] * 4 <= int(plan(3, nhid, 0, 0, 0, 0)[15]), nhid                 # the six blocks end inside the launch's size


def test_the_small_scene_is_the_former_functions(plan):
    for s in SMALL_SCENES:
        r16, r32, rows = (int(v) for v in plan(7, *s, 0))
        e16, e32 = restate_small_rollouts(*s, 16), restate_small_rollouts(*s, 32)
        assert (r16, r32) == (e16, e32), s
        assert rows == (32 if e16 <= 0 else 16 if e16 == e32 else 32), s               # step_small.hip:243-247 small_tile_rows
        if r32 > 0:
            assert r32 * s[2] <= 32 and r32 * s[3] <= SS_RK, s                         # the rollouts' rows fit the tile, their backward rows the group
