// Pass 1's LAUNCH PLAN, stated once: the size class of a launch, the grid of each launch form and which rows a workgroup owns, the LDS
// blocks pass1_tile and pass1_tile_dyn carve, the LDS size of every launch that runs them, the pair limit of the emitting launch, and
// the small scene's tile choice.  pass1_tile.h, pass1_tile_dyn.h, mlp_kernels.hip, screen_exact.hip and step_small.hip carve and launch
// by it and their kernels call the same rules; the stand-alone host build of tests/pass1_plan_host.cpp prints it for
// tests/test_pass1_plan_cpu.py.  Plain C++, integer arithmetic only, no HIP header (a constexpr function is host-and-device under hipcc).
#pragma once
#include <cstddef>

#include "omds.h"

// LDH (mfma_gemm.h), OMDS_WIDTH, OMDS_MAX_HIDDEN + 1 (omds_internal.h), OMDS_IDS (pass1_tile_dyn.h): asserted by the files that launch by this
constexpr int P1_LDH = 260, P1_WIDTH = 256, P1_MAX_NHID = 9, P1_IDS = P1_WIDTH + 64;

// ---- size classes -----------------------------------------------------------------------------------------------------------------
// Size class of a pass-1 launch over B*O rows: one rule for the dense, the compacted and the emitting launch.  Measured on
// MI355X (profiles/): 64-row tiles (8 waves, each 64 rows x 32 columns, 2 workgroups per CU) beat 128-row tiles at N*O = 301k
// rows (129 vs 123 TFLOP/s: shorter tail) and tie at 1.2M rows (134 TFLOP/s); once there are enough tiles to fill 256 CUs,
// ending the launch on one round of 32-row tiles shortens the drain (135 vs 133 TFLOP/s).  Tiny batches (<= 128 32-row tiles:
// integrator tick, planar toy shapes): 16-row tiles on the 16x16x4 MFMA halve the chain of dependent GEMMs that is the whole
// latency of such a launch.
enum class Pass1Size { Tiny, Small, Medium, Large };
constexpr Pass1Size pass1_size(long long total) {
    if (total >= 64LL * 1024) return Pass1Size::Large;   // 64-row tiles, the last round in 32-row tiles
    if (total >= 64LL * 512) return Pass1Size::Medium;   // 64-row tiles
    if (total > 32LL * 128) return Pass1Size::Small;     // 32-row tiles
    return Pass1Size::Tiny;                              // 16-row tiles
}
// 64-row tiles of a Large launch: the rows of its last 256 64-row tiles (one round of 512 workgroups) go to 32-row tiles
constexpr long long pass1_big_tiles(long long total) { return total / 64 > 256 ? total / 64 - 256 : 0; }

// ---- the natural-order grid -------------------------------------------------------------------------------------------------------
// A launch over the rows [0, total) of the rollout-major pair space: n_big tiles of big_rows rows, then n_small tiles of small_rows
// rows, in workgroup order.  Dense (k_pass1<MT>, k_pass1_mixed): one height per class, Large ending on 32-row tiles.  Compacting
// (m.compact; k_pass1_dyn has 64- and 32-row tiles only): Tiny is the dense 16-row launch, Small is all 32-row tiles, and Medium -- the
// one class where the two differ -- takes floor(total / 64) 64-row tiles and covers the rest with up to two 32-row tiles where the
// dense launch rounds up to one more 64-row tile.
struct Pass1Grid {
    int big_rows, small_rows;
    long long n_big, n_small;
    constexpr long long workgroups() const { return n_big + n_small; }
};
constexpr Pass1Grid pass1_grid(long long total, bool compact) {
    const Pass1Size size = pass1_size(total);
    if (size == Pass1Size::Tiny) return {16, 16, (total + 15) / 16, 0};
    if (!compact && size == Pass1Size::Small) return {32, 32, (total + 31) / 32, 0};
    if (!compact && size == Pass1Size::Medium) return {64, 64, (total + 63) / 64, 0};
    const long long n_big = size == Pass1Size::Large ? pass1_big_tiles(total) : size == Pass1Size::Medium ? total / 64 : 0;
    return {64, 32, n_big, (total - n_big * 64 + 31) / 32};
}
// The inverse: the tile of workgroup b in a launch of 64-row tiles followed by 32-row tiles (k_pass1_mixed, k_pass1_dyn).  The height
// is a template argument of the tile, so a kernel branches on rows == 64 and calls the rule again for row0 inside either branch: with
// one call in front of the branch the row arithmetic leaves the branches and the kernels are other instructions (EXPERIMENTS.md R31).
struct Pass1Tile {
    int rows;
    long long row0;
};
constexpr Pass1Tile pass1_mixed_tile(int b, int n_big) {
    return b < n_big ? Pass1Tile{64, (long long)b * 64} : Pass1Tile{32, (long long)n_big * 64 + (long long)(b - n_big) * 32};
}

// ---- the block grid ---------------------------------------------------------------------------------------------------------------
// The block-ordered form of the compacting launch (k_pass1_dyn_blk; tile_order.hip): the same size classes, counted in blocks of
// 4 obstacles (ncb of them per rollout block).  The first nrb16 * 16 entries of the rollout order go to 16-rollout blocks (64-row
// tiles), the rest to 8-rollout blocks (32-row tiles).  A Large launch ends on 8 x 4 blocks over its last ceil(256 / ncb) * 16
// rollouts, about the one round of 512 workgroups of the natural launch.
struct Pass1BlockGrid {
    int ncb, nrb16;
    long long n_big, n_small;
    constexpr long long workgroups() const { return n_big + n_small; }
};
constexpr Pass1BlockGrid pass1_block_grid(int N, int O) {
    const Pass1Size size = pass1_size((long long)N * O);
    const int ncb = (O + 3) / 4;
    const int last = (256 + ncb - 1) / ncb;
    const int nrb16 = size == Pass1Size::Large ? (N / 16 > last ? N / 16 - last : 0) : size == Pass1Size::Medium ? N / 16 : 0;
    return {ncb, nrb16, (long long)nrb16 * ncb, (long long)((N - nrb16 * 16 + 7) / 8) * ncb};
}
// Workgroup wg of that launch: block (b / ncb, b % ncb) of its part of the grid (b = wg, or wg - n_big behind the big blocks), rollout
// slots r0 .. r0 + nr - 1 and obstacle slots o0 .. o0 + no - 1 of the two orders.  div_ncb(b) = b / ncb: the kernel divides by
// multiplication (OmdsDivisor), the host program by division.
struct Pass1Block {
    bool big;         // 16 rollouts (a 64-row tile), or 8 (a 32-row tile)
    int r0, o0, nr, no;
};
template <class Div>
constexpr Pass1Block pass1_block(unsigned wg, int n_big, int nrb16, unsigned ncb, int N, int O, Div&& div_ncb) {
    if ((int)wg < n_big) {
        const unsigned b = wg, rbk = div_ncb(b), cbk = b - rbk * ncb;
        const int r0 = (int)rbk * 16, o0 = (int)cbk * 4;
        return {true, r0, o0, N - r0 < 16 ? N - r0 : 16, O - o0 < 4 ? O - o0 : 4};
    }
    const unsigned b = wg - (unsigned)n_big, rbk = div_ncb(b), cbk = b - rbk * ncb;
    const int r0 = nrb16 * 16 + (int)rbk * 8, o0 = (int)cbk * 4;
    return {false, r0, o0, N - r0 < 8 ? N - r0 : 8, O - o0 < 4 ? O - o0 : 4};
}

// ---- the emitting launch ----------------------------------------------------------------------------------------------------------
// Pass 1 that also leaves every pair's pass-2 forward (k_pass1e; the Emit route, propagate.hip has the measurements) runs up to this
// many pairs, which lies below the Medium class: the emitting launch exists on 16- and 32-row tiles only.
constexpr long long PASS1_EMIT_MAX_PAIRS = 24576;
constexpr bool pass1_emit_ok(long long total) { return total <= PASS1_EMIT_MAX_PAIRS; }
static_assert(pass1_size(PASS1_EMIT_MAX_PAIRS) < Pass1Size::Medium, "k_pass1e has no 64-row or mixed form");

// ---- the LDS blocks ---------------------------------------------------------------------------------------------------------------
// Where each block starts, in 4-byte words from the start of the dynamic LDS block.
// pass1_tile<MT>; nhid = hidden layers of the network (MlpDev::nhh + 1)
struct Pass1Lds {
    int Hs;       // [MT][LDH] activation tile
    int rowRad;   // [MT] obstacle radius of each row
    int rowIdx;   // [MT] the listed modes: pair index of each row
    int maskS;    // [MT][nhid][8] the modes that keep them: ReLU masks of the tile's rows
    int end;
    constexpr Pass1Lds(int MT, int nhid) : Hs(0), rowRad(Hs + MT * P1_LDH), rowIdx(rowRad + MT), maskS(rowIdx + MT), end(maskS + MT * nhid * 8) {}
};
// pass1_tile_dyn<MT>.  The block-ordered form keeps the radii of its four obstacles in rowRad[0 .. 3] and parks the rollout of every
// slot (slotT [MT / 4]) and the obstacle of every slot (slotO [4]) behind them, inside rowRad.
struct Pass1DynLds {
    int Hs;       // [MT][LDH]
    int rowRad;   // [MT]
    int slotT;    // inside rowRad
    int slotO;
    int aliveS;   // [8] which of a wave's 32 units fired in this tile at the current level
    int idsS;     // [OMDS_IDS] position -> unit * 1024 of the current level
    int end;
    constexpr Pass1DynLds(int MT)
        : Hs(0), rowRad(Hs + MT * P1_LDH), slotT(rowRad + 4), slotO(slotT + MT / 4), aliveS(rowRad + MT), idsS(aliveS + 8), end(idsS + P1_IDS) {}
};
static_assert(Pass1DynLds(32).slotO + 4 <= Pass1DynLds(32).aliveS && Pass1DynLds(64).slotO + 4 <= Pass1DynLds(64).aliveS,
              "the slot arrays of a block-ordered tile fit in rowRad");

// The LDS size of each launch.  A launch reserves the blocks its mode touches, which can be less than the carve's end: the Dmin
// launches (k_pass1<MT>, k_pass1_mixed) write neither rowIdx nor maskS and reserve up to rowIdx only, although pass1_tile forms both
// pointers; k_audit lists its rows and keeps no masks.  The size of a launch is part of how many workgroups a CU holds, so each stays
// the number it was.
constexpr size_t pass1_dmin_lds_bytes(int MT) { return (size_t)Pass1Lds(MT, 0).rowIdx * 4; }
constexpr size_t pass1_mixed_lds_bytes() { return pass1_dmin_lds_bytes(64); }               // its 32-row tiles fit inside
constexpr size_t pass1_dyn_lds_bytes() { return (size_t)Pass1DynLds(64).end * 4; }           // natural and block order alike
constexpr size_t pass1_emit_lds_bytes(int MT, int nhid) { return (size_t)Pass1Lds(MT, nhid).end * 4; }
constexpr size_t pass1_emit_lds_max_bytes(int MT) { return pass1_emit_lds_bytes(MT, P1_MAX_NHID); }   // what k_pass1e<MT> is configured for
// k_exact: 16-row tiles, every mode sized for the masks; k_audit: its 64-row tiles (the 32-row ones fit inside), no masks
constexpr size_t exact_lds_bytes(int nhh) { return (size_t)Pass1Lds(16, nhh + 1).end * 4; }
constexpr size_t audit_lds_bytes() { return (size_t)Pass1Lds(64, 0).maskS * 4; }

// ---- the small scene (k_step_small, step_small.hip) -------------------------------------------------------------------------------
constexpr int SS_RK = 4;      // backward rows per workgroup (R * k)
// Its block: pass1_tile's carve of TR rows with the masks, then its own arrays from Pass1Lds::end on (D1, Dr, Amin [32] each; selRow,
// selT, selO, dr [SS_RK] each; gx [SS_RK][12]; gf [16][33]; feat [SS_RK][3 OMDS_MAX_DOF]).  The last term: gemm4's A-operand reads
// span 32 tile rows (lanes 16-31 are never selected, but they read): a 16-row tile buffer is followed by at least another 16 rows'
// worth of allocation.
constexpr size_t small_lds_bytes(int nhid, int TR) {
    return (size_t)Pass1Lds(TR, nhid).end * 4 + (32 * 3 + SS_RK * 3) * 4 + (SS_RK + SS_RK * 12 + 16 * 33 + SS_RK * 3 * OMDS_MAX_DOF + 4) * 4 + 16 +
           (TR == 16 ? (size_t)Pass1Lds(16, 0).rowRad * 4 : 0);   // (rowRad = the words of a 16-row Hs block)
}
// rollouts per workgroup for (O, k) on a tile of `rows` rows, 0 = the scene does not qualify.  plain_relu: a ReLU network without
// skip concatenations.
constexpr int small_rollouts(bool plain_relu, int n_dof, int O, int k, int rows) {
    if (!plain_relu || (n_dof != 7 && n_dof != 2)) return 0;
    if (O < 1 || O > rows || k < 1 || k > SS_RK || k > O) return 0;
    const int r = rows / O < SS_RK / k ? rows / O : SS_RK / k;
    return r > 1 ? r : 1;
}
// Tile height: 16 rows when that costs no rollouts per workgroup (the cap of four backward rows binds, not the tile: half the
// forward's MFMA chain for the same work); else 32.  Halving the rollouts per workgroup to get two 16-row workgroups resident
// per CU (one's backward and modulation under the other's forward) was measured on planar 7-DoF 1024 x 32: 17.0 M against
// 18.9 M rollout-steps/s -- twice the workgroups stream the backward's weights twice.
constexpr int small_tile_rows(bool plain_relu, int n_dof, int O, int k) {
    const int r16 = small_rollouts(plain_relu, n_dof, O, k, 16), r32 = small_rollouts(plain_relu, n_dof, O, k, 32);
    if (r16 <= 0) return 32;
    return r16 == r32 ? 16 : 32;
}
