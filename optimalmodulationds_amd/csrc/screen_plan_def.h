// The screened step's LAUNCH PLAN, stated once: the geometry of k_screen, which pairs each of its workgroups owns, how many result
// tiles and how much LDS a launch gets, and the rounds of the audit kernels (the LDS of the k_exact / k_audit launches: pass1_plan_def.h).
// screen_kernel.hip and screen_exact.hip launch by it and their kernels call the same rules; the stand-alone host build of
// tests/screen_plan_host.cpp prints it for tests/test_screen_plan_cpu.py.  Plain C++, integer arithmetic only, no HIP header (a
// constexpr function is host-and-device under hipcc).
#pragma once
#include <algorithm>
#include <cstddef>

#include "pass1_plan_def.h"

constexpr int SC_WIDTH = 256;   // OMDS_WIDTH (omds_internal.h): asserted by the files that launch by this

// ---- k_screen's geometry ----------------------------------------------------------------------------------------------------------
// SC_WAVES waves per workgroup, each owning one block of 32 pairs; every A fragment (1 KiB of weights) a wave reads from the ring
// feeds one MFMA.  8 waves x 1 block (two waves per SIMD, 241 registers).  The alternative 4 waves x 2 blocks (one wave per SIMD with
// the 512-register budget: half the LDS reads per MFMA) is bit-identical and measured 104 vs 99 us per launch: the LDS port is not the
// limit (tools/ubench/mfma_f16_issue.hip: one fragment read per MFMA sustains 83-87 % of the fp16 MFMA peak at two waves per SIMD,
// 63-65 % at one), a single wave per SIMD hides less.  Rejected; the kernel is written for the one geometry.
constexpr int SC_WAVES = 8;
constexpr int SC_NT = SC_WAVES * 64;
constexpr int SC_ROWS = SC_WAVES * 32;        // pairs per workgroup and tile
constexpr int SC_SLICE = 16384;               // bytes: 16 k-chunks x 1 KiB fragment
constexpr int SC_RING = 4;                    // ring slots of 16 KB (a power of two)
constexpr int SC_DIST = 3;                    // slices in flight ahead of the one being multiplied (<= RING - 1)
constexpr int SC_PW = 16 / SC_WAVES;          // LDS-DMA pieces (1 KiB fragments) per wave and slice
constexpr int SC_MAX_TILES = 20;              // tiles per workgroup whose results fit the LDS next to the ring
constexpr int SEL_WAVES = 8;                  // waves (= rollouts per round) of a selecting workgroup: k_select, k_screen's flush phase
constexpr int EXACT_RESIDENT = 3;             // k_exact's grid: resident workgroups per CU (screen_exact.hip has the measurements)

// the ring and the bias table [nhh + 2][256] of a k_screen workgroup; its result tiles come on top (ScreenLaunchPlan::lds_bytes)
constexpr size_t omds_screen_lds_bytes(int nhh) { return (size_t)SC_RING * SC_SLICE + (size_t)(nhh + 2) * SC_WIDTH * 4; }
// the flush phase can select when a rollout's O screening values fit a workgroup's result buffer
constexpr bool omds_screen_can_select(int O) { return O <= SC_MAX_TILES * SC_ROWS; }

// ---- the chunk rule ---------------------------------------------------------------------------------------------------------------
// Workgroup w owns units_base + (w < units_rem) consecutive UNITS of `unit` pairs (a unit = a 256-pair tile, or -- when the flush
// phase selects -- a whole rollout of O pairs), starting at unit w * units_base + min(w, units_rem): the pairs [p0, p1) of the pair
// space [0, total), the last chunk cut at its end.
struct ScreenChunk {
    long long p0, p1;
    constexpr int pairs() const { return (int)(p1 - p0); }
    constexpr int tiles() const { return (pairs() + SC_ROWS - 1) / SC_ROWS; }   // >= 1: the grid never exceeds the chunks
};
constexpr ScreenChunk screen_chunk(int unit, int units_base, int units_rem, long long total, int w) {
    const long long p0 = ((long long)w * units_base + (w < units_rem ? w : units_rem)) * unit;
    const long long p1e = p0 + (long long)(units_base + (w < units_rem ? 1 : 0)) * unit;
    return {p0, p1e < total ? p1e : total};
}

// ---- the plan of a k_screen launch ------------------------------------------------------------------------------------------------
// Persistent: one workgroup per CU (256 on MI355X; more only when a workgroup's result buffer would overflow its LDS), each with a
// contiguous chunk of the B x O pair space.  ncu: CUs of the device (omds_cu_count()); want_select: the caller passed a sink.
struct ScreenLaunchPlan {
    bool selects;                        // whole rollouts per workgroup: the flush phase selects (no matrix, no k_select)
    int unit, units_base, units_rem;     // the chunk rule's three integers
    long long total;                     // B * O
    int grid;                            // workgroups
    int res_tiles;                       // tiles of the largest chunk = capacity of the result buffer in LDS
    size_t lds_bytes, lds_max_bytes;     // this launch's dynamic LDS, and the size every instantiation is configured for
    constexpr ScreenChunk chunk(int w) const { return screen_chunk(unit, units_base, units_rem, total, w); }
};
inline ScreenLaunchPlan screen_plan(int B, int O, int nhh, int ncu, bool want_select) {
    ScreenLaunchPlan p{};
    p.total = (long long)B * O;
    p.selects = want_select && omds_screen_can_select(O);
    long long gl;
    if (p.selects) {
        const long long Rmax = std::max<long long>(1, (long long)SC_MAX_TILES * SC_ROWS / O);   // rollouts whose values fit the result buffer
        gl = std::max<long long>(std::min<long long>(B, ncu), ((long long)B + Rmax - 1) / Rmax);
        p.unit = O;
        p.units_base = (int)(B / gl);
        p.units_rem = (int)(B % gl);
        p.res_tiles = (int)(((long long)(p.units_base + (p.units_rem ? 1 : 0)) * O + SC_ROWS - 1) / SC_ROWS);
    } else {
        const long long ntiles = (p.total + SC_ROWS - 1) / SC_ROWS;
        gl = std::min<long long>(ntiles, ncu);
        gl = std::max<long long>(gl, (ntiles + SC_MAX_TILES - 1) / SC_MAX_TILES);
        p.res_tiles = (int)((ntiles + gl - 1) / gl);
        p.unit = SC_ROWS;
        p.units_base = (int)(ntiles / gl);
        p.units_rem = (int)(ntiles % gl);
    }
    p.grid = (int)gl;
    p.lds_bytes = omds_screen_lds_bytes(nhh) + (size_t)p.res_tiles * SC_ROWS * 4;
    p.lds_max_bytes = omds_screen_lds_bytes(4) + (size_t)SC_MAX_TILES * SC_ROWS * 4;
    return p;
}

// ---- the audit kernels' rounds ----------------------------------------------------------------------------------------------------
// The list length is only known on the device: a grid of two resident 64-row workgroups per CU strides over it.
constexpr int AUDIT_MAX_GRID = 512;
inline unsigned audit_grid(int cap) { return (unsigned)std::min<long long>(((long long)cap + 63) / 64, AUDIT_MAX_GRID); }
// Whole rounds of 64-row tiles over the grid; a last round that would fill at most half the grid's row slots runs on 32-row tiles,
// half as long (72 k rows on 512 workgroups are 2.2 rounds of 64 rows: 2 + a half instead of 3).  n: list entries, G: workgroups.
struct AuditRounds {
    int full;          // rounds in which every workgroup has a full 64-row tile: workgroup w takes entries (r * G + w) * 64 ..
    int rest0, rest;   // first entry and length of the last round
    bool last64;       // the last round's tile height: 64 rows, or 32
    constexpr int last_rows() const { return last64 ? 64 : 32; }
    constexpr bool in_last(unsigned w) const { return (long long)w * last_rows() < rest; }   // workgroup w has a tile in the last round ...
    constexpr long long last_row0(unsigned w) const { return rest0 + (long long)w * last_rows(); }   // ... starting at this entry
};
constexpr AuditRounds audit_rounds(int n, int G) {
    const int full = n / (64 * G);
    const int rest0 = full * 64 * G, rest = n - rest0;
    return {full, rest0, rest, rest > 32 * G};
}

// ---- the LDS of the k_exact and k_audit launches ----------------------------------------------------------------------------------
// exact_lds_bytes(nhh) and audit_lds_bytes() are sums of the blocks pass1_tile carves: pass1_plan_def.h, beside the carve.
