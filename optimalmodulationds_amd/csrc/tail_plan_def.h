// The fused tails' PLAN, stated once: which tile height a launch of k_tail / k_tail_sel gets, which instantiations of the two kernels
// exist, which of them a launch looks up, and how large their dynamic LDS block is.  tail_kernel.hip launches by it; the stand-alone host
// build of tests/tail_plan_host.cpp prints it for tests/test_tail_plan_cpu.py.  Plain C++, integer arithmetic only, no HIP header.
#pragma once
#include <algorithm>
#include <cstddef>

#include "omds.h"

constexpr int TAIL_MT = 32, TAIL_NT = 512, TAIL_LDH = 260;   // P2_MT, P2_NT (pass2_device.h) and LDH (mfma_gemm.h): tail_kernel.hip asserts it

// ---- the tile height ------------------------------------------------------------------------------------------------------------
// ncu: CUs of the device (omds_cu_count()).  forced: the tile shape (4 | 16 | 32) of the test hook omds_debug_force_tile_rows
// (libomds_hip_test.so, include/omds_test.h), 0 = the launcher's own choice, the only value the release library passes.  Every shape
// computes the same bits, and the tests say so by running them against each other.

// The step in the moving frame (StepArgs::frame) runs on 16- or 32-row tiles: every tile shape computes the same bits, so the 4-row
// groups are a choice of speed that the frame's instantiations do without.
inline int frame_rows(int rows, int k) { return rows != 4 ? rows : (k <= 16 ? 16 : 32); }

// 16-row tiles (bit-identical to 32-row ones, mfma_gemm.h) while their workgroups still fit the CUs two at a time: twice as
// many, half as long, and the second resident fills the first one's top-k / gather / modulation phases
inline int tail_sel_rows(int N, int k, bool g4_ok, int ncu, int forced) {
    if (k > 16) return 32;
    if (forced == 4 && g4_ok && k <= 20) return 4;
    if (forced == 16 || forced == 32) return forced;
    // 4-row groups (20 rows per workgroup) where the busiest CU multiplies less that way: matrix-pipe cycles per layer of the CU
    // with the most workgroups, 5 groups x 2048 (x 1.1: one wave per SIMD issues a 4x4x1 every 9 cycles, not 8) against 8192 per
    // 16-row tile.  N = 1024, k = 5: 256 workgroups, one per CU, against 342 tiles of 16 rows (40.5 -> 35 us); N = 4096: four
    // per CU against six tiles (20.5 -> 20.1 ms per iteration); N = 1500: 375 workgroups would put two on 119 CUs where 500
    // tiles of 16 rows are two per CU and cheaper.  A lone 16-row tile (no CU with two) is the shorter chain anyway.
    const int RW16 = 16 / k;
    if (forced == 0 && g4_ok && k <= 10) {
        const int RW4 = 20 / k;
        const long long wg16 = (N + RW16 - 1) / RW16, wg4 = (N + RW4 - 1) / RW4;
        const long long cost16 = ((wg16 + ncu - 1) / ncu) * 8192, cost4 = ((wg4 + ncu - 1) / ncu) * (5 * 2048 * 11 / 10);
        if (wg16 > ncu && cost4 < cost16) return 4;
    }
    return (N + RW16 - 1) / RW16 <= 512 ? 16 : 32;
}

// 16-row tiles when 32-row tiles would leave most CUs without a workgroup; g4_ok (ReLU network without skip concatenations): 4-row groups, 20 rows per workgroup (k_tail<ND, ACT, 4>), while its workgroups fit the CUs in ONE
// round -- 5 groups x 2048 x 1.1 matrix-pipe cycles per hidden layer against 16 384 per 32-row tile.  N = 1024, k = 5: 256 workgroups,
// one per CU, against 171 tiles of 32 rows (71.6 -> 58.4 us).  Beyond one round the 32-row tile wins: the 4-row-group kernel holds
// the weight ring in 64 registers (134 in all: one workgroup per CU, nothing fills its top-k / modulation phases) and multiplies on
// four of its eight waves -- N = 4096: 233 against 200 us, N = 8192: 460 against 358 (tools/tail_rows_ab.sh).
inline int omds_tail_rows(int N, int k, bool g4_ok, int ncu, int forced) {
    if (k > 16) return 32;
    if (forced == 4 && g4_ok && k <= 20) return 4;
    if (forced == 16 || forced == 32) return forced;
    const int RW32 = 32 / k;
    const long long wg32 = (N + RW32 - 1) / RW32;
    if (wg32 <= 128) return 16;
    if (forced == 0 && g4_ok && k <= 10) {
        const int RW4 = 20 / k;
        const long long wg4 = (N + RW4 - 1) / RW4;
        if (wg4 <= ncu) return 4;
    }
    return 32;
}

// rows of the tanh-derivative scratch the tail may touch (either tile height)
inline int omds_tail_scratch_rows(int N, int k) {
    const int RW32 = TAIL_MT / k;
    int rows = (N + RW32 - 1) / RW32 * 32;
    if (k <= 16) { const int RW16 = 16 / k; rows = std::max(rows, (N + RW16 - 1) / RW16 * 16); }
    return rows;
}

// rollouts per workgroup and workgroups of a launch on tiles of `rows` rows (4: five 4-row groups, 20 network rows)
inline int tail_rollouts_per_wg(int rows, int k) { return (rows == 4 ? 20 : rows) / k; }
inline int tail_workgroups(int N, int rows, int k) { const int RW = tail_rollouts_per_wg(rows, k); return (N + RW - 1) / RW; }

// ---- the instantiations ---------------------------------------------------------------------------------------------------------
// X(n_dof, activation, rows, frame): k_tail<n_dof, activation, rows, frame> and k_tail_sel<n_dof, rows, activation, frame> exist for
// exactly these keys, the same 18 for both kernels (tail_kernel.hip expands the list once per kernel into its launchers).  4-row
// groups work on ReLU masks and outside the moving frame (frame_rows); everything else exists for both n_dof the fused step takes.
#define OMDS_TAIL_KEYS_OF(X, ND)                                                                                                  \
    X(ND, OMDS_ACT_RELU, 4, false) X(ND, OMDS_ACT_RELU, 16, false) X(ND, OMDS_ACT_RELU, 32, false)                                \
    X(ND, OMDS_ACT_TANH, 16, false) X(ND, OMDS_ACT_TANH, 32, false)                                                               \
    X(ND, OMDS_ACT_RELU, 16, true) X(ND, OMDS_ACT_RELU, 32, true) X(ND, OMDS_ACT_TANH, 16, true) X(ND, OMDS_ACT_TANH, 32, true)
#define OMDS_TAIL_KEYS(X) OMDS_TAIL_KEYS_OF(X, 7) OMDS_TAIL_KEYS_OF(X, 2)

struct TailKey {
    int n_dof, act, rows;
    bool frame;
};
#define OMDS_TAIL_KEY_ROW(ND, ACT, ROWS, FRAME) {ND, ACT, ROWS, FRAME},
constexpr TailKey TAIL_KEYS[] = {OMDS_TAIL_KEYS(OMDS_TAIL_KEY_ROW)};
constexpr int TAIL_N_KEYS = sizeof(TAIL_KEYS) / sizeof(TAIL_KEYS[0]);

// index of a key in TAIL_KEYS (= in the launcher arrays of tail_kernel.hip), -1: no such kernel
inline int tail_key_index(const TailKey& key) {
    for (int i = 0; i < TAIL_N_KEYS; ++i)
        if (TAIL_KEYS[i].n_dof == key.n_dof && TAIL_KEYS[i].act == key.act && TAIL_KEYS[i].rows == key.rows && TAIL_KEYS[i].frame == key.frame) return i;
    return -1;
}

// The key a launch looks up.  plain: a network without skip concatenations and with a hidden->hidden layer (MlpDev::skip_mask == 0,
// nhh >= 1), what the 4-row-group forms need beside ReLU.
inline TailKey tail_plan_key(int n_dof, int act, bool plain, bool frame, int N, int k, int ncu, int forced) {   // omds_launch_tail
    int rows = omds_tail_rows(N, k, act == OMDS_ACT_RELU && plain, ncu, forced);
    if (frame) rows = frame_rows(rows, k);
    return {n_dof, act, rows, frame};
}
inline TailKey tail_sel_plan_key(int n_dof, int act, bool plain, bool frame, int N, int k, int ncu, int forced) {   // omds_launch_tail_sel
    // tanh: derivative rows instead of masks, 16- or 32-row tiles (the 4-row-group backward is a ReLU-mask form)
    int rows = tail_sel_rows(N, k, !frame && act == OMDS_ACT_RELU && plain, ncu, forced);
    if (frame) rows = frame_rows(rows, k);
    return {n_dof, act, rows, frame};
}

// ---- the dynamic LDS block of k_tail and k_tail_sel ------------------------------------------------------------------------------
// Where each block starts, in 4-byte words from the start of the dynamic LDS block, and the size of the launch beside it.  nhid = hidden
// layers of the network (MlpDev::nhh + 1); with_sel: k_tail_sel.  The first six blocks are pass 2's (P2Smem, pass2_device.h).
struct TailLdsPlan {
    int Hs;       // [32][LDH] activation / gradient tile
    int gf;       // [32][33] feature gradients
    int maskL;    // [nhid rounded up to even][512] halfwords: ReLU masks, 16 bits per thread and layer
    int rowT;     // [32] rollout, obstacle, arg-min link of each row
    int rowO;
    int rowMin;
    int gx;       // [32][12] input gradients
    int dr;       // [32] pass-2 distances
    int feat;     // [32][3 OMDS_MAX_DOF] q_next, sin, cos of the workgroup's rollouts
    int sel;      // k_tail_sel only: [32] list entry of each backward row (-1: padding)
    int end;
    constexpr TailLdsPlan(int nhid, bool with_sel)
        : Hs(0), gf(Hs + TAIL_MT * TAIL_LDH), maskL(gf + 32 * 33), rowT(maskL + (nhid + 1) / 2 * 2 * TAIL_NT / 2), rowO(rowT + TAIL_MT),
          rowMin(rowO + TAIL_MT), gx(rowMin + TAIL_MT), dr(gx + 32 * 12), feat(dr + 32), sel(feat + 32 * 3 * OMDS_MAX_DOF),
          end(sel + (with_sel ? 32 : 0)) {}
    // The launch's LDS size: the carve's end plus what the mask block is over-counted by.  The launches have always reserved 4 bytes
    // per thread and layer for the masks, the size pass 2's own launch reserves (omds_launch_pass2), where the carve steps over 2
    // (layers rounded up to even): 2048 nhid - 1024 (nhid + nhid % 2) >= 0 bytes more for every nhid >= 1.  The size of a launch is
    // part of how many workgroups a CU holds, so it stays the number it was.
    static constexpr size_t mask_overcount(int nhid) { return (size_t)nhid * TAIL_NT * 4 - (size_t)((nhid + 1) / 2 * 2) * TAIL_NT * 2; }
    static constexpr size_t bytes(int nhid, bool with_sel) { return (size_t)TailLdsPlan(nhid, with_sel).end * 4 + mask_overcount(nhid); }
    // pass 2's own launch (k_pass2, mlp_kernels.hip): the first six blocks, with the same over-count
    static constexpr size_t pass2_bytes(int nhid) { return (size_t)TailLdsPlan(nhid, false).gx * 4 + mask_overcount(nhid); }
};
