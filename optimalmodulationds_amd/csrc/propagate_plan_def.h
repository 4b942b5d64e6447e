// The propagate's SCHEDULE, stated once: the routes of a horizon step (propagate.hip has their table) and whether the full steps of the
// Dense route run as one batch on one stream or as two halves of the batch on two streams (enqueue_dense, propagate.hip).
// propagate.hip enqueues by it; the stand-alone host build of tests/propagate_plan_host.cpp prints it for
// tests/test_propagate_plan_cpu.py.  Plain C++, integer arithmetic only, no HIP header.
#pragma once
#include "omds.h"
#include "pass1_plan_def.h"

enum class StepRoute { Unfused, SmallScene, Dense, Emit, ScreenList, ScreenMatrix };

// OMDS_ORDER_MAX_ROLLOUTS / OMDS_ORDER_MAX_OBS (omds_internal.h; propagate.hip asserts it): the orders are ranked in LDS
constexpr int PIPE_ORDER_MAX_ROLLOUTS = 8192, PIPE_ORDER_MAX_OBS = 4096;
// Full steps (launches over all N x O pairs: every step but the shared first one of a propagate from one state) a propagate needs
// before its halves are run in anti-phase.  What the two-part form pays once per propagate is the drain of the first half-size pass 1
// (the seed: the other half's first pass 1 waits for it) and the last tail of the second half, which nothing covers: together about
// one step's worth of what it can hide (the tail and the ordering launches of a step).  With the flag that forces the
// form the floor is two steps, the fewest at which a launch of one half can lie under a launch of the other at all.
constexpr int PIPE_MIN_FULL_STEPS = 3, PIPE_MIN_FULL_STEPS_FORCED = 2;

struct PipelinePlan {
    int parts;   // 1: every launch on the context's stream; 2: rollouts [0, split) there, [split, N) on the second stream
    int split;   // N when parts == 1
};
// split: N / 2 rounded up to a multiple of 16, so that the 16-rollout blocks of pass 1 and the 4-rollout groups of the tail stay whole
constexpr int omds_pipeline_split(int N) { return ((N + 1) / 2 + 15) & ~15; }
// the compacting block-ordered kernel (k_pass1_dyn_blk) serves a launch of N x O pairs by itself: omds_pass1_blocks_ok without the
// network's part of it
constexpr bool pipeline_blocks_shape_ok(int N, int O) {
    return N >= 1 && O >= 1 && N <= PIPE_ORDER_MAX_ROLLOUTS && O <= PIPE_ORDER_MAX_OBS && pass1_size((long long)N * O) != Pass1Size::Tiny;
}
// N rollouts x O obstacles over H steps; shared: step 1 is the shared first step (one row of pass 1 for all rollouts), which stays a
// whole-batch launch; blocks_ok: the context may run the block-ordered kernel at all (a compacting network, OMDS_FLAG_NATURAL_TILES
// not set).  Two parts by default where that kernel serves EACH part by the rule of the serial step -- its size class, and
// OMDS_BLOCK_TILES_MIN_PAIRS pairs per part -- and PIPE_MIN_FULL_STEPS full steps exist.  OMDS_FLAG_BLOCK_TILES does not lower the pair
// floor here as it does for the order itself: a context that sets it runs small batches, and its one order over the whole batch is
// what the order hooks of include/omds_test_tiles.h report.  OMDS_FLAG_PIPELINED_PROPAGATE waives both the size class and the
// pair floor (the block-ordered kernel computes every size on its 32-row tiles).
constexpr PipelinePlan omds_pipeline_plan(int N, int O, int H, bool shared, StepRoute route, unsigned flags, bool blocks_ok) {
    const PipelinePlan serial{1, N};
    if (route != StepRoute::Dense || !blocks_ok || (flags & OMDS_FLAG_SERIAL_PROPAGATE)) return serial;
    if (N < 2 || O < 1 || N > PIPE_ORDER_MAX_ROLLOUTS || O > PIPE_ORDER_MAX_OBS) return serial;
    const int split = omds_pipeline_split(N), full = H - (shared ? 1 : 0);
    if (split >= N) return serial;   // the second part would be empty
    if (flags & OMDS_FLAG_PIPELINED_PROPAGATE) return full >= PIPE_MIN_FULL_STEPS_FORCED ? PipelinePlan{2, split} : serial;
    const int rest = N - split;      // the smaller part
    if (full < PIPE_MIN_FULL_STEPS || !pipeline_blocks_shape_ok(rest, O) || (long long)rest * O < OMDS_BLOCK_TILES_MIN_PAIRS) return serial;
    return {2, split};
}
