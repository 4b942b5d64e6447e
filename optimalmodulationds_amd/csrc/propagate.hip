// The propagate step: which launch sequence a context runs per horizon step (choose_route), the sequences themselves, and
// omds_propagate / omds_get_rollouts / omds_get_rollout_rows.  Nothing of the screening controller lives here: the screened
// routes get their plan from screen_begin_propagate and hand what they measured to screen_finish_propagate (screening.hip).
#include "capi_internal.h"
#ifdef OMDS_TEST_HOOKS
#include "omds_test_tiles.h"
#endif

// The one-launch small-scene step (step_small.hip) when the scene qualifies and the batch is small enough that the
// two-kernel step's tail would sit on a fraction of the CUs (at R rollouts per workgroup; beyond ~3 rounds of workgroups
// k_pass1 + the 16/32-row MFMA tail win back what the extra launch costs).
bool small_step_wanted(omds_ctx* ctx) {
    if (ctx->wide.on || (ctx->cfg.flags & (OMDS_FLAG_UNFUSED_STEP | OMDS_FLAG_TWO_KERNEL_STEP))) return false;
    const int R = omds_step_small_rollouts(ctx->mlp, ctx->cfg.n_dof, ctx->n_obs, ctx->cfg.n_closest);
    if (R <= 0) return false;
    return (ctx->cfg.n_traj + R - 1) / R <= 768;
}

// Emit route: per PAIR what k_exact leaves per candidate (d_allDr / d_allMin / d_allMask), for n_traj * max_obs pairs.  Allocated
// at the first use, grown when the scene or the network asks for more; a request that failed is remembered and not retried at
// every propagate (hipMalloc / hipFree synchronise the device) until it changes.
static bool acquire_emit_buffers(omds_ctx* ctx) {
    const long long pairs = (long long)ctx->cfg.n_traj * ctx->cfg.max_obs;
    const int nhid = ctx->mlp.nhh + 1;
    const bool fits = (long long)ctx->d_allDr.count() >= pairs && ctx->all_nhid >= nhid;
    if (fits || (ctx->all_failed_pairs == pairs && ctx->all_failed_nhid == nhid)) return fits;
    ctx->d_allDr.reset(); ctx->d_allMin.reset(); ctx->d_allMask.reset();
    ctx->all_nhid = 0;
    const size_t mask_bytes = (size_t)pairs * nhid * 32;
    if (mask_bytes <= ((size_t)8 << 30) && ctx->d_allDr.alloc((size_t)pairs) == hipSuccess &&
        ctx->d_allMin.alloc((size_t)pairs) == hipSuccess && ctx->d_allMask.alloc(mask_bytes / 4) == hipSuccess) {
        ctx->all_nhid = nhid;
        return true;
    }
    (void)hipGetLastError();
    ctx->d_allDr.reset(); ctx->d_allMin.reset(); ctx->d_allMask.reset();
    ctx->all_failed_pairs = pairs; ctx->all_failed_nhid = nhid;
    return false;
}

// Screened tanh step: k_exact hands 1 - h^2 of every candidate's hidden units to k_tail_sel (ExactOut::deriv), so the step has
// the ReLU step's shape -- no matrix, no k_select, no second forward in the tail.  The buffer is allocated at the first
// screened tanh step; if that fails (an enormous batch) the step keeps the matrix route.
static bool acquire_deriv_buffer(omds_ctx* ctx) {
    if (ctx->d_exDeriv) return true;
    if (ctx->d_exDeriv.alloc((size_t)(ctx->mlp.nhh + 1) * (size_t)ctx->ex_cap * OMDS_WIDTH) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

// THE ROUTES OF A STEP.  Per horizon step a context runs exactly one of these launch sequences:
//
//   route         kernels per horizon step                                   when
//   ------------  ---------------------------------------------------------  ----------------------------------------------------
//   Unfused       enqueue_network (k_pass1, k_topk, k_pass2 -- or the wide    OMDS_FLAG_UNFUSED_STEP, an (n_dof, n_closest) the tail
//                 network's GEMMs, or k_net_small) + k_modulate              kernels are not built for, a SEDS nominal DS (only
//                                                                            k_modulate carries that branch), a wide network
//   ScreenList    k_screen [+ k_select unless it selects in its flush]       screening requested and usable; ReLU network, or tanh
//                 + k_exact + k_tail_sel                                     with the derivative hand-over buffer (d_exDeriv)
//   ScreenMatrix  k_screen + k_select + k_exact + k_tail                     screening requested and usable; tanh network whose
//                                                                            d_exDeriv could not be allocated
//   SmallScene    k_step_small                                               small_step_wanted: few obstacles, few workgroups
//   Emit          k_pass1 (emitting pass 2's forward of every pair)          ReLU network without skips, no OMDS_FLAG_TAIL_FORWARD,
//                 + k_tail_sel (backward only)                               n_traj * n_obs <= 24 576 pairs, buffers available
//   Dense         k_pass1 + k_tail                                           everything else (step 1 of a propagate from one state:
//                                                                            k_pass1 over ONE rollout's rows, enqueue_dense)
//
// Both screened routes add, per propagate, the sweep of a step when one is due (k_pass1 + k_screen + k_sweep_hist) and k_audit
// behind the loop (screening.hip).  Under an obstacle horizon every route reads slab i - 1 at step i (obstacle_tables); the screened
// routes only run then when the caller switched screening over the horizon on (screen_wanted) and read the slab's fp16 tables too
// (screen_tables), as do the sweep and -- per listed row -- k_audit_slabs.  choose_route acquires the lazily allocated buffers the route it is about to pick needs, and
// picks the next one down when they cannot be had.
//
// Emit: SMALL BATCHES of the all-fp32 step of a ReLU network run without a second forward: k_pass1 in its emitting mode leaves, for
// EVERY pair, what pass 2's forward would compute for it (pass-2 distance, arg-min link, ReLU masks: the two forwards are
// bit-identical), and k_tail_sel selects from the row of Dmin and runs the backward alone.  The chain of a step loses three
// dependent GEMMs: integrator tick (N = 1) 0.66 -> 0.56 ms per 10-step propagate, planner defaults (N = 40) 1.02 -> 0.95.
// Up to 24 576 pairs only (PASS1_EMIT_MAX_PAIRS, pass1_plan_def.h; pass1_emit_ok): the masks cost the pass-1 epilogue 32 ballots + 64 single-lane LDS stores per wave and layer, which
// a throughput-bound launch cannot hide (k_pass1 +18 % at 1024 x 294, the step 29.5 -> 33.3 ms: EXPERIMENTS.md B.5).
bool fused_step_available(const omds_ctx* ctx) {
    return !(ctx->cfg.flags & OMDS_FLAG_UNFUSED_STEP) && omds_tail_supported(ctx->cfg.n_dof, ctx->cfg.n_closest) && ctx->seds_G == 0 && !ctx->wide.on;
}

StepRoute choose_route(omds_ctx* ctx, bool screen_requested) {
    const int n = ctx->cfg.n_dof, k = ctx->cfg.n_closest;
    const bool relu = ctx->mlp.act == OMDS_ACT_RELU;
    if (!fused_step_available(ctx)) return StepRoute::Unfused;
    if (screen_requested) return (relu || acquire_deriv_buffer(ctx)) ? StepRoute::ScreenList : StepRoute::ScreenMatrix;
    if (small_step_wanted(ctx)) return StepRoute::SmallScene;
    if (relu && !(ctx->cfg.flags & OMDS_FLAG_TAIL_FORWARD) && ctx->mlp.skip_mask == 0 && ctx->mlp.nhh >= 1 && omds_tail_sel_supported(n, k) &&
        pass1_emit_ok((long long)ctx->cfg.n_traj * ctx->n_obs) && acquire_emit_buffers(ctx))
        return StepRoute::Emit;
    return StepRoute::Dense;
}

static int enqueue_unfused(omds_ctx* ctx, StepArgs& a) {
    int rc;
    for (int i = 1; i <= a.H; ++i) {   // MPPI.py:101: H network evaluations, the last velocity is not integrated
        if ((rc = enqueue_network(ctx, ctx->d_trajT + (size_t)(i - 1) * a.n * a.N, a.N, a.N, obstacle_tables(ctx, i)))) return rc;
        a.step = i;
        omds_launch_modulate(ctx->stream, a);
    }
    return OMDS_OK;
}

static int enqueue_small_scene(omds_ctx* ctx, StepArgs& a) {
    const int N = a.N;
    int rc;
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_trajT, N, N, ctx->d_Fq, nullptr, N);
    for (int i = 1; i <= a.H; ++i) {
        RoctxRange r1("TAG: evaluate NN_2-5 + Modulation-propagation (fused small-scene step)");
        a.step = i;
        if ((rc = prof_begin(ctx))) return rc;
        const ObsTables t = obstacle_tables(ctx, i);
        omds_launch_step_small(ctx->stream, ctx->mlp, t.Fp, t.radius, t.obs, ctx->d_Fq, ctx->n_obs,
                               ctx->prm.ignored_links, a);
        if ((rc = prof_end(ctx, (int64_t)N * ctx->n_obs, (double)N * ctx->n_obs * ctx->f_fwd + (double)N * a.k * ctx->f_bwd, "k_step_small"))) return rc;
    }
    return OMDS_OK;
}

// The orders of the block-ordered pass 1 (tile_order.hip), allocated at the first launch that uses them and zeroed, so that every
// entry names a row of the tables whatever happens; a request that failed leaves the step on the natural order.
static bool acquire_order_buffers(omds_ctx* ctx) {
    // rperm: one padded order of the batch, or the padded orders of its two parts behind each other (16 entries more)
    const size_t nr = (size_t)omds_order_pad(ctx->cfg.n_traj) + 16, no = (size_t)omds_order_pad(ctx->cfg.max_obs);
    const size_t gr = (size_t)omds_share_groups(ctx->cfg.n_traj), go = (size_t)omds_share_groups(ctx->cfg.max_obs);
    if (ctx->d_tileKeys && ctx->d_rperm.count() >= nr && ctx->d_operm.count() >= no && ctx->d_rkey.count() >= (size_t)ctx->cfg.n_traj &&
        ctx->d_okey.count() >= (size_t)ctx->cfg.max_obs && ctx->d_shareSum.count() >= (go + gr) * OMDS_WIDTH && ctx->d_shareCnt.count() >= gr * OMDS_WIDTH)
        return true;
    if (ctx->d_rperm.alloc(nr) == hipSuccess && ctx->d_operm.alloc(no) == hipSuccess && ctx->d_tileKeys.alloc(1) == hipSuccess &&
        ctx->d_rkey.alloc((size_t)ctx->cfg.n_traj) == hipSuccess && ctx->d_okey.alloc((size_t)ctx->cfg.max_obs) == hipSuccess &&
        ctx->d_shareSum.alloc((go + gr) * OMDS_WIDTH) == hipSuccess && ctx->d_shareCnt.alloc(gr * OMDS_WIDTH) == hipSuccess &&
        hipMemsetAsync(ctx->d_rperm, 0, nr * sizeof(int), ctx->stream) == hipSuccess &&
        hipMemsetAsync(ctx->d_operm, 0, no * sizeof(int), ctx->stream) == hipSuccess &&
        hipMemsetAsync(ctx->d_tileKeys, 0, sizeof(TileKeys), ctx->stream) == hipSuccess &&
        hipMemsetAsync(ctx->d_rkey, 0, ctx->d_rkey.bytes(), ctx->stream) == hipSuccess &&
        hipMemsetAsync(ctx->d_okey, 0, ctx->d_okey.bytes(), ctx->stream) == hipSuccess &&
        hipMemsetAsync(ctx->d_shareSum, 0, ctx->d_shareSum.bytes(), ctx->stream) == hipSuccess &&
        hipMemsetAsync(ctx->d_shareCnt, 0, ctx->d_shareCnt.bytes(), ctx->stream) == hipSuccess)
        return true;
    (void)hipGetLastError();
    ctx->d_rperm.reset(); ctx->d_operm.reset(); ctx->d_tileKeys.reset();
    ctx->d_rkey.reset(); ctx->d_okey.reset(); ctx->d_shareSum.reset(); ctx->d_shareCnt.reset();
    return false;
}

// The second stream and the events of the two-part propagate, at its first use on the context
static bool acquire_second_stream(omds_ctx* ctx) {
    if (ctx->stream2) return true;
    hipStream_t s2 = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    bool ok = hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < 3; ++i) ok = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {   // the propagate stays on one stream
        (void)hipGetLastError();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (s2) (void)hipStreamDestroy(s2);
        return false;
    }
    ctx->stream2 = s2;
    ctx->ev_fork = ev[0]; ctx->ev_seed = ev[1]; ctx->ev_join = ev[2];
    return true;
}

static_assert(PIPE_ORDER_MAX_ROLLOUTS == OMDS_ORDER_MAX_ROLLOUTS && PIPE_ORDER_MAX_OBS == OMDS_ORDER_MAX_OBS, "propagate_plan_def.h restates the order limits");

// Two launches per step: k_pass1 over all (rollout, obstacle) pairs, then the rollout-local tail.
// Rollouts do not depend on each other, so parts of the batch may run on streams of their own.  Three forms, two of them measured
// and rejected:
// (1) independent rollout groups on separate HIP streams for small batches -- planar7_1024x32 ran 9.0 M rollout-steps/s on one
//     stream, 7.1 / 3.3 / 2.4 M on 2 / 4 / 8;
// (2) a two-half ping-pong for large batches with EVENT-CHAINED pass-1 launches, so that one half's tail runs under the other half's
//     pass 1: parity-green, but the half-size launches drain twice per step, 1.00 M vs 1.03 M;
// (3) TWO HALVES IN ANTI-PHASE (enqueue_dense_halves; the plan: propagate_plan_def.h): the halves' pass-1 launches are free to overlap
//     each other, so nothing drains, and the phase is seeded ONCE -- the second half's first pass 1 waits for the first half's, and
//     from then on one half's tail and ordering launches lie under the other half's pass 1.  No event passes between the halves
//     after the seed until they are joined.  EXPERIMENTS.md R35 has what it measured.
// The full steps of the batch as the rollouts [0, split) on the context's stream and [split, N) on its second stream.
static int enqueue_dense_halves(omds_ctx* ctx, StepArgs& a, int split, bool shared) {
    const int N = a.N, O = ctx->n_obs;
    int rc;
    const hipStream_t str[2] = {ctx->stream, ctx->stream2};
    const int first[2] = {0, split}, count[2] = {split, N - split};
    int* const rperm[2] = {ctx->d_rperm, ctx->d_rperm + omds_order_pad(split)};   // each part ranks into its own padded order
    float* const sumO = ctx->d_shareSum;
    const TileOrderBufs ob{ctx->d_tileKeys, ctx->d_rperm, ctx->d_operm, ctx->d_rkey, ctx->d_okey, sumO,
                           sumO + (size_t)omds_share_groups(ctx->cfg.max_obs) * OMDS_WIDTH, ctx->d_shareCnt};
    bool picked = false, forked = false;
    // the second stream's work becomes part of the context's stream again: everything behind this on ctx->stream sees both halves
    auto join = [&]() -> int {
        if (!forked) return OMDS_OK;
        CK(hipEventRecord(ctx->ev_join, ctx->stream2));
        CK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        forked = false;
        return OMDS_OK;
    };
    for (int i = 1; i <= a.H; ++i) {
        const bool one_row = shared && i == 1;
        const ObsTables t = obstacle_tables(ctx, i);
        a.step = i;
        // THE WHOLE BATCH ON ONE STREAM: the shared first step, and every step whose pass 1 the profiling bracket encloses -- the
        // bracket times ONE launch that has the device to itself (omds_prof_read's rate is per launch), so the halves are joined in front
        // of it and forked and seeded again behind it.  Launches and rows are counted as the serial propagate counts them.
        if (one_row || prof_due(ctx)) {
            if ((rc = join())) return rc;
            {
                RoctxRange r1("TAG: evaluate NN_2 (forward pass)");
                if ((rc = prof_begin(ctx))) return rc;
                if (one_row) {
                    omds_launch_pass1(ctx->stream, ctx->mlp, ctx->d_Fq, t.Fp, t.radius, O, 1, ctx->prm.ignored_links, ctx->d_Dmin);
                } else {
                    omds_launch_tile_order(ctx->stream, ctx->mlp, ctx->d_Fq, N, obstacle_tables(ctx, 1).Fp, O, ob, !picked);
                    picked = true;
                    omds_launch_pass1_blocks(ctx->stream, ctx->mlp, ctx->d_Fq, t.Fp, t.radius, O, N, ctx->prm.ignored_links, ctx->d_Dmin,
                                             ctx->d_rperm, ctx->d_operm);
                }
                if ((rc = prof_end(ctx, (int64_t)(one_row ? 1 : N) * O))) return rc;
            }
            RoctxRange r2("TAG: evaluate NN_3-5 + Modulation-propagation");
            omds_launch_tail(ctx->stream, ctx->mlp, t.Fp, t.radius, t.obs, ctx->d_Dmin, ctx->d_Fq, ctx->d_dscr, O, a, TailScreen{}, one_row);
            continue;
        }
        prof_pass(ctx);
        // the key units and the obstacles' order are the whole batch's, picked where the serial propagate picks them
        if (!picked) omds_launch_tile_pick(ctx->stream, ctx->mlp, ctx->d_Fq, N, obstacle_tables(ctx, 1).Fp, O, ob);
        picked = true;
        const bool seed = !forked;
        if (seed) {
            CK(hipEventRecord(ctx->ev_fork, ctx->stream));
            CK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
            forked = true;
        }
        RoctxRange r1("TAG: evaluate NN_2-5 + Modulation-propagation (two halves)");
        for (int p = 0; p < 2; ++p) {
            omds_launch_rollout_order(str[p], ctx->d_tileKeys, ctx->d_Fq, first[p], count[p], ctx->d_rkey, rperm[p]);
            // THE SEED: the second half's first pass 1 starts behind the first half's, under its tail
            if (seed && p == 1) CK(hipStreamWaitEvent(ctx->stream2, ctx->ev_seed, 0));
            omds_launch_pass1_blocks(str[p], ctx->mlp, ctx->d_Fq, t.Fp, t.radius, O, count[p], ctx->prm.ignored_links, ctx->d_Dmin, rperm[p],
                                     ctx->d_operm, first[p]);
            if (seed && p == 0) CK(hipEventRecord(ctx->ev_seed, ctx->stream));
            omds_launch_tail(str[p], ctx->mlp, t.Fp, t.radius, t.obs, ctx->d_Dmin, ctx->d_Fq, ctx->d_dscr, O, a, TailScreen{}, false, first[p],
                             count[p]);
        }
    }
    return join();
}

static int enqueue_dense(omds_ctx* ctx, StepArgs& a) {
    const int N = a.N;
    int rc;
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_trajT, N, N, ctx->d_Fq, nullptr, N);
    // SHARED FIRST STEP: a propagate from one state (per_rollout == 0, what every planner iteration does) holds N copies of that
    // state at step 1, so its N x O pairs are N copies of O rows.  Pass 1 evaluates rollout 0's O rows once and every rollout's
    // tail selects from that row of Dmin (row stride 0).  A row's chain never depends on its tile-mates and every tile shape
    // computes the same bits, so the step's results are those of the full launch (OMDS_FLAG_NATURAL_PASS1 keeps that one).
    const bool shared = ctx->shared_start && !(ctx->cfg.flags & OMDS_FLAG_NATURAL_PASS1);
    // BLOCK-ORDERED TILES: every full launch of the compacting kernel forms its tiles from 16 (8) rollouts x 4 obstacles that are
    // neighbours in a key order of the rollouts (formed again at every step: k_order_keys + k_order_rank) and of the obstacles (formed
    // with the key units at the first full launch of the propagate, k_share_stats x 2 + k_tile_pick, on slab 0 of an obstacle horizon): rows that fire alike
    // share a tile, and the exact zero-skip multiplies fewer chunks.  A row's bits do not depend on its tile-mates
    // (OMDS_FLAG_NATURAL_TILES keeps the rows in their order).  The ordering launches sit INSIDE the profiling bracket of pass 1:
    // they are part of what the launch costs.
    // Below OMDS_BLOCK_TILES_MIN_PAIRS the natural order stays: at 128 / 256 / 384 rollouts x 294 obstacles the block order ran 6.8 / 2.0 /
    // 1.8 % slower (the ordering launches in front of a short pass 1 that does not fill the device twice over), at 512 / 768 / 1024
    // rollouts 0.9 / 3.3 / 3.9 % faster (EXPERIMENTS.md R15).
    const bool blocks = !(ctx->cfg.flags & OMDS_FLAG_NATURAL_TILES) && omds_pass1_blocks_ok(ctx->mlp, N, ctx->n_obs) &&
                        ((ctx->cfg.flags & OMDS_FLAG_BLOCK_TILES) || (long long)N * ctx->n_obs >= OMDS_BLOCK_TILES_MIN_PAIRS) && acquire_order_buffers(ctx);
    // THE SCHEDULE (propagate_plan_def.h): the full steps as two halves of the batch in anti-phase on two streams, or all on one
    const bool blocks_may = ctx->mlp.compact && !(ctx->cfg.flags & OMDS_FLAG_NATURAL_TILES);
    const PipelinePlan plan = omds_pipeline_plan(N, ctx->n_obs, a.H, shared, StepRoute::Dense, (unsigned)ctx->cfg.flags, blocks_may);
    if (plan.parts == 2 && acquire_order_buffers(ctx) && acquire_second_stream(ctx)) {
        ctx->pipe_parts = 2;
        ctx->pipe_split = plan.split;
        return enqueue_dense_halves(ctx, a, plan.split, shared);
    }
    bool picked = false;
    for (int i = 1; i <= a.H; ++i) {
        const bool one_row = shared && i == 1;
        const int B = one_row ? 1 : N;
        const ObsTables t = obstacle_tables(ctx, i);   // slab i - 1 of an obstacle horizon; slab 0 is one scene for all rollouts
        {
            RoctxRange r1("TAG: evaluate NN_2 (forward pass)");
            if ((rc = prof_begin(ctx))) return rc;
            if (blocks && !one_row) {
                float* const sumO = ctx->d_shareSum;
                const TileOrderBufs ob{ctx->d_tileKeys, ctx->d_rperm, ctx->d_operm, ctx->d_rkey, ctx->d_okey, sumO,
                                       sumO + (size_t)omds_share_groups(ctx->cfg.max_obs) * OMDS_WIDTH, ctx->d_shareCnt};
                omds_launch_tile_order(ctx->stream, ctx->mlp, ctx->d_Fq, N, obstacle_tables(ctx, 1).Fp, ctx->n_obs, ob, !picked);
                picked = true;
                omds_launch_pass1_blocks(ctx->stream, ctx->mlp, ctx->d_Fq, t.Fp, t.radius, ctx->n_obs, N, ctx->prm.ignored_links,
                                         ctx->d_Dmin, ctx->d_rperm, ctx->d_operm);
            } else {
                omds_launch_pass1(ctx->stream, ctx->mlp, ctx->d_Fq, t.Fp, t.radius, ctx->n_obs, B,
                                  ctx->prm.ignored_links, ctx->d_Dmin);
            }
            if ((rc = prof_end(ctx, (int64_t)B * ctx->n_obs))) return rc;
        }
        RoctxRange r2("TAG: evaluate NN_3-5 + Modulation-propagation");
        a.step = i;
        omds_launch_tail(ctx->stream, ctx->mlp, t.Fp, t.radius, t.obs, ctx->d_Dmin, ctx->d_Fq,
                         ctx->d_dscr, ctx->n_obs, a, TailScreen{}, one_row);
    }
    return OMDS_OK;
}

// Pass 1 leaves pass 2's forward of every pair (pass1_tile, TileMode::EmitAll); the tail runs the top-k over the rollout's row of Dmin, takes
// the masks of the k selected pairs and runs the backward, blend, modulation and Euler step.
static int enqueue_emit(omds_ctx* ctx, StepArgs& a) {
    const int N = a.N;
    int rc;
    const ExactOut ex_all{ctx->d_Dmin, ctx->d_allDr, ctx->d_allMin, ctx->d_allMask, (int)std::min<long long>((long long)N * ctx->n_obs, 0x7fffffffLL)};
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_trajT, N, N, ctx->d_Fq, nullptr, N);
    for (int i = 1; i <= a.H; ++i) {
        const ObsTables t = obstacle_tables(ctx, i);
        {
            RoctxRange r1("TAG: evaluate NN_2 (forward pass)");
            if ((rc = prof_begin(ctx))) return rc;
            omds_launch_pass1_emit(ctx->stream, ctx->mlp, ctx->d_Fq, t.Fp, t.radius, ctx->n_obs, N,
                                   ctx->prm.ignored_links, ctx->d_Dmin, ex_all);
            if ((rc = prof_end(ctx, (int64_t)N * ctx->n_obs))) return rc;
        }
        RoctxRange r2("TAG: evaluate NN_3-5 + Modulation-propagation");
        a.step = i;
        // every pair is an entry of ex_all: no list, no window, no slack to count
        omds_launch_tail_sel(ctx->stream, ctx->mlp, t.Fp, t.radius, t.obs, ctx->d_Fq, ctx->n_obs, a, ex_all, TailScreen{});
    }
    return OMDS_OK;
}

// k_pass1 becomes k_screen (fp16) + the selection + k_exact (fp32 on the candidates only).  list_tail (ScreenList): k_exact leaves
// what pass 2's forward would produce per list entry and k_tail_sel runs the backward only; otherwise (ScreenMatrix) k_exact
// patches the matrix and k_tail runs as in the dense step, guarded by the selection's tau.
static int enqueue_screened(omds_ctx* ctx, StepArgs& a, bool list_tail) {
    const int N = a.N, H = a.H;
    int rc;
    ScreenPlan p;
    if ((rc = screen_begin_propagate(ctx, a, list_tail, &p))) return rc;
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_trajT, N, N, p.fq0, ctx->d_FqH, N);
    for (int i = 1; i <= H; ++i) {
        float* fq_i = p.fq0 + (size_t)(i - 1) * p.fq_slab;
        float* fq_next = p.fq0 + (size_t)std::min(i, H - 1) * p.fq_slab;
        // slab i - 1 of an obstacle horizon, fp32 and fp16 (screening over the horizon, omds_set_screening_horizon); else the static scene.
        // The rows of the candidate list name the caller's obstacle index in either case (the moving frame's d_hzVel is indexed by it)
        const ObsTables t = obstacle_tables(ctx, i);
        const ScreenTables st = screen_tables(ctx, i);
        {
            RoctxRange r1("TAG: evaluate NN_2 (forward pass)");
            if ((rc = prof_begin(ctx))) return rc;
            omds_launch_screen(ctx->stream, ctx->screen, st.m, ctx->d_FqH, ctx->cfg.n_traj, st.FpH, st.ld, st.radius, ctx->n_obs, N,
                               ctx->prm.ignored_links, ctx->d_Dmin, p.fuse_select ? p.d_sinks + (i - 1) : nullptr);
            if ((rc = prof_end(ctx, (int64_t)N * ctx->n_obs, -1.0, "k_screen"))) return rc;
            if (!p.fuse_select) omds_launch_select(ctx->stream, ctx->d_Dmin, N, ctx->n_obs, p.h_sinks[i - 1]);
            omds_launch_exact(ctx->stream, ctx->mlp, fq_i, t.Fp, t.radius, ctx->n_obs, N,
                              ctx->prm.ignored_links, ctx->d_Dmin, ctx->d_rowlist, p.h_sinks[i - 1].total, ctx->d_scerr, p.ex);
        }
        enqueue_sweep_of_step(ctx, fq_i, N, i);
        RoctxRange r2("TAG: evaluate NN_3-5 + Modulation-propagation");
        a.step = i;
        TailScreen scr;
        scr.FqH = ctx->d_FqH; scr.ldF = N;
        scr.range = ctx->d_range; scr.e_bound = p.eps; scr.viol = ctx->d_scerr + 1;
        if (list_tail) {
            scr.rowlist = ctx->d_rowlist;
            omds_launch_tail_sel(ctx->stream, ctx->mlp, t.Fp, t.radius, t.obs, fq_next, ctx->n_obs, a, p.ex, scr);
        } else {
            scr.FqOut = fq_next;
            omds_launch_tail(ctx->stream, ctx->mlp, t.Fp, t.radius, t.obs, ctx->d_Dmin, fq_i, ctx->d_dscr, ctx->n_obs, a, scr, false);
        }
    }
    return screen_finish_propagate(ctx, p);
}

int enqueue_rollouts(omds_ctx* ctx, StepArgs& a, StepRoute route) {
    switch (route) {
        case StepRoute::Unfused: return enqueue_unfused(ctx, a);
        case StepRoute::SmallScene: return enqueue_small_scene(ctx, a);
        case StepRoute::Dense: return enqueue_dense(ctx, a);
        case StepRoute::Emit: return enqueue_emit(ctx, a);
        case StepRoute::ScreenList: return enqueue_screened(ctx, a, true);
        case StepRoute::ScreenMatrix: return enqueue_screened(ctx, a, false);
    }
    return OMDS_ERR_INVALID_ARG;
}

extern "C" {

int omds_propagate(omds_ctx* ctx, const float* q_cur, int per_rollout) {
    RoctxRange range("TAG: general propagation");
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(q_cur, OMDS_ERR_INVALID_ARG, "omds_propagate: null q_cur");
    int rc;
    if ((rc = check_ready(ctx, true))) return rc;
    REQUIRE(!(ctx->hz_mode && ctx->wide.on), OMDS_ERR_UNSUPPORTED,
            "omds_propagate: an obstacle horizon is not supported on networks wider than 256 (clear it: omds_set_obstacle_motion(ctx, NULL))");
    REQUIRE(!(ctx->frame_on && ctx->hz_mode == 2), OMDS_ERR_UNSUPPORTED,
            "omds_propagate: the moving frame needs the obstacles' velocities, and an explicit horizon table carries none (set them with "
            "omds_set_obstacle_motion, or switch the frame off: omds_set_obstacle_frame(ctx, 0, 0))");
    CK(hipSetDevice(ctx->dev));
    if ((rc = prepare_obstacle_horizon(ctx))) return rc;
    const int N = ctx->cfg.n_traj, H = ctx->cfg.horizon, n = ctx->cfg.n_dof;
    ctx->shared_start = per_rollout == 0;
    ctx->pipe_parts = 1;
    ctx->pipe_split = N;
    // all_traj[:, 0, :] = q_cur  (MPPI.py:99)
    if (per_rollout) {
        CK(hipMemcpyAsync(ctx->d_stage, q_cur, (size_t)N * n * 4, hipMemcpyHostToDevice, ctx->stream));
        omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_trajT, N, n);
        CK(hipStreamSynchronize(ctx->stream));  // q_cur is caller memory
    } else {
        // pinned staging + a device slot of its own (d_qcur): no synchronisation, and the policy means that k_sample may not
        // have consumed yet (d_means) stay untouched
        CK(hipEventSynchronize(ctx->ev_in_q));
        std::memcpy(ctx->h_in, q_cur, (size_t)n * 4);
        CK(hipMemcpyAsync(ctx->d_qcur, ctx->h_in, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        CK(hipEventRecord(ctx->ev_in_q, ctx->stream));
        omds_launch_broadcast_q(ctx->stream, ctx->d_qcur, n, N, ctx->d_trajT);
    }
    StepArgs a{};
    a.N = N; a.H = H; a.n = n; a.K = ctx->n_kernels; a.Kmax = ctx->cfg.n_kernel_max; a.k = ctx->cfg.n_closest; a.d = ctx->mlp.d;
    a.trajT = ctx->d_trajT; a.distT = ctx->d_distT; a.dotT = ctx->d_dotT; a.actT = ctx->d_actT; a.normalT = ctx->d_normalT;
    a.kvalT = ctx->d_kvalT; a.qdotT = ctx->d_qdotT; a.maxact = ctx->d_maxact; a.phisum0 = ctx->d_phisum0;
    a.muT = ctx->d_muT; a.sigmaT = ctx->d_sigmaT; a.alphaT = ctx->d_alphaT; a.gradx = ctx->d_gradx; a.drow = ctx->d_drow;
    std::memcpy(a.qf, ctx->qf, sizeof(a.qf));
    a.A = ctx->have_A ? ctx->d_A.get() : nullptr;
    a.seds = ctx->seds_G > 0 ? ctx->d_seds.get() : nullptr;
    a.seds_G = ctx->seds_G; a.seds_lin_thr = ctx->seds_lin_thr; a.seds_thr = ctx->seds_thr;
    a.prm = ctx->prm;
    // the moving frame: the preference acts while a motion horizon holds the velocities (d_hzVel, uploaded with the tables above)
    a.frame = (ctx->frame_on && ctx->hz_mode == 1) ? 1 : 0;
    a.frame_max = ctx->frame_max;
    a.hzVel = ctx->d_hzVel; a.ldVel = 3;
    a.rowObs = ctx->d_idx;
    // screening where the context asks for it, the fused step runs and a bound stands (measured now when none does)
    bool screen = fused_step_available(ctx) && screen_wanted(ctx);
    if (screen && ctx->hz_mode) {   // a bound measured without a horizon, or on another last slab, does not stand for this one (omds.h)
        std::vector<float> last;
        obstacle_horizon_last_slab(ctx, last);
        ctx->scr.horizon_changed(last.data(), ctx->n_obs);
    }
    if (screen && (rc = screen_calibrated(ctx, q_cur, &screen))) return rc;
    if ((rc = enqueue_rollouts(ctx, a, choose_route(ctx, screen)))) return rc;
    CK(hipGetLastError());
    ctx->have_cost_vals = false;
    CK(hipStreamSynchronize(ctx->stream));
    ctx->have_rollouts = true;
    if (screen && (rc = screened_verdict(ctx, a))) return rc;
    return OMDS_OK;
}

int omds_get_pipeline_info(omds_ctx* ctx, int32_t* parts, int32_t* split) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (parts) *parts = ctx->pipe_parts;
    if (split) *split = ctx->pipe_parts == 2 ? ctx->pipe_split : ctx->cfg.n_traj;
    return OMDS_OK;
}

int omds_get_rollouts(omds_ctx* ctx, float* all_traj, float* closest_dist_all, float* kernel_val_all, float* dot_products,
                      float* kernel_activations, float* qdot, float* normal) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CK(hipSetDevice(ctx->dev));
    const int N = ctx->cfg.n_traj, H = ctx->cfg.horizon, n = ctx->cfg.n_dof, K = ctx->n_kernels, Km = ctx->cfg.n_kernel_max;
    auto fetch = [&](const float* srcT, float* dst, int X, int Xld) -> int {
        if (!dst || X == 0) return OMDS_OK;
        omds_launch_permute_hxn_to_nhx(ctx->stream, srcT, ctx->d_stage, H, X, N, Xld);
        CK(hipMemcpyAsync(dst, ctx->d_stage, (size_t)N * H * X * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
        return OMDS_OK;
    };
    int rc;
    if ((rc = fetch(ctx->d_trajT, all_traj, n, n))) return rc;
    if ((rc = fetch(ctx->d_distT, closest_dist_all, 1, 1))) return rc;
    if ((rc = fetch(ctx->d_kvalT, kernel_val_all, K, Km))) return rc;
    if ((rc = fetch(ctx->d_dotT, dot_products, 1, 1))) return rc;
    if ((rc = fetch(ctx->d_actT, kernel_activations, 1, 1))) return rc;
    if ((rc = fetch(ctx->d_normalT, normal, n, n))) return rc;
    if (qdot) {
        omds_launch_transpose(ctx->stream, ctx->d_qdotT, ctx->d_stage, n, N);
        CK(hipMemcpyAsync(qdot, ctx->d_stage, (size_t)N * n * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

// The rows of a few rollouts (reference layouts): what a planner loop reads per iteration -- the best rollout for its FK
// payload, the rollout a new kernel's centre came from (frankaPlanner.py:147-168) -- without moving the N x H tensors.
int omds_get_rollout_rows(omds_ctx* ctx, const int32_t* t, int count, float* all_traj, float* closest_dist_all, float* kernel_val_all,
                          float* dot_products, float* kernel_activations, float* qdot, float* normal) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const int N = ctx->cfg.n_traj, H = ctx->cfg.horizon, n = ctx->cfg.n_dof, K = ctx->n_kernels, Km = ctx->cfg.n_kernel_max;
    REQUIRE(t && count >= 1 && count <= N, OMDS_ERR_INVALID_ARG, "omds_get_rollout_rows: need 1 <= count <= n_traj and a non-null index array");
    for (int r = 0; r < count; ++r) REQUIRE(t[r] >= 0 && t[r] < N, OMDS_ERR_INVALID_ARG, "omds_get_rollout_rows: rollout index out of range");
    REQUIRE(ctx->have_rollouts, OMDS_ERR_NOT_INITIALISED, "omds_get_rollout_rows: no rollouts yet (omds_propagate)");
    CK(hipSetDevice(ctx->dev));
    const size_t per = (size_t)H * (2 * n + 3 + K) + n;   // floats per rollout over all seven outputs
    REQUIRE((per * count + count) * 4 <= ctx->d_stage.bytes(), OMDS_ERR_INVALID_ARG, "omds_get_rollout_rows: too many rollouts for the staging buffer");
    int* d_t = reinterpret_cast<int*>(ctx->d_stage + per * count);
    CK(hipMemcpyAsync(d_t, t, (size_t)count * 4, hipMemcpyHostToDevice, ctx->stream));
    struct Out { const float* src; float* dst; int Hh, X, Xld; };
    const Out outs[] = {{ctx->d_trajT, all_traj, H, n, n}, {ctx->d_distT, closest_dist_all, H, 1, 1}, {ctx->d_kvalT, kernel_val_all, H, K, Km},
                        {ctx->d_dotT, dot_products, H, 1, 1}, {ctx->d_actT, kernel_activations, H, 1, 1}, {ctx->d_qdotT, qdot, 1, n, n},
                        {ctx->d_normalT, normal, H, n, n}};
    size_t off = 0, offs[7];
    for (int i = 0; i < 7; ++i) {
        offs[i] = off;
        if (!outs[i].dst || outs[i].X == 0) continue;
        omds_launch_gather_rows(ctx->stream, outs[i].src, ctx->d_stage + off, d_t, count, outs[i].Hh, outs[i].X, N, outs[i].Xld);
        off += (size_t)count * outs[i].Hh * outs[i].X;
    }
    CK(hipGetLastError());
    std::vector<float> host(off);
    if (off) CK(hipMemcpyAsync(host.data(), ctx->d_stage, off * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 7; ++i)
        if (outs[i].dst && outs[i].X) std::memcpy(outs[i].dst, host.data() + offs[i], (size_t)count * outs[i].Hh * outs[i].X * 4);
    return OMDS_OK;
}

#ifdef OMDS_TEST_HOOKS
// Test hooks (include/omds_test_tiles.h; libomds_hip_test.so only): the orders of the last block-ordered launch, the last step's Dmin
int omds_test_tile_orders(omds_ctx* ctx, int32_t* rperm, int32_t* operm) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->d_rperm && ctx->d_operm, OMDS_ERR_NOT_INITIALISED, "omds_test_tile_orders: no block-ordered launch has run on this context");
    REQUIRE(ctx->pipe_parts == 1, OMDS_ERR_UNSUPPORTED, "omds_test_tile_orders: the last propagate ran in two parts, each with an order of its own (OMDS_FLAG_SERIAL_PROPAGATE)");
    CK(hipSetDevice(ctx->dev));
    CK(hipStreamSynchronize(ctx->stream));
    if (rperm) CK(hipMemcpy(rperm, ctx->d_rperm, (size_t)ctx->cfg.n_traj * 4, hipMemcpyDeviceToHost));
    if (operm) CK(hipMemcpy(operm, ctx->d_operm, (size_t)ctx->n_obs * 4, hipMemcpyDeviceToHost));
    return OMDS_OK;
}
int omds_test_tile_state(omds_ctx* ctx, uint32_t* rkey, uint32_t* okey, int32_t* rperm, int32_t* operm, int32_t* unit, float* W, float* cR, float* cO) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(rkey && okey && rperm && operm && unit && W && cR && cO, OMDS_ERR_INVALID_ARG, "omds_test_tile_state: NULL output");
    REQUIRE(ctx->d_rperm && ctx->d_operm && ctx->d_tileKeys, OMDS_ERR_NOT_INITIALISED, "omds_test_tile_state: no block-ordered launch has run on this context");
    REQUIRE(ctx->pipe_parts == 1, OMDS_ERR_UNSUPPORTED, "omds_test_tile_state: the last propagate ran in two parts, each with an order of its own (OMDS_FLAG_SERIAL_PROPAGATE)");
    CK(hipSetDevice(ctx->dev));
    CK(hipStreamSynchronize(ctx->stream));
    TileKeys k;
    CK(hipMemcpy(&k, ctx->d_tileKeys, sizeof(TileKeys), hipMemcpyDeviceToHost));
    CK(hipMemcpy(rkey, ctx->d_rkey, (size_t)ctx->cfg.n_traj * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(okey, ctx->d_okey, (size_t)ctx->n_obs * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(rperm, ctx->d_rperm, (size_t)omds_order_pad(ctx->cfg.n_traj) * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(operm, ctx->d_operm, (size_t)omds_order_pad(ctx->n_obs) * 4, hipMemcpyDeviceToHost));
    std::memcpy(unit, k.unit, sizeof(k.unit));
    std::memcpy(W, k.W, sizeof(k.W));
    std::memcpy(cR, k.cR, sizeof(k.cR));
    std::memcpy(cO, k.cO, sizeof(k.cO));
    return OMDS_OK;
}
int omds_test_read_dmin(omds_ctx* ctx, float* dmin) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(dmin && ctx->have_rollouts, OMDS_ERR_NOT_INITIALISED, "omds_test_read_dmin: no propagate has run on this context");
    CK(hipSetDevice(ctx->dev));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipMemcpy(dmin, ctx->d_Dmin, (size_t)ctx->cfg.n_traj * ctx->n_obs * 4, hipMemcpyDeviceToHost));
    return OMDS_OK;
}
#endif

}  // extern "C"
