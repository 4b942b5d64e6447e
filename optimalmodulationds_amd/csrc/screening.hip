// The controller of the screened step (pass 1 in fp16 + exact re-selection, screen_kernel.hip; state: ScreenHost, omds_internal.h):
// mode, the unit order of the screening pack, calibration of the bound, the audit sample and the sweeps of a propagate, the
// verdict on what it measured and the fallback, the omds_set_screening* / omds_screen_* entry points and the two test hooks.
// The launch sequences of the screened routes are propagate.hip's; they call screen_begin_propagate / enqueue_sweep_of_step /
// screen_finish_propagate here.
#include "capi_internal.h"
#ifdef OMDS_TEST_HOOKS
#include "omds_test.h"
#include "omds_test_horizon.h"
#endif

bool screen_wanted(omds_ctx* ctx) {
    if (!ctx->scr.ok || ctx->scr.suspended) return false;
    // an obstacle horizon is screened only where the caller asked for it (omds_set_screening_horizon): the routes, the sweep and
    // k_audit then read the step's slab, and the bound is measured on three slabs (calibrate_screen); otherwise the all-fp32 step
    if (ctx->hz_mode && !ctx->scr.over_horizon) return false;
    int mode = ctx->scr.mode;
    if (mode < 0) {   // the library's default: the all-fp32 step -- screening is OPT-IN (omds.h); OMDS_SCREEN=0|1|2 sets the default of such contexts
        static int env = -2;
        if (env == -2) { const char* e = getenv("OMDS_SCREEN"); env = e ? atoi(e) : 0; }
        mode = env;
    }
    if (mode <= 0) return false;
    if (mode == 1) return true;
    // 2 = where it pays: once pass 1 is throughput-bound (below that a step is a chain of latency-bound launches and the
    // three extra launches cost more than the fp32 pass)
    return (long long)ctx->cfg.n_traj * ctx->n_obs >= 64LL * 1024 && ctx->n_obs >= 4 * ctx->cfg.n_closest;
}

// The screening pack's unit order from what the network does on the calibration batch.  k_exact (the fp32 tile code, TileMode::List) is run
// once on a uniform pseudo-random sample of the (state, obstacle) pairs of the B calibration states (their layer-1 halves are in
// d_Fq) and leaves their ReLU masks
// (ExactOut::mask, [entries][hidden levels][8 words]); per hidden level the units are sorted by how many of the sampled 32-pair blocks
// they fired in (ties by index), the pack is built again in that order and copied over the old one.  (The candidates' own masks would be
// there for free, but they are the NEAREST obstacles only: ordered by them, 17 % of the k-chunks of the shipped network are dead for a
// wave; ordered by a uniform sample, 25 %.)  Any order computes the same screening function up to the rounding of the fp32
// accumulation; what the order buys is that k_screen's zero test finds whole 16-unit chunks dead.  The fp32 kernels do not use this
// pack: no returned number changes.
// Called twice per calibration: by the calibration itself on its batch of states (B of them, layer-1 halves in d_Fq) -- so that the
// bound is measured on a sorted pack and the first propagate already runs on one -- and behind the first propagate that is accepted
// afterwards on the states its rollouts ended in (from_rollouts: B = n_traj), which is where the next rollouts will be: the
// calibration batch is deliberately broader than the rollouts, and fewer units are silent on it (3 / 41 / 92 / 120 of the shipped
// network's 256 per layer against 27 / 42 / 93 / 120).
static int screen_reorder(omds_ctx* ctx, int B, bool from_rollouts) {
    const MlpDev& m = ctx->mlp;
    if (from_rollouts) ctx->scr.reorder_pending = false;
    if (m.act != OMDS_ACT_RELU || m.skip_mask || ctx->scr.W.empty() || !ctx->d_exMask) return OMDS_OK;
    if (from_rollouts)   // layer-1 halves of the last states the propagate reached (d_Fq is rebuilt at the start of every propagate)
        omds_launch_rollout_features(ctx->stream, m, ctx->d_trajT + (size_t)(ctx->cfg.horizon - 1) * ctx->cfg.n_dof * ctx->cfg.n_traj, ctx->cfg.n_traj, B, ctx->d_Fq);
    const int nhid = m.nhh + 1, Wd = OMDS_WIDTH, O = ctx->n_obs;
    const long long pairs = (long long)B * O;
    const int S = (int)std::min<long long>({8192, (long long)ctx->ex_cap, pairs});
    if (S < 64) return OMDS_OK;
    CK(ctx->scr.d_tmp.reserve(8));
    std::vector<int32_t> list(S + 1);
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(ctx->scr.recals + 1);
    // the sample is made of BLOCKS of 32 consecutive pairs (one state, 32 consecutive obstacles): what a wave of k_screen multiplies
    // together, and so what a chunk has to be silent for
    for (int j = 0; j < S; j += 32) {   // splitmix64: a fixed sequence per calibration
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
        const long long p0 = (long long)(z % (uint64_t)std::max<long long>(pairs - 31, 1));
        for (int i = 0; i < 32 && j + i < S; ++i) list[j + i] = (int32_t)std::min<long long>(p0 + i, pairs - 1);
    }
    list[S] = S;
    // pageable sources: the copies have read them when the calls return
    CK(hipMemcpyAsync(ctx->d_rowlist, list.data(), (size_t)S * 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(ctx->scr.d_tmp, 0, 8 * sizeof(int), ctx->stream));
    CK(hipMemcpyAsync(ctx->scr.d_tmp + 4, &list[S], 4, hipMemcpyHostToDevice, ctx->stream));
    ExactOut ex{ctx->d_exD, ctx->d_exDr, ctx->d_exMin, ctx->d_exMask, ctx->ex_cap};
    omds_launch_exact(ctx->stream, m, ctx->d_Fq, ctx->d_Fp, ctx->d_radius, O, B, ctx->prm.ignored_links, ctx->d_Dmin, ctx->d_rowlist,
                      ctx->scr.d_tmp + 4, reinterpret_cast<unsigned*>(ctx->scr.d_tmp.get()), ex);
    CK(hipGetLastError());
    std::vector<uint32_t> masks((size_t)S * nhid * 8);
    CK(hipMemcpyAsync(masks.data(), ctx->d_exMask, masks.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> order((size_t)nhid * Wd);
    std::vector<int> count(Wd);
    for (int L = 0; L < nhid; ++L) {
        std::fill(count.begin(), count.end(), 0);
        for (int e0 = 0; e0 < S; e0 += 32) {   // a unit counts once per block it fires in
            uint32_t any[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int e = e0; e < std::min(e0 + 32, S); ++e)
                for (int wi = 0; wi < 8; ++wi) any[wi] |= masks[((size_t)e * nhid + L) * 8 + wi];
            const uint32_t* mr = any;
            for (int wi = 0; wi < 8; ++wi)
                for (uint32_t w = mr[wi]; w; w &= w - 1) {
                    const int bit = __builtin_ctz(w);
                    // level 0: word 2c + h holds the ballot of component c over lanes 32h .. 32h + 31, lane l <-> unit 4l + c;
                    // later levels: word wi holds units 32 wi .. 32 wi + 31 (pass1_tile.h)
                    count[L == 0 ? 4 * (32 * (wi & 1) + bit) + (wi >> 1) : 32 * wi + bit]++;
                }
        }
        int32_t* ord = &order[(size_t)L * Wd];
        for (int u = 0; u < Wd; ++u) ord[u] = u;
        std::stable_sort(ord, ord + Wd, [&](int a1, int a2) { return count[a1] > count[a2]; });
        ctx->scr.never_fired[L] = (int)std::count(count.begin(), count.end(), 0);
    }
    MlpPacks pk;
    pk.nhh = m.nhh; pk.C = m.C; pk.d = m.d; pk.act = m.act; pk.skip_mask = m.skip_mask;
    pk.host_W = std::move(ctx->scr.W); pk.host_b = std::move(ctx->scr.b); pk.out_dims = ctx->scr.out_dims;
    build_screen_pack(pk, order.data());
    ctx->scr.W = std::move(pk.host_W); ctx->scr.b = std::move(pk.host_b);
    // the stream is idle (synchronised above, nothing enqueued since): the pack is replaced in place
    CK(hipMemcpy(const_cast<void*>(ctx->screen.Wh), pk.wh.data(), pk.wh.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(const_cast<float*>(ctx->screen.bias), pk.sbias.data(), pk.sbias.size() * 4, hipMemcpyHostToDevice));
    ctx->scr.reorders++;
    return OMDS_OK;
}

// eps = 6 x the largest |screening value - fp32 value| over a calibration batch of up to 1024 states x all obstacles
// (~3e5 pairs: about what one propagate evaluates per step), against the CURRENT obstacle set: half of the states uniform
// inside the joint limits (omds_set_cost) or [-pi, pi], half drawn from the rollouts of the last propagate -- where the next
// rollouts will live -- or, before the first propagate, scattered around the start state (sigma 0.6 rad).  Everything runs on
// the device (k_calib_states -> layer 1 -> k_pass1 and k_screen -> k_max_abs_diff); four bytes come back.  Run at the first
// screened propagate after omds_set_mlp, after omds_set_obstacles with a changed scene (scene_differs_from_calibration), after
// a change of ignored_links and on request (omds_set_screening(mode, eps < 0)).  Between calibrations every propagate
// re-measures the error on its candidates and on the audit sample of the unevaluated pairs (omds_propagate).
// With an obstacle horizon in effect (screen_wanted let it through) the same states are measured against slabs 0, (H-1)/2 and H-1
// -- k_pass1 and k_screen on each slab's fp32 / fp16 tables -- and eps is 6 x the maximum over them; the unit re-sort stays on
// slab 0 (no returned number depends on it).  What the calibration stood on is recorded: slab 0, the last slab, and that a horizon
// was in effect (ScreenHost::horizon_changed).
static int calibrate_screen(omds_ctx* ctx, const float* q_center) {
    ctx->scr.cal = true;
    ctx->scr.obs_cal = ctx->obs_now;
    ctx->scr.cal_horizon = ctx->hz_mode != 0;
    if (ctx->scr.cal_horizon) obstacle_horizon_last_slab(ctx, ctx->scr.last_cal);
    else ctx->scr.last_cal.clear();
    const int n = ctx->cfg.n_dof, O = ctx->n_obs;
    const int B = std::min(ctx->cfg.n_traj, 1024);
    float lo[OMDS_MAX_DOF], hi[OMDS_MAX_DOF];
    for (int j = 0; j < n; ++j) {
        lo[j] = ctx->have_cost ? ctx->qmin[j] : -3.14159265f;
        hi[j] = ctx->have_cost ? ctx->qmax[j] : 3.14159265f;
    }
    omds_launch_calib_states(ctx->stream, ctx->d_qstage, B, n, lo, hi, q_center, ctx->have_rollouts ? ctx->d_trajT.get() : nullptr,
                             ctx->cfg.n_traj, ctx->cfg.horizon, 0x9E3779B9u * (unsigned)(ctx->scr.recals + 1));
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_qstage, B, B, ctx->d_Fq, ctx->d_FqH, ctx->cfg.n_traj);
    // first the unit order of the screening pack (it follows the scene and the states too), then the bound of THAT pack
    int rc;
    if ((rc = screen_reorder(ctx, B, false))) return rc;
    ctx->scr.reorder_pending = true;
    if (ctx->scr.eps_fixed && ctx->scr.eps > 0.f) return OMDS_OK;   // the bound was set by the caller (omds_set_screening)
    float* apx = ctx->d_stage;   // [B][O] screening values (d_stage holds >= n_traj * max_obs floats)
    CK(hipMemsetAsync(ctx->d_scerr + 3, 0, 4, ctx->stream));
    const int Hh = ctx->cfg.horizon;
    int steps[3] = {1, (Hh - 1) / 2 + 1, Hh}, n_steps = 0;   // horizon steps whose slabs are measured (step i reads slab i - 1), duplicates removed
    for (int j = 0; j < (ctx->scr.cal_horizon ? 3 : 1); ++j)
        if (n_steps == 0 || steps[j] != steps[n_steps - 1]) steps[n_steps++] = steps[j];
    for (int j = 0; j < n_steps; ++j) {   // the maximum over the slabs: k_max_abs_diff accumulates into the same word
        const ObsTables t = obstacle_tables(ctx, steps[j]);
        const ScreenTables st = screen_tables(ctx, steps[j]);
        omds_launch_pass1(ctx->stream, ctx->mlp, ctx->d_Fq, t.Fp, t.radius, O, B, ctx->prm.ignored_links, ctx->d_Dmin);
        omds_launch_screen(ctx->stream, ctx->screen, st.m, ctx->d_FqH, ctx->cfg.n_traj, st.FpH, st.ld, st.radius, O, B, ctx->prm.ignored_links, apx);
        omds_launch_max_abs_diff(ctx->stream, ctx->d_Dmin, apx, (long long)B * O, ctx->d_scerr + 3);
    }
    CK(hipGetLastError());
    float worst = 0.f;
    CK(hipMemcpyAsync(&worst, ctx->d_scerr + 3, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    ctx->scr.recals++;
    ctx->scr.err_seen = 0.f;
    ctx->scr.audit_err_seen = 0.f;
    ctx->scr.sweep_err_seen = 0.f;
    const bool finite = worst < 3.0e38f;
    if (!finite) { ctx->scr.suspended = true; ctx->scr.eps = 0.f; return OMDS_OK; }   // fp16 range exceeded on this scene: the fp32 step until the next calibration
    // The largest error over the ~10^7 pairs of a propagate was seen at up to 2x the calibration batch's maximum (3.8e-3 vs
    // 1.8e-3 .. 2.3e-3 on the shelf scene, depending on the batch drawn): 6x leaves the run-time guard (fallback above
    // eps / 2) room for a 3x larger error, and the accepted propagates then keep eps at >= 4x the largest error they saw --
    // on the shelf both routes end at 1.5e-2.  (8x of an unlucky batch, 1.9e-2, costs 1.2 candidates per rollout and step,
    // which at N = 1024 pushes k_exact past two tiles per CU: 4.8 M against 5.2 M rollout-steps/s.)
    ctx->scr.eps = std::max(6.f * worst, 1e-12f);
    return OMDS_OK;
}

int screen_calibrated(omds_ctx* ctx, const float* q_center, bool* usable) {
    int rc;
    if (!ctx->scr.cal && (rc = calibrate_screen(ctx, q_center))) return rc;
    *usable = ctx->scr.ok && !ctx->scr.suspended && ctx->scr.eps > 0.f;
    return OMDS_OK;
}

// Has the scene changed enough since the screening bound was calibrated that the calibration batch no longer stands for it?
// Another obstacle count, another radius, or any sphere more than 0.1 (scene units: metres for the Franka scenes) away from
// where it was: a translating / vibrating scene (obstacleStreamer.py:125-137) keeps its bound, a swapped scene does not.
// (Every step of every propagate additionally audits a sample of the unevaluated pairs, omds.h.)
static bool scene_differs(const std::vector<float>& was, const float* xyzr, int n_obs) {
    bool differs = was.size() != (size_t)n_obs * 4;
    for (int i = 0; i < n_obs && !differs; ++i) {
        const float* a = &was[(size_t)i * 4];
        const float* b = xyzr + (size_t)i * 4;
        for (int c = 0; c < 3; ++c) differs = differs || !(std::fabs(a[c] - b[c]) <= 0.1f);
        differs = differs || !(std::fabs(a[3] - b[3]) <= 1e-6f);
    }
    return differs;
}
void ScreenHost::scene_changed(const float* xyzr, int n_obs) {
    if (!cal || eps_fixed) return;
    if (scene_differs(obs_cal, xyzr, n_obs)) forget_calibration();   // calibrate again at the next screened propagate, against THIS scene
}
// The same question about the far end of an obstacle horizon, asked at every screened propagate that has one: a bound measured
// without a horizon has seen slab 0 only, and one measured on another last slab (other velocities, another table; the same test)
// does not stand for this one.  Slab 0 is omds_set_obstacles' business (scene_changed), so a scene that keeps translating at
// constant velocities recalibrates as often as a static translating scene does; a bound measured under a horizon also covers the
// static scene (clearing the horizon forgets nothing); the caller's own bound is never forgotten.
void ScreenHost::horizon_changed(const float* last, int n_obs) {
    if (!cal || eps_fixed) return;
    if (!cal_horizon || scene_differs(last_cal, last, n_obs)) forget_calibration();
}

// Buffers of the audit sample (allocated at the first screened propagate, grown when the scene or the rate asks for more):
// the list itself -- about N*H*O / one_in entries, room for twice that -- and the layer-1 table of all horizon steps.
static int prepare_audit(omds_ctx* ctx, SelectSink& sk) {
    ScreenHost& S = ctx->scr;
    sk.audit_rows = nullptr; sk.audit_da = nullptr; sk.audit_total = ctx->d_sctotal + (ctx->cfg.horizon + 1); sk.audit_cap = 0;
    sk.audit_mask = 0xffffffffu;
    const long long N = ctx->cfg.n_traj, H = ctx->cfg.horizon, O = ctx->n_obs;
    if (S.audit_one_in <= 0 || N * H * O >= (1LL << 31)) return OMDS_OK;   // no audit (or a row space beyond 32-bit indices)
    // an obstacle horizon: k_audit_slabs gathers the obstacle rows of all slabs through one buffer descriptor with 32-bit byte offsets
    if (ctx->hz_mode && (long long)H * ctx->hz_ld * (OMDS_FROW * 4) >= (1LL << 31)) return OMDS_OK;
    const size_t want = (size_t)(N * H * (2 * O / S.audit_one_in + 4));
    if (want > std::min(S.d_audit_rows.count(), S.d_audit_da.count())) {
        CK(hipStreamSynchronize(ctx->stream));
        CK(S.d_audit_rows.reserve(want));
        CK(S.d_audit_da.reserve(want));
    }
    if (!ctx->d_FqAll) {
        CK(ctx->d_FqAll.alloc((size_t)N * H * OMDS_FROW));
        CK(hipMemsetAsync(ctx->d_FqAll, 0, ctx->d_FqAll.bytes(), ctx->stream));   // the obstacles' slots and the padding stay zero
    }
    sk.audit_rows = S.d_audit_rows;
    sk.audit_da = S.d_audit_da;
    sk.audit_cap = (int)std::min<size_t>(S.d_audit_rows.count(), 0x7fffffff);
    sk.audit_mask = (unsigned)S.audit_one_in - 1u;
    return OMDS_OK;
}

// Buffers of a sweep (allocated at the first one): the fp32 values and the screening values of all pairs of ONE step, and the
// statistics every sweep adds to.
static int prepare_sweep(omds_ctx* ctx) {
    ScreenHost& S = ctx->scr;
    const size_t pairs = (size_t)ctx->cfg.n_traj * ctx->cfg.max_obs;
    if (pairs > std::min(S.d_sweepD.count(), S.d_sweepDa.count())) {
        CK(hipStreamSynchronize(ctx->stream));
        CK(S.d_sweepD.reserve(pairs));
        CK(S.d_sweepDa.reserve(pairs));
    }
    if (!S.d_sweep_hist) {
        CK(S.d_sweep_hist.alloc(OMDS_SWEEP_HIST_WORDS));
        CK(hipMemsetAsync(S.d_sweep_hist, 0, S.d_sweep_hist.bytes(), ctx->stream));
    }
    return OMDS_OK;
}

// One step swept: ALL N x O pairs in fp32 (k_pass1 on the step's layer-1 halves) beside all N x O screening values (k_screen in
// matrix mode on the step's fp16 inputs), compared against the tau the step's selection used (d_range): max |Da - D| ->
// d_scerr[3], the distribution of Da - D over the non-candidates -> d_sweep_hist.  Must be enqueued between the step's selection
// and its tail (the tail overwrites the fp16 inputs with the next step's states).  Does nothing unless the running propagate
// carries a sweep and this step is part of it (the last one, or every one in the soak mode).
void enqueue_sweep_of_step(omds_ctx* ctx, const float* fq_step, int N, int step) {
    if (!ctx->scr.sweep_now || !(ctx->scr.sweep_all_steps || step == ctx->cfg.horizon)) return;
    RoctxRange r4("screening sweep (all pairs of this step in fp32)");
    const ObsTables t = obstacle_tables(ctx, step);   // the scene this step saw: its slab of an obstacle horizon
    const ScreenTables st = screen_tables(ctx, step);
    omds_launch_pass1(ctx->stream, ctx->mlp, fq_step, t.Fp, t.radius, ctx->n_obs, N, ctx->prm.ignored_links, ctx->scr.d_sweepD);
    omds_launch_screen(ctx->stream, ctx->screen, st.m, ctx->d_FqH, ctx->cfg.n_traj, st.FpH, st.ld, st.radius, ctx->n_obs, N,
                       ctx->prm.ignored_links, ctx->scr.d_sweepDa);
    omds_launch_sweep_hist(ctx->stream, ctx->scr.d_sweepD, ctx->scr.d_sweepDa, ctx->d_range, N, ctx->n_obs, ctx->scr.eps, ctx->scr.d_sweep_hist, ctx->d_scerr + 3);
    ctx->scr.sweep_steps_now++;
}

// Everything a screened propagate sets up in front of its horizon loop.  list_tail: the tail works from k_exact's per-entry
// outputs (k_tail_sel: ReLU masks, or the tanh derivatives in d_exDeriv); then, when a rollout's obstacles fit a workgroup's
// LDS, k_screen selects in its flush phase (no matrix, no k_select).
// With an audit sample the rollout halves of layer 1 of ALL horizon steps are kept ([H][N][OMDS_FROW]: step i reads slab i - 1,
// its tail writes slab i) so that k_audit can re-evaluate pairs of any step at the end; otherwise one slab is updated in place.
int screen_begin_propagate(omds_ctx* ctx, const StepArgs& a, bool list_tail, ScreenPlan* plan) {
    ScreenHost& S = ctx->scr;
    const int N = a.N, H = a.H;
    int rc;
    plan->fq0 = ctx->d_Fq;
    plan->fq_slab = 0;
    plan->fuse_select = list_tail && omds_screen_can_select(ctx->n_obs);
    plan->eps = S.eps;
    CK(hipMemsetAsync(ctx->d_sctotal, 0, (size_t)(H + 2) * 4, ctx->stream));
    CK(hipMemsetAsync(ctx->d_scerr, 0, 16, ctx->stream));
    SelectSink sink{};
    sink.rowlist = ctx->d_rowlist;
    sink.listDa = plan->fuse_select ? ctx->d_listDa.get() : nullptr;
    sink.range = ctx->d_range;
    sink.k = a.k;
    sink.delta = OMDS_SCREEN_WINDOW * S.eps;
    if ((rc = prepare_audit(ctx, sink))) return rc;
    if (sink.audit_rows) { plan->fq0 = ctx->d_FqAll; plan->fq_slab = (size_t)N * OMDS_FROW; }
    plan->ex = ExactOut{ctx->d_exD, ctx->d_exDr, ctx->d_exMin, ctx->d_exMask, ctx->ex_cap};
    plan->ex.Da = sink.listDa;
    plan->ex.deriv = ctx->mlp.act == OMDS_ACT_RELU ? nullptr : ctx->d_exDeriv.get();
    // the sinks of all steps in one copy (the pinned staging is free: the previous propagate has been synchronised)
    SelectSink* hs = S.h_sinks;
    for (int i = 1; i <= H; ++i) {
        hs[i - 1] = sink;
        hs[i - 1].total = ctx->d_sctotal + (i - 1);
        hs[i - 1].audit_seed = 0x9E3779B9u * ++S.audit_counter;
        hs[i - 1].step_row0 = (i - 1) * N;
    }
    CK(hipMemcpyAsync(S.d_sinks, hs, (size_t)H * sizeof(SelectSink), hipMemcpyHostToDevice, ctx->stream));
    plan->h_sinks = hs;
    plan->d_sinks = S.d_sinks;
    // Every sweep_every-th screened propagate carries a SWEEP: a complete fp32 check of its last horizon step -- or, in the soak
    // mode, of every step (omds_set_screening_sweep).  The audit sample sees every step thinly, a sweep sees a step whole.
    S.sweep_now = false;
    S.sweep_steps_now = 0;
    // ... and so does the first propagate on a screening pack whose unit order changed after the bound was measured
    // (screened_verdict: the re-sort on the rollouts' own states): the bound is checked on every pair of a step of the new pack
    // before anything else relies on it
    if (S.sweep_every > 0 && ((S.propagates++ % S.sweep_every) == 0 || S.sweep_force_next)) {
        if ((rc = prepare_sweep(ctx))) return rc;
        S.sweep_now = true;
        S.sweep_force_next = false;
    }
    return OMDS_OK;
}

// The audit sample of this propagate in one throughput-shaped launch: k_audit on the recorded pairs against the kept
// layer-1 slabs of all horizon steps -> d_scerr[2] = max (Da - D); then everything the propagate measured about its
// screening values comes back through pinned memory.  (Measured and rejected in round 4: k_audit on a second,
// low-priority stream with the verdict deferred to the next call that publishes results, so that the cost and update
// kernels run beside it -- 5.92-5.97 ms per iteration against 5.86 ms for this form on the same box,
// profiles/r04_audit_stream_ab.txt: the cross-stream dependency costs more than the 0.07 ms of kernels it overlaps.)
int screen_finish_propagate(omds_ctx* ctx, const ScreenPlan& plan) {
    const SelectSink& sink = plan.h_sinks[0];   // the audit list is one for the whole propagate
    if (sink.audit_rows) {
        RoctxRange r3("screening audit sample (fp32 re-evaluation of unevaluated pairs)");
        if (ctx->hz_mode)   // every listed row against the slab of ITS step, still in one launch
            omds_launch_audit(ctx->stream, ctx->mlp, ctx->d_FqAll, ctx->d_hzFp, ctx->d_hzRadius, ctx->n_obs, ctx->prm.ignored_links,
                              sink.audit_rows, sink.audit_da, sink.audit_total, sink.audit_cap, ctx->d_scerr, ctx->cfg.n_traj, ctx->hz_ld);
        else
            omds_launch_audit(ctx->stream, ctx->mlp, ctx->d_FqAll, ctx->d_Fp, ctx->d_radius, ctx->n_obs, ctx->prm.ignored_links,
                              sink.audit_rows, sink.audit_da, sink.audit_total, sink.audit_cap, ctx->d_scerr);
    }
    CK(hipGetLastError());
    CK(hipMemcpyAsync(ctx->scr.h_verdict, ctx->d_scerr, 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(ctx->scr.h_verdict + 4, ctx->d_sctotal, (size_t)(ctx->cfg.horizon + 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
    return OMDS_OK;
}

// What a screened propagate MEASURED about the screening values it relied on (the pinned verdict words, complete once the stream
// has been synchronised):
//   err   = max |Da - D| over every candidate pair (the rows nearest the decision threshold, all re-evaluated);
//   aerr  = max (Da - D) over the audit sample, a uniform pseudo-random 1 in audit_one_in (another one every step) of
//           the pairs that were NOT re-evaluated -- the population the selection rule's assumption is about --
//           evaluated in fp32 by k_audit at the end of the horizon loop;
//   slack = rollouts whose exact k-th smallest candidate came within eps of tau;
//   serr  = (every sweep_every-th propagate) max |Da - D| over ALL pairs of the swept horizon step(s).
// Accepted only while the errors keep a 2x margin to eps and no slack check failed; otherwise the propagate is redone with
// the fp32 pass 1 -- its results are then the fp32 ones by construction -- before omds_propagate returns.
int screened_verdict(omds_ctx* ctx, StepArgs& a) {
    const int N = ctx->cfg.n_traj, H = ctx->cfg.horizon;
    const float* hv = ctx->scr.h_verdict;
    const float err = hv[0], aerr = hv[2], serr = ctx->scr.sweep_now ? hv[3] : 0.f;
    if (ctx->scr.sweep_now) { ctx->scr.sweeps += ctx->scr.sweep_steps_now; if (serr > ctx->scr.sweep_err_seen || serr != serr) ctx->scr.sweep_err_seen = serr; }
    if (err > ctx->scr.err_seen || err != err) ctx->scr.err_seen = err;
    if (aerr > ctx->scr.audit_err_seen || aerr != aerr) ctx->scr.audit_err_seen = aerr;
    const int32_t* tot = reinterpret_cast<const int32_t*>(hv + 4);
    const uint32_t slack_viol = reinterpret_cast<const uint32_t*>(hv)[1];
    bool overflow = false;   // a step listed more rows than k_exact's per-entry outputs hold: redo in fp32
    for (int i = 0; i < H; ++i) { ctx->scr.rows += tot[i]; overflow = overflow || tot[i] > ctx->ex_cap; }
    ctx->scr.audit_rows += std::min<double>(tot[H + 1], (double)ctx->scr.d_audit_rows.count());   // entries k_audit evaluated
    ctx->scr.steps += (double)N * H;
    const float worst = (err != err || aerr != aerr || serr != serr) ? __builtin_inff() : std::max({err, aerr, serr});
    if (!overflow && worst <= 0.5f * ctx->scr.eps && slack_viol == 0) {
        // accepted.  Keep the bound at >= 4x the largest error seen, so that states drifting into regions where the fp16
        // network is less accurate widen it gradually instead of tripping the fallback
        if (4.f * worst > ctx->scr.eps) ctx->scr.eps = 4.f * worst;
        ctx->scr.consec = 0;
        if (ctx->scr.reorder_pending) {   // the unit order once more, on the states the rollouts reached.  eps was measured on the
            // calibration's order: the next propagate carries a sweep (all N x O pairs of a step of the NEW pack in fp32).  The results
            // of this propagate are published already; d_Fq / d_Dmin / d_ex* are scratch between propagates (omds_internal.h)
            const long long before = ctx->scr.reorders;
            const int rrc = screen_reorder(ctx, N, true);
            if (ctx->scr.reorders != before) ctx->scr.sweep_force_next = true;
            return rrc;
        }
        return OMDS_OK;
    }
    // the bound lost its margin on live data (or the list outgrew its buffers): this propagate is redone in fp32 and the bound
    // is widened.  Three in a row: the screening network is not usable on this scene (out of its fp16 range, a scene far from
    // the calibration batch, corrupted weights); the context stays on the fp32 step until the next calibration
    // (omds_set_obstacles with a changed scene, omds_set_mlp, omds_set_screening(mode, eps < 0))
    ctx->scr.fallbacks++;
    if (overflow) ctx->scr.fb_overflow++;
    else if (!(worst <= 0.5f * ctx->scr.eps)) ctx->scr.fb_error++;
    else ctx->scr.fb_slack++;
    if (!overflow && worst < 3.0e38f) ctx->scr.eps = std::max(ctx->scr.eps, 4.f * worst);
    if (++ctx->scr.consec >= 3 || !(worst < 3.0e38f)) { if (!ctx->scr.suspended) ctx->scr.suspensions++; ctx->scr.suspended = true; }
    int rc;
    if ((rc = enqueue_rollouts(ctx, a, choose_route(ctx, false)))) return rc;   // from trajT[0], which no step overwrites
    CK(hipGetLastError());
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

// ---- screening controls ------------------------------------------------------------------------------
extern "C" {

int omds_set_screening(omds_ctx* ctx, int mode, float eps) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(mode >= -1 && mode <= 2 && eps == eps, OMDS_ERR_INVALID_ARG, "omds_set_screening: mode in {-1, 0, 1, 2}, eps not NaN");
    ctx->scr.mode = mode;
    if (eps > 0.f) {            // the caller's bound instead of a calibration (the run-time checks still widen it when they must)
        ctx->scr.eps = eps; ctx->scr.eps_fixed = true; ctx->scr.cal = true;
        ctx->scr.obs_cal = ctx->obs_now; ctx->scr.cal_horizon = false; ctx->scr.last_cal.clear();
        ctx->scr.suspended = false; ctx->scr.consec = 0;
    } else if (eps < 0.f) {     // forget the calibration: measured again at the next screened propagate
        ctx->scr.eps = 0.f; ctx->scr.eps_fixed = false;
        ctx->scr.forget_calibration();
    }                           // eps == 0: the mode only; bound, calibration and everything measured so far stay
    return OMDS_OK;
}
int omds_set_screening_horizon(omds_ctx* ctx, int on) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(on == 0 || on == 1, OMDS_ERR_INVALID_ARG, "omds_set_screening_horizon: on in {0, 1}");
    const bool was = ctx->scr.over_horizon;
    ctx->scr.over_horizon = on != 0;
    if (was && !on && (ctx->d_hzFpH || ctx->d_hzFpS)) {   // the fp16 slab tables go: the context is what it was before the switch
        CK(hipSetDevice(ctx->dev));
        CK(hipStreamSynchronize(ctx->stream));
        ctx->d_hzFpH.reset(); ctx->d_hzFpS.reset();
    }
    return OMDS_OK;   // on: prepare_obstacle_horizon builds the fp16 slab tables with the next rebuild
}
int omds_get_screening_horizon(omds_ctx* ctx, int32_t* on, int32_t* in_effect) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (on) *on = ctx->scr.over_horizon ? 1 : 0;
    if (in_effect) *in_effect = (ctx->hz_mode && ctx->scr.over_horizon && fused_step_available(ctx) && screen_wanted(ctx)) ? 1 : 0;
    return OMDS_OK;
}
int omds_set_screening_audit(omds_ctx* ctx, int one_in) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(one_in >= 0 && one_in <= (1 << 20) && (one_in & (one_in - 1)) == 0, OMDS_ERR_INVALID_ARG,
            "omds_set_screening_audit: one_in must be 0 (no audit rows) or a power of two <= 2^20");
    ctx->scr.audit_one_in = one_in;
    return OMDS_OK;
}
int omds_set_screening_sweep(omds_ctx* ctx, int every, int all_steps) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(every >= 0 && (all_steps == 0 || all_steps == 1), OMDS_ERR_INVALID_ARG, "omds_set_screening_sweep: every >= 0 (0 = no sweeps), all_steps in {0, 1}");
    ctx->scr.sweep_every = every;
    ctx->scr.sweep_all_steps = all_steps != 0;
    return OMDS_OK;
}
int omds_screen_sweep_hist(omds_ctx* ctx, uint64_t* words, int n_words, int reset) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(words && n_words == OMDS_SWEEP_HIST_WORDS, OMDS_ERR_INVALID_ARG, "omds_screen_sweep_hist: words must hold OMDS_SWEEP_HIST_WORDS entries");
    CK(hipSetDevice(ctx->dev));
    std::memset(words, 0, (size_t)n_words * 8);
    if (!ctx->scr.d_sweep_hist) return OMDS_OK;   // no sweep has run yet
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipMemcpy(words, ctx->scr.d_sweep_hist, (size_t)n_words * 8, hipMemcpyDeviceToHost));
    words[OMDS_HIST_STEPS] = (uint64_t)ctx->scr.sweeps;
    if (reset) { CK(hipMemset(ctx->scr.d_sweep_hist, 0, (size_t)n_words * 8)); ctx->scr.sweeps = 0; }
    return OMDS_OK;
}
int omds_screen_sweep_stats(omds_ctx* ctx, int32_t* every, int64_t* sweeps, float* sweep_max_err) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (every) *every = ctx->scr.sweep_every;
    if (sweeps) *sweeps = ctx->scr.sweeps;
    if (sweep_max_err) *sweep_max_err = ctx->scr.sweep_err_seen;
    return OMDS_OK;
}
int omds_screen_order_stats(omds_ctx* ctx, int64_t* reorders, int32_t* never_fired, int n_levels) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(n_levels >= 0 && n_levels <= OMDS_MAX_HIDDEN + 1, OMDS_ERR_INVALID_ARG, "omds_screen_order_stats: 0 <= n_levels <= 9");
    if (reorders) *reorders = ctx->scr.reorders;
    if (never_fired)
        for (int L = 0; L < n_levels; ++L) never_fired[L] = ctx->scr.never_fired[L];
    return OMDS_OK;
}
int omds_screen_fallback_stats(omds_ctx* ctx, int64_t* by_error, int64_t* by_slack, int64_t* by_overflow, int64_t* suspensions) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (by_error) *by_error = ctx->scr.fb_error;
    if (by_slack) *by_slack = ctx->scr.fb_slack;
    if (by_overflow) *by_overflow = ctx->scr.fb_overflow;
    if (suspensions) *suspensions = ctx->scr.suspensions;
    return OMDS_OK;
}
int omds_screen_audit_stats(omds_ctx* ctx, int32_t* one_in, double* audit_rows_per_rollout_step, float* audit_max_err,
                            int32_t* suspended, int64_t* calibrations) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (one_in) *one_in = ctx->scr.audit_one_in;
    if (audit_rows_per_rollout_step) *audit_rows_per_rollout_step = ctx->scr.steps > 0 ? ctx->scr.audit_rows / ctx->scr.steps : 0.0;
    if (audit_max_err) *audit_max_err = ctx->scr.audit_err_seen;
    if (suspended) *suspended = ctx->scr.suspended ? 1 : 0;
    if (calibrations) *calibrations = ctx->scr.recals;
    return OMDS_OK;
}
#ifdef OMDS_TEST_HOOKS
// Test hooks (include/omds_test.h; libomds_hip_test.so only -- the release library does not export them).
// omds_screen_debug_corrupt (tests/test_gpu_screen_audit.py): damages the screening network's inputs so that the run-time
// checks have something to catch.  what = 0: zeroes weight fragment `index` (1 KiB of slice index / 16) of the fp16 pack -- every
// screening value moves; what = 1: shifts obstacle `index` by `value` along x in the SCREENING input table only (undone by
// the next omds_set_obstacles) -- the fp16 network sees that one sphere elsewhere, so only the audit rows can notice.
int omds_debug_force_tile_rows(int tail_sel_rows, int tail_rows) {
    if (!((tail_sel_rows == 0 || tail_sel_rows == 4 || tail_sel_rows == 16 || tail_sel_rows == 32) && (tail_rows == 0 || tail_rows == 4 || tail_rows == 16 || tail_rows == 32)))
        return OMDS_ERR_INVALID_ARG;
    omds_force_tile_rows(tail_sel_rows, tail_rows);
    return OMDS_OK;
}

int omds_screen_debug_corrupt(omds_ctx* ctx, int what, int index, float value) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->scr.ok, OMDS_ERR_UNSUPPORTED, "omds_screen_debug_corrupt: no screening network for this model");
    CK(hipSetDevice(ctx->dev));
    CK(hipStreamSynchronize(ctx->stream));
    if (what == 0) {
        const int nfrag = (ctx->mlp.nhh * 8 + 2) * 16;
        REQUIRE(index >= 0 && index < nfrag, OMDS_ERR_INVALID_ARG, "omds_screen_debug_corrupt: fragment index out of range");
        CK(hipMemset(const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(ctx->screen.Wh)) + (size_t)index * 1024, 0, 1024));
        return OMDS_OK;
    }
    REQUIRE(what == 1 && index >= 0 && index < ctx->n_obs, OMDS_ERR_INVALID_ARG, "omds_screen_debug_corrupt: what in {0, 1}, obstacle index in range");
    const int n = ctx->cfg.n_dof, d = ctx->mlp.d, ld = ctx->cfg.max_obs;
    const float x = ctx->obs_now[(size_t)index * 4] + value;
    const float f[3] = {x, std::sin(x), std::cos(x)};
    for (int part = 0; part < 3; ++part) {
        const uint16_t h = f32_to_f16_bits(f[part]);
        CK(hipMemcpy(ctx->d_FpH + omds_screen_fidx(part * d + n, index, ld), &h, 2, hipMemcpyHostToDevice));
    }
    return OMDS_OK;
}
// omds_test_screen_corrupt_slab (include/omds_test_horizon.h; tests/test_gpu_screen_horizon.py): what = 1 above for ONE slab of an
// obstacle horizon -- the fp16 network sees that sphere elsewhere at that step only, the fp32 tables stay
int omds_test_screen_corrupt_slab(omds_ctx* ctx, int slab, int index, float dx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->hz_mode && ctx->d_hzFpH && !ctx->hz_dirty, OMDS_ERR_NOT_INITIALISED,
            "omds_test_screen_corrupt_slab: no fp16 slab tables (omds_set_screening_horizon, a horizon, then omds_get_obstacle_horizon)");
    REQUIRE(slab >= 0 && slab < ctx->cfg.horizon && index >= 0 && index < ctx->n_obs, OMDS_ERR_INVALID_ARG,
            "omds_test_screen_corrupt_slab: slab and obstacle index in range");
    CK(hipSetDevice(ctx->dev));
    CK(hipStreamSynchronize(ctx->stream));
    const int n = ctx->cfg.n_dof, d = ctx->mlp.d, ld = ctx->hz_ld;
    float x0 = 0.f;   // the sphere's x in that slab as the tables hold it
    CK(hipMemcpy(&x0, ctx->d_hzObs + ((size_t)slab * ld + index) * 4, 4, hipMemcpyDeviceToHost));
    const float x = x0 + dx;
    const float f[3] = {x, std::sin(x), std::cos(x)};
    for (int part = 0; part < 3; ++part) {
        const uint16_t h = f32_to_f16_bits(f[part]);
        CK(hipMemcpy(ctx->d_hzFpH + (size_t)slab * 32 * ld + omds_screen_fidx(part * d + n, index, ld), &h, 2, hipMemcpyHostToDevice));
    }
    return OMDS_OK;
}
#endif   // OMDS_TEST_HOOKS
// Diagnostic: the screening network alone on a batch (what k_select sees), for tests and for measuring eps.
int omds_screen_mindist(omds_ctx* ctx, const float* q, int B, float* mindist) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(q && mindist && B >= 1 && B <= ctx->cfg.n_traj, OMDS_ERR_INVALID_ARG, "omds_screen_mindist: need 1 <= batch <= n_traj and non-null arrays");
    int rc;
    if ((rc = check_ready(ctx, false))) return rc;
    REQUIRE(ctx->scr.ok, OMDS_ERR_UNSUPPORTED, "omds_screen_mindist: no screening network for this model (ReLU, 2..5 hidden layers)");
    CK(hipSetDevice(ctx->dev));
    const int n = ctx->cfg.n_dof, O = ctx->n_obs;
    CK(hipMemcpyAsync(ctx->d_stage, q, (size_t)B * n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_qstage, B, n);
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_qstage, B, B, ctx->d_Fq, ctx->d_FqH, ctx->cfg.n_traj);
    omds_launch_screen(ctx->stream, ctx->screen, ctx->mlp, ctx->d_FqH, ctx->cfg.n_traj, ctx->d_FpH, ctx->cfg.max_obs, ctx->d_radius, O, B, ctx->prm.ignored_links, ctx->d_Dmin);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(mindist, ctx->d_Dmin, (size_t)B * O * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}
int omds_screen_stats(omds_ctx* ctx, int32_t* active, float* eps, float* max_err_seen, double* cand_per_rollout_step,
                      int64_t* fallbacks) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (active) *active = (ctx->scr.ok && screen_wanted(ctx)) ? 1 : 0;
    if (eps) *eps = ctx->scr.eps;
    if (max_err_seen) *max_err_seen = ctx->scr.err_seen;
    if (cand_per_rollout_step) *cand_per_rollout_step = ctx->scr.steps > 0 ? ctx->scr.rows / ctx->scr.steps : 0.0;
    if (fallbacks) *fallbacks = ctx->scr.fallbacks;
    return OMDS_OK;
}

}  // extern "C"
