// C ABI of libomds_hip.so (include/omds.h), host side: the context's lifetime and buffers, the scene, DS, parameter, cost and
// policy-sample setters and getters, and the measurement entry points.  The other concerns live in mlp_pack.hip (weight packs),
// network.hip (installing and evaluating the distance network), screening.hip (the screened step's controller), propagate.hip
// (the step's routes), update.hip (cost and the cost-weighted update), sdf_data.hip and obstacle_horizon.hip (per-step obstacle tables).
#include "capi_internal.h"

thread_local std::string g_create_err;

extern "C" {

int omds_version(void) { return 512; }

int omds_device_count(int32_t* count) {
    if (!count) return OMDS_ERR_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }   // no device / no driver: zero devices, not a failure
    *count = n;
    return OMDS_OK;
}

void omds_default_params(omds_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->dt = 0.5f;
    p->dst_thr = 0.5f;                                    // MPPI.py:59
    p->lin_thr = 0.015f;                                  // LinDS.py:9
    const float lvel[5] = {0.f, 1.f, -1.f, 0.f, 10.f};    // MPPI.py:132
    const float ln[5] = {0.f, 1.f, 0.f, 0.1f, 100.f};     // MPPI.py:149-153
    const float ltau[5] = {5.f, 1.f, 0.f, 0.1f, 100.f};   // MPPI.py:155 (y_min = ltau_max)
    std::memcpy(p->lvel, lvel, sizeof(lvel));
    std::memcpy(p->ln, ln, sizeof(ln));
    std::memcpy(p->ltau, ltau, sizeof(ltau));
    p->goal_act_cut = 0.5f;
    p->norm_clamp = 0.5f;
    p->coll_slow = 0.1f;
    p->coll_repulse = 0.1f;
    p->softmax_k = -10.f;
    p->rbf_p = 2.f;
    p->ignored_links = 0;
    p->variant = 0;
    p->cost_terms = OMDS_COST_ALL;                        // cost.py:21
}

const char* omds_last_error(const omds_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// what no buffer handle owns (the DevBuf / PinBuf members free themselves when the context is deleted)
static void free_all(omds_ctx* ctx) {
    omds_comm_release(ctx);
    release_network(ctx);
    if (ctx->ev_in_q) (void)hipEventDestroy(ctx->ev_in_q);
    if (ctx->ev_in_means) (void)hipEventDestroy(ctx->ev_in_means);
    for (auto e : ctx->prof.start) (void)hipEventDestroy(e);
    for (auto e : ctx->prof.stop) (void)hipEventDestroy(e);
    for (hipEvent_t* e : {&ctx->ev_fork, &ctx->ev_seed, &ctx->ev_join}) {
        if (*e) (void)hipEventDestroy(*e);
        *e = nullptr;
    }
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    ctx->stream2 = nullptr;
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    ctx->stream = nullptr;
}

int omds_create(const omds_config* cfg, omds_ctx** out) {
    if (!cfg || !out) { g_create_err = "omds_create: null argument"; return OMDS_ERR_INVALID_ARG; }
    *out = nullptr;
    if (cfg->n_dof < 1 || cfg->n_dof > OMDS_MAX_DOF || cfg->n_traj < 1 || cfg->horizon < 1 || cfg->n_kernel_max < 1 ||
        cfg->max_obs < 1 || cfg->n_closest < 1 || cfg->n_closest > 64) {
        g_create_err = "omds_create: config out of range (1 <= n_dof <= 7, n_traj, horizon, n_kernel_max, max_obs >= 1, 1 <= n_closest <= 64)";
        return OMDS_ERR_INVALID_ARG;
    }
    if ((long long)cfg->n_traj * cfg->max_obs >= (1LL << 31) || (long long)cfg->n_traj * cfg->n_closest >= (1LL << 31)) {
        g_create_err = "omds_create: n_traj * max_obs (rows of the pair space) must stay below 2^31";
        return OMDS_ERR_INVALID_ARG;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = std::string("omds_create: no HIP device available (") + hipGetErrorString(e) +
                       "); this library has no CPU fallback";
        return OMDS_ERR_HIP;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_err = "omds_create: device ordinal out of range"; return OMDS_ERR_INVALID_ARG; }
    omds_ctx* ctx = new (std::nothrow) omds_ctx();
    if (!ctx) { g_create_err = "omds_create: out of host memory"; return OMDS_ERR_INVALID_ARG; }
    ctx->cfg = *cfg;
    ctx->dev = cfg->device;
    omds_default_params(&ctx->prm);
    auto fail = [&](const std::string& m, int code) {
        g_create_err = m;
        free_all(ctx);
        delete ctx;
        return code;
    };
#define CKC(expr)                                                                         \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(_e), OMDS_ERR_HIP); \
    } while (0)
    CKC(hipSetDevice(ctx->dev));
    CKC(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    const size_t N = cfg->n_traj, H = cfg->horizon, n = cfg->n_dof, Km = cfg->n_kernel_max, Om = cfg->max_obs,
                 k = cfg->n_closest, d = n + 3;
    const size_t rows2 = N * k;
    CKC(ctx->d_obs.alloc(Om * 4));
    CKC(ctx->d_A.alloc(OMDS_MAX_DOF * OMDS_MAX_DOF));
    CKC(ctx->d_Fp.alloc(std::max(Om, rows2) * OMDS_FROW));   // zeroed by omds_set_mlp (the slot assignment follows the network's d)
    CKC(ctx->d_radius.alloc(std::max(Om, rows2)));
    CKC(ctx->d_FpH.alloc(Om * 32));
    CKC(ctx->d_FqH.alloc(N * 32));
    CKC(hipMemsetAsync(ctx->d_FpH, 0, Om * 32 * 2, ctx->stream));
    CKC(hipMemsetAsync(ctx->d_FqH, 0, N * 32 * 2, ctx->stream));
    CKC(ctx->d_trajT.alloc(H * n * N));
    CKC(ctx->d_distT.alloc(H * N));
    CKC(ctx->d_dotT.alloc(H * N));
    CKC(ctx->d_actT.alloc(H * N));
    CKC(ctx->d_normalT.alloc(H * n * N));
    CKC(ctx->d_kvalT.alloc(H * Km * N));
    CKC(ctx->d_qdotT.alloc(n * N));
    CKC(ctx->d_maxact.alloc(Km * N));
    CKC(ctx->d_phisum0.alloc(Km));
    CKC(ctx->d_qstage.alloc(n * rows2));
    CKC(ctx->d_muT.alloc(Km * n * N));
    CKC(ctx->d_sigmaT.alloc(Km * N));
    CKC(ctx->d_alphaT.alloc(Km * n * N));
    CKC(ctx->d_means.alloc(Km * (2 * n + 1)));
    CKC(ctx->d_qcur.alloc(OMDS_MAX_DOF));
    CKC(ctx->d_Fq.alloc(rows2 * OMDS_FROW));
    CKC(ctx->d_Dmin.alloc(N * Om));
    CKC(ctx->d_rowlist.alloc(N * Om));
    CKC(ctx->d_listDa.alloc(N * Om));
    CKC(ctx->d_range.alloc(N * 4));
    ctx->ex_cap = (int)std::min<size_t>(N * Om, N * 32);   // 32 candidates per rollout on average; longer lists -> fp32 fallback
    CKC(ctx->d_exD.alloc((size_t)ctx->ex_cap));
    CKC(ctx->d_exDr.alloc((size_t)ctx->ex_cap));
    CKC(ctx->d_exMin.alloc((size_t)ctx->ex_cap));
    CKC(ctx->d_exMask.alloc((size_t)ctx->ex_cap * (OMDS_MAX_HIDDEN + 1) * 8));
    CKC(ctx->d_sctotal.alloc((H + 2)));
    CKC(ctx->scr.d_sinks.alloc(H));
    CKC(ctx->scr.h_sinks.alloc(H));
    CKC(ctx->d_scerr.alloc(4));
    CKC(ctx->d_idx.alloc(rows2));
    CKC(ctx->d_gradx.alloc(rows2 * d));
    CKC(ctx->d_drow.alloc(rows2));
    CKC(ctx->d_yraw.alloc(rows2 * OMDS_CPAD));
    CKC(ctx->d_minidx.alloc(rows2));
    CKC(ctx->d_dist.alloc(N));
    CKC(ctx->d_nngrad.alloc(N * n));
    CKC(ctx->d_cost.alloc(N));
    CKC(ctx->d_w.alloc(N));
    const size_t redn = std::max<size_t>((size_t)omds_red_size((int)Km, (int)n) + 8, 2 * H + 16);   // also the screening counters of a propagate (4 + 2 (H + 1))
    CKC(ctx->d_red.alloc(redn));
    CKC(ctx->h_red.alloc(redn));
    CKC(ctx->scr.h_verdict.alloc((H + 8)));
    CKC(ctx->h_in.alloc((Km * (2 * n + 1) + OMDS_MAX_DOF)));   // pinned staging of the small per-iteration inputs
    CKC(hipEventCreateWithFlags(&ctx->ev_in_q, hipEventDisableTiming));
    CKC(hipEventCreateWithFlags(&ctx->ev_in_means, hipEventDisableTiming));
    CKC(ctx->d_stage.alloc(std::max({N * H * std::max(Km, n), N * Om, Km * n * N, rows2 * OMDS_CPAD})));
    CKC(ctx->d_cflags.alloc(N * H));
    CKC(ctx->d_ccounts.alloc(N));
    CKC(ctx->d_coffsets.alloc((N + 1)));
    CKC(hipMemsetAsync(ctx->d_trajT, 0, H * n * N * 4, ctx->stream));
    CKC(hipMemsetAsync(ctx->d_kvalT, 0, H * Km * N * 4, ctx->stream));
    CKC(hipMemsetAsync(ctx->d_maxact, 0, Km * N * 4, ctx->stream));
    CKC(hipMemsetAsync(ctx->d_phisum0, 0, Km * 4, ctx->stream));
    CKC(hipStreamSynchronize(ctx->stream));
#undef CKC
    *out = ctx;
    return OMDS_OK;
}

void omds_destroy(omds_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->dev);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_all(ctx);
    delete ctx;
}

int omds_sync(omds_ctx* ctx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

#ifdef OMDS_TIMELINE
// Diagnostic build only (not in include/omds.h): phase timestamps of the last k_pass1 launch, see tools/pass1_timeline.py.
extern "C" OMDS_API int omds_timeline_fetch(omds_ctx* ctx, unsigned long long* host, int n_workgroups) {
    if (!ctx || !ctx->mlp.tl || n_workgroups > (1 << 16)) return OMDS_ERR_INVALID_ARG;
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipMemcpy(host, ctx->mlp.tl, (size_t)n_workgroups * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return OMDS_OK;
}
#endif

// The obstacle buffers grow on demand (MPPI.update_obstacles takes any obstacle count at any time, MPPI.py:347-350): everything
// sized by max_obs is re-allocated at twice the new count; the handle, the network, the policy samples, the communicator and
// the screening state survive.  Nothing of their old contents is needed: the caller is about to replace the scene.
static int grow_obstacle_capacity(omds_ctx* ctx, int n_obs) {
    const size_t N = ctx->cfg.n_traj, k = ctx->cfg.n_closest, H = ctx->cfg.horizon, n = ctx->cfg.n_dof, Km = ctx->cfg.n_kernel_max;
    // twice the new count, but never past what 32-bit pair indices allow: a count that fits is not rejected for its doubling
    const long long Omax = ((1LL << 31) - 1) / (long long)N;
    REQUIRE(n_obs <= Omax, OMDS_ERR_INVALID_ARG, "omds_set_obstacles: n_traj * n_obs must stay below 2^31");
    const size_t Om = (size_t)std::min<long long>(std::max(2LL * n_obs, 64LL), Omax), rows2 = N * k;
    CK(hipStreamSynchronize(ctx->stream));
    // Until every replacement exists the context holds NO scene: if an allocation below fails, check_ready refuses to run
    // (n_obs == 0) and the next omds_set_obstacles starts the growth again (max_obs == 0) instead of touching freed buffers
    ctx->n_obs = 0;
    ctx->cfg.max_obs = 0;
    const bool had_FpS = ctx->d_FpS != nullptr, had_horizon = ctx->d_hzFp != nullptr;
    ctx->d_obs.reset(); ctx->d_Fp.reset(); ctx->d_radius.reset(); ctx->d_FpH.reset(); ctx->d_Dmin.reset();
    ctx->d_rowlist.reset(); ctx->d_listDa.reset(); ctx->d_FpS.reset();
    ctx->d_hzVel.reset(); ctx->d_hzObs.reset(); ctx->d_hzRadius.reset(); ctx->d_hzFp.reset(); ctx->d_hzFpH.reset(); ctx->d_hzFpS.reset();
    ctx->hz_ld = 0;
    CK(ctx->d_obs.alloc(Om * 4));
    CK(ctx->d_Fp.alloc(std::max(Om, rows2) * OMDS_FROW));
    CK(hipMemsetAsync(ctx->d_Fp, 0, std::max(Om, rows2) * OMDS_FROW * 4, ctx->stream));   // the joints' slots and the padding stay zero
    CK(ctx->d_radius.alloc(std::max(Om, rows2)));
    CK(ctx->d_FpH.alloc(Om * 32));
    CK(hipMemsetAsync(ctx->d_FpH, 0, Om * 32 * 2, ctx->stream));
    CK(ctx->d_Dmin.alloc(N * Om));
    CK(ctx->d_rowlist.alloc(N * Om));
    CK(ctx->d_listDa.alloc(N * Om));
    if (had_FpS) {
        CK(ctx->d_FpS.alloc(Om * 32));
        CK(hipMemsetAsync(ctx->d_FpS, 0, Om * 32 * 2, ctx->stream));
        ctx->mlp.scrP = ctx->d_FpS;
    }
    CK(ctx->d_stage.reserve(std::max({N * H * std::max(Km, n), N * Om, Km * n * N, rows2 * OMDS_CPAD})));
    const int ex_cap = (int)std::min<size_t>(N * Om, N * 32);
    if (ex_cap > ctx->ex_cap) {
        ctx->d_exD.reset(); ctx->d_exDr.reset(); ctx->d_exMin.reset(); ctx->d_exMask.reset();
        ctx->d_exDeriv.reset();   // allocated again at the next screened tanh step
        ctx->ex_cap = 0;
        CK(ctx->d_exD.alloc((size_t)ex_cap));
        CK(ctx->d_exDr.alloc((size_t)ex_cap));
        CK(ctx->d_exMin.alloc((size_t)ex_cap));
        CK(ctx->d_exMask.alloc((size_t)ex_cap * (OMDS_MAX_HIDDEN + 1) * 8));
        ctx->ex_cap = ex_cap;
    }
    ctx->cfg.max_obs = (int)Om;
    ctx->n_obs = 0;
    if (had_horizon) { const int rc = alloc_obstacle_horizon(ctx); if (rc) return rc; }
    return OMDS_OK;
}

}  // extern "C"

int reserve_obstacle_capacity(omds_ctx* ctx, int n_obs) {
    return n_obs > ctx->cfg.max_obs ? grow_obstacle_capacity(ctx, n_obs) : OMDS_OK;
}

// What omds_set_obstacles does with a checked list xyzr [n_obs][4] in host memory (n_obs >= n_closest): omds_set_obstacles_from_cloud
// ends in the same body (scene_cloud.hip)
int install_obstacles(omds_ctx* ctx, const float* xyzr, int n_obs) {
    CK(hipSetDevice(ctx->dev));
    int rc;
    clear_obstacle_horizon(ctx);   // the new scene stands still until the caller says otherwise (omds_set_obstacle_motion / _horizon)
    ctx->focus.on = false;         // ... and is nobody's subset: any setter ends an obstacle focus (omds_focus_obstacles switches it on again)
    if (n_obs > ctx->cfg.max_obs && (rc = grow_obstacle_capacity(ctx, n_obs))) return rc;
    CK(hipMemcpyAsync(ctx->d_obs, xyzr, (size_t)n_obs * 16, hipMemcpyHostToDevice, ctx->stream));
    ctx->n_obs = n_obs;
    ctx->scr.scene_changed(xyzr, n_obs);
    ctx->obs_now.assign(xyzr, xyzr + (size_t)n_obs * 4);
    ctx->cloud.forget_labels();   // the labels of a scene belong to the objects call that installed it (scene_cloud.hip puts them back)
    if (ctx->have_mlp && !ctx->wide.on) {
        omds_launch_obstacle_features(ctx->stream, ctx->mlp, ctx->d_obs, n_obs, ctx->d_Fp, ctx->d_radius, ctx->d_FpH, ctx->cfg.max_obs);
        CK(hipGetLastError());
    }
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

// The SEDS components as the step reads them (omds_internal.h: StepArgs::seds), one record of omds_seds_stride(n) floats each
std::vector<float> omds_pack_seds(int n, int G, const float* mu_in, const float* b, const float* sigma_inv, const float* A,
                                  const float* prior, const float* den) {
    const int st = omds_seds_stride(n);
    std::vector<float> pk((size_t)G * st);
    for (int j = 0; j < G; ++j) {
        float* p = &pk[(size_t)j * st];
        std::memcpy(p, mu_in + (size_t)j * n, n * sizeof(float));
        std::memcpy(p + n, b + (size_t)j * n, n * sizeof(float));
        p[2 * n] = prior[j];
        p[2 * n + 1] = den[j];
        std::memcpy(p + 2 * n + 2, sigma_inv + (size_t)j * n * n, (size_t)n * n * sizeof(float));
        std::memcpy(p + 2 * n + 2 + n * n, A + (size_t)j * n * n, (size_t)n * n * sizeof(float));
    }
    return pk;
}

extern "C" {

int omds_set_obstacles(omds_ctx* ctx, const float* xyzr, int n_obs) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(xyzr && n_obs >= 1, OMDS_ERR_INVALID_ARG, "omds_set_obstacles: need n_obs >= 1 and a non-null [O,4] array");
    REQUIRE(n_obs >= ctx->cfg.n_closest, OMDS_ERR_INVALID_ARG, "omds_set_obstacles: fewer obstacles than n_closest");
    return install_obstacles(ctx, xyzr, n_obs);
}

int omds_get_obstacles(omds_ctx* ctx, float* xyzr, int32_t* n_obs_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (n_obs_out) *n_obs_out = ctx->n_obs;
    if (xyzr && ctx->n_obs > 0) std::memcpy(xyzr, ctx->obs_now.data(), (size_t)ctx->n_obs * 16);
    return OMDS_OK;
}

static void refresh_goal_fk(omds_ctx* ctx) {
    if (ctx->have_ds && ctx->have_cost) omds_host_link_endpoints(ctx->qf, ctx->dh, ctx->cfg.n_dof, ctx->goal_fk);
}

int omds_set_ds(omds_ctx* ctx, const float* q_goal) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(q_goal, OMDS_ERR_INVALID_ARG, "omds_set_ds: null q_goal");
    std::memcpy(ctx->qf, q_goal, ctx->cfg.n_dof * sizeof(float));
    ctx->have_ds = true;
    ctx->have_A = false;
    ctx->seds_G = 0;
    refresh_goal_fk(ctx);
    return OMDS_OK;
}

int omds_set_ds_matrix(omds_ctx* ctx, const float* q_goal, const float* A) {
    int rc = omds_set_ds(ctx, q_goal);
    if (rc || !A) return rc;
    const int n = ctx->cfg.n_dof;
    CK(hipSetDevice(ctx->dev));
    CK(hipMemcpy(ctx->d_A, A, (size_t)n * n * sizeof(float), hipMemcpyHostToDevice));
    ctx->have_A = true;
    return OMDS_OK;
}

int omds_set_ds_seds(omds_ctx* ctx, const float* q_goal, int G, const float* mu_in, const float* b, const float* sigma_inv,
                     const float* A, const float* prior, const float* den, float lin_thr, float seds_thr) {
    int rc = omds_set_ds(ctx, q_goal);
    if (rc || G == 0) return rc;
    REQUIRE(G >= 1 && G <= 64 && mu_in && b && sigma_inv && A && prior && den, OMDS_ERR_INVALID_ARG,
            "omds_set_ds_seds: need 1 <= n_gauss <= 64 and non-null component arrays");
    const std::vector<float> pk = omds_pack_seds(ctx->cfg.n_dof, G, mu_in, b, sigma_inv, A, prior, den);
    CK(hipSetDevice(ctx->dev));
    CK(hipStreamSynchronize(ctx->stream));
    CK(ctx->d_seds.alloc(pk.size()));
    CK(hipMemcpy(ctx->d_seds, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->seds_G = G;
    ctx->seds_lin_thr = lin_thr;
    ctx->seds_thr = seds_thr;
    return OMDS_OK;
}

int omds_set_params(omds_ctx* ctx, const omds_params* p) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(p, OMDS_ERR_INVALID_ARG, "omds_set_params: null params");
    REQUIRE(p->rbf_p > 0.f, OMDS_ERR_INVALID_ARG, "omds_set_params: rbf_p must be positive");
    REQUIRE((p->cost_terms & ~OMDS_COST_ALL) == 0 && (p->variant & ~3u) == 0, OMDS_ERR_INVALID_ARG,
            "omds_set_params: unknown bits in cost_terms / variant");
    if (p->ignored_links != ctx->prm.ignored_links) ctx->scr.links_changed();
    ctx->prm = *p;
    return OMDS_OK;
}

int omds_set_cost(omds_ctx* ctx, const float* dh_params, const float* q_min, const float* q_max) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(dh_params && q_min && q_max, OMDS_ERR_INVALID_ARG, "omds_set_cost: null argument");
    const int n = ctx->cfg.n_dof;
    std::memcpy(ctx->dh, dh_params, (size_t)(n + 1) * 4 * sizeof(float));
    std::memcpy(ctx->qmin, q_min, n * sizeof(float));
    std::memcpy(ctx->qmax, q_max, n * sizeof(float));
    ctx->have_cost = true;
    refresh_goal_fk(ctx);
    return OMDS_OK;
}

// ---- policy samples -------------------------------------------------------------------------------
int omds_set_policy_samples(omds_ctx* ctx, const float* mu, const float* sigma, const float* alpha, int K) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(K >= 0 && K <= ctx->cfg.n_kernel_max, OMDS_ERR_INVALID_ARG, "omds_set_policy_samples: 0 <= n_kernels <= n_kernel_max");
    CK(hipSetDevice(ctx->dev));
    ctx->n_kernels = K;
    if (K == 0) return OMDS_OK;
    REQUIRE(mu && sigma && alpha, OMDS_ERR_INVALID_ARG, "omds_set_policy_samples: null sample array");
    const int N = ctx->cfg.n_traj, n = ctx->cfg.n_dof;
    CK(hipMemcpyAsync(ctx->d_stage, mu, (size_t)N * K * n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_muT, N, K * n);
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipMemcpyAsync(ctx->d_stage, alpha, (size_t)N * K * n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_alphaT, N, K * n);
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipMemcpyAsync(ctx->d_stage, sigma, (size_t)N * K * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_sigmaT, N, K);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

int omds_sample_policy(omds_ctx* ctx, const float* mu_c, const float* sigma_c, const float* alpha_c, float mu_s,
                       float sigma_s, float alpha_s, int K, uint64_t seed, int64_t rollout_offset) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(K >= 0 && K <= ctx->cfg.n_kernel_max, OMDS_ERR_INVALID_ARG, "omds_sample_policy: 0 <= n_kernels <= n_kernel_max");
    CK(hipSetDevice(ctx->dev));
    ctx->n_kernels = K;
    if (K == 0) return OMDS_OK;
    REQUIRE(mu_c && sigma_c && alpha_c, OMDS_ERR_INVALID_ARG, "omds_sample_policy: null mean array");
    const int N = ctx->cfg.n_traj, n = ctx->cfg.n_dof;
    // through pinned staging: no stream synchronisation here.  The staging is normally rewritten one planner iteration later,
    // behind the synchronisations of omds_propagate and the update; the event covers back-to-back calls
    CK(hipEventSynchronize(ctx->ev_in_means));
    float* means = ctx->h_in + OMDS_MAX_DOF;
    std::memcpy(means, mu_c, (size_t)K * n * 4);
    std::memcpy(means + (size_t)K * n, sigma_c, (size_t)K * 4);
    std::memcpy(means + (size_t)K * n + K, alpha_c, (size_t)K * n * 4);
    CK(hipMemcpyAsync(ctx->d_means, means, (size_t)K * (2 * n + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipEventRecord(ctx->ev_in_means, ctx->stream));
    omds_launch_sample(ctx->stream, N, n, K, ctx->d_means, mu_s, sigma_s, alpha_s, seed, rollout_offset, ctx->d_muT,
                       ctx->d_sigmaT, ctx->d_alphaT);
    CK(hipGetLastError());
    return OMDS_OK;
}

int omds_get_policy_samples(omds_ctx* ctx, float* mu, float* sigma, float* alpha) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CK(hipSetDevice(ctx->dev));
    const int N = ctx->cfg.n_traj, n = ctx->cfg.n_dof, K = ctx->n_kernels;
    if (K == 0) return OMDS_OK;
    if (mu) {
        omds_launch_transpose(ctx->stream, ctx->d_muT, ctx->d_stage, K * n, N);
        CK(hipMemcpyAsync(mu, ctx->d_stage, (size_t)N * K * n * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    if (alpha) {
        omds_launch_transpose(ctx->stream, ctx->d_alphaT, ctx->d_stage, K * n, N);
        CK(hipMemcpyAsync(alpha, ctx->d_stage, (size_t)N * K * n * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    if (sigma) {
        omds_launch_transpose(ctx->stream, ctx->d_sigmaT, ctx->d_stage, K, N);
        CK(hipMemcpyAsync(sigma, ctx->d_stage, (size_t)N * K * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

// ---- measurement -------------------------------------------------------------------------------------
int omds_prof_enable(omds_ctx* ctx, int on) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    ctx->prof_on = on != 0;
    ctx->prof_stride = on > 1 ? on : 1;
    return OMDS_OK;
}
int omds_prof_reset(omds_ctx* ctx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    ctx->prof.ms = 0.0;
    ctx->prof_seen = 0;
    ctx->prof.launches = 0;
    ctx->prof.rows = 0;
    ctx->prof.flops = 0.0;
    ctx->prof.used = 0;
    ctx->scr.reset_stats();
    return OMDS_OK;
}
int omds_prof_read_ex(omds_ctx* ctx, double* ms, int64_t* launches, double* flops, const char** kernel) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    { const int rc = prof_collect(ctx); if (rc) return rc; }
    if (ms) *ms = ctx->prof.ms;
    if (launches) *launches = ctx->prof.launches;
    if (flops) *flops = ctx->prof.flops;
    if (kernel) *kernel = ctx->prof.kernel;
    return OMDS_OK;
}
int omds_prof_read(omds_ctx* ctx, double* pass1_ms, int64_t* pass1_launches, int64_t* pass1_rows) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    { const int rc = prof_collect(ctx); if (rc) return rc; }
    if (pass1_ms) *pass1_ms = ctx->prof.ms;
    if (pass1_launches) *pass1_launches = ctx->prof.launches;
    if (pass1_rows) *pass1_rows = ctx->prof.rows;
    return OMDS_OK;
}

}  // extern "C"
