// Cost, the cost-weighted policy update and the navigation-kernel candidates: omds_cost(_eval), omds_cost_sum, omds_local_sums,
// omds_apply_update, omds_weighted_update(_eval), omds_get_qdot, omds_kernel_candidates.
#include "capi_internal.h"

extern "C" {

// ---- cost and the cost-weighted update --------------------------------------------------------------
static int enqueue_cost(omds_ctx* ctx) {
    CostArgs a{};
    a.N = ctx->cfg.n_traj; a.H = ctx->cfg.horizon; a.n = ctx->cfg.n_dof;
    a.trajT = ctx->d_trajT; a.distT = ctx->d_distT; a.cost = ctx->d_cost;
    a.terms = ctx->prm.cost_terms;
    std::memcpy(a.qf, ctx->qf, sizeof(a.qf));
    std::memcpy(a.qmin, ctx->qmin, sizeof(a.qmin));
    std::memcpy(a.qmax, ctx->qmax, sizeof(a.qmax));
    std::memcpy(a.dh, ctx->dh, sizeof(a.dh));
    std::memcpy(a.goal_fk, ctx->goal_fk, sizeof(a.goal_fk));
    omds_launch_cost(ctx->stream, a);
    CK(hipGetLastError());
    ctx->have_cost_vals = true;
    return OMDS_OK;
}

int omds_cost(omds_ctx* ctx, float* cost_out) {
    RoctxRange range("TAG: cost calculation");
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->have_ds && ctx->have_cost, OMDS_ERR_NOT_INITIALISED, "omds_cost: call omds_set_ds and omds_set_cost first");
    CK(hipSetDevice(ctx->dev));
    int rc;
    if ((rc = enqueue_cost(ctx))) return rc;
    if (cost_out) {
        CK(hipMemcpyAsync(cost_out, ctx->d_cost, (size_t)ctx->cfg.n_traj * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

// Cost.evaluate_costs on caller-supplied tensors (cost.py:13-22 evaluates exactly its arguments): all_traj [B,H,n],
// closest_dist_all [B,H] in the reference layout, B <= n_traj.  The device rollouts of the context are not touched.
int omds_cost_eval(omds_ctx* ctx, const float* all_traj, const float* closest_dist_all, int B, float* cost_out) {
    RoctxRange range("TAG: cost calculation");
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(all_traj && closest_dist_all && cost_out && B >= 1 && B <= ctx->cfg.n_traj, OMDS_ERR_INVALID_ARG,
            "omds_cost_eval: need 1 <= batch <= n_traj and non-null arrays");
    REQUIRE(ctx->have_ds && ctx->have_cost, OMDS_ERR_NOT_INITIALISED, "omds_cost_eval: call omds_set_ds and omds_set_cost first");
    CK(hipSetDevice(ctx->dev));
    const size_t H = ctx->cfg.horizon, n = ctx->cfg.n_dof, N = ctx->cfg.n_traj;
    CK(ctx->d_evalT.reserve(H * n * N + H * N + N));
    float* trajT = ctx->d_evalT;                 // [H][n][B]
    float* distT = trajT + H * n * N;            // [H][B]
    float* costv = distT + H * N;                // [B]
    CK(hipMemcpyAsync(ctx->d_stage, all_traj, (size_t)B * H * n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, trajT, B, (int)(H * n));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipMemcpyAsync(ctx->d_stage, closest_dist_all, (size_t)B * H * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, distT, B, (int)H);
    CostArgs a{};
    a.N = B; a.H = (int)H; a.n = (int)n;
    a.trajT = trajT; a.distT = distT; a.cost = costv;
    a.terms = ctx->prm.cost_terms;
    std::memcpy(a.qf, ctx->qf, sizeof(a.qf));
    std::memcpy(a.qmin, ctx->qmin, sizeof(a.qmin));
    std::memcpy(a.qmax, ctx->qmax, sizeof(a.qmax));
    std::memcpy(a.dh, ctx->dh, sizeof(a.dh));
    std::memcpy(a.goal_fk, ctx->goal_fk, sizeof(a.goal_fk));
    omds_launch_cost(ctx->stream, a);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(cost_out, costv, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

// Local [sum(cost), N] of this shard.
int omds_cost_sum(omds_ctx* ctx, float* out2) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(out2, OMDS_ERR_INVALID_ARG, "omds_cost_sum: null output");
    REQUIRE(ctx->have_cost_vals, OMDS_ERR_NOT_INITIALISED, "no cost available: call omds_cost after omds_propagate");
    CK(hipSetDevice(ctx->dev));
    const int rs = omds_red_size(ctx->n_kernels, ctx->cfg.n_dof);
    float* red2 = ctx->d_red + rs;  // [sum cost, N] lives behind the packed buffer
    omds_launch_cost_sum(ctx->stream, ctx->d_cost, ctx->cfg.n_traj, red2);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(ctx->h_red + rs, red2, 8, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    out2[0] = ctx->h_red[rs];
    out2[1] = ctx->h_red[rs + 1];
    return OMDS_OK;
}

int omds_red_count(const omds_ctx* ctx) { return ctx ? omds_red_size(ctx->n_kernels, ctx->cfg.n_dof) : 0; }

// Packed partial sums of this shard for the GLOBAL beta = (sum_cost / n_total) / 50.
int omds_local_sums(omds_ctx* ctx, float sum_cost, float n_total, int include_rollout0, float* red_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(red_out && n_total > 0.f, OMDS_ERR_INVALID_ARG, "omds_local_sums: null output or n_total <= 0");
    REQUIRE(ctx->have_cost_vals, OMDS_ERR_NOT_INITIALISED, "no cost available: call omds_cost after omds_propagate");
    CK(hipSetDevice(ctx->dev));
    const int N = ctx->cfg.n_traj, n = ctx->cfg.n_dof, K = ctx->n_kernels;
    const int rs = omds_red_size(K, n);
    float* red2 = ctx->d_red + rs;
    ctx->h_red[rs] = sum_cost;
    ctx->h_red[rs + 1] = n_total;
    CK(hipMemcpyAsync(red2, ctx->h_red + rs, 8, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_weights(ctx->stream, ctx->d_cost, N, red2, ctx->d_w, nullptr);
    omds_launch_policy_sums(ctx->stream, N, n, K, ctx->d_w, ctx->d_muT, ctx->d_sigmaT, ctx->d_alphaT, ctx->d_maxact,
                            ctx->d_phisum0, ctx->d_qdotT, ctx->d_cost, include_rollout0, ctx->d_red);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(ctx->h_red, ctx->d_red, (size_t)rs * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    std::memcpy(red_out, ctx->h_red, (size_t)rs * 4);
    return OMDS_OK;
}

// Pure host arithmetic, no context: masks + theta_c update from the (globally) reduced buffer.
int omds_apply_update(int K, int n, int H, const float* red, float n_total, float rate, float ker_thr, uint32_t variant,
                      float* mu_c, float* sigma_c, float* alpha_c, int32_t* mask_out) {
    if (K < 0 || n < 1 || H < 1 || !red || n_total <= 0.f) return OMDS_ERR_INVALID_ARG;
    if (K > 0 && (!mu_c || !sigma_c || !alpha_c)) return OMDS_ERR_INVALID_ARG;
    const float sumw = red[0];
    const float *s_mu = red + 1, *s_sg = s_mu + K * n, *s_al = s_sg + K, *s_mx = s_al + K * n, *s_ph = s_mx + K;
    for (int kk = 0; kk < K; ++kk) {
        // mask 1: mean over ALL rollouts of max_h(phi*act) > ker_thr; mask 2: mean_h phi of rollout 0 (MPPI.py:336-342)
        const float m1 = s_mx[kk] / n_total, m2 = s_ph[kk] / (float)H;
        const bool upd = (m1 > ker_thr) && ((variant & OMDS_VARIANT_NO_BASE_MASK) || (m2 > ker_thr));   // NaN compares false, like torch
        if (mask_out) mask_out[kk] = upd ? 1 : 0;
        const float u = upd ? rate : 0.f;
        for (int j = 0; j < n; ++j) {
            mu_c[kk * n + j] = (1.f - u) * mu_c[kk * n + j] + u * (s_mu[kk * n + j] / sumw);
            alpha_c[kk * n + j] = (1.f - u) * alpha_c[kk * n + j] + u * (s_al[kk * n + j] / sumw);
        }
        sigma_c[kk] = (1.f - u) * sigma_c[kk] + u * (s_sg[kk] / sumw);
    }
    return OMDS_OK;
}

int omds_weighted_update(omds_ctx* ctx, float rate, float ker_thr, float* mu_c, float* sigma_c, float* alpha_c,
                         int32_t* mask_out, float* weights_out) {
    RoctxRange range("shift_policy_means");
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    int rc;
    if ((rc = omds_update_impl(ctx, false, rate, ker_thr, mu_c, sigma_c, alpha_c, mask_out, nullptr, nullptr, nullptr))) return rc;
    if (weights_out) {
        const int N = ctx->cfg.n_traj;
        std::vector<float> w(N);
        CK(hipMemcpy(w.data(), ctx->d_w, (size_t)N * 4, hipMemcpyDeviceToHost));
        for (int t = 0; t < N; ++t) weights_out[t] = w[t] / ctx->h_red[0];
    }
    return OMDS_OK;
}

// MPPI.shift_policy_means + TensorPolicyMPPI.update_policy (MPPI.py:331-345, policy.py:88-113) on caller-supplied tensors, the way
// omds_cost_eval serves Cost.evaluate_costs: cost [N], kernel_val_all [N,H,K], kernel_activations [N,H] in the reference layouts, against
// the policy samples the context holds.  The context's own rollouts, cost values and running maxima are not touched.
int omds_weighted_update_eval(omds_ctx* ctx, const float* cost, const float* kernel_val_all, const float* kernel_activations, float rate,
                              float ker_thr, float* mu_c, float* sigma_c, float* alpha_c, int32_t* mask_out, float* weights_out) {
    RoctxRange range("shift_policy_means");
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const int N = ctx->cfg.n_traj, H = ctx->cfg.horizon, n = ctx->cfg.n_dof, K = ctx->n_kernels, Km = ctx->cfg.n_kernel_max;
    REQUIRE(cost && kernel_activations && (K == 0 || (kernel_val_all && mu_c && sigma_c && alpha_c)), OMDS_ERR_INVALID_ARG,
            "omds_weighted_update_eval: null argument");
    CK(hipSetDevice(ctx->dev));
    CK(ctx->d_uev.reserve((size_t)N + (size_t)Km * N + Km + (size_t)N * H));
    float* d_costv = ctx->d_uev;
    float* d_maxact = d_costv + N;
    float* d_phisum0 = d_maxact + (size_t)Km * N;
    float* d_act = d_phisum0 + Km;
    CK(hipMemcpyAsync(d_costv, cost, (size_t)N * 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(d_act, kernel_activations, (size_t)N * H * 4, hipMemcpyHostToDevice, ctx->stream));
    if (K > 0) {
        CK(hipMemcpyAsync(ctx->d_stage, kernel_val_all, (size_t)N * H * K * 4, hipMemcpyHostToDevice, ctx->stream));   // d_stage holds >= N*H*Kmax floats
        omds_launch_update_inputs(ctx->stream, ctx->d_stage, d_act, N, H, K, (ctx->prm.variant & OMDS_VARIANT_KVAL_TIMES_ACT) ? 1 : 0, d_maxact, d_phisum0);
    }
    const int rs = omds_red_size(K, n);
    float* red2 = ctx->d_red + rs;
    omds_launch_cost_sum(ctx->stream, d_costv, N, red2);
    omds_launch_weights(ctx->stream, d_costv, N, red2, ctx->d_w, nullptr);
    omds_launch_policy_sums(ctx->stream, N, n, K, ctx->d_w, ctx->d_muT, ctx->d_sigmaT, ctx->d_alphaT, d_maxact, d_phisum0, ctx->d_qdotT, d_costv, 1, ctx->d_red);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(ctx->h_red, ctx->d_red, (size_t)(rs + 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const int rc = omds_apply_update(K, n, H, ctx->h_red, ctx->h_red[rs + 1], rate, ker_thr, ctx->prm.variant, mu_c, sigma_c, alpha_c, mask_out);
    if (rc) { ctx->err = "omds_apply_update: invalid argument"; return rc; }
    if (weights_out) {
        std::vector<float> w(N);
        CK(hipMemcpy(w.data(), ctx->d_w, (size_t)N * 4, hipMemcpyDeviceToHost));
        for (int t = 0; t < N; ++t) weights_out[t] = w[t] / ctx->h_red[0];
    }
    return OMDS_OK;
}

int omds_get_qdot(omds_ctx* ctx, int mode, float* out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(out && (mode == 0 || mode == 1), OMDS_ERR_INVALID_ARG, "omds_get_qdot: mode 0 ('best') or 1 ('weighted'), non-null out");
    // the sums of this shard only (means untouched: rate 0 on null arrays is not allowed, so run the reduction alone)
    int rc;
    float cs[2];
    if ((rc = omds_cost_sum(ctx, cs))) return rc;
    const int n = ctx->cfg.n_dof, K = ctx->n_kernels;
    std::vector<float> red(omds_red_size(K, n));
    if ((rc = omds_local_sums(ctx, cs[0], cs[1], 1, red.data()))) return rc;
    const int o_qd = 1 + K * (2 * n + 3), o_best = o_qd + n;
    for (int j = 0; j < n; ++j) out[j] = mode == 1 ? red[o_qd + j] / red[0] : red[o_best + 1 + j];
    return OMDS_OK;
}

// ---- navigation-kernel candidates (policy.py:153-175) --------------------------------------------------
int omds_kernel_candidates(omds_ctx* ctx, float thr_dist, float thr_kernel, float thr_dot, const float* mu_c,
                           const float* sigma_c, int K, int cap, float* cand_q, int32_t* cand_th, int32_t* count) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(count && cap >= 0 && K >= 0 && K <= ctx->cfg.n_kernel_max, OMDS_ERR_INVALID_ARG,
            "omds_kernel_candidates: bad arguments");
    REQUIRE(K == 0 || (mu_c && sigma_c), OMDS_ERR_INVALID_ARG, "omds_kernel_candidates: null kernel means");
    REQUIRE(cap == 0 || (cand_q && cand_th), OMDS_ERR_INVALID_ARG, "omds_kernel_candidates: null output with cap > 0");
    CK(hipSetDevice(ctx->dev));
    const int N = ctx->cfg.n_traj, H = ctx->cfg.horizon, n = ctx->cfg.n_dof;
    const size_t need = (size_t)cap * n * 4 + (size_t)cap * 8;
    REQUIRE(need <= ctx->d_stage.bytes(), OMDS_ERR_INVALID_ARG, "omds_kernel_candidates: cap too large for the staging buffer (<= N*H)");
    if (K > 0) {
        std::vector<float> means((size_t)K * (n + 1));
        std::memcpy(means.data(), mu_c, (size_t)K * n * 4);
        std::memcpy(means.data() + (size_t)K * n, sigma_c, (size_t)K * 4);
        CK(hipMemcpyAsync(ctx->d_means, means.data(), means.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    float* d_q = ctx->d_stage;
    int* d_th = reinterpret_cast<int*>(ctx->d_stage + (size_t)cap * n);
    omds_launch_candidates(ctx->stream, N, H, n, K, ctx->d_trajT, ctx->d_distT, ctx->d_dotT, ctx->d_means, thr_dist,
                           thr_kernel, thr_dot, ctx->prm.rbf_p, ctx->d_cflags, ctx->d_ccounts, ctx->d_coffsets, cap, d_q, d_th);
    CK(hipGetLastError());
    int32_t total = 0;
    CK(hipMemcpyAsync(&total, ctx->d_coffsets + N, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    *count = total;
    const int m = std::min<int>(total, cap);
    if (m > 0) {
        CK(hipMemcpyAsync(cand_q, d_q, (size_t)m * n * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(cand_th, d_th, (size_t)m * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

}  // extern "C"
