// Installing the distance network (fused MFMA packs, or the raw weights of a network wider than 256) and evaluating it on
// batches: omds_set_mlp(_ex), omds_dist_grad, omds_mlp_forward_vjp / omds_mlp_jacobian, omds_pass1_skip_stats.
#include "capi_internal.h"

// omds_ctx::mlp_allocs owns every device array MlpDev, ScreenDev and WideNet point to
void release_network(omds_ctx* ctx) {
    for (void* p : ctx->mlp_allocs)
        if (p) (void)hipFree(p);
    ctx->mlp_allocs.clear();
}

// The installed network goes, fused or wide, with everything that was derived from it; what the screening controller measured
// on it is forgotten.  Both install paths start here, once nothing can reject the call any more.
static int drop_network(omds_ctx* ctx) {
    CK(hipSetDevice(ctx->dev));
    CK(hipStreamSynchronize(ctx->stream));
    release_network(ctx);
    ctx->have_mlp = false;
    ctx->wide = WideNet{};
    ctx->screen = ScreenDev{};
    ctx->d_dscr.reset();
    ctx->d_exDeriv.reset();
    ctx->scr.reset_for_new_network();
    return OMDS_OK;
}

// ---- distance network on a batch: Fq -> pass 1 -> top-k -> pass 2 ---------------------------------
int enqueue_network(omds_ctx* ctx, const float* qT, int ldq, int B, const ObsTables& t) {
    const MlpDev& m = ctx->mlp;
    const int O = ctx->n_obs, k = ctx->cfg.n_closest;
    if (ctx->wide.on) {   // a hidden layer wider than 256: the unfused GEMM path (wide_kernels.hip)
        int rcw;
        if ((rcw = prof_begin(ctx))) return rcw;
        if ((rcw = omds_wide_network(ctx, qT, ldq, B))) return rcw;
        if ((rcw = prof_end(ctx, (int64_t)B * O, (double)B * O * ctx->f_fwd + (double)B * k * (ctx->f_fwd + ctx->f_bwd), "k_gemm (wide network)"))) return rcw;
        CK(hipGetLastError());
        return OMDS_OK;
    }
    omds_launch_rollout_features(ctx->stream, m, qT, ldq, B, ctx->d_Fq);
    int rc;
    if (small_step_wanted(ctx)) {   // the arithmetic the step of this context uses: the batch entry point reproduces it bit for bit
        if ((rc = prof_begin(ctx))) return rc;
        omds_launch_net_small(ctx->stream, m, t.Fp, t.radius, t.obs, ctx->d_Fq, O, ctx->prm.ignored_links,
                              ctx->cfg.n_dof, k, qT, ldq, B, ctx->d_gradx, ctx->d_drow, ctx->d_idx, ctx->d_Dmin);
        if ((rc = prof_end(ctx, (int64_t)B * O, (double)B * O * ctx->f_fwd + (double)B * k * ctx->f_bwd, "k_step_small"))) return rc;
        CK(hipGetLastError());
        return OMDS_OK;
    }
    if ((rc = prof_begin(ctx))) return rc;
    omds_launch_pass1(ctx->stream, m, ctx->d_Fq, t.Fp, t.radius, O, B, ctx->prm.ignored_links, ctx->d_Dmin);
    if ((rc = prof_end(ctx, (int64_t)B * O))) return rc;
    omds_launch_topk(ctx->stream, ctx->d_Dmin, B, O, k, ctx->d_idx);
    omds_launch_pass2(ctx->stream, m, ctx->d_Fq, t.Fp, t.radius, t.obs, ctx->d_idx, B, k, qT, ldq,
                      ctx->d_gradx, ctx->d_drow, nullptr, nullptr, ctx->d_dscr);
    CK(hipGetLastError());
    return OMDS_OK;
}

extern "C" {

// ---- weights -------------------------------------------------------------------------------------

int omds_set_mlp(omds_ctx* ctx, int n_linear, const int32_t* dims, const float* const* W, const float* const* b, int act,
                 float out_div) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(dims && n_linear >= 2, OMDS_ERR_INVALID_ARG, "omds_set_mlp: null argument or fewer than 2 Linear layers");
    return omds_set_mlp_ex(ctx, n_linear, dims, dims + 1, W, b, act, out_div, 0, nullptr);
}

// A network with a hidden layer wider than the fused kernels' 256 columns (MLPRegression is width-agnostic,
// network_macros_mod.py:96-135): raw weights on the device and the buffers of the unfused GEMM path (wide_kernels.hip).
static int set_mlp_wide(omds_ctx* ctx, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W,
                        const float* const* b, int act, float out_div, int n_skips) {
    const int n = ctx->cfg.n_dof;
    int rc;
    REQUIRE(n_skips == 0, OMDS_ERR_UNSUPPORTED, "omds_set_mlp_ex: skip concatenations are supported for hidden widths <= 256 only");
    if ((rc = check_mlp_args(n, n_linear, in_dims, out_dims, W, b, act, out_div, ctx->err))) return rc;
    const int d = in_dims[0] / 3, C = out_dims[n_linear - 1];
    int wmax = in_dims[0];
    for (int i = 0; i < n_linear; ++i) {
        REQUIRE(out_dims[i] >= 1 && out_dims[i] <= 4096, OMDS_ERR_UNSUPPORTED, "omds_set_mlp: layer widths above 4096 are not supported");
        REQUIRE(i == 0 || in_dims[i] == out_dims[i - 1], OMDS_ERR_INVALID_ARG,
                "omds_set_mlp: the input width of a Linear layer must be the previous output width");
        wmax = std::max(wmax, (int)out_dims[i]);
    }
    if ((rc = drop_network(ctx))) return rc;
    WideNet w;
    w.on = true;
    w.d = d; w.act = act; w.out_div = out_div;
    w.dims.assign(1, in_dims[0]);
    for (int i = 0; i < n_linear; ++i) w.dims.push_back(out_dims[i]);
    auto dalloc = [&](float** p, size_t floats) -> int {
        void* q = nullptr;
        CK(hipMalloc(&q, floats * sizeof(float)));
        ctx->mlp_allocs.push_back(q);
        *p = static_cast<float*>(q);
        return OMDS_OK;
    };
    for (int i = 0; i < n_linear; ++i) {
        float *dw = nullptr, *db = nullptr;
        const size_t nw = (size_t)in_dims[i] * out_dims[i];
        if ((rc = dalloc(&dw, nw)) || (rc = dalloc(&db, out_dims[i]))) return rc;
        CK(hipMemcpy(dw, W[i], nw * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(db, b[i], (size_t)out_dims[i] * 4, hipMemcpyHostToDevice));
        w.W.push_back(dw);
        w.b.push_back(db);
    }
    // pass 1 in chunks of ~256 MB per activation buffer; pass 2 keeps every layer's activation of its n_traj * n_closest rows
    const long long pairs = (long long)ctx->cfg.n_traj * ctx->cfg.max_obs;
    w.chunk_rows = (int)std::min<long long>(pairs, std::max<long long>(8192, std::min<long long>(262144, (1LL << 26) / wmax)));
    w.rows2 = ctx->cfg.n_traj * ctx->cfg.n_closest;
    if ((rc = dalloc(&w.X, (size_t)w.chunk_rows * in_dims[0])) || (rc = dalloc(&w.H[0], (size_t)w.chunk_rows * wmax)) ||
        (rc = dalloc(&w.H[1], (size_t)w.chunk_rows * wmax)) || (rc = dalloc(&w.X2, (size_t)w.rows2 * in_dims[0])) ||
        (rc = dalloc(&w.G[0], (size_t)w.rows2 * wmax)) || (rc = dalloc(&w.G[1], (size_t)w.rows2 * wmax)))
        return rc;
    for (int i = 0; i < n_linear; ++i) {
        float* a = nullptr;
        if ((rc = dalloc(&a, (size_t)w.rows2 * out_dims[i]))) return rc;
        w.A.push_back(a);
    }
    MlpDev m{};   // the fields the stand-alone kernels around the network read (k_modulate, k_blend, the cost)
    m.nhh = n_linear - 2; m.C = C; m.d = d; m.n_dof = n; m.out_div = out_div; m.act = act;
    ctx->mlp = m;
    ctx->wide = w;
    ctx->act = act;
    ctx->f_fwd = 0.0;
    for (int i = 0; i < n_linear; ++i) ctx->f_fwd += 2.0 * in_dims[i] * out_dims[i];
    ctx->f_bwd = ctx->f_fwd - 2.0 * in_dims[n_linear - 1] * out_dims[n_linear - 1];
    ctx->have_mlp = true;
    obstacle_horizon_network_changed(ctx);
    return OMDS_OK;
}

int omds_set_mlp_ex(omds_ctx* ctx, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W,
                    const float* const* b, int act, float out_div, int n_skips, const int32_t* skip_after) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const int n = ctx->cfg.n_dof;
    if (in_dims && out_dims && W && b && n_linear >= 2 && n_linear <= OMDS_MAX_HIDDEN + 1) {
        bool is_wide = false;
        for (int i = 0; i + 1 < n_linear; ++i) is_wide = is_wide || out_dims[i] > OMDS_WIDTH;
        if (is_wide) return set_mlp_wide(ctx, n_linear, in_dims, out_dims, W, b, act, out_div, n_skips);
    }
    // everything that can reject the call happens before the context is touched: a rejected network (bad act, bad dims, null W)
    // leaves the previous one -- fused or wide -- installed and usable
    MlpPacks pk;
    int rc;
    if ((rc = build_mlp_packs(n, n_linear, in_dims, out_dims, W, b, act, out_div, n_skips, skip_after, pk, ctx->err))) return rc;
    const int nhid = n_linear - 1;
    const uint32_t skip_mask = pk.skip_mask;
    if ((rc = drop_network(ctx))) return rc;
    MlpDev m{};
    m.nhh = pk.nhh;
    m.C = pk.C;
    m.d = pk.d;
    m.n_dof = n;
    m.out_div = out_div;
    m.act = act;
    m.skip_mask = skip_mask;
    std::memcpy(m.skip_col, pk.skip_col, sizeof(m.skip_col));
    {   // the encoded-input tables keep zeros in the slots the other operand owns and in the padding; the slot assignment follows d
        const size_t rows2 = (size_t)ctx->cfg.n_traj * ctx->cfg.n_closest, rowsB = std::max((size_t)ctx->cfg.max_obs, rows2);
        CK(hipMemsetAsync(ctx->d_Fq, 0, rows2 * OMDS_FROW * 4, ctx->stream));
        CK(hipMemsetAsync(ctx->d_Fp, 0, rowsB * OMDS_FROW * 4, ctx->stream));
        if (ctx->d_FqAll) CK(hipMemsetAsync(ctx->d_FqAll, 0, (size_t)ctx->cfg.n_traj * ctx->cfg.horizon * OMDS_FROW * 4, ctx->stream));
        if (ctx->d_vjp_B) CK(hipMemsetAsync(ctx->d_vjp_B, 0, ctx->d_vjp_B.bytes(), ctx->stream));
    }
    if (act == OMDS_ACT_TANH) {   // pass 2 keeps 1 - h^2 of every hidden layer for the backward (ReLU uses LDS bit masks)
        const size_t rows = std::max(((size_t)ctx->cfg.n_traj * ctx->cfg.n_closest + 31) / 32 * 32,
                                     (size_t)omds_tail_scratch_rows(ctx->cfg.n_traj, ctx->cfg.n_closest));
        CK(ctx->d_dscr.alloc((size_t)nhid * rows * OMDS_WIDTH));
        // the screened step's hand-over: the same derivatives for every candidate k_exact evaluates (1 KB per entry and hidden
        // layer; 400 MB at 4096 rollouts -- HBM capacity is not a constraint here).  Allocated lazily at the first screened step.
    }
    // the input tables keep zeros in the slots the other operand owns; the slot assignment depends on the network's d
    CK(hipMemsetAsync(ctx->d_FpH, 0, (size_t)ctx->cfg.max_obs * 32 * 2, ctx->stream));
    CK(hipMemsetAsync(ctx->d_FqH, 0, (size_t)ctx->cfg.n_traj * 32 * 2, ctx->stream));
    if (!pk.wh.empty()) {
        const uint16_t* dwh = nullptr;
        if ((rc = upload(ctx, pk.wh, &dwh))) return rc;
        if ((rc = upload(ctx, pk.sbias, &ctx->screen.bias))) return rc;
        ctx->screen.Wh = dwh;
        ctx->scr.adopt_pack(std::move(pk.host_W), std::move(pk.host_b), std::move(pk.out_dims));
        if (skip_mask) {   // the concatenation operands of the screening kernel (omds_screen_sidx), beside FqH / FpH
            CK(ctx->d_FqS.reserve((size_t)ctx->cfg.n_traj * 32));
            CK(ctx->d_FpS.reserve((size_t)ctx->cfg.max_obs * 32));
            CK(hipMemsetAsync(ctx->d_FqS, 0, ctx->d_FqS.bytes(), ctx->stream));
            CK(hipMemsetAsync(ctx->d_FpS, 0, ctx->d_FpS.bytes(), ctx->stream));
            m.scrQ = ctx->d_FqS;
            m.scrP = ctx->d_FpS;
        }
    }
    if ((rc = pk.for_each_pack([&](const auto& host, auto member) { return upload(ctx, host, &(m.*member)); }))) return rc;
    {
        std::vector<unsigned long long> zero(2 * (OMDS_MAX_HIDDEN + 1) + 2, 0ull);
        const unsigned long long* dz = nullptr;
        if ((rc = upload(ctx, zero, &dz))) return rc;
        m.skip_stats = const_cast<unsigned long long*>(dz);
    }
    // the exact zero-skip of k_pass1 (per-tile compaction): every ReLU network without skip concatenations
    m.compact = (act == OMDS_ACT_RELU && skip_mask == 0 && pk.nhh >= 1 && !(ctx->cfg.flags & OMDS_FLAG_DENSE_PASS1)) ? 1 : 0;
#ifdef OMDS_TIMELINE
    {
        static unsigned long long* tl = nullptr;
        if (!tl) { CK(hipMalloc(&tl, (size_t)(1 << 16) * 16 * sizeof(unsigned long long))); }
        CK(hipMemset(tl, 0, (size_t)(1 << 16) * 16 * sizeof(unsigned long long)));
        m.tl = tl;
    }
#endif
    ctx->mlp = m;
    ctx->act = act;
    ctx->f_fwd = pk.f_fwd;
    ctx->f_bwd = pk.f_bwd;
    ctx->have_mlp = true;
    obstacle_horizon_network_changed(ctx);
    if (ctx->n_obs > 0) {  // re-derive the obstacle half of layer 1 for the new weights
        omds_launch_obstacle_features(ctx->stream, ctx->mlp, ctx->d_obs, ctx->n_obs, ctx->d_Fp, ctx->d_radius, ctx->d_FpH, ctx->cfg.max_obs);
        CK(hipGetLastError());
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

int omds_dist_grad(omds_ctx* ctx, const float* q, int B, float* distance, float* nn_grad, float* mindist,
                   int32_t* closest_idx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(q && B >= 1 && B <= ctx->cfg.n_traj, OMDS_ERR_INVALID_ARG, "omds_dist_grad: need 1 <= batch <= n_traj and non-null q");
    int rc;
    if ((rc = check_ready(ctx, false))) return rc;
    CK(hipSetDevice(ctx->dev));
    const int n = ctx->cfg.n_dof, k = ctx->cfg.n_closest, O = ctx->n_obs, d = ctx->mlp.d;
    CK(hipMemcpyAsync(ctx->d_stage, q, (size_t)B * n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_qstage, B, n);   // -> [n][B]
    if ((rc = enqueue_network(ctx, ctx->d_qstage, B, B, obstacle_tables(ctx)))) return rc;
    omds_launch_blend(ctx->stream, ctx->d_gradx, ctx->d_drow, B, k, d, n, ctx->prm.softmax_k, ctx->d_dist, ctx->d_nngrad);
    CK(hipGetLastError());
    if (distance) CK(hipMemcpyAsync(distance, ctx->d_dist, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (nn_grad) CK(hipMemcpyAsync(nn_grad, ctx->d_nngrad, (size_t)B * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (mindist) CK(hipMemcpyAsync(mindist, ctx->d_Dmin, (size_t)B * O * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (closest_idx) CK(hipMemcpyAsync(closest_idx, ctx->d_idx, (size_t)B * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

// the raw rows x [B][d] through the network and the vjp of one output per row: the arg-min one (seed_col < 0) or column seed_col
static int mlp_rows_vjp(omds_ctx* ctx, const char* who, const float* x, int B, int seed_col, float* y, float* grad, int32_t* min_idx) {
    const int n = ctx->cfg.n_dof;
    const int cap = ctx->cfg.n_traj * ctx->cfg.n_closest;
    if (!(x && B >= 1 && B <= cap)) { ctx->err = std::string(who) + ": need 1 <= batch <= n_traj*n_closest and non-null x"; return OMDS_ERR_INVALID_ARG; }
    REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, "distance network not set (omds_set_mlp)");
    const int d = ctx->mlp.d;
    CK(hipSetDevice(ctx->dev));
    if (ctx->wide.on) {   // wide networks: the raw rows through the unfused GEMM path
        int rcw;
        CK(hipMemcpyAsync(ctx->d_stage, x, (size_t)B * d * 4, hipMemcpyHostToDevice, ctx->stream));
        if ((rcw = omds_wide_vjp(ctx, ctx->d_stage, B, seed_col))) return rcw;
    } else {
        // every row is its own (rollout, obstacle) pair: Fq from x[:, :n], Fp from x[:, n:], radius 0
        std::vector<float> xyzr((size_t)B * 4, 0.f), qrow((size_t)B * n);
        std::vector<int32_t> ident(B);
        for (int r = 0; r < B; ++r) {
            for (int j = 0; j < n; ++j) qrow[(size_t)r * n + j] = x[(size_t)r * d + j];
            for (int j = 0; j < d - n; ++j) xyzr[(size_t)r * 4 + j] = x[(size_t)r * d + n + j];
            ident[r] = r;
        }
        // per-row "obstacle" buffers of this entry point, allocated on first use for the context's capacity and kept
        if (!ctx->d_vjp_rad) {
            CK(ctx->d_vjp_xyzr.alloc((size_t)cap * 4));
            CK(ctx->d_vjp_B.alloc((size_t)cap * OMDS_FROW));
            CK(hipMemsetAsync(ctx->d_vjp_B, 0, ctx->d_vjp_B.bytes(), ctx->stream));
            CK(ctx->d_vjp_rad.alloc((size_t)cap));
        }
        float *d_xyzr = ctx->d_vjp_xyzr, *d_B = ctx->d_vjp_B, *d_rad = ctx->d_vjp_rad;
        // pageable sources: the copies have read them when the calls return
        CK(hipMemcpyAsync(d_xyzr, xyzr.data(), (size_t)B * 16, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(ctx->d_stage, qrow.data(), (size_t)B * n * 4, hipMemcpyHostToDevice, ctx->stream));
        CK(hipMemcpyAsync(ctx->d_idx, ident.data(), (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
        omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_qstage, B, n);
        omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_qstage, B, B, ctx->d_Fq);
        omds_launch_obstacle_features(ctx->stream, ctx->mlp, d_xyzr, B, d_B, d_rad);
        omds_launch_pass2(ctx->stream, ctx->mlp, ctx->d_Fq, d_B, d_rad, d_xyzr, ctx->d_idx, B, 1, ctx->d_qstage, B,
                          ctx->d_gradx, ctx->d_drow, ctx->d_yraw, ctx->d_minidx, ctx->d_dscr, seed_col);
    }
    CK(hipGetLastError());
    CK(hipStreamSynchronize(ctx->stream));
    if (y) {
        std::vector<float> ypad((size_t)B * OMDS_CPAD);
        CK(hipMemcpy(ypad.data(), ctx->d_yraw, ypad.size() * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < B; ++r)
            for (int c = 0; c < ctx->mlp.C; ++c) y[(size_t)r * ctx->mlp.C + c] = ypad[(size_t)r * OMDS_CPAD + c];
    }
    if (grad) CK(hipMemcpy(grad, ctx->d_gradx, (size_t)B * d * 4, hipMemcpyDeviceToHost));
    if (min_idx) CK(hipMemcpy(min_idx, ctx->d_minidx, (size_t)B * 4, hipMemcpyDeviceToHost));
    return OMDS_OK;
}

int omds_mlp_forward_vjp(omds_ctx* ctx, const float* x, int B, float* y, float* grad, int32_t* min_idx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    return mlp_rows_vjp(ctx, "omds_mlp_forward_vjp", x, B, -1, y, grad, min_idx);
}

int omds_mlp_jacobian(omds_ctx* ctx, const float* x, int B, const int32_t* cols, int n_cols, float* y, float* jac) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, "distance network not set (omds_set_mlp)");
    REQUIRE(cols && jac && n_cols >= 1 && n_cols <= OMDS_CPAD, OMDS_ERR_INVALID_ARG, "omds_mlp_jacobian: need cols, jac and 1 <= n_cols <= 16");
    for (int k = 0; k < n_cols; ++k)
        REQUIRE(cols[k] >= 0 && cols[k] < ctx->mlp.C, OMDS_ERR_INVALID_ARG, "omds_mlp_jacobian: a column index is outside 0 .. out_channels - 1");
    const int d = ctx->mlp.d;
    std::vector<float> g;
    for (int k = 0; k < n_cols; ++k) {   // one backward per column, like the reference's loop of .backward() calls (robot_sdf.py:94-100)
        int rc = mlp_rows_vjp(ctx, "omds_mlp_jacobian", x, B, cols[k], k == 0 ? y : nullptr, nullptr, nullptr);
        if (rc) return rc;
        g.resize((size_t)B * d);
        CK(hipMemcpy(g.data(), ctx->d_gradx, g.size() * 4, hipMemcpyDeviceToHost));
        for (int r = 0; r < B; ++r)
            for (int j = 0; j < d; ++j) jac[((size_t)r * d + j) * n_cols + k] = g[(size_t)r * d + j];
    }
    return OMDS_OK;
}
// the exact zero-skip of k_pass1 (omds.h): firing units and multiplied chunks per tile and hidden level, from the device's counters
int omds_pass1_skip_stats(omds_ctx* ctx, int32_t* active, double* mean_units, double* mean_chunks, int n_levels, int64_t* tiles) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, "distance network not set (omds_set_mlp)");
    REQUIRE(n_levels >= 0 && n_levels <= OMDS_MAX_HIDDEN + 1, OMDS_ERR_INVALID_ARG, "omds_pass1_skip_stats: 0 <= n_levels <= 9");
    const bool on = ctx->mlp.compact && !ctx->wide.on;
    if (active) *active = on ? 1 : 0;
    unsigned long long h[2 * (OMDS_MAX_HIDDEN + 1) + 2] = {0};
    if (on && ctx->mlp.skip_stats) {
        CK(hipSetDevice(ctx->dev));
        CK(hipStreamSynchronize(ctx->stream));
        CK(hipMemcpy(h, ctx->mlp.skip_stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    const double nt = h[0] ? (double)h[0] : 1.0;
    for (int L = 0; L < n_levels; ++L) {
        if (mean_chunks) mean_chunks[L] = on && L <= ctx->mlp.nhh ? (double)h[1 + L] / nt : 0.0;
        if (mean_units) mean_units[L] = on && L <= ctx->mlp.nhh ? (double)h[1 + (OMDS_MAX_HIDDEN + 1) + L] / nt : 0.0;
    }
    if (tiles) *tiles = (int64_t)h[0];
    return OMDS_OK;
}

}  // extern "C"
