// The obstacle horizon: per-step obstacle tables of a propagate (omds.h: omds_obstacle_horizon_predict, omds_set_obstacle_motion,
// omds_set_obstacle_horizon, omds_get_obstacle_horizon).  Step i of omds_propagate evaluates the network at all_traj[:, i - 1] and
// reads slab i - 1 of d_hzObs / d_hzRadius / d_hzFp (obstacle_tables, capi_internal.h); slab 0 is the current scene, whose static
// tables (d_obs / d_radius / d_Fp) every other entry point keeps using.  The tables are allocated at the first setter, grown with
// the other obstacle buffers (context.hip), and rebuilt by ONE launch (k_obstacle_horizon_features) when the velocities, params.dt
// or the network changed since they were built.
#include "capi_internal.h"

// slab h of a sphere moving at constant velocity: one fp32 product, one fmaf; slab 0 is the sphere itself
static inline float moved(float x, float v, int h, float dt) {
    if (h == 0) return x;
    const float t = (float)h * dt;
    return fmaf(v, t, x);
}

// The fp16 slab tables of the screened routes exist only where they can be used: screening over the horizon switched on
// (omds_set_screening_horizon) and a network with a screening pack; d_hzFpS only for its skip-connection form (MlpDev::scrP).
static bool horizon_fp16_wanted(const omds_ctx* ctx) { return ctx->scr.over_horizon && ctx->scr.ok && !ctx->wide.on; }

// (re-)allocates what of the fp16 tables is wanted and missing; the caller has synchronised the stream or is about to rebuild
static int alloc_horizon_fp16(omds_ctx* ctx) {
    if (!horizon_fp16_wanted(ctx) || ctx->hz_ld <= 0) return OMDS_OK;
    const size_t count = (size_t)ctx->cfg.horizon * ctx->hz_ld * 32;
    const bool skip = ctx->mlp.scrP != nullptr;
    if (ctx->d_hzFpH.count() >= count && (!skip || ctx->d_hzFpS.count() >= count)) return OMDS_OK;
    CK(hipStreamSynchronize(ctx->stream));
    if (ctx->d_hzFpH.count() < count) CK(ctx->d_hzFpH.alloc(count));
    if (skip && ctx->d_hzFpS.count() < count) CK(ctx->d_hzFpS.alloc(count));
    ctx->hz_zero = true;
    if (ctx->hz_mode) ctx->hz_dirty = true;
    return OMDS_OK;
}

int alloc_obstacle_horizon(omds_ctx* ctx) {
    const size_t H = ctx->cfg.horizon, ld = ((size_t)ctx->cfg.max_obs + 15) / 16 * 16;
    REQUIRE(H * ld < ((size_t)1 << 31), OMDS_ERR_INVALID_ARG, "obstacle horizon: horizon * max_obs must stay below 2^31");
    ctx->hz_ld = 0;
    ctx->d_hzFpH.reset(); ctx->d_hzFpS.reset();   // sized by ld: allocated again below when they are wanted
    CK(ctx->d_hzVel.alloc(ld * 3));
    CK(ctx->d_hzObs.alloc(H * ld * 4));
    CK(ctx->d_hzRadius.alloc(H * ld));
    CK(ctx->d_hzFp.alloc(H * ld * OMDS_FROW));
    ctx->hz_ld = (int)ld;
    ctx->hz_zero = true;
    return alloc_horizon_fp16(ctx);
}

void clear_obstacle_horizon(omds_ctx* ctx) {
    ctx->hz_mode = 0;
    ctx->hz_dirty = false;
    ctx->hz_vel.clear();
    ctx->hz_table.clear();
}

void obstacle_horizon_network_changed(omds_ctx* ctx) {
    ctx->hz_zero = true;   // the slot assignment of the encoded rows follows the network's d
    if (ctx->hz_mode) ctx->hz_dirty = true;
}

int prepare_obstacle_horizon(omds_ctx* ctx) {
    if (ctx->hz_mode == 0) return OMDS_OK;
    if (ctx->hz_mode == 1 && ctx->hz_dt != ctx->prm.dt) ctx->hz_dirty = true;
    int rc;
    if ((rc = alloc_horizon_fp16(ctx))) return rc;   // screening over the horizon was switched on, or the network brought a pack: dirty
    if (!ctx->hz_dirty) return OMDS_OK;
    REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, "distance network not set (omds_set_mlp)");
    const int H = ctx->cfg.horizon, O = ctx->n_obs, ld = ctx->hz_ld;
    const bool fp16 = horizon_fp16_wanted(ctx) && ctx->d_hzFpH;
    uint16_t* FpS = (fp16 && ctx->mlp.scrP) ? ctx->d_hzFpS.get() : nullptr;
    if (ctx->hz_zero) {   // the joints' slots and the padding stay zero
        CK(hipMemsetAsync(ctx->d_hzFp, 0, ctx->d_hzFp.bytes(), ctx->stream));
        if (ctx->d_hzFpH) CK(hipMemsetAsync(ctx->d_hzFpH, 0, ctx->d_hzFpH.bytes(), ctx->stream));
        if (ctx->d_hzFpS) CK(hipMemsetAsync(ctx->d_hzFpS, 0, ctx->d_hzFpS.bytes(), ctx->stream));
        ctx->hz_zero = false;
    }
    const float* vel = nullptr;
    if (ctx->hz_mode == 1) {
        CK(hipMemcpyAsync(ctx->d_hzVel, ctx->hz_vel.data(), (size_t)O * 12, hipMemcpyHostToDevice, ctx->stream));
        vel = ctx->d_hzVel;
    } else {
        CK(hipMemcpy2DAsync(ctx->d_hzObs, (size_t)ld * 16, ctx->hz_table.data(), (size_t)O * 16, (size_t)O * 16, H, hipMemcpyHostToDevice, ctx->stream));
    }
    omds_launch_obstacle_horizon_features(ctx->stream, ctx->mlp, ctx->d_obs, vel, ctx->prm.dt, H, O, ld, ctx->d_hzObs, ctx->d_hzRadius, ctx->d_hzFp,
                                          fp16 ? ctx->d_hzFpH.get() : nullptr, FpS);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(ctx->stream));   // the copies above read pageable host memory of the context
    ctx->hz_dt = ctx->prm.dt;
    ctx->hz_dirty = false;
    return OMDS_OK;
}

// The last slab of the horizon on the host, [n_obs][4]: what the screening calibration records and compares (screening.hip).  The
// arithmetic of the tables: omds_obstacle_horizon_predict's for a motion (a planar-point network keeps z), the caller's for a table.
void obstacle_horizon_last_slab(const omds_ctx* ctx, std::vector<float>& out) {
    const int H = ctx->cfg.horizon, O = ctx->n_obs;
    if (ctx->hz_mode == 2) {
        out.assign(ctx->hz_table.begin() + (size_t)(H - 1) * O * 4, ctx->hz_table.begin() + (size_t)H * O * 4);
        return;
    }
    out = ctx->obs_now;
    if (ctx->hz_mode != 1) return;
    const int po = ctx->mlp.d - ctx->mlp.n_dof;
    for (int o = 0; o < O; ++o)
        for (int c = 0; c < po && c < 3; ++c) out[(size_t)o * 4 + c] = moved(out[(size_t)o * 4 + c], ctx->hz_vel[(size_t)o * 3 + c], H - 1, ctx->prm.dt);
}

// what both setters need before they touch the context: a scene, and the tables
static int horizon_ready(omds_ctx* ctx, const char* who) {
    if (ctx->n_obs <= 0) { ctx->err = std::string(who) + ": obstacles not set (omds_set_obstacles)"; return OMDS_ERR_NOT_INITIALISED; }
    CK(hipSetDevice(ctx->dev));
    if (!ctx->d_hzFp || ctx->hz_ld < ctx->cfg.max_obs) {
        CK(hipStreamSynchronize(ctx->stream));
        return alloc_obstacle_horizon(ctx);
    }
    return OMDS_OK;
}

// while a focus is in force the motion and horizon setters would address the subset and be lost at the next focus
static std::string focus_refusal(const char* who) {
    return std::string(who) + ": an obstacle focus is in force (the call would address the kept subset and be lost at the next focus); "
                              "omds_clear_obstacle_focus first";
}

// the body of omds_set_obstacle_motion behind its focus check: the obstacle focus installs the kept velocities through it
int install_obstacle_motion(omds_ctx* ctx, const float* vel) {
    int rc;
    if ((rc = horizon_ready(ctx, "omds_set_obstacle_motion"))) return rc;
    clear_obstacle_horizon(ctx);
    if (!vel) return OMDS_OK;
    ctx->hz_vel.assign(vel, vel + (size_t)ctx->n_obs * 3);
    ctx->hz_mode = 1;
    ctx->hz_dirty = true;
    return OMDS_OK;
}

extern "C" {

int omds_obstacle_horizon_predict(const float* xyzr, const float* vel, int n_obs, int horizon, float dt, float* out) {
    if (!xyzr || !vel || !out || n_obs < 1 || horizon < 1) {
        g_create_err = "omds_obstacle_horizon_predict: need non-null xyzr [O,4], vel [O,3], out [H,O,4] and n_obs, horizon >= 1";
        return OMDS_ERR_INVALID_ARG;
    }
    for (int h = 0; h < horizon; ++h)
        for (int o = 0; o < n_obs; ++o) {
            float* q = out + ((size_t)h * n_obs + o) * 4;
            for (int c = 0; c < 3; ++c) q[c] = moved(xyzr[(size_t)o * 4 + c], vel[(size_t)o * 3 + c], h, dt);
            q[3] = xyzr[(size_t)o * 4 + 3];
        }
    return OMDS_OK;
}

int omds_set_obstacle_motion(omds_ctx* ctx, const float* vel) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(!obstacle_focus_active(ctx), OMDS_ERR_UNSUPPORTED, focus_refusal("omds_set_obstacle_motion"));
    return install_obstacle_motion(ctx, vel);
}

int omds_get_obstacle_motion(omds_ctx* ctx, float* vel, int32_t* have_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->n_obs > 0, OMDS_ERR_NOT_INITIALISED, "omds_get_obstacle_motion: obstacles not set (omds_set_obstacles)");
    const bool have = ctx->hz_mode == 1;
    if (have_out) *have_out = have ? 1 : 0;
    if (!vel) return OMDS_OK;
    if (have) std::memcpy(vel, ctx->hz_vel.data(), (size_t)ctx->n_obs * 12);
    else std::fill(vel, vel + (size_t)ctx->n_obs * 3, 0.f);
    return OMDS_OK;
}

int omds_set_obstacle_horizon(omds_ctx* ctx, const float* xyzr_h, int n_obs) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    int rc;
    REQUIRE(!obstacle_focus_active(ctx), OMDS_ERR_UNSUPPORTED, focus_refusal("omds_set_obstacle_horizon"));
    if ((rc = horizon_ready(ctx, "omds_set_obstacle_horizon"))) return rc;
    if (!xyzr_h) { clear_obstacle_horizon(ctx); return OMDS_OK; }
    REQUIRE(n_obs == ctx->n_obs, OMDS_ERR_INVALID_ARG, "omds_set_obstacle_horizon: n_obs differs from the scene's (omds_set_obstacles)");
    REQUIRE(ctx->obs_now.size() == (size_t)n_obs * 4 && std::memcmp(xyzr_h, ctx->obs_now.data(), (size_t)n_obs * 16) == 0, OMDS_ERR_INVALID_ARG,
            "omds_set_obstacle_horizon: slab 0 must be the current scene bit for bit (omds_set_obstacles)");
    clear_obstacle_horizon(ctx);
    ctx->hz_table.assign(xyzr_h, xyzr_h + (size_t)ctx->cfg.horizon * n_obs * 4);
    ctx->hz_mode = 2;
    ctx->hz_dirty = true;
    return OMDS_OK;
}

int omds_get_obstacle_horizon(omds_ctx* ctx, float* xyzr_h, int32_t* mode_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->n_obs > 0, OMDS_ERR_NOT_INITIALISED, "omds_get_obstacle_horizon: obstacles not set (omds_set_obstacles)");
    const int H = ctx->cfg.horizon, O = ctx->n_obs;
    if (mode_out) *mode_out = ctx->hz_mode;
    if (ctx->hz_mode == 0) {   // every step sees the static scene
        for (int h = 0; xyzr_h && h < H; ++h) std::memcpy(xyzr_h + (size_t)h * O * 4, ctx->obs_now.data(), (size_t)O * 16);
        return OMDS_OK;
    }
    CK(hipSetDevice(ctx->dev));
    int rc;
    if ((rc = prepare_obstacle_horizon(ctx))) return rc;
    if (!xyzr_h) return OMDS_OK;
    CK(hipMemcpy2DAsync(xyzr_h, (size_t)O * 16, ctx->d_hzObs, (size_t)ctx->hz_ld * 16, (size_t)O * 16, H, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

// ---- the moving frame (omds.h: THE MOVING FRAME) --------------------------------------------------------------------------------
int omds_moving_frame_velocity(int n_dof, int d, int k, const float* gradx, const float* drow, const float* vel, float softmax_k,
                               float max_speed, float* rate_out, float* qo_out) {
    if (!gradx || !drow || !vel || !rate_out || !qo_out || n_dof < 1 || n_dof > OMDS_MAX_DOF || k < 1 || (d != n_dof + 2 && d != n_dof + 3) ||
        max_speed != max_speed) {
        g_create_err = "omds_moving_frame_velocity: need non-null gradx [k,d], drow [k], vel [k,3], rate_out [1], qo_out [n_dof], "
                       "1 <= n_dof <= 7, k >= 1, d = n_dof + 2 or n_dof + 3, and a max_speed that is a number";
        return OMDS_ERR_INVALID_ARG;
    }
    if (!(max_speed > 0.f)) max_speed = 1.f;
    float mx = -INFINITY, s = 0.f, g[OMDS_MAX_DOF] = {0}, rate = 0.f, gn2 = 0.f;
    for (int j = 0; j < k; ++j) mx = fmaxf(mx, softmax_k * drow[j]);
    for (int j = 0; j < k; ++j) s += expf(softmax_k * drow[j] - mx);
    for (int j = 0; j < k; ++j) {
        const float w = expf(softmax_k * drow[j] - mx) / s;
        const float* gr = gradx + (size_t)j * d;
        for (int c = 0; c < n_dof; ++c) g[c] = fmaf(gr[c], w, g[c]);
        float sj = 0.f;
        for (int c = 0; c < d - n_dof; ++c) sj = fmaf(gr[n_dof + c], vel[(size_t)j * 3 + c], sj);
        rate = fmaf(sj, w, rate);
    }
    for (int c = 0; c < n_dof; ++c) gn2 = fmaf(g[c], g[c], gn2);
    const float gn = sqrtf(gn2);
    float r = rate / gn;
    if (gn == 0.f || !std::isfinite(r)) r = 0.f;
    r = fminf(fmaxf(r, -max_speed), max_speed);
    *rate_out = rate;
    for (int c = 0; c < n_dof; ++c) qo_out[c] = gn == 0.f ? 0.f : -r * (g[c] / gn);
    return OMDS_OK;
}

int omds_set_obstacle_frame(omds_ctx* ctx, int moving, float max_speed) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(max_speed == max_speed && max_speed < INFINITY, OMDS_ERR_INVALID_ARG, "omds_set_obstacle_frame: max_speed is not a finite number");
    ctx->frame_on = moving != 0;
    ctx->frame_max = max_speed > 0.f ? max_speed : 1.f;
    return OMDS_OK;
}

int omds_get_obstacle_frame(omds_ctx* ctx, int32_t* moving, float* max_speed, int32_t* in_effect) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (moving) *moving = ctx->frame_on ? 1 : 0;
    if (max_speed) *max_speed = ctx->frame_max;
    if (in_effect) *in_effect = (ctx->frame_on && ctx->hz_mode == 1) ? 1 : 0;
    return OMDS_OK;
}

int omds_approach_rate(omds_ctx* ctx, const float* q, int B, float* rate, float* qo) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(q && B >= 1 && B <= ctx->cfg.n_traj, OMDS_ERR_INVALID_ARG, "omds_approach_rate: need 1 <= batch <= n_traj and non-null q");
    int rc;
    if ((rc = check_ready(ctx, false))) return rc;
    REQUIRE(ctx->hz_mode == 1, OMDS_ERR_NOT_INITIALISED, "omds_approach_rate: no obstacle velocities (omds_set_obstacle_motion)");
    CK(hipSetDevice(ctx->dev));
    if ((rc = prepare_obstacle_horizon(ctx))) return rc;   // the velocities reach the device with the tables
    const int n = ctx->cfg.n_dof, k = ctx->cfg.n_closest, d = ctx->mlp.d;
    CK(ctx->d_frameOut.reserve((size_t)ctx->cfg.n_traj * (1 + n)));
    float* d_rate = ctx->d_frameOut;
    float* d_qo = d_rate + ctx->cfg.n_traj;
    CK(hipMemcpyAsync(ctx->d_stage, q, (size_t)B * n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_qstage, B, n);   // -> [n][B]
    if ((rc = enqueue_network(ctx, ctx->d_qstage, B, B, obstacle_tables(ctx)))) return rc;   // the current scene: slab 0
    omds_launch_approach_rate(ctx->stream, ctx->d_gradx, ctx->d_drow, ctx->d_idx, ctx->d_hzVel, 3, B, k, d, n, ctx->prm.softmax_k,
                              ctx->frame_max, d_rate, d_qo);
    CK(hipGetLastError());
    if (rate) CK(hipMemcpyAsync(rate, d_rate, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (qo) CK(hipMemcpyAsync(qo, d_qo, (size_t)B * n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return OMDS_OK;
}

}  // extern "C"
