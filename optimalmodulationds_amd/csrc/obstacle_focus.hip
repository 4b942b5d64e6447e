// The obstacle focus (omds.h: omds_focus_obstacles, omds_get_obstacle_focus, omds_clear_obstacle_focus, omds_obstacle_focus_select):
// narrow a large scene to the spheres near one joint state, on the device.  The state between calls is omds_ctx::focus (cloud_state.h):
// the MASTER -- the scene that was in force at the first focus call, with its motion velocities and the labels of an objects call --
// from which every later call selects again.  One call:
//   distances : the master's spheres as the obstacle rows of ONE fp32 pass-1 launch over one state, the way the self-filter of
//               scene_cloud.hip drives it; the value is the mindist row of omds_dist_grad(q, 1) on the master, bit for bit
//   selection : keys of the reaches, the one-workgroup radix select (obstacle_focus_kernels.hip), the ordered compaction with FocusSrc
//               (cloud_kernels.hip): the kept spheres in ascending master index with their indices and velocities; only those travel
//   install   : the kept list in through install_obstacles, the body of omds_set_obstacles; then the kept velocities through the body of
//               omds_set_obstacle_motion if the master moves and a kept component is non-zero; the labels gathered
// omds_focus_obstacles_path does the same along B states: pass 1 in chunks of at most n_traj states, per chunk the keys, the bar of
// every state and the merge into two words per sphere, then the selection on those words; everything around the distances and the
// selection (focus_open, focus_install) is shared.
#include "capi_internal.h"
#include "cloud_kernels.h"
#include "obstacle_focus_def.h"

namespace {

constexpr int FOCUS_MAX_MASTER = 1 << 30;   // the compaction's item index is an int, rounded up to whole blocks

// the scene in force becomes the master: device copies of the spheres (and velocities), host copies of everything
int capture_master(omds_ctx* ctx) {
    FocusState& f = ctx->focus;
    const int n = ctx->n_obs;
    const bool moving = ctx->hz_mode == 1;
    if (f.master.count() < (size_t)n || (moving && f.vel.count() < (size_t)n * 3)) CK(hipStreamSynchronize(ctx->stream));
    CK(f.master.reserve((size_t)n));
    if (moving) CK(f.vel.reserve((size_t)n * 3));
    CK(hipMemcpyAsync(f.master, ctx->d_obs, (size_t)n * 16, hipMemcpyDeviceToDevice, ctx->stream));
    f.h_master = ctx->obs_now;
    f.h_vel = moving ? ctx->hz_vel : std::vector<float>();
    if (moving) CK(hipMemcpyAsync(f.vel, f.h_vel.data(), (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    const CloudState& s = ctx->cloud;
    f.labelled = s.obj_label.size() == (size_t)n;
    f.label = f.labelled ? s.obj_label : std::vector<int32_t>();
    f.flag = f.labelled ? s.obj_flag : std::vector<int32_t>();
    f.obj_count = s.obj_count;
    f.n_master = n;
    f.moving = moving;
    return OMDS_OK;
}

int reserve_focus(omds_ctx* ctx) {
    FocusState& f = ctx->focus;
    const size_t n = (size_t)f.n_master, nb = (size_t)cloud_compaction_blocks(f.n_master) + 1, nv = f.moving ? n * 3 : 0;
    if (f.keys.count() < n || f.sums.count() < nb || f.res.count() < 4 || f.kept.count() < n || f.keptIdx.count() < n || f.keptVel.count() < nv)
        CK(hipStreamSynchronize(ctx->stream));
    CK(f.keys.reserve(n));
    CK(f.sums.reserve(nb));
    CK(f.res.reserve(4));
    CK(f.kept.reserve(n));
    CK(f.keptIdx.reserve(n));
    CK(f.keptVel.reserve(nv));
    return OMDS_OK;
}

// the labels of the master gathered to the scene in force (install_obstacles has forgotten those of the scene before)
void gather_labels(omds_ctx* ctx) {
    const FocusState& f = ctx->focus;
    if (!f.labelled) return;
    CloudState& s = ctx->cloud;
    s.obj_label.resize(f.idx.size());
    s.obj_flag.resize(f.idx.size());
    for (size_t i = 0; i < f.idx.size(); ++i) {
        s.obj_label[i] = f.label[(size_t)f.idx[i]];
        s.obj_flag[i] = f.flag[(size_t)f.idx[i]];
    }
    s.obj_count = f.obj_count;
}

// a path's scratch: the per-sphere words, the bars of a chunk of C states and the times of all n_states
int reserve_focus_path(omds_ctx* ctx, int C, int n_states) {
    FocusState& f = ctx->focus;
    const size_t n = (size_t)f.n_master;
    if (f.best.count() < n || f.pass.count() < n || f.bars.count() < (size_t)C || f.time.count() < (size_t)n_states) CK(hipStreamSynchronize(ctx->stream));
    CK(f.best.reserve(n));
    CK(f.pass.reserve(n));
    CK(f.bars.reserve((size_t)C));
    CK(f.time.reserve((size_t)n_states));
    return OMDS_OK;
}

// From here on the tables of the scene in force are overwritten: the context holds no scene until focus_install has put the kept one in
int focus_open(omds_ctx* ctx) {
    int rc;
    CK(hipSetDevice(ctx->dev));
    if (!obstacle_focus_active(ctx) && (rc = capture_master(ctx))) return rc;
    if ((rc = reserve_focus(ctx))) return rc;
    ctx->n_obs = 0;
    ctx->focus.on = false;
    clear_obstacle_horizon(ctx);
    return OMDS_OK;
}

// the selection res [4] over sel [n_master] is enqueued: compact, read back, install, gather the labels
int focus_install(omds_ctx* ctx, const unsigned* sel, int32_t* kept_out, int32_t* passed_out) {
    FocusState& f = ctx->focus;
    const int O = f.n_master;
    const float* vel = f.moving ? f.vel.get() : nullptr;
    int rc;
    omds_launch_focus_compact(ctx->stream, sel, f.res, f.master, vel, O, O, f.kept, f.keptIdx, f.keptVel, f.sums);
    CK(hipGetLastError());
    unsigned res[4] = {0, 0, 0, 0};
    CK(hipMemcpyAsync(res, f.res, 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    const int kept = (int)res[0];
    REQUIRE(kept >= ctx->cfg.n_closest && kept <= O, OMDS_ERR_HIP, "omds_focus_obstacles: the selection returned an impossible count");
    std::vector<float> list((size_t)kept * 4), kv(f.moving ? (size_t)kept * 3 : 0);
    f.idx.resize((size_t)kept);
    CK(hipMemcpyAsync(list.data(), f.kept, (size_t)kept * 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(f.idx.data(), f.keptIdx, (size_t)kept * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (f.moving) CK(hipMemcpyAsync(kv.data(), f.keptVel, (size_t)kept * 12, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    if ((rc = install_obstacles(ctx, list.data(), kept))) return rc;
    bool moves = false;
    for (float v : kv) moves |= v != 0.f;
    if (moves && (rc = install_obstacle_motion(ctx, kv.data()))) return rc;
    gather_labels(ctx);
    f.on = true;
    if (kept_out) *kept_out = kept;
    if (passed_out) *passed_out = (int32_t)res[1];
    return OMDS_OK;
}

int focus_body(omds_ctx* ctx, const FocusRule& r, const float* q, int32_t* kept_out, int32_t* passed_out) {
    FocusState& f = ctx->focus;
    if (int rc = focus_open(ctx)) return rc;
    const int n = ctx->cfg.n_dof, O = f.n_master;
    CK(hipMemcpyAsync(ctx->d_qcur, q, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_qcur, 1, 1, ctx->d_Fq);
    omds_launch_obstacle_features(ctx->stream, ctx->mlp, reinterpret_cast<const float*>(f.master.get()), O, ctx->d_Fp, ctx->d_radius);
    omds_launch_pass1(ctx->stream, ctx->mlp, ctx->d_Fq, ctx->d_Fp, ctx->d_radius, O, 1, ctx->prm.ignored_links, ctx->d_Dmin);
    CK(hipGetLastError());
    const float* vel = f.moving ? f.vel.get() : nullptr;
    omds_launch_focus_keys(ctx->stream, ctx->d_Dmin, vel, ctx->mlp.d - ctx->mlp.n_dof, r.lookahead, O, f.keys);
    omds_launch_focus_select(ctx->stream, f.keys, O, ctx->cfg.n_closest, r.margin, r.all_pass, r.max_keep, f.res);
    return focus_install(ctx, f.keys, kept_out, passed_out);
}

constexpr int FOCUS_PATH_MAX_STATES = 65536, FOCUS_PATH_MAX_CHUNK = 4096;

// The states in chunks of at most C = min(n_traj, 4096): what d_stage, d_qstage, d_Fq and d_Dmin ([n_traj][max_obs]) hold.  A chunk
// goes through pass 1 the way a batch of omds_dist_grad does, and its rows into the per-sphere words; the selection follows the last
int focus_path_body(omds_ctx* ctx, const FocusRule& r, const float* q_path, const float* ahead, int n_states, int32_t* kept_out, int32_t* passed_out) {
    FocusState& f = ctx->focus;
    int rc;
    if ((rc = focus_open(ctx))) return rc;
    const int n = ctx->cfg.n_dof, O = f.n_master, C = std::min({ctx->cfg.n_traj, n_states, FOCUS_PATH_MAX_CHUNK});
    if ((rc = reserve_focus_path(ctx, C, n_states))) return rc;
    const float* vel = f.moving ? f.vel.get() : nullptr;
    std::vector<float> time((size_t)n_states);
    for (int b = 0; b < n_states; ++b) time[(size_t)b] = ahead ? focus_path_time(r.lookahead, ahead[b]) : r.lookahead;
    CK(hipMemcpyAsync(f.time, time.data(), (size_t)n_states * 4, hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemsetAsync(f.best, 0xff, (size_t)O * 4, ctx->stream));
    CK(hipMemsetAsync(f.pass, 0, (size_t)O * 4, ctx->stream));
    omds_launch_obstacle_features(ctx->stream, ctx->mlp, reinterpret_cast<const float*>(f.master.get()), O, ctx->d_Fp, ctx->d_radius);
    for (int b0 = 0; b0 < n_states; b0 += C) {
        const int c = std::min(C, n_states - b0);
        CK(hipMemcpyAsync(ctx->d_stage, q_path + (size_t)b0 * n, (size_t)c * n * 4, hipMemcpyHostToDevice, ctx->stream));
        omds_launch_transpose(ctx->stream, ctx->d_stage, ctx->d_qstage, c, n);   // -> [n][c]
        omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_qstage, c, c, ctx->d_Fq);
        omds_launch_pass1(ctx->stream, ctx->mlp, ctx->d_Fq, ctx->d_Fp, ctx->d_radius, O, c, ctx->prm.ignored_links, ctx->d_Dmin);
        omds_launch_focus_path_chunk(ctx->stream, ctx->d_Dmin, vel, ctx->mlp.d - ctx->mlp.n_dof, f.time.get() + b0, c, O, ctx->cfg.n_closest, r.margin,
                                     r.all_pass, f.bars, f.best, f.pass);
        CK(hipGetLastError());
    }
    omds_launch_focus_path_select(ctx->stream, f.best, f.pass, O, ctx->cfg.n_closest, r.max_keep, f.keys, f.res);
    return focus_install(ctx, f.keys, kept_out, passed_out);
}

}  // namespace

extern "C" {

int omds_obstacle_focus_select(const omds_obstacle_focus_spec* spec, const float* d, const float* vel, int n_obs, int n_closest, int32_t* idx_out,
                               int32_t cap, int32_t* kept_out, int32_t* passed_out) {
    return focus_select_host(spec, d, vel, n_obs, n_closest, idx_out, cap, kept_out, passed_out, &g_create_err);
}

int omds_obstacle_focus_select_path(const omds_obstacle_focus_spec* spec, const float* d, const float* ahead, const float* vel, int n_states, int n_obs,
                                    int n_closest, int32_t* idx_out, int32_t cap, int32_t* kept_out, int32_t* passed_out) {
    return focus_select_path_host(spec, d, ahead, vel, n_states, n_obs, n_closest, idx_out, cap, kept_out, passed_out, &g_create_err);
}

// the state refusals both device calls share; they leave scene, master and focus as they were
static int focus_state_checks(omds_ctx* ctx) {
    REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, "omds_focus_obstacles: the distances need the distance network (omds_set_mlp)");
    REQUIRE(!ctx->wide.on, OMDS_ERR_UNSUPPORTED, "omds_focus_obstacles: no focus on networks wider than 256 (no obstacle tables)");
    REQUIRE(ctx->n_obs > 0, OMDS_ERR_NOT_INITIALISED, "omds_focus_obstacles: obstacles not set (omds_set_obstacles)");
    const bool active = obstacle_focus_active(ctx);
    REQUIRE(active || ctx->hz_mode != 2, OMDS_ERR_UNSUPPORTED,
            "omds_focus_obstacles: the scene carries an explicit horizon table (omds_set_obstacle_horizon), which a subset cannot keep");
    REQUIRE((active ? ctx->focus.n_master : ctx->n_obs) <= FOCUS_MAX_MASTER, OMDS_ERR_UNSUPPORTED, "omds_focus_obstacles: more than 2^30 spheres");
    return OMDS_OK;
}

// the cloud calls' guarantee: a failure behind the argument checks leaves the context without a scene
static int focus_failed(omds_ctx* ctx, int rc) {
    if (rc) {
        ctx->n_obs = 0;
        ctx->focus.on = false;
        clear_obstacle_horizon(ctx);
    }
    return rc;
}

int omds_focus_obstacles(omds_ctx* ctx, const omds_obstacle_focus_spec* spec, const float* q, int32_t* kept_out, int32_t* passed_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    FocusRule r;
    if (int rc = focus_resolve_spec(spec, ctx->cfg.n_closest, &r, &ctx->err)) return rc;
    REQUIRE(q, OMDS_ERR_INVALID_ARG, "omds_focus_obstacles: null q [n_dof]");
    if (int rc = focus_state_checks(ctx)) return rc;
    return focus_failed(ctx, focus_body(ctx, r, q, kept_out, passed_out));
}

int omds_focus_obstacles_path(omds_ctx* ctx, const omds_obstacle_focus_spec* spec, const float* q_path, const float* ahead, int n_states,
                              int32_t* kept_out, int32_t* passed_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    FocusRule r;
    if (int rc = focus_resolve_spec(spec, ctx->cfg.n_closest, &r, &ctx->err)) return rc;
    REQUIRE(q_path && n_states >= 1 && n_states <= FOCUS_PATH_MAX_STATES, OMDS_ERR_INVALID_ARG,
            "omds_focus_obstacles_path: need non-null q_path [n_states][n_dof] and 1 <= n_states <= 65536");
    if (ahead)
        for (int b = 0; b < n_states; ++b) REQUIRE(focus_ahead_ok(ahead[b]), OMDS_ERR_INVALID_ARG, "omds_focus_obstacles_path: every ahead must be finite and >= 0");
    if (int rc = focus_state_checks(ctx)) return rc;
    return focus_failed(ctx, focus_path_body(ctx, r, q_path, ahead, n_states, kept_out, passed_out));
}

int omds_get_obstacle_focus(omds_ctx* ctx, int32_t* idx, int32_t* n_master_out, int32_t* n_kept_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const bool active = obstacle_focus_active(ctx);
    if (n_master_out) *n_master_out = active ? ctx->focus.n_master : 0;
    if (n_kept_out) *n_kept_out = ctx->n_obs;
    if (idx && active) std::memcpy(idx, ctx->focus.idx.data(), (size_t)ctx->n_obs * 4);
    return OMDS_OK;
}

int omds_clear_obstacle_focus(omds_ctx* ctx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    if (!obstacle_focus_active(ctx)) return OMDS_OK;
    FocusState& f = ctx->focus;
    int rc;
    if ((rc = install_obstacles(ctx, f.h_master.data(), f.n_master))) return rc;
    if (f.moving && (rc = install_obstacle_motion(ctx, f.h_vel.data()))) return rc;
    if (f.labelled) {
        ctx->cloud.obj_label = f.label;
        ctx->cloud.obj_flag = f.flag;
        ctx->cloud.obj_count = f.obj_count;
    }
    return OMDS_OK;
}

}  // extern "C"
