// Host-only declarations shared by the translation units of the C ABI (include/omds.h): context.hip, mlp_pack.hip, network.hip,
// screening.hip, propagate.hip, update.hip, sdf_data.hip, obstacle_horizon.hip, scene_cloud.hip and obstacle_focus.hip.  No kernel file includes this header.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include <dlfcn.h>

#include "omds_internal.h"
#include "propagate_plan_def.h"

// message of a call that has no context to keep it in (omds_last_error(NULL)); defined in context.hip
extern thread_local std::string g_create_err;

// Optional roctx ranges named like the reference's torch.profiler record_function tags (MPPI.py:102-268,
// frankaPlanner.py:135-145), so that a `rocprofv3 --marker-trace --kernel-trace` timeline reads like the reference's
// Chrome trace.  Enabled with OMDS_ROCTX=1; the roctx library is dlopen'ed, never linked.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char* e = getenv("OMDS_ROCTX");
        if (!e || atoi(e) == 0) return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
        pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
struct RoctxRange {
    static Roctx& api() { static Roctx r; return r; }
    bool on;
    explicit RoctxRange(const char* name) : on(api().push != nullptr) { if (on) api().push(name); }
    ~RoctxRange() { if (on) api().pop(); }
};

#define CK(expr) OMDS_HIP_CHECK(ctx, expr)
#define REQUIRE(cond, code, msg)            \
    do {                                    \
        if (!(cond)) {                      \
            ctx->err = (msg);               \
            return (code);                  \
        }                                   \
    } while (0)

// a host array into a device allocation of the network's own (omds_ctx::mlp_allocs)
template <typename T>
inline int upload(omds_ctx* ctx, const std::vector<T>& h, const T** dptr) {
    void* p = nullptr;
    CK(hipMalloc(&p, h.size() * sizeof(T)));
    ctx->mlp_allocs.push_back(p);
    CK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *dptr = reinterpret_cast<const T*>(p);
    return OMDS_OK;
}

// ---- measurement: event brackets around the dominant kernel of a step (omds_prof_*: context.hip) ---------------------------
inline int prof_collect(omds_ctx* ctx) {
    ProfEvents& p = ctx->prof;
    for (size_t i = 0; i < p.used; ++i) {
        float ms = 0.f;
        CK(hipEventSynchronize(p.stop[i]));
        CK(hipEventElapsedTime(&ms, p.start[i], p.stop[i]));
        p.ms += ms;
    }
    p.used = 0;
    return OMDS_OK;
}
inline int prof_begin(omds_ctx* ctx) {
    if (!ctx->prof_on) return OMDS_OK;
    // an event record between two kernels costs ~5.7 us of idle GPU (tools/gap_probe.py: back-to-back launches
    // otherwise start with no gap), so a measurement run brackets only every prof_stride-th launch
    ctx->prof_open = (ctx->prof_seen++ % ctx->prof_stride) == 0;
    if (!ctx->prof_open) return OMDS_OK;
    ProfEvents& p = ctx->prof;
    if (p.used >= 4096) { int rc = prof_collect(ctx); if (rc) return rc; }   // elapsed times are read lazily (omds_prof_read); bound the open events
    if (p.used == p.start.size()) {
        hipEvent_t a, b;
        CK(hipEventCreate(&a));
        CK(hipEventCreate(&b));
        p.start.push_back(a);
        p.stop.push_back(b);
    }
    CK(hipEventRecord(p.start[p.used], ctx->stream));
    return OMDS_OK;
}
// the next prof_begin will open a bracket / a launch of the dominant kernel that is counted but, by the caller's choice, not bracketed
// (enqueue_dense: only a step that runs alone on the device is bracketed)
inline bool prof_due(const omds_ctx* ctx) { return ctx->prof_on && ctx->prof_seen % ctx->prof_stride == 0; }
inline void prof_pass(omds_ctx* ctx) { if (ctx->prof_on) ctx->prof_seen++; }
inline int prof_end(omds_ctx* ctx, int64_t rows, double flops = -1.0, const char* kernel = "k_pass1") {
    if (!ctx->prof_on || !ctx->prof_open) return OMDS_OK;
    ctx->prof_open = false;
    ProfEvents& p = ctx->prof;
    CK(hipEventRecord(p.stop[p.used], ctx->stream));
    p.used++;
    p.launches++;
    p.rows += rows;
    p.flops += flops >= 0.0 ? flops : (double)rows * ctx->f_fwd;
    p.kernel = kernel;
    return OMDS_OK;
}

inline int check_ready(omds_ctx* ctx, bool need_ds) {
    REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, "distance network not set (omds_set_mlp)");
    REQUIRE(ctx->n_obs > 0, OMDS_ERR_NOT_INITIALISED, "obstacles not set (omds_set_obstacles)");
    if (need_ds) REQUIRE(ctx->have_ds, OMDS_ERR_NOT_INITIALISED, "nominal DS not set (omds_set_ds)");
    return OMDS_OK;
}

// ---- mlp_pack.hip: everything a network install derives from the caller's weights on the HOST -------------------------------
// Validation, zero-padding to the kernels' width, and the MFMA fragment packs.  No device, no context: the sanitizer build runs
// it on the CPU (tests/test_asan_cpu.py through omds_test_pack_mlp).
struct MlpPacks {
    int nhh = 0, C = 0, d = 0, act = 0;
    float out_div = 1.f;
    uint32_t skip_mask = 0;
    uint8_t skip_col[OMDS_MAX_HIDDEN + 1] = {0};
    std::vector<float4> wf, wb, wf16, wb16, wb4, wf4, wl, w1b, w1b16, w1f, w1f16;
    std::vector<float> bh, bl, wlraw, whraw, w1t, b1, wht, wlt;
    std::vector<uint16_t> wh;     // the screening pack (ScreenDev::Wh / bias): empty when the screening kernel does not take the network
    std::vector<float> sbias;
    double f_fwd = 0.0, f_bwd = 0.0;
    // what build_screen_pack needs to build wh / sbias again in another unit order (ReLU / tanh networks the screening kernel takes)
    std::vector<std::vector<float>> host_W, host_b;   // zero-padded to width 256
    std::vector<int32_t> out_dims;
    // THE list of MlpDev's packs: v(host vector, the MlpDev member it is uploaded to) for each, in upload order; stops at the
    // first non-zero return and hands it on.  omds_set_mlp_ex uploads through it, omds_test_pack_mlp checksums through it.
    template <typename V>
    int for_each_pack(V&& v) const {
        int rc;
        if ((rc = v(wf16, &MlpDev::Wf16)) || (rc = v(wb16, &MlpDev::Wb16)) || (rc = v(wb4, &MlpDev::Wb4)) || (rc = v(wf4, &MlpDev::Wf4)) ||
            (rc = v(w1b16, &MlpDev::W1b16)) || (rc = v(wf, &MlpDev::Wf)) || (rc = v(wb, &MlpDev::Wb)) || (rc = v(bh, &MlpDev::bh)) ||
            (rc = v(wl, &MlpDev::Wl)) || (rc = v(bl, &MlpDev::bl)) || (rc = v(wlraw, &MlpDev::Wlraw)) || (rc = v(whraw, &MlpDev::Whraw)) ||
            (rc = v(w1t, &MlpDev::W1t)) || (rc = v(b1, &MlpDev::b1)) || (rc = v(w1b, &MlpDev::W1b)) || (rc = v(w1f, &MlpDev::W1f)) ||
            (rc = v(w1f16, &MlpDev::W1f16)) || (rc = v(wht, &MlpDev::WhT)) || (rc = v(wlt, &MlpDev::WlT)))
            return rc;
        return OMDS_OK;
    }
};
uint16_t f32_to_f16_bits(float f);
// the argument checks the fused and the wide install share; fills err and returns the error code of the first that fails
int check_mlp_args(int n_dof, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W, const float* const* b,
                   int act, float out_div, std::string& err);
void build_screen_pack(MlpPacks& pk, const int32_t* order);
int build_mlp_packs(int n, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W,
                    const float* const* b, int act, float out_div, int n_skips, const int32_t* skip_after, MlpPacks& pk,
                    std::string& err);

// ---- obstacle_horizon.hip: per-step obstacle tables of a propagate ------------------------------------------------------------
// The three obstacle tables a launch reads: Fp [O][OMDS_FROW], radius [O], obs [O][4]
struct ObsTables { const float* Fp; const float* radius; const float* obs; };
// ... of horizon step `step` (1-based): slab step - 1 of the horizon while one is set, else the static scene (step 0: the static
// scene in any case, for the batch entry points; slab 0 holds the same values)
inline ObsTables obstacle_tables(const omds_ctx* ctx, int step = 0) {
    if (ctx->hz_mode == 0 || step < 1) return {ctx->d_Fp, ctx->d_radius, ctx->d_obs};
    const size_t r = (size_t)(step - 1) * ctx->hz_ld;
    return {ctx->d_hzFp + r * OMDS_FROW, ctx->d_hzRadius + r, ctx->d_hzObs + r * 4};
}
// ... and what the screening kernel reads beside them: the fp16 table of the obstacle points with its row capacity, the radii, and
// the network descriptor carrying the skip-connection operand (MlpDev::scrP) of the same table.  Step i of a propagate with a
// horizon: slab i - 1 of d_hzFpH / d_hzFpS / d_hzRadius (built by prepare_obstacle_horizon while screening over the horizon is on)
struct ScreenTables { const uint16_t* FpH; int ld; const float* radius; MlpDev m; };
inline ScreenTables screen_tables(const omds_ctx* ctx, int step = 0) {
    if (ctx->hz_mode == 0 || step < 1) return {ctx->d_FpH, ctx->cfg.max_obs, ctx->d_radius, ctx->mlp};
    const size_t r = (size_t)(step - 1) * ctx->hz_ld;
    ScreenTables t{ctx->d_hzFpH + r * 32, ctx->hz_ld, ctx->d_hzRadius + r, ctx->mlp};
    if (t.m.scrP) t.m.scrP = ctx->d_hzFpS + r * 32;
    return t;
}
void obstacle_horizon_last_slab(const omds_ctx* ctx, std::vector<float>& out);   // [n_obs][4] the scene step H sees, on the host
int alloc_obstacle_horizon(omds_ctx* ctx);             // the tables for cfg.horizon x cfg.max_obs (first setter; grow_obstacle_capacity)
void clear_obstacle_horizon(omds_ctx* ctx);            // omds_set_obstacles: back to the static scene
void obstacle_horizon_network_changed(omds_ctx* ctx);  // omds_set_mlp*: the feature slabs are derived again at the next propagate
int prepare_obstacle_horizon(omds_ctx* ctx);           // omds_propagate: rebuilds the tables when they are dirty (one launch)
int install_obstacle_motion(omds_ctx* ctx, const float* vel);   // the body of omds_set_obstacle_motion behind its focus check

// ---- context.hip: the scene ----------------------------------------------------------------------------------------------------
int reserve_obstacle_capacity(omds_ctx* ctx, int n_obs);             // grows the obstacle buffers when n_obs exceeds max_obs (the scene is then gone)
int install_obstacles(omds_ctx* ctx, const float* xyzr, int n_obs);   // the body of omds_set_obstacles behind its argument checks
// an obstacle focus is in force (obstacle_focus.hip): the scene is a subset of omds_ctx::focus's master.  install_obstacles ends it
inline bool obstacle_focus_active(const omds_ctx* ctx) { return ctx->focus.on && ctx->n_obs > 0; }

// ---- network.hip ------------------------------------------------------------------------------------------------------------
void release_network(omds_ctx* ctx);   // frees omds_ctx::mlp_allocs (omds_destroy; every install starts with it)
// the distance network on a batch of states qT [n][ldq] against the obstacle tables t: Fq -> pass 1 -> top-k -> pass 2 (or the
// context's other arithmetic)
int enqueue_network(omds_ctx* ctx, const float* qT, int ldq, int B, const ObsTables& t);

// ---- screening.hip: the controller of the screened step -----------------------------------------------------------------------
bool screen_wanted(omds_ctx* ctx);   // mode, packs, not suspended, no horizon unless screening over it is on: this propagate should screen
// calibrates when no bound stands (q_center: the start state of the propagate); *usable = a bound exists and screening is not suspended
int screen_calibrated(omds_ctx* ctx, const float* q_center, bool* usable);
// What screen_begin_propagate hands the horizon loop of the screened routes
struct ScreenPlan {
    float* fq0 = nullptr;        // layer-1 table of step i: fq0 + (i - 1) * fq_slab (fq_slab = 0: one slab, updated in place)
    size_t fq_slab = 0;
    bool fuse_select = false;    // k_screen selects in its flush phase (no matrix, no k_select)
    const SelectSink* h_sinks = nullptr;   // [H] the sinks of all steps, host copy / device copy
    const SelectSink* d_sinks = nullptr;
    ExactOut ex{};               // k_exact's per-entry outputs
    float eps = 0.f;             // the bound the tails' slack guard checks against
};
// zeroes the counters, builds and uploads the sinks, prepares the audit sample and (when one is due) the sweep
int screen_begin_propagate(omds_ctx* ctx, const StepArgs& a, bool list_tail, ScreenPlan* plan);
// between a step's selection and its tail: the sweep of that step, when this propagate carries one and the step is part of it
void enqueue_sweep_of_step(omds_ctx* ctx, const float* fq_step, int N, int step);
// behind the horizon loop: k_audit and the copies of what the propagate measured into the pinned verdict words
int screen_finish_propagate(omds_ctx* ctx, const ScreenPlan& plan);
// after the stream has been synchronised: accept the propagate, or redo it on the non-screened route
int screened_verdict(omds_ctx* ctx, StepArgs& a);

// ---- propagate.hip ------------------------------------------------------------------------------------------------------------
// (StepRoute: propagate_plan_def.h)
bool small_step_wanted(omds_ctx* ctx);
bool fused_step_available(const omds_ctx* ctx);   // the fused tail kernels take this context (else Unfused, never screened)
StepRoute choose_route(omds_ctx* ctx, bool screen_requested);
int enqueue_rollouts(omds_ctx* ctx, StepArgs& a, StepRoute route);
