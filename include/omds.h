/*
 * omds.h -- C-ABI of the MI355X-native MPPI rollout + DS-modulation hot path.
 *
 * The reference (epfl-lasa/OptimalModulationDS) is pure Python on PyTorch-CPU and has NO
 * FFI / plugin boundary of its own; its "interface" for this path is the Python class API of
 * python_scripts/ds_mppi/functions/{MPPI,policy,cost,LinDS}.py and
 * python_scripts/mlp_learn/sdf/robot_sdf.py.  Each entry point below names the reference
 * method(s) it replaces (file:line relative to python_scripts/).  A maintainer binds these with
 * ctypes; optimalmodulationds_amd/_lib.py is that binding.
 *
 * Conventions
 *   - every function returns an omds_status (0 = OK); omds_last_error() gives the message;
 *     nothing aborts the process and there is no CPU fallback: without a usable HIP device
 *     omds_create() fails with OMDS_ERR_HIP.
 *   - all host arrays are C-contiguous fp32 / int32 in the reference's axis order; the caller
 *     owns host buffers, the library owns device buffers for the life of the context.
 *   - one context per device; calls on a context are not re-entrant; every call enqueues on the
 *     context's HIP stream and synchronises before returning unless stated otherwise.
 */
#ifndef OMDS_H
#define OMDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OMDS_API __attribute__((visibility("default")))

typedef struct omds_ctx omds_ctx;

typedef enum {
    OMDS_OK = 0,
    OMDS_ERR_INVALID_ARG = 1,
    OMDS_ERR_HIP = 2,
    OMDS_ERR_RCCL = 3,
    OMDS_ERR_NOT_INITIALISED = 4,
    OMDS_ERR_UNSUPPORTED = 5
} omds_status;

#define OMDS_MAX_DOF 7
#define OMDS_ACT_RELU 0
#define OMDS_ACT_TANH 1

/* MPPI.__init__ arguments (ds_mppi/functions/MPPI.py:22-66). */
typedef struct {
    int32_t n_dof;         /* n: joints (<= OMDS_MAX_DOF)                                   */
    int32_t n_traj;        /* N: rollouts held by THIS context (the shard, in multi-GPU)   */
    int32_t horizon;       /* H: dt_H                                                      */
    int32_t n_kernel_max;  /* TensorPolicyMPPI.N_KERNEL_MAX (policy.py:18), 50             */
    int32_t max_obs;       /* capacity of the obstacle buffer                              */
    int32_t n_closest;     /* k: n_closest_obs                                             */
    int32_t device;        /* HIP device ordinal                                           */
    int32_t flags;         /* OMDS_FLAG_* bits, 0 = defaults                               */
} omds_config;

/* omds_config.flags: the generic step of omds_propagate -- five launches (k_pass1, k_topk, k_pass2, k_modulate,
 * k_rollout_layer1), the only one for n_dof other than 2 and 7 -- instead of the two-launch k_pass1 + k_tail step. */
#define OMDS_FLAG_UNFUSED_STEP 1
/* Keep scenes with few obstacles (O <= 32) on the two-launch k_pass1 + k_tail step instead of the one-launch fused
 * small-scene step (k_step_small) that omds_propagate picks for them by itself.                                      */
#define OMDS_FLAG_TWO_KERNEL_STEP 2
/* the all-fp32 step keeps its tail with a forward of its own (k_tail) instead of taking pass 2's forward from pass 1 (k_pass1 in
 * its emitting mode + k_tail_sel: same bits, one forward less); for A/B runs and the tests that compare the two            */
#define OMDS_FLAG_TAIL_FORWARD 4
/* k_pass1 multiplies every k-chunk of every layer instead of compacting every tile to the hidden units that fire in it (the exact
 * zero-skip of ReLU networks: same bits either way); for A/B runs and the tests that compare the two                              */
#define OMDS_FLAG_DENSE_PASS1 8
/* pass 1 over the plain row space at every horizon step: a propagate from ONE state (per_rollout == 0) evaluates its first step
 * for each of the N rollouts instead of once for all of them (same bits either way); for A/B runs and the tests that compare */
#define OMDS_FLAG_NATURAL_PASS1 16
/* every pass-1 tile covers consecutive rows of the rollout-major pair space, instead of a block of rollouts x obstacles that are
 * neighbours in a key order of their layer-1 signs, which the full launches of the compacting kernel form so that the rows of a tile
 * fire alike (same bits either way: a row does not depend on its tile-mates); for A/B runs and the tests that compare the two    */
#define OMDS_FLAG_NATURAL_TILES 32
/* the block order of the tiles at every batch size, not only from OMDS_BLOCK_TILES_MIN_PAIRS rollout-obstacle pairs on, below which
 * the ordering launches cost more than they save (EXPERIMENTS.md R15: bracketed by 112 896 pairs, slower, and 150 528, faster, at 294
 * obstacles; not located); for A/B runs and the tests, which run small batches                                                    */
#define OMDS_FLAG_BLOCK_TILES 64
#define OMDS_BLOCK_TILES_MIN_PAIRS 131072
/* THE SCHEDULE OF A PROPAGATE'S FULL STEPS (csrc/propagate_plan_def.h).  The rollouts of a batch do not depend on each
 * other over the whole horizon, so the dense block-ordered step may run the batch as two halves on two streams, one half's tail and
 * ordering launches under the other half's pass 1.  Either schedule computes the same bits: a row's chain never depends on its
 * tile-mates, the tail is local to a rollout, and the key units and the obstacle order are picked on the whole batch either way.
 * By default omds_propagate runs the two halves where each holds OMDS_BLOCK_TILES_MIN_PAIRS pairs and at least three full steps
 * follow the shared first one (Franka shelf 1024 x 32: +4.0 %, EXPERIMENTS.md R35).  SERIAL_PROPAGATE keeps every launch of every
 * step on one stream; PIPELINED_PROPAGATE runs the two halves wherever the dense route's compacting kernel runs and at least two full
 * steps exist, at any batch size (A/B runs and the tests, which run small batches).  Both set: serial.  omds_get_pipeline_info
 * reports what the last omds_propagate ran.  While omds_prof_enable is on, a step whose pass 1 is bracketed runs as one whole-batch
 * launch in either case.                                                                                                          */
#define OMDS_FLAG_SERIAL_PROPAGATE 128
#define OMDS_FLAG_PIPELINED_PROPAGATE 256

/* The constants the reference hard-codes inside propagate() (MPPI.py:117-217,277) and
 * LinDS (LinDS.py:9), as parameters; omds_default_params() fills the reference values.   */
typedef struct {
    float dt;              /* integration step of the rollouts (MPPI.py:221)               */
    float dst_thr;         /* subtracted from the network distance (MPPI.py:117)           */
    float lin_thr;         /* LinDS.lin_thr (LinDS.py:9)                                   */
    float lvel[5];         /* generalized_sigmoid (y_min,y_max,x0,x1,k) of l_vel  (:132)   */
    float ln[5];           /* ... of l_n   (:143-153)                                      */
    float ltau[5];         /* ... of l_tau (:155)                                          */
    float goal_act_cut;    /* goal activation hard cut, 0.5 (:194)                         */
    float norm_clamp;      /* velocities with norm <= this are not normalised, 0.5 (:212)  */
    float coll_slow;       /* in-collision slow-down factor 0.1 (:215)                     */
    float coll_repulse;    /* in-collision repulsion gain 0.1 (:216)                       */
    float softmax_k;       /* -10: weights of the k closest gradients (:277)               */
    float rbf_p;           /* Policy.p, RBF norm order (policy.py:41), 2                   */
    uint32_t ignored_links;/* bit c set: link c is masked in pass 1 (MPPI.py:241)          */
    uint32_t variant;      /* OMDS_VARIANT_* bits; 0 = MPPI.py, see below                  */
    uint32_t cost_terms;   /* OMDS_COST_* bits summed by Cost.evaluate_costs; default all  */
} omds_params;

/* ds_mppi/functions/MPPI_toy.py (the 2-D toy drivers' variant of MPPI.py) differs from MPPI.py in constants
 * (all of them fields above) and in two behaviours:                                                        */
#define OMDS_VARIANT_KVAL_TIMES_ACT 1u /* kernel_val_all holds phi * activation (MPPI_toy.py:178-179)       */
#define OMDS_VARIANT_NO_BASE_MASK   2u /* update mask without the rollout-0 term (MPPI_toy.py:318-321)      */
/* Cost.evaluate_costs terms (cost.py:14-21); cost_toy.py:14-18 sums GOAL | COLLISION | STAGNATION only.    */
#define OMDS_COST_GOAL         1u
#define OMDS_COST_COLLISION    2u
#define OMDS_COST_JOINT_LIMITS 4u
#define OMDS_COST_STAGNATION   8u
#define OMDS_COST_FK          16u
#define OMDS_COST_ALL         31u

OMDS_API void omds_default_params(omds_params* p);

/* MPPI.__init__ tensor allocation (MPPI.py:37-66); no warm-up propagates are run. */
OMDS_API int omds_create(const omds_config* cfg, omds_ctx** out);
OMDS_API void omds_destroy(omds_ctx* ctx);
/* Message of the last failure on ctx (ctx == NULL: last omds_create failure of this thread). */
OMDS_API const char* omds_last_error(const omds_ctx* ctx);

/* RobotSdfCollisionNet.load_weights + model preparation (robot_sdf.py:31-51,
 * frankaPlanner.py:43-51).  n_linear Linear layers; dims[n_linear+1] = {3(n+3), hidden...,
 * C}; W[i] is [dims[i+1], dims[i]] row-major like torch, b[i] is [dims[i+1]].  act =
 * OMDS_ACT_*; out_div = 100 when C == 9 (cm -> m, MPPI.py:236-237) else 1.  dims[0] may also
 * be 3(n+2): the toy networks take planar obstacle points (in_channels = DOF+2,
 * scripts/standaloneToy2d.py:33); the z column of the obstacle array is then ignored.
 * Widths: hidden layers of up to 256 units (every network the reference ships: 256 and 128) run on the fused LDS-resident MFMA
 * kernels (narrower ones zero-padded).  MLPRegression itself is width-agnostic (network_macros_mod.py:96-135): a network with a
 * hidden layer of 257 .. 4096 units takes the unfused path of csrc/wide_kernels.hip -- the reference's own op sequence on exact-fp32
 * MFMA GEMMs with the activations materialised in HBM; no screening, no skip concatenations there.  Same results contract.
 * The encoding's sin / cos (csrc/trig_device.h) are the oracle's bits for |x| < 125, the range they restate; above it (and for
 * inf / NaN) both round the double-precision sin / cos to float, which agree but are not the same code (tests/test_gpu_trig.py). */
OMDS_API int omds_set_mlp(omds_ctx* ctx, int n_linear, const int32_t* dims, const float* const* W,
                          const float* const* b, int act, float out_div);
/* The same for MLPRegression(..., skips=[...]) (network_macros_mod.py:113-146): behind the activations of
 * the Linear layers named in skip_after[n_skips] (indices into the flat sequence of Linear layers, 0 ..
 * n_linear-2) the encoded input [x, sin x, cos x] is concatenated, so the next Linear layer is 3(n+3)
 * wider than the previous one's output: W[i] is [out_dims[i], in_dims[i]] with in_dims[0] = 3(n+3) and
 * in_dims[i] = out_dims[i-1] (+ 3(n+3) behind a concatenation, its columns last, as torch.cat((y, x_nerf))
 * orders them).  out_dims[i] + 3(n+3) <= 256 for those layers (the reference narrows them by 3(n+3) itself).
 * n_skips = 0 is omds_set_mlp.  Skip-connection networks are screened like plain ones (the screening kernel ORs the
 * encoded input into the last two k-chunks of the layer behind a concatenation).                                        */
OMDS_API int omds_set_mlp_ex(omds_ctx* ctx, int n_linear, const int32_t* in_dims, const int32_t* out_dims,
                             const float* const* W, const float* const* b, int act, float out_div,
                             int n_skips, const int32_t* skip_after);

/* MPPI.update_obstacles (MPPI.py:347-350): xyzr is [O,4] spheres (x,y,z,r).  n_obs may exceed config.max_obs: the obstacle
 * buffers then grow (to twice n_obs) inside the context -- handle, network, samples, communicator and screening state stay. */
OMDS_API int omds_set_obstacles(omds_ctx* ctx, const float* xyzr, int n_obs);
/* THE OBSTACLE HORIZON (new work: the reference holds one self.obs for all H steps of a propagate, MPPI.py:347-350).  Step i of
 * omds_propagate (1-based) evaluates the network at all_traj[:, i-1]; with a horizon it sees the spheres of SLAB i-1 of a table
 * [H,O,4] instead of the current scene: collision distance, kernel-candidate search and modulation of steps 2..H then run against
 * the scene as it is predicted for their time, not frozen at now.  Slab 0 is always the current scene, so omds_dist_grad and the
 * other batch entry points (which keep reading it) stay consistent with step 1.  By default only the distance field moves; with
 * omds_set_obstacle_frame the modulation also runs in the frame in which the obstacle rests (THE MOVING FRAME, below).  Without a
 * horizon nothing changes: same launches, same bits.
 *   omds_obstacle_horizon_predict : host only (no context, no GPU), the DEFINITION of constant-velocity prediction:
 *                           out[h][o][c] = fmaf(vel[o][c], (float)h * dt, xyzr[o][c]) for c < 3 and h >= 1 (the product one fp32
 *                           multiply), out[0][o] = xyzr[o], out[h][o][3] = xyzr[o][3].  xyzr [O,4], vel [O,3], out [H,O,4].
 *   omds_set_obstacle_motion : constant velocities vel [O,3] of the n_obs spheres of the last omds_set_obstacles; the table is
 *                           built on the device by the same formula with the params.dt in force at the propagate, and built again
 *                           when vel, dt or the network changed.  Planar-point networks (dims[0] = 3(n+2)) ignore vel[:,2] as they
 *                           ignore z.  NULL clears the horizon.
 *   omds_set_obstacle_horizon : the caller's own predictions xyzr_h [H,O,4] (a motion predictor, radii inflated with h: the radius
 *                           may differ per slab).  n_obs must be the scene's and slab 0 the current scene bit for bit, else
 *                           OMDS_ERR_INVALID_ARG.  NULL clears the horizon.
 *   omds_get_obstacle_horizon : the table the next propagate will use (built now if it is stale) into xyzr_h [H,O,4] (NULL: no copy);
 *                           *mode_out = 0 none (every slab is the static scene), 1 motion, 2 explicit.
 * omds_set_obstacles CLEARS the horizon (MPPI.update_obstacles keeps its meaning); a setter before any scene is
 * OMDS_ERR_NOT_INITIALISED.  The tables (H * max_obs * 37 floats: 2.8 MB at H = 32, 588 spheres) are allocated at the first setter and
 * grow with the other obstacle buffers.  SCREENING: by default a horizon puts omds_propagate on the all-fp32 step whatever mode was
 * requested; omds_screen_stats reports active = 0, the calibration is kept and screening resumes when the horizon is cleared.
 * With omds_set_screening_horizon(ctx, 1) (below, beside omds_set_screening) a propagate with a horizon is screened like a static
 * one: every step's fp16 pass, re-evaluation, sweep and audit rows read that step's slab (fp16 tables per slab, H * max_obs * 64
 * bytes more, twice that for skip-connection networks), and the bound is measured on three slabs.  Networks wider than 256:
 * omds_propagate returns OMDS_ERR_UNSUPPORTED while a horizon is set.                                                              */
OMDS_API int omds_obstacle_horizon_predict(const float* xyzr, const float* vel, int n_obs, int horizon, float dt, float* out);
OMDS_API int omds_set_obstacle_motion(omds_ctx* ctx, const float* vel);
OMDS_API int omds_set_obstacle_horizon(omds_ctx* ctx, const float* xyzr_h, int n_obs);
OMDS_API int omds_get_obstacle_horizon(omds_ctx* ctx, float* xyzr_h, int32_t* mode_out);
/* THE MOVING FRAME (new work; the standard remedy of the modulation-DS literature for moving obstacles).  M = E diag(l_nv, l_tau, ..) E^T
 * removes the normal component of the velocity near a surface as if that surface were at rest: against a sphere that approaches, a
 * rollout that stands still is "safe" and is hit anyway, and l_vel ("already moving away") switches the modulation off for a robot
 * that retreats more slowly than the obstacle chases.  With the frame on and a MOTION horizon set, every step evaluates the
 * modulation relative to the obstacle's velocity as the joints see it, and adds that velocity back.
 *   omds_moving_frame_velocity : host only (no context, no GPU), the DEFINITION.  gradx [k,d] are the full input gradients of the k
 *       selected rows (d = n_dof + 3, or n_dof + 2 for planar points: vel[:,2] is then not read), drow [k] their distances, vel [k,3]
 *       the velocity of the sphere of each row.  In fp32, every fmaf one rounding, sums ascending from 0:
 *         mx = max_j softmax_k drow_j;  s = sum_j expf(softmax_k drow_j - mx);  w_j = expf(softmax_k drow_j - mx) / s
 *         for j ascending: g[c] = fmaf(gradx_j[c], w_j, g[c]) (c < n);  s_j = fmaf chain over a of gradx_j[n+a] vel_j[a];
 *                          rate = fmaf(s_j, w_j, rate)
 *         gn = sqrtf(fmaf chain of g[c] g[c]);  r = rate / gn, 0 if gn == 0 or r is not finite, else clamped to +-max_speed
 *         qo[c] = -r * (g[c] / gn), 0 if gn == 0
 *       rate is the rate at which the blended distance changes because the spheres move (negative: they approach); qo is the
 *       minimum-norm joint velocity that keeps it constant.  max_speed <= 0 selects 1.
 *   omds_set_obstacle_frame : a preference of the context, off at creation; max_speed <= 0 selects the default 1.0, the unit speed
 *       rollout velocities are normalised to.  It survives omds_set_obstacles (which clears the horizon: the frame then has no
 *       effect until velocities are set again).  At omds_propagate: frame off, or no horizon -- exactly the launches and bits
 *       without it; a motion horizon -- the step below on every unscreened route (the fused kernels then run on 16- or 32-row
 *       tiles); an explicit table -- OMDS_ERR_UNSUPPORTED (the table carries no velocities).
 *       THE STEP: up to g, distance, normal, l_n, l_tau, the RBF policy and vnorm = |v| nothing changes.  Then v_rel = v - qo;
 *       dot = g^ . v_rel/|v_rel| (what dot_products holds and what feeds l_vel, hence l_nv, the activation and the kernel-candidate
 *       search); vt = v_rel + (act pol) vnorm; u = l_tau vt + ((l_nv - l_tau)(g^ . vt)) g^; s = |u| (1 where <= norm_clamp);
 *       u = nan_to_num(u / s); in collision u coll_slow + g^ vnorm coll_repulse; u_world = u + qo; q_next = q + dt u_world, and qdot
 *       of step 1 is u_world.  With qo = 0 every line is the arithmetic without the frame.
 *   omds_get_obstacle_frame : the preference, its clamp, and *in_effect = 1 when the next propagate will run the step above.
 *   omds_approach_rate : the batch form beside omds_dist_grad, on the device: rate [B] and qo [B,n] of the states q [B,n] against
 *       the current scene (slab 0) and the motion's velocities, clamped by the frame's max_speed -- a driver's feed-forward term.
 *       OMDS_ERR_NOT_INITIALISED without a motion horizon.                                                                        */
OMDS_API int omds_moving_frame_velocity(int n_dof, int d, int k, const float* gradx, const float* drow, const float* vel,
                                        float softmax_k, float max_speed, float* rate_out, float* qo_out);
OMDS_API int omds_set_obstacle_frame(omds_ctx* ctx, int moving, float max_speed);
OMDS_API int omds_get_obstacle_frame(omds_ctx* ctx, int32_t* moving, float* max_speed, int32_t* in_effect);
OMDS_API int omds_approach_rate(omds_ctx* ctx, const float* q, int batch, float* rate, float* qo);
/* THE SCENE FROM A DEPTH POINT CLOUD (new work: the reference's obstacle streamers send finished spheres).  A depth camera delivers
 * 1e4 .. 1e5 points per frame, the robot's own arm among them; the three steps between it and omds_set_obstacles -- a workspace crop,
 * a voxel down-sample, a robot self-filter -- run here, on the device, and the self-filter uses the distance network the context
 * already holds.  Additive: no other entry point changes its launches or its bits.
 *   omds_point_cloud_spheres : host only (no context, no GPU), the DEFINITION.  All fp32, every operation named one rounding:
 *       inv = 1.0f / voxel (once);  a point with a coordinate that is not finite is dropped;  f_c = floorf((p_c - origin_c) * inv), the
 *       point is kept only if 0 <= f_c < dims_c on all three axes (compared as floats, then converted);  cell = (i_z dims_y + i_y) dims_x
 *       + i_x;  a cell is occupied when at least min_points points fall in it;  the output lists the occupied cells in ascending cell
 *       order, each as the sphere (fmaf((float)i_c + 0.5f, voxel, origin_c), radius).  No centroids, no float atomics: the list is a
 *       function of the SET of points, whatever their order.  xyz [P,3], 0 <= P <= 16 777 216; xyzr_out [cap,4]; *count_out = occupied
 *       cells.  More of them than max_spheres or cap: OMDS_ERR_INVALID_ARG with *count_out set and nothing written.
 *   omds_set_obstacles_from_cloud : the same list built on the device and installed as the scene.  xyz is host memory, or (xyz_on_device
 *       = 1) device memory on the context's device that the caller has finished writing and leaves alone until the call returns.  One
 *       pass over the points counts them per cell (integer atomics on a count buffer sized to the spec at first use); an ordered
 *       compaction (per-block sums, a scan of the sums, per-block emission) writes the candidates in cell order, bit for bit the list
 *       above.  q_now [n_dof] != NULL: THE SELF-FILTER -- candidate c is dropped when d_c <= self_margin, where d_c is the pass-1 value
 *       of the library (minimum over the links not in params.ignored_links of y_j / out_div - radius) at the input (q_now, centre_c),
 *       evaluated by the fp32 pass-1 kernels over one state with the candidates as its obstacle rows (a NaN distance keeps the sphere);
 *       a second ordered compaction gives the final list.  It needs a network (else OMDS_ERR_NOT_INITIALISED) of hidden width <= 256
 *       (else OMDS_ERR_UNSUPPORTED); with q_now == NULL neither applies.  If fewer than n_closest spheres remain, copies of spec.pad are
 *       appended up to n_closest (omds_set_obstacles requires that many).  The list then goes through exactly what omds_set_obstacles
 *       does (horizon cleared, buffers grown, screening told).  *n_spheres_out = spheres before padding, *n_occupied_out = occupied
 *       cells before the self-filter (NULL = skip).  More occupied cells than max_spheres: OMDS_ERR_INVALID_ARG, *n_occupied_out set,
 *       the scene exactly as it was -- that guarantee covers this refusal and the argument checks only: a HIP failure later in the call
 *       leaves the context without a scene (and without a horizon) until the next successful scene setter.  Synchronous.
 *   omds_get_obstacles : the scene in force, xyzr [n_obs,4] (NULL: the count only); host state, no GPU work.                          */
typedef struct {
    float   origin[3];    /* lower corner of the voxel grid                                           */
    float   voxel;        /* edge length > 0                                                          */
    int32_t dims[3];      /* cells per axis, each >= 1, product <= 4 194 304 (2^22)                   */
    float   radius;       /* sphere radius; <= 0 selects 0.8660254f * voxel (the cell's circumsphere) */
    int32_t min_points;   /* a cell is occupied when at least this many points fall in it; < 1 -> 1   */
    int32_t max_spheres;  /* more occupied cells than this is an error; < 1 -> 4096; at most 65 536   */
    float   self_margin;  /* self-filter threshold, used only when a joint state is passed            */
    float   pad[4];       /* the sphere that fills an (almost) empty scene up to n_closest            */
} omds_cloud_spec;
OMDS_API int omds_point_cloud_spheres(const omds_cloud_spec* spec, const float* xyz, int64_t n_points, float* xyzr_out, int32_t cap,
                                      int32_t* count_out);
OMDS_API int omds_set_obstacles_from_cloud(omds_ctx* ctx, const omds_cloud_spec* spec, const float* xyz, int64_t n_points,
                                           int xyz_on_device, const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out);
OMDS_API int omds_get_obstacles(omds_ctx* ctx, float* xyzr, int32_t* n_obs_out);
/* SPHERE VELOCITIES FROM SUCCESSIVE CLOUDS (new work: the reference's streamers took velocities from mocap rigid bodies; a depth
 * camera gives none).  The tracked form of the cloud call estimates one velocity per sphere from the previous tracked frame, on the
 * device, and installs the velocities as the motion horizon (omds_set_obstacle_motion), so that a sensed scene can use the obstacle
 * horizon, the moving frame and screening over the horizon.  Additive: no other entry point changes its launches or its bits.
 * WHAT IT MEASURES: the NORMAL flow of a surface -- the centroid of a cell now minus the pooled centroid of the nearest previously
 * occupied cell(s).  Motion along a surface's own tangent is invisible to it (a sliding plane occupies the same cells); an object
 * thicker than its displacement along the motion is under-estimated (its interior cells find themselves at d2 = 0).  The normal
 * component is the part omds_approach_rate and the moving frame consume, because the distance gradient points along it.  No
 * segmentation or clustering, no tangential flow, no motion model beyond constant velocity, no smoothing of positions: out of scope
 * (smoothing of the velocities over frames: THE VELOCITY FILTER below).
 *   omds_point_cloud_flow : host only (no context, no GPU), the DEFINITION.  All fp32, every operation named one rounding, every
 *       conversion to float round-to-nearest; all sums are integers, so the result is a function of the two SETS of points.
 *       Per frame, for every point omds_point_cloud_spheres keeps: u_c = (p_c - origin_c) * inv, f_c = floorf(u_c), r_c = u_c - f_c
 *       (exact), k_c = (int)(r_c * 256.0f) (the product exact, the conversion truncates: 0 .. 255); the cell's record is four uint32,
 *       n += 1 and s_c += k_c (P <= 2^24 points: s <= 255 * 2^24 < 2^32).  The sphere list is that of omds_point_cloud_spheres(spec,
 *       xyz_now): same occupancy (n >= min_points), same order, same error for more occupied cells than max_spheres or cap (*count_out
 *       set, nothing else written).  Per occupied NOW cell c = (i_x, i_y, i_z) with record (n, s): the window is every cell j = c + k,
 *       |k_c| <= reach on all axes, inside the grid, whose PREVIOUS record has n'_j >= min_points; d2 = k . k.  Empty window: vel = 0,
 *       not matched.  Else m = min d2, T = {j : d2 = m}, t = |T|, A_c = -sum_T k_c (int32), P_c = sum_T s'_jc (uint64), N' = sum_T n'_j
 *       (uint64), and   whole_c = (float)A_c / (float)t;   sub_c = ((float)s_c / (float)n - (float)P_c / (float)N') * 0.00390625f;
 *       vel_c = ((whole_c + sub_c) * voxel) / dt_frame.   Ties are averaged, so no axis is favoured.  still > 0: with s2 = fmaf(v_z, v_z,
 *       fmaf(v_y, v_y, v_x * v_x)), s2 < still * still makes all three components +0.  *matched_out counts the cells with a non-empty
 *       window, zeroed by still or not.  xyzr_out [cap,4], vel_out [cap,3].  OMDS_ERR_INVALID_ARG before anything is written: a bad
 *       spec, reach outside 1 .. 4, dt_frame not finite or not > 0, still not finite, null pointers, a point count outside 0 .. 2^24.
 *   omds_set_obstacles_from_cloud_tracked : everything omds_set_obstacles_from_cloud does, in the same order, with the same final list
 *       bit for bit (self-filter and padding included); its counting pass also sums the sub-cell offsets (records of 16 bytes per cell,
 *       two such buffers in the context, integer atomics only), both compactions carry each sphere's cell index, and one launch (one
 *       wave per final sphere) evaluates the definition above against the stored frame.  After the list is installed the velocities go
 *       in through omds_set_obstacle_motion (padding spheres: 0).  THE PREVIOUS FRAME is the occupancy AS COUNTED by the last successful
 *       tracked call: the self-filter is not applied to it, so a sphere within reach cells of where the arm was can match the arm.
 *       There is no previous frame at the first call, after omds_cloud_track_reset, and when origin, voxel or dims are not bitwise
 *       those of the stored frame or min_points (resolved: < 1 is 1) differs: then the frame is stored, *n_matched_out = -1 and no
 *       horizon is set.  If every velocity of the final list is exactly 0 (a static scene; everything under still) the horizon stays
 *       cleared and the propagate that follows is the static one: same launches, same bits.  Otherwise the context is in horizon mode
 *       1.  *n_matched_out = final spheres (after the self-filter) with a non-empty window.  The stored frame is touched only by a
 *       successful tracked call and by the reset: omds_set_obstacles_from_cloud and omds_set_obstacles leave it alone, and a refusal
 *       (too many occupied cells, an argument check) leaves the scene AND the stored frame exactly as they were.
 *   omds_cloud_track_reset : forget the stored frame.
 *   omds_get_obstacle_motion : *have_out = 1 while a motion horizon is set, and its velocities into vel [n_obs,3] (zeros without one;
 *       NULL: no copy); host state, no GPU work.  OMDS_ERR_NOT_INITIALISED before any scene.                                          */
typedef struct {
    int32_t reach;     /* search window, cells per axis each way: 1 .. 4                                    */
    float   dt_frame;  /* seconds between the previous tracked frame and this one: finite, > 0              */
    float   still;     /* speeds below this become exactly 0; <= 0 disables                                 */
} omds_cloud_track_spec;
OMDS_API int omds_point_cloud_flow(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const float* xyz_prev,
                                   int64_t n_prev, const float* xyz_now, int64_t n_now, float* xyzr_out, float* vel_out, int32_t cap,
                                   int32_t* count_out, int32_t* matched_out);
OMDS_API int omds_set_obstacles_from_cloud_tracked(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track,
                                                   const float* xyz, int64_t n_points, int xyz_on_device, const float* q_now,
                                                   int32_t* n_spheres_out, int32_t* n_occupied_out, int32_t* n_matched_out);
OMDS_API int omds_cloud_track_reset(omds_ctx* ctx);
OMDS_API int omds_get_obstacle_motion(omds_ctx* ctx, float* vel, int32_t* have_out);
/* OBJECT VELOCITIES FROM SUCCESSIVE CLOUDS.  The tracked call above measures the normal flow per cell: it is blind to motion
 * along a surface and under-estimates an object thicker than its displacement.  The objects form segments the final sphere list into
 * connected components, matches the components of successive frames by their centroids, and gives every sphere of a matched object the
 * velocity of the object's centroid; everywhere else the sphere keeps the tracked call's velocity, so this route is never worse.
 * Additive: no other entry point changes its launches or its bits.
 * WHAT IT MEASURES: the rigid TRANSLATION of an object, from the displacement of the centroid of its visible points.  Rotation shows up
 * as the centroid's motion alone; two objects that touch (within link cells) are one object; an object entering the view, or being
 * uncovered, shifts its visible centroid and so reports a velocity it does not have (THE VELOCITY FILTER below damps it); no motion
 * model beyond constant velocity, no smoothing of positions.
 *   omds_point_cloud_object_flow : host only (no context, no GPU), the DEFINITION.  Records, occupancy and spheres are those of
 *       omds_point_cloud_flow.  keep_prev / keep_now: one uint8 per OCCUPIED cell of that frame in ascending cell order, NULL = keep all;
 *       they stand for the self-filter.  The output lists the occupied NOW cells with keep_now != 0 in cell order; *count_out = occupied
 *       NOW cells BEFORE the mask; more of them than max_spheres or cap: OMDS_ERR_INVALID_ARG with *count_out set, nothing else written.
 *       COMPONENTS, per frame over that frame's kept cells: two cells are linked when max_c |i_c - j_c| <= link; a component is a
 *       connected set; its label is the smallest cell index in it (a function of the set of cells).  Its record, all integers: m = cells
 *       (uint32), N = sum n (uint64), Q_c = sum (256 i_c n + s_c) (uint64, < 2^54): the sum of the points' coordinates in 1/256 cell.
 *       OBJECTS: a NOW component with m >= min_cells; *n_objects_out counts them.  Centroids in fp64, each operation one rounding,
 *       conversions round-to-nearest: cen_c = (double)Q_c / (double)N.  The candidate of a NOW object is, over all PREVIOUS components
 *       with m' >= min_cells, the one with the smallest d2 = (dx dx + dy dy) + dz dz (d = cen - cen', three products, two sums), ties to
 *       the smaller label.  It is accepted when d2 <= (256.0 * reach)^2 (the centroid moved at most reach cells) and 2 min(m, m') >=
 *       max(m, m') in integers (the guard against merges and splits).  Then per axis g = (float)((cen_c - cen'_c) * 0.00390625) and
 *       vel_c = (g * voxel) / dt_frame in fp32, followed by the still rule of omds_point_cloud_flow.  PER SPHERE: in an accepted object
 *       vel_out is the object's velocity and object_out = 1; everywhere else (small components, objects without a candidate, rejected
 *       matches, no previous cloud) vel_out is bit for bit omds_point_cloud_flow's for that cell against the UNMASKED previous records and
 *       object_out = 0.  label_out = the component's label.  *matched_out counts the spheres with object_out = 1, or with a non-empty
 *       window; *n_objects_matched_out the accepted objects (NULL = skip, and so for n_objects_out).  xyzr_out [cap,4], vel_out [cap,3],
 *       label_out, object_out [cap].  OMDS_ERR_INVALID_ARG before anything is written: what omds_point_cloud_flow refuses, link outside
 *       1 .. 2, a null obj, a null label_out or object_out with cap > 0.
 *   omds_set_obstacles_from_cloud_objects : everything omds_set_obstacles_from_cloud_tracked does, in the same order, with the same final
 *       list bit for bit (self-filter and padding included) and the same stored record frame; its velocity launch runs unchanged and
 *       supplies the fallback.  Between it and the install, a fixed number of launches: a slot map (cell -> list index), a lock-free
 *       union-find over the lower half of every sphere's window (the larger root hooks under the smaller, compare-and-swap; no launch
 *       waits on another wave), a flatten to labels, the component sums (equal roots are combined inside the wave and the workgroup before
 *       the 64-bit integer atomics), an ordered compaction of the roots into the component table, one wave per NOW component for the match, and
 *       one pass that overwrites the velocity of every sphere of an accepted object.  Padding spheres: velocity 0, label -1, object 0.
 *       THE PREVIOUS TABLE is the component table of the FINAL list (after the self-filter: the arm is not in it) of the last successful
 *       objects call.  There is none at the first objects call, after omds_cloud_track_reset, when there is no previous record frame on
 *       this grid (origin, voxel, dims, min_points as for the tracked call), when link or min_cells (resolved: < 1 is 1) differ from
 *       the stored table's, and after a plain tracked call, which stores its records but invalidates the table.  Without one every
 *       sphere takes the fallback, *n_objects_matched_out = -1, and the table is stored.  omds_set_obstacles_from_cloud and
 *       omds_set_obstacles leave records and table alone; a refusal (too many occupied cells, an argument check) leaves the scene, the
 *       record frame and the table exactly as they were.  A scene whose velocities are all exactly 0 keeps the static propagate.
 *   omds_get_cloud_objects : label [n_obs] and object [n_obs] of the scene in force (NULL: no copy), *n_objects_out its objects; host
 *       state, no GPU work.  OMDS_ERR_NOT_INITIALISED unless the scene in force was installed by the objects call.                    */
typedef struct {
    int32_t link;       /* cells are neighbours when their Chebyshev distance is <= link: 1 .. 2 */
    int32_t min_cells;  /* a component of fewer cells is no object; < 1 -> 1                     */
} omds_cloud_object_spec;
OMDS_API int omds_point_cloud_object_flow(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const omds_cloud_object_spec* obj,
                                          const float* xyz_prev, int64_t n_prev, const uint8_t* keep_prev, const float* xyz_now,
                                          int64_t n_now, const uint8_t* keep_now, float* xyzr_out, float* vel_out, int32_t* label_out,
                                          int32_t* object_out, int32_t cap, int32_t* count_out, int32_t* matched_out,
                                          int32_t* n_objects_out, int32_t* n_objects_matched_out);
OMDS_API int omds_set_obstacles_from_cloud_objects(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track,
                                                   const omds_cloud_object_spec* obj, const float* xyz, int64_t n_points,
                                                   int xyz_on_device, const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out,
                                                   int32_t* n_matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out);
OMDS_API int omds_get_cloud_objects(omds_ctx* ctx, int32_t* label, int32_t* object, int32_t* n_objects_out);
/* THE SCENE STRAIGHT FROM DEPTH IMAGES, SEVERAL CAMERAS.  The three cloud calls above start from xyz [P,3] in the frame of the voxel
 * grid; a depth camera delivers a uint16 (or float32) image, intrinsics and a pose, and a cell around an arm has two or three of them.
 * The depth call deprojects inside the counting pass, without ever writing a point: everything after that pass is integer sums and
 * ordered compactions, a function of the SET of points.  Additive: no other entry point changes its launches or its bits.
 * OUT OF SCOPE: range-type depth (z is depth along the optical axis; an unrectified image: THE LENS OF A DEPTH CAMERA below),
 * registration of the cameras against each other (the poses are taken as given), a motion model beyond constant velocity; smoothing
 * of positions.  (Flying pixels and speckle: THE DEPTH FILTER below; velocities smoothed over frames: THE VELOCITY FILTER below.)
 *   omds_depth_points : host only (no context, no GPU), the DEFINITION.  All fp32, every operation named one rounding.  Once per
 *       camera: ifx = 1.0f / fx, ify = 1.0f / fy.  The visited pixels are columns u and rows v in 0, step, 2 step, ... (step < 1 is 1),
 *       in row-major order, ceil(H / step) * ceil(W / step) of them; the raw value is d = image[v * pitch + u] (pitch in ELEMENTS, 0 is
 *       width).  OMDS_DEPTH_U16: d == 0 drops the pixel (no return), else z = (float)d * depth_scale.  OMDS_DEPTH_F32: z = d.  The pixel
 *       is kept only if z >= z_min && z <= z_max (NaN, +-inf, negative values and -0 fail by the comparison).  Then
 *       a = ((float)u - cx) * ifx;  b = ((float)v - cy) * ify;  xc = a * z;  yc = b * z;  and for r = 0, 1, 2
 *       w_r = fmaf(pose[4r], xc, fmaf(pose[4r+1], yc, fmaf(pose[4r+2], z, pose[4r+3]))).   z is depth along the optical axis, not
 *       range; no distortion model; R is not checked for orthonormality.  xyz_out [cap_points,3] takes one row per visited pixel, a
 *       dropped one as three NaNs (omds_point_cloud_spheres drops those); *n_valid_out = kept pixels.  OMDS_ERR_INVALID_ARG before
 *       anything is written: a camera outside the ranges of the struct (cx, cy must be finite too), null pointers, cap_points smaller
 *       than the visited count.
 *   omds_set_obstacles_from_depth : THE CONTRACT -- every effect of the call (status, every out value, the installed scene and its
 *       padding, velocities and horizon mode, labels and object flags, the stored record frame and component table) is that of
 *       omds_set_obstacles_from_cloud (track == NULL, obj == NULL) / _tracked (track) / _objects (track and obj) on the concatenation, in
 *       camera order, of omds_depth_points of each image, bit for bit.  The depth call and the cloud calls share the one stored frame
 *       and the one stored table: frames may alternate between them.  cams [n_cams], images [n_cams] (images[i]: uint16 or float
 *       elements as cams[i].format says, at least (H - 1) pitch + W of them); 1 <= n_cams <= OMDS_DEPTH_MAX_CAMERAS; the visited pixels
 *       of all cameras together at most 16 777 216 (2^24, the bound the record sums rest on), checked from the shapes before anything is
 *       read; obj without track is an argument error.  images_on_device = 0: host images, each through a staging buffer of the context
 *       by one asynchronous copy; 1: device memory on the context's device that the caller has finished writing and leaves alone until
 *       the call returns, read in place -- any base aligned to the element size and any pitch (a sliced view with an odd element offset
 *       included).  ONE launch counts all cameras (the camera table travels by value in the kernel arguments): a lane takes a run of 4
 *       consecutive visited pixels of a row, deprojects them with the functions of the definition and adds to the cell counters (the
 *       records when tracked) of the cloud calls -- equal cells are combined inside the lane and, for at most 8 rounds, across the wave
 *       before the integer atomics, which changes no bit; from there on the call IS the cloud call.  Argument refusals and the too-many-cells
 *       refusal leave the scene, the stored frame and the stored table exactly as they were.  Synchronous.                           */
#define OMDS_DEPTH_U16 0
#define OMDS_DEPTH_F32 1
#define OMDS_DEPTH_MAX_CAMERAS 8
typedef struct {
    int32_t width, height;   /* pixels, each >= 1                                                         */
    int32_t pitch;           /* ELEMENTS between row starts; 0 -> width; else >= width                    */
    int32_t format;          /* OMDS_DEPTH_U16: raw units, 0 = no return;  OMDS_DEPTH_F32: metres         */
    int32_t step;            /* visit rows and columns 0, step, 2 step, ...; < 1 -> 1                     */
    float   fx, fy, cx, cy;  /* pinhole intrinsics of the (rectified) image; fx, fy finite and != 0        */
    float   depth_scale;     /* metres per raw unit (U16 only; finite, > 0)                               */
    float   z_min, z_max;    /* range gate along the optical axis: 0 < z_min <= z_max, finite             */
    float   pose[12];        /* row-major [R | t], camera -> the frame of the voxel grid; finite          */
} omds_depth_camera;
OMDS_API int omds_depth_points(const omds_depth_camera* cam, const void* image, float* xyz_out, int64_t cap_points, int64_t* n_valid_out);
OMDS_API int omds_set_obstacles_from_depth(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track,
                                           const omds_cloud_object_spec* obj, const omds_depth_camera* cams, const void* const* images,
                                           int32_t n_cams, int images_on_device, const float* q_now, int32_t* n_spheres_out,
                                           int32_t* n_occupied_out, int32_t* n_matched_out, int32_t* n_objects_out,
                                           int32_t* n_objects_matched_out);
/* THE SCENE MEMORY OF THE DEPTH ROUTE: KEEP OCCLUDED OBSTACLES, CLEAR CELLS SEEN THROUGH (new work).  Every call above is memoryless
 * about occupancy: a cell that got no points this frame is gone, whether a camera looked through it or the arm, a dropout (raw 0) or
 * the edge of a frustum kept every camera from telling.  This route keeps one word per cell between calls and asks the cameras.
 * Additive: no other entry point changes its launches or its bits.
 * OUT OF SCOPE: velocities on THIS route (it installs a static scene; memory together with the tracked / objects routes is
 * omds_set_obstacles_from_depth_memory_tracked, below), the plain cloud route (no cameras, so no visibility), per-cell occupancy
 * probabilities or log-odds, sub-voxel footprints that follow the cell's projected size, motion compensation of the memory when the
 * grid frame moves.
 *   THE WORD: m[c] (uint32) per grid cell; 0 = empty, k >= 1 = occupied and last counted k - 1 calls ago.
 *   omds_depth_scene_memory : host only (no context, no GPU), the DEFINITION.  All fp32, every operation named one rounding.  n[c] are
 *       the counts of the depth route's counting pass (omds_depth_points of every image, cloud_cell), unchanged.  mem_in [cells] (NULL =
 *       all empty) -> mem_out [cells] (may be the same array), per cell:
 *       1. n[c] >= min_points: m' = 1, SEEN.   2. else m[c] == 0: m' = 0.   3. else every camera i = 0 .. n_cams - 1 gives a verdict on
 *       the cell centre p (the three fmaf of the cell's sphere): d_r = p_r - pose[4r+3];  xc = fmaf(pose[0], d_0, fmaf(pose[4], d_1,
 *       pose[8] * d_2)), yc with pose[1], [5], [9], zc with pose[2], [6], [10] -- R taken as orthonormal and applied transposed, NOT
 *       checked;  !(zc >= z_min && zc <= z_max): SILENT;  iz = 1.0f / zc (IEEE-rounded);  uf = fmaf(xc * iz, fx, cx), vf = fmaf(yc * iz,
 *       fy, cy);  ju = rintf(uf * istep), jv = rintf(vf * istep) with istep = 1.0f / (float)step taken once (ties to even);
 *       !(ju >= 0 && ju < nu && jv >= 0 && jv < nv), compared as floats before any conversion: SILENT;  lim = zc + clear_margin;  every
 *       visited pixel (ju + a, jv + b), |a|, |b| <= footprint, inside [0, nu) x [0, nv) reads the raw element at column (ju + a) step,
 *       row (jv + b) step: U16 with d == 0: SILENT, else z_pix = (float)d * depth_scale; F32: z_pix = the element;
 *       !(fabsf(z_pix) <= FLT_MAX && z_pix > lim): SILENT.  The range gate is deliberately not applied to z_pix: a return beyond z_max
 *       is still a return from behind the cell.  All window pixels passed: FREE.   4. any camera FREE: m' = 0, CLEARED.   5. else m' =
 *       m + 1 saturating at 0xFFFFFFFF; max_age >= 1 && m' > (uint32)max_age + 1: m' = 0, EXPIRED; else REMEMBERED -- a cell survives
 *       exactly max_age unseen calls.  counts_out [4] = cells seen, remembered, cleared, expired (NULL = skip).  No self-filter here.
 *       OMDS_ERR_INVALID_ARG before anything is written: a bad cloud spec or camera, footprint outside 0 .. 3, NaN clear_margin, null
 *       mem_spec, cams, images, an image or mem_out, n_cams outside 1 .. 8, more than 2^24 visited pixels.
 *   omds_set_obstacles_from_depth_memory : THE CONTRACT -- the candidates are the cells with m' != 0 in ascending cell order, as their
 *       spheres; with q_now the self-filter of omds_set_obstacles_from_cloud runs on them, and a candidate it drops sets m'[cell] = 0
 *       (SELF-FORGOTTEN: otherwise the arm's own past poses would haunt the scene wherever no camera can see).  The installed scene and
 *       its padding are those of omds_set_obstacles on the spheres of the final m'; the stored memory afterwards is the final m'; both
 *       are bit for bit the definition iterated from the stored memory.  The memory is keyed by origin, voxel, dims (bitwise), the
 *       resolved min_points and the resolved memory spec (clear_margin bitwise): a call on another key starts from empty memory.
 *       seen + remembered > max_spheres: OMDS_ERR_INVALID_ARG with counts_out filled ([4] = 0), scene and stored memory exactly as they
 *       were (the call writes the buffer that is not the stored one and commits behind everything that can fail); so do the argument
 *       checks.  Like every scene setter it ends an obstacle focus and clears a motion horizon.  The stored record frame and component
 *       table of the tracked / objects routes are left alone.  counts_out [5] = the four above and the self-forgotten cells (NULL =
 *       skip); *n_spheres_out = spheres before padding.  On the device: the counting pass as it is; ONE launch maps (counts, stored
 *       words) to the new words, 4 consecutive cells per lane by 16-byte loads and one 16-byte store -- a lane whose four stored words
 *       are 0 (nearly all of them) projects nothing and reads no image; the others loop the camera table, which travels by value;
 *       integer counters, reduced per wave.  Then the ordered compaction on m' != 0 with the cell indices, the self-filter, one launch
 *       that zeroes the dropped cells, one that gathers the ages.  Synchronous.
 *   omds_scene_memory_reset : forgets the stored memory; the next memory call starts from empty.
 *   omds_get_scene_memory : age [n_obs] of the scene in force: m' - 1 of every sphere's cell (0: seen in the installing call), -1 for a
 *       padding sphere and for every sphere when another setter (an obstacle focus included) installed the scene; grid [cells] = the
 *       stored words (NULL: no copy; untouched without a stored memory); *n_cells_out = cells of the stored memory, 0 without one.    */
typedef struct {
    int32_t max_age;       /* a cell unseen for more calls than this is dropped; < 1: never                          */
    float   clear_margin;  /* a return must be farther than the cell's depth + this to clear it; <= 0: the sphere radius; not NaN */
    int32_t footprint;     /* the window of a verdict is (2 footprint + 1)^2 visited pixels: 0 .. 3                   */
} omds_scene_memory_spec;
OMDS_API int omds_depth_scene_memory(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_camera* cams,
                                     const void* const* images, int32_t n_cams, const uint32_t* mem_in /* [cells] or NULL = empty */,
                                     uint32_t* mem_out /* [cells] */, int32_t counts_out[4] /* seen, remembered, cleared, expired */);
OMDS_API int omds_set_obstacles_from_depth_memory(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec,
                                                  const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                                  int images_on_device, const float* q_now, int32_t* n_spheres_out,
                                                  int32_t counts_out[5] /* the four above + self-forgotten */);
OMDS_API int omds_scene_memory_reset(omds_ctx* ctx);
OMDS_API int omds_get_scene_memory(omds_ctx* ctx, int32_t* age /* [n_obs] or NULL */, uint32_t* grid /* [cells] or NULL */,
                                   int32_t* n_cells_out);
/* THE DEPTH FILTER: FLYING PIXELS AND SPECKLE LEAVE INSIDE THE COUNTING PASS (new work).  At a depth discontinuity a camera returns
 * mixed pixels with depths between foreground and background, and in low-texture regions isolated speckle; each becomes a sphere in
 * free space that the planner bends around and the scene memory keeps.  The filter asks the neighbours of a pixel whether they see the
 * same surface, inside the counting pass of the depth routes: still no point is ever written.  Additive: with no filter set every entry
 * point keeps its launches and its bits.
 * OUT OF SCOPE: bilateral or temporal smoothing of depth VALUES (a kept pixel keeps its depth), confidence images, tolerances that
 * follow the z^2 noise model of stereo cameras (tol is affine in z).
 *   THE RULE.  All fp32, every operation named one rounding.  A visited pixel (ju, jv) that omds_depth_points keeps (return, range
 *       gate) at depth z is kept by the filter iff s >= min_support, where tol = fmaf(edge_rel, z, edge_abs) and s counts the window
 *       positions (ju + a, jv + b) with |a|, |b| <= radius, (a, b) != (0, 0), inside [0, nu) x [0, nv), whose raw element at column
 *       (ju + a) step, row (jv + b) step is a return (U16: d != 0, z_n = (float)d * depth_scale; F32: z_n = the element) with
 *       fabsf(z_n - z) <= tol (NaN fails the comparison).  The window is one of VISITED pixels: with step > 1 the neighbours are step
 *       elements apart.  Neighbours are deliberately NOT range-gated: a surface just beyond z_max still supports its neighbour, for the
 *       same reason as the scene memory's z_pix.  Positions outside the image give no support: a corner pixel at radius 1 has 3
 *       possible supporters, a border pixel 5.
 *   omds_depth_points_filtered : host only, the DEFINITION.  The output of omds_depth_points with a rejected pixel written as three
 *       NaNs; *n_valid_out = pixels kept by both, *n_rejected_out = pixels omds_depth_points keeps and the filter drops.  filt == NULL
 *       is exactly omds_depth_points (*n_rejected_out = 0 when given).  OMDS_ERR_INVALID_ARG before anything is written: as
 *       omds_depth_points, a spec outside the ranges of the struct, and with a filter a null n_rejected_out.
 *   omds_depth_scene_memory_filtered : omds_depth_scene_memory with the counts n[c] of the filtered points (filt == NULL: the same
 *       call).  Only the counts change: the verdicts of step 3 read the RAW images -- a flying pixel is still a return.
 *   omds_set_depth_filter : the filter is CONTEXT STATE, off at creation; spec == NULL turns it off.  A refused spec leaves the stored
 *       filter as it was.  omds_set_obstacles_from_depth (plain, tracked, objects) and omds_set_obstacles_from_depth_memory consult it.
 *       THE CONTRACT with a filter set -- every effect of those calls is that of the cloud call on the concatenation of
 *       omds_depth_points_filtered of each image, bit for bit; of the memory call, omds_depth_scene_memory_filtered iterated.  The filter
 *       is not part of the scene memory's key.  On the device: k_depth_count_filt / k_depth_count_filt_rec in place of the counting
 *       kernels -- a workgroup owns a tile of 32 x 32 visited pixels, stages it with a halo of radius as z_n into LDS (NaN: no return,
 *       or outside the image; every raw element read once per tile), one barrier, the support test on LDS alone, and the surviving
 *       pixels go on as before.  Integer counters, reduced per wave.
 *   omds_get_depth_filter_stats : out[0] = pixels kept, out[1] = pixels rejected by the filter in the last depth call of the context
 *       that got as far as its counting pass (the too-many-cells refusal included), summed over cameras; 0, 0 when no filter ran.    */
typedef struct {
    int32_t radius;       /* window = (2 radius + 1)^2 VISITED pixels around the pixel: 1 .. 3                             */
    int32_t min_support;  /* kept when at least this many OTHER window pixels support it: 1 .. (2 radius + 1)^2 - 1        */
    float   edge_abs;     /* metres; finite, >= 0                                                                          */
    float   edge_rel;     /* per metre of the pixel's depth; finite, >= 0                                                  */
} omds_depth_filter_spec;
OMDS_API int omds_depth_points_filtered(const omds_depth_camera* cam, const omds_depth_filter_spec* filt /* NULL: off */, const void* image,
                                        float* xyz_out, int64_t cap_points, int64_t* n_valid_out, int64_t* n_rejected_out);
OMDS_API int omds_depth_scene_memory_filtered(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec,
                                              const omds_depth_filter_spec* filt /* NULL: off */, const omds_depth_camera* cams,
                                              const void* const* images, int32_t n_cams, const uint32_t* mem_in, uint32_t* mem_out,
                                              int32_t counts_out[4]);
OMDS_API int omds_set_depth_filter(omds_ctx* ctx, const omds_depth_filter_spec* spec /* NULL: off */);
OMDS_API int omds_get_depth_filter_stats(omds_ctx* ctx, int64_t out[2] /* kept, rejected */);
/* MEMORY AND VELOCITIES IN ONE DEPTH CALL (new work).  The memory route keeps the shelf the arm reaches across and freezes the person
 * walking by; the tracked / objects routes predict the person and lose the shelf the moment it is occluded; each installs its own scene,
 * so calling both does not help.  This route does both in one call, on the stored memory, the stored record frame and the stored
 * component table that the other routes already keep.  And the two have something to tell each other: a wall cell uncovered after a few
 * occluded frames has no record in the previous frame, so the tracked route matches it with its neighbours and reports a sideways
 * velocity it does not have -- the memory knows the cell was occupied all along.  Additive: no other entry point changes its launches
 * or its bits.
 * OUT OF SCOPE: velocities for remembered cells (dead reckoning behind an occluder: a remembered sphere stands still), objects formed
 * over remembered cells, the centroid shift of an uncovered surface on the objects route, memory on the plain cloud route (no cameras),
 * a motion model beyond constant velocity; smoothing of positions.
 *   omds_depth_scene_memory_flow : host only (no context, no GPU), the DEFINITION, a composition of the definitions above.  The
 *       previous frame is given as its cameras and images (cams_prev == NULL: none); it stands for the stored record frame AND, with obj,
 *       the stored component table (the components of its kept occupied cells).  filt (NULL: off) filters both frames.
 *       1. RECORDS: those of the depth route's counting pass (omds_depth_points[_filtered] of every image, cloud_cell_sub); n[c] their count.
 *       2. WORDS: m' = omds_depth_scene_memory[_filtered] on the same images and mem_in.  The candidates are the cells with m' != 0 in
 *       cell order; keep_now [candidates] (NULL: keep all) stands for the self-filter, and a dropped candidate sets m'[cell] = 0 (counts
 *       [4]).  seen + remembered > max_spheres (or cap): OMDS_ERR_INVALID_ARG with counts_out and *count_out filled, nothing else written.
 *       3. THE SEEN SUBLIST T: the final spheres with n[c] >= min_points, in cell order.  On T the velocities and matched flags, and with
 *       obj the labels, object flags, n_objects and n_objects_matched, are those of omds_point_cloud_flow / omds_point_cloud_object_flow
 *       on the points of the two frames with keep_prev [occupied cells of the previous frame] and T as the kept cells of this one: T is
 *       that call's final list; the memory adds spheres around it and changes nothing inside it.
 *       4. PER FINAL SPHERE, LAST (it wins over an accepted object's velocity): a sphere not in T: velocity +0, not matched, label -1,
 *       object 0.  A sphere of T whose STORED word mem_in[c] >= 2 (occupied and unseen at the previous memory call): velocity +0, not
 *       matched, object 0; its label stays.  Every other sphere of T keeps step 3's values.
 *       5. xyzr_out, vel_out, age_out (m' - 1), label_out (-1 without obj), object_out [count]; *n_matched_out = final spheres whose
 *       matched flag survives step 4, -1 without a previous frame; *n_objects_matched_out = -1 without one.
 *       OMDS_ERR_INVALID_ARG before anything is written: as omds_depth_scene_memory, omds_point_cloud_flow and, with obj,
 *       omds_point_cloud_object_flow; a bad filter spec; null mem_out or count_out; cap < 0 or cap > 0 with a null output array.
 *   omds_set_obstacles_from_depth_memory_tracked : THE CONTRACT -- stored words, counts_out [5], the installed spheres and their ages
 *       are bit for bit those of omds_set_obstacles_from_depth_memory on the same stored memory (self-filter, self-forgetting and the
 *       refusal included); on T, velocities, matched flags, labels, object flags, the component table that gets stored, *n_objects_out
 *       and *n_objects_matched_out are bit for bit those of omds_set_obstacles_from_depth(track[, obj]) on the same images, q_now,
 *       stored frame and stored table; step 4 then overrides.  *n_matched_out as in step 5 (-1 without a stored frame on this grid).
 *       If every velocity is exactly 0 the horizon stays cleared (the static propagate follows); else horizon mode 1 through
 *       omds_set_obstacle_motion.  Padding spheres: velocity 0, age -1, label -1.  obj == NULL: per-cell flow only, and the stored table
 *       is invalidated as by a plain tracked call.  STATE: the route shares the one stored memory (and its key) with the memory route and
 *       the one stored record frame and component table with the tracked / objects routes; a successful call commits all of them, a
 *       refusal leaves scene, memory, frame and table exactly as they were.  Frames may alternate with every other route: the result is
 *       a function of the stored state, and dt_frame is the caller's claim about the stored frame's age.  omds_get_scene_memory reports
 *       this scene's ages, with obj omds_get_cloud_objects its labels and flags.  The context's depth filter is consulted.  On the
 *       device: ONE counting pass (into the record buffer that is not the stored frame) and ONE staging copy; k_scene_memory<uint4>,
 *       the memory kernel as a template, reads the .x of four consecutive records per lane; compaction, self-filter, forget and ages as on the memory route; one more ordered
 *       compaction of the final list to T (cell and list index); the tracked / objects launchers on T, unchanged; one launch, one lane
 *       per final sphere, carries T's results back under step 4's rule (the matched flag stays in .w: the host counts).  Synchronous.  */
OMDS_API int omds_depth_scene_memory_flow(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_cloud_track_spec* track,
                                          const omds_cloud_object_spec* obj /* NULL: per-cell flow only */,
                                          const omds_depth_filter_spec* filt /* NULL: off */, const omds_depth_camera* cams_prev /* NULL: none */,
                                          const void* const* images_prev, int32_t n_cams_prev, const uint8_t* keep_prev,
                                          const omds_depth_camera* cams, const void* const* images, int32_t n_cams, const uint8_t* keep_now,
                                          const uint32_t* mem_in /* [cells] or NULL = empty */, uint32_t* mem_out /* [cells] */,
                                          int32_t counts_out[5], float* xyzr_out /* [cap,4] */, float* vel_out /* [cap,3] */,
                                          int32_t* age_out, int32_t* label_out, int32_t* object_out /* [cap] each */, int32_t cap,
                                          int32_t* count_out, int32_t* n_matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out);
OMDS_API int omds_set_obstacles_from_depth_memory_tracked(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec,
                                                          const omds_cloud_track_spec* track, const omds_cloud_object_spec* obj /* NULL: per-cell flow only */,
                                                          const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                                          int images_on_device, const float* q_now, int32_t* n_spheres_out,
                                                          int32_t counts_out[5], int32_t* n_matched_out, int32_t* n_objects_out,
                                                          int32_t* n_objects_matched_out);
/* THE LENS OF A DEPTH CAMERA: UNRECTIFIED IMAGES INSIDE THE DEPTH ROUTES (new work).  Stereo cameras deliver rectified depth;
 * time-of-flight cameras and every simulated camera with a lens model deliver the raw image and Brown-Conrady coefficients.  The ray of
 * a pixel is a property of the camera, not of the frame: a per-camera table of rays that the counting pass reads in place of
 * ((float)u - cx) * ifx, and the closed-form forward model where the scene memory projects a cell centre.  Additive: with no lens set
 * every entry point keeps its launches and its bits, and omds_depth_camera keeps its layout.
 * OUT OF SCOPE: range-type depth, fisheye (Kannala-Brandt), thin-prism and tilt terms, caller-supplied ray tables, models that fold
 * back inside the image, resampling an image to a rectified one, registration of the cameras against each other.
 *   THE MODEL (csrc/depth_lens_def.h).  All fp32, every operation named one rounding, IEEE division.  OpenCV's rational model,
 *       k = k1 k2 p1 p2 k3 k4 k5 k6 (plumb-bob: k4 = k5 = k6 = 0).  With r2 = fmaf(a, a, b * b), num = 1 + k1 r2 + k2 r2^2 + k3 r2^3 and
 *       den = 1 + k4 r2 + k5 r2^2 + k6 r2^3 in Horner form (fmaf), dx = fmaf(2 p1, a b, p2 fmaf(2, a a, r2)) and
 *       dy = fmaf(2 p2, a b, p1 fmaf(2, b b, r2)):
 *       FORWARD (a, b) -> (ad, bd): s = num / den; ad = fmaf(a, s, dx); bd = fmaf(b, s, dy); the pixel is (fx ad + cx, fy bd + cy).
 *       INVERSE, the ray of visited pixel (u, v): x0 = ((float)u - cx) * ifx, y0 likewise; (x, y) = (x0, y0); exactly `iters` rounds of
 *       ic = den / num; x = (x0 - dx) * ic; y = (y0 - dy) * ic (num, den, dx, dy at the current (x, y)); then FORWARD at (x, y): the ray is
 *       (x, y) iff s > 0 && fabsf((ad - x0) * fx) <= max_residual && fabsf((bd - y0) * fy) <= max_residual (NaN fails), else the pixel
 *       has NO RAY, stored as (NaN, NaN).  With all eight coefficients zero the ray is (x0, y0) exactly.  Plumb-bob (-0.3, 0.1, 1e-3,
 *       -5e-4) at 640 x 480, fx 600 is within 1.1e-4 px after 10 rounds; a Kinect-NFOV-like rational set within 2.4e-4 px after 20.
 *   omds_depth_lens_rays : host only, the table of the visited pixels, row-major: ab_out [nv * nu][2]; *r2_max_out = the largest
 *       fmaf(a, a, b * b) over the valid entries (0 when there is none), *n_invalid_out = the pixels without a ray (either may be
 *       NULL).  lens == NULL or model 0: the pinhole rays.
 *   omds_depth_points_lens : host only, the DEFINITION: omds_depth_points_filtered with xc = a * z, yc = b * z from the pixel's ray,
 *       then the same three pose fmafs.  A pixel that passes the gate and the filter but has no ray is three NaNs, counted neither as
 *       valid nor as rejected; it is still a return for the filter's support test and for the memory's verdicts, which read raw depths
 *       and never rays.  lens == NULL or model 0: exactly omds_depth_points_filtered.
 *   omds_depth_scene_memory_lens : omds_depth_scene_memory_filtered with lenses [n_cams] (NULL: none).  The counts come from the lens
 *       points.  In a verdict of a camera with a lens, after iz: a = xc * iz; b = yc * iz; !(fmaf(a, a, b * b) <= r2_max) is SILENT
 *       (beyond the table's field of view the polynomial may fold back; SILENT never clears a cell); otherwise
 *       uf = fmaf(ad, fx, cx), vf = fmaf(bd, fy, cy) from FORWARD, and from rintf on everything is as without a lens.
 *   omds_depth_scene_memory_flow_lens : omds_depth_scene_memory_flow composed from the two above; lenses_prev [n_cams_prev], lenses
 *       [n_cams], either may be NULL.
 *   omds_set_depth_lenses : CONTEXT STATE like the depth filter, off at creation: lens i belongs to camera i of every later depth call
 *       (plain, tracked, objects, memory, memory-tracked, with or without the depth filter); a camera index >= n, or an entry of model
 *       0, is pinhole.  0 <= n <= OMDS_DEPTH_MAX_CAMERAS; lenses == NULL or n == 0 turns lenses off.  A refused array leaves the stored
 *       lenses as they were.  THE CONTRACT with lenses set -- every effect of a depth call is that of the cloud call on the concatenated
 *       omds_depth_points_lens of each image, bit for bit; of the memory calls, omds_depth_scene_memory[_flow]_lens iterated;
 *       omds_get_depth_filter_stats counts a pixel without a ray neither as kept nor as rejected.  The lenses are not part of the scene
 *       memory's key or the velocity filter's.  On the device: the table of a slot lives in the context under the bitwise key (width,
 *       height, step, fx, fy, cx, cy, lens); k_depth_rays builds it on the context's stream in the first depth call that needs it (one
 *       lane per visited pixel, one 8-byte store, r2_max as an integer maximum on the float's bits) and only a changed key rebuilds it:
 *       a camera whose pose changes every frame never does.  The counting kernels and k_scene_memory have lens forms, launched only when
 *       some camera of the call has a lens; without one every call enqueues the launches it always did.  A call refused for too many
 *       cells may keep a freshly built table: a cache, not scene state.
 *   omds_get_depth_lens_table : the device table of slot i as the last depth call that needed one left it: ab_out [n_entries][2] (NULL:
 *       not fetched), its r2_max, its pixels without a ray, and *n_entries_out = nv * nu, 0 when the slot holds no table.          */
typedef struct {
    int32_t model;         /* 0: none (pinhole arithmetic, no table); 1: rational Brown-Conrady                              */
    float   k[8];          /* k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order); finite                                               */
    int32_t iters;         /* rounds of the fixed-point inverse, <= 64; < 1: the default, 20                                 */
    float   max_residual;  /* pixels: a ray whose forward image misses its pixel by more has no ray; finite; <= 0: 0.01      */
} omds_depth_lens;
OMDS_API int omds_depth_lens_rays(const omds_depth_camera* cam, const omds_depth_lens* lens, float* ab_out /* [nv*nu,2] */, float* r2_max_out,
                                  int64_t* n_invalid_out);
OMDS_API int omds_depth_points_lens(const omds_depth_camera* cam, const omds_depth_lens* lens /* NULL: none */,
                                    const omds_depth_filter_spec* filt /* NULL: off */, const void* image, float* xyz_out, int64_t cap_points,
                                    int64_t* n_valid_out, int64_t* n_rejected_out);
OMDS_API int omds_depth_scene_memory_lens(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec,
                                          const omds_depth_filter_spec* filt /* NULL: off */, const omds_depth_lens* lenses /* [n_cams] or NULL */,
                                          const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                          const uint32_t* mem_in /* [cells] or NULL = empty */, uint32_t* mem_out /* [cells] */,
                                          int32_t counts_out[4]);
OMDS_API int omds_depth_scene_memory_flow_lens(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec,
                                               const omds_cloud_track_spec* track, const omds_cloud_object_spec* obj,
                                               const omds_depth_filter_spec* filt, const omds_depth_lens* lenses_prev,
                                               const omds_depth_camera* cams_prev, const void* const* images_prev, int32_t n_cams_prev,
                                               const uint8_t* keep_prev, const omds_depth_lens* lenses, const omds_depth_camera* cams,
                                               const void* const* images, int32_t n_cams, const uint8_t* keep_now, const uint32_t* mem_in,
                                               uint32_t* mem_out, int32_t counts_out[5], float* xyzr_out, float* vel_out, int32_t* age_out,
                                               int32_t* label_out, int32_t* object_out, int32_t cap, int32_t* count_out,
                                               int32_t* n_matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out);
OMDS_API int omds_set_depth_lenses(omds_ctx* ctx, const omds_depth_lens* lenses /* [n] or NULL: off */, int32_t n);
OMDS_API int omds_get_depth_lens_table(omds_ctx* ctx, int32_t i, float* ab_out /* [n_entries,2] or NULL */, float* r2_max_out,
                                       int64_t* n_invalid_out, int64_t* n_entries_out);
/* THE VELOCITY FILTER: SENSED SPHERE VELOCITIES SMOOTHED OVER FRAMES (new work).  Every velocity route above estimates from two frames
 * only, and omds_set_obstacle_motion extrapolates that one estimate over the whole horizon: at H = 32 a one-frame error is multiplied
 * by the horizon before pass 1 sees the predicted spheres.  The filter keeps one smoothed velocity per grid cell between calls and
 * blends every new estimate against its predecessor, on the device.  Additive: with no filter set every entry point keeps its launches
 * and its bits.
 * OUT OF SCOPE: a motion model beyond constant velocity; smoothing of positions (the spheres stay the cell centres of this frame);
 * compensation of the state when the grid frame moves.
 *   THE STATE: per grid cell four int32 (q_x, q_y, q_z, hits).  hits == 0: no history.  hits >= 1: q is the smoothed velocity in units
 *       of 2^-16 m/s and hits the frames behind it, saturating at 255.
 *   omds_velocity_filter_step : host only (no context, no GPU), the DEFINITION.  All fp32, every operation named one rounding, every
 *       conversion to float round-to-nearest; all sums are integers.  INPUTS: cell [n] the cells of the final list, ascending, without
 *       padding; raw [n,3] its velocities as the route computes them (the still rule applied); live [n] (NULL: all 1): 1 where the
 *       route's matched flag is set (a non-empty window, or the sphere moves with an accepted object, and the memory route did not force
 *       it still); group [n] (NULL: none): the sphere's label where it moves with an accepted object, else -1.  state_in [cells,4] (NULL:
 *       all empty) -> state_out [cells,4] (may be the same array).
 *       1. PREDECESSOR of sphere i: over the cells j = cell_i + k, |k_c| <= reach (the track spec's) on all axes, inside the grid, whose
 *       state_in has hits >= 1: d2 = k . k, m = min d2, T = {j : d2 = m};  S_c = sum_T q_jc (int64), t = |T|, h = min_T hits_j.  An empty
 *       window: h = 0.   2. GROUPS: per group, over its live spheres with h_i > 0:  G_c = sum S_ic,  Gt = sum t_i (int64),  Gh = min h_i
 *       (0 when there are none).  A grouped sphere uses (G, Gt, Gh) in place of its own (S, t, h): every sphere of an object blends
 *       against one predecessor and, the raw velocity of an object being one, receives one velocity -- the objects route stays rigid.
 *       3. BLEND, for a live sphere.  h == 0: v = raw, hits' = 1.  Else  p_c = ((float)S_c / (float)t) * 1.52587890625e-5f;
 *       a = fmaxf(alpha, 1.0f / (float)(h + 1)) with alpha_object for a grouped sphere;  d_c = raw_c - p_c;  j2 = fmaf(d_z, d_z,
 *       fmaf(d_y, d_y, d_x * d_x)).  max_jump > 0 && j2 > max_jump * max_jump: v = raw, hits' = 1, a RESTART.  Else a >= 1.0f: v = raw;
 *       else v_c = fmaf(a, d_c, p_c); in both hits' = min(h + 1, 255).  The 1 / (h + 1) term makes the first frames a running mean, so
 *       that the filter converges at the rate of the data and not of alpha.   4. state_out[cell_i] = ((int)rintf(fminf(fmaxf(v_c,
 *       -1024.f), 1024.f) * 65536.0f), hits'); vel_out [n,3] is v behind the still rule of omds_point_cloud_flow (the stored q is not
 *       zeroed by it).  A sphere with live == 0 outputs +0 and stores nothing; every cell not written is hits = 0 in state_out.
 *       stats_out [3] (NULL = skip): the live spheres that had a predecessor (h > 0, restarts included), the restarts, the groups with
 *       history.  OMDS_ERR_INVALID_ARG before anything is written: a bad cloud, track or filter spec, n < 0, cell not strictly ascending
 *       or outside the grid, a group outside -1 .. cells - 1, a null state_out, null cell, raw or vel_out with n > 0.
 *   omds_set_velocity_filter : the filter is CONTEXT STATE, off at creation; spec == NULL turns it off and empties the history.  A
 *       refused spec leaves the stored filter as it was.  omds_set_obstacles_from_cloud_tracked / _objects, omds_set_obstacles_from_depth
 *       with track (and obj) and omds_set_obstacles_from_depth_memory_tracked consult it.  THE CONTRACT with a filter set -- a filtered
 *       call is the unfiltered call, bit for bit, in everything except the velocities it installs: the scene and its padding, labels and
 *       flags, the stored records, table and memory, every out value (*n_matched_out keeps its meaning).  The installed velocities and
 *       the stored state are omds_velocity_filter_step on the stored state and on that call's final list (cells, raw velocities, matched
 *       flags, and label where the object flag is set).  Padding spheres stay at 0.  A scene whose OUTPUT velocities are all exactly 0
 *       keeps the cleared horizon and the static propagate.  The state is keyed like the stored record frame (origin, voxel, dims
 *       bitwise, resolved min_points) plus the resolved filter spec, bitwise; it is shared by all those routes, which may alternate.
 *       THE HISTORY IS EMPTY after a call on another key, after a call without a previous frame (*n_matched_out == -1), after
 *       omds_cloud_track_reset and after clearing the filter.  The state is written in the buffer that is not the stored one and
 *       committed with the frame, behind everything that can fail: a refused call leaves it as it was.  On the device, between the
 *       velocity launches (which run unchanged) and the install: k_vel_pred, one wave per sphere -- the own cell first (d2 = 0 is the
 *       unique minimum), else the lanes stride the clipped window, a wave minimum and shuffle-added integer sums; k_vel_group (only with
 *       an object spec), one lane per sphere, equal groups combined inside the wave and the workgroup before the 64-bit integer atomics at the list index
 *       of the label's cell; k_vel_blend, one lane per sphere: the fp32 lines, the velocity with the matched flag kept, one 16-byte
 *       state store.  In front of them one launch empties the cells the written buffer last held.
 *   omds_get_velocity_filter : *spec_out = the spec in force as it was given, *on_out = 1 while one is set (either may be NULL).
 *   omds_get_velocity_filter_frame : raw [n_obs,3] and live [n_obs] of the scene in force: the unfiltered velocities and matched flags of
 *       the call that installed it (padding: 0), stats [3] its counts as stats_out above (each may be NULL); host state, no GPU work.
 *       OMDS_ERR_NOT_INITIALISED unless a filtered call installed the scene in force.
 *   omds_get_velocity_filter_state : grid [cells,4] = the stored state (NULL: no copy; untouched without one); *n_cells_out = its cells,
 *       0 while the history is empty for want of a key.                                                                              */
typedef struct {
    float alpha;         /* weight of the new estimate once the running mean has passed it: finite, in (0, 1]     */
    float alpha_object;  /* ... for a sphere that moves with an accepted object; <= 0: alpha; else in (0, 1]      */
    float max_jump;      /* m/s; a new estimate farther than this from its predecessor restarts; <= 0: off; not NaN */
} omds_velocity_filter_spec;
OMDS_API int omds_velocity_filter_step(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const omds_velocity_filter_spec* filt,
                                       const int32_t* state_in /* [cells,4] or NULL = empty */, const int32_t* cell /* [n] */,
                                       const float* raw /* [n,3] */, const int32_t* live /* [n] or NULL: all */,
                                       const int32_t* group /* [n] or NULL: none */, int32_t n, float* vel_out /* [n,3] */,
                                       int32_t* state_out /* [cells,4] */, int32_t stats_out[3] /* with history, restarts, groups */);
OMDS_API int omds_set_velocity_filter(omds_ctx* ctx, const omds_velocity_filter_spec* spec /* NULL: off */);
OMDS_API int omds_get_velocity_filter(omds_ctx* ctx, omds_velocity_filter_spec* spec_out, int32_t* on_out);
OMDS_API int omds_get_velocity_filter_frame(omds_ctx* ctx, float* raw /* [n_obs,3] */, int32_t* live /* [n_obs] */, int32_t stats[3]);
OMDS_API int omds_get_velocity_filter_state(omds_ctx* ctx, int32_t* grid /* [cells,4] or NULL */, int32_t* n_cells_out);
/* THE OBSTACLE FOCUS (new work).  A sensed scene has thousands of spheres; everything behind pass 1 uses the n_closest nearest per
 * (rollout, step).  A focus call evaluates the distance of every sphere of the scene at ONE joint state, selects the near ones and
 * installs them as the scene in force, on the device; the full scene (the MASTER) is kept, so that the next call selects from it again
 * -- at every planner iteration, without a new camera frame.  Additive: without a focus call every entry point keeps its launches and
 * its bits.
 *   omds_obstacle_focus_select : host only (no context, no GPU), the DEFINITION.  All fp32, every operation named one rounding.
 *       REACH: with vel == NULL r_o = d_o; else s2 = fmaf(v_z, v_z, fmaf(v_y, v_y, v_x * v_x)), speed = sqrtf(s2),
 *       r_o = fmaf(-speed, lookahead, d_o).  A NaN r_o counts as -inf (such a sphere is always kept, like the self-filter's "a NaN
 *       distance keeps the sphere").  ORDER: by (r_o, o) -- the fp32 comparison decides, -0 equals +0, ties go to the smaller index.
 *       THRESHOLD: t = the reach of the n_closest-th sphere of that order.  PASSING: with margin == +inf every sphere passes; else
 *       bar = t + margin and a sphere passes when r_o <= bar; P of them (>= n_closest).  KEPT: M = min(P, max_keep), or P without a cap;
 *       the first M spheres of the order, listed in idx_out in ASCENDING INDEX; *kept_out = M, *passed_out = P.  A function of the
 *       values only.  OMDS_ERR_INVALID_ARG before anything is written: a bad spec, n_obs < n_closest, n_closest < 1, null pointers
 *       (vel may be NULL).  cap < M: OMDS_ERR_INVALID_ARG with both counts set and idx_out untouched.
 *   omds_focus_obstacles : THE MASTER is the scene in force with its motion velocities (horizon mode 1) when no focus is in force, else
 *       the one already stored; it lives on the device (spheres, velocities) and on the host (with the labels and flags of an objects
 *       scene).  d_o is pass 1's value at (q, master sphere o): the fp32 pass-1 kernel over one state with the master as its obstacle
 *       rows, bit for bit the mindist row of omds_dist_grad(q, 1) on the master.  It needs a network (else OMDS_ERR_NOT_INITIALISED) of
 *       hidden width <= 256 (else OMDS_ERR_UNSUPPORTED) and a scene (else OMDS_ERR_NOT_INITIALISED) of at most 2^30 spheres;
 *       planar-point networks take v_z = 0, as the horizon does.  The selection: integer keys that carry the order of the reaches
 *       (NaN as -inf, -0 as +0), an exact k-th-smallest run twice on them (n_closest, then M) by ONE workgroup of 1024 lanes -- a
 *       radix select over 256-bin LDS histograms, the keys read from global memory in every pass, so any count takes the same path --
 *       and the ordered compaction of the cloud calls, which emits the kept spheres in ascending index with their master indices and
 *       velocities; the group of keys equal to the last kept one is cut by index.  Integer adds only: nothing depends on scheduling.
 *       Only the M kept items travel to the host.  The kept list goes in through the body of omds_set_obstacles (buffers, the cleared
 *       horizon, the screening notification as for any setter; the capacity stays at the master's); the kept velocities through the
 *       body of omds_set_obstacle_motion when the master is in mode 1 AND some kept component is non-zero, else the horizon stays
 *       cleared and the propagate that follows is the static one (the cloud calls' rule).  The labels and flags of an objects master
 *       are gathered: omds_get_cloud_objects, omds_get_obstacles and omds_get_obstacle_motion answer for the scene in force
 *       (*n_objects_out stays the master's).  kept_out, passed_out: M and P (NULL = skip).  Synchronous.
 *       THE CONTRACT: after a successful call every entry point behaves as on a context that was given omds_set_obstacles(master[idx])
 *       and, where motion is installed, omds_set_obstacle_motion(vel[idx]) -- propagate on every route, omds_dist_grad, cost, update,
 *       bit for bit.  The call says NOTHING about whether that equals the propagate on the full master: equality holds exactly when no
 *       dropped sphere would have entered a (rollout, step)'s n_closest; margin is the caller's bet on how much a distance can change
 *       over (H - 1) dt of joint motion (lookahead: the seconds a moving sphere is given to approach); it is measured by
 *       tools/studies/obstacle_focus_cost.py (EXPERIMENTS R22), not proven.
 *       STATE: any scene setter (omds_set_obstacles, the three cloud calls, the depth call) ends the focus; its scene is the next
 *       master.  While a focus is in force omds_set_obstacle_motion and omds_set_obstacle_horizon return OMDS_ERR_UNSUPPORTED for every
 *       argument, NULL included (they would address the subset and be lost at the next focus; omds_clear_obstacle_focus first).  A
 *       master with an explicit horizon table (mode 2): OMDS_ERR_UNSUPPORTED, the scene stays as it was.  The stored cloud frame, the
 *       component table and the moving-frame preference are untouched.  Argument refusals leave the scene, the master and the focus
 *       exactly as they were; a HIP failure later in the call leaves the context without a scene.
 *       SCREENING: a focus that changes the sphere count discards a measured calibration, as any setter does (a calibration every
 *       planner iteration costs more than the focus saves): a caller who screens sets a fixed eps > 0 (omds_set_screening).
 *   A FOCUS ALONG A PATH.  One state makes margin cover everything a rollout travels in (H - 1) dt; the planner knows where its
 *   rollouts went last iteration.  A focus over B states keeps what EACH state needs, and margin covers only the deviation from them.
 *   omds_obstacle_focus_select_path : host only, the DEFINITION over d [n_states][n_obs] (state-major), ahead [n_states] seconds or
 *       NULL, vel [n_obs][3] or NULL.  All fp32, every operation named one rounding.  SPEED: s_o = sqrtf(s2) as above.  TIME:
 *       L_b = lookahead + ahead_b (NULL: lookahead).  REACH: r_bo = d_bo without vel, else fmaf(-s_o, L_b, d_bo): a lower bound on the
 *       distance the sphere can have when state b is reached; NaN as -inf, -0 as +0.  THRESHOLD per state: t_b = the reach of the
 *       n_closest-th sphere of row b ordered by (r_bo, o); bar_b = t_b + margin.  PASSING: sphere o passes when r_bo <= bar_b for SOME
 *       b; margin == +inf: every sphere; P of them (>= n_closest).  NEAREST: m_o = min_b r_bo.  KEPT: M = min(P, max_keep), or P; the
 *       first M PASSING spheres of the order (m_o, o), listed in ascending index.  Minimum and OR over the states: their order does not
 *       matter, nor does a state given twice; n_states == 1 with ahead NULL or {0} is omds_obstacle_focus_select.  Refusals as there,
 *       and: n_states < 1, an ahead_b that is negative, NaN or infinite (checked without vel too).
 *   omds_focus_obstacles_path : omds_focus_obstacles over q_path [n_states][n_dof] (host), 1 <= n_states <= 65536, ahead as above:
 *       the same master, refusals, install, static rule, label gather, screening note, state rules and CONTRACT; omds_get_obstacle_focus
 *       and omds_clear_obstacle_focus serve both.  d_bo is pass 1's value at (q_b, master sphere o), bit for bit row b of the mindist
 *       matrix of omds_dist_grad(q_path, n_states) on the master.  The states go through the fp32 pass 1 in chunks of at most
 *       min(n_traj, 4096) states (what the context's buffers hold; every size class of pass 1 computes the same bits): per chunk the
 *       keys in place over pass 1's rows, one workgroup per row for its bar (the same k-th-smallest), and a merge of "passes in some
 *       row" and "nearest key" into two words per sphere by integer atomic OR and minimum, which nothing reads back; after the last
 *       chunk the selection above on (passing ? nearest key : 0xffffffff, above every key) and the same compaction.  The result
 *       depends neither on the chunk size nor on scheduling.  omds_focus_obstacles itself keeps its launches and its bits.
 *   omds_get_obstacle_focus : the master index of every sphere in force into idx [n_obs] (NULL: no copy; untouched without a focus);
 *       *n_master_out = the master's size, 0 when no focus is in force; *n_kept_out = n_obs.  Host state, no GPU work.
 *   omds_clear_obstacle_focus : puts the master and its motion (and labels) back; a no-op without a focus.                            */
typedef struct {
    float   margin;     /* >= 0, or +inf (every sphere passes); NaN or negative: OMDS_ERR_INVALID_ARG        */
    float   lookahead;  /* seconds a moving sphere is given to approach; >= 0 and finite                    */
    int32_t max_keep;   /* at most this many spheres; < 1: no cap; else >= n_closest, or OMDS_ERR_INVALID_ARG */
} omds_obstacle_focus_spec;
OMDS_API int omds_obstacle_focus_select(const omds_obstacle_focus_spec* spec, const float* d, const float* vel /* [O,3] or NULL */,
                                        int n_obs, int n_closest, int32_t* idx_out /* [cap] */, int32_t cap, int32_t* kept_out,
                                        int32_t* passed_out);
OMDS_API int omds_focus_obstacles(omds_ctx* ctx, const omds_obstacle_focus_spec* spec, const float* q /* [n_dof] */, int32_t* kept_out,
                                  int32_t* passed_out);
OMDS_API int omds_obstacle_focus_select_path(const omds_obstacle_focus_spec* spec, const float* d /* [n_states][O] */,
                                             const float* ahead /* [n_states] or NULL */, const float* vel /* [O,3] or NULL */,
                                             int n_states, int n_obs, int n_closest, int32_t* idx_out /* [cap] */, int32_t cap,
                                             int32_t* kept_out, int32_t* passed_out);
OMDS_API int omds_focus_obstacles_path(omds_ctx* ctx, const omds_obstacle_focus_spec* spec, const float* q_path /* [n_states][n_dof] */,
                                       const float* ahead /* [n_states] or NULL */, int n_states, int32_t* kept_out,
                                       int32_t* passed_out);
OMDS_API int omds_get_obstacle_focus(omds_ctx* ctx, int32_t* idx /* [n_obs] or NULL */, int32_t* n_master_out, int32_t* n_kept_out);
OMDS_API int omds_clear_obstacle_focus(omds_ctx* ctx);
/* LinDS(q_goal) / MPPI.reset_DS / switch_DS_idx (LinDS.py:7-10, MPPI.py:76-84). */
OMDS_API int omds_set_ds(omds_ctx* ctx, const float* q_goal);
/* MPPI_toy's nominal DS (MPPI_toy.py:89-91): velocity = (q - q_goal) @ A, A [n,n] row-major, not
 * normalised.  A == NULL switches back to LinDS.                                            */
OMDS_API int omds_set_ds_matrix(omds_ctx* ctx, const float* q_goal, const float* A);
/* SEDS nominal DS (ds_mppi/functions/SEDS.py:8-74): a Gaussian mixture regression x -> velocity on x = q - q_goal with
 * G components.  The caller passes the quantities SEDS.__init__ / GMR derive from the .mat file (so that a caller who
 * derives them like the reference -- torch.inverse / torch.det in float32 -- gets the reference's numbers):
 *   mu_in [G][n]      Mu[:n, j]                          b [G][n]          Mu[n:, j]
 *   sigma_inv [G][n][n]  inverse(Sigma[:n,:n,j])         A [G][n][n]       Sigma[n:,:n,j] @ inverse(Sigma[:n,:n,j])
 *   prior [G]         Priors[j]                          den [G]           sqrt(2 pi^n |det Sigma[:n,:n,j]| + 1e-100)
 * velocity (SEDS.get_velocity): beta_j = clamp(nan_to_num(prior_j N_j / sum), 1e-8), y = sum_j beta_j (b_j + A_j (x - mu_j));
 * farther than lin_thr from the goal: y / |y|, or -x / |x| where |y| < seds_thr.  G = 0 switches back to LinDS.            */
OMDS_API int omds_set_ds_seds(omds_ctx* ctx, const float* q_goal, int n_gauss, const float* mu_in, const float* b,
                              const float* sigma_inv, const float* A, const float* prior, const float* den,
                              float lin_thr, float seds_thr);
OMDS_API int omds_set_params(omds_ctx* ctx, const omds_params* p);
/* Cost(q_f, dh_params) + the q_min/q_max attributes (cost.py:5-12): dh_params [n+1,4]
 * rows (d, theta, a, alpha); q_min/q_max [n].                                             */
OMDS_API int omds_set_cost(omds_ctx* ctx, const float* dh_params, const float* q_min, const float* q_max);

/* TensorPolicyMPPI.sample_policy (policy.py:51-74) with injected samples (parity runs):
 * mu [N,K,n], sigma [N,K], alpha [N,K,n] = the first K kernels of mu_tmp/sigma_tmp/alpha_tmp. */
OMDS_API int omds_set_policy_samples(omds_ctx* ctx, const float* mu, const float* sigma, const float* alpha,
                                     int n_kernels);
/* TensorPolicyMPPI.sample_policy on the device (Philox4x32-10 + Box-Muller): theta_tmp =
 * N(0, theta_s) + theta_c; mean arrays are [K,n], [K], [K,n].  rollout_offset = global index
 * of this shard's rollout 0 (the global rollout 0 gets alpha_tmp = alpha_c, policy.py:74).
 * Draws: Philox4x32-10, key (seed lo, seed hi), counter (g lo, g hi, kernel, block c) with g = rollout_offset + rollout as 64 bits,
 * so a sample depends on (seed, g, kernel) only.  Block c gives the normals z[4c .. 4c+3] = r cos t, r sin t of words (0, 1), then of
 * words (2, 3), with r = sqrt(-2 ln((w_a + 1) 2^-32)), t = 2 pi w_b 2^-32; mu_j takes z[j], sigma z[n], alpha_j z[n+1+j]
 * (tests/philox_ref.py restates it, tests/test_gpu_random_draws.py holds the device to it). */
OMDS_API int omds_sample_policy(omds_ctx* ctx, const float* mu_c, const float* sigma_c, const float* alpha_c,
                                float mu_s, float sigma_s, float alpha_s, int n_kernels, uint64_t seed,
                                int64_t rollout_offset);
/* Read back the sampled tensors in the reference layout (first K kernels). NULL = skip. */
OMDS_API int omds_get_policy_samples(omds_ctx* ctx, float* mu, float* sigma, float* alpha);

/* MPPI.propagate (MPPI.py:97-224).  q_cur is [n] (broadcast to all rollouts, per_rollout = 0)
 * or [N,n] (per-rollout start states, per_rollout = 1: used for teacher-forced parity tests). */
OMDS_API int omds_propagate(omds_ctx* ctx, const float* q_cur, int per_rollout);
/* The 5-tuple returned by propagate() plus its side outputs, reference layouts:
 * all_traj [N,H,n], closest_dist_all [N,H], kernel_val_all [N,H,K], dot_products [N,H],
 * kernel_activations [N,H], qdot [N,n], normal [N,H,n] (= norm_basis[..., 0]).  NULL = skip. */
OMDS_API int omds_get_rollouts(omds_ctx* ctx, float* all_traj, float* closest_dist_all, float* kernel_val_all,
                               float* dot_products, float* kernel_activations, float* qdot, float* normal);

/* The same outputs for `count` chosen rollouts t[count] only: all_traj [count,H,n], ..., qdot [count,n], normal [count,H,n] (NULL =
 * skip).  What the reference's planner loop reads per iteration is a few rollouts -- the best one for its FK payload, the one a new
 * kernel centre came from (frankaPlanner.py:147-168: closests_dist_all[i, h], norm_basis[i, h], all_traj[best_idx]) -- so a driver
 * need not move the N x H tensors across PCIe at all.                                                                     */
OMDS_API int omds_get_rollout_rows(omds_ctx* ctx, const int32_t* t, int count, float* all_traj, float* closest_dist_all,
                                   float* kernel_val_all, float* dot_products, float* kernel_activations, float* qdot, float* normal);

/* MPPI.distance_repulsion_nn on an arbitrary batch (MPPI.py:227-282): q [B,n], B <= N.
 * Outputs (NULL = skip): distance [B], nn_grad [B,n], mindist [B,O] (pass-1 matrix),
 * closest_idx [B,k] (ascending distance).  Also serves update_kernel_normal_bases (:284-304). */
OMDS_API int omds_dist_grad(omds_ctx* ctx, const float* q, int batch, float* distance, float* nn_grad,
                            float* mindist, int32_t* closest_idx);
/* MLPRegression.forward on raw rows (network_macros_mod.py:137-146) and the vjp of the
 * arg-min output (robot_sdf.py:153-158): x [B,n+3]; y [B,C], grad [B,n+3], min_idx [B]. B <= N*k. */
OMDS_API int omds_mlp_forward_vjp(omds_ctx* ctx, const float* x, int batch, float* y, float* grad,
                                  int32_t* min_idx);
/* RobotSdfCollisionNet.compute_signed_distance_wgrad with a column list (mlp_learn/sdf/robot_sdf.py:68-100): the Jacobian columns of
 * the listed raw outputs, one backward per column as the reference's loop of .backward() calls does.  x [B,n+3]; cols [n_cols],
 * 0 <= cols[k] < C, 1 <= n_cols <= 16; y [B,C] or NULL; jac [B, n+3, n_cols] (the reference's grads[:, :, k]). B <= N*k.   */
OMDS_API int omds_mlp_jacobian(omds_ctx* ctx, const float* x, int batch, const int32_t* cols, int n_cols, float* y,
                               float* jac);

/* MPPI.get_cost -> Cost.evaluate_costs (MPPI.py:315-317, cost.py:13-22). cost_out [N] or NULL. */
OMDS_API int omds_cost(omds_ctx* ctx, float* cost_out);
/* Cost.evaluate_costs on caller-supplied tensors (cost.py:13-22 evaluates exactly what it is given): all_traj
 * [B,H,n], closest_dist_all [B,H], B <= n_traj; cost_out [B].  Evaluated on the device; the context's own rollouts and
 * their cost stay untouched.                                                                                   */
OMDS_API int omds_cost_eval(omds_ctx* ctx, const float* all_traj, const float* closest_dist_all, int batch,
                            float* cost_out);
/* MPPI.shift_policy_means + TensorPolicyMPPI.update_policy (MPPI.py:331-345,
 * policy.py:88-113), single-shard form.  mu_c/sigma_c/alpha_c: in/out host means of the first K
 * kernels; mask_out [K] (1 = updated); weights_out [N] (normalised MPPI weights) or NULL.   */
OMDS_API int omds_weighted_update(omds_ctx* ctx, float rate, float ker_thr, float* mu_c, float* sigma_c,
                                  float* alpha_c, int32_t* mask_out, float* weights_out);
/* The same update on caller-supplied tensors (MPPI.shift_policy_means reads self.cost, self.kernel_val_all and
 * self.kernel_activations, MPPI.py:333-341), the way omds_cost_eval serves Cost.evaluate_costs: cost [N], kernel_val_all [N,H,K],
 * kernel_activations [N,H] in the reference layouts (K = the kernel count of the policy samples the context holds; they are the
 * theta_tmp of the update).  The context's own rollouts, cost and running maxima stay untouched.  Teacher-forced parity: the
 * reference's own rollout tensors in, its updated means out.                                                              */
OMDS_API int omds_weighted_update_eval(omds_ctx* ctx, const float* cost, const float* kernel_val_all, const float* kernel_activations,
                                       float rate, float ker_thr, float* mu_c, float* sigma_c, float* alpha_c, int32_t* mask_out,
                                       float* weights_out);
/* MPPI.get_qdot (MPPI.py:319-329): mode 0 = 'best', 1 = 'weighted'; out [n]. */
OMDS_API int omds_get_qdot(omds_ctx* ctx, int mode, float* out);

/* TensorPolicyMPPI.check_traj_for_kernels (policy.py:153-175) on the device-resident rollouts of
 * the last omds_propagate: candidate kernel centres = states (t, h) with closest_dist < thr_dist
 * and dot_product < thr_dot whose largest RBF value w.r.t. the K existing kernels (mu_c [K,n],
 * sigma_c [K], norm order = params.rbf_p) is < thr_kernel (K == 0: every close state).  Output
 * in the reference's boolean-mask order (rollout-major, then horizon): cand_q [cap,n], cand_th
 * [cap,2] = (t, h); *count = number found (may exceed cap, only min(count, cap) rows are written;
 * cap <= N*H).                                                                              */
OMDS_API int omds_kernel_candidates(omds_ctx* ctx, float thr_dist, float thr_kernel, float thr_dot, const float* mu_c,
                                    const float* sigma_c, int n_kernels, int cap, float* cand_q, int32_t* cand_th,
                                    int32_t* count);

/* Multi-GPU (new work; the reference is single-process): rollouts shard across one process per GPU,
 * every rank holds one context with N_local rollouts, and the only exchange is the cost-weighted update
 * (MPPI.shift_policy_means / get_qdot, MPPI.py:319-345 + policy.py:88-113).
 *
 * Native path (comm.hip): a RCCL communicator per context; the update runs on the context stream on device
 * buffers -- all-reduce SUM of [sum cost, N_local] (8 bytes) -> global beta; all-reduce SUM of the packed partial
 * sums (<= 3.4 KB); all-gather of (min cost, qdot of the arg-min) only when qdot_best is asked for.
 *   omds_comm_unique_id   : rank 0 creates the 128-byte id (ncclGetUniqueId); the launcher ships it to the other
 *                           ranks by whatever bootstrap it has (bench.py: a gloo broadcast).  No context needed;
 *                           omds_comm_last_error() holds the message of a failure.
 *   omds_comm_init_rank   : collective over all ranks (ncclCommInitRank on the context's device).  The shard of
 *                           rank 0 owns the global rollout 0 (policy.py:74): pass rollout_offset = rank * N_local
 *                           to omds_sample_policy.
 *   omds_weighted_update_sharded : collective.  mu_c/sigma_c/alpha_c in/out (identical on every rank afterwards),
 *                           mask_out [K]; qdot_weighted [n] = get_qdot('weighted') or NULL; qdot_best [n] =
 *                           get_qdot('best') over all shards or NULL (NULL skips the MINLOC gather);
 *                           n_total_out = number of rollouts over all shards or NULL.  Without a communicator it
 *                           is the single-shard update.  Failures of RCCL return OMDS_ERR_RCCL.
 *   omds_comm_probe       : OMDS_OK when RCCL can be loaded in this process (no device touched, no communicator made),
 *                           OMDS_ERR_RCCL otherwise (message: omds_comm_last_error).  A launcher calls it on EVERY rank and
 *                           lets the ranks agree before any of them enters omds_comm_init_rank: a rank that cannot load
 *                           RCCL would otherwise leave the others waiting inside ncclCommInitRank.                    */
#define OMDS_COMM_ID_BYTES 128
OMDS_API int omds_comm_probe(void);
OMDS_API int omds_comm_unique_id(uint8_t* out128);
OMDS_API const char* omds_comm_last_error(void);
OMDS_API int omds_comm_init_rank(omds_ctx* ctx, const uint8_t* id128, int rank, int world);
OMDS_API int omds_comm_destroy(omds_ctx* ctx);
OMDS_API int omds_comm_info(const omds_ctx* ctx, int32_t* rank, int32_t* world);
/* 1 while the context owns a communicator (a single-rank one included), else 0. */
OMDS_API int omds_comm_active(const omds_ctx* ctx);
OMDS_API int omds_weighted_update_sharded(omds_ctx* ctx, float rate, float ker_thr, float* mu_c, float* sigma_c,
                                          float* alpha_c, int32_t* mask_out, float* qdot_weighted, float* qdot_best,
                                          float* n_total_out);
/* Host-mediated form of the same exchange, for launchers without RCCL (tests/test_dist_gloo.py runs it over gloo,
 * world size 2, on CPU-side reductions): the library produces this shard's partial sums in two phases and the host
 * (optimalmodulationds_amd/dist.py) all-reduces them:
 *   omds_cost_sum    -> out2 = [sum_t cost, N_local]                 (all-reduce SUM, 8 bytes)
 *   omds_local_sums  -> packed buffer of omds_red_count() floats for the GLOBAL beta:
 *        [0] sum w' | sum w' mu (K*n) | sum w' sigma (K) | sum w' alpha (K*n) |
 *        sum_t max_h(phi*act) (K) | sum_h phi of GLOBAL rollout 0 (K; include_rollout0 != 0
 *        only on the shard that owns it) | sum w' qdot (n)            (all-reduce SUM)
 *        | min cost of the shard, qdot of its arg-min (1+n)          (all-gather, MINLOC)
 *   omds_apply_update: pure host arithmetic on the reduced buffer (masks MPPI.py:336-342 +
 *        TensorPolicyMPPI.update_policy policy.py:88-113); needs no context / no GPU.
 *        variant = omds_params.variant (OMDS_VARIANT_NO_BASE_MASK drops the rollout-0 mask). */
OMDS_API int omds_cost_sum(omds_ctx* ctx, float* out2);
OMDS_API int omds_red_count(const omds_ctx* ctx);
OMDS_API int omds_local_sums(omds_ctx* ctx, float sum_cost, float n_total, int include_rollout0, float* red_out);
OMDS_API int omds_apply_update(int n_kernels, int n_dof, int horizon, const float* red, float n_total, float rate,
                               float ker_thr, uint32_t variant, float* mu_c, float* sigma_c, float* alpha_c,
                               int32_t* mask_out);

/* Screening of pass 1 (screen_kernel.hip).  The N*O first-pass evaluations of MPPI.distance_repulsion_nn only feed the
 * sort that picks the k closest obstacles (MPPI.py:245-253); omds_propagate may therefore evaluate them in fp16 and
 * re-evaluate in fp32 only the candidates {o : Da(o) <= tau}, tau = k-th smallest Da + 1.25 eps (and every o whose Da is
 * not finite).  They contain the fp32 top-k (ties included) whenever the pairs that are NOT re-evaluated have a screening
 * error Da - D <= eps and the exact k-th smallest candidate stays eps below tau.  The distances and gradients a step uses
 * always come from the fp32 pass 2, and omds_dist_grad always uses the fp32 pass 1.
 * The identity with the all-fp32 step is therefore CONDITIONAL on eps, and eps is a measured quantity, not an a-priori one.
 * THE CONTRACT OF THE DEFAULT.  A context runs the ALL-FP32 step unless the caller opts in (mode 1 | 2 below, or OMDS_SCREEN=1|2 in the
 * environment): by default every network evaluation of omds_propagate is the reference's arithmetic on every pair, unconditionally.
 * Screening is an opt-in 5x: its results are the all-fp32 step's bit for bit in every test and soak run of this repository, but on
 * the strength of a MEASURED bound.  There is no usable a-priori one: propagating the f16 rounding of inputs, weights and activations
 * (2^-11 relative each) through sum |W| per layer gives |Da - D| <= 455 m for the shipped Franka network on |q| <= 2.9, |p| <= 1.5 m
 * (first order with sampled activation magnitudes: 58-81 m; planar 7-DoF: 5.8e3) against a measured eps of 0.016 m -- the norm
 * bound ignores the cancellation a trained network lives on, and is 3e4 times too large to select anything
 * (tools/studies/screen_apriori_bound.py).
 * What is measured, and when:
 *   - calibration: eps = 6 x the largest |Da - D| over ~3e5 pairs (states uniform in the joint box + states of the last
 *     propagate's rollouts, against the current obstacles), at the first screened propagate after omds_set_mlp, after
 *     omds_set_obstacles when the scene differs from the calibrated one (another count or radius, a sphere moved by more
 *     than 0.1), after a change of params.ignored_links, and on request (eps < 0 below).
 *     LATENCY: a calibration runs inside the omds_propagate that needs it -- one fp32 and one f16 pass over the batch plus two
 *     host re-sorts of the f16 weight pack by how often the hidden units fire (one in the calibration, one behind the first
 *     accepted propagate) -- about 21 ms on the first screened propagate against 5.8 ms for an ordinary 1024 x 32 iteration
 *     (tools/studies/reorder_cost.py), and the propagate after the second re-sort carries a sweep (+1 ms).  A translating
 *     scene does not recalibrate; a caller who SWAPS scenes at rate and cannot take the spike fixes the bound (eps > 0) or
 *     switches screening off for those iterations;
 *     UNDER AN OBSTACLE HORIZON (omds_set_screening_horizon on): the same states are measured against slabs 0, (H-1)/2 and H-1
 *     (duplicates once), each on its own fp32 / fp16 tables, and eps = 6 x the maximum over them; the re-sort stays on slab 0.  The
 *     calibration records slab 0, the LAST slab and that a horizon was in effect.  A screened propagate with a horizon first
 *     discards a calibration that was made without one, or whose recorded last slab differs from the present one by the test
 *     above (count, radius, 0.1 per coordinate; the last slab is omds_obstacle_horizon_predict's, or the caller's table's) -- and
 *     so recalibrates inside that propagate.  Hence: a scene that keeps translating at constant velocities recalibrates no more
 *     often than a static translating one; a bound set by the caller (eps > 0) is never recalibrated; a calibration made under
 *     a horizon also covers the static scene, so clearing the horizon does not recalibrate.  LATENCY: the measuring part (the
 *     fp32 and the f16 pass) then runs on three slabs instead of one; the cost of the first screened propagate under a horizon
 *     has not been measured yet (tools/studies/screen_horizon_cost.py measures it);
 *   - every step of every propagate: |Da - D| of every candidate; Da - D of the AUDIT rows, a pseudo-random 1-in-`one_in`
 *     sample (another one every step) of the pairs that are not candidates, re-evaluated in fp32 by one launch at the end
 *     of the horizon loop (k_audit; under a horizon every audit row against the slab of its own step, still one launch); the
 *     slack of every rollout (tau - exact k-th smallest >= eps).
 *   - every 32nd screened propagate (omds_set_screening_sweep): a SWEEP -- all N x O pairs of the propagate's last horizon
 *     step (soak runs: of EVERY horizon step) in fp32 beside all their screening values, max |Da - D| over every one of them,
 *     and the distribution of Da - D over the pairs that were not candidates (omds_screen_sweep_hist): the quantity the
 *     selection rule's assumption is about, counted exhaustively instead of sampled.  profiles/r04_screen_error_hist.txt
 *     holds that distribution over > 1e11 pairs (tools/sweep_soak.py).
 * A propagate is accepted only while all these maxima stay <= eps / 2 and no slack check failed; otherwise it is redone with the
 * fp32 pass 1 (its results are then the fp32 ones by construction) and eps is widened; three fallbacks in a row suspend
 * screening until the next calibration.  A row outside the audit sample whose error exceeds eps can still go unseen in
 * one propagate: at run time the identity is measured on a sample, not proven.  What the sample stands on: the exhaustive count of
 * tools/sweep_soak.py -- every horizon step of 5 183 propagates swept, 1.93e11 pairs over ten scene / network legs, none of the
 * 1.87e11 unevaluated pairs above eps / 2, the worst at 0.197 eps (profiles/r04_screen_error_hist.txt; the round-5 build: 2.4e11 more pairs, none above eps / 2, worst 0.182 eps,
 * profiles/r05_screen_error_hist.txt; the survival function of
 * (Da - D) / eps falls by half a decade or more per 1/128).
 * mode: -1 the library's default = off (env OMDS_SCREEN=0|1|2 changes the default of contexts left at -1), 0 off, 1 on, 2 on where it pays
 * (ReLU / tanh networks, with or without skip concatenations, n_traj * n_obs >= 65536 and n_obs >= 4 n_closest; else the fp32 step).  eps > 0 sets the bound in place of a calibration (never recalibrated; the run-time checks
 * still widen it when they must); eps == 0 changes the mode only; eps < 0 discards the calibration (measured again at the next screened propagate).
 * omds_set_screening_audit: one_in = 0 (no audit sample) or a power of two; default 128 (EXPERIMENTS.md C 4.1b has the measured cost per rate).
 * omds_screen_stats: active, eps in use, largest candidate error seen since the last calibration, mean candidates per
 * (rollout, step) since the last omds_prof_reset, fp32 fallbacks since creation (NULL = skip).
 * omds_screen_audit_stats: one_in, mean audit rows per (rollout, step) since the last omds_prof_reset, largest audit error
 * seen since the last calibration, suspended flag, calibrations run since creation.                                   */
OMDS_API int omds_set_screening(omds_ctx* ctx, int mode, float eps);
OMDS_API int omds_set_screening_audit(omds_ctx* ctx, int one_in);
/* Screening while an obstacle horizon is set.  on = 0 (default at creation): as before -- a horizon puts the context on the
 * all-fp32 step and omds_screen_stats reports active = 0.  on = 1: a propagate with a horizon (motion or explicit table, with or
 * without the moving frame) is screened under the same mode / eps / audit / sweep settings and the same contract as a static one.
 * *in_effect = 1 when the next propagate would run a screened route with a horizon set (NULL = skip).  Where horizon * max_obs
 * rounded up to 16 reaches 2^24 rows the audit sample is not taken (as for n_traj * horizon * n_obs >= 2^31).                     */
OMDS_API int omds_set_screening_horizon(omds_ctx* ctx, int on);
OMDS_API int omds_get_screening_horizon(omds_ctx* ctx, int32_t* on, int32_t* in_effect);
/* every = 0: no sweeps; default 32.  all_steps = 0: a sweeping propagate checks its last horizon step (0.5 % of the run at the
 * default period); 1: every horizon step (a soak / qualification mode: each step then also runs the fp32 pass 1, so the propagate
 * is slower than the unscreened one).  Stats: the setting, sweeps (swept steps) run since creation, largest |Da - D| a sweep saw
 * since the last calibration (NULL = skip).
 * omds_screen_sweep_hist: what all sweeps since creation (or the last reset != 0) have counted, OMDS_SWEEP_HIST_WORDS 64-bit words:
 *   [0] pairs swept  [1] of them NOT candidates (never re-evaluated by the step: the population the bound eps is about)
 *   [2] non-candidates with Da - D > eps / 2 (the acceptance margin)  [3] with Da - D > eps (a possible miss)
 *   [4] non-candidates with a non-finite difference  [5] largest Da - D over the non-candidates (float bits)
 *   [6] largest |Da - D| over all pairs (float bits)  [7] steps swept
 *   [8 .. 8 + L)     non-candidates with Da - D >= 0 by magnitude: bin b holds 2^(b - L) <= |x| < 2^(b + 1 - L) (bin 0 also zero
 *                    and everything smaller, bin L - 1 everything >= 1/2), L = OMDS_SWEEP_HIST_LOG_BINS
 *   [8 + L .. 8 + 2L)   the same for Da - D < 0 (the harmless side: the pair is even farther than its screening value said)
 *   [8 + 2L .. 8 + 2L + R)  non-candidates with Da - D > 0 by (Da - D) / eps in R = OMDS_SWEEP_HIST_RATIO_BINS linear bins over [0, 1)
 *                    (the last bin also holds everything >= 1), eps = the bound in use when the step was swept.            */
#define OMDS_SWEEP_HIST_LOG_BINS 32
#define OMDS_SWEEP_HIST_RATIO_BINS 128
#define OMDS_SWEEP_HIST_WORDS (8 + 2 * OMDS_SWEEP_HIST_LOG_BINS + OMDS_SWEEP_HIST_RATIO_BINS)
OMDS_API int omds_set_screening_sweep(omds_ctx* ctx, int every, int all_steps);
OMDS_API int omds_screen_sweep_stats(omds_ctx* ctx, int32_t* every, int64_t* sweeps, float* sweep_max_err);
OMDS_API int omds_screen_sweep_hist(omds_ctx* ctx, uint64_t* words, int n_words, int reset);
OMDS_API int omds_screen_audit_stats(omds_ctx* ctx, int32_t* one_in, double* audit_rows_per_rollout_step, float* audit_max_err,
                                     int32_t* suspended, int64_t* calibrations);
/* What tripped the fp32 fallbacks since creation (NULL = skip): a measured error above eps / 2 (candidates, audit sample or sweep);
 * a rollout whose exact k-th smallest candidate came within eps of tau (slack guard); a step whose candidate list outgrew the
 * per-entry buffers (32 candidates per rollout on average: near-flat distance fields); and how often three in a row (or a
 * non-finite error) suspended screening until the next calibration.                                                      */
OMDS_API int omds_screen_fallback_stats(omds_ctx* ctx, int64_t* by_error, int64_t* by_slack, int64_t* by_overflow, int64_t* suspensions);
/* Unit order of the screening network.  k_screen does not issue the MFMAs of a k-chunk (16 hidden units) whose activations are zero
 * for all 32 pairs of a wave -- exact: such a chunk adds nothing to any output.  Which units fire is a property of the trained
 * weights (of the shipped Franka network's 1024 hidden units, 300 fire for no pair of the shelf scene), so every calibration
 * sorts the hidden units of the fp16 pack by how often they fire on a uniform sample of 256 wave-sized blocks of (state, obstacle)
 * pairs (one k_exact launch, 6-7 ms; once on its own batch, once more on the states the first accepted propagate reaches),
 * which puts the silent ones into whole chunks.  ReLU networks without skip
 * concatenations; the fp32 kernels do not use this pack, so no returned number depends on the order.
 * reorders: packs rebuilt since creation; never_fired [n_levels <= 9] (NULL = skip): per hidden level, units that fired in no
 * sampled row at the last reorder.                                                                                          */
OMDS_API int omds_screen_order_stats(omds_ctx* ctx, int64_t* reorders, int32_t* never_fired, int n_levels);
/* The EXACT ZERO-SKIP of the fp32 pass 1 (k_pass1; ReLU networks without skip concatenations).  A hidden unit whose activation is
 * exactly zero in every row of a 64-row tile adds fmaf(0, w, acc) = acc to every chain of the next layer, so leaving it out changes
 * no bit -- as long as the units that ARE multiplied keep their ascending order.  k_pass1 therefore stores every hidden level of a
 * tile COMPACTED to the units that fire in that tile (rank order = unit order) and multiplies only those, fetching the weights by
 * unit; on the Franka shelf task 164 / 195 / 146 / 130 of the 256 units of the four levels fire in a tile.  Nothing is presumed
 * about which units fire: the result is the reference's chain bit for bit for every input (tests/test_gpu_sparse.py;
 * OMDS_FLAG_DENSE_PASS1 switches the compaction off).
 * active: 1 when the installed network qualifies; mean_units[L] / mean_chunks[L], L = 0 .. n_levels-1: firing units per tile of hidden
 * level L and k-chunks multiplied over it (of 8 positions; the last hidden level: of 16), averaged over the `tiles` tiles since
 * omds_set_mlp (NULL = skip).                                                                                                      */
OMDS_API int omds_pass1_skip_stats(omds_ctx* ctx, int32_t* active, double* mean_units, double* mean_chunks, int n_levels, int64_t* tiles);
/* The schedule of the last omds_propagate (OMDS_FLAG_SERIAL_PROPAGATE / OMDS_FLAG_PIPELINED_PROPAGATE above): parts = 2 when its full
 * steps ran as the rollouts [0, split) on the context's stream and [split, n_traj) on its second stream, else parts = 1 and
 * split = n_traj.  Either pointer may be NULL.  Before the first propagate: 1 part.                                                */
OMDS_API int omds_get_pipeline_info(omds_ctx* ctx, int32_t* parts, int32_t* split);
/* (The two test hooks that damage the screening inputs / force a tile shape are NOT part of this library: they are declared in
 * include/omds_test.h and exported by libomds_hip_test.so only.)                                                           */
/* Diagnostic: the fp16 screening network alone on q [B,n] -> mindist [B,O] (the values the candidate selection sees). */
OMDS_API int omds_screen_mindist(omds_ctx* ctx, const float* q, int batch, float* mindist);
OMDS_API int omds_screen_stats(omds_ctx* ctx, int32_t* active, float* eps, float* max_err_seen,
                               double* cand_per_rollout_step, int64_t* fallbacks);

/* SDF training (mlp_learn/train_sdf.py:96-151): full-batch regression of the distance network on a data set
 * (x [B, d] raw inputs = joint angles then the obstacle point, y [B, C] link distances) -- per epoch one forward through
 * [x, sin x, cos x] -> Linear + act ... -> Linear (network_macros_mod.py:137-146), F.mse_loss(reduction = 'mean'), the backward
 * through every layer and one torch.optim.Adam step (single-tensor arithmetic: lerp of exp_avg, bias-corrected step size,
 * denom = sqrt(exp_avg_sq) / sqrt(bc2) + eps), all on the device in exact-fp32 MFMA GEMMs (csrc/train.hip).  The scheduler
 * (ReduceLROnPlateau), validation metrics and the checkpoint dictionary of the reference stay on the host
 * (tools/train_sdf_hip.py).  A trainer is its own object (no omds_ctx needed); dims[n_linear + 1] = {3 d, hidden ..., C}; W[i] is
 * [dims[i+1], dims[i]] row-major like torch.  omds_trainer_set_weights also resets the optimizer state and step count.
 * omds_trainer_step returns the loss BEFORE the update (what train_sdf.py prints as train loss); omds_trainer_eval runs the
 * forward + loss with the current weights, no update, on the training set (which = 0) or on the validation set of
 * omds_trainer_set_val_data (which = 1: train_sdf.py:84-86, 117-121; no weight copy, the optimizer state untouched); pred_out
 * [B, C] or NULL.  omds_trainer_get / set_optimizer_state: torch.optim.Adam's exp_avg (m) and exp_avg_sq (v) of every weight and
 * bias and the step count -- what train_sdf.py:130-138 saves as optimizer.state_dict() and a resumed run restores (arrays shaped
 * like the weights; get: a NULL array or entry is skipped).  From a zero optimizer state (a new trainer, or after
 * omds_trainer_set_weights) omds_trainer_step with lr = 0, beta1 = beta2 = 0 and eps > 0 leaves the weights as they are and
 * exp_avg equal to the gradient bit for bit (exp_avg_sq its square): how tests/test_gpu_train_grad.py reads gradients.          */
typedef struct omds_trainer omds_trainer;
OMDS_API int omds_trainer_create(int device, int n_linear, const int32_t* dims, int act, omds_trainer** out);
OMDS_API void omds_trainer_destroy(omds_trainer* tr);
OMDS_API const char* omds_trainer_last_error(const omds_trainer* tr);
OMDS_API int omds_trainer_set_weights(omds_trainer* tr, const float* const* W, const float* const* b);
OMDS_API int omds_trainer_get_weights(omds_trainer* tr, float* const* W, float* const* b);
OMDS_API int omds_trainer_set_data(omds_trainer* tr, const float* x, const float* y, int batch);
OMDS_API int omds_trainer_step(omds_trainer* tr, float lr, float beta1, float beta2, float eps, float* loss_out);
OMDS_API int omds_trainer_set_val_data(omds_trainer* tr, const float* x, const float* y, int batch);
OMDS_API int omds_trainer_eval(omds_trainer* tr, int which, float* mse_out, float* pred_out);
OMDS_API int omds_trainer_get_optimizer_state(omds_trainer* tr, float* const* mW, float* const* mb, float* const* vW, float* const* vb,
                                              int64_t* step);
OMDS_API int omds_trainer_set_optimizer_state(omds_trainer* tr, const float* const* mW, const float* const* mb, const float* const* vW,
                                              const float* const* vb, int64_t step);

/* SDF training data (mlp_learn/gen_dataset.py:12-50 for a DH chain, mlp_learn/gen_dataset_2dtoy.py for the point robot), made
 * on the device (csrc/dataset_kernels.hip).  Configuration i is a block of n_uniform + n_near rows: first points uniform in the
 * box [p_min, p_max], then points near the robot.  DH chain (kind OMDS_SDF_DATA_DH): q uniform in [q_min, q_max]; link l is
 * sampled at lspan * [a_{l+1}, 0, 0] in frame l + 1 (fk_num.py numeric_fk_model); near point j is link point j mod (n * n_pts),
 * link-major, plus an offset uniform in near_scale * [p_min, p_max]; a row is [q (n), p (3), d_1 .. d_n] with d_l the distance
 * from p to the nearest sample point of link l.  Point robot (kind OMDS_SDF_DATA_POINT, n_dof = 2 or 3 point dimensions): near
 * point j is q + offset; a row is [q (n), p (n), |p - q|].  The draws come from Philox4x32-10 keyed by the seed with counter
 * (configuration index, stream, draw), so the rows of configuration i are a pure function of (spec, seed, i): cfg0 = k, n_cfg = m
 * returns rows k (n_uniform + n_near) .. (k + m) (n_uniform + n_near) - 1 of one call with cfg0 = 0, whatever the chunking.
 * lspan [n_pts] (DH only) holds the link sample fractions: the reference's torch.linspace(0.01, 1, n_pts) fp32 values, which
 * the caller supplies (optimalmodulationds_amd.dataset takes them from torch) and the device never recomputes.
 * omds_sdf_data_generate / _from_draws write n_cfg (n_uniform + n_near) rows of cols floats to HOST memory `out`; _from_draws takes
 * the draws (q [n_cfg, n], p_uniform [n_cfg, n_uniform, pd], near_offsets [n_cfg, n_near, pd], pd = 3 or n) instead of Philox:
 * the reference's own np.random values in, its rows out.  omds_trainer_generate_data writes the rows straight into a trainer's
 * training set (which = 0) or validation set (which = 1) on the trainer's stream, no host copy; the trainer's raw inputs must be
 * n + pd and its outputs the label count.  Context-free entry points report through omds_last_error(NULL).  An invalid spec
 * (sizes < 1 or over the limits below, dh_rows < n + 1, a box with min > max, rows x cols beyond int64) is
 * OMDS_ERR_INVALID_ARG before any device is touched.                                                                          */
#define OMDS_SDF_DATA_DH 0
#define OMDS_SDF_DATA_POINT 1
#define OMDS_SDF_DATA_MAX_PTS_PER_LINK 256
#define OMDS_SDF_DATA_MAX_LINK_PTS 2048      /* n_dof * n_pts: the link points one workgroup holds in LDS */
typedef struct {
    int32_t kind;              /* OMDS_SDF_DATA_DH | OMDS_SDF_DATA_POINT                                     */
    int32_t n_dof;             /* joints n (1 .. OMDS_MAX_DOF); point robot: its point dimensions (2 or 3)   */
    int32_t n_pts;             /* sample points per link (DH only)                                            */
    int32_t n_cfg;             /* configurations of the whole data set (omds_sdf_data_shape)                  */
    int32_t n_uniform;         /* rows per configuration with uniform points                                  */
    int32_t n_near;            /* rows per configuration with points near the robot                           */
    float near_scale;          /* the near-point offset box is near_scale * [p_min, p_max] (the reference: 0.1) */
    int32_t dh_rows;           /* rows dh_params holds (DH: at least n_dof + 1)                               */
    const float* dh_params;    /* [dh_rows, 4] (d, theta, a, alpha) rows (DH only)                            */
    const float* q_min;        /* [n_dof]                                                                     */
    const float* q_max;
    const float* p_min;        /* [3] for a DH chain, [n_dof] for the point robot                            */
    const float* p_max;
    const float* lspan;        /* [n_pts] (DH only)                                                           */
} omds_sdf_data_spec;
OMDS_API int omds_sdf_data_shape(const omds_sdf_data_spec* spec, int64_t* rows, int32_t* cols);
OMDS_API int omds_sdf_data_generate(int device, const omds_sdf_data_spec* spec, uint64_t seed, int64_t cfg0, int64_t n_cfg, float* out);
OMDS_API int omds_sdf_data_from_draws(int device, const omds_sdf_data_spec* spec, const float* q, const float* p_uniform,
                                      const float* near_offsets, int64_t n_cfg, float* out);
OMDS_API int omds_trainer_generate_data(omds_trainer* tr, const omds_sdf_data_spec* spec, uint64_t seed, int64_t cfg0, int64_t n_cfg,
                                        int which);

/* Measurement: when enabled, launches of the dominant kernel (k_pass1) are bracketed by HIP events on the
 * context stream -- every launch for on == 1, every on-th launch for on > 1 (an event record between two
 * kernels idles the GPU for ~6 us, so throughput runs sample) -- and omds_prof_read returns the summed elapsed
 * ms and the number of bracketed launches since the last omds_prof_reset.                                  */
OMDS_API int omds_prof_enable(omds_ctx* ctx, int on);
OMDS_API int omds_prof_reset(omds_ctx* ctx);
OMDS_API int omds_prof_read(omds_ctx* ctx, double* pass1_ms, int64_t* pass1_launches, int64_t* pass1_rows);
/* Same, with the algorithmic FLOPs of the bracketed launches and the kernel's name. */
OMDS_API int omds_prof_read_ex(omds_ctx* ctx, double* ms, int64_t* launches, double* flops, const char** kernel);
/* Asynchronous form used by bench loops: propagate + cost + weighted update enqueued without
 * host round trips of rollout data; omds_sync waits for the stream.                       */
OMDS_API int omds_sync(omds_ctx* ctx);
/* Number of HIP devices this process can see (0 on a box without a GPU: not an error).  Launchers size their rank count by it
 * (bench.py --gpus N refuses when N exceeds it); no context needed.                                                        */
OMDS_API int omds_device_count(int32_t* count);
OMDS_API int omds_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OMDS_H */
