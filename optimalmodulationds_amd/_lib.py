"""ctypes binding of libomds_hip.so (C-ABI declared in include/omds.h).

This is exactly the binding a maintainer of the reference would add to call the MI355X path
(see INTEGRATION.md).  There is no fallback: if the shared library is missing or a call fails,
an exception is raised."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# OMDS_LIB: another build of the same library (the test library, diagnostic builds, an A/B build under csrc/), never a different backend
LIB_PATH = os.environ.get("OMDS_LIB") or os.path.join(_HERE, "csrc", "libomds_hip.so")

OMDS_MAX_DOF = 7
SWEEP_HIST_LOG_BINS, SWEEP_HIST_RATIO_BINS = 32, 128
SWEEP_HIST_WORDS = 8 + 2 * SWEEP_HIST_LOG_BINS + SWEEP_HIST_RATIO_BINS    # omds.h: OMDS_SWEEP_HIST_WORDS
# float* / int32_t* arguments are declared as plain addresses: numpy's ``a.ctypes.data_as(POINTER(c_float))`` goes through
# ``ctypes.cast`` (~28 us per call: 0.8 ms of a planner iteration through the facade), ``a.ctypes.data`` is an attribute read
F32P = C.c_void_p
I32P = C.c_void_p


class OmdsConfig(C.Structure):
    _fields_ = [("n_dof", C.c_int32), ("n_traj", C.c_int32), ("horizon", C.c_int32), ("n_kernel_max", C.c_int32),
                ("max_obs", C.c_int32), ("n_closest", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32)]


class OmdsParams(C.Structure):
    _fields_ = [("dt", C.c_float), ("dst_thr", C.c_float), ("lin_thr", C.c_float), ("lvel", C.c_float * 5),
                ("ln", C.c_float * 5), ("ltau", C.c_float * 5), ("goal_act_cut", C.c_float),
                ("norm_clamp", C.c_float), ("coll_slow", C.c_float), ("coll_repulse", C.c_float),
                ("softmax_k", C.c_float), ("rbf_p", C.c_float), ("ignored_links", C.c_uint32),
                ("variant", C.c_uint32), ("cost_terms", C.c_uint32)]


FLAG_UNFUSED_STEP = 1
FLAG_TAIL_FORWARD = 4      # the fp32 step's tail keeps its own forward (omds.h: OMDS_FLAG_TAIL_FORWARD)
FLAG_DENSE_PASS1 = 8       # k_pass1 multiplies every k-chunk (omds.h: OMDS_FLAG_DENSE_PASS1; same bits as the per-tile compaction)
FLAG_NATURAL_PASS1 = 16    # first step of a propagate from one state evaluated per rollout (omds.h: OMDS_FLAG_NATURAL_PASS1; same bits)
FLAG_NATURAL_TILES = 32    # pass-1 tiles over consecutive rows instead of key-ordered rollout x obstacle blocks (omds.h: OMDS_FLAG_NATURAL_TILES; same bits)
FLAG_BLOCK_TILES = 64      # the block order at every batch size, not only from 131 072 pairs on (omds.h: OMDS_FLAG_BLOCK_TILES; same bits)
FLAG_SERIAL_PROPAGATE = 128      # every launch of a propagate on one stream (omds.h: OMDS_FLAG_SERIAL_PROPAGATE; same bits)
FLAG_PIPELINED_PROPAGATE = 256   # the dense step's full steps as two halves of the batch on two streams, at any batch size (omds.h; same bits)
FLAG_TWO_KERNEL_STEP = 2  # keep few-obstacle scenes on k_pass1 + k_tail (omds.h: OMDS_FLAG_TWO_KERNEL_STEP)   # omds_config.flags
# omds_params.variant / cost_terms bits (include/omds.h)
VARIANT_KVAL_TIMES_ACT = 1
VARIANT_NO_BASE_MASK = 2
COST_GOAL, COST_COLLISION, COST_JOINT_LIMITS, COST_STAGNATION, COST_FK, COST_ALL = 1, 2, 4, 8, 16, 31


SDF_DATA_DH, SDF_DATA_POINT = 0, 1     # omds_sdf_data_spec.kind


class OmdsSdfDataSpec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_dof", C.c_int32), ("n_pts", C.c_int32), ("n_cfg", C.c_int32), ("n_uniform", C.c_int32),
                ("n_near", C.c_int32), ("near_scale", C.c_float), ("dh_rows", C.c_int32), ("dh_params", F32P), ("q_min", F32P),
                ("q_max", F32P), ("p_min", F32P), ("p_max", F32P), ("lspan", F32P)]


class OmdsCloudSpec(C.Structure):
    """omds_cloud_spec (include/omds.h): the voxel grid a point cloud is turned into obstacle spheres on."""
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("dims", C.c_int32 * 3), ("radius", C.c_float),
                ("min_points", C.c_int32), ("max_spheres", C.c_int32), ("self_margin", C.c_float), ("pad", C.c_float * 4)]


class OmdsCloudTrackSpec(C.Structure):
    """omds_cloud_track_spec (include/omds.h): how the tracked cloud call matches a frame against the previous one."""
    _fields_ = [("reach", C.c_int32), ("dt_frame", C.c_float), ("still", C.c_float)]


class OmdsCloudObjectSpec(C.Structure):
    """omds_cloud_object_spec (include/omds.h): how the objects cloud call segments the sphere list into components."""
    _fields_ = [("link", C.c_int32), ("min_cells", C.c_int32)]


DEPTH_U16, DEPTH_F32, DEPTH_MAX_CAMERAS = 0, 1, 8     # omds_depth_camera.format; cameras per omds_set_obstacles_from_depth


class OmdsDepthCamera(C.Structure):
    """omds_depth_camera (include/omds.h): one depth image's shape, intrinsics, range gate and pose."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32), ("format", C.c_int32), ("step", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("depth_scale", C.c_float),
                ("z_min", C.c_float), ("z_max", C.c_float), ("pose", C.c_float * 12)]


class OmdsSceneMemorySpec(C.Structure):
    """omds_scene_memory_spec (include/omds.h): how the depth route's scene memory ages and clears an unseen cell."""
    _fields_ = [("max_age", C.c_int32), ("clear_margin", C.c_float), ("footprint", C.c_int32)]


class OmdsDepthFilterSpec(C.Structure):
    """omds_depth_filter_spec (include/omds.h): which depth pixels the depth routes drop as flying pixels or speckle."""
    _fields_ = [("radius", C.c_int32), ("min_support", C.c_int32), ("edge_abs", C.c_float), ("edge_rel", C.c_float)]


class OmdsDepthLens(C.Structure):
    """omds_depth_lens (include/omds.h): the lens of a depth camera, OpenCV's rational Brown-Conrady model."""
    _fields_ = [("model", C.c_int32), ("k", C.c_float * 8), ("iters", C.c_int32), ("max_residual", C.c_float)]


class OmdsVelocityFilterSpec(C.Structure):
    """omds_velocity_filter_spec (include/omds.h): how the velocity routes blend a new sphere velocity against its predecessor."""
    _fields_ = [("alpha", C.c_float), ("alpha_object", C.c_float), ("max_jump", C.c_float)]


class OmdsObstacleFocusSpec(C.Structure):
    """omds_obstacle_focus_spec (include/omds.h): which spheres of a large scene an obstacle focus keeps."""
    _fields_ = [("margin", C.c_float), ("lookahead", C.c_float), ("max_keep", C.c_int32)]


class OmdsTestModulateArgs(C.Structure):
    """omds_test_modulate_args (include/omds_test.h): one horizon step of the modulation on caller-supplied inputs."""
    _fields_ = ([(f, C.c_int32) for f in ("n_dof", "nsub", "N", "K", "Kmax", "k", "d", "step", "H", "frame", "O", "ldVel", "seds_G")]
                + [(f, C.c_float) for f in ("frame_max", "seds_lin_thr", "seds_thr")] + [("prm", OmdsParams)]
                + [(f, C.c_void_p) for f in ("qf", "A", "seds_mu_in", "seds_b", "seds_sigma_inv", "seds_A", "seds_prior", "seds_den", "vel",
                                             "rowObs", "q", "drow", "gradx", "mu", "sigma", "alpha", "maxact", "phisum0", "q_next", "qdot",
                                             "dist", "dot", "act", "normal", "kval")])


class OmdsError(RuntimeError):
    pass


# name -> (restype, argtypes); every symbol include/omds.h declares
SIGNATURES = {
    "omds_version": (C.c_int, []),
    "omds_default_params": (None, [C.POINTER(OmdsParams)]),
    "omds_create": (C.c_int, [C.POINTER(OmdsConfig), C.POINTER(C.c_void_p)]),
    "omds_destroy": (None, [C.c_void_p]),
    "omds_last_error": (C.c_char_p, [C.c_void_p]),
    "omds_set_mlp": (C.c_int, [C.c_void_p, C.c_int, I32P, C.POINTER(F32P), C.POINTER(F32P), C.c_int, C.c_float]),
    "omds_set_mlp_ex": (C.c_int, [C.c_void_p, C.c_int, I32P, I32P, C.POINTER(F32P), C.POINTER(F32P), C.c_int, C.c_float,
                                  C.c_int, I32P]),
    "omds_set_obstacles": (C.c_int, [C.c_void_p, F32P, C.c_int]),
    "omds_obstacle_horizon_predict": (C.c_int, [F32P, F32P, C.c_int, C.c_int, C.c_float, F32P]),
    "omds_set_obstacle_motion": (C.c_int, [C.c_void_p, F32P]),
    "omds_set_obstacle_horizon": (C.c_int, [C.c_void_p, F32P, C.c_int]),
    "omds_get_obstacle_horizon": (C.c_int, [C.c_void_p, F32P, I32P]),
    "omds_moving_frame_velocity": (C.c_int, [C.c_int, C.c_int, C.c_int, F32P, F32P, F32P, C.c_float, C.c_float, F32P, F32P]),
    "omds_set_obstacle_frame": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "omds_get_obstacle_frame": (C.c_int, [C.c_void_p, I32P, F32P, I32P]),
    "omds_approach_rate": (C.c_int, [C.c_void_p, F32P, C.c_int, F32P, F32P]),
    "omds_point_cloud_spheres": (C.c_int, [C.POINTER(OmdsCloudSpec), F32P, C.c_int64, F32P, C.c_int32, I32P]),
    "omds_set_obstacles_from_cloud": (C.c_int, [C.c_void_p, C.POINTER(OmdsCloudSpec), C.c_void_p, C.c_int64, C.c_int, F32P, I32P, I32P]),
    "omds_get_obstacles": (C.c_int, [C.c_void_p, F32P, I32P]),
    "omds_point_cloud_flow": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsCloudTrackSpec), F32P, C.c_int64, F32P, C.c_int64, F32P, F32P,
                                        C.c_int32, I32P, I32P]),
    "omds_set_obstacles_from_cloud_tracked": (C.c_int, [C.c_void_p, C.POINTER(OmdsCloudSpec), C.POINTER(OmdsCloudTrackSpec), C.c_void_p,
                                                        C.c_int64, C.c_int, F32P, I32P, I32P, I32P]),
    "omds_cloud_track_reset": (C.c_int, [C.c_void_p]),
    "omds_get_obstacle_motion": (C.c_int, [C.c_void_p, F32P, I32P]),
    "omds_point_cloud_object_flow": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsCloudTrackSpec), C.POINTER(OmdsCloudObjectSpec), F32P,
                                               C.c_int64, C.c_void_p, F32P, C.c_int64, C.c_void_p, F32P, F32P, I32P, I32P, C.c_int32, I32P,
                                               I32P, I32P, I32P]),
    "omds_set_obstacles_from_cloud_objects": (C.c_int, [C.c_void_p, C.POINTER(OmdsCloudSpec), C.POINTER(OmdsCloudTrackSpec),
                                                        C.POINTER(OmdsCloudObjectSpec), C.c_void_p, C.c_int64, C.c_int, F32P, I32P, I32P,
                                                        I32P, I32P, I32P]),
    "omds_get_cloud_objects": (C.c_int, [C.c_void_p, I32P, I32P, I32P]),
    "omds_depth_points": (C.c_int, [C.POINTER(OmdsDepthCamera), C.c_void_p, F32P, C.c_int64, C.POINTER(C.c_int64)]),
    "omds_set_obstacles_from_depth": (C.c_int, [C.c_void_p, C.POINTER(OmdsCloudSpec), C.POINTER(OmdsCloudTrackSpec),
                                                C.POINTER(OmdsCloudObjectSpec), C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p), C.c_int32,
                                                C.c_int, F32P, I32P, I32P, I32P, I32P, I32P]),
    "omds_depth_scene_memory": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsSceneMemorySpec), C.POINTER(OmdsDepthCamera),
                                          C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_void_p, I32P]),
    "omds_set_obstacles_from_depth_memory": (C.c_int, [C.c_void_p, C.POINTER(OmdsCloudSpec), C.POINTER(OmdsSceneMemorySpec),
                                                       C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p), C.c_int32, C.c_int, F32P, I32P, I32P]),
    "omds_scene_memory_reset": (C.c_int, [C.c_void_p]),
    "omds_get_scene_memory": (C.c_int, [C.c_void_p, I32P, C.c_void_p, I32P]),
    "omds_depth_points_filtered": (C.c_int, [C.POINTER(OmdsDepthCamera), C.POINTER(OmdsDepthFilterSpec), C.c_void_p, F32P, C.c_int64,
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "omds_depth_scene_memory_filtered": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsSceneMemorySpec), C.POINTER(OmdsDepthFilterSpec),
                                                   C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_void_p, I32P]),
    "omds_set_depth_filter": (C.c_int, [C.c_void_p, C.POINTER(OmdsDepthFilterSpec)]),
    "omds_get_depth_filter_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "omds_depth_scene_memory_flow": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsSceneMemorySpec), C.POINTER(OmdsCloudTrackSpec),
                                               C.POINTER(OmdsCloudObjectSpec), C.POINTER(OmdsDepthFilterSpec), C.POINTER(OmdsDepthCamera),
                                               C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p),
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, I32P, F32P, F32P, I32P, I32P, I32P, C.c_int32,
                                               I32P, I32P, I32P, I32P]),
    "omds_set_obstacles_from_depth_memory_tracked": (C.c_int, [C.c_void_p, C.POINTER(OmdsCloudSpec), C.POINTER(OmdsSceneMemorySpec),
                                                               C.POINTER(OmdsCloudTrackSpec), C.POINTER(OmdsCloudObjectSpec),
                                                               C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p), C.c_int32, C.c_int, F32P, I32P,
                                                               I32P, I32P, I32P, I32P]),
    "omds_depth_lens_rays": (C.c_int, [C.POINTER(OmdsDepthCamera), C.POINTER(OmdsDepthLens), F32P, F32P, C.POINTER(C.c_int64)]),
    "omds_depth_points_lens": (C.c_int, [C.POINTER(OmdsDepthCamera), C.POINTER(OmdsDepthLens), C.POINTER(OmdsDepthFilterSpec), C.c_void_p, F32P,
                                         C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "omds_depth_scene_memory_lens": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsSceneMemorySpec), C.POINTER(OmdsDepthFilterSpec),
                                               C.POINTER(OmdsDepthLens), C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p), C.c_int32, C.c_void_p,
                                               C.c_void_p, I32P]),
    "omds_depth_scene_memory_flow_lens": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsSceneMemorySpec), C.POINTER(OmdsCloudTrackSpec),
                                                    C.POINTER(OmdsCloudObjectSpec), C.POINTER(OmdsDepthFilterSpec), C.POINTER(OmdsDepthLens),
                                                    C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p), C.c_int32, C.c_void_p,
                                                    C.POINTER(OmdsDepthLens), C.POINTER(OmdsDepthCamera), C.POINTER(C.c_void_p), C.c_int32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, I32P, F32P, F32P, I32P, I32P, I32P, C.c_int32, I32P, I32P,
                                                    I32P, I32P]),
    "omds_set_depth_lenses": (C.c_int, [C.c_void_p, C.POINTER(OmdsDepthLens), C.c_int32]),
    "omds_get_depth_lens_table": (C.c_int, [C.c_void_p, C.c_int32, F32P, F32P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "omds_velocity_filter_step": (C.c_int, [C.POINTER(OmdsCloudSpec), C.POINTER(OmdsCloudTrackSpec), C.POINTER(OmdsVelocityFilterSpec), I32P, I32P,
                                            F32P, I32P, I32P, C.c_int32, F32P, I32P, I32P]),
    "omds_set_velocity_filter": (C.c_int, [C.c_void_p, C.POINTER(OmdsVelocityFilterSpec)]),
    "omds_get_velocity_filter": (C.c_int, [C.c_void_p, C.POINTER(OmdsVelocityFilterSpec), I32P]),
    "omds_get_velocity_filter_frame": (C.c_int, [C.c_void_p, F32P, I32P, I32P]),
    "omds_get_velocity_filter_state": (C.c_int, [C.c_void_p, I32P, I32P]),
    "omds_obstacle_focus_select": (C.c_int, [C.POINTER(OmdsObstacleFocusSpec), F32P, F32P, C.c_int, C.c_int, I32P, C.c_int32, I32P, I32P]),
    "omds_focus_obstacles": (C.c_int, [C.c_void_p, C.POINTER(OmdsObstacleFocusSpec), F32P, I32P, I32P]),
    "omds_obstacle_focus_select_path": (C.c_int, [C.POINTER(OmdsObstacleFocusSpec), F32P, F32P, F32P, C.c_int, C.c_int, C.c_int, I32P, C.c_int32, I32P,
                                                  I32P]),
    "omds_focus_obstacles_path": (C.c_int, [C.c_void_p, C.POINTER(OmdsObstacleFocusSpec), F32P, F32P, C.c_int, I32P, I32P]),
    "omds_get_obstacle_focus": (C.c_int, [C.c_void_p, I32P, I32P, I32P]),
    "omds_clear_obstacle_focus": (C.c_int, [C.c_void_p]),
    "omds_set_ds": (C.c_int, [C.c_void_p, F32P]),
    "omds_set_ds_matrix": (C.c_int, [C.c_void_p, F32P, F32P]),
    "omds_set_ds_seds": (C.c_int, [C.c_void_p, F32P, C.c_int, F32P, F32P, F32P, F32P, F32P, F32P, C.c_float, C.c_float]),
    "omds_set_params": (C.c_int, [C.c_void_p, C.POINTER(OmdsParams)]),
    "omds_set_cost": (C.c_int, [C.c_void_p, F32P, F32P, F32P]),
    "omds_set_policy_samples": (C.c_int, [C.c_void_p, F32P, F32P, F32P, C.c_int]),
    "omds_sample_policy": (C.c_int, [C.c_void_p, F32P, F32P, F32P, C.c_float, C.c_float, C.c_float, C.c_int,
                                     C.c_uint64, C.c_int64]),
    "omds_get_policy_samples": (C.c_int, [C.c_void_p, F32P, F32P, F32P]),
    "omds_propagate": (C.c_int, [C.c_void_p, F32P, C.c_int]),
    "omds_get_rollouts": (C.c_int, [C.c_void_p, F32P, F32P, F32P, F32P, F32P, F32P, F32P]),
    "omds_get_rollout_rows": (C.c_int, [C.c_void_p, I32P, C.c_int, F32P, F32P, F32P, F32P, F32P, F32P, F32P]),
    "omds_dist_grad": (C.c_int, [C.c_void_p, F32P, C.c_int, F32P, F32P, F32P, I32P]),
    "omds_mlp_forward_vjp": (C.c_int, [C.c_void_p, F32P, C.c_int, F32P, F32P, I32P]),
    "omds_mlp_jacobian": (C.c_int, [C.c_void_p, F32P, C.c_int, I32P, C.c_int, F32P, F32P]),
    "omds_cost": (C.c_int, [C.c_void_p, F32P]),
    "omds_cost_eval": (C.c_int, [C.c_void_p, F32P, F32P, C.c_int, F32P]),
    "omds_weighted_update": (C.c_int, [C.c_void_p, C.c_float, C.c_float, F32P, F32P, F32P, I32P, F32P]),
    "omds_weighted_update_eval": (C.c_int, [C.c_void_p, F32P, F32P, F32P, C.c_float, C.c_float, F32P, F32P, F32P, I32P, F32P]),
    "omds_get_qdot": (C.c_int, [C.c_void_p, C.c_int, F32P]),
    "omds_kernel_candidates": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, F32P, F32P, C.c_int, C.c_int,
                                         F32P, I32P, I32P]),
    "omds_cost_sum": (C.c_int, [C.c_void_p, F32P]),
    "omds_red_count": (C.c_int, [C.c_void_p]),
    "omds_local_sums": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_int, F32P]),
    "omds_apply_update": (C.c_int, [C.c_int, C.c_int, C.c_int, F32P, C.c_float, C.c_float, C.c_float, C.c_uint32,
                                    F32P, F32P, F32P, I32P]),
    "omds_comm_probe": (C.c_int, []),
    "omds_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "omds_comm_last_error": (C.c_char_p, []),
    "omds_comm_init_rank": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int, C.c_int]),
    "omds_comm_destroy": (C.c_int, [C.c_void_p]),
    "omds_comm_info": (C.c_int, [C.c_void_p, I32P, I32P]),
    "omds_comm_active": (C.c_int, [C.c_void_p]),
    "omds_weighted_update_sharded": (C.c_int, [C.c_void_p, C.c_float, C.c_float, F32P, F32P, F32P, I32P, F32P, F32P,
                                               F32P]),
    "omds_set_screening": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "omds_set_screening_audit": (C.c_int, [C.c_void_p, C.c_int]),
    "omds_set_screening_horizon": (C.c_int, [C.c_void_p, C.c_int]),
    "omds_get_screening_horizon": (C.c_int, [C.c_void_p, I32P, I32P]),
    "omds_screen_audit_stats": (C.c_int, [C.c_void_p, I32P, C.POINTER(C.c_double), F32P, I32P, C.POINTER(C.c_int64)]),
    "omds_screen_fallback_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "omds_screen_order_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), I32P, C.c_int]),
    "omds_pass1_skip_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int64)]),
    "omds_get_pipeline_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "omds_set_screening_sweep": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "omds_screen_sweep_hist": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_int]),
    "omds_screen_sweep_stats": (C.c_int, [C.c_void_p, I32P, C.POINTER(C.c_int64), F32P]),
    "omds_screen_mindist": (C.c_int, [C.c_void_p, F32P, C.c_int, F32P]),
    "omds_screen_stats": (C.c_int, [C.c_void_p, I32P, F32P, F32P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "omds_trainer_create": (C.c_int, [C.c_int, C.c_int, I32P, C.c_int, C.POINTER(C.c_void_p)]),
    "omds_trainer_destroy": (None, [C.c_void_p]),
    "omds_trainer_last_error": (C.c_char_p, [C.c_void_p]),
    "omds_trainer_set_weights": (C.c_int, [C.c_void_p, C.POINTER(F32P), C.POINTER(F32P)]),
    "omds_trainer_get_weights": (C.c_int, [C.c_void_p, C.POINTER(F32P), C.POINTER(F32P)]),
    "omds_trainer_set_data": (C.c_int, [C.c_void_p, F32P, F32P, C.c_int]),
    "omds_trainer_step": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, F32P]),
    "omds_trainer_set_val_data": (C.c_int, [C.c_void_p, F32P, F32P, C.c_int]),
    "omds_trainer_eval": (C.c_int, [C.c_void_p, C.c_int, F32P, F32P]),
    "omds_trainer_get_optimizer_state": (C.c_int, [C.c_void_p, C.POINTER(F32P), C.POINTER(F32P), C.POINTER(F32P), C.POINTER(F32P),
                                                   C.POINTER(C.c_int64)]),
    "omds_trainer_set_optimizer_state": (C.c_int, [C.c_void_p, C.POINTER(F32P), C.POINTER(F32P), C.POINTER(F32P), C.POINTER(F32P), C.c_int64]),
    "omds_sdf_data_shape": (C.c_int, [C.POINTER(OmdsSdfDataSpec), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "omds_sdf_data_generate": (C.c_int, [C.c_int, C.POINTER(OmdsSdfDataSpec), C.c_uint64, C.c_int64, C.c_int64, F32P]),
    "omds_sdf_data_from_draws": (C.c_int, [C.c_int, C.POINTER(OmdsSdfDataSpec), F32P, F32P, F32P, C.c_int64, F32P]),
    "omds_trainer_generate_data": (C.c_int, [C.c_void_p, C.POINTER(OmdsSdfDataSpec), C.c_uint64, C.c_int64, C.c_int64, C.c_int]),
    "omds_prof_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "omds_prof_reset": (C.c_int, [C.c_void_p]),
    "omds_prof_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "omds_prof_read_ex": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                    C.POINTER(C.c_char_p)]),
    "omds_sync": (C.c_int, [C.c_void_p]),
    "omds_device_count": (C.c_int, [C.POINTER(C.c_int32)]),
}

# include/omds_test.h: exported by libomds_hip_test.so only (the product library does not have them)
TEST_HOOK_SIGNATURES = {
    "omds_screen_debug_corrupt": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float]),
    "omds_debug_force_tile_rows": (C.c_int, [C.c_int, C.c_int]),
    "omds_debug_trainer_general_gemm": (C.c_int, [C.c_int]),
    "omds_test_pack_mlp": (C.c_int, [C.c_int, C.c_int, I32P, I32P, C.POINTER(F32P), C.POINTER(F32P), C.c_int, C.c_float, C.c_int, I32P,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    "omds_test_trig": (C.c_int, [F32P, F32P, F32P, C.c_int64]),
    "omds_test_trig_sweep": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "omds_test_philox": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "omds_test_topk": (C.c_int, [F32P, C.c_int, C.c_int, C.c_int, I32P]),
    "omds_test_modulate": (C.c_int, [C.POINTER(OmdsTestModulateArgs)]),
}
# include/omds_test_tiles.h: the hooks of the block-ordered pass 1, in the test library likewise
TILE_HOOK_SIGNATURES = {
    "omds_test_tile_orders": (C.c_int, [C.c_void_p, I32P, I32P]),
    "omds_test_tile_state": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), I32P, I32P, I32P, F32P, F32P, F32P]),
    "omds_test_read_dmin": (C.c_int, [C.c_void_p, F32P]),
}
# include/omds_test_horizon.h: the hook of screening under an obstacle horizon, in the test library likewise
HORIZON_HOOK_SIGNATURES = {
    "omds_test_screen_corrupt_slab": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float]),
}
TEST_LIB_PATH = os.path.join(_HERE, "csrc", "libomds_hip_test.so")

ABI_VERSION = 512     # omds_version() of the library this binding was written against
_libs = {}             # path -> bound CDLL


def _autobuild(path=LIB_PATH):
    """`make` in csrc/, serialised across processes (torchrun starts one rank per GPU at once) by an exclusive
    lock; the Makefile links to a temporary name and renames, so no rank can dlopen a half-written library."""
    import fcntl
    import subprocess
    csrc = os.path.join(_HERE, "csrc")
    with open(os.path.join(csrc, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if os.path.exists(path):     # another rank built it while this one waited
                return
            r = subprocess.run(["make", "-C", csrc, "-j4"], capture_output=True, text=True)
            if r.returncode != 0:
                raise OmdsError(f"building {path} failed (make exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


def load(path=None, extra_signatures=None):
    """dlopen the in-tree library (or another build of it at ``path``) and bind every entry point.  Fails loudly when it
    is missing.  A handle created by one loaded library must only be passed to that library (``Engine`` keeps its own)."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path) and os.environ.get("OMDS_NO_AUTOBUILD") != "1":
        # the library is built in-tree by __graft_entry__.build(); if a checkout arrives without it, build it
        # here (hipcc, gfx950) -- still no fallback of any kind: without the library nothing runs
        _autobuild(path)
    if not os.path.exists(path):
        raise OmdsError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"or `make -C optimalmodulationds_amd/csrc` (there is no CPU fallback)")
    lib = C.CDLL(path)
    try:
        lib.omds_version.restype = C.c_int
        have = int(lib.omds_version())
    except AttributeError:
        have = -1
    if have != ABI_VERSION:     # a stale build of an older checkout: say so instead of failing on a missing symbol
        raise OmdsError(f"{path} is ABI version {have}, this package needs {ABI_VERSION}: rebuild it with "
                        f"`make -C optimalmodulationds_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`)")
    for name, (res, args) in dict(SIGNATURES, **(extra_signatures or {})).items():
        fn = getattr(lib, name)      # AttributeError = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    return lib


def load_test_hooks():
    """libomds_hip_test.so: the product's objects plus the hooks of include/omds_test.h (damage the screening inputs, force a tile
    shape, the trainer's general GEMM, the host half of omds_set_mlp_ex, the encoding's sin / cos, the raw words of the device's
    Philox4x32-10: omds_test_philox(ctr [n, 4] uint32, key [n, 2] uint32, out [n, 4] uint32, n), the top-k selection on given rows:
    ``select_topk`` below, one step of the modulation on given inputs: ``modulate_step`` below).  For tests only:
    ``Engine(..., lib=load_test_hooks())``."""
    return load(TEST_LIB_PATH, dict(TEST_HOOK_SIGNATURES, **TILE_HOOK_SIGNATURES, **HORIZON_HOOK_SIGNATURES))


def select_topk(rows, k):
    """omds_test_topk (include/omds_test.h): rows [B, O] float32 -> int32 [B, k], the indices of each row's k smallest entries as the
    production top-k kernel selects them.  Needs no context; loads the test library."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert rows.ndim == 2
    idx = np.full((rows.shape[0], int(k)), -2, np.int32)
    rc = load_test_hooks().omds_test_topk(rows.ctypes.data, rows.shape[0], rows.shape[1], int(k), idx.ctypes.data)
    if rc != 0:
        raise OmdsError(f"omds_test_topk failed ({rc})")
    return idx


def modulate_step(*, nsub, step, H, prm, qf, q, drow, gradx, mu, sigma, alpha, Kmax, maxact=None, phisum0=None, A=None, seds=None,
                  frame=False, frame_max=1.0, vel=None, row_obs=None, check=True):
    """omds_test_modulate (include/omds_test.h): ONE horizon step of the per-rollout modulation on the device, in the reference's
    layouts: q [N, n], drow [N, k], gradx [N, k, d], mu / alpha [N, K, n], sigma [N, K], the previous maxact [N, Kmax] and phisum0
    [Kmax] (None: the bits 0xFFFFFFFF), prm an OmdsParams, seds the keyword arguments of Engine.set_ds_seds, vel [O, ldVel] and
    row_obs [N, k] with ``frame``.  -> dict of float32 arrays q_next, qdot, normal [N, n], dist, dot, act [N], kval, maxact [N, Kmax],
    phisum0 [Kmax]; what the step did not write holds the bits 0xFFFFFFFF.  ``check`` False: returns the status code instead of
    raising.  Needs no context; loads the test library."""
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    q, drow, gradx, qf = f32(q), f32(drow), f32(gradx), f32(qf)
    N, n = q.shape
    k, d = gradx.shape[1], gradx.shape[2]
    assert drow.shape == (N, k) and gradx.shape[0] == N and qf.shape == (n,)
    mu, sigma, alpha = f32(mu), f32(sigma), f32(alpha)
    K = sigma.shape[1]
    assert mu.shape == (N, K, n) and alpha.shape == (N, K, n) and sigma.shape == (N, K)
    sentinel = lambda *shape: np.full(shape, 0xFFFFFFFF, np.uint32).view(np.float32)
    keep = [f32(mu.transpose(1, 2, 0)), f32(sigma.T), f32(alpha.transpose(1, 2, 0)), f32(q.T),
            sentinel(Kmax, N) if maxact is None else f32(np.asarray(maxact, np.float32).T),
            sentinel(Kmax) if phisum0 is None else f32(phisum0).copy()]
    muT, sigmaT, alphaT, qT, maxactT, ph0 = keep
    assert maxactT.shape == (Kmax, N) and ph0.shape == (Kmax,)
    out = dict(q_next=np.zeros((n, N), np.float32), qdot=np.zeros((n, N), np.float32), dist=np.zeros(N, np.float32),
               dot=np.zeros(N, np.float32), act=np.zeros(N, np.float32), normal=np.zeros((n, N), np.float32),
               kval=np.zeros((Kmax, N), np.float32))
    a = OmdsTestModulateArgs(n_dof=n, nsub=nsub, N=N, K=K, Kmax=Kmax, k=k, d=d, step=step, H=H, frame=int(bool(frame)), frame_max=frame_max,
                             prm=prm, qf=qf.ctypes.data, q=qT.ctypes.data, drow=drow.ctypes.data, gradx=gradx.ctypes.data,
                             mu=muT.ctypes.data if K else None, sigma=sigmaT.ctypes.data if K else None,
                             alpha=alphaT.ctypes.data if K else None, maxact=maxactT.ctypes.data, phisum0=ph0.ctypes.data,
                             **{name: arr.ctypes.data for name, arr in out.items()})
    if A is not None:
        A = f32(A)
        assert A.shape == (n, n)
        a.A = A.ctypes.data
    if seds is not None:
        sd = {name: f32(seds[name]) for name in ("mu_in", "b", "sigma_inv", "A", "prior", "den")}
        G = sd["prior"].shape[0]
        assert sd["mu_in"].shape == (G, n) and sd["b"].shape == (G, n) and sd["sigma_inv"].shape == (G, n, n) and sd["A"].shape == (G, n, n) \
            and sd["den"].shape == (G,)
        a.seds_G, a.seds_lin_thr, a.seds_thr = G, float(seds["lin_thr"]), float(seds["seds_thr"])
        for name, arr in sd.items():
            setattr(a, "seds_" + name, arr.ctypes.data)
    if frame:
        vel = f32(vel)
        row_obs = np.ascontiguousarray(row_obs, dtype=np.int32)
        assert vel.ndim == 2 and row_obs.shape == (N, k)
        a.O, a.ldVel, a.vel, a.rowObs = vel.shape[0], vel.shape[1], vel.ctypes.data, row_obs.ctypes.data
    rc = load_test_hooks().omds_test_modulate(C.byref(a))
    if not check:
        return rc
    if rc != 0:
        raise OmdsError(f"omds_test_modulate failed ({rc})")
    res = {name: np.ascontiguousarray(arr.T) for name, arr in out.items()}
    res["maxact"], res["phisum0"] = np.ascontiguousarray(maxactT.T), ph0
    return res


def f32(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    if shape is not None:
        a = a.reshape(shape)
    return a


def fptr(a):
    """Address of a C-contiguous float32 array (None -> NULL).  The argtypes are plain addresses, so ctypes neither checks the
    element type nor keeps ``a`` alive: pass a NAMED array that outlives the call -- never an inline temporary such as
    ``fptr(f32(x))`` or ``fptr(arr[::2].copy())`` -- and convert with ``f32`` first."""
    if a is None:
        return None
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"], "fptr: float32, C-contiguous arrays only"
    return a.ctypes.data


def iptr(a):
    """Address of a C-contiguous int32 array (None -> NULL); the same named-array rule as ``fptr``."""
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"], "iptr: int32, C-contiguous arrays only"
    return a.ctypes.data


def check(ctx, rc, lib=None):
    if rc != 0:
        msg = (lib or load()).omds_last_error(ctx)
        raise OmdsError(f"omds error {rc}: {msg.decode() if msg else '?'}")


def device_count() -> int:
    """HIP devices visible to this process (omds_device_count; 0 on a box without a GPU)."""
    n = C.c_int32(0)
    rc = load().omds_device_count(C.byref(n))
    if rc != 0:
        raise OmdsError(f"omds_device_count failed ({rc})")
    return int(n.value)


def comm_probe() -> str:
    """'' when RCCL can be loaded in this process, else the loader's message (omds_comm_probe)."""
    lib = load()
    return "" if lib.omds_comm_probe() == 0 else (lib.omds_comm_last_error() or b"RCCL not available").decode()


def default_params() -> OmdsParams:
    p = OmdsParams()
    load().omds_default_params(C.byref(p))
    return p
