"""Thin object wrapper over one ``omds_ctx`` (one per GPU): numpy in, numpy out.

The reference-shaped classes (MPPI, TensorPolicyMPPI, ...) and bench.py sit on top of this."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


class Engine:
    def __init__(self, n_dof, n_traj, horizon, n_closest, max_obs, n_kernel_max=50, device=0, flags=0, lib=None):
        self.lib = lib or L.load()   # lib: another build of the library (tests: _lib.load_test_hooks())
        self.n, self.N, self.H, self.k = int(n_dof), int(n_traj), int(horizon), int(n_closest)
        self.max_obs, self.Kmax, self.device = int(max_obs), int(n_kernel_max), int(device)
        cfg = L.OmdsConfig(self.n, self.N, self.H, self.Kmax, self.max_obs, self.k, self.device, int(flags))
        h = C.c_void_p()
        rc = self.lib.omds_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise L.OmdsError(f"omds_create failed ({rc}): {self.lib.omds_last_error(None).decode()}")
        self.h = h
        self.params = L.default_params()
        self.K = 0
        self.n_obs = 0
        self.depth_filter = None      # the depth filter in force (set_depth_filter), None: off
        self.depth_lenses = None      # the lenses in force (set_depth_lenses), None: off
        self.velocity_filter = None   # the velocity filter in force (set_velocity_filter), None: off
        self.C = 0
        self.config_version = 0      # bumped by every call that changes params / nominal DS / cost on the context (MPPI._push re-syncs on it)

    def close(self):
        if getattr(self, "h", None):
            self.lib.omds_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        L.check(self.h, rc, self.lib)

    # ---- configuration ------------------------------------------------------------------------
    def set_mlp(self, weights, biases, act="relu", out_div=None, skip_after=()):
        """``skip_after``: indices of the Linear layers behind whose activations the encoded input is concatenated
        (MLPRegression skips, network_macros_mod.py:142-146); empty for the plain sequential network."""
        Ws = [L.f32(w) for w in weights]
        bs = [L.f32(b) for b in biases]
        ins = np.array([w.shape[1] for w in Ws], dtype=np.int32)
        outs = np.array([w.shape[0] for w in Ws], dtype=np.int32)
        nl = len(Ws)
        Wp = (L.F32P * nl)(*[L.fptr(w) for w in Ws])
        bp = (L.F32P * nl)(*[L.fptr(b) for b in bs])
        C_out = int(outs[-1])
        if out_div is None:
            out_div = 100.0 if C_out == 9 else 1.0      # MPPI.py:236-237
        a = 0 if act == "relu" else 1
        sk = np.asarray(list(skip_after), dtype=np.int32)
        if sk.size or (ins[1:] != outs[:-1]).any():   # the explicit form also validates every layer's input width
            self._ck(self.lib.omds_set_mlp_ex(self.h, nl, L.iptr(ins), L.iptr(outs), Wp, bp, a, float(out_div), int(sk.size), L.iptr(sk)))
        else:
            dims = np.concatenate((ins[:1], outs)).astype(np.int32)
            self._ck(self.lib.omds_set_mlp(self.h, nl, L.iptr(dims), Wp, bp, a, float(out_div)))
        # a rejected network leaves the previous one installed (network.hip), so the wrapper's view changes only on success
        self.C = C_out
        self.n_hidden_levels = nl - 1
        self.d = int(ins[0]) // 3                       # raw network inputs: n + 3, or n + 2 for the toy networks

    def set_obstacles(self, obs):
        """Any obstacle count: beyond ``max_obs`` the context grows its obstacle buffers (omds.h)."""
        obs = L.f32(obs).reshape(-1, 4)
        self._ck(self.lib.omds_set_obstacles(self.h, L.fptr(obs), obs.shape[0]))
        self.n_obs = obs.shape[0]
        self.max_obs = max(self.max_obs, self.n_obs)

    # ---- the scene from a depth point cloud (omds.h: THE SCENE FROM A DEPTH POINT CLOUD) ------------------------------------------
    def set_obstacles_from_cloud(self, points, spec, q=None):
        """Crop, voxel down-sample and (``q`` [n] given: self-filter at that joint state, threshold ``spec.self_margin``) the cloud
        ``points`` [P, 3] on the device and install the spheres as the scene -> (n_spheres before padding, n_occupied cells).
        ``points``: host memory (numpy, a CPU tensor), or a float32 torch tensor on the context's device, which is passed by address.
        ``spec``: an ``OmdsCloudSpec`` (``cloud_spec`` builds one)."""
        return self._scene_from_cloud("set_obstacles_from_cloud", points, spec, q, None)[:2]

    def set_obstacles_from_cloud_tracked(self, points, spec, track, q=None):
        """``set_obstacles_from_cloud`` with one velocity per sphere, estimated on the device from the previous tracked frame (the
        normal flow of the surfaces: omds.h, SPHERE VELOCITIES FROM SUCCESSIVE CLOUDS) and installed as the motion horizon ->
        (n_spheres, n_occupied, n_matched).  ``track``: an ``OmdsCloudTrackSpec`` (``cloud_track_spec`` builds one).  n_matched is -1
        when there was no previous frame on this grid (the first call, after ``cloud_track_reset``, another grid): the frame is
        stored and the scene stands still.  It also stands still (horizon mode 0) when every velocity came out 0."""
        return self._scene_from_cloud("set_obstacles_from_cloud_tracked", points, spec, q, track)

    def set_obstacles_from_cloud_objects(self, points, spec, track, obj, q=None):
        """``set_obstacles_from_cloud_tracked`` with one velocity per OBJECT where one can be had (omds.h, OBJECT VELOCITIES FROM
        SUCCESSIVE CLOUDS): the final list is segmented into connected components on the device, the components are matched with those
        of the previous objects call by their centroids, and every sphere of a matched object takes the centroid's velocity; the
        other spheres keep the tracked call's -> (n_spheres, n_occupied, n_matched, n_objects, n_objects_matched).  ``obj``: an
        ``OmdsCloudObjectSpec`` (``cloud_object_spec`` builds one).  n_objects_matched is -1 when there was no previous component
        table (the first call, after ``cloud_track_reset``, another grid or object spec, a plain tracked call in between)."""
        return self._scene_from_cloud("set_obstacles_from_cloud_objects", points, spec, q, track, obj)

    def cloud_objects(self):
        """(label [n_obs], object [n_obs], n_objects) of the scene the objects cloud call installed: per sphere the label of its
        component (its smallest cell index; padding: -1) and whether it moves with a matched object (omds_get_cloud_objects; host
        state of the context, no GPU work)."""
        n_obs, n_objects = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacles(self.h, None, L.iptr(n_obs)))
        label, flag = np.zeros(max(int(n_obs[0]), 1), np.int32), np.zeros(max(int(n_obs[0]), 1), np.int32)
        self._ck(self.lib.omds_get_cloud_objects(self.h, L.iptr(label), L.iptr(flag), L.iptr(n_objects)))
        return label[:int(n_obs[0])], flag[:int(n_obs[0])], int(n_objects[0])

    def _scene_from_cloud(self, who, points, spec, q, track, obj=None):
        if hasattr(points, "data_ptr") and not points.is_cuda:      # a torch tensor in host memory
            points = points.detach().numpy()
        if hasattr(points, "data_ptr"):      # a torch tensor on a device
            if points.device.index != self.device:
                raise ValueError(f"{who}: a tensor must live on the context's device {self.device}, got {points.device}")
            import torch
            keep = points.detach().to(torch.float32).reshape(-1, 3).contiguous()
            torch.cuda.current_stream(keep.device).synchronize()      # the library reads it on its own stream
            addr, P, on_dev = keep.data_ptr() if keep.shape[0] else None, keep.shape[0], 1
        else:
            keep = L.f32(points).reshape(-1, 3)
            addr, P, on_dev = L.fptr(keep) if keep.shape[0] else None, keep.shape[0], 0
        qn = None if q is None else L.f32(q).reshape(self.n)
        o, p = _scene_outs()
        if obj is not None:
            rc = self.lib.omds_set_obstacles_from_cloud_objects(self.h, C.byref(spec), C.byref(track), C.byref(obj), addr, P, on_dev, L.fptr(qn),
                                                                *p[:5])
        elif track is None:
            rc = self.lib.omds_set_obstacles_from_cloud(self.h, C.byref(spec), addr, P, on_dev, L.fptr(qn), *p[:2])
        else:
            rc = self.lib.omds_set_obstacles_from_cloud_tracked(self.h, C.byref(spec), C.byref(track), addr, P, on_dev, L.fptr(qn), *p[:3])
        return self._scene_call_done(rc, qn, o, False, 5 if obj is not None else 3)

    def _scene_call_done(self, rc, qn, o, memory, n_out):
        """what follows every cloud / depth scene call (``o``: its counts, ``_scene_outs``): the wrapper's view of the scene, the error with
        its counts, and the first ``n_out`` of (n_spheres, n_occupied -- ``memory``: the five counts --, n_matched, n_objects,
        n_objects_matched)"""
        counts = tuple(int(v) for v in o[5:])
        candidates = counts[0] + counts[1] if memory else int(o[1])
        n_obs = np.zeros(1, np.int32)
        self.lib.omds_get_obstacles(self.h, None, L.iptr(n_obs))      # also after a failure: the context may have dropped its scene
        self.n_obs = int(n_obs[0])
        self.max_obs = max(self.max_obs, self.n_obs, candidates if (rc == 0 and qn is not None) else 0)      # the candidates were obstacle rows
        try:
            self._ck(rc)
        except L.OmdsError as e:
            e.n_occupied = candidates
            if memory:
                e.counts = counts
            raise
        return (int(o[0]), counts if memory else int(o[1]), int(o[2]), int(o[3]), int(o[4]))[:n_out]

    def _depth_call(self, who, images, cams, q):
        """what opens every depth scene call -> (the arguments from the camera table to q, q as the library takes it, the counts and their
        addresses as ``_scene_outs`` makes them, what has to stay alive over the call)"""
        table, addrs, n, on_dev, keep = _depth_table(who, images, cams, self.device)
        qn = None if q is None else L.f32(q).reshape(self.n)
        return (table, addrs, n, on_dev, L.fptr(qn)), qn, *_scene_outs(), keep

    def set_obstacles_from_depth(self, images, cams, spec, q=None, track=None, obj=None):
        """The scene straight from depth images (omds.h: THE SCENE STRAIGHT FROM DEPTH IMAGES): every effect is that of
        ``set_obstacles_from_cloud`` (``track`` None) / ``_tracked`` (``track``) / ``_objects`` (``track`` and ``obj``) on the
        concatenation of ``depth_points`` of each image, bit for bit, and so is what is returned (2, 3 or 5 counts).  ``images``: one
        per camera (a single image and camera may be passed bare), all numpy ``uint16`` / ``float32`` arrays [H, W], or all torch
        tensors on the engine's device (``uint16``; ``int16``, reinterpreted; ``float32``), which are read in place -- rows need not
        be contiguous as long as the last dimension has stride 1 (the camera's ``pitch`` is then taken from the row stride).  ``cams``:
        ``OmdsDepthCamera`` s (``depth_camera`` builds one); shape and format must be the image's."""
        args, qn, o, p, keep = self._depth_call("set_obstacles_from_depth", images, cams, q)
        rc = self.lib.omds_set_obstacles_from_depth(self.h, C.byref(spec), None if track is None else C.byref(track),
                                                    None if obj is None else C.byref(obj), *args, *p[:5])
        return self._scene_call_done(rc, qn, o, False, 2 if track is None else 5 if obj is not None else 3)

    # ---- the scene memory of the depth route (omds.h: THE SCENE MEMORY OF THE DEPTH ROUTE) ---------------------------------------------
    def set_obstacles_from_depth_memory(self, images, cams, spec, mem, q=None):
        """``set_obstacles_from_depth`` (the plain route) with a memory of occupancy between calls: a cell that got no points this call
        stays in the scene unless a camera looked through it (a return farther than the cell by ``mem.clear_margin``), it is older
        than ``mem.max_age`` calls, or the self-filter at ``q`` drops it -> (n_spheres before padding, counts): ``counts`` the cells
        (seen, remembered, cleared, expired, self-forgotten) as a tuple.  ``images``, ``cams``, ``spec``, ``q`` as there; ``mem``: an
        ``OmdsSceneMemorySpec`` (``scene_memory_spec`` builds one).  Installs a static scene.  More seen and remembered cells than
        ``spec.max_spheres`` raises with scene and memory unchanged; the error carries ``counts`` and ``n_occupied``."""
        args, qn, o, p, keep = self._depth_call("set_obstacles_from_depth_memory", images, cams, q)
        rc = self.lib.omds_set_obstacles_from_depth_memory(self.h, C.byref(spec), C.byref(mem), *args, p[0], p[5])
        return self._scene_call_done(rc, qn, o, True, 2)

    def set_obstacles_from_depth_memory_tracked(self, images, cams, spec, mem, track, objects=None, q=None):
        """``set_obstacles_from_depth_memory`` and ``set_obstacles_from_depth(track=[, obj=])`` in one call (omds.h: MEMORY AND
        VELOCITIES IN ONE DEPTH CALL), on the stored memory, record frame and component table those routes keep: the scene, the stored
        words, ``counts`` and the ages are the memory call's; the spheres whose cell was counted now carry the tracked (``objects``
        None) or objects (an ``OmdsCloudObjectSpec``) call's velocities, labels and flags; a remembered sphere, and a seen one that
        was occupied and unseen at the previous memory call, stands still -> (n_spheres, counts, n_matched, n_objects,
        n_objects_matched); n_matched is -1 without a stored frame on this grid, n_objects_matched -1 without a stored table, and
        n_objects 0 without ``objects``.  Raises like ``set_obstacles_from_depth_memory``, with scene, memory, frame and table
        unchanged."""
        args, qn, o, p, keep = self._depth_call("set_obstacles_from_depth_memory_tracked", images, cams, q)
        rc = self.lib.omds_set_obstacles_from_depth_memory_tracked(self.h, C.byref(spec), C.byref(mem), C.byref(track),
                                                                   None if objects is None else C.byref(objects), *args, p[0], p[5], *p[2:5])
        return self._scene_call_done(rc, qn, o, True, 5)

    # ---- the depth filter (omds.h: THE DEPTH FILTER) --------------------------------------------------------------------------------
    def set_depth_filter(self, spec):
        """The context's depth filter: an ``OmdsDepthFilterSpec`` (``depth_filter_spec`` builds one; a dict of its arguments is taken
        too), or None to turn it off; ``self.depth_filter`` holds the spec in force (None: off).  While set,
        ``set_obstacles_from_depth`` (every route) and ``set_obstacles_from_depth_memory`` drop flying pixels and speckle inside their
        counting pass: every effect is that of the cloud call on ``depth_points(image, cam, filter=spec)``.  A refused spec raises and
        leaves the stored filter as it was."""
        spec = _filter_of(spec)
        self._ck(self.lib.omds_set_depth_filter(self.h, None if spec is None else C.byref(spec)))
        self.depth_filter = spec      # behind the check: a refused spec leaves the stored one, here as in the library

    def depth_filter_stats(self):
        """(kept, rejected): the pixels the depth filter kept and rejected in the last depth call, summed over cameras; (0, 0) when
        no filter ran."""
        out = (C.c_int64 * 2)()
        self._ck(self.lib.omds_get_depth_filter_stats(self.h, out))
        return int(out[0]), int(out[1])

    # ---- the lenses of the depth cameras (omds.h: THE LENS OF A DEPTH CAMERA) ---------------------------------------------------------
    def set_depth_lenses(self, lenses):
        """The context's lenses: a list of ``OmdsDepthLens`` (``depth_lens`` builds one; a coefficient sequence or a dict of its
        arguments is taken too; None entries: no lens), lens i for camera i of every later depth call, or None to turn them off;
        ``self.depth_lenses`` holds the list in force (None: off).  While set, every depth route reads unrectified images: every effect
        is that of the cloud call on ``depth_points(image, cam, filter=, lens=)``.  A refused list raises and leaves the stored one."""
        table, n = _lens_table(lenses)
        self._ck(self.lib.omds_set_depth_lenses(self.h, table, n))
        self.depth_lenses = None if not n else [_lens_of(l) for l in lenses]

    def depth_lens_table(self, i):
        """(ab [entries, 2], r2_max, n_invalid) of the ray table the context holds for camera slot ``i``, as the last depth call that
        needed one left it: a pixel without a ray is (NaN, NaN).  No table: an empty array, 0.0, 0."""
        n, r2, bad = C.c_int64(0), C.c_float(0.0), C.c_int64(0)
        self._ck(self.lib.omds_get_depth_lens_table(self.h, int(i), None, None, None, C.byref(n)))
        ab = np.zeros((max(int(n.value), 1), 2), np.float32)
        self._ck(self.lib.omds_get_depth_lens_table(self.h, int(i), L.fptr(ab), C.addressof(r2), C.byref(bad), C.byref(n)))
        return ab[:int(n.value)], float(np.float32(r2.value)), int(bad.value)

    # ---- the velocity filter (omds.h: THE VELOCITY FILTER) ------------------------------------------------------------------------------
    def set_velocity_filter(self, spec):
        """The context's velocity filter: an ``OmdsVelocityFilterSpec`` (``velocity_filter_spec`` builds one; a dict of its arguments is
        taken too), or None to turn it off, which also empties its history; ``self.velocity_filter`` holds the spec in force (None:
        off).  While set, every call that estimates velocities (``set_obstacles_from_cloud_tracked`` / ``_objects``,
        ``set_obstacles_from_depth`` with ``track``, ``set_obstacles_from_depth_memory_tracked``) blends them against the smoothed
        velocity the context keeps per grid cell: everything but the installed velocities is the unfiltered call, bit for bit, and the
        velocities are ``velocity_filter_step`` on the stored state.  A refused spec raises and leaves the stored filter as it was."""
        spec = _vfilter_of(spec)
        self._ck(self.lib.omds_set_velocity_filter(self.h, None if spec is None else C.byref(spec)))
        self.velocity_filter = spec

    def velocity_filter_frame(self):
        """(raw [n_obs, 3], live [n_obs], stats) of the scene in force: the unfiltered velocities and matched flags of the filtered call
        that installed it (padding: 0), and (live spheres with history, restarts, groups with history) of that call
        (omds_get_velocity_filter_frame; host state, no GPU work).  Raises unless a filtered call installed the scene."""
        n_obs = np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacles(self.h, None, L.iptr(n_obs)))
        n = int(n_obs[0])
        raw, live, stats = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.int32), np.zeros(3, np.int32)
        self._ck(self.lib.omds_get_velocity_filter_frame(self.h, L.fptr(raw), L.iptr(live), L.iptr(stats)))
        return raw[:n], live[:n], tuple(int(v) for v in stats)

    def velocity_filter_state(self):
        """The stored state of the velocity filter, [cells, 4] int32 (q_x, q_y, q_z in 2^-16 m/s, hits), or None while the history
        is empty for want of a stored state (no filtered call yet, the filter cleared, ``cloud_track_reset``, a call without a
        previous frame)."""
        n_cells = np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_velocity_filter_state(self.h, None, L.iptr(n_cells)))
        if int(n_cells[0]) == 0:
            return None
        grid = np.zeros((int(n_cells[0]), 4), np.int32)
        self._ck(self.lib.omds_get_velocity_filter_state(self.h, L.iptr(grid), None))
        return grid

    def scene_memory_reset(self):
        """Forget the stored scene memory: the next ``set_obstacles_from_depth_memory`` starts from an empty one."""
        self._ck(self.lib.omds_scene_memory_reset(self.h))

    def get_scene_memory(self, grid=False):
        """age [n_obs] (int32) of the scene in force: calls since each sphere's cell was last counted (0: seen in the installing call),
        -1 for a padding sphere and everywhere when another setter installed the scene.  ``grid=True``: (age, words) with the stored
        memory words [cells] (uint32; 0 empty, k: last counted k - 1 calls ago), empty when no memory is stored."""
        n_obs, n_cells = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacles(self.h, None, L.iptr(n_obs)))
        age = np.full(max(int(n_obs[0]), 1), -1, np.int32)
        self._ck(self.lib.omds_get_scene_memory(self.h, L.iptr(age), None, L.iptr(n_cells)))
        age = age[:int(n_obs[0])]
        if not grid:
            return age
        words = np.zeros(max(int(n_cells[0]), 1), np.uint32)
        self._ck(self.lib.omds_get_scene_memory(self.h, None, words.ctypes.data, None))
        return age, words[:int(n_cells[0])]

    def cloud_track_reset(self):
        """Forget the previous tracked frame: the next ``set_obstacles_from_cloud_tracked`` stores its own and sets no velocities."""
        self._ck(self.lib.omds_cloud_track_reset(self.h))

    def get_obstacle_motion(self):
        """(vel [n_obs, 3], have): the velocities of the motion horizon in force (``set_obstacle_motion``, or the tracked cloud call)
        and whether there is one; zeros without (omds_get_obstacle_motion; host state of the context, no GPU work)."""
        n_obs, have = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacles(self.h, None, L.iptr(n_obs)))
        vel = np.zeros((int(n_obs[0]), 3), np.float32)
        self._ck(self.lib.omds_get_obstacle_motion(self.h, L.fptr(vel), L.iptr(have)))
        return vel, bool(have[0])

    def get_obstacles(self):
        """The scene in force, [n_obs, 4] (omds_get_obstacles; host state of the context, no GPU work)."""
        n_obs = np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacles(self.h, None, L.iptr(n_obs)))
        out = np.zeros((int(n_obs[0]), 4), np.float32)
        self._ck(self.lib.omds_get_obstacles(self.h, L.fptr(out), None))
        return out

    # ---- the obstacle focus: the spheres of a large scene near one joint state as the scene in force (omds.h) ---------------------
    def focus_obstacles(self, q, margin, max_keep=0, lookahead=0.0):
        """Select, on the device, the spheres of the MASTER scene (the scene in force at the first call; kept for the next) that are
        near joint state ``q`` [n] and install them as the scene in force -> (kept, passed).  Kept are the ``n_closest`` nearest and
        every sphere within ``margin`` metres of the farthest of those (``np.inf``: all), at most ``max_keep`` (0: no cap); a moving
        sphere is given ``lookahead`` seconds to approach.  Every scene setter ends the focus; ``set_obstacle_motion`` and
        ``set_obstacle_horizon`` raise while one is in force."""
        qn = L.f32(q).reshape(self.n)
        spec = obstacle_focus_spec(margin, max_keep, lookahead)
        kept, passed = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.lib.omds_focus_obstacles(self.h, C.byref(spec), L.fptr(qn), L.iptr(kept), L.iptr(passed)))
        self.n_obs = int(kept[0])
        return int(kept[0]), int(passed[0])

    def focus_obstacles_path(self, q_path, margin, max_keep=0, lookahead=0.0, ahead=None):
        """``focus_obstacles`` along joint states ``q_path`` [B, n] (1 <= B <= 65 536) -> (kept, passed): a sphere passes when it is
        within ``margin`` of the ``n_closest``-th nearest at SOME state, and the cap keeps those nearest to any state.  ``ahead`` [B]:
        the seconds until each state is reached, added to ``lookahead`` for a moving sphere (None: zeros)."""
        qn = L.f32(q_path).reshape(-1, self.n)
        a = None if ahead is None else L.f32(ahead).reshape(-1)
        if a is not None and a.shape[0] != qn.shape[0]:
            raise ValueError(f"focus_obstacles_path: ahead must be [{qn.shape[0]}], got {a.shape}")
        spec = obstacle_focus_spec(margin, max_keep, lookahead)
        kept, passed = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.lib.omds_focus_obstacles_path(self.h, C.byref(spec), L.fptr(qn), L.fptr(a), qn.shape[0], L.iptr(kept), L.iptr(passed)))
        self.n_obs = int(kept[0])
        return int(kept[0]), int(passed[0])

    def obstacle_focus(self):
        """The master index of every sphere in force (ascending, int32 [n_obs]), or None when no focus is in force."""
        n_master, n_kept = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacle_focus(self.h, None, L.iptr(n_master), L.iptr(n_kept)))
        if int(n_master[0]) == 0:
            return None
        idx = np.zeros(int(n_kept[0]), np.int32)
        self._ck(self.lib.omds_get_obstacle_focus(self.h, L.iptr(idx), None, None))
        return idx

    def clear_obstacle_focus(self):
        """Put the master scene and its motion back (a no-op without a focus)."""
        self._ck(self.lib.omds_clear_obstacle_focus(self.h))
        n_obs = np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacles(self.h, None, L.iptr(n_obs)))
        self.n_obs = int(n_obs[0])

    # ---- obstacle horizon: step i of a propagate sees slab i - 1 of a table [H, O, 4] (omds.h) ---------------------------------
    def set_obstacle_motion(self, vel):
        """Constant velocities ``vel`` [O, 3] of the spheres of the last ``set_obstacles``: step i of ``propagate`` sees them moved by
        (i - 1) dt vel (the table is built on the device with the ``params.dt`` in force at the propagate).  ``None`` clears it;
        so does every ``set_obstacles``."""
        if vel is None:
            self._ck(self.lib.omds_set_obstacle_motion(self.h, None))
            return
        v = L.f32(vel).reshape(-1, 3)
        if self.n_obs and v.shape[0] != self.n_obs:      # (no scene yet: the library says so)
            raise ValueError(f"set_obstacle_motion: velocities must be [{self.n_obs}, 3], got {v.shape}")
        self._ck(self.lib.omds_set_obstacle_motion(self.h, L.fptr(v)))

    def set_obstacle_horizon(self, xyzr_h):
        """The caller's own predictions ``xyzr_h`` [H, O, 4] (radii may change per slab); slab 0 must be the current scene bit for
        bit.  ``None`` clears it; so does every ``set_obstacles``."""
        if xyzr_h is None:
            self._ck(self.lib.omds_set_obstacle_horizon(self.h, None, 0))
            return
        t = L.f32(xyzr_h)
        if t.ndim != 3 or t.shape[0] != self.H or t.shape[2] != 4:
            raise ValueError(f"set_obstacle_horizon: the table must be [{self.H}, O, 4], got {t.shape}")
        self._ck(self.lib.omds_set_obstacle_horizon(self.h, L.fptr(t), t.shape[1]))

    def get_obstacle_horizon(self):
        """(table [H, O, 4] the next propagate will use, mode): mode 0 none (every slab is the static scene), 1 motion, 2 explicit."""
        out = np.zeros((self.H, self.n_obs, 4), np.float32)
        mode = np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_obstacle_horizon(self.h, L.fptr(out), L.iptr(mode)))
        return out, int(mode[0])

    # ---- the moving frame: the modulation relative to the obstacle's velocity as the joints see it (omds.h) ---------------------
    def set_obstacle_frame(self, moving, max_speed=None):
        """A preference: with ``moving`` and a motion horizon (``set_obstacle_motion``) every step of ``propagate`` modulates in the
        frame in which the blended obstacle rests and adds its velocity back.  ``max_speed`` clamps the approach speed (None: 1.0,
        the unit speed of the rollouts).  Without a motion horizon it changes nothing; with an explicit table ``propagate`` raises."""
        self._ck(self.lib.omds_set_obstacle_frame(self.h, 1 if moving else 0, 0.0 if max_speed is None else float(max_speed)))

    def get_obstacle_frame(self):
        """(moving, max_speed, in_effect): the preference, its clamp, and whether the next propagate runs in the moving frame."""
        mv, eff, ms = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
        self._ck(self.lib.omds_get_obstacle_frame(self.h, L.iptr(mv), L.fptr(ms), L.iptr(eff)))
        return bool(mv[0]), float(ms[0]), bool(eff[0])

    def approach_rate(self, q):
        """States ``q`` [B, n] -> (rate [B], qo [B, n]) against the current scene and the motion's velocities: the rate at which the
        blended distance changes because the spheres move (negative: approaching) and the joint velocity that keeps it constant."""
        q = L.f32(q).reshape(-1, self.n)
        rate, qo = np.zeros(q.shape[0], np.float32), np.zeros((q.shape[0], self.n), np.float32)
        self._ck(self.lib.omds_approach_rate(self.h, L.fptr(q), q.shape[0], L.fptr(rate), L.fptr(qo)))
        return rate, qo

    def set_ds(self, q_goal):
        q = L.f32(q_goal).reshape(self.n)
        self._ck(self.lib.omds_set_ds(self.h, L.fptr(q)))
        self.config_version += 1

    def set_ds_matrix(self, q_goal, A):
        """MPPI_toy's nominal DS: velocity = (q - q_goal) @ A (MPPI_toy.py:89)."""
        q = L.f32(q_goal).reshape(self.n)
        a = L.f32(A).reshape(self.n, self.n)
        self._ck(self.lib.omds_set_ds_matrix(self.h, L.fptr(q), L.fptr(a)))
        self.config_version += 1

    def set_ds_seds(self, q_goal, mu_in, b, sigma_inv, A, prior, den, lin_thr=1e-2, seds_thr=1e-2):
        """SEDS nominal DS (SEDS.py): G components; mu_in/b [G,n], sigma_inv/A [G,n,n], prior/den [G] as SEDS.__init__ / GMR
        derive them from the .mat file (optimalmodulationds_amd.seds.SEDS.device_params)."""
        q = L.f32(q_goal).reshape(self.n)
        mu_in, b = L.f32(mu_in), L.f32(b)
        G = mu_in.shape[0]
        si, a = L.f32(sigma_inv).reshape(G, self.n, self.n), L.f32(A).reshape(G, self.n, self.n)
        pr, dn = L.f32(prior).reshape(G), L.f32(den).reshape(G)
        self._ck(self.lib.omds_set_ds_seds(self.h, L.fptr(q), G, L.fptr(mu_in), L.fptr(b), L.fptr(si), L.fptr(a), L.fptr(pr), L.fptr(dn),
                                           float(lin_thr), float(seds_thr)))
        self.config_version += 1

    def push_params(self):
        self._ck(self.lib.omds_set_params(self.h, C.byref(self.params)))
        self.config_version += 1

    def set_cost(self, dh_params, q_min, q_max):
        dh = L.f32(dh_params).reshape(self.n + 1, 4)
        lo, hi = L.f32(q_min).reshape(self.n), L.f32(q_max).reshape(self.n)
        self._ck(self.lib.omds_set_cost(self.h, L.fptr(dh), L.fptr(lo), L.fptr(hi)))
        self.config_version += 1

    # ---- policy samples -----------------------------------------------------------------------
    def set_policy_samples(self, mu, sigma, alpha):
        mu = L.f32(mu)
        K = mu.shape[1] if mu.ndim == 3 else 0
        if K == 0:
            self._ck(self.lib.omds_set_policy_samples(self.h, None, None, None, 0))
        else:
            mu = mu.reshape(self.N, K, self.n)
            sg = L.f32(sigma).reshape(self.N, K)
            al = L.f32(alpha).reshape(self.N, K, self.n)
            self._ck(self.lib.omds_set_policy_samples(self.h, L.fptr(mu), L.fptr(sg), L.fptr(al), K))
        self.K = K

    def sample_policy(self, mu_c, sigma_c, alpha_c, mu_s, sigma_s, alpha_s, K, seed, rollout_offset=0):
        K = int(K)
        if K == 0:
            self._ck(self.lib.omds_sample_policy(self.h, None, None, None, 0, 0, 0, 0, int(seed), int(rollout_offset)))
        else:
            mu = L.f32(mu_c)[:K].reshape(K, self.n)
            sg = L.f32(sigma_c)[:K].reshape(K)
            al = L.f32(alpha_c)[:K].reshape(K, self.n)
            mu, sg, al = (np.ascontiguousarray(x) for x in (mu, sg, al))
            self._ck(self.lib.omds_sample_policy(self.h, L.fptr(mu), L.fptr(sg), L.fptr(al), float(mu_s), float(sigma_s),
                                                 float(alpha_s), K, int(seed), int(rollout_offset)))
        self.K = K

    def get_policy_samples(self):
        K = self.K
        mu = np.zeros((self.N, K, self.n), np.float32)
        sg = np.zeros((self.N, K), np.float32)
        al = np.zeros((self.N, K, self.n), np.float32)
        if K:
            self._ck(self.lib.omds_get_policy_samples(self.h, L.fptr(mu), L.fptr(sg), L.fptr(al)))
        return mu, sg, al

    # ---- rollouts -----------------------------------------------------------------------------
    def propagate(self, q_cur):
        q = L.f32(q_cur)
        per = 1 if q.ndim == 2 else 0
        q = q.reshape(self.N, self.n) if per else q.reshape(self.n)
        self._ck(self.lib.omds_propagate(self.h, L.fptr(q), per))

    def get_rollouts(self, want=("all_traj", "closest_dist_all", "kernel_val_all", "dot_products",
                                 "kernel_activations", "qdot", "normal")):
        N, H, n, K = self.N, self.H, self.n, self.K
        shapes = {"all_traj": (N, H, n), "closest_dist_all": (N, H), "kernel_val_all": (N, H, K),
                  "dot_products": (N, H), "kernel_activations": (N, H), "qdot": (N, n), "normal": (N, H, n)}
        out = {k: (np.zeros(shapes[k], np.float32) if k in want else None) for k in shapes}
        order = ["all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal"]
        ptrs = [L.fptr(out[k]) if (out[k] is not None and out[k].size) else None for k in order]
        self._ck(self.lib.omds_get_rollouts(self.h, *ptrs))
        return {k: v for k, v in out.items() if v is not None}

    def get_rollout_rows(self, t, want=("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations",
                                        "qdot", "normal")):
        """The same tensors for the rollouts ``t`` (indices) only: [len(t), H, ...] -- a few KB instead of the N x H tensors."""
        t = np.ascontiguousarray(np.atleast_1d(np.asarray(t)).astype(np.int32))
        R, H, n, K = t.shape[0], self.H, self.n, self.K
        shapes = {"all_traj": (R, H, n), "closest_dist_all": (R, H), "kernel_val_all": (R, H, K), "dot_products": (R, H),
                  "kernel_activations": (R, H), "qdot": (R, n), "normal": (R, H, n)}
        out = {k: (np.zeros(shapes[k], np.float32) if k in want else None) for k in shapes}
        order = ["all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal"]
        ptrs = [L.fptr(out[k]) if (out[k] is not None and out[k].size) else None for k in order]
        self._ck(self.lib.omds_get_rollout_rows(self.h, L.iptr(t), R, *ptrs))
        return {k: v for k, v in out.items() if v is not None}

    def dist_grad(self, q, want_mindist=False, want_idx=False):
        q = L.f32(q).reshape(-1, self.n)
        B = q.shape[0]
        dist = np.zeros(B, np.float32)
        grad = np.zeros((B, self.n), np.float32)
        mind = np.zeros((B, self.n_obs), np.float32) if want_mindist else None
        idx = np.zeros((B, self.k), np.int32) if want_idx else None
        self._ck(self.lib.omds_dist_grad(self.h, L.fptr(q), B, L.fptr(dist), L.fptr(grad), L.fptr(mind), L.iptr(idx)))
        return dist, grad, mind, idx

    def mlp_forward_vjp(self, x):
        x = L.f32(x).reshape(-1, self.d)
        B = x.shape[0]
        y = np.zeros((B, self.C), np.float32)
        g = np.zeros((B, self.d), np.float32)
        mi = np.zeros(B, np.int32)
        self._ck(self.lib.omds_mlp_forward_vjp(self.h, L.fptr(x), B, L.fptr(y), L.fptr(g), L.iptr(mi)))
        return y, g, mi

    def mlp_jacobian(self, x, cols):
        """(y [B,C], jac [B,d,len(cols)]): Jacobian columns of the listed raw outputs (omds_mlp_jacobian)."""
        x = L.f32(x).reshape(-1, self.d)
        cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        B = x.shape[0]
        y = np.zeros((B, self.C), np.float32)
        jac = np.zeros((B, self.d, cols.size), np.float32)
        self._ck(self.lib.omds_mlp_jacobian(self.h, L.fptr(x), B, L.iptr(cols), int(cols.size), L.fptr(y), L.fptr(jac)))
        return y, jac

    # ---- cost / update ------------------------------------------------------------------------
    def cost(self, fetch=True):
        c = np.zeros(self.N, np.float32) if fetch else None
        self._ck(self.lib.omds_cost(self.h, L.fptr(c)))
        return c

    def cost_eval(self, all_traj, closest_dist_all):
        """Cost.evaluate_costs on arbitrary [B,H,n] / [B,H] tensors (device evaluation, any B: chunks of N)."""
        tr = L.f32(all_traj).reshape(-1, self.H, self.n)
        di = L.f32(closest_dist_all).reshape(-1, self.H)
        out = np.zeros(tr.shape[0], np.float32)
        for s in range(0, tr.shape[0], self.N):
            a, b, o = np.ascontiguousarray(tr[s:s + self.N]), np.ascontiguousarray(di[s:s + self.N]), out[s:s + self.N]
            self._ck(self.lib.omds_cost_eval(self.h, L.fptr(a), L.fptr(b), a.shape[0], L.fptr(o)))
        return out

    def weighted_update(self, rate, ker_thr, mu_c, sigma_c, alpha_c, want_weights=False):
        K = self.K
        # copies: the C function updates the means in place and must not alias the caller's arrays
        mu = np.array(np.asarray(mu_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, self.n)
        sg = np.array(np.asarray(sigma_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K)
        al = np.array(np.asarray(alpha_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, self.n)
        mask = np.zeros(K, np.int32)
        w = np.zeros(self.N, np.float32) if want_weights else None
        self._ck(self.lib.omds_weighted_update(self.h, float(rate), float(ker_thr), L.fptr(mu), L.fptr(sg), L.fptr(al),
                                               L.iptr(mask), L.fptr(w)))
        return mu, sg, al, mask.astype(bool), w

    def weighted_update_eval(self, cost, kernel_val_all, kernel_activations, rate, ker_thr, mu_c, sigma_c, alpha_c, want_weights=False):
        """shift_policy_means on caller-supplied tensors (cost [N], kernel_val_all [N,H,K], kernel_activations [N,H]) against the
        policy samples the context holds; the context's own rollouts and cost stay untouched."""
        K = self.K
        c = L.f32(cost).reshape(self.N)
        kv = np.ascontiguousarray(L.f32(kernel_val_all).reshape(self.N, self.H, -1)[:, :, :K]) if K else None
        ka = L.f32(kernel_activations).reshape(self.N, self.H)
        mu = np.array(np.asarray(mu_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, self.n)
        sg = np.array(np.asarray(sigma_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K)
        al = np.array(np.asarray(alpha_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, self.n)
        mask = np.zeros(K, np.int32)
        w = np.zeros(self.N, np.float32) if want_weights else None
        self._ck(self.lib.omds_weighted_update_eval(self.h, L.fptr(c), L.fptr(kv), L.fptr(ka), float(rate), float(ker_thr),
                                                    L.fptr(mu), L.fptr(sg), L.fptr(al), L.iptr(mask), L.fptr(w)))
        return mu, sg, al, mask.astype(bool), w

    def get_qdot(self, mode="best"):
        out = np.zeros(self.n, np.float32)
        self._ck(self.lib.omds_get_qdot(self.h, 0 if mode == "best" else 1, L.fptr(out)))
        return out

    def cost_sum(self):
        out = np.zeros(2, np.float32)
        self._ck(self.lib.omds_cost_sum(self.h, L.fptr(out)))
        return out

    def local_sums(self, sum_cost, n_total, include_rollout0=True):
        red = np.zeros(self.lib.omds_red_count(self.h), np.float32)
        self._ck(self.lib.omds_local_sums(self.h, float(sum_cost), float(n_total), 1 if include_rollout0 else 0,
                                          L.fptr(red)))
        return red

    # ---- multi-GPU: native RCCL exchange (comm.hip) -------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128-byte RCCL id (rank 0 makes it, the launcher ships it to the other ranks)."""
        lib = L.load()
        buf = (C.c_uint8 * 128)()
        rc = lib.omds_comm_unique_id(buf)
        if rc != 0:
            raise L.OmdsError(f"omds_comm_unique_id failed ({rc}): {(lib.omds_comm_last_error() or b'?').decode()}")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._ck(self.lib.omds_comm_init_rank(self.h, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._ck(self.lib.omds_comm_destroy(self.h))

    def comm_info(self):
        r, w = C.c_int32(), C.c_int32()
        self._ck(self.lib.omds_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_active(self):
        """True while the context owns an RCCL communicator (a single-rank one included)."""
        return bool(self.lib.omds_comm_active(self.h))

    def weighted_update_sharded(self, rate, ker_thr, mu_c, sigma_c, alpha_c, want_best=False):
        """MPPI.shift_policy_means + get_qdot over all shards of the communicator (all-reduces on the context
        stream, device buffers).  Returns (mu, sigma, alpha, mask, qdot_weighted, qdot_best | None, n_total)."""
        K = self.K
        mu = np.array(np.asarray(mu_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, self.n)
        sg = np.array(np.asarray(sigma_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K)
        al = np.array(np.asarray(alpha_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, self.n)
        mask = np.zeros(K, np.int32)
        qw = np.zeros(self.n, np.float32)
        qb = np.zeros(self.n, np.float32) if want_best else None
        nt = C.c_float()
        self._ck(self.lib.omds_weighted_update_sharded(self.h, float(rate), float(ker_thr), L.fptr(mu), L.fptr(sg),
                                                       L.fptr(al), L.iptr(mask), L.fptr(qw), L.fptr(qb),
                                                       C.cast(C.byref(nt), L.F32P)))
        return mu, sg, al, mask.astype(bool), qw, qb, nt.value

    def kernel_candidates(self, thr_dist, thr_kernel, thr_dot, mu_c, sigma_c, K, cap=None):
        """Device-side TensorPolicyMPPI.check_traj_for_kernels: (cand_q [m,n], cand_th [m,2], total)."""
        K = int(K)
        cap = int(self.N * self.H if cap is None else cap)
        mu = np.array(np.asarray(mu_c, dtype=np.float32)[:K], dtype=np.float32, order="C").reshape(K, self.n)
        sg = np.array(np.asarray(sigma_c, dtype=np.float32)[:K], dtype=np.float32, order="C").reshape(K)
        q = np.zeros((cap, self.n), np.float32)
        th = np.zeros((cap, 2), np.int32)
        cnt = C.c_int32(0)
        self._ck(self.lib.omds_kernel_candidates(self.h, float(thr_dist), float(thr_kernel), float(thr_dot), L.fptr(mu),
                                                 L.fptr(sg), K, cap, L.fptr(q), L.iptr(th), C.byref(cnt)))
        m = min(cnt.value, cap)
        return q[:m], th[:m], cnt.value

    # ---- screening of pass 1 (fp16 + exact re-selection) ----------------------------------------
    def set_screening(self, mode=-1, eps=0.0):
        """mode: -1 library default (off, or `OMDS_SCREEN`), 0 off, 1 on, 2 on where it pays; eps > 0 fixes the error bound, 0 keeps bound and calibration
        (mode change only), < 0 discards the calibration (measured again at the next screened propagate)."""
        self._ck(self.lib.omds_set_screening(self.h, int(mode), float(eps)))

    def set_screening_horizon(self, on=True):
        """Screening while an obstacle horizon is set (``set_obstacle_motion`` / ``set_obstacle_horizon``).  Off (the default): a
        horizon puts the context on the all-fp32 step.  On: such a propagate is screened like a static one, every step against its
        own slab (omds.h: omds_set_screening_horizon)."""
        self._ck(self.lib.omds_set_screening_horizon(self.h, 1 if on else 0))

    def get_screening_horizon(self):
        """(on, in_effect): the switch, and whether the next propagate would run a screened route with a horizon set."""
        on, eff = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self._ck(self.lib.omds_get_screening_horizon(self.h, L.iptr(on), L.iptr(eff)))
        return bool(on[0]), bool(eff[0])

    def set_screening_audit(self, one_in=64):
        """Audit sample of the pairs the screened step does not re-evaluate: 1 in ``one_in`` (power of two), 0 = none."""
        self._ck(self.lib.omds_set_screening_audit(self.h, int(one_in)))

    def set_screening_sweep(self, every=32, all_steps=False):
        """Every ``every``-th screened propagate checks ALL pairs of its last horizon step in fp32 (0 = never); with
        ``all_steps`` of every horizon step (soak / qualification runs)."""
        self._ck(self.lib.omds_set_screening_sweep(self.h, int(every), 1 if all_steps else 0))

    def sweep_hist(self, reset=False):
        """What all sweeps so far have counted (omds.h: omds_screen_sweep_hist), as a dict: pair counts, the largest
        ``Da - D`` over the pairs that were NOT candidates, and its distribution in log2 bins (``pos`` / ``neg``: bin b holds
        2^(b-32) <= |x| < 2^(b-31)) and in 128 linear bins of ``(Da - D) / eps`` over [0, 1) (``ratio``)."""
        w = (C.c_uint64 * L.SWEEP_HIST_WORDS)()
        self._ck(self.lib.omds_screen_sweep_hist(self.h, w, L.SWEEP_HIST_WORDS, 1 if reset else 0))
        a = np.frombuffer(w, dtype=np.uint64).copy()
        f = lambda bits: float(np.array([bits & 0xffffffff], np.uint32).view(np.float32)[0])
        Lb, Rb = L.SWEEP_HIST_LOG_BINS, L.SWEEP_HIST_RATIO_BINS
        return dict(pairs=int(a[0]), non_candidates=int(a[1]), above_half_eps=int(a[2]), above_eps=int(a[3]), non_finite=int(a[4]),
                    max_pos=f(int(a[5])), max_abs=f(int(a[6])), steps=int(a[7]), pos=a[8:8 + Lb].astype(np.int64),
                    neg=a[8 + Lb:8 + 2 * Lb].astype(np.int64), ratio=a[8 + 2 * Lb:8 + 2 * Lb + Rb].astype(np.int64))

    def screen_debug_corrupt(self, what, index, value=0.0):
        """Test hook (include/omds_test.h; needs ``lib=_lib.load_test_hooks()``): 0 = zero a weight fragment of the fp16 pack,
        1 = shift an obstacle in the screening inputs."""
        self._ck(self.lib.omds_screen_debug_corrupt(self.h, int(what), int(index), float(value)))

    def test_screen_corrupt_slab(self, slab, index, dx):
        """Test hook (include/omds_test_horizon.h; needs ``lib=_lib.load_test_hooks()``): shift obstacle ``index`` by ``dx`` along x
        in the fp16 screening table of horizon slab ``slab`` only; the tables must exist (``get_obstacle_horizon`` builds them)."""
        self._ck(self.lib.omds_test_screen_corrupt_slab(self.h, int(slab), int(index), float(dx)))

    def debug_force_tile_rows(self, tail_sel_rows=0, tail_rows=0):
        """Test hook (include/omds_test.h; needs ``lib=_lib.load_test_hooks()``; wide to that library): tile shape of the tail
        kernels; 0 = the launcher's own choice again."""
        self._ck(self.lib.omds_debug_force_tile_rows(int(tail_sel_rows), int(tail_rows)))

    def test_tile_orders(self):
        """Test hook (include/omds_test_tiles.h; needs ``lib=_lib.load_test_hooks()``): (rperm [n_traj], operm [n_obs]) of the last
        block-ordered pass-1 launch (``flags``: ``_lib.FLAG_BLOCK_TILES`` forces that order, ``FLAG_NATURAL_TILES`` forbids it)."""
        rperm, operm = np.zeros(self.N, np.int32), np.zeros(self.n_obs, np.int32)
        self._ck(self.lib.omds_test_tile_orders(self.h, L.iptr(rperm), L.iptr(operm)))
        return rperm, operm

    def test_tile_state(self):
        """Test hook (include/omds_test_tiles.h; needs ``lib=_lib.load_test_hooks()``): what the ordering launches of the last
        block-ordered pass 1 left, as a dict: ``rkey`` [n_traj] / ``okey`` [n_obs] (uint32: sign bits << 20 | index), ``rperm`` /
        ``operm`` WITH their padding (``order_pad(n)`` entries), and the propagate's key units ``unit`` [12], ``W`` [12, 32],
        ``cR`` [12], ``cO`` [12]."""
        import ctypes as C
        pad = lambda n: ((n + 15) & ~15) + 16      # omds_test_order_pad
        out = {"rkey": np.zeros(self.N, np.uint32), "okey": np.zeros(self.n_obs, np.uint32),
               "rperm": np.zeros(pad(self.N), np.int32), "operm": np.zeros(pad(self.n_obs), np.int32),
               "unit": np.zeros(12, np.int32), "W": np.zeros((12, 32), np.float32), "cR": np.zeros(12, np.float32),
               "cO": np.zeros(12, np.float32)}
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        self._ck(self.lib.omds_test_tile_state(self.h, u32(out["rkey"]), u32(out["okey"]), L.iptr(out["rperm"]), L.iptr(out["operm"]),
                                               L.iptr(out["unit"]), L.fptr(out["W"]), L.fptr(out["cR"]), L.fptr(out["cO"])))
        return out

    def test_read_dmin(self):
        """Test hook (include/omds_test_tiles.h; needs ``lib=_lib.load_test_hooks()``): the [n_traj, n_obs] pass-1 matrix the last
        step of the last propagate left."""
        out = np.zeros((self.N, self.n_obs), np.float32)
        self._ck(self.lib.omds_test_read_dmin(self.h, L.fptr(out)))
        return out

    def screen_mindist(self, q):
        q = L.f32(q).reshape(-1, self.n)
        out = np.zeros((q.shape[0], self.n_obs), np.float32)
        self._ck(self.lib.omds_screen_mindist(self.h, L.fptr(q), q.shape[0], L.fptr(out)))
        return out

    def screen_stats(self):
        act, eps, err = C.c_int32(), C.c_float(), C.c_float()
        cand, fb = C.c_double(), C.c_int64()
        self._ck(self.lib.omds_screen_stats(self.h, C.byref(act), C.cast(C.byref(eps), L.F32P), C.cast(C.byref(err), L.F32P),
                                            C.byref(cand), C.byref(fb)))
        one_in, susp, aerr = C.c_int32(), C.c_int32(), C.c_float()
        arows, ncal = C.c_double(), C.c_int64()
        self._ck(self.lib.omds_screen_audit_stats(self.h, C.byref(one_in), C.byref(arows), C.cast(C.byref(aerr), L.F32P),
                                                  C.byref(susp), C.byref(ncal)))
        sw_every, sw_n, sw_err = C.c_int32(), C.c_int64(), C.c_float()
        self._ck(self.lib.omds_screen_sweep_stats(self.h, C.byref(sw_every), C.byref(sw_n), C.byref(sw_err)))
        fe, fs, fo, ns = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self.lib.omds_screen_fallback_stats(self.h, C.byref(fe), C.byref(fs), C.byref(fo), C.byref(ns)))
        nre = C.c_int64()
        never = np.zeros(9, np.int32)
        self._ck(self.lib.omds_screen_order_stats(self.h, C.byref(nre), L.iptr(never), 9))
        return dict(unit_reorders=nre.value, units_never_fired=[int(v) for v in never[:max(1, getattr(self, "n_hidden_levels", 9))]],
                    fallbacks_by_error=fe.value, fallbacks_by_slack=fs.value, fallbacks_by_overflow=fo.value, suspensions=ns.value,
                    active=bool(act.value), eps=eps.value, max_err_seen=err.value, candidates_per_rollout_step=cand.value,
                    fallbacks=fb.value, audit_one_in=one_in.value, audit_rows_per_rollout_step=arows.value,
                    audit_max_err=aerr.value, suspended=bool(susp.value), calibrations=ncal.value,
                    sweep_every=sw_every.value, sweeps=sw_n.value, sweep_max_err=sw_err.value)

    # ---- measurement --------------------------------------------------------------------------
    def pass1_skip_stats(self):
        """omds_pass1_skip_stats: dict(active, units, chunks [mean per tile and hidden level since set_mlp], tiles)."""
        act, tiles = C.c_int32(), C.c_int64()
        un, ch = (C.c_double * 9)(), (C.c_double * 9)()
        self._ck(self.lib.omds_pass1_skip_stats(self.h, C.byref(act), un, ch, 9, C.byref(tiles)))
        nl = getattr(self, "n_hidden_levels", 9)
        return dict(active=bool(act.value), units=[float(u) for u in un][:nl], chunks=[float(c) for c in ch][:nl], tiles=int(tiles.value))

    def pipeline_info(self):
        """omds_get_pipeline_info: (parts, split) of the last propagate -- (2, split) when its full steps ran as the rollouts [0, split)
        and [split, N) on two streams, else (1, N)."""
        parts, split = C.c_int32(), C.c_int32()
        self._ck(self.lib.omds_get_pipeline_info(self.h, C.byref(parts), C.byref(split)))
        return int(parts.value), int(split.value)

    def sync(self):
        """Waits for everything enqueued on the context's stream (omds_sync)."""
        self._ck(self.lib.omds_sync(self.h))

    def prof_enable(self, on=True):
        """on: False/0 off, True/1 every launch of the dominant kernel, n > 1 every n-th launch."""
        self._ck(self.lib.omds_prof_enable(self.h, int(on)))

    def prof_reset(self):
        self._ck(self.lib.omds_prof_reset(self.h))

    def prof_read(self):
        ms, nl, nr = C.c_double(), C.c_int64(), C.c_int64()
        self._ck(self.lib.omds_prof_read(self.h, C.byref(ms), C.byref(nl), C.byref(nr)))
        return ms.value, nl.value, nr.value


def _prof_read_ex(self):
    ms, nl, fl, name = C.c_double(), C.c_int64(), C.c_double(), C.c_char_p()
    self._ck(self.lib.omds_prof_read_ex(self.h, C.byref(ms), C.byref(nl), C.byref(fl), C.byref(name)))
    return ms.value, nl.value, fl.value, (name.value or b"").decode()


Engine.prof_read_ex = _prof_read_ex


def predict_obstacle_horizon(obs, vel, horizon, dt):
    """Constant-velocity prediction on the host (omds_obstacle_horizon_predict, no GPU): obs [O, 4], vel [O, 3] ->
    [horizon, O, 4] with slab h = obs moved by (h dt) vel, radii kept.  What ``Engine.set_obstacle_motion`` builds on the device."""
    lib = L.load()
    o = L.f32(obs).reshape(-1, 4)
    v = L.f32(vel).reshape(-1, 3)
    if v.shape[0] != o.shape[0]:
        raise ValueError(f"predict_obstacle_horizon: {o.shape[0]} obstacles but {v.shape[0]} velocities")
    out = np.zeros((int(horizon), o.shape[0], 4), np.float32)
    rc = lib.omds_obstacle_horizon_predict(L.fptr(o), L.fptr(v), o.shape[0], int(horizon), float(dt), L.fptr(out))
    if rc != 0:
        raise L.OmdsError(f"omds_obstacle_horizon_predict failed ({rc}): {lib.omds_last_error(None).decode()}")
    return out


def cloud_spec(origin, voxel, dims, radius=0.0, min_points=1, max_spheres=4096, self_margin=0.0, pad=(10.0, 10.0, 10.0, 0.0)):
    """An ``OmdsCloudSpec``: the voxel grid with lower corner ``origin``, edge ``voxel`` and ``dims`` cells per axis; ``radius <= 0``
    selects the cell's circumsphere; ``pad`` is the sphere that fills a scene of fewer than n_closest spheres (default: far away)."""
    s = L.OmdsCloudSpec()
    s.origin[:] = [float(v) for v in origin]
    s.voxel = float(voxel)
    s.dims[:] = [int(v) for v in dims]
    s.radius = float(radius)
    s.min_points, s.max_spheres = int(min_points), int(max_spheres)
    s.self_margin = float(self_margin)
    s.pad[:] = [float(v) for v in pad]
    return s


def cloud_track_spec(reach, dt_frame, still=0.0):
    """An ``OmdsCloudTrackSpec``: match within ``reach`` cells (1 .. 4) per axis each way, ``dt_frame`` seconds since the previous
    tracked frame, speeds below ``still`` become exactly 0 (<= 0: off)."""
    t = L.OmdsCloudTrackSpec()
    t.reach, t.dt_frame, t.still = int(reach), float(dt_frame), float(still)
    return t


def cloud_object_spec(link=1, min_cells=4):
    """An ``OmdsCloudObjectSpec``: spheres whose cells are at most ``link`` cells apart (1 .. 2, Chebyshev) belong to one component; a
    component of fewer than ``min_cells`` cells is no object."""
    o = L.OmdsCloudObjectSpec()
    o.link, o.min_cells = int(link), int(min_cells)
    return o


def obstacle_focus_spec(margin, max_keep=0, lookahead=0.0):
    """An ``OmdsObstacleFocusSpec``: keep the spheres within ``margin`` metres (>= 0, ``np.inf``: all) of the n_closest-th nearest, at
    most ``max_keep`` of them (< 1: no cap), a moving sphere given ``lookahead`` seconds to approach."""
    s = L.OmdsObstacleFocusSpec()
    s.margin, s.lookahead, s.max_keep = float(margin), float(lookahead), int(max_keep)
    return s


def obstacle_focus_select(d, n_closest, margin, max_keep=0, lookahead=0.0, vel=None, cap=None):
    """The definition of the obstacle focus on the host (omds_obstacle_focus_select; no context, no GPU): distances ``d`` [O] and
    optional velocities ``vel`` [O, 3] -> (idx, passed): the kept indices in ascending order (int32) and the number that passed."""
    lib = L.load()
    d = L.f32(d).reshape(-1)
    v = None if vel is None else L.f32(vel).reshape(-1, 3)
    if v is not None and v.shape[0] != d.shape[0]:
        raise ValueError(f"obstacle_focus_select: velocities must be [{d.shape[0]}, 3], got {v.shape}")
    cap = d.shape[0] if cap is None else int(cap)
    spec = obstacle_focus_spec(margin, max_keep, lookahead)
    idx, kept, passed = np.zeros(max(cap, 1), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = lib.omds_obstacle_focus_select(C.byref(spec), L.fptr(d), L.fptr(v), d.shape[0], int(n_closest), L.iptr(idx), cap, L.iptr(kept),
                                        L.iptr(passed))
    if rc != 0:
        raise L.OmdsError(f"omds_obstacle_focus_select failed ({rc}): {lib.omds_last_error(None).decode()}")
    return idx[:int(kept[0])].copy(), int(passed[0])


def obstacle_focus_select_path(d, n_closest, margin, max_keep=0, lookahead=0.0, ahead=None, vel=None, cap=None):
    """The definition of the obstacle focus along a path on the host (omds_obstacle_focus_select_path; no context, no GPU): distances
    ``d`` [B, O], one row per state, optional ``ahead`` [B] seconds and velocities ``vel`` [O, 3] -> (idx, passed)."""
    lib = L.load()
    d = L.f32(d)
    if d.ndim != 2:
        raise ValueError(f"obstacle_focus_select_path: distances must be [B, O], got {d.shape}")
    B, O = d.shape
    a = None if ahead is None else L.f32(ahead).reshape(-1)
    v = None if vel is None else L.f32(vel).reshape(-1, 3)
    if a is not None and a.shape[0] != B:
        raise ValueError(f"obstacle_focus_select_path: ahead must be [{B}], got {a.shape}")
    if v is not None and v.shape[0] != O:
        raise ValueError(f"obstacle_focus_select_path: velocities must be [{O}, 3], got {v.shape}")
    cap = O if cap is None else int(cap)
    spec = obstacle_focus_spec(margin, max_keep, lookahead)
    idx, kept, passed = np.zeros(max(cap, 1), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = lib.omds_obstacle_focus_select_path(C.byref(spec), L.fptr(d), L.fptr(a), L.fptr(v), B, O, int(n_closest), L.iptr(idx), cap, L.iptr(kept),
                                             L.iptr(passed))
    if rc != 0:
        raise L.OmdsError(f"omds_obstacle_focus_select_path failed ({rc}): {lib.omds_last_error(None).decode()}")
    return idx[:int(kept[0])].copy(), int(passed[0])


def depth_camera(width, height, fx, fy, cx, cy, pose=None, format=L.DEPTH_U16, depth_scale=0.001, z_min=0.1, z_max=10.0, step=1, pitch=0):
    """An ``OmdsDepthCamera``: a ``width`` x ``height`` depth image (``format``: ``DEPTH_U16`` raw units of ``depth_scale`` metres, 0 = no
    return, or ``DEPTH_F32`` metres) of a pinhole camera (``fx``, ``fy``, ``cx``, ``cy``), range-gated to ``z_min`` .. ``z_max`` along the
    optical axis, of which rows and columns 0, ``step``, 2 ``step``, ... are visited.  ``pose``: camera -> the frame of the voxel grid,
    a 3 x 4 or 4 x 4 matrix [R | t] (None: the identity).  ``pitch``: elements between row starts (0: ``width``)."""
    c = L.OmdsDepthCamera()
    c.width, c.height, c.pitch, c.format, c.step = int(width), int(height), int(pitch), int(format), int(step)
    c.fx, c.fy, c.cx, c.cy = float(fx), float(fy), float(cx), float(cy)
    c.depth_scale, c.z_min, c.z_max = float(depth_scale), float(z_min), float(z_max)
    m = np.eye(4, dtype=np.float32)[:3] if pose is None else np.asarray(pose, np.float32)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"depth_camera: pose must be a 3 x 4 or 4 x 4 matrix, got {m.shape}")
    c.pose[:] = [float(v) for v in m[:3].reshape(-1)]
    return c


_DEPTH_NUMPY = {L.DEPTH_U16: (np.uint16,), L.DEPTH_F32: (np.float32,)}


def _scene_outs():
    """the counts a cloud / depth scene call writes, zeroed, and the address of each: n_spheres, n_occupied, n_matched, n_objects,
    n_objects_matched (-1 until written) and the five counts of the memory routes"""
    o = np.zeros(10, np.int32)
    o[4] = -1
    return o, [o.ctypes.data + 4 * i for i in range(6)]


def _depth_image(im, cam, device=None):
    """(object to keep alive, address of element (0, 0), pitch in elements or None: the camera's) of one depth image"""
    if hasattr(im, "data_ptr") and not im.is_cuda:
        im = im.detach().numpy()
    shape = (int(cam.height), int(cam.width))
    if hasattr(im, "data_ptr"):      # a torch tensor on a device: read in place
        import torch
        if im.device.index != device:
            raise ValueError(f"depth image: a tensor must live on the context's device {device}, got {im.device}")
        u16 = tuple(t for t in (getattr(torch, "uint16", None), torch.int16) if t is not None)      # int16: the same bits, reinterpreted
        want = u16 if cam.format == L.DEPTH_U16 else (torch.float32,)
        if im.dtype not in want or tuple(im.shape) != shape:
            raise ValueError(f"depth image: need a tensor {shape} of {want}, got {tuple(im.shape)} of {im.dtype}")
        if shape[1] > 1 and im.stride(1) != 1:
            raise ValueError("depth image: the last dimension must have stride 1")
        return im, im.data_ptr(), (int(im.stride(0)) if shape[0] > 1 else shape[1])
    im = np.asarray(im)
    if im.dtype not in _DEPTH_NUMPY.get(int(cam.format), ()):
        raise ValueError(f"depth image: format {cam.format} needs dtype {_DEPTH_NUMPY.get(int(cam.format))}, got {im.dtype}")
    if im.shape == shape and (shape[1] == 1 or im.strides[1] == im.itemsize) and (shape[0] == 1 or (im.strides[0] > 0 and im.strides[0] % im.itemsize == 0)):
        return im, im.ctypes.data, (im.strides[0] // im.itemsize if shape[0] > 1 else shape[1])
    flat = np.ascontiguousarray(im).reshape(-1)      # a flat buffer laid out by the camera's own pitch
    pitch = int(cam.pitch) if cam.pitch else shape[1]
    if flat.size < (shape[0] - 1) * pitch + shape[1]:
        raise ValueError(f"depth image: {flat.size} elements, the camera needs {(shape[0] - 1) * pitch + shape[1]}")
    return flat, flat.ctypes.data, None


def _depth_table(who, images, cams, device=None):
    """(camera table, image addresses, n_cams, images_on_device, objects to keep alive) of a depth call; ``device`` None: host images
    only.  A single image and camera may be passed bare; a strided image puts its row stride into the table's pitch."""
    if isinstance(cams, L.OmdsDepthCamera):
        images, cams = [images], [cams]
    images, cams = list(images), list(cams)
    if len(images) != len(cams):
        raise ValueError(f"{who}: {len(images)} images but {len(cams)} cameras")
    n = len(cams)
    table = (L.OmdsDepthCamera * max(n, 1))()
    addrs = (C.c_void_p * max(n, 1))()
    on_dev = [hasattr(im, "data_ptr") and im.is_cuda for im in images]
    if n and any(on_dev) != all(on_dev):
        raise ValueError(f"{who}: the images must all be on the host or all on the engine's device")
    if device is None and any(on_dev):
        raise ValueError(f"{who}: host images only")
    keep = []
    for i, (im, cam) in enumerate(zip(images, cams)):
        C.memmove(C.byref(table[i]), C.byref(cam), C.sizeof(L.OmdsDepthCamera))
        if im is None:
            continue                      # a null image: the library refuses the call
        im, addr, pitch = _depth_image(im, cam, device)
        keep.append(im)
        addrs[i] = addr
        if pitch is not None:
            table[i].pitch = pitch
    if n and all(on_dev):
        import torch
        torch.cuda.current_stream(device).synchronize()      # the library reads the images on its own stream
    return table, addrs, n, (1 if n and all(on_dev) else 0), keep


def scene_memory_spec(max_age, clear_margin=0.0, footprint=0):
    """An ``OmdsSceneMemorySpec``: a cell unseen for more than ``max_age`` calls is dropped (< 1: never); a camera clears an unseen cell
    when every pixel within ``footprint`` (0 .. 3) visited pixels of the cell centre's projection returns from more than
    ``clear_margin`` metres behind it (<= 0: the grid's sphere radius)."""
    m = L.OmdsSceneMemorySpec()
    m.max_age, m.clear_margin, m.footprint = int(max_age), float(clear_margin), int(footprint)
    return m


def depth_filter_spec(radius=1, min_support=4, edge_abs=0.01, edge_rel=0.01):
    """An ``OmdsDepthFilterSpec``: a depth pixel at depth z stays when at least ``min_support`` of the other pixels of its window of
    (2 ``radius`` + 1)^2 visited pixels (``radius`` 1 .. 3) return a depth within ``edge_abs`` + ``edge_rel`` z metres of z."""
    f = L.OmdsDepthFilterSpec()
    f.radius, f.min_support, f.edge_abs, f.edge_rel = int(radius), int(min_support), float(edge_abs), float(edge_rel)
    return f


def depth_lens(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, k4=0.0, k5=0.0, k6=0.0, iters=0, max_residual=0.0):
    """An ``OmdsDepthLens``: OpenCV's rational Brown-Conrady model (plumb-bob: ``k4`` = ``k5`` = ``k6`` = 0).  ``k1`` may be a sequence of
    4, 5 or 8 coefficients in OpenCV's order (k1 k2 p1 p2 [k3 [k4 k5 k6]]).  ``iters``: rounds of the fixed-point inverse (< 1: 20; at
    most 64); ``max_residual``: a pixel whose ray's forward image misses it by more pixels than this gets no ray (<= 0: 0.01)."""
    if np.ndim(k1) > 0:
        seq = [float(v) for v in np.asarray(k1, np.float64).reshape(-1)]
        if len(seq) not in (4, 5, 8):
            raise ValueError(f"depth_lens: a coefficient sequence must hold 4, 5 or 8 values in OpenCV's order, got {len(seq)}")
        k = seq + [0.0] * (8 - len(seq))
    else:
        k = [k1, k2, p1, p2, k3, k4, k5, k6]
    l = L.OmdsDepthLens()
    l.model, l.iters, l.max_residual = 1, int(iters), float(max_residual)
    l.k[:] = [float(v) for v in k]
    return l


def _lens_of(lens):
    """None, an ``OmdsDepthLens``, a dict of ``depth_lens``'s arguments or a coefficient sequence -> None or the lens"""
    if lens is None or isinstance(lens, L.OmdsDepthLens):
        return lens
    return depth_lens(**lens) if isinstance(lens, dict) else depth_lens(lens)


def _lens_table(lenses, n_cams=None, who="set_depth_lenses"):
    """(array of ``OmdsDepthLens`` or None, its length) of a list of lenses with None entries (model 0); None or empty: (None, 0).
    ``n_cams``: the list must have one entry per camera"""
    if lenses is None:
        return None, 0
    lenses = [_lens_of(l) for l in lenses]
    if n_cams is not None and len(lenses) != n_cams:
        raise ValueError(f"{who}: {len(lenses)} lenses but {n_cams} cameras")
    if not lenses:
        return None, 0
    table = (L.OmdsDepthLens * len(lenses))()
    for i, l in enumerate(lenses):
        if l is not None:
            C.memmove(C.byref(table[i]), C.byref(l), C.sizeof(L.OmdsDepthLens))
    return table, len(lenses)


def depth_lens_rays(cam, lens):
    """The ray table of a camera on the host (omds_depth_lens_rays, no GPU): (ab [visited, 2], r2_max, n_invalid) -- the normalised ray
    of every visited pixel in row-major order, (NaN, NaN) where the inverse did not arrive within ``lens.max_residual`` pixels."""
    lib = L.load()
    lens = _lens_of(lens)
    step = max(int(cam.step), 1)
    visited = max(-(-int(cam.height) // step), 0) * max(-(-int(cam.width) // step), 0)
    ab, r2, bad = np.zeros((max(visited, 1), 2), np.float32), C.c_float(0.0), C.c_int64(0)
    rc = lib.omds_depth_lens_rays(C.byref(cam), None if lens is None else C.byref(lens), L.fptr(ab), C.addressof(r2), C.byref(bad))
    if rc != 0:
        raise L.OmdsError(f"omds_depth_lens_rays failed ({rc}): {lib.omds_last_error(None).decode()}")
    return ab[:visited], float(np.float32(r2.value)), int(bad.value)


def velocity_filter_spec(alpha=0.3, alpha_object=0.0, max_jump=0.0):
    """An ``OmdsVelocityFilterSpec``: a new sphere velocity enters the smoothed one with weight max(``alpha``, 1 / frames so far) (a
    running mean first, then an exponential one; ``alpha`` in (0, 1], 1: no smoothing); ``alpha_object`` (<= 0: ``alpha``) is the
    weight for the spheres of a matched object; a new velocity more than ``max_jump`` m/s (<= 0: off) from the smoothed one restarts."""
    f = L.OmdsVelocityFilterSpec()
    f.alpha, f.alpha_object, f.max_jump = float(alpha), float(alpha_object), float(max_jump)
    return f


def _vfilter_of(spec):
    """None, an ``OmdsVelocityFilterSpec`` or a dict of ``velocity_filter_spec``'s arguments -> None or the spec"""
    return velocity_filter_spec(**spec) if isinstance(spec, dict) else spec


def velocity_filter_step(spec, track, filt, state_in, cell, raw, live=None, group=None):
    """The definition of the velocity filter on the host (omds_velocity_filter_step, no GPU): the stored state ``state_in`` [cells, 4]
    (int32; None: empty), the cells ``cell`` [n] of a final list (ascending), its velocities ``raw`` [n, 3], matched flags ``live``
    [n] (None: all) and groups ``group`` [n] (the label of a sphere that moves with a matched object, else -1; None: none) ->
    (vel [n, 3], state_out [cells, 4], (live spheres with history, restarts, groups with history)).  ``spec``: the grid's
    ``OmdsCloudSpec``; ``track``: the ``OmdsCloudTrackSpec`` (its reach and still); ``filt``: an ``OmdsVelocityFilterSpec`` or a dict."""
    lib = L.load()
    filt = _vfilter_of(filt)
    cells = max(int(spec.dims[0]), 0) * max(int(spec.dims[1]), 0) * max(int(spec.dims[2]), 0)
    if cells > 1 << 22:
        cells = 0                         # more than the library takes: it refuses the call
    src = None
    if state_in is not None:
        src = np.ascontiguousarray(state_in, np.int32).reshape(-1, 4)
        if src.shape[0] != cells:
            raise ValueError(f"velocity_filter_step: state_in must hold {cells} records, got {src.shape[0]}")
    cell = np.ascontiguousarray(cell, np.int32).reshape(-1)
    n = cell.size
    raw = L.f32(raw).reshape(n, 3)
    live = None if live is None else np.ascontiguousarray(live, np.int32).reshape(n)
    group = None if group is None else np.ascontiguousarray(group, np.int32).reshape(n)
    vel, out, stats = np.zeros((max(n, 1), 3), np.float32), np.zeros((max(cells, 1), 4), np.int32), np.zeros(3, np.int32)
    rc = lib.omds_velocity_filter_step(C.byref(spec), C.byref(track), None if filt is None else C.byref(filt), L.iptr(src), L.iptr(cell),
                                       L.fptr(raw), L.iptr(live), L.iptr(group), n, L.fptr(vel), L.iptr(out), L.iptr(stats))
    if rc != 0:
        raise L.OmdsError(f"omds_velocity_filter_step failed ({rc}): {lib.omds_last_error(None).decode()}")
    return vel[:n], out[:cells], tuple(int(v) for v in stats)


def _filter_of(filter):
    """None, an ``OmdsDepthFilterSpec`` or a dict of ``depth_filter_spec``'s arguments -> None or the spec"""
    return depth_filter_spec(**filter) if isinstance(filter, dict) else filter


def depth_scene_memory(images, cams, spec, mem, mem_in=None, filter=None, lenses=None):
    """The definition of the scene memory on the host (omds_depth_scene_memory[_filtered], no GPU, no self-filter): the depth images of
    one call and the stored words ``mem_in`` [cells] (uint32; None: all empty) -> (words [cells] uint32, (seen, remembered, cleared,
    expired)).  ``filter`` (an ``OmdsDepthFilterSpec`` or a dict of ``depth_filter_spec``'s arguments): the counts are those of the
    filtered points.  ``lenses`` (one per camera, entries may be None; omds_depth_scene_memory_lens): the counts are those of the points
    on the lenses' rays, and the verdicts of a camera with a lens go through its forward model."""
    lib = L.load()
    table, addrs, n, _, keep = _depth_table("depth_scene_memory", images, cams)
    ltable, _ = _lens_table(lenses, n, "depth_scene_memory")
    cells = max(int(spec.dims[0]), 0) * max(int(spec.dims[1]), 0) * max(int(spec.dims[2]), 0)
    if cells > 1 << 22:
        cells = 0                         # more than the library takes: it refuses the call
    src = None
    if mem_in is not None:
        src = np.ascontiguousarray(mem_in, np.uint32).reshape(-1)
        if src.size != cells:
            raise ValueError(f"depth_scene_memory: mem_in must hold {cells} words, got {src.size}")
    out, counts = np.zeros(max(cells, 1), np.uint32), np.zeros(4, np.int32)
    filt = _filter_of(filter)
    if ltable is not None:
        rc = lib.omds_depth_scene_memory_lens(C.byref(spec), C.byref(mem), None if filt is None else C.byref(filt), ltable, table, addrs, n,
                                              None if src is None else src.ctypes.data, out.ctypes.data, L.iptr(counts))
    elif filt is None:
        rc = lib.omds_depth_scene_memory(C.byref(spec), C.byref(mem), table, addrs, n, None if src is None else src.ctypes.data, out.ctypes.data,
                                         L.iptr(counts))
    else:
        rc = lib.omds_depth_scene_memory_filtered(C.byref(spec), C.byref(mem), C.byref(filt), table, addrs, n,
                                                  None if src is None else src.ctypes.data, out.ctypes.data, L.iptr(counts))
    if rc != 0:
        raise L.OmdsError(f"omds_depth_scene_memory failed ({rc}): {lib.omds_last_error(None).decode()}")
    return out[:cells], tuple(int(v) for v in counts)


def depth_scene_memory_flow(images, cams, spec, mem, track, objects=None, prev=None, mem_in=None, keep_prev=None, keep_now=None, filter=None,
                            cap=None, lenses=None):
    """The definition of ``Engine.set_obstacles_from_depth_memory_tracked`` on the host (omds_depth_scene_memory_flow, no GPU): the depth
    images of one call, the previous frame ``prev`` = (images, cams) standing for the stored record frame and component table (None: no
    previous frame) and the stored words ``mem_in`` (None: all empty) -> dict(words [cells] uint32, counts (seen, remembered, cleared,
    expired, self-forgotten), spheres [n, 4], vel [n, 3], age [n], label [n], object [n], n_matched, n_objects, n_objects_matched).
    ``keep_prev`` one flag per occupied cell of the previous frame, ``keep_now`` one per candidate cell (the cells with a word that is
    not 0, in cell order) stand for the self-filter; None: keep all.  More candidates than ``spec.max_spheres`` or ``cap`` raises; the
    error carries ``counts`` and ``n_occupied``.  ``lenses`` (one per camera, entries may be None; omds_depth_scene_memory_flow_lens): the
    lenses of the cameras, of both frames."""
    lib = L.load()
    table, addrs, n, _, keep = _depth_table("depth_scene_memory_flow", images, cams)
    ltable, _ = _lens_table(lenses, n, "depth_scene_memory_flow")
    if prev is None:
        ptable, paddrs, pn, pkeep = None, None, 0, None
    else:
        ptable, paddrs, pn, _, pkeep = _depth_table("depth_scene_memory_flow", prev[0], prev[1])
        if ltable is not None and pn != n:
            raise ValueError(f"depth_scene_memory_flow: lenses need the same cameras in both frames, got {pn} and {n}")
    cells = max(int(spec.dims[0]), 0) * max(int(spec.dims[1]), 0) * max(int(spec.dims[2]), 0)
    if cells > 1 << 22:
        cells = 0                         # more than the library takes: it refuses the call
    src = None
    if mem_in is not None:
        src = np.ascontiguousarray(mem_in, np.uint32).reshape(-1)
        if src.size != cells:
            raise ValueError(f"depth_scene_memory_flow: mem_in must hold {cells} words, got {src.size}")
    kp = None if keep_prev is None else np.ascontiguousarray(np.asarray(keep_prev) != 0, np.uint8)
    kn = None if keep_now is None else np.ascontiguousarray(np.asarray(keep_now) != 0, np.uint8)
    cap = int(cap) if cap is not None else (spec.max_spheres if spec.max_spheres >= 1 else 4096)
    words, counts = np.zeros(max(cells, 1), np.uint32), np.zeros(5, np.int32)
    out, vel = np.zeros((max(cap, 1), 4), np.float32), np.zeros((max(cap, 1), 3), np.float32)
    age, label, flag = (np.zeros(max(cap, 1), np.int32) for _ in range(3))
    cnt, matched, n_obj, n_acc = (np.zeros(1, np.int32) for _ in range(4))
    filt = _filter_of(filter)
    head = (C.byref(spec), C.byref(mem), C.byref(track), None if objects is None else C.byref(objects), None if filt is None else C.byref(filt))
    frames = ((ptable, paddrs, pn, None if kp is None or not kp.size else kp.ctypes.data),
              (table, addrs, n, None if kn is None or not kn.size else kn.ctypes.data))
    tail = (None if src is None else src.ctypes.data, words.ctypes.data, L.iptr(counts), L.fptr(out), L.fptr(vel), L.iptr(age), L.iptr(label),
            L.iptr(flag), cap, L.iptr(cnt), L.iptr(matched), L.iptr(n_obj), L.iptr(n_acc))
    if ltable is None:
        rc = lib.omds_depth_scene_memory_flow(*head, *frames[0], *frames[1], *tail)
    else:
        rc = lib.omds_depth_scene_memory_flow_lens(*head, ltable if prev is not None else None, *frames[0], ltable, *frames[1], *tail)
    if rc != 0:
        e = L.OmdsError(f"omds_depth_scene_memory_flow failed ({rc}): {lib.omds_last_error(None).decode()}")
        e.counts = tuple(int(v) for v in counts)
        e.n_occupied = int(cnt[0])
        raise e
    k = int(cnt[0])
    return dict(words=words[:cells], counts=tuple(int(v) for v in counts), spheres=out[:k].copy(), vel=vel[:k].copy(), age=age[:k].copy(),
                label=label[:k].copy(), object=flag[:k].copy(), n_matched=int(matched[0]), n_objects=int(n_obj[0]),
                n_objects_matched=int(n_acc[0]))


def depth_points(image, cam, filter=None, lens=None):
    """The definition on the host (omds_depth_points, no GPU): one depth image (numpy ``uint16`` / ``float32``) -> (xyz [visited, 3],
    n_valid): the visited pixels in row-major order as points in the frame of the voxel grid, a dropped pixel as three NaNs (which
    the cloud calls drop), and how many were kept.  ``filter`` (an ``OmdsDepthFilterSpec`` or a dict of ``depth_filter_spec``'s
    arguments; omds_depth_points_filtered): a pixel the depth filter rejects is three NaNs too -> (xyz, n_valid, n_rejected).
    ``lens`` (an ``OmdsDepthLens``, a dict of ``depth_lens``'s arguments or a coefficient sequence; omds_depth_points_lens): the points lie
    on the rays of the lens, and a kept pixel without a ray is three NaNs, counted neither as valid nor as rejected."""
    lib = L.load()
    c = L.OmdsDepthCamera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(L.OmdsDepthCamera))
    keep, addr, pitch = _depth_image(image, c)
    if pitch is not None:
        c.pitch = pitch
    step = max(int(c.step), 1)
    visited = max(-(-int(c.height) // step), 0) * max(-(-int(c.width) // step), 0)
    out, n_valid = np.zeros((max(visited, 1), 3), np.float32), C.c_int64(0)
    filt = _filter_of(filter)
    lens = _lens_of(lens)
    if lens is not None:
        n_rejected = C.c_int64(0)
        rc = lib.omds_depth_points_lens(C.byref(c), C.byref(lens), None if filt is None else C.byref(filt), addr, L.fptr(out), visited,
                                        C.byref(n_valid), C.byref(n_rejected))
        if rc != 0:
            raise L.OmdsError(f"omds_depth_points_lens failed ({rc}): {lib.omds_last_error(None).decode()}")
        return (out[:visited], int(n_valid.value)) + (() if filt is None else (int(n_rejected.value),))
    if filt is not None:
        n_rejected = C.c_int64(0)
        rc = lib.omds_depth_points_filtered(C.byref(c), C.byref(filt), addr, L.fptr(out), visited, C.byref(n_valid), C.byref(n_rejected))
        if rc != 0:
            raise L.OmdsError(f"omds_depth_points_filtered failed ({rc}): {lib.omds_last_error(None).decode()}")
        return out[:visited], int(n_valid.value), int(n_rejected.value)
    rc = lib.omds_depth_points(C.byref(c), addr, L.fptr(out), visited, C.byref(n_valid))
    if rc != 0:
        raise L.OmdsError(f"omds_depth_points failed ({rc}): {lib.omds_last_error(None).decode()}")
    return out[:visited], int(n_valid.value)


def point_cloud_spheres(points, spec, cap=None):
    """The definition on the host (omds_point_cloud_spheres, no GPU): points [P, 3] -> spheres [count, 4] of the occupied cells in
    ascending cell order.  More of them than ``spec.max_spheres`` or ``cap`` raises; the error carries ``n_occupied``."""
    lib = L.load()
    p = L.f32(points).reshape(-1, 3)
    cap = int(cap) if cap is not None else (spec.max_spheres if spec.max_spheres >= 1 else 4096)
    out, cnt = np.zeros((max(cap, 1), 4), np.float32), np.zeros(1, np.int32)
    rc = lib.omds_point_cloud_spheres(C.byref(spec), L.fptr(p) if p.shape[0] else None, p.shape[0], L.fptr(out), cap, L.iptr(cnt))
    if rc != 0:
        e = L.OmdsError(f"omds_point_cloud_spheres failed ({rc}): {lib.omds_last_error(None).decode()}")
        e.n_occupied = int(cnt[0])
        raise e
    return out[:int(cnt[0])].copy()


def point_cloud_flow(prev, now, spec, track, cap=None):
    """The definition of the tracked cloud call on the host (omds_point_cloud_flow, no GPU): clouds ``prev`` and ``now`` [P, 3] ->
    (spheres [count, 4] of ``point_cloud_spheres(now, spec)``, vel [count, 3], matched).  Raises like ``point_cloud_spheres``."""
    lib = L.load()
    a, b = L.f32(prev).reshape(-1, 3), L.f32(now).reshape(-1, 3)
    cap = int(cap) if cap is not None else (spec.max_spheres if spec.max_spheres >= 1 else 4096)
    out, vel = np.zeros((max(cap, 1), 4), np.float32), np.zeros((max(cap, 1), 3), np.float32)
    cnt, matched = np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = lib.omds_point_cloud_flow(C.byref(spec), C.byref(track), L.fptr(a) if a.shape[0] else None, a.shape[0],
                                   L.fptr(b) if b.shape[0] else None, b.shape[0], L.fptr(out), L.fptr(vel), cap, L.iptr(cnt), L.iptr(matched))
    if rc != 0:
        e = L.OmdsError(f"omds_point_cloud_flow failed ({rc}): {lib.omds_last_error(None).decode()}")
        e.n_occupied = int(cnt[0])
        raise e
    return out[:int(cnt[0])].copy(), vel[:int(cnt[0])].copy(), int(matched[0])


def point_cloud_object_flow(prev, now, spec, track, obj, keep_prev=None, keep_now=None, cap=None):
    """The definition of the objects cloud call on the host (omds_point_cloud_object_flow, no GPU): clouds ``prev`` and ``now`` [P, 3],
    ``keep_prev`` / ``keep_now`` one flag per occupied cell of that frame in cell order (None: keep all; they stand for the
    self-filter) -> (spheres [kept, 4], vel [kept, 3], label [kept], object [kept], matched, n_objects, n_objects_matched).  Raises
    like ``point_cloud_spheres``."""
    lib = L.load()
    a, b = L.f32(prev).reshape(-1, 3), L.f32(now).reshape(-1, 3)
    kp = None if keep_prev is None else np.ascontiguousarray(np.asarray(keep_prev) != 0, np.uint8)
    kn = None if keep_now is None else np.ascontiguousarray(np.asarray(keep_now) != 0, np.uint8)
    cap = int(cap) if cap is not None else (spec.max_spheres if spec.max_spheres >= 1 else 4096)
    out, vel = np.zeros((max(cap, 1), 4), np.float32), np.zeros((max(cap, 1), 3), np.float32)
    label, flag = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
    cnt, matched, n_obj, n_acc = (np.zeros(1, np.int32) for _ in range(4))
    for k, pts, what in ((kp, a, "keep_prev"), (kn, b, "keep_now")):
        if k is not None and k.size != len(point_cloud_spheres(pts, spec, cap=65536)):
            raise ValueError(f"point_cloud_object_flow: {what} needs one entry per occupied cell")
    rc = lib.omds_point_cloud_object_flow(C.byref(spec), C.byref(track), C.byref(obj), L.fptr(a) if a.shape[0] else None, a.shape[0],
                                          None if kp is None or not kp.size else kp.ctypes.data, L.fptr(b) if b.shape[0] else None, b.shape[0],
                                          None if kn is None or not kn.size else kn.ctypes.data, L.fptr(out), L.fptr(vel), L.iptr(label),
                                          L.iptr(flag), cap, L.iptr(cnt), L.iptr(matched), L.iptr(n_obj), L.iptr(n_acc))
    if rc != 0:
        e = L.OmdsError(f"omds_point_cloud_object_flow failed ({rc}): {lib.omds_last_error(None).decode()}")
        e.n_occupied = int(cnt[0])
        raise e
    n = int(cnt[0]) if kn is None else int(kn.sum())
    return out[:n].copy(), vel[:n].copy(), label[:n].copy(), flag[:n].copy(), int(matched[0]), int(n_obj[0]), int(n_acc[0])


def moving_frame_velocity(gradx, drow, vel, n_dof, softmax_k=-10.0, max_speed=1.0):
    """The moving frame's definition on the host (omds_moving_frame_velocity, no GPU): gradx [k, d] full input gradients of the k
    selected rows, drow [k] their distances, vel [k, 3] the velocity of each row's sphere -> (rate, qo [n_dof])."""
    lib = L.load()
    g = L.f32(gradx)
    g = g.reshape(-1, g.shape[-1])
    k, d = g.shape
    dr, v = L.f32(drow).reshape(-1), L.f32(vel).reshape(-1, 3)
    if dr.shape[0] != k or v.shape[0] != k:
        raise ValueError(f"moving_frame_velocity: {k} gradient rows but {dr.shape[0]} distances and {v.shape[0]} velocities")
    rate, qo = np.zeros(1, np.float32), np.zeros(int(n_dof), np.float32)
    rc = lib.omds_moving_frame_velocity(int(n_dof), d, k, L.fptr(g), L.fptr(dr), L.fptr(v), float(softmax_k), float(max_speed),
                                        L.fptr(rate), L.fptr(qo))
    if rc != 0:
        raise L.OmdsError(f"omds_moving_frame_velocity failed ({rc}): {lib.omds_last_error(None).decode()}")
    return float(rate[0]), qo


def red_layout(K, n):
    """Offsets into the packed reduction buffer (include/omds.h, omds_local_sums)."""
    o_mu = 1
    o_sg = o_mu + K * n
    o_al = o_sg + K
    o_mx = o_al + K * n
    o_ph = o_mx + K
    o_qd = o_ph + K
    o_best = o_qd + n
    return dict(sumw=0, mu=o_mu, sigma=o_sg, alpha=o_al, maxact=o_mx, phi0=o_ph, qdot=o_qd, best=o_best,
                n_sum=o_best, size=o_best + 1 + n)


def apply_update(K, n, H, red, n_total, rate, ker_thr, mu_c, sigma_c, alpha_c, variant=0):
    """Host arithmetic of the policy update on the (globally) reduced buffer -- omds_apply_update."""
    lib = L.load()
    red = L.f32(red)
    mu = np.array(np.asarray(mu_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, n)
    sg = np.array(np.asarray(sigma_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K)
    al = np.array(np.asarray(alpha_c, dtype=np.float32)[:K], dtype=np.float32, order="C", copy=True).reshape(K, n)
    mask = np.zeros(K, np.int32)
    rc = lib.omds_apply_update(int(K), int(n), int(H), L.fptr(red), float(n_total), float(rate), float(ker_thr),
                               int(variant), L.fptr(mu), L.fptr(sg), L.fptr(al), L.iptr(mask))
    if rc != 0:
        raise L.OmdsError(f"omds_apply_update failed ({rc})")
    return mu, sg, al, mask.astype(bool)
