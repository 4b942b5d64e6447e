"""MPPI controller -- mirrors ``ds_mppi/functions/MPPI.py`` (class MPPI, lines 21-350).

Same constructor, methods and mutable attributes as the reference; every array computation of
the hot path (distance network forward/backward over rollouts x obstacles, modulation, policy,
Euler step, cost, cost-weighted reduction) runs in the HIP kernels behind ``Engine``.  Tensors
handed back to the caller are torch CPU tensors in the reference's layouts."""
from __future__ import annotations

import numpy as np
import torch

from .cost import Cost
from .engine import Engine
from .lazy import LazyRollout
from .policy import TensorPolicyMPPI


def _np(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().astype(np.float32)
    return np.asarray(x, dtype=np.float32)


def _qr_complete(g):
    """E = qr([g, e_2 .. e_n]).Q with column 0 := g, batched over the leading axes of g [..., n]."""
    n = g.shape[-1]
    A = np.broadcast_to(np.eye(n, dtype=np.float32), g.shape[:-1] + (n, n)).copy()
    A[..., 0] = g
    Q, _ = np.linalg.qr(A)
    Q = Q.astype(np.float32)
    Q[..., 0] = g
    return torch.from_numpy(Q)


class _LazyBasis:
    """Indexable stand-in for the reference's ``norm_basis`` tensor; ``[i, h]`` builds one basis,
    any other index (or ``.tensor()``) materialises the selection."""

    def __init__(self, normals):
        self._g = normals                                   # [N, H, n]: a LazyRollout (row fetches) or an array
        self.shape = tuple(normals.shape) + (normals.shape[-1],)

    def __getitem__(self, idx):
        if not isinstance(idx, tuple):
            idx = (idx,)
        lead = tuple(int(i) if isinstance(i, torch.Tensor) and i.ndim == 0 else i for i in idx[:2])
        out = _qr_complete(np.asarray(self._g[lead], dtype=np.float32))
        return out[(Ellipsis,) + tuple(idx[2:])] if len(idx) > 2 else out

    def tensor(self):
        return _qr_complete(np.asarray(self._g, dtype=np.float32))

    def __torch_function__(self, func, types, args=(), kwargs=None):
        args = tuple(a.tensor() if isinstance(a, _LazyBasis) else a for a in args)
        return func(*args, **(kwargs or {}))

    def transpose(self, *a):
        return self.tensor().transpose(*a)

    def __matmul__(self, other):
        return self.tensor() @ (other.tensor() if isinstance(other, _LazyBasis) else other)


class MPPI:
    def __init__(self, q0, qf, dh_params, obs, dt, dt_H, N_traj, DS_ARRAY, dh_a, nn_model, n_closest_obs,
                 device=0, warmup=False, seed=1234, rollout_offset=0, max_obs=None, lazy_rollouts=False):
        self.tensor_args = {'device': 'cpu', 'dtype': torch.float32}
        self.q0 = torch.as_tensor(_np(q0))
        self.n_dof = self.q0.shape[0]
        self.DS_idx = 0
        self.DS_ARRAY = DS_ARRAY
        self.DS = DS_ARRAY[self.DS_idx]
        self.qf = self.DS.q_goal.squeeze()
        self.dh_params = torch.as_tensor(_np(dh_params))
        self.obs = torch.as_tensor(_np(obs)).reshape(-1, 4)
        self.n_obs = self.obs.shape[0]
        self.dt = dt
        self.dt_H = dt_H
        self.N_traj = N_traj
        self.dh_a = dh_a
        self.nn_model = nn_model
        self.n_closest_obs = n_closest_obs
        self.q_cur = self.q0
        self.policy_upd_rate = 0.1                      # MPPI.py:58 (the rate that is actually used, :344)
        self.dst_thr = 0.5
        self.ker_thr = 1e-3
        self.ignored_links = [0, 1, 2] if self.n_dof >= 7 else []
        self._device = device
        self._max_obs = int(max_obs or max(64, 2 * self.n_obs))
        self._engine = Engine(self.n_dof, N_traj, dt_H, n_closest_obs, self._max_obs, device=device)
        self._engine.set_mlp(nn_model.model.W, nn_model.model.b, nn_model.model.act, skip_after=getattr(nn_model.model, 'skip_after', ()))
        self._engine.set_obstacles(self.obs.numpy())
        self.Policy = TensorPolicyMPPI(N_traj, self.n_dof, self.tensor_args, engine=self._engine, seed=seed,
                                       rollout_offset=rollout_offset)
        self.Policy._owner = self
        self.Cost = Cost(self.qf, self.dh_params, owner=self)
        self.obs_focus = None         # focus_obstacles: the master index of every sphere of self.obs, else None
        self.obs_age = None           # update_obstacles_from_depth(memory=): calls since every sphere's cell was last counted, else None
        self.depth_filter_stats = None   # update_obstacles_from_depth(filter=): (pixels kept, pixels rejected) of the last such call
        self.vel_filter_stats = None  # update_obstacles_from_*(smooth=): (spheres with history, restarts, groups with history), else None
        self.cur_cost = None
        self._cache = {}
        self._generation = 0          # propagate() calls so far (LazyRollout tensors belong to one of them)
        # False (default): propagate() returns and binds torch CPU tensors like the reference (one fetch of all rollout tensors per
        # call, 0.4 ms at 1024 x 32).  True: LazyRollout objects that stay on the GPU until read (lazy.py) -- for loops that, like
        # the reference's planner, read a handful of rows per iteration and never keep a tensor across propagate() calls
        self.lazy_rollouts = bool(lazy_rollouts)
        self._pushed = None           # what the device context last received (_push skips an unchanged set)
        self._pushed_version = -1     # Engine.config_version after that push
        self._qdot_cache = {}         # get_qdot values of the current cost (filled by shift_policy_means)
        self.all_traj = torch.zeros(N_traj, dt_H, self.n_dof)
        self.closest_dist_all = 100 + torch.zeros(N_traj, dt_H)
        self.qdot = torch.zeros(N_traj, self.n_dof)
        if warmup:                                       # MPPI.py:69-73 (optional here)
            for _ in range(5):
                self.Policy.sample_policy()
                self.propagate()

    # ---- DS switching (MPPI.py:75-84) -------------------------------------------------------------
    def reset_DS(self, DS):
        self.DS = DS
        self.qf = DS.q_goal.squeeze()
        self.Cost = Cost(self.qf, self.dh_params, owner=self)

    def switch_DS_idx(self, idx):
        self.DS_idx = idx
        self.DS = self.DS_ARRAY[idx]
        self.qf = self.DS.q_goal.squeeze()
        self.Cost = Cost(self.qf, self.dh_params, owner=self)

    def update_obstacles(self, obs, velocities=None, moving_frame=False):
        """MPPI.py:347-350.  ``velocities`` [O, 3] (new here; the reference's obstacle streamers know them and drop them): step i of
        the next propagates sees the spheres moved by (i - 1) dt velocities instead of frozen at ``obs`` (Engine.set_obstacle_motion,
        with the ``dt`` in force at the propagate).  Every call without them is the reference's: a static scene.  ``moving_frame``: the
        modulation also runs relative to those velocities (Engine.set_obstacle_frame); it needs ``velocities`` to act."""
        self.obs = torch.as_tensor(_np(obs)).reshape(-1, 4)
        self.n_obs = self.obs.shape[0]
        vel = None if velocities is None else _np(velocities).reshape(self.n_obs, 3)
        # the reference takes any obstacle count at any time: the context grows its own obstacle buffers (omds_set_obstacles),
        # so the handle -- network, samples, RCCL communicator, screening state -- survives
        self._engine.set_obstacles(self.obs.numpy())
        self.obs_focus = None                        # (and ended an obstacle focus)
        self.obs_age = None
        self._max_obs = self._engine.max_obs
        if vel is not None:                          # (set_obstacles cleared the previous motion)
            self._engine.set_obstacle_motion(vel)
        self._engine.set_obstacle_frame(bool(moving_frame))
        return 0

    def update_obstacles_from_cloud(self, points, voxel, lo, hi, radius=None, self_margin=None, min_points=1, max_spheres=4096,
                                    dt_frame=None, reach=2, still=0.0, moving_frame=False, objects=False, link=1, min_cells=4, **route):
        """The scene from a depth point cloud ``points`` [P, 3] (new here; numpy, or a torch tensor on the engine's device): cropped
        to the box ``lo`` .. ``hi``, down-sampled to one sphere per occupied ``voxel`` cell (``radius`` None: the cell's circumsphere)
        and, when ``self_margin`` is given, without the spheres the distance network places within that margin of the robot at
        ``self.q_cur`` (Engine.set_obstacles_from_cloud).  Like ``update_obstacles`` it leaves a static scene in ``self.obs``.
        Returns (spheres before padding to n_closest, occupied cells).
        ``dt_frame`` (seconds since the previous such call): the tracked route (Engine.set_obstacles_from_cloud_tracked) -- one
        velocity per sphere from the previous frame, the surfaces' normal flow, searched ``reach`` cells each way, speeds below
        ``still`` zeroed, and installed as ``update_obstacles(obs, velocities=)`` would.  ``self.obs_velocities`` then holds them
        ([O, 3], a CPU tensor) or None when the scene stands still (no previous frame, or every velocity 0), ``self.cloud_matched``
        the spheres that found a previous surface (-1: no previous frame), and ``moving_frame`` acts as in ``update_obstacles``.
        ``objects`` (needs ``dt_frame``): the objects route (Engine.set_obstacles_from_cloud_objects) -- the spheres are segmented into
        connected components (cells at most ``link`` apart), a component of at least ``min_cells`` cells that is matched with one of
        the previous such call moves as a rigid body with its centroid, the other spheres keep the tracked velocities.
        ``self.cloud_objects`` then holds the objects of the scene and ``self.cloud_objects_matched`` those that were matched (-1: no
        previous component table); both are None on the other routes.
        ``smooth`` (needs ``dt_frame``; an ``OmdsVelocityFilterSpec``, or a dict of ``engine.velocity_filter_spec``'s arguments, as in
        ``smooth=dict(alpha=0.3)``): sets the engine's velocity filter (Engine.set_velocity_filter), which STAYS set -- its history
        lives in the context between calls, and turning it off empties it: the velocities of this and the following tracked / objects
        calls are blended against the smoothed velocity kept per grid cell, and ``self.vel_filter_stats`` holds (spheres with
        history, restarts, groups with history) of the call.  False turns the filter off; None (the default) leaves whatever filter
        the engine has as it is.  (``smooth`` is the one keyword ``**route`` takes here: the named keywords stay what they were.)"""
        smooth = route.pop("smooth", None)
        if route:
            raise TypeError(f"update_obstacles_from_cloud: unexpected keyword arguments {sorted(route)}")
        self._set_smooth("update_obstacles_from_cloud", smooth, dt_frame)
        return self._update_obstacles_sensed("update_obstacles_from_cloud", lambda e, spec, q, track, obj: (
            e.set_obstacles_from_cloud(points, spec, q) if track is None else
            e.set_obstacles_from_cloud_tracked(points, spec, track, q) if obj is None else
            e.set_obstacles_from_cloud_objects(points, spec, track, obj, q)),
            voxel, lo, hi, radius, self_margin, min_points, max_spheres, dt_frame, reach, still, moving_frame, objects, link, min_cells)

    def _set_smooth(self, who, smooth, dt_frame):
        """the ``smooth`` keyword of the sensed-scene calls: None leaves the engine's velocity filter, False turns it off, a spec sets it"""
        self.vel_filter_stats = None
        if smooth is None:
            return
        if smooth is False:
            self._engine.set_velocity_filter(None)
            return
        if dt_frame is None:
            raise ValueError(f"{who}: smooth= needs dt_frame (only the tracked routes estimate velocities)")
        self._engine.set_velocity_filter(smooth)

    def update_obstacles_from_depth(self, images, cameras, voxel, lo, hi, radius=None, self_margin=None, min_points=1, max_spheres=4096,
                                    dt_frame=None, reach=2, still=0.0, moving_frame=False, objects=False, link=1, min_cells=4, **route):
        """``update_obstacles_from_cloud`` straight from depth images (new here): ``images`` [H, W] one per camera (numpy ``uint16`` /
        ``float32``, or torch tensors on the engine's device, read in place) and ``cameras`` their ``OmdsDepthCamera`` s
        (``engine.depth_camera``: intrinsics, range gate, pose in the frame of ``lo`` .. ``hi``).  The pixels are deprojected inside the
        counting pass on the device (Engine.set_obstacles_from_depth); everything else -- arguments, routes, return value and the
        attributes set -- is ``update_obstacles_from_cloud`` on the points of the images, bit for bit.
        ``memory`` (an ``OmdsSceneMemorySpec``, or a dict of ``engine.scene_memory_spec``'s arguments): the route with a memory of
        occupancy between calls (Engine.set_obstacles_from_depth_memory) -- a cell without points stays in the scene unless a camera
        looked through it, it is older than ``max_age`` calls or the self-filter drops it.  Returns (spheres before padding, (seen,
        remembered, cleared, expired, self-forgotten)); ``self.obs_age`` then holds, per sphere, the calls since its cell was last
        counted (-1: padding), and is None after every other call.  A static scene: not together with ``dt_frame`` or ``objects``.
        ``filter`` (an ``OmdsDepthFilterSpec``, or a dict of ``engine.depth_filter_spec``'s arguments): sets the engine's depth filter
        for this call (Engine.set_depth_filter) -- flying pixels at depth edges and isolated speckle leave inside the counting pass, and
        everything is the cloud call on ``engine.depth_points(image, camera, filter=...)``; ``self.depth_filter_stats`` then holds
        (pixels kept, pixels rejected), and the engine's filter is what it was before the call (off, or what
        ``Engine.set_depth_filter`` had installed).  None (the default) leaves the call, and whatever filter the engine has, as it is.  Works
        together with ``dt_frame``, ``objects`` and ``memory``.
        ``memory_motion=True`` (with ``memory`` and ``dt_frame``, optionally ``objects``): memory and velocities in one call
        (Engine.set_obstacles_from_depth_memory_tracked) -- the scene, the counts returned and ``self.obs_age`` are the memory route's,
        the spheres counted in this frame carry the tracked / objects route's velocities (``self.obs_velocities``,
        ``self.cloud_matched``, ``self.cloud_objects[_matched]`` as there, ``moving_frame`` honoured), remembered spheres and seen
        ones that were occluded at the previous memory call stand still.  Without it, ``memory`` together with ``dt_frame`` /
        ``objects`` is the error it was.
        ``lenses`` (a list, one ``engine.depth_lens`` per camera, entries may be None): sets the engine's lenses for this call
        (Engine.set_depth_lenses) -- the images are unrectified, every pixel is deprojected along the ray of its camera's lens, and
        everything is the cloud call on ``engine.depth_points(image, camera, filter=..., lens=...)``; the engine's lenses are what they
        were before the call.  None (the default) leaves the call, and whatever lenses the engine has, as it is.  Works with every route.
        ``smooth``: as in ``update_obstacles_from_cloud``; the cloud and depth calls share the one filter and its history.
        (``memory``, ``filter``, ``lenses``, ``memory_motion`` and ``smooth`` are the keywords ``**route`` takes, default None / None /
        None / False / None: the named keywords stay those of ``update_obstacles_from_cloud``.)"""
        memory, filt, motion = route.pop("memory", None), route.pop("filter", None), bool(route.pop("memory_motion", False))
        smooth, lenses = route.pop("smooth", None), route.pop("lenses", None)
        if lenses is not None:
            before = self._engine.depth_lenses
            self._engine.set_depth_lenses(lenses)
            try:
                return self.update_obstacles_from_depth(images, cameras, voxel, lo, hi, radius, self_margin, min_points, max_spheres, dt_frame,
                                                        reach, still, moving_frame, objects, link, min_cells, memory=memory, filter=filt,
                                                        memory_motion=motion, smooth=smooth, **route)
            finally:
                self._engine.set_depth_lenses(before)
        if route:
            raise TypeError(f"update_obstacles_from_depth: unexpected keyword arguments {sorted(route)}")
        self._set_smooth("update_obstacles_from_depth", smooth, dt_frame)
        if motion and (memory is None or dt_frame is None):
            raise ValueError("update_obstacles_from_depth: memory_motion=True needs both memory= and dt_frame=")
        if filt is None:
            return self._update_obstacles_from_depth(images, cameras, voxel, lo, hi, radius, self_margin, min_points, max_spheres, dt_frame, reach,
                                                     still, moving_frame, objects, link, min_cells, memory, motion)
        before = self._engine.depth_filter
        self._engine.set_depth_filter(filt)
        try:
            return self._update_obstacles_from_depth(images, cameras, voxel, lo, hi, radius, self_margin, min_points, max_spheres, dt_frame, reach,
                                                     still, moving_frame, objects, link, min_cells, memory, motion)
        finally:
            self.depth_filter_stats = self._engine.depth_filter_stats()
            self._engine.set_depth_filter(before)

    def _update_obstacles_from_depth(self, images, cameras, voxel, lo, hi, radius, self_margin, min_points, max_spheres, dt_frame, reach, still,
                                     moving_frame, objects, link, min_cells, memory, motion=False):
        """``update_obstacles_from_depth`` behind its route keywords"""
        if memory is None:
            return self._update_obstacles_sensed("update_obstacles_from_depth", lambda e, spec, q, track, obj: (
                e.set_obstacles_from_depth(images, cameras, spec, q, track, obj)),
                voxel, lo, hi, radius, self_margin, min_points, max_spheres, dt_frame, reach, still, moving_frame, objects, link, min_cells)
        from .engine import scene_memory_spec
        if not motion and (dt_frame is not None or objects):
            raise ValueError("update_obstacles_from_depth: memory= installs a static scene; not together with dt_frame or objects "
                             "(memory_motion=True asks for the route that does both)")
        mem = scene_memory_spec(**memory) if isinstance(memory, dict) else memory
        counts = []

        def install(e, spec, q, track, obj):      # the counts go round the tracked route's unpacking: (n, [matched, [objects, objects matched]])
            if motion:
                n, c, *rest = e.set_obstacles_from_depth_memory_tracked(images, cameras, spec, mem, track, obj, q)
            else:
                n, c, *rest = e.set_obstacles_from_depth_memory(images, cameras, spec, mem, q)
            counts.append(c)
            return (n, *rest) if obj is not None else (n, *rest[:1])
        (n,) = self._update_obstacles_sensed("update_obstacles_from_depth", install, voxel, lo, hi, radius, self_margin, min_points, max_spheres,
                                             dt_frame, reach, still, moving_frame, objects, link, min_cells)
        self.obs_age = torch.as_tensor(self._engine.get_scene_memory())
        return n, counts[0]

    def _update_obstacles_sensed(self, who, install, voxel, lo, hi, radius, self_margin, min_points, max_spheres, dt_frame, reach, still,
                                 moving_frame, objects, link, min_cells):
        """what ``update_obstacles_from_cloud`` and ``update_obstacles_from_depth`` share: the specs, ``install(engine, spec, q, track,
        obj)`` (the engine call of the route; its counts come back), and the attributes the facade keeps of the sensed scene"""
        from .engine import cloud_object_spec, cloud_spec, cloud_track_spec
        if objects and dt_frame is None:
            raise ValueError(f"{who}: objects=True needs dt_frame (the objects route is a tracked one)")
        lo, hi = _np(lo).reshape(3).astype(np.float32), _np(hi).reshape(3).astype(np.float32)
        dims = np.maximum(np.ceil((hi - lo) / np.float32(voxel) - 1e-4), 1).astype(np.int32)
        spec = cloud_spec(lo, voxel, dims, 0.0 if radius is None else radius, min_points, max_spheres,
                          0.0 if self_margin is None else self_margin)
        q = None if self_margin is None else _np(self.q_cur).reshape(-1)
        if q is not None:
            self._push()                             # the filter takes its minimum over the links not in self.ignored_links
        self.obs_velocities, self.cloud_matched = None, None
        self.cloud_objects, self.cloud_objects_matched = None, None
        self.obs_focus = None                        # a scene setter ends an obstacle focus
        self.obs_age = None                          # ... and only the memory route says how old a sphere is
        if dt_frame is None:
            out = install(self._engine, spec, q, None, None)
        else:
            track = cloud_track_spec(reach, dt_frame, still)
            if objects:
                *out, self.cloud_matched, self.cloud_objects, self.cloud_objects_matched = install(
                    self._engine, spec, q, track, cloud_object_spec(link, min_cells))
            else:
                *out, self.cloud_matched = install(self._engine, spec, q, track, None)
            out = tuple(out)
            vel, have = self._engine.get_obstacle_motion()
            if have:
                self.obs_velocities = torch.as_tensor(vel)
            if self._engine.velocity_filter is not None:
                self.vel_filter_stats = self._engine.velocity_filter_frame()[2]
        self.obs = torch.as_tensor(self._engine.get_obstacles())
        self.n_obs = self.obs.shape[0]
        self._max_obs = self._engine.max_obs
        self._engine.set_obstacle_frame(bool(moving_frame))       # as update_obstacles leaves it
        return out

    def focus_obstacles(self, margin, max_keep=0, q=None, along=None, stride=1):
        """Narrow a large scene to the spheres near the robot, on the device (new here; Engine.focus_obstacles): of the MASTER -- the
        scene the last ``update_obstacles*`` call installed, kept for the next call -- the ``n_closest_obs`` spheres nearest to ``q``
        (None: ``self.q_cur``) and every sphere within ``margin`` metres of the farthest of those stay in force, at most ``max_keep``
        (0: no cap); a moving sphere is given the horizon, (dt_H - 1) dt seconds, to approach.  Meant for every planner iteration,
        before ``propagate``.  ``self.obs``, ``self.n_obs`` and ``self.obs_velocities`` then describe the scene in force and
        ``self.obs_focus`` holds the master index of each of its spheres.  Returns (kept, passed).  Whether the propagate equals the one
        on the full scene is the caller's bet on ``margin`` (omds.h: THE OBSTACLE FOCUS).
        ``along`` focuses along a path of states instead (Engine.focus_obstacles_path): a sphere stays when it is near at SOME state, and
        ``margin`` covers only the deviation from them.  An array or tensor [B, n]: ``q`` and those states, a moving sphere given the
        whole horizon at each.  A sequence of rollout indices: ``q`` and the states ``all_traj[r, ::stride]`` of the last propagate
        (fetched per rollout when ``lazy_rollouts``), a moving sphere given step * dt seconds to reach a state and (stride - 1) dt more."""
        self._push()                                 # the distances take their minimum over the links not in self.ignored_links
        q = _np(self.q_cur if q is None else q).reshape(-1)
        dt = float(self.dt)
        if along is None:
            out = self._engine.focus_obstacles(q, margin, max_keep, (self.dt_H - 1) * dt)
        else:
            a = _np(along)
            if a.ndim == 2:
                path = np.concatenate([q[None], a.astype(np.float32)])
                out = self._engine.focus_obstacles_path(path, margin, max_keep, (self.dt_H - 1) * dt)
            else:
                rows, stride = np.atleast_1d(a).astype(np.int64).reshape(-1), int(stride)
                if stride < 1 or rows.size == 0 or rows.min() < 0 or rows.max() >= self.N_traj:
                    raise ValueError("focus_obstacles: along needs rollout indices in [0, N_traj) and stride >= 1")
                if self.lazy_rollouts:
                    traj = self._engine.get_rollout_rows(rows, want=("all_traj",))["all_traj"]
                else:
                    traj = _np(self.all_traj)[rows]
                steps = np.arange(0, self.dt_H, stride)
                path = np.concatenate([q[None], traj[:, steps].reshape(-1, self.n_dof).astype(np.float32)])
                ahead = np.concatenate([[0.0], np.tile(steps * dt, rows.size)]).astype(np.float32)
                out = self._engine.focus_obstacles_path(path, margin, max_keep, (stride - 1) * dt, ahead)
        self._focus_refresh()
        return out

    def clear_obstacle_focus(self):
        """Put the master scene and its velocities back in force (a no-op without a focus)."""
        self._engine.clear_obstacle_focus()
        self._focus_refresh()

    def _focus_refresh(self):
        self.obs = torch.as_tensor(self._engine.get_obstacles())
        self.n_obs = self.obs.shape[0]
        vel, have = self._engine.get_obstacle_motion()
        self.obs_velocities = torch.as_tensor(vel) if have else None
        idx = self._engine.obstacle_focus()
        self.obs_focus = None if idx is None else torch.as_tensor(idx)
        self.obs_age = None                          # the ages belong to the scene the memory call installed

    def set_screening(self, mode, eps=0.0, over_horizon=False):
        """The screened pass 1 (Engine.set_screening: mode -1 | 0 | 1 | 2, ``eps`` as there); ``over_horizon``: also while
        ``update_obstacles(..., velocities=)`` has set an obstacle horizon (Engine.set_screening_horizon), which otherwise puts the
        propagate on the all-fp32 step."""
        self._engine.set_screening(mode, eps)
        self._engine.set_screening_horizon(bool(over_horizon))

    # ---- parameters -> device ----------------------------------------------------------------------
    def _push(self):
        """The mutable attributes the reference's callers poke (dt, dst_thr, ignored_links, Policy.p, DS, Cost limits) -> the
        device context; skipped while nothing changed since the last call (three ctypes calls per use otherwise)."""
        e = self._engine
        mask = 0
        for l in self.ignored_links:
            mask |= 1 << int(l)
        qf, dh, qmin, qmax = _np(self.qf), _np(self.dh_params), _np(self.Cost.q_min), _np(self.Cost.q_max)
        # the nominal DS by VALUE (an id() can be reused by a new object, and a SEDS DS can be edited in place)
        seds = self.DS.device_params() if hasattr(self.DS, "device_params") else None
        ds_sig = (type(self.DS).__name__, float(getattr(self.DS, "seds_thr", 0.0)), b"".join(a.tobytes() for a in seds) if seds else b"")
        sig = (float(self.dt), float(self.dst_thr), float(self.DS.lin_thr), float(self.Policy.p), mask, ds_sig, qf.tobytes(),
               dh.tobytes(), qmin.tobytes(), qmax.tobytes(), e.params.variant, e.params.cost_terms)
        # config_version: somebody configured the context through the Engine directly since our last push -> ours again
        if sig == self._pushed and e.config_version == self._pushed_version:
            return
        p = e.params
        p.dt, p.dst_thr, p.lin_thr, p.rbf_p, p.ignored_links = sig[0], sig[1], sig[2], sig[3], mask
        e.push_params()
        if seds is not None:                        # SEDS nominal DS (seds.py)
            e.set_ds_seds(qf, *seds, lin_thr=float(self.DS.lin_thr), seds_thr=float(self.DS.seds_thr))
        else:
            e.set_ds(qf)
        e.set_cost(dh, qmin, qmax)
        self._pushed = sig
        self._pushed_version = e.config_version

    # ---- rollouts (MPPI.py:97-224) -------------------------------------------------------------------
    def propagate(self, fetch=None):
        """MPPI.py:97-224.  Returns the reference's 5-tuple (all_traj, closest_dist_all, kernel_val_all[:, :, :K], dot_products,
        kernel_activations) and sets the same attributes.  By default they are torch CPU tensors, as in the reference (fresh ones
        every call, MPPI.py:86-91).  With ``lazy_rollouts = True`` (or ``fetch=False``) they are LazyRollout tensors (lazy.py): they
        stay on the GPU until read, single rollouts are fetched as rows, and the candidate search / cost / update work on the
        device-resident copies either way."""
        if fetch is None:
            fetch = not self.lazy_rollouts
        self._push()
        if self._engine.K != self.Policy.n_kernels:
            # like the reference, propagate() consumes whatever sample tensors exist; with a changed
            # kernel count and no sample_policy() call yet there is nothing valid to consume
            raise RuntimeError("Policy.n_kernels changed since the last sample_policy()/set_samples()")
        self._engine.propagate(_np(self.q_cur))
        self._cache = {}
        self.cur_cost = None
        self._qdot_cache = {}
        self._generation += 1
        N, H, n, K = self.N_traj, self.dt_H, self.n_dof, self.Policy.n_kernels
        if fetch:
            c = self._fetch()
            self.all_traj, self.closest_dist_all, self.kernel_val_all = c["all_traj"], c["closest_dist_all"], c["kernel_val_all"]
            self.dot_products, self.kernel_activations, self.qdot, self.normal_dirs = c["dot_products"], c["kernel_activations"], c["qdot"], c["normal"]
            # torch counts in-place writes: a caller who edits a returned tensor WITH TORCH OPERATIONS gets the host path of
            # check_traj_for_kernels.  (A write through a numpy view of the tensor -- t.numpy()[...] = x, np.asarray(t) -- shares its memory
            # without bumping t._version and is NOT seen: pass an edited copy instead.)
            self._versions = {id(t): t._version for t in c.values()}
        else:
            self._versions = {}
            lz = lambda key, shape: LazyRollout(self, key, shape, self._generation)
            self.all_traj = lz("all_traj", (N, H, n))
            self.closest_dist_all = lz("closest_dist_all", (N, H))
            self.kernel_val_all = lz("kernel_val_all", (N, H, K))
            self.dot_products = lz("dot_products", (N, H))
            self.kernel_activations = lz("kernel_activations", (N, H))
            self.qdot = lz("qdot", (N, n))
            self.normal_dirs = lz("normal", (N, H, n))      # norm_basis[..., 0]
        return (self.all_traj, self.closest_dist_all, self.kernel_val_all, self.dot_products, self.kernel_activations)

    def _is_device_copy(self, t):
        """True while ``t`` is a rollout tensor of the last propagate() that still equals the device-resident copy: a LazyRollout of
        this generation, or a fetched torch tensor nobody has written into since."""
        if isinstance(t, LazyRollout):
            return t._owner is self and t._gen == self._generation and not t._dirty
        return isinstance(t, torch.Tensor) and getattr(self, "_versions", {}).get(id(t), -1) == t._version

    def _fetch(self):
        """All rollout tensors of the last propagate as torch CPU tensors (one omds_get_rollouts), cached until the next one."""
        if not self._cache:
            self._cache = {k: torch.from_numpy(v) for k, v in self._engine.get_rollouts().items()}
        return self._cache

    @property
    def ker_w(self):
        kv = self._fetch()["kernel_val_all"]
        return kv[:, -1:, :].transpose(1, 2) if kv.numel() else None

    @property
    def norm_basis(self):
        """[N, H, n, n] basis whose column 0 is the obstacle normal (MPPI.py:122-127).  Column 0 comes
        from the device (normal_dirs); the tangent completion is the same LAPACK QR the reference calls
        (geqrf/orgqr via numpy), evaluated lazily and only for the entries a caller indexes -- nothing
        on the rollout path reads it (M v uses the closed form), the drivers read ONE entry per
        iteration (frankaPlanner.py:162)."""
        return _LazyBasis(self.normal_dirs)

    # ---- distance + gradient on arbitrary states (MPPI.py:227-282) ------------------------------------
    def distance_repulsion_nn(self, q_prev, aot=False):
        self._push()
        q = _np(q_prev).reshape(-1, self.n_dof)
        out_d, out_g = [], []
        for s in range(0, q.shape[0], self.N_traj):
            d, g, _, _ = self._engine.dist_grad(q[s:s + self.N_traj])
            out_d.append(d)
            out_g.append(g)
        self.nn_grad = torch.from_numpy(np.concatenate(out_g))
        return torch.from_numpy(np.concatenate(out_d)), self.nn_grad

    def update_kernel_normal_bases(self):
        """MPPI.py:284-304: re-evaluate the obstacle normal at every kernel centre."""
        K = self.Policy.n_kernels
        if K > 0:
            _, grad = self.distance_repulsion_nn(self.Policy.mu_c[0:K])
            g = grad.numpy()
            A = np.tile(np.eye(self.n_dof, dtype=np.float32), (K, 1, 1))
            A[:, :, 0] = g
            Q, _ = np.linalg.qr(A)
            Q = Q.astype(np.float32)
            Q[:, :, 0] = g / np.linalg.norm(g, axis=1, keepdims=True)
            self.Policy.kernel_obstacle_bases[0:K] = torch.from_numpy(Q)
        return 0

    # ---- cost and update (MPPI.py:315-345) -------------------------------------------------------------
    def get_cost(self):
        self._push()
        self.cur_cost = torch.from_numpy(self._engine.cost())
        self._qdot_cache = {}
        return self.cur_cost

    def init_comm(self, group=None):
        """Multi-GPU (one process per GPU, this object holds one shard of the rollouts; pass ``rollout_offset = rank * N_traj``
        to the constructor): creates the library's RCCL communicator over the ranks of ``group`` (any torch.distributed
        backend, it only carries the 128-byte id).  From then on ``shift_policy_means`` / ``get_qdot`` reduce over ALL shards
        on the device (csrc/comm.hip).  Raises OmdsError if RCCL is unusable -- there is no fallback."""
        from .dist import init_native_comm
        return init_native_comm(self._engine, group)

    def get_qdot(self, mode='best'):
        """MPPI.py:319-329.  After ``shift_policy_means()`` this is a local read, as in the reference: the update's reduction already
        produced both velocities (over ALL shards when a communicator exists) and they are kept until the next propagate / cost.
        Called BEFORE ``shift_policy_means()`` on a sharded context it has to run that reduction itself, which is a COLLECTIVE:
        then every rank must call it (a driver in which only rank 0 asks for the velocity would hang inside RCCL)."""
        if self.cur_cost is None:
            self.get_cost()
        if mode in self._qdot_cache:
            return self._qdot_cache[mode].clone()
        if self._engine.comm_info()[1] > 1:      # sharded: the arg-min / weighted mean over the rollouts of every rank (collective)
            K = self.Policy.n_kernels
            P = self.Policy
            _, _, _, _, qw, qb, _ = self._engine.weighted_update_sharded(0.0, self.ker_thr, P.mu_c.numpy()[:K], P.sigma_c.numpy()[:K],
                                                                         P.alpha_c.numpy()[:K], want_best=True)
            self._qdot_cache = {'weighted': torch.from_numpy(qw), 'best': torch.from_numpy(qb)}
            return self._qdot_cache[mode].clone()
        return torch.from_numpy(self._engine.get_qdot(mode))

    def shift_policy_means(self):
        """MPPI.py:331-345.  With a communicator (``init_comm``) the sums run over the rollouts of every rank: two all-reduces
        on the context stream inside ``omds_weighted_update_sharded``; without one the same call is the single-shard update."""
        if self.cur_cost is None:
            self.get_cost()
        P = self.Policy
        K = P.n_kernels
        mu, sg, al, mask, qw, qb, _ = self._engine.weighted_update_sharded(self.policy_upd_rate, self.ker_thr, P.mu_c.numpy(),
                                                                           P.sigma_c.numpy(), P.alpha_c.numpy(), want_best=True)
        if K > 0:
            P.mu_c[:K] = torch.from_numpy(mu)
            P.sigma_c[:K] = torch.from_numpy(sg)
            P.alpha_c[:K] = torch.from_numpy(al)
        self.update_mask = torch.from_numpy(mask)
        self.qdot_weighted = torch.from_numpy(qw)
        # get_qdot() of this cost is a local read from here on (the reduction above is the same one, over every shard)
        self._qdot_cache = {'weighted': torch.from_numpy(qw.copy()), 'best': torch.from_numpy(qb.copy())}
        return 0, int(mask.sum())
