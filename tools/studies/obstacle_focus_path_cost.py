"""What the obstacle focus along a path costs and what it buys (omds_focus_obstacles_path) beside the single-state call, on the two
sensed scenes of obstacle_focus_cost.py (EXPERIMENTS.md R22): the rendered 640 x 480 depth scene (7 035 spheres) and the 131 072-point
cloud (29 713), on the same 1024 x 32 Franka context (n_closest 5, dt 0.5, three kernels of fixed samples).  EXPERIMENTS.md R28.
  cost     R22's protocol: a host clock around the synchronous call, five warm-up calls, the median of 50 with minimum and maximum; the
           single-state call and the path call at B = 1, 8, 32, 128 states, alternating in blocks, at margin 0.1.  The B states are the
           first B of the 8 lowest-cost rollouts of the full propagate, taken step by step.  Run the whole command twice
  effect   the full propagate first (its rollouts are "the previous iteration's"); then per focus the kept count and the share of
           (rollout, step) rows whose closest_dist_all / all_traj equal the full propagate's bit for bit:
             single   the single-state focus at q0, margins 0.05 .. 0.4 (R22's rows)
             path-1   the path focus over q0 + the 32 states of rollout 0, ahead = step dt
             path-8   the path focus over q0 + the 256 states of the 8 lowest-cost rollouts
           each path at margins 0 .. 0.2 without a cap, and -- THE COMPARISON AT EQUAL KEPT COUNT -- at margin +inf with max_keep = the
           single-state focus's kept count at each of its margins (the kept-count nearest to any state of the path)
  --only-focus : nothing but 20 path calls at B = 128 per scene, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- ...)

    python tools/studies/obstacle_focus_path_cost.py [--calls 50] [--out profiles/r28_obstacle_focus_path_cost.txt] [--only-focus]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cloud_cost as r20  # noqa: E402
import point_cloud_cost as r17  # noqa: E402
from optimalmodulationds_amd import scenes  # noqa: E402
from optimalmodulationds_amd.cost import FRANKA_Q_MAX, FRANKA_Q_MIN  # noqa: E402
from optimalmodulationds_amd.engine import Engine, cloud_spec, depth_camera  # noqa: E402

F32 = np.float32
N, H, K, DT = 1024, 32, 5, 0.5
MARGINS = (0.05, 0.1, 0.2, 0.4)
PATH_MARGINS = (0.0, 0.05, 0.1, 0.2)
BS = (1, 8, 32, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_obstacle_focus_path_cost.txt"))
    ap.add_argument("--only-focus", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    z = np.load(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
    n = len([k for k in z.files if k.startswith("W")])
    e = Engine(7, N, H, K, max_obs=2 * scenes.shelf_scene().shape[0])
    e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
    e.params.dt, e.params.dst_thr, e.params.ignored_links = DT, 0.01, 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_cost(scenes.franka_dh_params(), np.array(FRANKA_Q_MIN, F32), np.array(FRANKA_Q_MAX, F32))
    q0 = np.asarray(scenes.FRANKA_Q0, F32)
    rng = np.random.RandomState(0)
    e.set_policy_samples((q0 + 0.2 * rng.standard_normal((N, 3, 7))).astype(F32), np.ones((N, 3), F32), rng.standard_normal((N, 3, 7)).astype(F32))
    spec = cloud_spec(r20.ORIGIN, r20.VOXEL, r20.DIMS, max_spheres=65536)

    def depth_scene():
        cam = depth_camera(640, 480, 600.0, 600.0, 319.5, 239.5, r20.look_at(r20.EYES[0], r20.TARGET), 0, 0.001, 0.2, 6.0)
        return e.set_obstacles_from_depth([r20.render(cam, r20.scene_spheres(), 1.15)], [cam], spec)

    def cloud_scene():
        return e.set_obstacles_from_cloud(r17.make_cloud()[0], spec)

    def propagate():
        e.propagate(q0)
        e.sync()
        got = e.get_rollouts(want=("all_traj", "closest_dist_all"))
        return got["all_traj"], got["closest_dist_all"]

    def timed(call):
        t = []
        for it in range(5 + a.calls):
            t0 = time.perf_counter()
            call()
            if it >= 5:
                t.append((time.perf_counter() - t0) * 1e3)
        return np.asarray(t)

    rows, costs = [], []
    for scene, install in (("depth 640x480x1 (R20)", depth_scene), ("cloud 131072 (R17)", cloud_scene)):
        counts = install()
        O = e.n_obs
        say(f"# {scene}: {O} spheres in force (the call's counts: {tuple(int(c) for c in counts)})")
        traj_full, dist_full = propagate()
        best = np.argsort(e.cost(), kind="stable")[:8]
        ahead_of = (np.arange(H) * DT).astype(F32)
        # step-major over the 8 best rollouts: the first B states are the early steps of all eight
        states8 = np.ascontiguousarray(traj_full[best].transpose(1, 0, 2).reshape(-1, 7))
        ahead8 = np.repeat(ahead_of, 8)
        path1 = (np.concatenate([q0[None], traj_full[0]]), np.concatenate([[0.0], ahead_of]).astype(F32))
        path8 = (np.concatenate([q0[None], states8]), np.concatenate([[0.0], ahead8]).astype(F32))
        if a.only_focus:
            for _ in range(20):
                e.focus_obstacles_path(states8[:128], 0.1, 0, 0.0, ahead8[:128])
            e.clear_obstacle_focus()
            continue
        say(f"{'call':>12s} | {'kept':>6s} {'passed':>6s} | call ms: {'median':>7s} {'min':>7s} {'max':>7s}   (margin 0.1, two blocks each, alternating)")
        for block in (1, 2):
            t = timed(lambda: e.focus_obstacles(q0, 0.1))
            kept, passed = e.focus_obstacles(q0, 0.1)
            costs.append(dict(scene=scene, spheres=O, call="single", block=block, kept=kept, ms=float(np.median(t)), min=float(t.min()), max=float(t.max())))
            say(f"{'single':>12s} | {kept:6d} {passed:6d} | {'':9s}{np.median(t):7.3f} {t.min():7.3f} {t.max():7.3f}")
            for B in BS:
                t = timed(lambda: e.focus_obstacles_path(states8[:B], 0.1, 0, 0.0, ahead8[:B]))
                kept, passed = e.focus_obstacles_path(states8[:B], 0.1, 0, 0.0, ahead8[:B])
                costs.append(dict(scene=scene, spheres=O, call=f"path B={B}", block=block, kept=kept, ms=float(np.median(t)), min=float(t.min()),
                                  max=float(t.max())))
                say(f"{'path B=' + str(B):>12s} | {kept:6d} {passed:6d} | {'':9s}{np.median(t):7.3f} {t.min():7.3f} {t.max():7.3f}")
        e.clear_obstacle_focus()

        def effect(label, margin, max_keep, focus):
            kept, passed = focus()
            t0 = time.perf_counter()
            traj, dist = propagate()
            ms = (time.perf_counter() - t0) * 1e3
            eq_d = float((dist.view(np.uint32) == dist_full.view(np.uint32)).mean())
            eq_t = float((traj.view(np.uint32) == traj_full.view(np.uint32)).all(axis=2).mean())
            rows.append(dict(scene=scene, spheres=O, focus=label, margin=float(margin), max_keep=int(max_keep), kept=kept, passed=passed,
                             rows_equal_dist=eq_d, rows_equal_traj=eq_t, propagate_and_fetch_ms=ms))
            say(f"{label:>8s} {margin:6.2f} {max_keep:7d} | {kept:6d} {passed:6d} | {eq_d:7.4f} {eq_t:7.4f} | {ms:9.2f}")
            return kept

        say(f"{'focus':>8s} {'margin':>6s} {'cap':>7s} | {'kept':>6s} {'passed':>6s} | rows equal: dist, traj | one propagate + fetch ms")
        kept_single = [effect("single", m, 0, lambda m=m: e.focus_obstacles(q0, m)) for m in MARGINS]
        for label, (path, ahead) in (("path-1", path1), ("path-8", path8)):
            for m in PATH_MARGINS:
                effect(label, m, 0, lambda m=m: e.focus_obstacles_path(path, m, 0, 0.0, ahead))
            for cap in kept_single:
                effect(label, np.inf, cap, lambda cap=cap: e.focus_obstacles_path(path, np.inf, cap, 0.0, ahead))
        e.clear_obstacle_focus()
    say(json.dumps(dict(study="obstacle_focus_path_cost", N=N, H=H, n_closest=K, costs=costs, rows=rows)))
    e.close()
    if not a.only_focus:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
