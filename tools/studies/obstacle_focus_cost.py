"""What the obstacle focus costs and what it buys (omds_focus_obstacles), on the two sensed scenes the earlier studies left behind: the
rendered 640 x 480 one-camera depth scene of depth_cloud_cost.py (EXPERIMENTS.md R20) and the 131 072-point cloud of point_cloud_cost.py
(R17), both on R17's grid (64 x 64 x 48 cells of 2.5 cm), on a 1024 x 32 Franka context with q at FRANKA_Q0.  EXPERIMENTS.md R22.
  focus call   R17's protocol: a host clock around the synchronous call, five warm-up calls, the median of 50 with minimum and maximum,
               per margin; every call selects from the stored master again.  Run the whole command twice: the spread is part of the result
  propagate    on the full master (one warm-up, then three repetitions: it is long) and on the focused scene at margin 0.05 / 0.1 /
               0.2 / 0.4 m (two warm-ups, the median of ten), in fp32 and screened with a fixed eps; host clock around propagate + sync
  equality     per margin the share of (rollout, step) rows whose closest_dist_all and all_traj equal the full propagate's bit for bit
               (fp32 against fp32, screened against screened), on the same context, scene and policy samples
The comparison to read: focus call + focused propagate against the full propagate.
  --only-focus : nothing but 20 focus calls per scene, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python ...)

    python tools/studies/obstacle_focus_cost.py [--calls 50] [--out profiles/r22_obstacle_focus_cost.txt] [--only-focus]"""
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
from optimalmodulationds_amd.engine import Engine, cloud_spec, depth_camera  # noqa: E402

F32 = np.float32
N, H, K, EPS = 1024, 32, 5, 0.02
MARGINS = (0.05, 0.1, 0.2, 0.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_obstacle_focus_cost.txt"))
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
    e.params.dt, e.params.dst_thr, e.params.ignored_links = 0.5, 0.01, 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    q0 = np.asarray(scenes.FRANKA_Q0, F32)
    rng = np.random.RandomState(0)
    e.set_policy_samples((q0 + 0.2 * rng.standard_normal((N, 3, 7))).astype(F32), np.ones((N, 3), F32), rng.standard_normal((N, 3, 7)).astype(F32))
    spec = cloud_spec(r20.ORIGIN, r20.VOXEL, r20.DIMS, max_spheres=65536)

    def depth_scene():
        cam = depth_camera(640, 480, 600.0, 600.0, 319.5, 239.5, r20.look_at(r20.EYES[0], r20.TARGET), 0, 0.001, 0.2, 6.0)
        return e.set_obstacles_from_depth([r20.render(cam, r20.scene_spheres(), 1.15)], [cam], spec)

    def cloud_scene():
        return e.set_obstacles_from_cloud(r17.make_cloud()[0], spec)

    def propagate_ms(warm, reps):
        t = []
        for it in range(warm + reps):
            t0 = time.perf_counter()
            e.propagate(q0)
            e.sync()
            if it >= warm:
                t.append((time.perf_counter() - t0) * 1e3)
        got = e.get_rollouts(want=("all_traj", "closest_dist_all"))
        return np.asarray(t), got["all_traj"].view(np.uint32).copy(), got["closest_dist_all"].view(np.uint32).copy()

    rows = []
    for scene, install in (("depth 640x480x1 (R20)", depth_scene), ("cloud 131072 (R17)", cloud_scene)):
        counts = install()
        O = e.n_obs
        say(f"# {scene}: {O} spheres in force (the call's counts: {tuple(int(c) for c in counts)})")
        if a.only_focus:
            for _ in range(20):
                e.focus_obstacles(q0, 0.1)
            e.clear_obstacle_focus()
            continue
        say(f"{'margin':>7s} | {'kept':>6s} {'passed':>6s} | focus call ms: {'median':>7s} {'min':>7s} {'max':>7s}")
        kept_of = {}
        for margin in MARGINS:
            t = []
            for it in range(5 + a.calls):
                t0 = time.perf_counter()
                kept, passed = e.focus_obstacles(q0, margin)
                if it >= 5:
                    t.append((time.perf_counter() - t0) * 1e3)
            t = np.asarray(t)
            kept_of[margin] = dict(kept=kept, passed=passed, focus_ms=float(np.median(t)), focus_min=float(t.min()), focus_max=float(t.max()))
            say(f"{margin:7.2f} | {kept:6d} {passed:6d} | {'':15s}{np.median(t):7.3f} {t.min():7.3f} {t.max():7.3f}")
        e.clear_obstacle_focus()
        for mode, label in ((0, "fp32"), (1, f"screened eps={EPS}")):
            e.set_screening(mode, EPS if mode else 0.0)
            e.clear_obstacle_focus()
            fb0 = e.screen_stats()["fallbacks"]
            t_full, traj_full, dist_full = propagate_ms(1, 3)
            fb_full = e.screen_stats()["fallbacks"] - fb0
            say(f"{label}: full master {O} spheres: propagate ms {np.median(t_full):9.3f} (three: {', '.join(f'{x:.3f}' for x in t_full)}), screening fallbacks {fb_full}")
            say(f"{'margin':>7s} | {'kept':>6s} | {'propagate':>9s} {'min':>8s} {'max':>8s} | {'focus + propagate':>17s} {'of full':>8s} | rows equal: {'dist':>7s} {'traj':>7s} | fallbacks")
            for margin in MARGINS:
                e.focus_obstacles(q0, margin)
                fb0 = e.screen_stats()["fallbacks"]
                t, traj, dist = propagate_ms(2, 10)
                fb = e.screen_stats()["fallbacks"] - fb0
                eq_d = float((dist == dist_full).mean())
                eq_t = float((traj == traj_full).all(axis=2).mean())
                k = kept_of[margin]
                both = k["focus_ms"] + float(np.median(t))
                rows.append(dict(scene=scene, spheres=O, mode=label, margin=margin, kept=k["kept"], passed=k["passed"], focus_ms=k["focus_ms"],
                                 focus_min=k["focus_min"], focus_max=k["focus_max"], propagate_ms=float(np.median(t)), propagate_min=float(t.min()),
                                 propagate_max=float(t.max()), full_ms=float(np.median(t_full)), full_all=[float(x) for x in t_full],
                                 rows_equal_dist=eq_d, rows_equal_traj=eq_t, fallbacks=int(fb), fallbacks_full=int(fb_full)))
                say(f"{margin:7.2f} | {k['kept']:6d} | {np.median(t):9.3f} {t.min():8.3f} {t.max():8.3f} | {both:17.3f} {both / np.median(t_full):8.4f} | "
                    f"{'':11s} {eq_d:7.4f} {eq_t:7.4f} | {fb}")
        e.set_screening(0, 0.0)
        e.clear_obstacle_focus()
    say(json.dumps(dict(study="obstacle_focus_cost", N=N, H=H, n_closest=K, eps=EPS, rows=rows)))
    e.close()
    if not a.only_focus:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
