"""What the velocity filter costs (omds_set_velocity_filter) and what it buys.  EXPERIMENTS.md R32.
  cost      the filtered tracked, objects and memory-tracked calls against the same calls without a filter, which ARE the parent's: the
            filter adds a stage and leaves every existing launch as it is.  Scenes and specs of the studies that measured those calls:
            tracked / objects : R18 / R19's pair of clouds (131 072 points, 64 x 64 x 48 cells of 2.5 cm, the shelf half moved one cell
                        between the frames, host arrays, reach 2, link 1, min_cells 4), frames alternating;
            memory  : R29's frame B (640 x 480 U16, a plate over the left half in front of a wall, 128^3 cells of 5 cm) from the
                        memory frame A left, with an object spec.
  protocol  R17's: a host clock around the synchronous call, the filtered and the unfiltered leg alternating call by call on contexts
            of their own, five warm-up calls per leg, the median of --calls with its minimum and maximum.  Run the whole command
            twice: the spread is part of the result
  accuracy  a sphere shell of radius 0.15 m translating at 0.3 m/s across the view of one 320 x 240 U16 camera 1.2 m away, 30 frames
            per second, gaussian depth noise of --noise metres per pixel (new draws every frame), 2.5 cm cells: per frame the error
            |v - v_true| of every live sphere, raw (velocity_filter_frame) and filtered (get_obstacle_motion), as RMS over the spheres
            and the frames behind --warm; per-cell flow and objects
  --only-filtered : nothing but 50 filtered memory-tracked calls at 128^3, for a kernel trace of their own (rocprofv3 --kernel-trace
            --stats -- python ...): k_vel_clear beside the fill of the record grid, which is what clearing the whole state grid
            (the same 32 MiB) would cost

    python tools/studies/velocity_filter_cost.py [--calls 200] [--out profiles/r30_velocity_filter_cost.txt] [--only-filtered]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cloud_cost as r20  # noqa: E402
import point_cloud_flow_cost as r18  # noqa: E402
import scene_memory_cost as r23  # noqa: E402
from optimalmodulationds_amd.engine import (Engine, cloud_object_spec, cloud_spec, cloud_track_spec, depth_camera,  # noqa: E402
                                            scene_memory_spec)

FILT = dict(alpha=0.3, alpha_object=0.3, max_jump=0.0)


def shell_frame(cam_args, centre, radius, noise, rng):
    """a depth image (U16, 1 mm units) of a sphere seen by a pinhole camera at the origin looking along +z of its own frame"""
    w, h, f = cam_args
    u, v = np.meshgrid(np.arange(w) - (w - 1) / 2.0, np.arange(h) - (h - 1) / 2.0)
    d = np.stack([u / f, v / f, np.ones_like(u)], -1)               # the ray of every pixel, z = 1
    dd, dc = (d * d).sum(-1), d @ centre
    disc = dc * dc - dd * (centre @ centre - radius * radius)
    z = np.where(disc > 0, (dc - np.sqrt(np.maximum(disc, 0))) / dd, 0.0)
    z = np.where(z > 0, z + noise * rng.standard_normal(z.shape), 0.0)
    return np.clip(np.rint(z * 1000.0), 0, 65535).astype(np.uint16)


def accuracy(say, noise, warm, frames=24):
    w, h, f, dt, voxel, radius = 320, 240, 300.0, 1.0 / 30.0, 0.025, 0.15
    v_true = np.array([0.3, 0.0, 0.0])
    pose = np.eye(4)[:3]                                             # the grid's frame is the camera's
    cam = depth_camera(w, h, f, f, (w - 1) / 2.0, (h - 1) / 2.0, pose, 0, 0.001, 0.2, 4.0)
    spec = cloud_spec((-0.8, -0.4, 0.8), voxel, (64, 32, 32), min_points=2, max_spheres=16384)
    track = cloud_track_spec(3, dt, 0.0)
    say(f"accuracy: shell r = {radius} m at {v_true[0]} m/s, {w} x {h} U16, noise {noise * 1e3:.1f} mm, {voxel * 100:.1f} cm cells, "
        f"{frames} frames, RMS over live spheres behind frame {warm}; filter {FILT}")
    for name, obj in (("per-cell flow", None), ("objects", cloud_object_spec(1, 4))):
        e = Engine(7, 32, 3, 5, max_obs=64)
        e.set_velocity_filter(FILT)
        rng = np.random.RandomState(7)
        err = {"raw": [], "filtered": []}
        for t in range(frames):
            img = shell_frame((w, h, f), np.array([-0.25, 0.0, 1.2]) + v_true * dt * t, radius, noise, rng)
            n = e.set_obstacles_from_depth([img], [cam], spec, None, track, obj)[0]
            if t < warm:
                continue
            raw, live, _ = e.velocity_filter_frame()
            vel, _ = e.get_obstacle_motion()
            on = live[:n] != 0
            err["raw"].append(((raw[:n][on] - v_true) ** 2).sum(1))
            err["filtered"].append(((vel[:n][on] - v_true) ** 2).sum(1))
        rms = {k: float(np.sqrt(np.concatenate(v).mean())) for k, v in err.items()}
        mean = float(np.concatenate([vel[:n][on]]).mean(0)[0])
        say(f"  {name:14s} raw {rms['raw']:.4f} m/s   filtered {rms['filtered']:.4f} m/s   ({rms['raw'] / max(rms['filtered'], 1e-12):.2f} x; "
            f"{int(on.sum())} live spheres in the last frame, their mean filtered v_x {mean:.4f})")
        e.close()


def main():
    import torch  # noqa: F401  (first, so that its HIP runtime is the one that starts)
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--noise", type=float, default=0.002)
    ap.add_argument("--warm", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_velocity_filter_cost.txt"))
    ap.add_argument("--only-filtered", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    track, obj, mem = cloud_track_spec(2, r18.DT_FRAME, 0.0), cloud_object_spec(1, 4), scene_memory_spec(0)
    cam, wall, plate = r23.frames()
    mspec = cloud_spec(r23.ORIGIN, r23.VOXEL, r23.DIMS, max_spheres=16384)
    mtrack = cloud_track_spec(2, 0.1, 0.0)
    if a.only_filtered:
        e = Engine(7, 32, 3, 5, max_obs=64)
        e.set_velocity_filter(FILT)
        e.set_obstacles_from_depth_memory_tracked([wall], [cam], mspec, mem, mtrack, obj)
        for _ in range(50):
            e.set_obstacles_from_depth_memory_tracked([plate], [cam], mspec, mem, mtrack, obj)
        return
    clouds = (r18.make_cloud()[0], r18.make_cloud((r18.VOXEL, 0.0, 0.0))[0])
    cspec = cloud_spec(r18.ORIGIN, r18.VOXEL, r18.DIMS, max_spheres=65536)
    legs = ("tracked", "objects", "memory")
    engines = {(leg, f): Engine(7, 32, 3, 5, max_obs=64) for leg in legs for f in (False, True)}
    for (leg, f), e in engines.items():
        if f:
            e.set_velocity_filter(FILT)
        if leg == "memory":
            e.set_obstacles_from_depth_memory_tracked([wall], [cam], mspec, mem, mtrack, obj)

    def call(leg, f, it):
        e = engines[(leg, f)]
        if leg == "tracked":
            return e.set_obstacles_from_cloud_tracked(clouds[it % 2], cspec, track)
        if leg == "objects":
            return e.set_obstacles_from_cloud_objects(clouds[it % 2], cspec, track, obj)
        return e.set_obstacles_from_depth_memory_tracked([plate], [cam], mspec, mem, mtrack, obj)

    t = {k: [] for k in engines}
    for it in range(5 + a.calls):
        for k in engines:
            t0 = time.perf_counter()
            got = call(*k, it)
            if it >= 5:
                t[k].append((time.perf_counter() - t0) * 1e3)
            if it == 4 + a.calls and k[1]:
                e = engines[k]
                say(f"{k[0]:8s} returns {got}; filter counts {e.velocity_filter_frame()[2]}; "
                    f"cells with history {int((e.velocity_filter_state()[:, 3] > 0).sum())}")
    for leg in legs:
        off, on = np.asarray(t[(leg, False)]), np.asarray(t[(leg, True)])
        say(f"{leg:8s} call: unfiltered median {np.median(off):.4f} ms  min {off.min():.4f}  max {off.max():.4f} | filtered median "
            f"{np.median(on):.4f} ms  min {on.min():.4f}  max {on.max():.4f} | {np.median(on) - np.median(off):+.4f} ms  "
            f"x {np.median(on) / np.median(off):.3f}  ({a.calls} calls)")
    for e in engines.values():
        e.close()
    accuracy(say, a.noise, a.warm)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
