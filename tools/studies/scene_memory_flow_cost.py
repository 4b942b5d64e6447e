"""What memory and velocities in one depth call cost (omds_set_obstacles_from_depth_memory_tracked) beside the two calls it stands for:
the parent's memory call (omds_set_obstacles_from_depth_memory, R23) and the parent's tracked depth call (omds_set_obstacles_from_depth
with a track spec, R20), on the same images in the same run.  Both are unchanged by this work (their kernels keep their code), so the
calls of this tree ARE the parent's.  EXPERIMENTS.md R29.
  scene     R23's: one 640 x 480 U16 camera (1 mm units) in front of a wall 3 m away, into a 128^3 grid of 5 cm cells.  Frame A: the wall
            (about 3 000 cells).  Frame B: a plate at 1.2 m over the left half of the image: half of the wall's cells are occluded and
            stay remembered, the other half and the plate are seen.  max_age = 0: every call of a leg does the same work
  legs      memory  : the memory call on frame B, from the memory frame A left
            tracked : the tracked call on frame B, its stored frame the previous call's (frame B: every seen cell finds itself)
            both    : the new call on frame B, from the memory frame A left, its stored frame the previous call's
            objects / both_obj : the last two with an object spec (link 1, min_cells 4)
  expected  both < memory + tracked: one counting pass, one staging copy and one install where they make two; it adds one compaction
            (the seen sublist) and one scatter launch, and its k_scene_memory reads the counts out of 16-byte records
  protocol  R17's: a host clock around the synchronous call, the legs alternating call by call on contexts of their own, five warm-up
            calls per leg, the median of --calls with its minimum and maximum.  Run the whole command twice: the spread is part of the result
  kernel    k_scene_memory of both forms by HIP events on the context's stream (omds_prof_enable brackets it), the mean of 50 launches
  --only-both : nothing but 50 calls of the new route (with objects), for a kernel trace of its own: the per-launch times of
            k_scene_memory<uint4>, k_compact_*<SeenSrc> and k_scene_memory_flow (rocprofv3 --kernel-trace --stats -- python ...)

    python tools/studies/scene_memory_flow_cost.py [--calls 200] [--out profiles/r29_scene_memory_flow_cost.txt] [--only-both]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_memory_cost as r23  # noqa: E402
from optimalmodulationds_amd.engine import Engine, cloud_object_spec, cloud_spec, cloud_track_spec, scene_memory_spec  # noqa: E402


def main():
    import torch  # noqa: F401  (first, so that its HIP runtime is the one that starts)
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_scene_memory_flow_cost.txt"))
    ap.add_argument("--only-both", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cam, wall, plate = r23.frames()
    spec = cloud_spec(r23.ORIGIN, r23.VOXEL, r23.DIMS, max_spheres=16384)
    mem, track, obj = scene_memory_spec(0), cloud_track_spec(2, 0.1, 0.0), cloud_object_spec(1, 4)
    legs = ("memory", "tracked", "both", "objects", "both_obj")
    engines = {leg: Engine(7, 32, 3, 5, max_obs=64) for leg in legs}
    engines["memory"].set_obstacles_from_depth_memory([wall], [cam], spec, mem)
    engines["both"].set_obstacles_from_depth_memory_tracked([wall], [cam], spec, mem, track)
    engines["both_obj"].set_obstacles_from_depth_memory_tracked([wall], [cam], spec, mem, track, obj)
    calls = dict(memory=lambda: engines["memory"].set_obstacles_from_depth_memory([plate], [cam], spec, mem),
                 tracked=lambda: engines["tracked"].set_obstacles_from_depth([plate], [cam], spec, track=track),
                 both=lambda: engines["both"].set_obstacles_from_depth_memory_tracked([plate], [cam], spec, mem, track),
                 objects=lambda: engines["objects"].set_obstacles_from_depth([plate], [cam], spec, track=track, obj=obj),
                 both_obj=lambda: engines["both_obj"].set_obstacles_from_depth_memory_tracked([plate], [cam], spec, mem, track, obj))
    if a.only_both:
        for _ in range(50):
            calls["both_obj"]()
        return
    for _ in range(5):
        got = {leg: f() for leg, f in calls.items()}
    say(f"grid {r23.DIMS} x {r23.VOXEL} m, one 640 x 480 U16 camera, frame B")
    for leg in legs:
        say(f"  {leg:8s} returns {got[leg]}")
    t = {leg: [] for leg in calls}
    for _ in range(a.calls):
        for leg, f in calls.items():
            t0 = time.perf_counter()
            f()
            t[leg].append((time.perf_counter() - t0) * 1e3)
    med = {leg: float(np.median(t[leg])) for leg in calls}
    for leg in calls:
        v = np.asarray(t[leg])
        say(f"{leg:8s} call: median {med[leg]:.4f} ms  min {v.min():.4f}  max {v.max():.4f}  ({a.calls} calls)")
    say(f"both     - (memory + tracked): {med['both'] - med['memory'] - med['tracked']:+.4f} ms  (the sum: {med['memory'] + med['tracked']:.4f})")
    say(f"both_obj - (memory + objects): {med['both_obj'] - med['memory'] - med['objects']:+.4f} ms  (the sum: {med['memory'] + med['objects']:.4f})")
    for leg in ("memory", "both"):
        e = engines[leg]
        e.prof_enable(1)
        e.prof_reset()
        for _ in range(50):
            calls[leg]()
        ms, launches, _, name = e.prof_read_ex()
        e.prof_enable(0)
        say(f"{name} ({leg}: {'counts' if leg == 'memory' else 'records'}): {1e3 * ms / max(launches, 1):.2f} us per launch over {launches} launches "
            f"(HIP events on the context's stream)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
