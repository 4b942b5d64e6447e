"""What the scene memory of the depth route costs (omds_set_obstacles_from_depth_memory) beside the plain depth call of its parent
(omds_set_obstacles_from_depth, 0.14 ms in R20), on the same images.  EXPERIMENTS.md R23.
  scene     one 640 x 480 U16 camera (1 mm units) in front of a wall 3 m away, into a 128^3 grid of 5 cm cells (2 097 152 cells; the
            count buffer, the stored words and the new words are 8 MB each).  Frame A: the wall (about 3 000 cells).  Frame B: a plate at
            1.2 m over the left half of the image: half of the wall's cells are occluded -- they take k_scene_memory's slow path and stay
            remembered -- the other half and the plate are seen.  max_age = 0: nothing expires, every call of a leg does the same work
  legs      plain   : the parent's call on frame B
            memory  : the memory call on frame B, from the memory frame A left (steady state: the same cells are remembered every call)
            memory0 : the memory call on frame A again and again: every stored cell is seen, no lane takes the slow path
  protocol  R17's: a host clock around the synchronous call, the legs alternating call by call on contexts of their own, five warm-up
            calls per leg, the median of --calls with its minimum and maximum.  Run the whole command twice: the spread is part of the result
  kernel    k_scene_memory alone, by HIP events on the context's stream (omds_prof_enable brackets it), the mean of 50 launches per leg
  yardstick what streaming 25 MB costs on this device (a device-to-device copy of 12.5 MB, torch events, the median of 200) and what a
            launch costs (1 000 one-element kernels back to back over their count)
  --only-memory : nothing but 50 memory calls on frame B, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python ...)

    python tools/studies/scene_memory_cost.py [--calls 200] [--out profiles/r23_scene_memory_cost.txt] [--only-memory]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cloud_cost as r20  # noqa: E402
from optimalmodulationds_amd.engine import Engine, cloud_spec, depth_camera, scene_memory_spec  # noqa: E402

DIMS, VOXEL, ORIGIN = (128, 128, 128), 0.05, (-1.0, -3.2, -3.2)
WALL, PLATE = 3.0, 1.2


def frames():
    cam = depth_camera(640, 480, 600.0, 600.0, 319.5, 239.5, r20.look_at((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)), 0, 0.001, 0.2, 6.0)
    wall = np.full((480, 640), int(WALL * 1000), np.uint16)
    plate = wall.copy()
    plate[:, :320] = int(PLATE * 1000)
    return cam, wall, plate


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_scene_memory_cost.txt"))
    ap.add_argument("--only-memory", action="store_true")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cam, wall, plate = frames()
    spec = cloud_spec(ORIGIN, VOXEL, DIMS, max_spheres=16384)
    mem = scene_memory_spec(0)
    engines = {leg: Engine(7, 32, 3, 5, max_obs=64) for leg in ("plain", "memory", "memory0")}
    engines["memory"].set_obstacles_from_depth_memory([wall], [cam], spec, mem)
    calls = dict(plain=lambda: engines["plain"].set_obstacles_from_depth([plate], [cam], spec),
                 memory=lambda: engines["memory"].set_obstacles_from_depth_memory([plate], [cam], spec, mem),
                 memory0=lambda: engines["memory0"].set_obstacles_from_depth_memory([wall], [cam], spec, mem))
    if a.only_memory:
        for _ in range(50):
            calls["memory"]()
        return
    for _ in range(5):
        got = {leg: f() for leg, f in calls.items()}
    say(f"grid {DIMS} x {VOXEL} m, one 640 x 480 U16 camera; frame B: plain call {got['plain']}, memory call {got['memory']}; "
        f"frame A again: {got['memory0']}  (n_spheres, (seen, remembered, cleared, expired, self-forgotten))")
    t = {leg: [] for leg in calls}
    for _ in range(a.calls):
        for leg, f in calls.items():
            t0 = time.perf_counter()
            f()
            t[leg].append((time.perf_counter() - t0) * 1e3)
    for leg in calls:
        v = np.asarray(t[leg])
        say(f"{leg:8s} call: median {np.median(v):.4f} ms  min {v.min():.4f}  max {v.max():.4f}  ({a.calls} calls)")
    say(f"memory - plain: {np.median(t['memory']) - np.median(t['plain']):+.4f} ms;  memory0 - plain (against frame A's own plain call: see "
        f"the kernel times): {np.median(t['memory0']) - np.median(t['plain']):+.4f} ms")
    for leg in ("memory", "memory0"):
        e = engines[leg]
        e.prof_enable(1)
        e.prof_reset()
        for _ in range(50):
            calls[leg]()
        ms, launches, _, name = e.prof_read_ex()
        e.prof_enable(0)
        say(f"{name} ({leg}): {1e3 * ms / max(launches, 1):.2f} us per launch over {launches} launches (HIP events on the context's stream)")
    dev = f"cuda:{engines['plain'].device}"
    src, dst = torch.empty(12_500_000 // 4, dtype=torch.int32, device=dev), torch.empty(12_500_000 // 4, dtype=torch.int32, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(205)]
    for s, f in ev:
        s.record()
        dst.copy_(src)
        f.record()
    torch.cuda.synchronize()
    copy = np.asarray([s.elapsed_time(f) for s, f in ev[5:]])
    say(f"yardstick: a 12.5 MB device-to-device copy (25 MB of traffic) takes {1e3 * np.median(copy):.2f} us median of 200 "
        f"= {25e6 / (np.median(copy) * 1e-3) / 1e12:.2f} TB/s")
    one = torch.zeros(1, device=dev)
    for _ in range(100):
        one.add_(1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(1000):
        one.add_(1.0)
    torch.cuda.synchronize()
    say(f"yardstick: 1 000 one-element launches back to back: {(time.perf_counter() - t0) * 1e3:.2f} us per launch")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
