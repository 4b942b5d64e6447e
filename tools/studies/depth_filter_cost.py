"""What the depth filter costs (omds_set_depth_filter in front of omds_set_obstacles_from_depth) beside the unfiltered depth call and
beside the route a user would otherwise take, on one rendered 640 x 480 U16 image: R20's scene (the shelf's spheres, balls along the
arm, clutter, a back wall) from R20's first camera, into R17's grid (64 x 64 x 48 cells of 2.5 cm) on a 1024 x 32 context, with one
pixel in sixteen turned into speckle or a hole.  EXPERIMENTS.md R27.
R17's protocol: a host clock around the synchronous call, the legs alternating call by call, five warm-up calls per leg, the median
of --calls with its minimum and maximum.  Run the whole command twice: the spread between the runs is part of the result.
  a        the unfiltered depth call (no filter set): the parent's call
  b r      the filtered depth call at radius r = 1, 2, 3 (min_support 4, 10, 20; edge 0.01 + 0.01 z), plain and tracked
  c r      the filter restated as torch operations on the device (z_n, a padded image, one shifted comparison per window position,
           the deprojection of R20's torch route on the kept pixels), then the cloud call on the device tensor
  each from host images ("host": leg c uploads the image first) and from an image that is already on the device ("dev")
  d        the LDS-tile form against the direct-load form, kernel times: tools/ubench/depth_filter_forms, when it has been built

    python tools/studies/depth_filter_cost.py [--calls 200] [--out profiles/r27_depth_filter_cost.txt]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_cloud_cost as r20  # noqa: E402
from optimalmodulationds_amd import scenes  # noqa: E402
from optimalmodulationds_amd.engine import Engine, cloud_spec, cloud_track_spec, depth_camera, depth_filter_spec, depth_points  # noqa: E402

FILTERS = {1: dict(radius=1, min_support=4, edge_abs=0.01, edge_rel=0.01), 2: dict(radius=2, min_support=10, edge_abs=0.01, edge_rel=0.01),
           3: dict(radius=3, min_support=20, edge_abs=0.01, edge_rel=0.01)}
FORMS = os.path.join(ROOT, "tools", "ubench", "depth_filter_forms")


def noisy(img, seed=0):
    """one pixel in sixteen: half of them holes (raw 0), half speckle at a random depth of 0.5 .. 3.5 m"""
    rng = np.random.RandomState(seed)
    img = img.copy()
    what = rng.randint(0, 32, img.shape)
    img[what == 0] = 0
    speckle = what == 1
    img[speckle] = rng.randint(500, 3500, int(speckle.sum())).astype(np.uint16)
    return img


class TorchFilterRoute(r20.TorchRoute):
    """R20's torch route with the filter in front of the deprojection, all on the device"""

    def points_filtered(self, t16, filt):
        torch = self.torch
        a, b, Rt, t, scale, z_min, z_max = self.cams[0]
        R = int(filt["radius"])
        raw = t16.to(torch.int32) & 0xffff
        z = torch.where(raw != 0, raw.to(torch.float32) * scale, torch.full((), float("nan"), device=self.dev))
        keep = (z >= z_min) & (z <= z_max)
        tol = filt["edge_rel"] * z + filt["edge_abs"]
        pad = torch.nn.functional.pad(z, (R, R, R, R), value=float("nan"))
        H, W = z.shape
        support = torch.zeros_like(raw)
        for dy in range(2 * R + 1):
            for dx in range(2 * R + 1):
                if dy != R or dx != R:
                    support += ((pad[dy:dy + H, dx:dx + W] - z).abs() <= tol).to(torch.int32)
        keep &= support >= int(filt["min_support"])
        zz = torch.where(keep, z, torch.zeros_like(z))
        pts = torch.stack([a * zz, b * zz, zz], -1).reshape(-1, 3) @ Rt + t
        return torch.where(keep.reshape(-1, 1), pts, torch.full_like(pts, float("nan")))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_depth_filter_cost.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    z = np.load(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
    n = len([k for k in z.files if k.startswith("W")])
    e = Engine(7, 1024, 32, 5, max_obs=2 * scenes.shelf_scene().shape[0])
    e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
    dev = f"cuda:{e.device}"
    spec = cloud_spec(r20.ORIGIN, r20.VOXEL, r20.DIMS, max_spheres=65536)
    track = cloud_track_spec(2, r20.DT_FRAME)
    cam = depth_camera(640, 480, 600.0, 600.0, 319.5, 239.5, r20.look_at(r20.EYES[0], r20.TARGET), 0, 0.001, 0.2, 6.0)
    img = noisy(r20.render(cam, r20.scene_spheres(), 1.15))
    route = TorchFilterRoute([cam], dev)
    img_dev = route.upload([img])[0]
    torch.cuda.synchronize()
    say(f"one 640 x 480 U16 image, {depth_points(img, cam)[1]} pixels kept by the range gate; grid {r20.DIMS} x {r20.VOXEL} m; {a.calls} calls per leg, ms")
    for r, f in FILTERS.items():
        _, kept, rejected = depth_points(img, cam, filter=f)
        say(f"# radius {r} min_support {f['min_support']}: the filter keeps {kept} pixels and rejects {rejected}")

    def with_filter(f, call):
        def run():
            e.set_depth_filter(None if f is None else depth_filter_spec(**f))
            return call()
        return run

    def timed(legs):
        ms, last = {k: [] for k in legs}, {}
        for it in range(5 + a.calls):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                last[name] = fn()
                t1 = time.perf_counter()
                if it >= 5:
                    ms[name].append((t1 - t0) * 1e3)
        for name in legs:
            t = np.asarray(ms[name])
            say(f"{name:22s} | {np.median(t):8.4f} {t.min():8.4f} {t.max():8.4f} | {[int(g) for g in last[name]]}")
        return {k: float(np.median(v)) for k, v in ms.items()}

    say(f"{'leg':22s} | {'median':>8s} {'min':>8s} {'max':>8s} | counts (spheres, occupied[, matched])")
    med = {}
    for where, src in (("host", img), ("dev", img_dev)):
        legs = {f"a {where}": with_filter(None, lambda: e.set_obstacles_from_depth([src], [cam], spec))}
        for r, f in FILTERS.items():
            legs[f"b r{r} {where}"] = with_filter(f, lambda: e.set_obstacles_from_depth([src], [cam], spec))
            if where == "host":
                legs[f"c r{r} {where}"] = lambda f=f: e.set_obstacles_from_cloud(route.points_filtered(route.upload([img])[0], f), spec)
            else:
                legs[f"c r{r} {where}"] = lambda f=f: e.set_obstacles_from_cloud(route.points_filtered(img_dev, f), spec)
        med.update(timed(legs))
        e.cloud_track_reset()
        legs = {f"a tracked {where}": with_filter(None, lambda: e.set_obstacles_from_depth([src], [cam], spec, track=track))}
        for r, f in FILTERS.items():
            legs[f"b r{r} tracked {where}"] = with_filter(f, lambda: e.set_obstacles_from_depth([src], [cam], spec, track=track))
        med.update(timed(legs))
    for where in ("host", "dev"):
        for r in FILTERS:
            b, c, plain = med[f"b r{r} {where}"], med[f"c r{r} {where}"], med[f"a {where}"]
            say(f"radius {r} {where:4s}: filtered call {b:.4f} ms = unfiltered {plain:.4f} {b - plain:+.4f};  torch filter + cloud call {c:.4f} ms: "
                f"{c / b:.2f} x the filtered call ({c - b:+.4f} ms)")
    e.close()
    if os.path.exists(FORMS):
        say("# d: the two forms of the kernel (tools/ubench/depth_filter_forms)")
        out = subprocess.run([FORMS, str(a.calls)], capture_output=True, text=True, timeout=300)
        for line in (out.stdout + out.stderr).strip().splitlines():
            say(line)
    else:
        say("# d: tools/ubench/depth_filter_forms is not built: the two forms were not measured in this run")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
