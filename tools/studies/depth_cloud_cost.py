"""What the scene straight from depth images costs (omds_set_obstacles_from_depth) beside the routes a user had before it, on rendered
scenes: the shelf's spheres, balls along the arm at FRANKA_Q0 and a few clutter balls in front of a back wall, seen by one or three
pinhole cameras (U16, 1 mm units), into R17's grid (64 x 64 x 48 cells of 2.5 cm) on a 1024 x 32 context.  EXPERIMENTS.md R20.
R17's protocol: a host clock around the synchronous call, the legs of one configuration alternating call by call, five warm-up calls
per leg, the median of 50 with its minimum and maximum.  Run the whole command twice: the spread between the runs is part of the result.
  a        the depth call, host images
  b        the depth call, device images (int16 tensors holding the uint16 bits)
  c        the parent's host route: omds_depth_points per image on the host, concatenated, the cloud call on the host array
  d_host   the parent's device route from host images: the images copied to the device, the deprojection as torch operations there
           (pixel grids and poses cached on the device), torch.cat, the cloud call on the device tensor
  d_dev    the same from images that are already on the device
  tracked / objects: legs a and d_host through the tracked / objects calls (the same frame every call: the front ends differ, the
           rest is R18's / R19's static case)
  --ab-flags F: the tracked leg a on a second context created with config flags F, alternating with the first.  R20's A/B of the two
           counting forms was run on a build in which bit 128 selected the plain form (one atomic per kept pixel); HEAD holds one form.

    python tools/studies/depth_cloud_cost.py [--calls 50] [--out profiles/r20_depth_cloud_cost.txt] [--ab-flags 128]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from optimalmodulationds_amd import scenes  # noqa: E402
from optimalmodulationds_amd.engine import (Engine, cloud_object_spec, cloud_spec, cloud_track_spec, depth_camera,  # noqa: E402
                                            depth_points)
from oracle import omds_oracle as orc  # noqa: E402

DIMS, VOXEL, ORIGIN, DT_FRAME = (64, 64, 48), 0.025, (-0.4, -0.8, 0.0), 1.0 / 30.0
F32, F64 = np.float32, np.float64
EYES = ((-0.9, -0.9, 1.0), (-0.9, 0.9, 1.1), (-1.2, 0.0, 1.5))
TARGET = (0.4, 0.0, 0.5)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    eye, target = np.asarray(eye, F64), np.asarray(target, F64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, F64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), eye.reshape(3, 1)], 1).astype(F32)


def scene_spheres(seed=0):
    rng = np.random.RandomState(seed)
    q0 = np.asarray(scenes.FRANKA_Q0, F32)
    ends = np.concatenate([np.zeros((1, 3)), orc.link_endpoints(q0, scenes.franka_dh_params())])
    arm = [np.append(ends[i] * (1 - s) + ends[i + 1] * s, 0.06) for i in range(len(ends) - 1) for s in (0.0, 0.33, 0.67)]
    lo, ext = np.array(ORIGIN), np.array(DIMS) * VOXEL
    clutter = np.concatenate([lo + rng.uniform(0.1, 0.9, (12, 3)) * ext, rng.uniform(0.02, 0.06, (12, 1))], 1)
    return np.concatenate([scenes.shelf_scene(), np.asarray(arm), clutter]).astype(F64)


def render(cam, spheres, wall_x):
    """depth along the optical axis [H, W] of the nearest sphere or of the wall x = wall_x, in raw units of 1 mm (uint16)"""
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    u, v = np.meshgrid(np.arange(cam.width, dtype=F64), np.arange(cam.height, dtype=F64))
    d = np.stack([(u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, np.ones_like(u)], -1) @ p[:, :3].T
    o = p[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        best = (wall_x - o[0]) / d[..., 0]
        best = np.where(best > 0, best, np.inf)
        A = (d * d).sum(-1)
        for s in spheres:
            oc = o - s[:3]
            B = 2 * (d @ oc)
            disc = B * B - 4 * A * (oc @ oc - s[3] * s[3])
            t = (-B - np.sqrt(disc)) / (2 * A)
            best = np.minimum(best, np.where((disc >= 0) & (t > 0), t, np.inf))
    return np.clip(np.round(np.where(np.isfinite(best), best, 0.0) * 1000.0), 0, 65535).astype(np.uint16)


class TorchRoute:
    """the parent's device route: per camera the cached pixel grids and pose on the device, the deprojection as torch operations"""

    def __init__(self, cams, dev):
        import torch
        self.torch, self.dev, self.cams = torch, dev, []
        for c in cams:
            u, v = np.meshgrid(np.arange(c.width, dtype=F32), np.arange(c.height, dtype=F32))
            a, b = (u - F32(c.cx)) * (F32(1) / F32(c.fx)), (v - F32(c.cy)) * (F32(1) / F32(c.fy))
            p = np.array(list(c.pose), F32).reshape(3, 4)
            self.cams.append((torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(p[:, :3].T.copy()).to(dev),
                              torch.from_numpy(p[:, 3].copy()).to(dev), float(c.depth_scale), float(c.z_min), float(c.z_max)))

    def points(self, images_dev):
        torch, out = self.torch, []
        for t16, (a, b, Rt, t, scale, z_min, z_max) in zip(images_dev, self.cams):
            raw = t16.to(torch.int32) & 0xffff
            z = raw.to(torch.float32) * scale
            keep = (raw != 0) & (z >= z_min) & (z <= z_max)
            pts = torch.stack([a * z, b * z, z], -1).reshape(-1, 3) @ Rt + t
            out.append(torch.where(keep.reshape(-1, 1), pts, torch.full_like(pts, float("nan"))))
        return out[0] if len(out) == 1 else torch.cat(out)

    def upload(self, images):
        return [self.torch.from_numpy(im.view(np.int16)).to(self.dev) for im in images]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_depth_cloud_cost.txt"))
    ap.add_argument("--ab-flags", type=int, default=0)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    z = np.load(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
    n = len([k for k in z.files if k.startswith("W")])

    def engine(flags=0):
        e = Engine(7, 1024, 32, 5, max_obs=2 * scenes.shelf_scene().shape[0], flags=flags)
        e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
        e.params.ignored_links = 0b111
        e.push_params()
        return e

    e = engine()
    e_ab = engine(a.ab_flags) if a.ab_flags else None
    dev = f"cuda:{e.device}"
    spec = cloud_spec(ORIGIN, VOXEL, DIMS, max_spheres=65536)
    track, obj = cloud_track_spec(2, DT_FRAME), cloud_object_spec(1, 4)
    spheres = scene_spheres()
    rows = []

    def timed(legs):
        """legs: name -> callable returning the call's counts; alternating call by call -> name -> (ms array, last counts)"""
        ms, last = {k: [] for k in legs}, {}
        for it in range(5 + a.calls):
            for name, fn in legs.items():
                t0 = time.perf_counter()
                last[name] = fn()
                t1 = time.perf_counter()
                if it >= 5:
                    ms[name].append((t1 - t0) * 1e3)
        return {k: (np.asarray(v), last[k]) for k, v in ms.items()}

    def report(config, route, res):
        for name, (t, got) in res.items():
            row = dict(config=config, route=route, leg=name, ms=float(np.median(t)), min=float(t.min()), max=float(t.max()), calls=int(t.size),
                       counts=[int(g) for g in got])
            rows.append(row)
            say(f"{config:14s} {route:9s} {name:8s} | {row['ms']:8.3f} {row['min']:8.3f} {row['max']:8.3f} | {row['counts']}")

    say(f"{'config':14s} {'route':9s} {'leg':8s} | {'median':>8s} {'min':>8s} {'max':>8s} | counts (spheres, occupied[, matched[, objects, matched objects]])  -- ms")
    for config, (W, H, n_cams) in (("640x480x1", (640, 480, 1)), ("640x480x3", (640, 480, 3)), ("1280x720x1", (1280, 720, 1))):
        f = 600.0 * W / 640
        cams = [depth_camera(W, H, f, f, W / 2 - 0.5, H / 2 - 0.5, look_at(eye, TARGET), 0, 0.001, 0.2, 6.0) for eye in EYES[:n_cams]]
        t0 = time.perf_counter()
        images = [render(c, spheres, 1.15) for c in cams]
        n_valid = sum(depth_points(im, c)[1] for im, c in zip(images, cams))
        say(f"# {config}: {n_cams} camera(s), {n_cams * W * H} pixels, {n_valid} kept by the range gate (rendered in {time.perf_counter() - t0:.1f} s)")
        route_t = TorchRoute(cams, dev)
        images_dev = route_t.upload(images)
        torch.cuda.synchronize()

        def host_points():
            return np.concatenate([depth_points(im, c)[0] for im, c in zip(images, cams)]) if n_cams > 1 else depth_points(images[0], cams[0])[0]

        res = timed({
            "a": lambda: e.set_obstacles_from_depth(images, cams, spec),
            "b": lambda: e.set_obstacles_from_depth(images_dev, cams, spec),
            "c": lambda: e.set_obstacles_from_cloud(host_points(), spec),
            "d_host": lambda: e.set_obstacles_from_cloud(route_t.points(route_t.upload(images)), spec),
            "d_dev": lambda: e.set_obstacles_from_cloud(route_t.points(images_dev), spec),
        })
        report(config, "untracked", res)
        for route, kw in (("tracked", dict(track=track)), ("objects", dict(track=track, obj=obj))):
            e.cloud_track_reset()
            if route == "tracked":
                d_call = lambda: e.set_obstacles_from_cloud_tracked(route_t.points(route_t.upload(images)), spec, track)
            else:
                d_call = lambda: e.set_obstacles_from_cloud_objects(route_t.points(route_t.upload(images)), spec, track, obj)
            res = timed({"a": lambda: e.set_obstacles_from_depth(images, cams, spec, **kw), "d_host": d_call})
            report(config, route, res)
        if e_ab is not None and W == 640:
            for where, ims in (("host", images), ("device", images_dev)):
                e.cloud_track_reset()
                e_ab.cloud_track_reset()
                res = timed({"flags=0": lambda: e.set_obstacles_from_depth(ims, cams, spec, track=track),
                             f"flags={a.ab_flags}": lambda: e_ab.set_obstacles_from_depth(ims, cams, spec, track=track)})
                report(config, "ab-" + where, res)
                assert np.array_equal(e.get_obstacles().view(np.uint32), e_ab.get_obstacles().view(np.uint32))
                assert np.array_equal(e.get_obstacle_motion()[0].view(np.uint32), e_ab.get_obstacle_motion()[0].view(np.uint32))
    say(json.dumps(dict(study="depth_cloud_cost", dims=DIMS, voxel=VOXEL, dt_frame=DT_FRAME, ab_flags=a.ab_flags, rows=rows)))
    e.close()
    if e_ab is not None:
        e_ab.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
