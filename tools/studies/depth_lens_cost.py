"""What the lens of a depth camera costs (omds_set_depth_lenses in front of the depth routes) beside the pinhole call on the same image
and beside the route a user would otherwise take, on one 640 x 480 U16 image from host memory: R20's scene (the shelf's spheres, balls
along the arm, clutter, a back wall) seen through a plumb-bob lens (-0.3, 0.1, 1e-3, -5e-4; fx = fy = 600) from R20's first camera,
into R17's grid (64 x 64 x 48 cells of 2.5 cm) on a 1024 x 32 context.  EXPERIMENTS.md R33.
R17's protocol: a host clock around the synchronous call, the legs alternating call by call, five warm-up calls per leg, the median
of --calls with its minimum and maximum.  Run the whole command twice: the spread between the runs is part of the result.
  pinhole / lens           the plain depth call without and with the lens (the ray table cached in the context)
  ... filter, memory, memory tracked: the same pair on the filtered (radius 1), memory and memory-tracked routes
  lens rebuild             the lens call with cx moved by 2^-10 pixels every call: the table's key changes, k_depth_rays runs, its two
                           words come back -- the one-off build, every call (a group of its own: slot 0 holds one table)
  torch rays               the parent's device route with the lens: the image copied to the device, the deprojection as torch
                           operations on the cached undistorted rays, the cloud call on the device tensor
  torch undistort          ... with the 20 rounds of the inverse as torch operations in every call as well (a camera whose
                           intrinsics change)
  --pinhole-only [--tree DIR]: the four pinhole legs alone, on the pinhole rendering of the scene, with the package of the checkout
                           DIR (default: this one) and nothing of the lens interface -- run in a build of the parent commit and in
                           this build, alternating, it shows what the unchanged routes cost before and after.

    python tools/studies/depth_lens_cost.py [--calls 200] [--out profiles/r33_depth_lens_cost.txt] [--pinhole-only [--tree DIR]]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32, F64 = np.float32, np.float64
PLUMB = (-0.3, 0.1, 1e-3, -5e-4)
FILTER = dict(radius=1, min_support=4, edge_abs=0.01, edge_rel=0.01)


def render_through(cam, ab, spheres, wall_x):
    """R20's render along the rays ab [H * W, 2] of the lens instead of the pinhole ones; a pixel without a ray: no return"""
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    ab = ab.astype(F64).reshape(cam.height, cam.width, 2)
    ok = ~np.isnan(ab[..., 0])
    d = np.stack([np.where(ok, ab[..., 0], 0.0), np.where(ok, ab[..., 1], 0.0), np.ones(ok.shape)], -1) @ p[:, :3].T
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
    return np.clip(np.round(np.where(np.isfinite(best) & ok, best, 0.0) * 1000.0), 0, 65535).astype(np.uint16)


def torch_lens_route(r20, ab, cam, lens, dev):
    """R20's torch route along the rays ab of a lens: cached (the table uploaded once), or undistorted in every call"""

    class TorchLensRoute(r20.TorchRoute):
        def __init__(self):
            super().__init__([cam], dev)
            torch = self.torch
            rays = ab.reshape(cam.height, cam.width, 2)
            self.x0, self.y0 = self.cams[0][0], self.cams[0][1]
            self.cams[0] = (torch.from_numpy(rays[..., 0].copy()).to(dev), torch.from_numpy(rays[..., 1].copy()).to(dev)) + self.cams[0][2:]
            self.k = [float(v) for v in lens.k]
            self.iters = 20

        def undistort(self):
            k1, k2, p1, p2, k3, k4, k5, k6 = self.k
            x0, y0 = self.x0, self.y0
            x, y = x0, y0
            for _ in range(self.iters):
                r2 = x * x + y * y
                ic = (1 + r2 * (k4 + r2 * (k5 + r2 * k6))) / (1 + r2 * (k1 + r2 * (k2 + r2 * k3)))
                dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
                dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
                x, y = (x0 - dx) * ic, (y0 - dy) * ic
            return x, y

        def points_undistorting(self, t16):
            cached = self.cams[0]
            self.cams[0] = self.undistort() + cached[2:]
            try:
                return self.points([t16])
            finally:
                self.cams[0] = cached

    return TorchLensRoute()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_depth_lens_cost.txt"))
    ap.add_argument("--pinhole-only", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, os.path.join(tree, "tools", "studies"))
    import depth_cloud_cost as r20      # puts its own checkout in front of the path: the package below is that checkout's
    from optimalmodulationds_amd import engine as E, scenes
    assert os.path.abspath(E.__file__).startswith(tree + os.sep), (E.__file__, tree)
    Engine, cloud_spec, cloud_track_spec, depth_camera, depth_filter_spec, depth_points, scene_memory_spec = (
        E.Engine, E.cloud_spec, E.cloud_track_spec, E.depth_camera, E.depth_filter_spec, E.depth_points, E.scene_memory_spec)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    z = np.load(os.path.join(tree, "tests", "golden", "weights", "franka.npz"))
    n = len([k for k in z.files if k.startswith("W")])
    e = Engine(7, 1024, 32, 5, max_obs=2 * scenes.shelf_scene().shape[0])
    e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
    dev = f"cuda:{e.device}"
    spec = cloud_spec(r20.ORIGIN, r20.VOXEL, r20.DIMS, max_spheres=65536)
    track, mem = cloud_track_spec(2, r20.DT_FRAME), scene_memory_spec(5)
    pose = r20.look_at(r20.EYES[0], r20.TARGET)
    cam = depth_camera(640, 480, 600.0, 600.0, 319.5, 239.5, pose, 0, 0.001, 0.2, 6.0)

    def flat(out):
        return [int(g) for g in np.hstack([np.ravel(o) for o in out])]

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
            say(f"{name:24s} | {np.median(t):8.4f} {t.min():8.4f} {t.max():8.4f} | {flat(last[name])}")
        return {k: float(np.median(v)) for k, v in ms.items()}

    if a.pinhole_only:
        img = r20.render(cam, r20.scene_spheres(), 1.15)
        say(f"# pinhole legs only, the package of {tree}: one 640 x 480 U16 image, {depth_points(img, cam)[1]} points; {a.calls} calls per leg, ms")

        def filtered(f, call):
            def run():
                e.set_depth_filter(None if f is None else depth_filter_spec(**f))
                return call()
            return run

        timed({"pinhole": filtered(None, lambda: e.set_obstacles_from_depth([img], [cam], spec)),
               "pinhole filter": filtered(FILTER, lambda: e.set_obstacles_from_depth([img], [cam], spec))})
        e.set_depth_filter(None)
        timed({"pinhole memory": lambda: e.set_obstacles_from_depth_memory([img], [cam], spec, mem)})
        e.scene_memory_reset()
        timed({"pinhole memory tracked": lambda: e.set_obstacles_from_depth_memory_tracked([img], [cam], spec, mem, track)})
        e.close()
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    lens = E.depth_lens(PLUMB)
    ab, r2_max, n_invalid = E.depth_lens_rays(cam, lens)
    img = render_through(cam, ab, r20.scene_spheres(), 1.15)
    route = torch_lens_route(r20, ab, cam, lens, dev)
    torch.cuda.synchronize()
    say(f"one 640 x 480 U16 image through the plumb-bob lens {PLUMB}: {n_invalid} pixels without a ray, r2_max {r2_max:.4f}; "
        f"{depth_points(img, cam, lens=lens)[1]} points; grid {r20.DIMS} x {r20.VOXEL} m; {a.calls} calls per leg, ms")

    def under(lenses, filt, call):
        def run():
            e.set_depth_lenses(lenses)
            e.set_depth_filter(None if filt is None else depth_filter_spec(**filt))
            return call()
        return run

    moved = [0]

    def rebuild():
        moved[0] += 1
        c = depth_camera(640, 480, 600.0, 600.0, 319.5 + (moved[0] % 1024) * 2.0 ** -10, 239.5, pose, 0, 0.001, 0.2, 6.0)
        e.set_depth_lenses([lens])
        e.set_depth_filter(None)
        return e.set_obstacles_from_depth([img], [c], spec)

    say(f"{'leg':24s} | {'median':>8s} {'min':>8s} {'max':>8s} | counts")
    med = {}
    med.update(timed({
        "pinhole": under(None, None, lambda: e.set_obstacles_from_depth([img], [cam], spec)),
        "lens": under([lens], None, lambda: e.set_obstacles_from_depth([img], [cam], spec)),
        "torch rays": lambda: e.set_obstacles_from_cloud(route.points(route.upload([img])), spec),
        "torch undistort": lambda: e.set_obstacles_from_cloud(route.points_undistorting(route.upload([img])[0]), spec),
    }))
    med.update(timed({"lens rebuild": rebuild}))      # alone: in a group it would also change the key under the "lens" leg's table
    med.update(timed({
        "pinhole filter": under(None, FILTER, lambda: e.set_obstacles_from_depth([img], [cam], spec)),
        "lens filter": under([lens], FILTER, lambda: e.set_obstacles_from_depth([img], [cam], spec)),
    }))
    for name, lenses in (("pinhole", None), ("lens", [lens])):      # one after the other: the two would share the stored memory
        e.scene_memory_reset()
        med.update(timed({f"{name} memory": under(lenses, None, lambda: e.set_obstacles_from_depth_memory([img], [cam], spec, mem))}))
    for name, lenses in (("pinhole", None), ("lens", [lens])):
        e.scene_memory_reset()
        e.cloud_track_reset()
        med.update(timed({f"{name} memory tracked": under(lenses, None,
                                                          lambda: e.set_obstacles_from_depth_memory_tracked([img], [cam], spec, mem, track))}))
    for route_name in ("", " filter", " memory", " memory tracked"):
        p, l = med["pinhole" + route_name], med["lens" + route_name]
        say(f"{('plain' if not route_name else route_name.strip()):15s}: lens {l:.4f} ms = pinhole {p:.4f} {l - p:+.4f}")
    say(f"one-off table build: lens rebuild {med['lens rebuild']:.4f} ms = lens {med['lens']:.4f} {med['lens rebuild'] - med['lens']:+.4f}")
    for name in ("torch rays", "torch undistort"):
        say(f"{name}: {med[name]:.4f} ms = {med[name] / med['lens']:.2f} x the lens call ({med[name] - med['lens']:+.4f} ms)")
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
