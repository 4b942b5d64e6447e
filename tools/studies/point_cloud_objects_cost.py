"""What the objects scene update from a depth point cloud costs (omds_set_obstacles_from_cloud_objects) beside the tracked one of the
same build (omds_set_obstacles_from_cloud_tracked, whose launches the objects call leaves as they are), on the scene and with the
protocol of point_cloud_flow_cost.py (EXPERIMENTS.md R18): P = 131 072 points in a 64 x 64 x 48 grid of 2.5 cm cells on a 1024 x 32
context that holds the Franka network.  Host clock around the synchronous call; per configuration the two legs alternate call by call
(objects, tracked, objects, ...), five warm-up calls per leg, then the median of 50 with its spread.  The legs run on TWO contexts
of the one process: a plain tracked call invalidates the component table, so on one context the objects call would never match.
  pair   : static (the same cloud every frame) or moving (frames alternate between the cloud and the cloud with its shelf half one
           cell further in x)
  filter : without, or with the self-filter at FRANKA_Q0 (margin 0.03)
  link   : 1, 2 (26 or 124 neighbours, half of them visited per sphere)
  input  : a host array, or a device-resident tensor

    python tools/studies/point_cloud_objects_cost.py [--calls 50]

--quality needs no GPU: the host definitions (omds_point_cloud_flow, omds_point_cloud_object_flow) on R18's prototype scene -- the
camera-side half of a sphere shell of radius 0.15 m, sampled afresh in every frame with 2 mm noise, 2.5 cm cells, min_points 2 -- moved
by 0.3 / 1.0 / 2.4 cells towards the camera, across its view and diagonally: the mean estimated velocity projected on the true
direction, as a fraction of the true speed, for the per-cell flow and for the object estimate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from optimalmodulationds_amd.engine import (cloud_object_spec, cloud_spec, cloud_track_spec, point_cloud_flow,  # noqa: E402
                                            point_cloud_object_flow)

F32 = np.float32


def quality(seeds=5):
    voxel, radius, noise, n = 0.025, 0.15, 0.002, 6000
    spec = cloud_spec((-0.4, -0.4, 0.0), voxel, (32, 32, 32), min_points=2)
    centre = np.array([0.0, 0.0, 0.4])
    rows = []
    print(f"{'direction':12s} {'shift':>5s} | {'per-cell flow':>13s} {'object':>7s} | spheres objects matched")
    for name, d in (("to camera", (0.0, 0.0, -1.0)), ("across", (1.0, 0.0, 0.0)), ("diagonal", (0.6, 0.0, -0.8))):
        d = np.asarray(d)
        for shift in (0.3, 1.0, 2.4):
            flow_r, obj_r, counts = [], [], None
            for seed in range(seeds):
                rng = np.random.RandomState(100 + seed)

                def frame(c):
                    u = rng.standard_normal((n, 3))
                    u /= np.linalg.norm(u, axis=1, keepdims=True)
                    u[:, 2] = -np.abs(u[:, 2])                    # the half that faces a camera at z = -inf
                    return (c + radius * u + noise * rng.standard_normal((n, 3))).astype(F32)

                prev, now = frame(centre), frame(centre + shift * voxel * d)
                track = cloud_track_spec(3, 1.0)
                _, v_flow, _ = point_cloud_flow(prev, now, spec, track)
                sph, v_obj, _, flag, _, n_obj, n_acc = point_cloud_object_flow(prev, now, spec, track, cloud_object_spec(1, 4))
                true = shift * voxel
                flow_r.append(float((v_flow @ d).mean() / true))
                obj_r.append(float((v_obj @ d).mean() / true))
                counts = (len(sph), n_obj, n_acc, int(flag.sum()))
            rows.append(dict(direction=name, shift_cells=shift, flow_ratio=float(np.mean(flow_r)), flow_min=min(flow_r), flow_max=max(flow_r),
                             object_ratio=float(np.mean(obj_r)), object_min=min(obj_r), object_max=max(obj_r), spheres=counts[0],
                             objects=counts[1], objects_matched=counts[2]))
            print(f"{name:12s} {shift:5.1f} | {np.mean(flow_r):13.2f} {np.mean(obj_r):7.2f} | {counts[0]} {counts[1]} {counts[2]}")
    print(json.dumps(dict(study="point_cloud_objects_quality", voxel=voxel, radius=radius, noise=noise, points=n, seeds=seeds, rows=rows)))


def cost(calls):
    import torch
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import Engine
    from point_cloud_flow_cost import DIMS, DT_FRAME, MARGIN, ORIGIN, P, VOXEL, make_cloud
    still_cloud, q0 = make_cloud()
    moved_cloud, _ = make_cloud((VOXEL, 0.0, 0.0))
    z = np.load(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
    n = len([k for k in z.files if k.startswith("W")])
    engines = []
    for _ in range(2):
        e = Engine(7, 1024, 32, 5, max_obs=2 * scenes.shelf_scene().shape[0])
        e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
        e.params.ignored_links = 0b111
        e.push_params()
        engines.append(e)
    eo, et = engines
    spec = cloud_spec(ORIGIN, VOXEL, DIMS, max_spheres=65536, self_margin=MARGIN)
    dev = f"cuda:{eo.device}"
    frames = {"host": (still_cloud, moved_cloud), "device": (torch.from_numpy(still_cloud).to(dev), torch.from_numpy(moved_cloud).to(dev))}
    track = cloud_track_spec(2, DT_FRAME)
    rows = []
    print(f"{'input':6s} {'pair':6s} {'filter':6s} {'link':>4s} | {'objects ms':>10s} {'min':>7s} {'max':>7s} | {'tracked':>9s} {'min':>7s} {'max':>7s} | "
          f"{'ratio':>5s} {'+ ms':>6s} | spheres matched objects obj-matched obj-spheres moving mode")
    for where in ("host", "device"):
        for pair in ("static", "moving"):
            for filt in (False, True):
                for link in (1, 2):
                    obj = cloud_object_spec(link, 4)
                    q = q0 if filt else None
                    eo.cloud_track_reset()
                    et.cloud_track_reset()
                    ms = {"objects": [], "tracked": []}
                    for it in range(5 + calls):
                        pts = frames[where][it % 2 if pair == "moving" else 0]
                        t0 = time.perf_counter()
                        got = eo.set_obstacles_from_cloud_objects(pts, spec, track, obj, q=q)
                        t1 = time.perf_counter()
                        et.set_obstacles_from_cloud_tracked(pts, spec, track, q=q)
                        t2 = time.perf_counter()
                        if it >= 5:
                            ms["objects"].append((t1 - t0) * 1e3)
                            ms["tracked"].append((t2 - t1) * 1e3)
                    vel, mode, flags = eo.get_obstacle_motion()[0], eo.get_obstacle_horizon()[1], eo.cloud_objects()[1]
                    ob, tr = np.asarray(ms["objects"]), np.asarray(ms["tracked"])
                    row = dict(input=where, pair=pair, filter=filt, link=link, objects_ms=float(np.median(ob)), objects_min=float(ob.min()),
                               objects_max=float(ob.max()), tracked_ms=float(np.median(tr)), tracked_min=float(tr.min()), tracked_max=float(tr.max()),
                               calls=int(ob.size), n_spheres=got[0], n_occupied=got[1], n_matched=got[2], n_objects=got[3], n_objects_matched=got[4],
                               n_object_spheres=int(flags.sum()), n_moving=int((vel != 0).any(1).sum()), horizon_mode=int(mode))
                    rows.append(row)
                    print(f"{where:6s} {pair:6s} {str(filt):6s} {link:4d} | {row['objects_ms']:10.3f} {row['objects_min']:7.3f} {row['objects_max']:7.3f} | "
                          f"{row['tracked_ms']:9.3f} {row['tracked_min']:7.3f} {row['tracked_max']:7.3f} | {row['objects_ms'] / row['tracked_ms']:5.2f} "
                          f"{row['objects_ms'] - row['tracked_ms']:6.3f} | {got[0]} {got[2]} {got[3]} {got[4]} {row['n_object_spheres']} {row['n_moving']} {mode}",
                          flush=True)
    print(json.dumps(dict(study="point_cloud_objects_cost", points=P, dims=DIMS, voxel=VOXEL, dt_frame=DT_FRAME, reach=2, min_cells=4, rows=rows)))
    eo.close()
    et.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--quality", action="store_true")
    a = ap.parse_args()
    quality() if a.quality else cost(a.calls)
