"""What the tracked scene update from a depth point cloud costs (omds_set_obstacles_from_cloud_tracked) beside the untracked one of
the same build (omds_set_obstacles_from_cloud), on the scene of point_cloud_cost.py (EXPERIMENTS.md R17): P = 131 072 points in a
64 x 64 x 48 grid of 2.5 cm cells -- half on the shelf's spheres, a quarter around the arm at FRANKA_Q0, a quarter clutter -- on a
1024 x 32 context that holds the Franka network.  Host clock around the synchronous call; per configuration the two legs alternate
call by call (tracked, untracked, tracked, ...), five warm-up calls per leg, then the median of 50 with its spread.
  pair   : static (the same cloud every frame: every sphere finds itself, d2 = 0, the horizon stays cleared) or moving (frames
           alternate between the cloud and the cloud with its shelf half one cell further in x: a motion horizon every frame)
  filter : without, or with the self-filter at FRANKA_Q0 (margin 0.03)
  reach  : 1, 2, 4 cells (windows of 27, 125, 729 cells)
  input  : a host array, or a device-resident tensor
The untracked call between two tracked ones leaves the stored frame alone, so every tracked call is matched against the tracked
call before it.

    python tools/studies/point_cloud_flow_cost.py [--calls 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from optimalmodulationds_amd import scenes  # noqa: E402
from optimalmodulationds_amd.engine import Engine, cloud_spec, cloud_track_spec  # noqa: E402
from oracle import omds_oracle as orc  # noqa: E402

P, DIMS, VOXEL, ORIGIN, MARGIN, DT_FRAME = 131072, (64, 64, 48), 0.025, (-0.4, -0.8, 0.0), 0.03, 1.0 / 30.0
F32 = np.float32


def make_cloud(shelf_shift=(0.0, 0.0, 0.0), seed=0):
    """point_cloud_cost.make_cloud (the same draws in the same order), its shelf half moved by ``shelf_shift`` metres"""
    rng = np.random.RandomState(seed)
    obs = scenes.shelf_scene()
    q0 = np.asarray(scenes.FRANKA_Q0, F32)
    n_shelf, n_arm = P // 2, P // 4
    u = rng.standard_normal((n_shelf, 3))
    o = obs[rng.randint(0, obs.shape[0], n_shelf)]
    shelf = o[:, :3] + o[:, 3:] * u / np.linalg.norm(u, axis=1, keepdims=True) + np.asarray(shelf_shift)
    ends = np.concatenate([np.zeros((1, 3)), orc.link_endpoints(q0, scenes.franka_dh_params())])
    seg = rng.randint(0, len(ends) - 1, n_arm)
    s = rng.uniform(0, 1, (n_arm, 1))
    arm = ends[seg] * (1 - s) + ends[seg + 1] * s + 0.04 * rng.standard_normal((n_arm, 3))
    lo, ext = np.array(ORIGIN), np.array(DIMS) * VOXEL
    clutter = lo - 0.1 + rng.uniform(0, 1, (P - n_shelf - n_arm, 3)) * (ext + 0.2)      # some of it outside the box
    return np.ascontiguousarray(rng.permutation(np.concatenate([shelf, arm, clutter])), F32), q0


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    still_cloud, q0 = make_cloud()
    moved_cloud, _ = make_cloud((VOXEL, 0.0, 0.0))
    z = np.load(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
    n = len([k for k in z.files if k.startswith("W")])
    e = Engine(7, 1024, 32, 5, max_obs=2 * scenes.shelf_scene().shape[0])
    e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
    e.params.ignored_links = 0b111
    e.push_params()
    spec = cloud_spec(ORIGIN, VOXEL, DIMS, max_spheres=65536, self_margin=MARGIN)
    dev = f"cuda:{e.device}"
    frames = {"host": (still_cloud, moved_cloud), "device": (torch.from_numpy(still_cloud).to(dev), torch.from_numpy(moved_cloud).to(dev))}
    rows = []
    print(f"{'input':6s} {'pair':6s} {'filter':6s} {'reach':>5s} | {'tracked ms':>10s} {'min':>7s} {'max':>7s} | {'untracked':>9s} {'min':>7s} {'max':>7s} | "
          f"{'ratio':>5s} {'+ ms':>6s} | spheres matched moving mode")
    for where in ("host", "device"):
        for pair in ("static", "moving"):
            for filt in (False, True):
                for reach in (1, 2, 4):
                    track = cloud_track_spec(reach, DT_FRAME)
                    q = q0 if filt else None
                    e.cloud_track_reset()
                    ms = {"tracked": [], "untracked": []}
                    for it in range(5 + a.calls):
                        pts = frames[where][it % 2 if pair == "moving" else 0]
                        t0 = time.perf_counter()
                        got = e.set_obstacles_from_cloud_tracked(pts, spec, track, q=q)
                        t1 = time.perf_counter()
                        if it == 4 + a.calls:      # what the last tracked call left, read between the two windows
                            vel, mode = e.get_obstacle_motion()[0], e.get_obstacle_horizon()[1]
                        t2 = time.perf_counter()
                        e.set_obstacles_from_cloud(pts, spec, q=q)
                        t3 = time.perf_counter()
                        if it >= 5:
                            ms["tracked"].append((t1 - t0) * 1e3)
                            ms["untracked"].append((t3 - t2) * 1e3)
                    tr, un = np.asarray(ms["tracked"]), np.asarray(ms["untracked"])
                    row = dict(input=where, pair=pair, filter=filt, reach=reach, tracked_ms=float(np.median(tr)), tracked_min=float(tr.min()),
                               tracked_max=float(tr.max()), untracked_ms=float(np.median(un)), untracked_min=float(un.min()), untracked_max=float(un.max()),
                               calls=int(tr.size), n_spheres=int(got[0]), n_occupied=int(got[1]), n_matched=int(got[2]),
                               n_moving=int((vel != 0).any(1).sum()), horizon_mode=int(mode))
                    rows.append(row)
                    print(f"{where:6s} {pair:6s} {str(filt):6s} {reach:5d} | {row['tracked_ms']:10.3f} {row['tracked_min']:7.3f} {row['tracked_max']:7.3f} | "
                          f"{row['untracked_ms']:9.3f} {row['untracked_min']:7.3f} {row['untracked_max']:7.3f} | {row['tracked_ms'] / row['untracked_ms']:5.2f} "
                          f"{row['tracked_ms'] - row['untracked_ms']:6.3f} | {got[0]} {got[2]} {row['n_moving']} {mode}")
    print(json.dumps(dict(study="point_cloud_flow_cost", points=P, dims=DIMS, voxel=VOXEL, dt_frame=DT_FRAME, rows=rows)))
    e.close()


if __name__ == "__main__":
    main()
