"""What an obstacle horizon costs (omds_set_obstacle_motion, csrc/obstacle_horizon.hip): Franka shelf 1024 x 32, one process, one
context.  Static and motion propagates in interleaved 20-iteration blocks, ten blocks each, host clock around calls that end in a
stream synchronise; and the rebuild of the tables alone (H2D copy of the velocities + k_obstacle_horizon_features + synchronise),
which a planner that streams new obstacles pays once per iteration.  Steps >= 2 read another slab of the same size, so the
per-step kernels should not move.  python tools/studies/obstacle_horizon_cost.py"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from optimalmodulationds_amd import scenes  # noqa: E402
from optimalmodulationds_amd.engine import Engine  # noqa: E402

N, H, K, BLOCKS, ITERS = 1024, 32, 10, 10, 20
z = np.load(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
n = len([k for k in z.files if k.startswith("W")])
obs = scenes.shelf_scene()
vel = np.random.RandomState(3).uniform(-0.2, 0.2, (obs.shape[0], 3)).astype(np.float32)
q0 = np.asarray(scenes.FRANKA_Q0, np.float32)
rng = np.random.RandomState(0)
mu_c = (q0 + 0.2 * rng.standard_normal((K, 7))).astype(np.float32)
sg_c, al_c = np.ones(K, np.float32), rng.standard_normal((K, 7)).astype(np.float32)

e = Engine(7, N, H, 5, max_obs=2 * obs.shape[0])
e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
e.set_obstacles(obs)
e.params.dt, e.params.dst_thr, e.params.ignored_links = 0.5, 0.01, 0b111
e.push_params()
e.set_ds(scenes.FRANKA_QF)
e.set_screening(0)


def block(moving, seed0):
    """ms per propagate over one block of ITERS iterations (sample_policy + propagate, the propagate synchronises)."""
    e.set_obstacle_motion(vel if moving else None)
    e.sample_policy(mu_c, sg_c, al_c, 0.0, 0.0, 3.0, K, seed=seed0)
    e.propagate(q0)                                   # builds the tables of a motion block; not timed
    t0 = time.perf_counter()
    for it in range(ITERS):
        e.sample_policy(mu_c, sg_c, al_c, 0.0, 0.0, 3.0, K, seed=seed0 + 1 + it)
        e.propagate(q0)
    return (time.perf_counter() - t0) * 1e3 / ITERS


for w in range(3):                                    # warm-up: both shapes, code objects loaded
    block(False, 1000 + 100 * w)
    block(True, 2000 + 100 * w)
ms = {False: [], True: []}
for b in range(BLOCKS):
    for moving in (False, True):
        ms[moving].append(block(moving, 100 * (2 * b + moving)))
rebuild = []
mode = C.c_int32()
for it in range(200):
    e.set_obstacle_motion(vel)                        # marks the tables stale (host copy of the velocities)
    t0 = time.perf_counter()
    e._ck(e.lib.omds_get_obstacle_horizon(e.h, None, C.byref(mode)))   # NULL: rebuild + synchronise, no copy back
    rebuild.append((time.perf_counter() - t0) * 1e3)
e.close()
for moving, name in ((False, "static"), (True, "motion")):
    a = np.asarray(ms[moving])
    print(f"{name}: ms per propagate, median of {BLOCKS} x {ITERS}-iteration blocks {np.median(a):.4f}  min {a.min():.4f}  max {a.max():.4f}  "
          f"-> {N * H / np.median(a) / 1e3:.4f} M rollout-steps/s")
r = np.asarray(rebuild[20:])
print(f"rebuild alone (H = {H}, O = {obs.shape[0]}; copy + launch + synchronise, host clock): median {np.median(r) * 1e3:.1f} us  "
      f"min {r.min() * 1e3:.1f}  max {r.max() * 1e3:.1f} over {r.size} calls")
print(f"motion / static (medians): {np.median(ms[True]) / np.median(ms[False]):.4f}")
