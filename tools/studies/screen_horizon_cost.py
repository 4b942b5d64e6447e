"""What a screened propagate under an obstacle horizon costs (omds_set_screening_horizon): Franka shelf 1024 x 32, K = 10, velocities
uniform in +-0.2 m/s.  Whole planner iterations (sample_policy -> propagate -> cost -> weighted update), host clock (every iteration
ends in a synchronise), three warm-up blocks per leg, then blocks of 20 iterations; the legs alternate inside one process, one
context each, and the median over the blocks is reported with its spread:
  (a) the all-fp32 step with the horizon  -- what a context without omds_set_screening_horizon runs for the same request,
  (b) screened with the horizon,
  (c) screened, static scene.
Then the latency of the FIRST screened propagates of a fresh context, under a horizon (the three-slab calibration) and static.

    python tools/studies/screen_horizon_cost.py [--blocks 10] [--legs abc] [--trace b]

--legs a runs on a checkout without the switch too (the parent commit); --trace b runs leg (b) alone, without timing, for a
kernel trace taken from outside (rocprofv3 --kernel-trace --stats -- python tools/studies/screen_horizon_cost.py --trace b)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from optimalmodulationds_amd import scenes  # noqa: E402
from optimalmodulationds_amd.engine import Engine  # noqa: E402

N, H, K, ITERS = 1024, 32, 10, 20
z = np.load(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
n = len([k for k in z.files if k.startswith("W")])
obs = scenes.shelf_scene()
vel = np.random.RandomState(3).uniform(-0.2, 0.2, (obs.shape[0], 3)).astype(np.float32)
q0, qf = np.asarray(scenes.FRANKA_Q0, np.float32), np.asarray(scenes.FRANKA_QF, np.float32)
LEGS = {"a": ("fp32 step, motion horizon", 0, True), "b": ("screened, motion horizon", 1, True), "c": ("screened, static scene", 1, False)}


def make(screen, moving):
    from optimalmodulationds_amd.cost import FRANKA_Q_MAX, FRANKA_Q_MIN
    e = Engine(7, N, H, 5, max_obs=2 * obs.shape[0])
    e.set_mlp([z[f"W{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
    e.set_obstacles(obs)
    e.params.dt, e.params.dst_thr, e.params.ignored_links = 0.5, 0.01, 0b111
    e.push_params()
    e.set_ds(qf)
    e.set_cost(scenes.franka_dh_params(), np.array(FRANKA_Q_MIN, np.float32), np.array(FRANKA_Q_MAX, np.float32))
    e.set_screening(screen)
    if screen and moving:
        e.set_screening_horizon(True)
    if moving:
        e.set_obstacle_motion(vel)
    return e


class Leg:
    """One context and the policy it carries from block to block (a block starts from the same means, like bench.py's)."""

    def __init__(self, key):
        self.name, screen, moving = LEGS[key]
        self.e = make(screen, moving)
        rng = np.random.RandomState(0)
        s = (np.arange(K) + 0.5) / K
        self.mu0 = (q0 + s[:, None] * (qf - q0) + 0.15 * rng.standard_normal((K, 7))).astype(np.float32)
        self.al0 = rng.standard_normal((K, 7)).astype(np.float32)
        self.ms = []

    def block(self, seed0, timed=True):
        e = self.e
        mu_c, sg_c, al_c = self.mu0.copy(), np.ones(K, np.float32), self.al0.copy()
        q = q0.copy()
        t0 = time.perf_counter()
        for it in range(ITERS):
            e.sample_policy(mu_c, sg_c, al_c, 0.0, 0.0, 3.0, K, seed=seed0 + it)
            e.propagate(q)
            e.cost(fetch=False)
            mu_c, sg_c, al_c, _, qd_w, _, _ = e.weighted_update_sharded(0.1, 0.1, mu_c, sg_c, al_c)
            q = (q + 0.05 * qd_w).astype(np.float32)
        if timed:
            self.ms.append((time.perf_counter() - t0) * 1e3 / ITERS)


def first_propagates(moving):
    e = make(1, moving)
    ts = []
    for it in range(6):
        e.sample_policy(None, None, None, 0, 0, 0, 0, seed=it)
        t0 = time.perf_counter()
        e.propagate(q0)
        ts.append((time.perf_counter() - t0) * 1e3)
    st = e.screen_stats()
    e.close()
    return ts, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--trace", default=None, help="run this leg alone for 3 untimed blocks (for a kernel trace taken from outside)")
    a = ap.parse_args()
    if a.trace:
        leg = Leg(a.trace)
        for w in range(3):
            leg.block(1000 * w, timed=False)
        print(leg.name, leg.e.screen_stats())
        leg.e.close()
        return
    legs = [Leg(k) for k in a.legs]
    for w in range(3):
        for i, leg in enumerate(legs):
            leg.block(100000 + 1000 * (3 * w + i), timed=False)
    for b in range(a.blocks):
        for i, leg in enumerate(legs):
            leg.block(1000 * (len(legs) * b + i))
    med = {}
    for key, leg in zip(a.legs, legs):
        x = np.asarray(leg.ms)
        med[key] = float(np.median(x))
        st = leg.e.screen_stats()
        print(f"({key}) {leg.name}: ms per iteration, median of {x.size} x {ITERS}-iteration blocks {np.median(x):.3f}  min {x.min():.3f}  max {x.max():.3f}"
              f"  -> {N * H / np.median(x) / 1e3:.3f} M rollout-steps/s   [active {st['active']}  eps {st['eps']:.4g}  cand/step "
              f"{st['candidates_per_rollout_step']:.2f}  fallbacks {st['fallbacks']}  calibrations {st['calibrations']}]")
        leg.e.close()
    if "a" in med and "b" in med:
        print(f"(a) / (b): {med['a'] / med['b']:.2f} x")
    if "b" in med and "c" in med:
        print(f"(b) / (c): {med['b'] / med['c']:.4f}")
    if "b" in a.legs:
        for moving, name in ((True, "under a motion horizon (three-slab calibration)"), (False, "static (one slab)")):
            ts, st = first_propagates(moving)
            print(f"first screened propagates of a fresh context {name}: ms {[round(t, 2) for t in ts]}  calibrations {st['calibrations']}  "
                  f"reorders {st['unit_reorders']}")


if __name__ == "__main__":
    main()
