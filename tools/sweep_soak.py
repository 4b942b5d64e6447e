#!/usr/bin/env python3
"""Exhaustive check of the screening assumption (omds.h, "Screening of pass 1") over >= 1e10 (rollout, obstacle)
pairs: every horizon step of every propagate SWEPT -- all N x O pairs in fp32 (k_pass1) beside their fp16 screening values --
and the difference Da - D of the pairs that were NOT candidates (never re-evaluated: the population the bound eps is about)
counted into histograms on the device (omds_set_screening_sweep(1, all_steps=1), omds_screen_sweep_hist).

Legs: the shelf (static; moving like bench.py's dynamic workload), every streamed scene of the reference's obstacle streamers
(scenes.STREAMED_SCENES), start states uniform in the joint box (per-rollout starts), the tanh 256x3 and the skip-connection
networks.  Prints a report (committed as profiles/r04_screen_error_hist.txt):

    python tools/sweep_soak.py [--pairs 1e10] > profiles/r04_screen_error_hist.txt

--legs moving: the MOVING-SCENE legs instead -- obstacle velocities (a motion horizon: every step sees its own slab) with screening
over the horizon (omds_set_screening_horizon), the scene advanced by v dt from iteration to iteration; the same with the moving
frame; the caller's own table with radii growing over the horizon; the tanh and skip-connection networks.  Sized to a few minutes:

    python tools/sweep_soak.py --legs moving --pairs 3e10 > profiles/r14_screen_horizon_error_hist.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_weights(kind):
    z = np.load(os.path.join(ROOT, "tests", "golden", "weights", kind + ".npz"))
    nl = len([k for k in z.files if k.startswith("W")])
    skips = tuple(int(s) for s in z["skip_after"]) if "skip_after" in z.files else ()
    return [z[f"W{i}"] for i in range(nl)], [z[f"b{i}"] for i in range(nl)], skips


def make_engine(kind, N, H, obs, act="relu"):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.cost import FRANKA_Q_MAX, FRANKA_Q_MIN
    from optimalmodulationds_amd.engine import Engine
    W, b, skips = load_weights(kind)
    e = Engine(7, N, H, 5, max_obs=max(64, obs.shape[0]))
    e.set_mlp(W, b, act=act, skip_after=skips)
    e.set_obstacles(obs)
    e.params.dt, e.params.dst_thr, e.params.ignored_links = 0.5, 0.01, 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_cost(scenes.franka_dh_params(), np.array(FRANKA_Q_MIN, np.float32), np.array(FRANKA_Q_MAX, np.float32))
    e.set_screening(1)
    e.set_screening_sweep(1, all_steps=True)
    return e


def run_leg(name, e, n_iter, obs_of=None, uniform_starts=False, seed=0, horizon_of=None):
    """n_iter planner iterations (sample + propagate + cost + update) with every step swept; returns the leg's statistics.
    horizon_of(e, it): sets the iteration's scene AND its obstacle horizon (set_obstacles clears the previous one)."""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.cost import FRANKA_Q_MAX, FRANKA_Q_MIN
    rng = np.random.RandomState(1000 + seed)
    q0, qf = scenes.FRANKA_Q0, scenes.FRANKA_QF
    K = 10
    s = (np.arange(K) + 0.5) / K
    mu_c = (q0 + s[:, None] * (qf - q0) + 0.15 * rng.standard_normal((K, 7))).astype(np.float32)
    sg_c, al_c = np.ones(K, np.float32), rng.standard_normal((K, 7)).astype(np.float32)
    lo, hi = np.array(FRANKA_Q_MIN, np.float32), np.array(FRANKA_Q_MAX, np.float32)
    q = q0.copy()
    e.sweep_hist(reset=True)
    t0 = time.perf_counter()
    for it in range(n_iter):
        if obs_of is not None:
            e.set_obstacles(obs_of(it))
        if horizon_of is not None:
            horizon_of(e, it)
        e.sample_policy(mu_c, sg_c, al_c, 0.0, 0.0, 3.0, K, seed=77 * 1000003 + 131 * seed + it)
        if uniform_starts:
            e.propagate(rng.uniform(lo, hi, (e.N, 7)).astype(np.float32))
        else:
            e.propagate(q)
        e.cost(fetch=False)
        mu_c, sg_c, al_c, _, qd_w, _, _ = e.weighted_update_sharded(0.1, 0.1, mu_c, sg_c, al_c)
        q = (q + 0.05 * qd_w + 0.02 * rng.standard_normal(7)).astype(np.float32)
        if e.screen_stats()["suspended"]:    # three fallbacks in a row: what a driver would do -- calibrate again (counted in the report)
            e.set_screening(1, -1.0)
        if it % 16 == 15:      # a fresh start somewhere between the two ends, so that the legs do not sit in one region
            q = (q0 + rng.uniform(0, 1) * (qf - q0) + 0.3 * rng.standard_normal(7)).astype(np.float32)
            q = np.clip(q, lo, hi)
    hs, st = e.sweep_hist(), e.screen_stats()
    return dict(name=name, seconds=time.perf_counter() - t0, iterations=n_iter, hist=hs, stats=st)


def report(legs, out=sys.stdout):
    from optimalmodulationds_amd import _lib
    Lb, Rb = _lib.SWEEP_HIST_LOG_BINS, _lib.SWEEP_HIST_RATIO_BINS
    tot = dict(pairs=0, non_candidates=0, above_half_eps=0, above_eps=0, non_finite=0, steps=0)
    pos, neg, ratio = np.zeros(Lb, np.int64), np.zeros(Lb, np.int64), np.zeros(Rb, np.int64)
    w = out.write
    w("Screening error of the pairs the screened step does NOT re-evaluate, counted exhaustively (tools/sweep_soak.py)\n")
    w("x = Da - D: fp16 screening value minus fp32 pass-1 value of a (rollout, obstacle) pair that was not a candidate.\n")
    w("The selection rule (omds.h) is exact while every such x <= eps; a propagate is accepted only while the largest error it\n")
    w("measured stays <= eps / 2.  Every horizon step of every propagate below was swept: all N x O pairs in fp32.\n\n")
    w(f"{'leg':38s} {'iters':>5s} {'pairs':>14s} {'non-candidates':>15s} {'eps [m]':>10s} {'max x [m]':>10s} {'max x/eps':>9s} {'max|x| all':>10s} "
      f"{'> eps/2':>7s} {'> eps':>5s} {'nonfin':>6s} {'fallb. e/s/o':>12s} {'susp.':>5s} {'calib.':>6s} {'cand/step':>9s} {'s':>6s}\n")
    worst_ratio = 0.0
    for lg in legs:
        h, st = lg["hist"], lg["stats"]
        for k in tot:
            tot[k] += h[k]
        pos += h["pos"]; neg += h["neg"]; ratio += h["ratio"]
        r = h["max_pos"] / st["eps"] if st["eps"] > 0 else float("nan")
        worst_ratio = max(worst_ratio, r)
        fb = f"{st['fallbacks_by_error']}/{st['fallbacks_by_slack']}/{st['fallbacks_by_overflow']}"
        w(f"{lg['name']:38s} {lg['iterations']:5d} {h['pairs']:14d} {h['non_candidates']:15d} {st['eps']:10.3e} {h['max_pos']:10.3e} {r:9.3f} "
          f"{h['max_abs']:10.3e} {h['above_half_eps']:7d} {h['above_eps']:5d} {h['non_finite']:6d} {fb:>12s} {st['suspensions']:5d} {st['calibrations']:6d} "
          f"{st['candidates_per_rollout_step']:9.2f} {lg['seconds']:6.1f}\n")
    w("(fallb. e/s/o: propagates redone in fp32 because a measured error exceeded eps / 2, because a rollout's slack guard failed, because a\n"
      " candidate list outgrew its buffers; susp.: times screening was suspended after three in a row -- a suspended leg is unscreened, and unswept, from there on)\n")
    w(f"\nTOTAL: {tot['pairs']:.4e} pairs in {tot['steps']} swept steps, {tot['non_candidates']:.4e} of them not candidates; "
      f"above eps/2: {tot['above_half_eps']}, above eps: {tot['above_eps']}, non-finite: {tot['non_finite']}; largest x / eps of any leg: {worst_ratio:.3f}\n")
    w("\nDistribution of x over the non-candidates, all legs (log2 bins of |x| in metres; the network's outputs are <= ~1 m):\n")
    w(f"{'|x| from':>12s} {'to':>12s} {'x >= 0':>16s} {'x < 0':>16s}\n")
    for b in range(Lb):
        if pos[b] or neg[b]:
            lo_ = 0.0 if b == 0 else 2.0 ** (b - Lb)
            w(f"{lo_:12.3e} {2.0 ** (b + 1 - Lb):12.3e} {pos[b]:16d} {neg[b]:16d}\n")
    w("\nDistribution of x / eps for x > 0 (eps = the bound in use when the step was swept; a miss needs x / eps > 1):\n")
    w(f"{'from':>8s} {'to':>8s} {'pairs':>16s} {'survival P(x/eps >= from | non-candidate)':>44s}\n")
    n_non = max(tot["non_candidates"], 1)
    surv = np.cumsum(ratio[::-1])[::-1]
    for b in range(Rb):
        if surv[b]:
            w(f"{b / Rb:8.4f} {(b + 1) / Rb:8.4f} {ratio[b]:16d} {surv[b] / n_non:44.3e}\n")
    # tail estimate: log-linear fit of the survival function over its populated upper bins, extrapolated to x / eps = 1
    idx = [b for b in range(Rb) if surv[b] > 0]
    est = None
    if len(idx) >= 3:
        top = idx[-min(len(idx), 8):]
        xs = np.array([b / Rb for b in top]); ys = np.log10(np.array([surv[b] / n_non for b in top]))
        A = np.vstack([xs, np.ones_like(xs)]).T
        slope, icpt = np.linalg.lstsq(A, ys, rcond=None)[0]
        est = 10.0 ** (slope * 1.0 + icpt)
        w(f"\nTail estimate: log10 survival falls by {-slope:.1f} per unit of x / eps over the last {len(top)} populated bins "
          f"(x/eps in [{xs[0]:.3f}, {xs[-1] + 1 / Rb:.3f})); extrapolated to x / eps = 1: P(miss-capable pair) ~ {est:.1e} per unevaluated pair.\n")
        w("(An upper-bound reading: a pair with x > eps only changes a result if its exact value also lies below the k-th smallest of its rollout;\n")
        w(" and before it gets there it has to pass x > eps / 2, which makes the library redo the propagate in fp32 and widen eps.)\n")
    w(f"\nRule of three on the count itself: 0 pairs above eps / 2 among {tot['non_candidates']:.3e} gives P(x > eps / 2) < {3.0 / n_non:.1e} at 95 % confidence.\n")
    return dict(tot, worst_ratio=worst_ratio, tail_estimate=est)


def moving_legs(a):
    """Screening over an obstacle horizon, every step of every propagate swept against the slab it saw."""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    N, H, DT = a.rollouts, a.horizon, 0.5
    shelf = scenes.shelf_scene()
    O = shelf.shape[0]
    share = lambda f: max(2, int(round(f * a.pairs / (N * H * O))))

    def streamer(frame=False, table=False, period=8):
        """The shelf's spheres drift at velocities uniform in +-0.2 m/s, drawn again every `period` iterations from the shelf itself
        (up to 0.8 m of drift at dt = 0.5; the horizon adds up to (H - 1) dt v on top)."""
        state = {}

        def set_scene(e, it):
            if it % period == 0:
                state["vel"] = np.random.RandomState(500 + it).uniform(-0.2, 0.2, (O, 3)).astype(np.float32)
                state["obs"] = shelf.copy()
            else:
                state["obs"] = state["obs"].copy()
                state["obs"][:, :3] += np.float32(DT) * state["vel"]
            e.set_obstacles(state["obs"])
            if table:      # the caller's own predictions: the same motion, radii growing by 2 % per step
                t = predict_obstacle_horizon(state["obs"], state["vel"], H, DT)
                t[:, :, 3] *= (1 + np.float32(0.02) * np.arange(H, dtype=np.float32))[:, None]
                e.set_obstacle_horizon(t)
            else:
                e.set_obstacle_motion(state["vel"])
            e.set_obstacle_frame(frame)
        return set_scene

    legs = []
    e = make_engine("franka", N, H, shelf)
    e.set_screening_horizon(True)
    legs.append(run_leg("shelf, motion horizon +-0.2 m/s", e, share(0.34), horizon_of=streamer(), seed=41))
    legs.append(run_leg("  ... in the moving frame", e, share(0.22), horizon_of=streamer(frame=True), seed=42))
    legs.append(run_leg("  ... explicit table, radii +2 %/step", e, share(0.16), horizon_of=streamer(table=True), seed=43))
    e.close()
    for kind, act, name, sd in (("franka_tanh", "tanh", "tanh 256x3, motion horizon", 44), ("franka_skip", "relu", "skip-connection net, motion horizon", 45)):
        e = make_engine(kind, N, H, shelf, act=act)
        e.set_screening_horizon(True)
        legs.append(run_leg(name, e, share(0.14), horizon_of=streamer(), seed=sd))
        e.close()
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=float, default=1.0e10, help="total (rollout, obstacle) pairs to sweep, split over the legs")
    ap.add_argument("--rollouts", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--json", default=None, help="also write the raw per-leg numbers there")
    ap.add_argument("--legs", default="static", choices=["static", "moving"], help="moving: the legs with an obstacle horizon (screening over it)")
    a = ap.parse_args()
    if a.legs == "moving":
        return finish(moving_legs(a), a)
    from optimalmodulationds_amd import scenes
    N, H = a.rollouts, a.horizon
    shelf = scenes.shelf_scene()
    per_iter = N * H * shelf.shape[0]
    share = lambda f: max(2, int(round(f * a.pairs / per_iter)))
    legs = []

    e = make_engine("franka", N, H, shelf)
    legs.append(run_leg("shelf static (ReLU 256x4, shipped)", e, share(0.28), seed=1))
    legs.append(run_leg("shelf moving +-0.05 m (dynamic)", e, share(0.22), obs_of=lambda it: shelf + np.array([0, 0.05 * np.sin(0.3 * it), 0, 0], np.float32), seed=2))
    legs.append(run_leg("shelf, starts uniform in joint box", e, share(0.22), uniform_starts=True, seed=3))
    e.close()
    for si, (sname, fn) in enumerate(scenes.STREAMED_SCENES.items()):
        if sname == "shelf":
            continue
        obs = fn()
        e = make_engine("franka", N, H, obs)
        n_it = max(2, int(round(0.04 * a.pairs / (N * H * obs.shape[0]))))
        legs.append(run_leg(f"streamed scene '{sname}' (O = {obs.shape[0]})", e, min(n_it, 40), seed=10 + si))
        e.close()
    e = make_engine("franka_tanh", N, H, shelf, act="tanh")
    legs.append(run_leg("shelf, tanh 256x3 (synthetic weights)", e, share(0.12), seed=30))
    e.close()
    e = make_engine("franka_skip", N, H, shelf)
    legs.append(run_leg("shelf, skip-connection net (synthetic)", e, share(0.12), seed=31))
    e.close()
    finish(legs, a)


def finish(legs, a):
    summary = report(legs)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(summary=summary, legs=[dict(name=l["name"], iterations=l["iterations"], seconds=l["seconds"], stats=l["stats"],
                                                       hist={k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in l["hist"].items()}) for l in legs]), f, indent=1)
    if summary["above_half_eps"] or summary["above_eps"] or summary["non_finite"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
