"""The definition of the obstacle focus along a path (include/omds.h: omds_obstacle_focus_select_path) restated in numpy in the
header's operation order, and the cases of tests/test_obstacle_focus_path_cpu.py (the GPU tests restate with the same function)."""
import numpy as np

from obstacle_focus_cases import F32, INF, above, below, reach


def clean(r):
    """NaN counts as -inf; -0 + 0 = +0: the comparison never told them apart"""
    return np.where(np.isnan(r), -INF, r) + F32(0)


def restate_path(d, k, margin, max_keep=0, lookahead=0.0, ahead=None, vel=None):
    """d [B, O] -> (kept indices ascending int32, passed)"""
    d = np.asarray(d, F32)
    B, O = d.shape
    passing = np.zeros(O, bool)
    nearest = np.full(O, INF, F32)
    index = np.arange(O)
    with np.errstate(all="ignore"):
        for b in range(B):
            time = F32(lookahead) if ahead is None else F32(F32(lookahead) + F32(ahead[b]))      # TIME: one rounding
            r = clean(reach(d[b], vel, time))
            t = r[np.lexsort((index, r))[k - 1]]
            passing |= True if np.isinf(F32(margin)) else r <= F32(t + F32(margin))
            nearest = np.minimum(nearest, r)
    order = [o for o in np.lexsort((index, nearest)) if passing[o]]
    passed = len(order)
    kept = min(passed, max_keep) if max_keep >= 1 else passed
    return np.sort(order[:kept]).astype(np.int32), passed


def path_cases(k=10):
    """-> list of (name, d [B, O], ahead or None, vel or None, k, margin, max_keep, lookahead)"""
    rng = np.random.RandomState(17)
    out = []
    # random rows: every state has another set of near spheres
    for B in (1, 2, 3, 16, 17, 64, 300):
        for O in (k, k + 1, 65, 1025, 5000):
            d = rng.uniform(0.02, 1.5, (B, O)).astype(F32)
            out.append((f"random_B{B}_O{O}", d, None, None, k, 0.02, 0, 0.0))
            out.append((f"random_B{B}_O{O}_cap", d, None, None, k, 0.05, max(k, O // 3), 0.0))
    # a sphere that passes at exactly one state: sphere 30 is far everywhere but in row 2, where it is the nearest
    base = np.concatenate([(np.arange(k) + 1) / 64.0, np.linspace(1.0, 2.0, 30)]).astype(F32)
    d = np.stack([rng.permutation(base[:k]).tolist() + base[k:].tolist() for _ in range(4)]).astype(F32)
    d[2, 30] = F32(1 / 256.0)
    out.append(("passes_at_one_state", d, None, None, k, 0.0, 0, 0.0))
    # thresholds that differ by orders of magnitude: row 0 around 1e-3, row 1 around 1e+2; a margin of 0.5 means everything in row 0's
    # scale and nothing beyond the k-th in row 1's
    d = np.stack([np.linspace(1e-3, 4e-3, 40), np.linspace(400.0, 100.0, 40)]).astype(F32)
    out.append(("thresholds_far_apart", d, None, None, k, 0.5, 0, 0.0))
    out.append(("thresholds_far_apart_small_margin", d, None, None, k, 1e-4, 0, 0.0))
    # margins around a gap in ONE row (the construction of obstacle_focus_cases.cases: dyadic values, exact sums); the other row has
    # its k nearest elsewhere and a gap no margin here reaches
    row = np.concatenate([(np.arange(k) + 1) / 128.0, [k / 128.0 + 0.625], np.linspace(1.0, 2.0, 30)]).astype(F32)
    gap = F32(row[k] - row[k - 1])
    other = np.concatenate([np.linspace(4.0, 8.0, k + 1), (np.arange(k) + 1) / 128.0, np.full(20, 16.0)]).astype(F32)
    for name, m in (("zero", F32(0)), ("below_gap", below(gap)), ("gap", gap), ("above_gap", above(gap)), ("inf", INF)):
        out.append((f"margin_{name}", np.stack([row, other]), None, None, k, m, 0, 0.0))
    # a cap cutting a tie group of m_o: twelve spheres whose nearest reach is 0.5, reached in different rows
    d = rng.uniform(0.6, 1.0, (3, 44)).astype(F32)
    d[:, :7] = F32(0.25)
    for j in range(12):
        d[j % 3, 7 + j] = F32(0.5)
    d[:, 19:24] = F32(0.125)
    p = rng.permutation(44)
    d = np.ascontiguousarray(d[:, p])
    for mk in (k, 15, 18, 24, 25):
        out.append((f"ties_keep{mk}", d, None, None, k, 0.3, mk, 0.0))
    out.append(("cap_with_inf_margin", d, None, None, k, INF, 20, 0.0))
    out.append(("inf_margin", d, None, None, k, INF, 0, 0.0))
    # a NaN distance in one row only: always kept, whatever the cap leaves
    d = rng.uniform(0.1, 1.0, (5, 50)).astype(F32)
    d[3, 41] = np.nan
    d[:3, 41] = d[4, 41] = F32(5.0)
    out.append(("nan_in_one_row", d, None, None, k, 0.0, 0, 0.0))
    out.append(("nan_in_one_row_cap", d, None, None, k, 0.0, k, 0.0))
    # a row whose threshold is +inf: everything passes there
    d = rng.uniform(0.1, 1.0, (3, 50)).astype(F32)
    d[1, : 45] = np.inf
    out.append(("threshold_is_inf", d, None, None, k, 0.01, 0, 0.0))
    out.append(("threshold_is_inf_cap", d, None, None, k, 0.01, 30, 0.0))
    # -0 beside +0
    z = np.array([0.0, -0.0] * 8 + [0.5, -0.5, 1.0], F32)
    d = np.stack([z, z[::-1], np.abs(z)]).astype(F32)
    out.append(("zeros_cut", d, None, None, k, 0.0, 12, 0.0))
    out.append(("zeros_threshold", d, None, None, 5, 0.0, 0, 0.0))
    # a moving sphere that passes only through a late state's ahead: speed 1.3, distance 2 everywhere; reach 2 - 1.3 * 1.5 = 0.05 in
    # the last row alone
    row = np.concatenate([np.linspace(0.1, 0.3, 12), [2.0, 2.0, 2.0, 2.0]]).astype(F32)
    d = np.stack([row] * 4)
    vel = np.zeros((16, 3), F32)
    vel[12] = [0.3, -0.4, 1.2]
    vel[13] = [0.01, 0.0, 0.0]
    ahead = np.array([0.0, 0.5, 1.0, 1.5], F32)
    out.append(("late_ahead_pulls_in", d, ahead, vel, k, 0.0, 0, 0.0))
    out.append(("ahead_too_short", d, ahead[[0, 1, 2, 2]], vel, k, 0.0, 0, 0.0))
    out.append(("ahead_and_lookahead", d, ahead[[0, 1, 1, 2]], vel, k, 0.0, 0, 0.5))
    out.append(("ahead_without_velocities", d, ahead, None, k, 0.0, 0, 0.0))
    bad = vel.copy()
    bad[14] = [np.inf, 0.0, 0.0]
    bad[15] = [0.0, np.nan, 0.0]
    out.append(("velocity_not_finite", d, ahead, bad, k, 0.0, 0, 0.0))
    out.append(("velocity_not_finite_no_time", d, None, bad, k, 0.05, 0, 0.0))
    rv = rng.uniform(0.05, 2.0, (6, 300)).astype(F32)
    out.append(("random_moving", rv, rng.uniform(0.0, 1.0, 6).astype(F32), (0.3 * rng.standard_normal((300, 3))).astype(F32), k, 0.1, 0, 0.25))
    out.append(("random_moving_cap", rv, rng.uniform(0.0, 1.0, 6).astype(F32), (0.3 * rng.standard_normal((300, 3))).astype(F32), k, 0.1, 50, 0.25))
    return out
