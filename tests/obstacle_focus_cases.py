"""The definition of the obstacle focus (include/omds.h: omds_obstacle_focus_select) restated in numpy in the header's operation order,
and the cases of tests/test_obstacle_focus_cpu.py (the GPU tests restate with the same function)."""
import numpy as np

from cloud_flow_cases import fmaf

F32 = np.float32
INF = F32(np.inf)


def reach(d, vel, lookahead):
    d = np.asarray(d, F32).reshape(-1)
    if vel is None:
        return d.copy()
    v = np.asarray(vel, F32).reshape(-1, 3)
    r = np.empty_like(d)
    with np.errstate(all="ignore"):
        for o in range(d.size):
            s2 = fmaf(v[o, 2], v[o, 2], fmaf(v[o, 1], v[o, 1], v[o, 0] * v[o, 0]))
            r[o] = fmaf(-np.sqrt(F32(s2)), F32(lookahead), d[o])
    return r


def restate(d, k, margin, max_keep=0, lookahead=0.0, vel=None):
    """-> (kept indices ascending int32, passed)"""
    r = reach(d, vel, lookahead)
    r = np.where(np.isnan(r), -INF, r) + F32(0)          # NaN counts as -inf; -0 + 0 = +0: the comparison never told them apart
    order = np.lexsort((np.arange(r.size), r))
    with np.errstate(all="ignore"):
        t = r[order[k - 1]]
        passed = r.size if np.isinf(F32(margin)) else int((r <= F32(t + F32(margin))).sum())
    kept = min(passed, max_keep) if max_keep >= 1 else passed
    return np.sort(order[:kept]).astype(np.int32), passed


def below(x):
    return np.nextafter(F32(x), -INF)


def above(x):
    return np.nextafter(F32(x), INF)


def cases(k=10):
    """-> list of (name, d, vel or None, k, margin, max_keep, lookahead)"""
    rng = np.random.RandomState(7)
    out = []
    for O in (k, k + 1, 64, 65, 1023, 1024, 1025, 5000):
        d = rng.uniform(0.02, 1.5, O).astype(F32)
        out.append((f"random{O}", d, None, k, 0.1, 0, 0.0))
        out.append((f"random{O}_cap", d, None, k, 0.3, max(k, O // 3), 0.0))
    # margins around a gap: the k nearest at (i + 1) / 128, one sphere at t + 0.625.  Dyadic values, and the gap lies in the binade of
    # the sum: t + gap, t + the float below gap and t + the float above it are all exact, so the three bars are three different floats
    d = np.concatenate([(np.arange(k) + 1) / 128.0, [k / 128.0 + 0.625], rng.uniform(1.0, 2.0, 30)]).astype(F32)
    gap = F32(d[k] - d[k - 1])
    for name, m in (("zero", F32(0)), ("below_gap", below(gap)), ("gap", gap), ("above_gap", above(gap)), ("inf", INF)):
        out.append((f"margin_{name}", rng.permutation(d).astype(F32), None, k, m, 0, 0.0))
    # duplicated distances, max_keep cutting through the tie group; max_keep = k
    d = np.concatenate([np.full(7, 0.25), np.full(12, 0.5), np.full(5, 0.125), rng.uniform(0.6, 1.0, 20)]).astype(F32)
    d = rng.permutation(d).astype(F32)
    for mk in (k, 15, 18, 24, 25):
        out.append((f"ties_keep{mk}", d, None, k, 0.3, mk, 0.0))
    out.append(("ties_at_threshold", d, None, k, 0.0, 0, 0.0))          # the k-th lies inside the group at 0.5: the whole group passes
    out.append(("all_equal", np.full(33, 0.5, F32), None, k, 0.0, 20, 0.0))
    # negative distances, -0 beside +0
    d = np.concatenate([rng.uniform(-0.3, 0.3, 40), [0.0, -0.0, 0.0, -0.0]]).astype(F32)
    out.append(("negative", d, None, k, 0.05, 0, 0.0))
    z = np.array([0.0, -0.0] * 8 + [0.5, -0.5, 1.0], F32)
    out.append(("zeros_cut", z, None, k, 0.0, 12, 0.0))
    out.append(("zeros_threshold", z, None, 5, 0.0, 0, 0.0))
    # NaN and +-inf distances: fewer than k NaNs, at least k NaNs
    base = rng.uniform(0.1, 1.0, 50).astype(F32)
    few = base.copy(); few[[3, 17, 40]] = np.nan; few[[5, 9]] = np.inf; few[11] = -np.inf
    out.append(("nan_few", few, None, k, 0.1, 0, 0.0))
    out.append(("nan_few_cap", few, None, k, 0.1, k, 0.0))
    many = base.copy(); many[::4] = np.nan
    out.append(("nan_many", many, None, k, 0.1, 0, 0.0))
    out.append(("nan_many_inf_margin", many, None, k, INF, 20, 0.0))
    infs = base.copy(); infs[: 45] = np.inf
    out.append(("threshold_is_inf", infs, None, k, 0.1, 0, 0.0))
    # velocities whose lookahead pulls a far sphere in; a non-finite velocity
    d = np.concatenate([np.linspace(0.1, 0.3, 12), [2.0, 2.0, 2.0, 2.0]]).astype(F32)
    vel = np.zeros((16, 3), F32)
    vel[12] = [0.3, -0.4, 1.2]          # speed 1.3: reach 2 - 1.3 * 1.5 = 0.05
    vel[13] = [0.01, 0.0, 0.0]
    out.append(("lookahead_pulls_in", d, vel, k, 0.0, 0, 1.5))
    out.append(("lookahead_zero", d, vel, k, 0.0, 0, 0.0))
    bad = vel.copy(); bad[14] = [np.inf, 0.0, 0.0]; bad[15] = [0.0, np.nan, 0.0]
    out.append(("velocity_not_finite", d, bad, k, 0.0, 0, 1.5))
    out.append(("velocity_not_finite_no_lookahead", d, bad, k, 0.05, 0, 0.0))
    rv = rng.uniform(0.05, 2.0, 300).astype(F32)
    out.append(("random_moving", rv, (0.3 * rng.standard_normal((300, 3))).astype(F32), k, 0.2, 0, 0.75))
    return out
