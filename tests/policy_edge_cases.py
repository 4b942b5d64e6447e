"""The inputs of the policy-edge tests, shared by tests/test_policy_edges_cpu.py (the references against the oracle, and wrong
references against the bars) and tests/test_gpu_policy_edges.py (the device against the references): both must see the same
numbers, or the sensitivity check says nothing about the device test.  Plain numpy, no GPU."""
import numpy as np

import policy_ref as pr

F32 = np.float32
C0 = 37.0                                  # cost = C0 (1 + 0.02 u): the exponents span 50 +- 1, every normalised weight stays above 0.25 / N (checked on the CPU)
UPDATE_N = (1, 255, 256, 257, 1000, 1300)  # one thread slot short of a stride, exact, one over; past 1024; no multiple of 32
UPDATE_DOF = (2, 7)
UPDATE_K = (0, 1, 3, 50)
UPDATE_H = (1, 3)
KMAX = 50
RATE = 0.7
COST_N = 300
COST_B = (1, 31, 33, 255, 257)
COST_H = (1, 2, 5)
COST_TERM_SETS = (1, 2, 4, 8, 16, pr.COST_ALL, pr.COST_TOY)


def update_case(N, n, K, H, seed=0):
    """cost [N], the sampled policy [N, K, ...], qdot [N, n], kernel values [N, H, K] and activations [N, H] in (0, 1) with a
    per-kernel scale (so that the means of the mask spread over (0, 1)), current means, and ``ker_thr``: the middle of the widest gap
    in the central half of the means the mask compares, so that kernels fall on both sides (asserted to leave 1e-3 on either side)."""
    rng = np.random.RandomState(1000 * seed + 7 * N + 3 * n + 11 * K + H)
    c = dict(cost=(C0 * (1 + 0.02 * rng.uniform(-1, 1, N))).astype(F32),
             mu_tmp=rng.standard_normal((N, K, n)).astype(F32), sigma_tmp=rng.standard_normal((N, K)).astype(F32),
             alpha_tmp=rng.standard_normal((N, K, n)).astype(F32), qdot=rng.standard_normal((N, n)).astype(F32),
             kval=(rng.uniform(0.05, 1, (N, H, K)) * np.linspace(0.15, 1.0, max(K, 1))[None, None, :K]).astype(F32),
             act=rng.uniform(0.05, 1, (N, H)).astype(F32),
             mu_c=rng.standard_normal((K, n)).astype(F32), sigma_c=(1 + rng.rand(K)).astype(F32),
             alpha_c=rng.standard_normal((K, n)).astype(F32), ker_thr=0.3)
    if K:
        means = []
        for variant in (0, pr.KVAL_TIMES_ACT):
            _, m1, m2 = pr.update_mask(c["kval"], c["act"], 0.0, variant)
            means += [m1, m2]
        v = np.sort(np.concatenate(means + [np.array([0.0, 1.0])]))
        lo = len(v) // 4
        g = lo + int(np.argmax(np.diff(v)[lo:len(v) - 1 - lo]))
        assert v[g + 1] - v[g] >= 4e-3, "no gap of 4e-3 between the means of the mask"
        c["ker_thr"] = float(F32(0.5 * (v[g] + v[g + 1])))
        assert np.abs(np.concatenate(means) - c["ker_thr"]).min() >= 1e-3
    return c


def dyadic_kernel_values(N, H, K, value):
    """Kernel values all ``value`` (0.25, 0.5, 0.75), activations all 1: every sum over rollouts or steps is exact in float32 in any
    order, and so are the means, so ``ker_thr = 0.5`` tests the strict > without a rounding argument."""
    return np.full((N, H, K), value, F32), np.ones((N, H), F32)


def dyadic_tail_thr(N):
    """A threshold between 0.5, the exact mean of N kernel values of 0.5, and 0.5 (N - 1) / N, the mean of a sum that lost one."""
    return float(F32(0.5 - 0.25 / N))


def cost_limits(n):
    """(q_min, q_max, qf, dh [n + 1, 4]) of the first n Franka joints."""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.cost import FRANKA_Q_MAX, FRANKA_Q_MIN
    return (np.array(FRANKA_Q_MIN, F32)[:n], np.array(FRANKA_Q_MAX, F32)[:n], scenes.FRANKA_QF[:n].astype(F32),
            scenes.franka_dh_params()[:n + 1].astype(F32))


CRAFTED = ("ulp_above_last", "on_min", "on_max", "ulp_below_first", "ulp_above_middle", "neg_zero_dist", "pos_zero_dist",
           "denormal_dist", "no_motion", "no_motion_at_goal", "nan_dist")


def cost_case(n, H, B, seed=0):
    """all_traj [B, H, n] inside the joint limits, closest_dist_all [B, H] of both signs, with the crafted rows written over the LAST
    rows of the batch (row B - 1 - i holds CRAFTED[i], as far as B reaches) -- where a dropped tail or a wrong stride shows -- and,
    from B = 33 on, over the first rows as well.  -> (all_traj, closest_dist_all, {name: [rows]})."""
    q_min, q_max, qf, _ = cost_limits(n)
    rng = np.random.RandomState(100 * seed + 13 * n + 5 * H + B)
    tr = (q_min + (q_max - q_min) * rng.uniform(0.1, 0.9, (B, H, n))).astype(F32)
    di = rng.uniform(-0.05, 0.3, (B, H)).astype(F32)
    where = {name: [] for name in CRAFTED}
    j_mid, h_mid = n // 2, H // 2
    for i, name in enumerate(CRAFTED):
        for row in ([B - 1 - i] if i < B else []) + ([i] if B >= 33 else []):
            where[name].append(row)
            if name == "on_min":
                tr[row, 0, 0] = q_min[0]
            elif name == "on_max":
                tr[row, H - 1, n - 1] = q_max[n - 1]
            elif name == "ulp_below_first":
                tr[row, 0, j_mid] = np.nextafter(q_min[j_mid], F32(-np.inf))
            elif name == "ulp_above_middle":
                tr[row, h_mid, 0] = np.nextafter(q_max[0], F32(np.inf))
            elif name == "ulp_above_last":
                tr[row, H - 1, n - 1] = np.nextafter(q_max[n - 1], F32(np.inf))
            elif name == "neg_zero_dist":
                di[row] = F32(-0.0)
            elif name == "pos_zero_dist":
                di[row] = F32(0.0)
            elif name == "denormal_dist":
                di[row] = F32(-1e-45)
            elif name == "no_motion":
                tr[row, :, :] = tr[row, 0, :]
            elif name == "no_motion_at_goal":
                tr[row, :, :] = qf
            elif name == "nan_dist":
                di[row, h_mid] = np.nan
    return tr, di, where


def best_case(N=1000, n_out=300):
    """Per-rollout starts of the planar two-link arm for the shared-minimum propagate: rollouts 0 .. n_out - 1 start beyond q_max of
    joint 0, the others well inside the limits."""
    rng = np.random.RandomState(5)
    q = rng.uniform(-2.0, 2.0, (N, 2)).astype(F32)
    q[:n_out, 0] = rng.uniform(3.12, 3.14, n_out).astype(F32)
    return q


def planar_starts(N, seed):
    return np.random.RandomState(seed).uniform(-3.0, 3.0, (N, 2)).astype(F32)
