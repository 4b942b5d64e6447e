"""The float64 references of tests/policy_ref.py, without a GPU:

  a. against the fp32 oracle (oracle/omds_oracle.py) on the inputs tests/test_gpu_policy_edges.py gives the device
     (tests/policy_edge_cases.py), within the bars that test applies -- the reference and the oracle are two independent restatements.
     The candidates are the exception: the device test gates the device's own rollouts, here the same gates run on random states.
  b. sensitivity: a reference that drops rollout N - 1, every t >= 1024 or every t >= 256 from its sums, takes the last of equal minima,
     or compares >= where the mask has >, MISSES those bars on those inputs -- so a kernel with that defect would fail the device
     test; and an fp32 emulation of the kernels' own order (stride 256 per thread, then the LDS tree) meets them.
  c. omds_apply_update (host arithmetic of csrc/update.hip) against float64: every variant, a mean exactly on ker_thr, NaN sums, K = 0.
"""
import numpy as np
import pytest

import policy_edge_cases as pc
import policy_ref as pr
from helpers import OWN, RTOL, rel_err
from oracle import omds_oracle as orc

F32 = np.float32
W_TOL = 2e-5          # MPPI weights and alpha_c: the bar of test_free_running_cost_update


def _w_err(got, want):
    return rel_err(got, want, floor=float(np.max(want)))


# ---- a. reference against oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 8))
def test_cost_reference_against_the_oracle(n):
    q_min, q_max, qf, dh = pc.cost_limits(n)
    for H in pc.COST_H:
        tr, di, where = pc.cost_case(n, H, 257)
        total, parts = pr.evaluate_costs(tr, di, qf, dh, q_min, q_max)
        with np.errstate(over="ignore", invalid="ignore"):
            o_total, o_parts = orc.evaluate_costs(tr, di, qf, dh, q_min, q_max)
        pr.assert_close_nonfinite(np.asarray(o_total, F32), total, RTOL, f"total, n {n} H {H}")
        for name in ("goal", "stag", "fk"):
            pr.assert_close_nonfinite(np.asarray(o_parts[name], F32), parts[name], RTOL, f"{name}, n {n} H {H}")
        for name in ("coll", "jl"):       # the discrete terms: exact
            assert np.array_equal(np.asarray(o_parts[name], np.float64), parts[name]), (name, n, H)
        # the crafted rows say what they were made to say
        for r in where["on_min"] + where["on_max"]:
            assert parts["jl"][r] == 0
        for r in where["ulp_below_first"] + where["ulp_above_middle"] + where["ulp_above_last"]:
            assert parts["jl"][r] == 100
        for r in where["neg_zero_dist"] + where["pos_zero_dist"]:
            assert parts["coll"][r] == 0
        for r in where["denormal_dist"]:
            assert parts["coll"][r] == 100 * H
        for r in where["no_motion"]:
            assert np.isposinf(pr.f32(parts["stag"][r])) and np.isposinf(pr.f32(total[r]))
        for r in where["no_motion_at_goal"]:
            assert parts["stag"][r] == 0 and parts["goal"][r] == 0
        for ts in pc.COST_TERM_SETS:      # a term set is the left-to-right sum of its parts
            t2, _ = pr.evaluate_costs(tr, di, qf, dh, q_min, q_max, ts)
            names = tuple(k for k, bit in pr.TERMS.items() if ts & bit)
            with np.errstate(over="ignore", invalid="ignore"):
                o2, _ = orc.evaluate_costs(tr[:33], di[:33], qf, dh, q_min, q_max, names)
            pr.assert_close_nonfinite(np.asarray(o2, F32), t2[:33], RTOL, f"terms {ts}, n {n} H {H}")


@pytest.mark.parametrize("N", pc.UPDATE_N)
def test_update_reference_against_the_oracle(N):
    for n in pc.UPDATE_DOF:
        for K in pc.UPDATE_K:
            for H in pc.UPDATE_H:
                c = pc.update_case(N, n, K, H)
                for variant in (0, pr.KVAL_TIMES_ACT | pr.NO_BASE_MASK):      # the two the oracle knows: MPPI.py and MPPI_toy.py
                    mu, sg, al, mask, w = pr.shift_policy_means(c["cost"], c["kval"], c["act"], c["mu_c"], c["sigma_c"], c["alpha_c"],
                                                                c["mu_tmp"], c["sigma_tmp"], c["alpha_tmp"], c["ker_thr"], pc.RATE, variant)
                    omu, osg, oal, omask, ow = orc.shift_policy_means(c["cost"], c["kval"], c["act"], c["mu_c"], c["sigma_c"], c["alpha_c"],
                                                                      c["mu_tmp"], c["sigma_tmp"], c["alpha_tmp"], c["ker_thr"], pc.RATE,
                                                                      toy=bool(variant))
                    what = f"N {N} n {n} K {K} H {H} variant {variant}"
                    assert w.min() * N > 0.25, what      # exp(-1) / mean(exp(-u)) = 0.31 in expectation
                    assert _w_err(ow, w) <= W_TOL, what
                    assert np.array_equal(mask, omask), what
                    assert rel_err(omu, mu) <= RTOL and rel_err(osg, sg) <= RTOL and rel_err(oal, al) <= W_TOL, what
                assert rel_err(orc.get_qdot(c["cost"], c["qdot"], "weighted"), pr.get_qdot(c["cost"], c["qdot"], "weighted"), OWN) <= W_TOL
                assert np.array_equal(orc.get_qdot(c["cost"], c["qdot"], "best"), pr.get_qdot(c["cost"], c["qdot"], "best"))


def _random_rollouts(N, H, n, seed):
    rng = np.random.RandomState(seed)
    return (rng.uniform(-3, 3, (N, H, n)).astype(F32), rng.uniform(-0.2, 1.0, (N, H)).astype(F32), rng.uniform(-1, 1, (N, H)).astype(F32),
            rng.uniform(-3, 3, (3, n)).astype(F32), rng.uniform(0.05, 0.5, 3).astype(F32))


@pytest.mark.parametrize("p", [1, 2, 3])
def test_candidate_reference_against_the_oracle(p):
    tr, di, dots, mu_c, sg_c = _random_rollouts(1300, 3, 2, 9)
    for K in (0, 3):
        gated, rbf, cand = pr.check_traj_for_kernels(tr, di, dots, mu_c[:K], sg_c[:K], 0.4, 0.2, 0.1, p)
        with np.errstate(under="ignore"):
            want = orc.check_traj_for_kernels(tr, di, dots, mu_c[:K], sg_c[:K], F32(0.4), F32(0.2), F32(0.1), p)
        near = gated & (np.abs(rbf - float(F32(0.2))) <= 2e-5 * 0.2)
        assert near.sum() <= 0.01 * gated.sum()
        if not near.any():
            assert np.array_equal(tr[cand], want)
        assert 0.2 < gated.mean() < 0.8 and (K == 0 or 0.1 < cand.sum() / gated.sum() < 0.9)


def test_topk_reference():
    rng = np.random.RandomState(4)
    rows = rng.standard_normal((16, 700)).astype(F32)
    rows[:, ::7] = rows[:, 3:4]                                               # ties
    for row in rows:
        assert np.array_equal(pr.topk_ref(row, 64), np.argsort(row, kind="stable")[:64])
    inf, nan = np.inf, np.nan
    assert pr.topk_ref([nan, nan, nan, 7.0, nan, nan, nan, nan, nan, nan, inf], 4).tolist() == [3, 10, 0, 0]   # dry: index 0, not the inf again
    assert pr.topk_ref([0.0, -0.0, 0.5, -0.0, -1.0], 5).tolist() == [4, 0, 1, 3, 2]                            # -0 equals +0
    assert pr.topk_ref([inf, -inf, nan, inf, -inf], 5).tolist() == [1, 4, 0, 3, 0]
    assert pr.topk_ref([nan, nan], 2).tolist() == [0, 0]


# ---- b. sensitivity ---------------------------------------------------------------------------------------------------------------------
def _strided_tree_sum(x):
    """fp32 sum of x [N, ...] over axis 0 in the kernels' order: thread tid adds t = tid, tid + 256, ... in turn, then the LDS tree."""
    x = np.asarray(x, F32)
    pad = (-x.shape[0]) % 256
    x = np.concatenate([x, np.zeros((pad,) + x.shape[1:], F32)]).reshape((-1, 256) + x.shape[1:])
    part = np.zeros(x.shape[1:], F32)
    for r in x:
        part = (part + r).astype(F32)
    s = 128
    while s:
        part[:s] = (part[:s] + part[s:2 * s]).astype(F32)
        s //= 2
    return part[0]


def _fp32_kernel_order(c, K):
    """What the device computes for the weights and the weighted sums, emulated in float32 in its order of operations."""
    cost = c["cost"]
    N = cost.shape[0]
    beta = F32(F32(_strided_tree_sum(cost) / F32(N)) / F32(50))
    w = np.exp((F32(-1) / beta) * cost).astype(F32)
    sw = _strided_tree_sum(w)
    out = dict(w=(w / sw).astype(F32), qdot=(_strided_tree_sum(w[:, None] * c["qdot"]) / sw).astype(F32))
    if K:
        out.update(mu=(_strided_tree_sum(w[:, None, None] * c["mu_tmp"]) / sw).astype(F32), sigma=(_strided_tree_sum(w[:, None] * c["sigma_tmp"]) / sw).astype(F32),
                   alpha=(_strided_tree_sum(w[:, None, None] * c["alpha_tmp"]) / sw).astype(F32))
    return out


def _blend(cur, s):
    return (1 - pc.RATE) * cur.astype(np.float64) + pc.RATE * np.asarray(s, np.float64)


def _wrong_keeps(N):
    keeps = {"rollout N-1 dropped": np.arange(N) < N - 1}
    if N > 1024:
        keeps["t >= 1024 dropped"] = np.arange(N) < 1024
    if N > 256:
        keeps["t >= 256 dropped"] = np.arange(N) < 256
    return keeps


@pytest.mark.parametrize("N", [N for N in pc.UPDATE_N if N > 1])
def test_wrong_sums_miss_the_bars(N):
    """On the inputs of the device test every sum with a dropped tail misses the bar the device test applies to it, by more than a
    decade; the kernels' own order in fp32 meets it four times over (the weights carry the rounding of an exponent near -50: 50 x 2^-24
    = 3e-6 relative, whatever the order of the sums)."""
    for n in pc.UPDATE_DOF:
        K, H = 3, 3
        c = pc.update_case(N, n, K, H)
        args = (c["cost"], c["kval"], c["act"], c["mu_c"], c["sigma_c"], c["alpha_c"], c["mu_tmp"], c["sigma_tmp"], c["alpha_tmp"])
        mu, sg, al, mask, w = pr.shift_policy_means(*args, -1.0, pc.RATE)            # ker_thr below every mean: all kernels move
        assert mask.all()
        qd = pr.get_qdot(c["cost"], c["qdot"], "weighted")
        emu = _fp32_kernel_order(c, K)
        assert _w_err(emu["w"], w) <= W_TOL / 4 and rel_err(emu["qdot"], qd, OWN) <= W_TOL / 4
        assert rel_err(_blend(c["mu_c"], emu["mu"]), mu) <= RTOL / 4 and rel_err(_blend(c["sigma_c"], emu["sigma"]), sg) <= RTOL / 4
        assert rel_err(_blend(c["alpha_c"], emu["alpha"]), al) <= W_TOL / 4
        for name, keep in _wrong_keeps(N).items():
            bmu, bsg, bal, _, bw = pr.shift_policy_means(*args, -1.0, pc.RATE, keep=keep)
            bqd = pr.get_qdot(c["cost"], c["qdot"], "weighted", keep=keep)
            what = f"{name}, N {N} n {n}"
            assert _w_err(pr.f32(bw), w) > 10 * W_TOL, what
            assert rel_err(pr.f32(bqd), qd, OWN) > 10 * W_TOL, what
            assert rel_err(pr.f32(bmu), mu) > 10 * RTOL and rel_err(pr.f32(bsg), sg) > 10 * RTOL and rel_err(pr.f32(bal), al) > 10 * W_TOL, what


@pytest.mark.parametrize("N", pc.UPDATE_N)
def test_wrong_masks_differ(N):
    """The dyadic kernel values make the mask's means exact, so a >= for the >, or a sum that lost a rollout, flips a mask bit."""
    K, H = 3, 3
    for variant in (0, 1, 2, 3):
        kv, act = pc.dyadic_kernel_values(N, H, K, 0.5)
        right, m1, m2 = pr.update_mask(kv, act, 0.5, variant)
        assert (m1 == 0.5).all() and (m2 == 0.5).all() and not right.any()
        assert pr.update_mask(kv, act, 0.5, variant, strict=False)[0].all()
        assert not pr.update_mask(*pc.dyadic_kernel_values(N, H, K, 0.25), 0.5, variant)[0].any()
        assert pr.update_mask(*pc.dyadic_kernel_values(N, H, K, 0.75), 0.5, variant)[0].all()
        thr = pc.dyadic_tail_thr(N)            # between the mean of N rollouts and the mean that lost one
        assert pr.update_mask(kv, act, thr, variant)[0].all()
        for name, keep in _wrong_keeps(N).items():
            assert not pr.update_mask(kv, act, thr, variant, keep=keep)[0].any(), name


def test_last_minimum_is_not_the_first():
    cost = np.r_[np.full(300, 100.0), np.zeros(700)].astype(F32)
    qdot = np.random.RandomState(1).standard_normal((1000, 2)).astype(F32)
    best = pr.get_qdot(cost, qdot, "best")
    assert np.array_equal(best, qdot[300])
    for wrong in (999, 556, 812):           # the last minimum; the two that share rollout 300's reduction slot (t mod 256 = 44)
        assert cost[wrong] == cost[300] and not np.array_equal(qdot[wrong], best)
    assert 556 % 256 == 812 % 256 == 300 % 256


def test_dropped_candidates_change_the_count():
    tr, di, dots, mu_c, sg_c = _random_rollouts(1300, 3, 2, 9)
    di[1299], dots[1299] = -0.2, -1.0                  # the last rollout passes the gates, as the device test makes sure it does
    gated, _, _ = pr.check_traj_for_kernels(tr, di, dots, mu_c[:0], sg_c[:0], 0.4, 0.2, 0.1, 2)
    for lim in (1299, 1024, 256):
        assert gated[:lim].sum() < gated.sum()


# ---- c. omds_apply_update ---------------------------------------------------------------------------------------------------------------
def _apply_update(K, n, H, red, n_total, rate, thr, variant, mu, sg, al):
    from optimalmodulationds_amd import _lib
    lib = _lib.load()
    red = np.ascontiguousarray(red, F32)
    mu, sg, al = (np.array(x, F32, order="C", copy=True) for x in (mu, sg, al))
    mask = np.full(max(K, 1), -7, np.int32)
    rc = lib.omds_apply_update(K, n, H, _lib.fptr(red), float(n_total), float(rate), float(thr), int(variant),
                               _lib.fptr(mu) if K else None, _lib.fptr(sg) if K else None, _lib.fptr(al) if K else None, _lib.iptr(mask))
    assert rc == 0
    return mu, sg, al, mask[:K]


def _red(K, n, sumw, s_mu, s_sg, s_al, s_mx, s_ph):
    return np.concatenate([[sumw], np.ravel(s_mu), np.ravel(s_sg), np.ravel(s_al), np.ravel(s_mx), np.ravel(s_ph), np.zeros(2 * n + 1)]).astype(F32)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_apply_update_against_float64(variant):
    rng = np.random.RandomState(variant)
    for K, n, H in ((0, 2, 1), (1, 1, 1), (3, 2, 2), (50, 7, 4)):        # n_total and H powers of two: the means below are exact
        n_total, thr, rate = 8.0, 0.5, 0.7
        mu, sg, al = rng.standard_normal((K, n)).astype(F32), rng.rand(K).astype(F32), rng.standard_normal((K, n)).astype(F32)
        sumw = F32(3.25e-22)
        s_mu, s_sg, s_al = (sumw * rng.standard_normal((K, n))).astype(F32), (sumw * rng.rand(K)).astype(F32), (sumw * rng.standard_normal((K, n))).astype(F32)
        # the two means of kernel kk, cycled: on the threshold exactly, one ulp above, well below, NaN
        kinds = np.arange(K) % 4
        on, above = thr, float(np.nextafter(F32(thr), F32(1)))
        m1 = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3], [on, above, 0.1, np.nan])
        m2 = np.select([(np.arange(K) // 4) % 3 == 0, (np.arange(K) // 4) % 3 == 1, (np.arange(K) // 4) % 3 == 2], [above, on, np.nan])
        s_mx, s_ph = (m1 * n_total).astype(F32), (m2 * H).astype(F32)
        got = _apply_update(K, n, H, _red(K, n, sumw, s_mu, s_sg, s_al, s_mx, s_ph), n_total, rate, thr, variant, mu, sg, al)
        with np.errstate(invalid="ignore"):
            want_mask = (m1 > thr) & ((m2 > thr) | bool(variant & pr.NO_BASE_MASK))
        assert np.array_equal(got[3], want_mask.astype(np.int32)), (K, variant)
        if K >= 4:
            assert got[3][0] == 0 and got[3][2] == 0 and got[3][3] == 0      # exactly on the threshold, below it, NaN: no update
            assert got[3][1] == 1
        u = np.where(want_mask, float(F32(rate)), 0.0)
        for g, cur, s in ((got[0], mu, s_mu), (got[1], sg, s_sg), (got[2], al, s_al)):
            uu = u[:, None] if cur.ndim == 2 else u
            want = (1 - uu) * cur.astype(np.float64) + uu * (s.astype(np.float64) / float(sumw))
            assert rel_err(g, want) <= RTOL, (K, variant)
            assert np.array_equal(g[~want_mask], cur[~want_mask])             # a kernel that does not move keeps its bits


def test_apply_update_nan_sums_move_nothing():
    K, n, H = 2, 2, 2
    mu, sg, al = np.ones((K, n), F32), np.ones(K, F32), np.ones((K, n), F32)
    red = _red(K, n, 1.0, np.zeros((K, n)), np.zeros(K), np.zeros((K, n)), [np.nan, 8.0], [2.0, np.nan])
    for variant, want in ((0, [0, 0]), (pr.NO_BASE_MASK, [0, 1])):
        got = _apply_update(K, n, H, red, 8.0, 0.5, 0.5, variant, mu, sg, al)
        assert got[3].tolist() == want
