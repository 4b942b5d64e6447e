"""The selections and reductions around the network at their edges (run on a real MI355X: ``pytest -m gpu``): k_cost, k_cost_sum,
k_weights, k_policy_sums, k_update_inputs, k_cand_*, k_transpose, k_permute and k_gather_rows (csrc/rollout_kernels.hip) against the
float64 references of tests/policy_ref.py, at the sizes where their second code paths run -- N no multiple of 256 or 32, N > 1024
through the candidate scan, every n_dof instantiation of the cost, B < n_traj, K = n_kernel_max -- and on the inputs where a
reduction can go wrong unseen: a cost of +inf, a cost minimum two rollouts share, a mean exactly on ker_thr, a NaN kernel value.

Bars, the project's own: helpers.RTOL for costs and updated means; 2e-5 of the largest weight for the MPPI weights, 2e-5 for alpha_c
and the weighted qdot (test_free_running_cost_update's); exact equality for masks, indices, counts, gathers, the discrete cost terms
and non-finite values.  tests/test_policy_edges_cpu.py shows, on these very inputs (tests/policy_edge_cases.py), that a reference
with a dropped tail, a last minimum or a >= misses these bars, and that the kernels' order of summation in fp32 meets them.

Left out, one thing: a candidate state whose float64 largest RBF value lies within 2e-5 (relative) of thr_kernel -- the test fails
when that is more than 1 % of the gated states.

Measured on an MI355X (the tests print it): weights and updated means at most 2.0e-6 of their scale, costs at most 2.7e-6 (n = 7),
none of 290 .. 3200 gated states left out at thr_kernel.  The whole module takes under 10 s there."""
import numpy as np
import pytest

import policy_edge_cases as pc
import policy_ref as pr
from helpers import OWN, RTOL, load, rel_err, weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32
W_TOL = 2e-5


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- weights, sums, mask: omds_weighted_update_eval (no network, no scene) ------------------------------------------------------------
def _check_update(eng, c, K, variant, kval, act, thr, what):
    mu, sg, al, mask, w = eng.weighted_update_eval(c["cost"], kval, act, pc.RATE, thr, c["mu_c"], c["sigma_c"], c["alpha_c"], want_weights=True)
    rmu, rsg, ral, rmask, rw = pr.shift_policy_means(c["cost"], kval, act, c["mu_c"], c["sigma_c"], c["alpha_c"], c["mu_tmp"], c["sigma_tmp"],
                                                     c["alpha_tmp"], thr, pc.RATE, variant)
    e_w = rel_err(w, rw, floor=float(rw.max()))
    assert e_w <= W_TOL, f"{what}: weights {e_w:.2e}"
    assert np.array_equal(mask, rmask), f"{what}: mask {mask.astype(int)} != {rmask.astype(int)}"
    e = (rel_err(mu, rmu), rel_err(sg, rsg), rel_err(al, ral))
    assert e[0] <= RTOL and e[1] <= RTOL and e[2] <= W_TOL, f"{what}: mu {e[0]:.2e} sigma {e[1]:.2e} alpha {e[2]:.2e}"
    for got, cur in ((mu, c["mu_c"]), (sg, c["sigma_c"]), (al, c["alpha_c"])):
        assert _bits_equal(got[~rmask], cur[~rmask]), f"{what}: a kernel outside the mask moved"
    return max(e_w, *e), rmask


@pytest.mark.parametrize("N", pc.UPDATE_N)
def test_weights_sums_and_mask(N):
    from optimalmodulationds_amd.engine import Engine
    worst, moved, stayed = 0.0, 0, 0
    for n in pc.UPDATE_DOF:
        for H in pc.UPDATE_H:
            eng = Engine(n, N, H, 1, max_obs=1, n_kernel_max=pc.KMAX)
            for K in pc.UPDATE_K:
                c = pc.update_case(N, n, K, H)
                eng.set_policy_samples(c["mu_tmp"], c["sigma_tmp"], c["alpha_tmp"])
                gmu, gsg, gal = eng.get_policy_samples()
                assert _bits_equal(gmu, c["mu_tmp"]) and _bits_equal(gsg, c["sigma_tmp"]) and _bits_equal(gal, c["alpha_tmp"])
                for variant in (0, 1, 2, 3):
                    eng.params.variant = variant
                    eng.push_params()
                    what = f"N {N} n {n} H {H} K {K} variant {variant}"
                    e, m = _check_update(eng, c, K, variant, c["kval"], c["act"], c["ker_thr"], what)       # means >= 1e-3 off ker_thr
                    worst, moved, stayed = max(worst, e), moved + int(m.sum()), stayed + int((~m).sum())
                    if K == 0:
                        continue
                    for value, want in ((0.5, False), (0.25, False), (0.75, True)):       # exact means: 0.5 > 0.5 must be false
                        kv, act = pc.dyadic_kernel_values(N, H, K, value)
                        _, m = _check_update(eng, c, K, variant, kv, act, 0.5, f"{what}, kernel values all {value}")
                        assert (m == want).all()
                    kv, act = pc.dyadic_kernel_values(N, H, K, 0.5)                       # a sum that lost one rollout would say false
                    _, m = _check_update(eng, c, K, variant, kv, act, pc.dyadic_tail_thr(N), f"{what}, threshold between N and N - 1 rollouts")
                    assert m.all()
                    kv = c["kval"].copy()
                    kv[N // 2, 0, K - 1] = np.nan                                         # torch's max and mean carry it: no update
                    _, m = _check_update(eng, c, K, variant, kv, c["act"], c["ker_thr"], f"{what}, a NaN kernel value")
                    assert not m[K - 1]
            eng.close()
    assert moved > 0 and stayed > 0
    print(f"N {N}: worst error / scale {worst:.2e}; {moved} kernels moved, {stayed} stayed")


# ---- cost: omds_cost_eval --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 8))
def test_cost_every_dof_and_batch(n):
    from optimalmodulationds_amd.engine import Engine
    q_min, q_max, qf, dh = pc.cost_limits(n)
    worst, n_inf = 0.0, 0
    for H in pc.COST_H:
        eng = Engine(n, pc.COST_N, H, 1, max_obs=1)
        eng.set_ds(qf)
        eng.set_cost(dh, q_min, q_max)
        cases = [pc.cost_case(n, H, B) for B in pc.COST_B + (700,)]       # 700 rows: chunks of 300, 300 and 100 < n_traj
        for ts in pc.COST_TERM_SETS:
            eng.params.cost_terms = ts
            eng.push_params()
            for tr, di, where in cases:
                got = eng.cost_eval(tr, di)
                want, parts = pr.evaluate_costs(tr, di, qf, dh, q_min, q_max, ts)
                what = f"n {n} H {H} B {tr.shape[0]} terms {ts}"
                if ts in (pr.TERMS["coll"], pr.TERMS["jl"]):              # the discrete terms: exact
                    assert _bits_equal(got, pr.f32(want)), f"{what}: rows {np.nonzero(got != pr.f32(want))[0][:8]}"
                worst = max(worst, pr.assert_close_nonfinite(got, want, RTOL, what))
                n_inf += int(np.isinf(got).sum())
                if ts & pr.TERMS["stag"]:
                    for r in where["no_motion"]:
                        assert np.isposinf(got[r]), what
                if ts == pr.TERMS["stag"]:
                    for r in where["no_motion_at_goal"]:
                        assert got[r] == 0, what
        eng.close()
    assert n_inf > 0
    print(f"n {n}: worst cost error / scale {worst:.2e}, {n_inf} infinite costs")


# ---- propagates on the planar two-link network ------------------------------------------------------------------------------------------
def _planar_engine(N, H, dt=None, flags=0):
    """The planar two-link network and its two obstacles, k = 2, the fixture's constants; ``dt``: None = the fixture's 0.3."""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import Engine
    fx = load("planar2_c1_K0")
    m = orc.Mlp.from_npz(weights_path("planar2"))
    eng = Engine(2, N, H, 2, max_obs=8, n_kernel_max=pc.KMAX, flags=flags)
    eng.set_mlp(m.W, m.b, act=m.act)
    eng.set_obstacles(scenes.planar2_scene(2))
    eng.params.dt, eng.params.dst_thr = float(fx["dt"] if dt is None else dt), float(fx["dst_thr"])
    eng.push_params()
    eng.set_ds(fx["qf"])
    eng.set_cost(fx["dh_params"], fx["cost_q_min"], fx["cost_q_max"])
    return eng, fx


def test_best_takes_the_first_of_shared_minima():
    """N = 1000, joint-limit cost alone: rollouts 0 .. 299 cost 100, the others 0.  The first minimum is rollout 300; rollouts 556
    and 812 have the same cost and go through the same reduction slot (t mod 256 = 44)."""
    N = 1000
    eng, fx = _planar_engine(N, 2, 0.01)
    eng.params.cost_terms = pr.TERMS["jl"]
    eng.push_params()
    eng.propagate(pc.best_case(N, 300))
    r = eng.get_rollouts()
    cost = eng.cost()
    want, _ = pr.evaluate_costs(r["all_traj"], r["closest_dist_all"], fx["qf"], fx["dh_params"], fx["cost_q_min"], fx["cost_q_max"], pr.TERMS["jl"])
    assert _bits_equal(cost, pr.f32(want))
    assert (cost[:300] == 100).all() and (cost[300:] == 0).all()
    assert not _bits_equal(r["qdot"][300], r["qdot"][556]) and not _bits_equal(r["qdot"][300], r["qdot"][812])
    assert _bits_equal(eng.get_qdot("best"), r["qdot"][300])
    e = rel_err(eng.get_qdot("weighted"), pr.get_qdot(cost, r["qdot"], "weighted"), OWN)
    assert e <= W_TOL, f"weighted qdot {e:.2e}"
    eng.close()


def _propagated(N, K, p, seed):
    """An H = 3 propagate from N random starts with K sampled kernels and RBF norm p -> (engine, rollouts)."""
    eng, _ = _planar_engine(N, 3)
    eng.params.rbf_p = float(p)
    eng.push_params()
    rng = np.random.RandomState(seed)
    eng.set_policy_samples(rng.uniform(-3, 3, (N, K, 2)).astype(F32), rng.uniform(0.05, 0.5, (N, K)).astype(F32), rng.standard_normal((N, K, 2)).astype(F32))
    eng.propagate(pc.planar_starts(N, seed))
    return eng, eng.get_rollouts()


def _gates(r):
    """thr_dist, thr_dot taken from the device's own floats (so that the gates are exact comparisons): the median distance and the
    0.7 quantile of the dot products, raised where needed so that state (N - 1, 0) passes -- a scan that lost the last rollout shows."""
    d, dots = r["closest_dist_all"], r["dot_products"]
    up = lambda x: float(np.nextafter(F32(x), F32(np.inf)))
    return up(max(np.median(d), d[-1, 0])), up(max(np.quantile(dots, 0.7), dots[-1, 0]))


def _check_candidates_without_kernels(eng, r):
    N, H, n = r["all_traj"].shape
    thr_dist, thr_dot = _gates(r)
    gated, _, cand = pr.check_traj_for_kernels(r["all_traj"], r["closest_dist_all"], r["dot_products"], np.zeros((0, n)), np.zeros(0), thr_dist, 0.0, thr_dot)
    th_want, q_want = np.argwhere(cand).astype(np.int32), r["all_traj"][cand]
    count = int(cand.sum())
    assert cand[-1, 0] and 0 < count < N * H
    for cap in (None, 0, 5, count):
        q, th, total = eng.kernel_candidates(thr_dist, 0.0, thr_dot, np.zeros((0, n), F32), np.zeros(0, F32), 0, cap=cap)
        m = count if cap is None else min(cap, count)
        assert total == count, f"cap {cap}: count {total} != {count}"
        assert np.array_equal(th, th_want[:m]) and _bits_equal(q, q_want[:m]), f"cap {cap}"


def _check_candidates_with_kernels(eng, r, K, p, seed):
    N, H, n = r["all_traj"].shape
    thr_dist, thr_dot = _gates(r)
    rng = np.random.RandomState(seed)
    mu_c, sg_c = rng.uniform(-3, 3, (K, n)).astype(F32), rng.uniform(0.05, 0.5, K).astype(F32)
    args = (r["all_traj"], r["closest_dist_all"], r["dot_products"], mu_c, sg_c)
    gated, rbf, _ = pr.check_traj_for_kernels(*args, thr_dist, 0.0, thr_dot, p)
    v = np.sort(rbf[gated])
    thr_kernel = float(F32(0.5 * (v[v.size // 2 - 1] + v[v.size // 2])))       # between the two middle values
    _, _, cand = pr.check_traj_for_kernels(*args, thr_dist, thr_kernel, thr_dot, p)
    near = gated & (np.abs(rbf - thr_kernel) <= 2e-5 * thr_kernel)
    assert near.sum() <= 0.01 * gated.sum(), f"{int(near.sum())} of {int(gated.sum())} gated states straddle thr_kernel"
    q, th, total = eng.kernel_candidates(thr_dist, thr_kernel, thr_dot, mu_c, sg_c, K)
    assert total == th.shape[0] and abs(total - int(cand.sum())) <= int(near.sum())
    keep = ~near[th[:, 0], th[:, 1]]
    want = cand & ~near
    assert 0.2 * gated.sum() < want.sum() < 0.8 * gated.sum()
    assert np.array_equal(th[keep], np.argwhere(want).astype(np.int32)), "candidate set or order"
    assert _bits_equal(q[keep], r["all_traj"][want])
    print(f"N {N} n {n} p {p}: {int(gated.sum())} gated, {total} candidates, {int(near.sum())} left out at the threshold")


@pytest.mark.parametrize("N", [257, 1025, 1300])
def test_candidates_without_kernels(N):
    eng, r = _propagated(N, 0, 2, N)
    _check_candidates_without_kernels(eng, r)
    eng.close()


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("N", [257, 1025, 1300])
def test_candidates_with_kernels(N, p):
    eng, r = _propagated(N, 3, p, N + p)
    _check_candidates_with_kernels(eng, r, 3, p, N + p)
    eng.close()


def test_candidates_three_joints_unfused():
    """n_dof = 3 (k_modulate<3>, k_cand_flags<3>) on the unfused step, with a three-joint network of the test's own making: torch's
    default initialisation, seeded, two hidden layers of 256.  What it computes does not matter here: the gates compare the device's own
    floats and the RBF values are re-derived in float64 from the device's states."""
    from optimalmodulationds_amd import _lib
    from optimalmodulationds_amd.engine import Engine
    n, N, H, K = 3, 257, 3, 3
    rng = np.random.RandomState(33)
    dims = [3 * (n + 3), 256, 256, n]
    W = [rng.uniform(-1, 1, (dims[i + 1], dims[i])).astype(F32) / F32(np.sqrt(dims[i])) for i in range(3)]
    b = [rng.uniform(-1, 1, dims[i + 1]).astype(F32) / F32(np.sqrt(dims[i])) for i in range(3)]
    b[-1] = (b[-1] + 1).astype(F32)
    eng = Engine(n, N, H, 2, max_obs=8, n_kernel_max=pc.KMAX, flags=_lib.FLAG_UNFUSED_STEP)
    eng.set_mlp(W, b)
    eng.set_obstacles(np.c_[rng.uniform(-2, 2, (5, 3)), np.full(5, 0.3)].astype(F32))
    eng.params.dt, eng.params.dst_thr = 0.3, 0.25
    eng.push_params()
    eng.set_ds(np.array([1.0, -0.5, 0.5], F32))
    eng.set_policy_samples(rng.uniform(-3, 3, (N, K, n)).astype(F32), rng.uniform(0.05, 0.5, (N, K)).astype(F32), rng.standard_normal((N, K, n)).astype(F32))
    eng.propagate(rng.uniform(-3, 3, (N, n)).astype(F32))
    r = eng.get_rollouts()
    assert all(np.isfinite(v).all() for v in r.values())
    _check_candidates_without_kernels(eng, r)
    _check_candidates_with_kernels(eng, r, K, 2, 5)
    eng.close()


# ---- row gather and layouts --------------------------------------------------------------------------------------------------------------
def test_rollout_rows_any_index_list():
    """K = 3 of n_kernel_max = 50: the kernel values sit in a slab of leading dimension 50, not 3."""
    N = 1300
    eng, r = _propagated(N, 3, 2, 77)
    assert r["kernel_val_all"].shape == (N, 3, 3) and np.abs(r["kernel_val_all"]).max() > 0
    rng = np.random.RandomState(3)
    for t in ([0], [N - 1], list(range(N - 1, N - 40, -3)), [5, 5, 1299, 5, 0, 1299, 256, 255, 1024, 1023, 256], rng.randint(0, N, 300).tolist()):
        rows = eng.get_rollout_rows(t)
        assert set(rows) == set(r)
        for key, full in r.items():
            assert _bits_equal(rows[key], full[np.asarray(t)]), f"{key}, {len(t)} indices starting {t[:4]}"
    eng.close()


@pytest.mark.parametrize("N", [1, 31, 33, 257])
@pytest.mark.parametrize("K,n", [(1, 1), (33, 1), (11, 3)])
def test_policy_samples_round_trip(N, K, n):
    """k_transpose on partial 32 x 32 tiles in both directions: K n in {1, 33} columns, N rows."""
    from optimalmodulationds_amd.engine import Engine
    rng = np.random.RandomState(N + K)
    eng = Engine(n, N, 1, 1, max_obs=1, n_kernel_max=pc.KMAX)
    mu, sg, al = rng.standard_normal((N, K, n)).astype(F32), rng.standard_normal((N, K)).astype(F32), rng.standard_normal((N, K, n)).astype(F32)
    eng.set_policy_samples(mu, sg, al)
    gmu, gsg, gal = eng.get_policy_samples()
    assert _bits_equal(gmu, mu) and _bits_equal(gsg, sg) and _bits_equal(gal, al)
    eng.close()
