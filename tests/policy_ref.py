"""Float64 restatement of the selections and reductions around the network, plain numpy, no GPU: what k_cost, k_cost_sum, k_weights,
k_policy_sums, k_update_inputs, k_cand_* (csrc/rollout_kernels.hip), omds_apply_update (csrc/update.hip) and topk_row
(csrc/topk_device.h) must produce.  tests/test_gpu_policy_edges.py and tests/test_gpu_topk.py compare the device with these
functions; tests/test_policy_edges_cpu.py checks the functions themselves against the fp32 oracle (oracle/omds_oracle.py) and shows
that deliberately wrong versions of them miss the bars on the inputs the device is given.

Written from the formulas, not from the kernels:
    cost      total = 10 |q_H - qf|  +  100 #{h : d_h < 0}  +  100 [any q outside (q_min, q_max)]
                      +  10 (10 |q_H - qf|) nan_to_num(1 / |q_0 - q_H|)  +  10 sum_links |p_link(q_H) - p_link(qf)|
              p_link = the modified-DH frame of joint i applied to (a_{i+1}, 0, 0); nan_to_num is float32's (1 / 0 -> FLT_MAX)
    weights   beta = mean(cost) / 50,  w = exp(-cost / beta) / sum
    update    kernel kappa moves when  mean_t max_h(phi act) > ker_thr  (and, unless NO_BASE_MASK, mean_h phi[0, h] > ker_thr);
              max over h with torch's rule (a NaN wins); theta <- (1 - rate) theta + rate sum_t w theta_t
    qdot      'best': row of the FIRST smallest cost; 'weighted': sum_t w qdot_t
    candidates   states with d < thr_dist and dot < thr_dot whose largest RBF value exp(-sigma |q - mu|_p^2) is < thr_kernel
    top-k     the rule at the top of csrc/topk_device.h

Everything is computed in float64 from the float32 inputs; the caller casts to float32 at the end (``f32``), so a value beyond
float32's range is an expected ``inf``.  The arguments ``keep`` / ``strict`` exist for the sensitivity checks only: ``keep`` [N] bool
makes every sum over rollouts see the kept ones alone (counts stay N), the way a kernel that drops a tail would."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
TERMS = {"goal": 1, "coll": 2, "jl": 4, "stag": 8, "fk": 16}       # include/omds.h: OMDS_COST_*
COST_ALL, COST_TOY = 31, 1 | 2 | 8
KVAL_TIMES_ACT, NO_BASE_MASK = 1, 2                                 # include/omds.h: OMDS_VARIANT_*


def f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(a):
    """The float32 a float64 result is compared as: beyond float32's range it is +-inf."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


# ---- forward kinematics and cost -----------------------------------------------------------------------------------------------------
def link_endpoints(q, dh):
    """q [B, n], dh [n + 1, 4] rows (d, theta, a, alpha), modified DH (Craig): T_i = Rx(alpha) Tx(a) Rz(q + theta) Tz(d).
    -> [B, n, 3]: the frame of joint i applied to (a_{i+1}, 0, 0)."""
    q, dh = f64(q), f64(dh)
    B, n = q.shape
    T = np.broadcast_to(np.eye(4), (B, 4, 4)).copy()
    pts = np.zeros((B, n, 3))
    for i in range(n):
        d, th, a, al = dh[i]
        sa, ca = np.sin(al), np.cos(al)
        sq, cq = np.sin(q[:, i] + th), np.cos(q[:, i] + th)
        M = np.zeros((B, 4, 4))
        M[:, 0, 0], M[:, 0, 1], M[:, 0, 3] = cq, -sq, a
        M[:, 1, 0], M[:, 1, 1], M[:, 1, 2], M[:, 1, 3] = sq * ca, cq * ca, -sa, -d * sa
        M[:, 2, 0], M[:, 2, 1], M[:, 2, 2], M[:, 2, 3] = sq * sa, cq * sa, ca, d * ca
        M[:, 3, 3] = 1.0
        T = T @ M
        pts[:, i] = T[:, :3, 0] * dh[i + 1, 2] + T[:, :3, 3]
    return pts


def evaluate_costs(all_traj, closest_dist_all, qf, dh, q_min, q_max, terms=COST_ALL):
    """all_traj [B, H, n], closest_dist_all [B, H]; ``terms``: a bit set of TERMS -> (total [B] float64, the five parts)."""
    tr, dist, qf = f64(all_traj), f64(closest_dist_all), f64(qf)
    q0, qe = tr[:, 0, :], tr[:, -1, :]
    goal = 10.0 * np.sqrt(((qe - qf) ** 2).sum(axis=1))
    coll = 100.0 * (dist < 0).sum(axis=1)
    jl = 100.0 * ((tr < f64(q_min)) | (tr > f64(q_max))).any(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sqrt(((q0 - qe) ** 2).sum(axis=1))
    inv = np.where(np.isnan(inv), 0.0, np.clip(inv, -FLT_MAX, FLT_MAX))       # float32's nan_to_num
    stag = 10.0 * goal * inv
    diff = link_endpoints(qe, dh) - link_endpoints(qf[None, :], dh)
    fk = 10.0 * np.sqrt((diff ** 2).sum(axis=2)).sum(axis=1)
    parts = dict(goal=goal, coll=coll, jl=jl, stag=stag, fk=fk)
    total = np.zeros(tr.shape[0])
    for name in ("goal", "coll", "jl", "stag", "fk"):
        if terms & TERMS[name]:
            total = total + parts[name]
    return total, parts


# ---- weights, update, qdot -----------------------------------------------------------------------------------------------------------
def _sum_t(x, keep):
    x = f64(x)
    return x.sum(axis=0) if keep is None else x[np.asarray(keep, bool)].sum(axis=0)


def mppi_weights(cost, keep=None):
    """-> normalised weights [N] float64 (a rollout outside ``keep`` has weight 0)."""
    c = f64(cost)
    beta = _sum_t(c, keep) / c.shape[0] / 50.0
    w = np.exp(-c / beta)
    if keep is not None:
        w = np.where(np.asarray(keep, bool), w, 0.0)
    return w / w.sum()


def _max_h(prod):
    """max over axis 1 with torch's rule: a NaN anywhere along h makes the maximum NaN."""
    nan = np.isnan(prod).any(axis=1)
    return np.where(nan, np.nan, np.where(np.isnan(prod), -np.inf, prod).max(axis=1))


def update_mask(kernel_val_all, kernel_activations, ker_thr, variant=0, keep=None, strict=True):
    """-> (mask [K] bool, m1 [K], m2 [K]): the two means the mask compares with ker_thr (a NaN mean compares false)."""
    kv, act = f64(kernel_val_all), f64(kernel_activations)
    prod = kv if variant & KVAL_TIMES_ACT else kv * act[:, :, None]
    m1 = _sum_t(_max_h(prod), keep) / kv.shape[0]
    m2 = kv[0].sum(axis=0) / kv.shape[1]
    thr = float(np.float32(ker_thr))
    with np.errstate(invalid="ignore"):
        gt = (lambda a: a > thr) if strict else (lambda a: a >= thr)
        mask = gt(m1) & (gt(m2) if not variant & NO_BASE_MASK else True)
    return mask, m1, m2


def shift_policy_means(cost, kernel_val_all, kernel_activations, mu_c, sigma_c, alpha_c, mu_tmp, sigma_tmp, alpha_tmp, ker_thr, rate,
                       variant=0, keep=None, strict=True):
    """-> (mu_c, sigma_c, alpha_c after the update, mask [K], weights [N]); K = mu_c.shape[0] kernels."""
    w = mppi_weights(cost, keep)
    K = np.asarray(mu_c).shape[0]
    if K == 0:
        return f64(mu_c), f64(sigma_c), f64(alpha_c), np.zeros(0, bool), w
    mask, _, _ = update_mask(f64(kernel_val_all)[:, :, :K], kernel_activations, ker_thr, variant, keep, strict)
    u = np.where(mask, float(np.float32(rate)), 0.0)
    mu_s = (w[:, None, None] * f64(mu_tmp)[:, :K]).sum(axis=0)
    sg_s = (w[:, None] * f64(sigma_tmp)[:, :K]).sum(axis=0)
    al_s = (w[:, None, None] * f64(alpha_tmp)[:, :K]).sum(axis=0)
    return ((1 - u)[:, None] * f64(mu_c) + u[:, None] * mu_s, (1 - u) * f64(sigma_c) + u * sg_s,
            (1 - u)[:, None] * f64(alpha_c) + u[:, None] * al_s, mask, w)


def get_qdot(cost, qdot, mode="best", keep=None):
    if mode == "best":
        return f64(qdot)[int(np.argmin(f64(cost)))]          # numpy's argmin: the first of equal minima
    return (mppi_weights(cost, keep)[:, None] * f64(qdot)).sum(axis=0)


# ---- navigation-kernel candidates ---------------------------------------------------------------------------------------------------
def check_traj_for_kernels(all_traj, dist_all, dots_all, mu_c, sigma_c, thr_dist, thr_kernel, thr_dot, p=2):
    """-> (gated [N, H] bool: d < thr_dist and dot < thr_dot; rbf_max [N, H] float64: the largest RBF value of every gated state, NaN
    elsewhere and without kernels; cand [N, H] bool: gated and (no kernels, or rbf_max < thr_kernel)).  The candidate list is
    all_traj[cand] -- rollout-major."""
    tr = f64(all_traj)
    gated = (f64(dist_all) < float(np.float32(thr_dist))) & (f64(dots_all) < float(np.float32(thr_dot)))
    rbf = np.full(gated.shape, np.nan)
    K = np.asarray(mu_c).shape[0]
    if K == 0:
        return gated, rbf, gated.copy()
    diff = np.abs(tr[gated][:, None, :] - f64(mu_c)[None])            # [G, K, n]
    nrm = (diff ** float(p)).sum(axis=2) ** (1.0 / float(p))
    rbf[gated] = np.exp(-f64(sigma_c)[None] * nrm ** 2).max(axis=1)
    with np.errstate(invalid="ignore"):
        cand = gated & (rbf < float(np.float32(thr_kernel)))
    return gated, rbf, cand


# ---- top-k -----------------------------------------------------------------------------------------------------------------------------
def topk_ref(row, k):
    """Indices of the k smallest entries of ``row``, ordered by (value, index) with -0 equal to +0; a NaN is never picked; the
    positions beyond the pickable entries hold index 0."""
    order = sorted((float(v) + 0.0, i) for i, v in enumerate(np.asarray(row).tolist()) if v == v)
    out = [i for _, i in order[:k]]
    return np.array(out + [0] * (k - len(out)), np.int32)


# ---- comparison ------------------------------------------------------------------------------------------------------------------------
def err_with_nonfinite(got, want, floor=1.0):
    """helpers.rel_err of the FINITE entries of ``want`` cast to float32 (max |got - want| / max(floor, max |want|)), after asserting
    that the non-finite ones -- NaN, +inf, -inf -- sit at the same positions of ``got`` with the same sign.  helpers.rel_err alone
    turns inf - inf into a failure."""
    from helpers import rel_err
    got, want32 = np.asarray(got), f32(want)
    assert got.shape == want32.shape, (got.shape, want32.shape)
    for name, fn in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        a, b = fn(got), fn(want32)
        assert np.array_equal(a, b), f"{name} pattern differs: {int(a.sum())} got, {int(b.sum())} expected, first at {np.argwhere(a != b)[0]}"
    fin = np.isfinite(want32)
    return rel_err(got[fin], f64(want)[fin], floor)


def assert_close_nonfinite(got, want, tol, what, floor=1.0):
    e = err_with_nonfinite(got, want, floor)
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"
    return e
