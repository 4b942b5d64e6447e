"""The moving frame on the CPU (include/omds.h: THE MOVING FRAME; csrc/obstacle_horizon.hip: omds_moving_frame_velocity).

1. The host definition against a float64 restatement.  "1e-6 relative" is relative to the SCALE of each quantity, the only meaning
   an fp32 sum of signed terms admits: rate = sum_j w_j sum_a gradx_j[n+a] vel_j[a] cancels, so its error is bounded by
   (roundings) x sum |terms|, not by a fraction of the result.  The roundings: softmax_k drow_j and the subtraction of the maximum
   (|argument| <= 3: 2 x 1.2e-7 absolute = relative in w), expf and the division (3 x 6e-8), the fmaf chains (k + 3 steps x 6e-8):
   about 9e-7 in the worst case.  So |rate - rate64| <= 1e-6 S with S = sum_j w_j sum_a |gradx_j[n+a] vel_j[a]|, likewise
   |g_c - g64_c| <= 1e-6 A_c with A_c = sum_j w_j |gradx_j[c]|, and to first order in those for qo_c = -rate g_c / gn^2:
   |qo_c - qo64_c| <= 1e-6 (S |g_c| + |rate| A_c + 2 |rate| |g_c| |A| / gn) / gn^2 (the clamp kept out of the way: it has its own case).
2. A numpy restatement of the whole step in the moving frame (frame_step / frame_propagate), built from the oracle's pieces.  With
   zero velocities it must be orc.propagate EXACTLY: that pins the restatement tests/test_gpu_moving_frame.py leans on.
3. The surface: the new symbols, and the argument checks of the context-free entry point."""
import ctypes as C

import numpy as np
import pytest

from helpers import weights_path
from oracle import omds_oracle as orc

F32 = np.float32
DT, K_CLOSEST, K_POLICY = 0.5, 5, 3
MARGIN = 1e-5     # rows whose branch quantities lie this close to their threshold may take the other branch on the device


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def frame_quantities(grad, d, w, sort_idx, vel, n, max_speed=1.0):
    """rate [N] and qo [N, n] from the full gradient rows grad [N*k, n+pd], distances d [N, k], softmax weights w [N, k], the
    selected obstacles sort_idx [N, k] and the velocities vel [O, 3]; also the blended gradient and its norm."""
    N, k = d.shape
    pd = grad.shape[1] - n
    g = (grad[:, :n].reshape(N, k, n) * w[:, :, None]).sum(axis=1).astype(F32)
    vsel = np.asarray(vel, F32)[sort_idx][:, :, :pd]
    sj = (grad[:, n:].reshape(N, k, pd) * vsel).sum(axis=2).astype(F32)
    rate = (sj * w).sum(axis=1).astype(F32)
    gn = np.sqrt((g * g).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = (rate / gn).astype(F32)
        r[(gn == 0) | ~np.isfinite(r)] = 0
        r = np.clip(r, -F32(max_speed), F32(max_speed)).astype(F32)
        qo = (-r[:, None] * (g / gn[:, None]).astype(F32)).astype(F32)
    qo[gn == 0] = 0
    return rate, qo, g, gn


def network_rows(m, q, obs, k, ignored_links, softmax_k=-10.0):
    """MPPI.distance_repulsion_nn as the oracle restates it (orc.distance_repulsion_nn, line for line), keeping what the frame
    needs: the FULL gradient rows [N*k, n+pd], the distances [N, k], the weights and the selected obstacles."""
    q = np.asarray(q, dtype=F32)
    n_in = q.shape[0]
    nn_input, mind = orc.pass1_mindist(m, q, obs, ignored_links)
    sort_idx = np.argsort(mind, axis=1, kind="stable")[:, :k]
    rows = (np.arange(n_in)[:, None] + sort_idx * n_in).reshape(-1)
    nn_in2 = nn_input[rows]
    y, grad, min_idx = orc.mlp_vjp_argmin(m, nn_in2[:, :-1])
    if m.out_channels == 9:
        y = y / F32(100)
    y = y - nn_in2[:, -1:]
    d = y[np.arange(y.shape[0]), min_idx].reshape(n_in, k)
    e = np.exp((F32(softmax_k) * d) - (F32(softmax_k) * d).max(axis=1, keepdims=True))
    w = (e / e.sum(axis=1, keepdims=True)).astype(F32)
    return grad, d, w, sort_idx


def frame_step(m, q_prev, qf, obs, vel, k, ignored_links, mu_tmp, sigma_tmp, alpha_tmp, prm, max_speed=1.0):
    """One horizon step in the moving frame: orc.modulation_step with v_rel = v - qo in the dot product and in the total velocity,
    and qo added back behind the collision handling.  With vel = 0 every line is modulation_step's."""
    q_prev = np.asarray(q_prev, dtype=F32)
    qf = np.asarray(qf, dtype=F32)
    n = q_prev.shape[1]
    K = mu_tmp.shape[1]
    grad, d, w, sort_idx = network_rows(m, q_prev, obs, k, ignored_links, prm.softmax_k)
    rate, qo, g_raw, _ = frame_quantities(grad, d, w, sort_idx, vel, n, max_speed)
    distance_raw = d[:, 0].copy()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if prm.A is None:
            v = orc.lin_ds_velocity(q_prev, qf, prm.lin_thr)
        else:
            v = ((q_prev - qf).astype(F32) @ np.asarray(prm.A, dtype=F32)).astype(F32)
        vnorm = np.sqrt((v * v).sum(axis=1)).reshape(-1, 1)
        v_rel = (v - qo).astype(F32)
        vhat = v_rel / np.sqrt((v_rel * v_rel).sum(axis=1)).reshape(-1, 1)
        distance = (distance_raw - F32(prm.dst_thr)).astype(F32)
        ghat = (g_raw / np.sqrt((g_raw * g_raw).sum(axis=1))[:, None]).astype(F32)
        dot = (ghat * vhat).sum(axis=-1)
        l_vel = orc.generalized_sigmoid(dot, *prm.lvel)
        l_n = orc.generalized_sigmoid(distance, *prm.ln)
        l_nv = l_vel * F32(1) + (F32(1) - l_vel) * l_n
        l_tau = orc.generalized_sigmoid(distance, *prm.ltau)
        if K > 0:
            phi = orc.eval_rbf(q_prev, mu_tmp, sigma_tmp, prm.p)
            pol = (alpha_tmp * phi[:, :, None]).sum(axis=1).astype(F32)
        else:
            phi = np.zeros((q_prev.shape[0], 0), dtype=F32)
            pol = v * F32(0)
        ca = (F32(1) - l_n)[:, None]
        va = (F32(1) - l_vel)[:, None]
        ga_raw = (np.sqrt(np.abs(q_prev - qf)).sum(axis=1) ** 2).clip(0, 1)[:, None].astype(F32)
        ga = ga_raw.copy()
        ga[ga < F32(prm.goal_act_cut)] = 0
        act = ca * va * ga
        v_tot = v_rel + act * pol * vnorm
        u = l_tau[:, None] * v_tot + ((l_nv - l_tau) * (ghat * v_tot).sum(axis=1))[:, None] * ghat
        unorm = np.sqrt((u * u).sum(axis=1)).reshape(-1, 1)
        s = unorm.copy()
        s[s <= F32(prm.norm_clamp)] = 1
        u = orc.nan_to_num(u / s)
        coll = distance < 0
        u[coll] *= F32(prm.coll_slow)
        rep = ghat * vnorm * F32(prm.coll_repulse)
        u[coll] += rep[coll]
        u = (u + qo).astype(F32)
    near = (np.abs(unorm[:, 0] - F32(prm.norm_clamp)) < MARGIN) | (np.abs(distance) < MARGIN) | (np.abs(ga_raw[:, 0] - F32(prm.goal_act_cut)) < MARGIN)
    kval = phi * act if prm.kval_times_act else phi
    return dict(u=u, distance=distance, ghat=ghat, dot=dot.astype(F32), act=act[:, 0].astype(F32), kval=kval.astype(F32), rate=rate, qo=qo,
                near=near, sort_idx=sort_idx)


def frame_propagate(m, q_cur, qf, table, vel, *, N, k, ignored_links, mu_tmp, sigma_tmp, alpha_tmp, prm, dt, max_speed=1.0):
    """MPPI.propagate with step i on slab i - 1 of ``table`` [H, O, 3 or 4] (x, y, [z,] r) in the moving frame of ``vel`` [O, 3]."""
    H, n = table.shape[0], np.asarray(q_cur).shape[-1]
    out = dict(all_traj=np.zeros((N, H, n), F32), closest_dist_all=np.zeros((N, H), F32), dot_products=np.zeros((N, H), F32),
               kernel_activations=np.zeros((N, H), F32), kernel_val_all=np.zeros((N, H, mu_tmp.shape[1]), F32), normal=np.zeros((N, H, n), F32),
               near=np.zeros((N, H), bool))
    out["all_traj"][:, 0] = q_cur
    for i in range(1, H + 1):
        st = frame_step(m, out["all_traj"][:, i - 1], qf, table[i - 1], vel, k, ignored_links, mu_tmp, sigma_tmp, alpha_tmp, prm, max_speed)
        for name, key in (("closest_dist_all", "distance"), ("dot_products", "dot"), ("kernel_activations", "act"), ("kernel_val_all", "kval"),
                          ("normal", "ghat"), ("near", "near")):
            out[name][:, i - 1] = st[key]
        if i < H:
            out["all_traj"][:, i] = out["all_traj"][:, i - 1] + F32(dt) * st["u"]
        if i == 1:
            out["qdot"] = st["u"].copy()
    return out


# ---- the set-ups tests/test_gpu_moving_frame.py runs on the device (conventions of tests/test_gpu_obstacle_horizon.py) ----------------------
def franka_inputs(N, seed=11):
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(seed)
    q_cur = (np.asarray(scenes.FRANKA_Q0, F32) + 0.1 * rng.standard_normal(7)).astype(F32)
    mu = (q_cur + 0.2 * rng.standard_normal((N, K_POLICY, 7))).astype(F32)
    samples = (mu, np.ones((N, K_POLICY), F32), rng.standard_normal((N, K_POLICY, 7)).astype(F32))
    return q_cur, samples


def velocities(O, seed=3):
    return np.random.RandomState(seed).uniform(-0.2, 0.2, (O, 3)).astype(F32)


FRANKA_PRM = orc.Params(dst_thr=0.01)
# route -> (network, N, H, seed of the inputs, seed of the velocities); the Dense case holds 96 x 294 > 24 576 pairs
FRANKA_CASES = {"dense": ("franka", 96, 4, 11, 3), "emit": ("franka", 16, 3, 12, 4), "unfused": ("franka", 32, 3, 12, 4),
                "dense_tanh": ("franka_tanh", 16, 3, 12, 4)}


def franka_case(route):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    kind, N, H, seed, vseed = FRANKA_CASES[route]
    obs = scenes.shelf_scene()
    q_cur, samples = franka_inputs(N, seed)
    vel = velocities(obs.shape[0], vseed)
    return dict(kind=kind, N=N, H=H, obs=obs, q_cur=q_cur, samples=samples, vel=vel, table=predict_obstacle_horizon(obs, vel, H, DT),
                m=orc.Mlp.from_npz(weights_path(kind)), qf=np.asarray(scenes.FRANKA_QF, F32), prm=FRANKA_PRM, dt=DT, k=K_CLOSEST,
                ignored=[0, 1, 2])


def planar7_case(N=64, H=3, O=8, k=2, K=6):
    """The planar-7 set-up of tests/test_gpu_small_step.py (k_step_small: O = 8, k = 2; dt = 0.3, dst_thr = 0.25); planar7.npz reads
    x, y and z, so all three velocity components act."""
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    from test_gpu_small_step import _policy, _scene
    obs = _scene(O)
    q0 = np.zeros(7, F32); q0[0] = np.pi / 2
    qf = np.zeros(7, F32); qf[0] = -np.pi / 2
    rng = np.random.RandomState(3)
    mu_c, sg_c, al_c = _policy(rng, q0, qf, K)
    samples = (np.tile(mu_c, (N, 1, 1)).astype(F32), np.tile(sg_c, (N, 1)).astype(F32),
               (al_c[None] + 0.75 * rng.standard_normal((N, K, 7))).astype(F32))
    vel = velocities(O, seed=6)
    return dict(kind="planar7", N=N, H=H, obs=obs, q_cur=q0, samples=samples, vel=vel, table=predict_obstacle_horizon(obs, vel, H, 0.3),
                m=orc.Mlp.from_npz(weights_path("planar7")), qf=qf, prm=orc.Params(dst_thr=0.25), dt=0.3, k=k, ignored=[], O=O)


def toy_case(H=3):
    """The toy2_arc_K0 set-up of tests/test_toy_variant.py: the planar-point network (d = n + 2), 20 spheres, 100 rollouts, no policy
    kernels.  The restatement's spheres are (x, y, r); the device's carry a z that nothing reads, and vel[:, 2] is not read either."""
    from helpers import load
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    from test_toy_variant import _obs4, toy_prm
    fx = load("toy2_arc_K0")
    N = int(fx["N"])
    obs4 = _obs4(fx)
    vel = velocities(obs4.shape[0], seed=7)
    table4 = predict_obstacle_horizon(obs4, vel * np.array([1, 1, 0], F32), H, float(fx["dt"]))
    empty = (np.zeros((N, 0, 2), F32), np.zeros((N, 0), F32), np.zeros((N, 0, 2), F32))
    return dict(kind="toy2", N=N, H=H, obs=obs4, q_cur=fx["it0_q_cur"].astype(F32), samples=empty, vel=vel, table=table4[:, :, [0, 1, 3]], table4=table4,
                m=orc.Mlp.from_npz(weights_path("toy2")), qf=fx["qf"].astype(F32), prm=toy_prm(fx), dt=float(fx["dt"]), k=int(fx["k"]),
                ignored=[], fx=fx)


def chase_case(N=32, H=16):
    """THE POINT OF IT: one sphere (r = 0.5) starts 2.5 behind the planar-point robot and chases it at 1.5 along the nominal DS's
    direction, faster than the unit speed the rollouts are normalised to.  The rollouts start in a box around (-5, 0); no policy
    kernels; the frame's clamp is 3.  The restatement (CPU): frame off, the closest distance goes below zero within 16 steps for
    32 of 32 rollouts (the least affected reaches -0.023, the worst -0.52); frame on, for none (smallest distance of any rollout
    at any step: 1.19)."""
    c = toy_case(H)
    rng = np.random.RandomState(1)
    q0 = (np.array([-5, 0], F32) + rng.uniform(-1, 1, (N, 2)) * np.array([0.5, 1.0])).astype(F32)
    obs4 = np.array([[-7.5, 0, 0, 0.5]], F32)
    vel = np.array([[1.5, 0, 0]], F32)
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    table4 = predict_obstacle_horizon(obs4, vel, H, c["dt"])
    empty = (np.zeros((N, 0, 2), F32), np.zeros((N, 0), F32), np.zeros((N, 0, 2), F32))
    c.update(N=N, H=H, obs=obs4, q_cur=q0, samples=empty, vel=vel, table=table4[:, :, [0, 1, 3]], table4=table4, max_speed=3.0)
    return c


def restate(c, table=None, vel=None, q_cur=None, max_speed=1.0):
    mu, sg, al = c["samples"]
    return frame_propagate(c["m"], c["q_cur"] if q_cur is None else q_cur, c["qf"], c["table"] if table is None else table,
                           c["vel"] if vel is None else vel, N=c["N"], k=c["k"], ignored_links=c["ignored"], mu_tmp=mu, sigma_tmp=sg,
                           alpha_tmp=al, prm=c["prm"], dt=c["dt"], max_speed=max_speed)


# ---- 1. the host definition ----------------------------------------------------------------------------------------------------------
def _definition64(gradx, drow, vel, n, softmax_k, max_speed):
    g64, d64, v64 = gradx.astype(np.float64), drow.astype(np.float64), vel.astype(np.float64)
    pd = gradx.shape[1] - n
    a = softmax_k * d64
    w = np.exp(a - a.max())
    w /= w.sum()
    g = (g64[:, :n] * w[:, None]).sum(axis=0)
    terms = g64[:, n:] * v64[:, :pd] * w[:, None]
    rate, S = terms.sum(), np.abs(terms).sum()
    A = (np.abs(g64[:, :n]) * w[:, None]).sum(axis=0)
    gn = np.linalg.norm(g)
    r = float(np.clip(rate / gn, -max_speed, max_speed)) if gn > 0 else 0.0
    qo_scale = (S * np.abs(g) + abs(rate) * A + 2 * abs(rate) * np.abs(g) * np.linalg.norm(A) / gn) / gn ** 2 if gn > 0 else np.ones(n)
    return rate, (-r * g / gn if gn > 0 else np.zeros(n)), S, gn, g, qo_scale


@pytest.mark.parametrize("n,d,k", [(7, 10, 5), (2, 4, 2), (7, 10, 1)])
def test_definition_against_float64(n, d, k):
    from optimalmodulationds_amd.engine import moving_frame_velocity
    rng = np.random.RandomState(100 + 10 * n + k)
    worst = 0.0
    for _ in range(200):
        gradx = rng.standard_normal((k, d)).astype(F32)
        drow = rng.uniform(-0.05, 0.3, k).astype(F32)
        vel = rng.uniform(-0.2, 0.2, (k, 3)).astype(F32)
        rate, qo = moving_frame_velocity(gradx, drow, vel, n, softmax_k=-10.0, max_speed=1e6)
        rate64, qo64, S, gn, g, qo_scale = _definition64(gradx, drow, vel, n, -10.0, 1e6)
        e_rate = abs(rate - rate64) / S
        e_qo = float((np.abs(qo - qo64) / qo_scale).max())
        worst = max(worst, e_rate, e_qo)
        assert e_rate <= 1e-6 and e_qo <= 1e-6, (e_rate, e_qo)
        # g . qo = -rate while the clamp does not bite: to rounding, at the scale of the sums behind both sides
        assert abs(rate64 / gn) < 1e6
        assert abs(float(g @ qo.astype(np.float64)) + rate64) <= 1e-6 * (S + float(np.abs(g) @ qo_scale))
    print(f"n = {n}, d = {d}, k = {k}: worst error / scale {worst:.2e}")


def test_definition_exact_cases():
    from optimalmodulationds_amd.engine import moving_frame_velocity
    rng = np.random.RandomState(5)
    gradx = rng.standard_normal((5, 10)).astype(F32)
    drow = rng.uniform(0, 0.3, 5).astype(F32)
    vel = rng.uniform(-0.2, 0.2, (5, 3)).astype(F32)
    rate, qo = moving_frame_velocity(gradx, drow, np.zeros((5, 3), F32), 7)
    assert rate == 0.0 and not qo.any(), "vel = 0"
    flat = gradx.copy()
    flat[:, :7] = 0
    rate, qo = moving_frame_velocity(flat, drow, vel, 7)
    assert rate != 0.0 and not qo.any() and np.isfinite(qo).all(), "gn = 0"
    # the clamp: 100 x the velocities ask for more than max_speed
    rate, qo = moving_frame_velocity(gradx, drow, 100 * vel, 7, max_speed=0.25)
    rate64, _, _, gn, _, _ = _definition64(gradx, drow, 100 * vel, 7, -10.0, 0.25)
    assert abs(rate64 / gn) > 0.25 and abs(float(np.linalg.norm(qo.astype(np.float64))) - 0.25) <= 0.25 * 1e-6
    rate1, qo1 = moving_frame_velocity(gradx, drow, 100 * vel, 7, max_speed=0.0)      # <= 0: the default 1.0
    assert abs(float(np.linalg.norm(qo1.astype(np.float64))) - min(1.0, abs(rate64 / gn))) <= 1e-6 and rate1 == rate
    # planar points (d = n + 2) do not read vel[:, 2]
    g4 = rng.standard_normal((2, 4)).astype(F32)
    v = rng.uniform(-0.2, 0.2, (2, 3)).astype(F32)
    v2 = v.copy()
    v2[:, 2] = 7.0
    a, b = moving_frame_velocity(g4, drow[:2], v, 2), moving_frame_velocity(g4, drow[:2], v2, 2)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[0] != 0.0


# ---- 2. the restatement is the oracle at rest ----------------------------------------------------------------------------------------
def test_restatement_at_rest_is_the_oracle():
    from optimalmodulationds_amd import scenes
    N, H = 8, 3
    obs = scenes.shelf_scene()
    q_cur, (mu, sg, al) = franka_inputs(N)
    m = orc.Mlp.from_npz(weights_path("franka"))
    ref = orc.propagate(m, q_cur, scenes.FRANKA_QF, obs, N=N, H=H, dt=DT, k=K_CLOSEST, ignored_links=[0, 1, 2], mu_tmp=mu, sigma_tmp=sg,
                        alpha_tmp=al, prm=FRANKA_PRM)
    got = frame_propagate(m, q_cur, scenes.FRANKA_QF, np.tile(obs, (H, 1, 1)), np.zeros((obs.shape[0], 3), F32), N=N, k=K_CLOSEST,
                          ignored_links=[0, 1, 2], mu_tmp=mu, sigma_tmp=sg, alpha_tmp=al, prm=FRANKA_PRM, dt=DT)
    for name, want in (("all_traj", ref.all_traj), ("closest_dist_all", ref.closest_dist_all), ("dot_products", ref.dot_products),
                       ("kernel_activations", ref.kernel_activations), ("kernel_val_all", ref.kernel_val_all), ("normal", ref.norm_basis_n),
                       ("qdot", ref.qdot)):
        assert np.array_equal(got[name], want), name
    # ... and it moves once the spheres do
    moving = frame_propagate(m, q_cur, scenes.FRANKA_QF, np.tile(obs, (H, 1, 1)), velocities(obs.shape[0]), N=N, k=K_CLOSEST,
                             ignored_links=[0, 1, 2], mu_tmp=mu, sigma_tmp=sg, alpha_tmp=al, prm=FRANKA_PRM, dt=DT)
    assert not np.array_equal(moving["qdot"], ref.qdot) and np.array_equal(moving["closest_dist_all"][:, 0], ref.closest_dist_all[:, 0])


@pytest.mark.parametrize("route", sorted(FRANKA_CASES))
def test_franka_cases_stay_clear_of_their_branch_thresholds(route):
    """The seeds of the device test's cases: the free-running restatement excludes no row (|u| - norm_clamp, distance and
    ga - goal_act_cut all farther than 1e-5 from zero), so the device's rows, a rounding away, have the same room."""
    c = franka_case(route)
    r = restate(c)
    assert not r["near"].any(), int(r["near"].sum())
    assert np.isfinite(r["all_traj"]).all()


@pytest.mark.parametrize("case", ["planar7", "toy"])
def test_small_scene_cases_stay_clear_of_their_branch_thresholds(case):
    c = planar7_case() if case == "planar7" else toy_case()
    r = restate(c)
    assert not r["near"].any(), int(r["near"].sum())
    assert np.isfinite(r["all_traj"]).all()
    assert not np.array_equal(r["qdot"], restate(c, vel=np.zeros_like(c["vel"]))["qdot"]), "the frame acts on this case"


def test_chasing_sphere_on_the_restatement():
    """Fixes the scene of the device test: without the frame most rollouts are hit, with it none, both with clear margin."""
    c = chase_case()
    off = restate(c, vel=np.zeros_like(c["vel"]))["closest_dist_all"].min(axis=1)
    on = restate(c, max_speed=c["max_speed"])["closest_dist_all"].min(axis=1)
    print("frame off: share hit", float((off < 0).mean()), "least / most", float(off.max()), float(off.min()), "| frame on: share hit",
          float((on < 0).mean()), "smallest distance", float(on.min()))
    assert (off < 0).mean() >= 0.9 and off.max() < -0.01
    assert (on < 0).mean() == 0.0 and on.min() > 0.5


# ---- 3. the surface ------------------------------------------------------------------------------------------------------------------
def test_symbols_and_argument_checks():
    from optimalmodulationds_amd import _lib as L
    lib = L.load()
    for name in ("omds_moving_frame_velocity", "omds_set_obstacle_frame", "omds_get_obstacle_frame", "omds_approach_rate"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    g, dr, v = np.ones((2, 10), F32), np.zeros(2, F32), np.zeros((2, 3), F32)
    rate, qo = np.zeros(1, F32), np.zeros(7, F32)
    f = lib.omds_moving_frame_velocity
    ok = (7, 10, 2, L.fptr(g), L.fptr(dr), L.fptr(v), C.c_float(-10.0), C.c_float(1.0), L.fptr(rate), L.fptr(qo))
    assert f(*ok) == 0
    bad = [dict({0: 0}), dict({0: 8}), dict({1: 8}), dict({1: 11}), dict({2: 0}), dict({3: None}), dict({4: None}), dict({5: None}),
           dict({8: None}), dict({9: None}), dict({7: C.c_float(float("nan"))})]
    for change in bad:
        args = list(ok)
        for i, val in change.items():
            args[i] = val
        assert f(*args) == 1, change          # OMDS_ERR_INVALID_ARG
        assert b"omds_moving_frame_velocity" in lib.omds_last_error(None)
    assert lib.omds_set_obstacle_frame(None, 1, C.c_float(1.0)) == 1 and lib.omds_approach_rate(None, None, 1, None, None) == 1
