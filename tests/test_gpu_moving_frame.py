"""The moving frame on the device (include/omds.h: THE MOVING FRAME; csrc/step_device.h: modulate_core<.., FRAME>): with
set_obstacle_frame(True) and a motion horizon every step of a propagate modulates relative to the obstacle's velocity as the joints see
it and adds that velocity back.  The yardstick is the numpy restatement of tests/test_moving_frame_cpu.py (pinned there to the oracle
at rest), evaluated step by step at the device's OWN states (teacher-forced) on the slab that step saw; the bar is the project's
plain 1e-5 on every row.  Conventions of tests/test_gpu_obstacle_horizon.py: Franka weights, the shelf scene, dt = 0.5, K = 3 injected
samples, ignored_links = 0b111, velocities uniform in +-0.2."""
import numpy as np
import pytest

from helpers import RTOL, assert_close, plain_bar, weights_path
from oracle import omds_oracle as orc
from test_moving_frame_cpu import (DT, K_CLOSEST, chase_case, frame_quantities, frame_step, franka_case, franka_inputs, planar7_case,
                                   toy_case, velocities)

pytestmark = pytest.mark.gpu

KEYS = ("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal")


def _franka_engine(c, flags=0, N=None, H=None):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import Engine
    e = Engine(7, N or c["N"], H or c["H"], K_CLOSEST, max_obs=512, flags=flags)
    e.set_mlp(c["m"].W, c["m"].b, act="tanh" if c["kind"].endswith("tanh") else "relu")
    e.set_obstacles(c["obs"])
    e.params.dt = DT
    e.params.dst_thr = 0.01
    e.params.ignored_links = 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_policy_samples(*c["samples"])
    return e


def _planar7_engine(c):
    from test_gpu_small_step import _engine
    e = _engine(c["N"], c["H"], c["O"], c["k"])[0]
    e.set_policy_samples(*c["samples"])
    return e


def _toy_engine(c):
    from test_toy_variant import _engine
    e = _engine(c["fx"], c["N"], c["H"])
    e.set_obstacles(c["obs"])
    e.set_policy_samples(*c["samples"])
    return e


def _run(e, c, frame=True, motion=True, max_speed=None):
    if motion:
        e.set_obstacle_motion(c["vel"])
    e.set_obstacle_frame(frame, max_speed)
    e.prof_enable(1)
    e.propagate(c["q_cur"])
    A = e.get_rollouts()
    A["kernel"] = e.prof_read_ex()[3]
    return A


def _assert_steps(A, c, what, max_speed=1.0):
    """Every step of the device's rollouts A against the restatement at A's own states on that step's slab."""
    mu, sg, al = c["samples"]
    H, dt = c["H"], np.float32(c["dt"])
    worst = {}
    for i in range(1, H + 1):
        q_prev = A["all_traj"][:, i - 1]
        st = frame_step(c["m"], q_prev, c["qf"], c["table"][i - 1], c["vel"], c["k"], c["ignored"], mu, sg, al, c["prm"], max_speed)
        keep = ~st["near"]
        assert (~keep).mean() <= 0.01, f"{what}: step {i}: {int((~keep).sum())} rows within 1e-5 of a branch threshold"
        for name, want in (("closest_dist_all", st["distance"]), ("dot_products", st["dot"]), ("kernel_activations", st["act"]),
                           ("normal", st["ghat"])):
            e = assert_close(A[name][keep, i - 1], want[keep], RTOL, f"{what}: {name} of step {i}")
            worst[name] = max(worst.get(name, 0.0), e)

        def velocity(u_dev, pad, tag):
            counts, err = plain_bar(u_dev[keep], st["u"][keep])
            scale = max(float(np.abs(st["u"][keep]).max()), 1e-30)
            worst[tag] = max(worst.get(tag, 0.0), float(err.max()))
            print(f"{what}: step {i} {tag}: worst row {err.max():.3e} of scale {scale:.3f} (allowed {RTOL + pad / scale:.2e})")
            assert err.max() <= RTOL + pad / scale, f"{what}: {tag} of step {i}: {err.max():.3e}, row {int(err.argmax())}"

        if i < H:    # (q_next - q) / dt loses ulp(q) / dt: the pad of helpers.assert_velocity_plain
            pad = float(np.spacing(np.float32(np.abs(A["all_traj"][:, i - 1:i + 1]).max()))) / float(dt)
            velocity((A["all_traj"][:, i] - q_prev) / dt, pad, "velocity from the states")
        if i == 1:
            velocity(A["qdot"], 0.0, "qdot")
    print(what, "worst:", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- 4. the stage check --------------------------------------------------------------------------------------------------------------
def test_approach_rate_against_the_restatement():
    """Engine.approach_rate on 32 states: the device's selected obstacles (omds_dist_grad's indices), the oracle's gradient rows and
    distances for them (the device's are those bits), the restatement's sums: 1e-6 absolute, only the summation order differs."""
    B = 32
    c = dict(franka_case("emit"), samples=franka_inputs(B, 12)[1])
    e = _franka_engine(c, N=B)
    rng = np.random.RandomState(21)
    q = (c["q_cur"] + 0.3 * rng.standard_normal((B, 7))).astype(np.float32)
    e.set_obstacle_motion(c["vel"])
    rate, qo = e.approach_rate(q)
    idx = e.dist_grad(q, want_idx=True)[3]
    e.close()
    obs, m = c["obs"], c["m"]
    x = np.concatenate((np.repeat(q, K_CLOSEST, axis=0), obs[idx.reshape(-1), :3]), axis=1).astype(np.float32)
    y, grad, min_idx = orc.mlp_vjp_argmin(m, x)
    d = ((y / np.float32(100))[np.arange(y.shape[0]), min_idx] - obs[idx.reshape(-1), 3]).reshape(B, K_CLOSEST)
    ex = np.exp((np.float32(-10.0) * d) - (np.float32(-10.0) * d).max(axis=1, keepdims=True))
    w = (ex / ex.sum(axis=1, keepdims=True)).astype(np.float32)
    want_rate, want_qo, _, gn = frame_quantities(grad, d, w, idx, c["vel"], 7, 1.0)
    print("approach_rate: max |rate - restatement|", float(np.abs(rate - want_rate).max()), "max |qo - restatement|",
          float(np.abs(qo - want_qo).max()), "| rate in", float(rate.min()), float(rate.max()), "| smallest |g|", float(gn.min()))
    assert np.abs(rate).max() > 0.01, "the spheres do move"
    assert np.abs(rate - want_rate).max() <= 1e-6
    assert np.abs(qo - want_qo).max() <= 1e-6


# ---- 5. every route, step by step ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    c = franka_case("dense")
    assert c["N"] * c["obs"].shape[0] > 24576
    e = _franka_engine(c)
    e.set_screening(0)
    on = _run(e, c, frame=True)
    table, mode = e.get_obstacle_horizon()
    off = _run(e, c, frame=False, motion=False)        # the same context, the frame switched off: the moving scene of today
    e.close()
    assert mode == 1 and np.array_equal(table.view(np.uint32), c["table"].view(np.uint32))
    return dict(c=c, on=on, off=off)


def test_dense_route_step_by_step(dense):
    assert dense["on"]["kernel"] == "k_pass1"
    _assert_steps(dense["on"], dense["c"], "Dense")


@pytest.mark.parametrize("route", ["emit", "unfused", "dense_tanh"])
def test_other_franka_routes_step_by_step(route):
    from optimalmodulationds_amd import _lib as L
    c = franka_case(route)
    assert c["N"] * c["obs"].shape[0] <= 24576
    e = _franka_engine(c, flags=L.FLAG_UNFUSED_STEP if route == "unfused" else 0)
    A = _run(e, c)
    assert e.get_obstacle_frame() == (True, 1.0, True)
    e.close()
    assert A["kernel"] == "k_pass1", A["kernel"]
    _assert_steps(A, c, route)


def test_small_scene_route_step_by_step():
    c = planar7_case()
    e = _planar7_engine(c)
    A = _run(e, c)
    e.close()
    assert A["kernel"] == "k_step_small", A["kernel"]
    _assert_steps(A, c, "SmallScene")


def test_planar_point_network_step_by_step():
    """d = n + 2: the frame reads vel[:, 0:2] only (the table keeps every z, the restatement's spheres have none)."""
    c = toy_case()
    e = _toy_engine(c)
    A = _run(e, c)
    table, mode = e.get_obstacle_horizon()
    e.close()
    print("planar points ran on", A["kernel"])
    assert mode == 1 and np.array_equal(table.view(np.uint32), c["table4"].view(np.uint32))
    _assert_steps(A, c, "planar points")
    v2 = c["vel"].copy()
    v2[:, 2] = 5.0
    e = _toy_engine(c)
    B = _run(e, dict(c, vel=v2))
    e.close()
    for name in KEYS:
        assert np.array_equal(A[name], B[name]), f"vel[:, 2] changed {name}"


# ---- 6. it bites ---------------------------------------------------------------------------------------------------------------------
def test_the_frame_changes_the_rollouts(dense):
    on, off = dense["on"], dense["off"]
    share = float((on["all_traj"][:, 2:] != off["all_traj"][:, 2:]).any(axis=(1, 2)).mean())
    print("rollouts whose states beyond step 1 differ between frame on and frame off:", share)
    assert share >= 0.5
    assert np.array_equal(on["closest_dist_all"][:, 0], off["closest_dist_all"][:, 0])
    assert np.array_equal(on["normal"][:, 0], off["normal"][:, 0])
    assert not np.array_equal(on["dot_products"][:, 0], off["dot_products"][:, 0])
    assert not np.array_equal(on["qdot"], off["qdot"])


# ---- 7. the neutral cases, bit for bit -----------------------------------------------------------------------------------------------
def _same(a, b, what):
    for name in KEYS:
        assert np.array_equal(a[name], b[name]), f"{what}: {name}"


@pytest.mark.parametrize("route", ["dense", "emit"])
def test_zero_velocities_are_neutral(route, dense):
    c = dense["c"] if route == "dense" else franka_case(route)
    z = dict(c, vel=np.zeros_like(c["vel"]))
    e = _franka_engine(c)
    on = _run(e, z, frame=True)
    assert e.get_obstacle_frame()[2]
    off = _run(e, z, frame=False)
    e.close()
    _same(on, off, f"{route}: frame on with zero velocities")


def test_frame_without_a_horizon_and_switched_off_again():
    c = franka_case("emit")
    never = _franka_engine(c)          # a context that never hears of the frame
    never.propagate(c["q_cur"])
    static = never.get_rollouts()
    never.set_obstacle_motion(c["vel"])
    never.propagate(c["q_cur"])
    moving = never.get_rollouts()
    never.close()
    e = _franka_engine(c)
    got = _run(e, c, frame=True, motion=False)
    assert e.get_obstacle_frame() == (True, 1.0, False)
    _same(got, static, "frame on, no horizon")
    framed = _run(e, c, frame=True)
    assert not np.array_equal(framed["qdot"], moving["qdot"])
    _same(_run(e, c, frame=False), moving, "frame off after on")
    e.close()


# ---- 8. life cycle -------------------------------------------------------------------------------------------------------------------
def test_life_cycle():
    from optimalmodulationds_amd._lib import OmdsError
    c = franka_case("emit")
    e = _franka_engine(c)
    assert e.get_obstacle_frame() == (False, 1.0, False), "off at creation"
    with pytest.raises(OmdsError, match="omds error 4"):
        e.approach_rate(c["q_cur"][None])
    framed = _run(e, c, frame=True)
    # an explicit table carries no velocities
    e.set_obstacle_horizon(c["table"])
    with pytest.raises(OmdsError, match="omds error 5.*velocities"):
        e.propagate(c["q_cur"])
    with pytest.raises(OmdsError, match="omds error 4"):
        e.approach_rate(c["q_cur"][None])
    e.set_obstacle_frame(False)
    e.propagate(c["q_cur"])
    # the preference survives set_obstacles; it acts again once the motion is back
    e.set_obstacle_frame(True, 0.5)
    e.set_obstacles(c["obs"])
    assert e.get_obstacle_frame() == (True, 0.5, False)
    e.set_obstacle_motion(c["vel"])
    assert e.get_obstacle_frame() == (True, 0.5, True)
    e.set_obstacle_frame(True)
    assert e.get_obstacle_frame() == (True, 1.0, True), "max_speed None selects the default"
    _same(_run(e, c, frame=True), framed, "after set_obstacles + set_obstacle_motion")
    # the clamp
    e.set_obstacle_frame(True, 1e-3)
    rng = np.random.RandomState(22)
    q = (c["q_cur"] + 0.3 * rng.standard_normal((c["N"], 7))).astype(np.float32)
    rate, qo = e.approach_rate(q)
    speed = np.sqrt((qo.astype(np.float64) ** 2).sum(axis=1))
    print("clamped |qo|: max", float(speed.max()), "rows at the clamp:", int((speed > 0.999e-3).sum()), "of", len(speed))
    assert (speed <= 1e-3 * (1 + 1e-6)).all() and (speed > 0.999e-3).any()
    e.close()


# ---- 9. the point of it --------------------------------------------------------------------------------------------------------------
def test_a_chasing_sphere_hits_without_the_frame_and_not_with_it():
    """The scene of test_moving_frame_cpu.chase_case (fixed there on the restatement: frame off 32 of 32 rollouts hit, the least
    affected at -0.023; frame on none, smallest distance 1.19).  The same two signs on the device, with the same margins."""
    c = chase_case()
    assert c["N"] <= 64 and c["H"] <= 16
    e = _toy_engine(c)
    off = _run(e, c, frame=False)["closest_dist_all"].min(axis=1)
    on = _run(e, c, frame=True, max_speed=c["max_speed"])["closest_dist_all"].min(axis=1)
    e.close()
    print("device, frame off: share hit", float((off < 0).mean()), "least / most", float(off.max()), float(off.min()), "| frame on: share hit",
          float((on < 0).mean()), "smallest distance", float(on.min()))
    assert (off < 0).mean() >= 0.9 and off.max() < -0.01
    assert (on < 0).mean() == 0.0 and on.min() > 0.5


# ---- 10. the facade ------------------------------------------------------------------------------------------------------------------
def test_facade_update_obstacles_with_a_moving_frame():
    import torch
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    from optimalmodulationds_amd.engine import Engine
    N, H = 16, 4
    obs = scenes.shelf_scene()
    vel = velocities(obs.shape[0])
    q_cur, samples = franka_inputs(N)
    c = dict(franka_case("emit"), N=N, H=H, q_cur=q_cur, samples=samples, vel=vel)
    e = _franka_engine(c)
    moving = _run(e, c, frame=False)
    framed = _run(e, c, frame=True)
    e.close()
    assert not np.array_equal(moving["qdot"], framed["qdot"])

    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    mppi = MPPI(torch.tensor(q_cur), q_f, dh, torch.tensor(obs), DT, H, N, [LinDS(q_f)], dh[:, 2], nn_model, K_CLOSEST)
    mppi.dst_thr = 0.01
    mppi.Policy.n_kernels = samples[0].shape[1]
    mppi.Policy.set_samples(*samples)
    keys = ("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations")
    for want, kw in ((framed, dict(moving_frame=True)), (moving, dict(moving_frame=False)), (framed, dict(moving_frame=True)), (moving, {})):
        assert mppi.update_obstacles(torch.tensor(obs), velocities=vel, **kw) == 0
        got = mppi.propagate()
        for name, t in zip(keys, got):
            assert np.array_equal(t.numpy(), want[name]), (kw, name)
        assert np.array_equal(mppi.qdot.numpy(), want["qdot"]), kw
