"""The obstacle horizon (csrc/obstacle_horizon.hip, include/omds.h): step i of a propagate evaluates the network at all_traj[:, i - 1]
against slab i - 1 of a table [H, O, 4] -- constant velocities (set_obstacle_motion) or the caller's own predictions
(set_obstacle_horizon) -- instead of the scene frozen at now.  No MFMA kernel changes its arithmetic, so every step is checked BIT FOR
BIT against the existing static path: a fresh static context holding slab i - 1 as its scene, started per rollout at the states step
i started from, must give step i's tensors.  (A row's bits depend neither on the tile shape nor on the batch around it:
tests/test_gpu_shared_first_step.py, tests/test_gpu_sparse.py.)  Conventions of tests/test_gpu_shared_first_step.py: Franka weights,
the shelf scene, dt = 0.5, injected policy samples with K = 3, ignored_links = 0b111; velocities uniform in +-0.2 m/s per axis."""
import numpy as np
import pytest

from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

K_CLOSEST, K_POLICY, DT = 5, 3, 0.5
STEP_KEYS = ("closest_dist_all", "dot_products", "kernel_val_all", "kernel_activations", "normal")


def _inputs(N, seed=11):
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(seed)
    q_cur = (np.asarray(scenes.FRANKA_Q0, np.float32) + 0.1 * rng.standard_normal(7)).astype(np.float32)
    mu = (q_cur + 0.2 * rng.standard_normal((N, K_POLICY, 7))).astype(np.float32)
    samples = (mu, np.ones((N, K_POLICY), np.float32), rng.standard_normal((N, K_POLICY, 7)).astype(np.float32))
    return q_cur, samples


def _velocities(O, seed=3):
    return np.random.RandomState(seed).uniform(-0.2, 0.2, (O, 3)).astype(np.float32)


def _franka_engine(samples, N, H, obs, kind="franka", flags=0, max_obs=512):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import Engine
    m = orc.Mlp.from_npz(weights_path(kind))
    e = Engine(7, N, H, K_CLOSEST, max_obs=max_obs, flags=flags)
    e.set_mlp(m.W, m.b, act="tanh" if kind.endswith("tanh") else "relu")
    e.set_obstacles(obs)
    e.params.dt = DT
    e.params.dst_thr = 0.01
    e.params.ignored_links = 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_policy_samples(*samples)
    return e


def _assert_reduces_to_static(A, table, make_static, what):
    """Step i of A against a fresh static context (horizon 2) whose scene is slab i - 1, started per rollout where step i started."""
    H = table.shape[0]
    for i in range(1, H + 1):
        e = make_static(table[i - 1])
        e.propagate(np.ascontiguousarray(A["all_traj"][:, i - 1]))
        B = e.get_rollouts()
        e.close()
        for name in STEP_KEYS:
            assert np.array_equal(B[name][:, 0], A[name][:, i - 1]), f"{what}: {name} of step {i} is not the static path's on slab {i - 1}"
        if i < H:
            assert np.array_equal(B["all_traj"][:, 1], A["all_traj"][:, i]), f"{what}: the state after step {i}"
        if i == 1:
            assert np.array_equal(B["qdot"], A["qdot"]), f"{what}: qdot"


def _same(a, b, what):
    for name in a:
        assert np.array_equal(a[name], b[name]), f"{what}: {name}"


N_DENSE, H_DENSE = 96, 4


@pytest.fixture(scope="module")
def dense():
    """Run A of the Dense route (N x O > 24 576 pairs): one propagate from one q_cur with moving obstacles; computed once."""
    from optimalmodulationds_amd import scenes
    obs = scenes.shelf_scene()
    assert N_DENSE * obs.shape[0] > 24576
    q_cur, samples = _inputs(N_DENSE)
    vel = _velocities(obs.shape[0])
    e = _franka_engine(samples, N_DENSE, H_DENSE, obs)
    e.set_screening(0)
    e.set_obstacle_motion(vel)
    table, mode = e.get_obstacle_horizon()
    e.propagate(q_cur)
    A = e.get_rollouts()
    e.close()
    return dict(obs=obs, vel=vel, q_cur=q_cur, samples=samples, table=table, mode=mode, A=A)


def test_motion_table_is_the_host_prediction(dense):
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    want = predict_obstacle_horizon(dense["obs"], dense["vel"], H_DENSE, DT)
    assert dense["mode"] == 1
    assert np.array_equal(dense["table"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(dense["table"][0].view(np.uint32), dense["obs"].view(np.uint32))
    step = np.abs(dense["table"][1, :, :3] - dense["obs"][:, :3])
    assert step.max() <= 0.1 + 1e-6 and step.max() > 0.05, "every sphere moves at most 0.1 m per step, and they do move"


def test_dense_route_reduces_to_the_static_path(dense):
    _assert_reduces_to_static(dense["A"], dense["table"], lambda slab: _franka_engine(dense["samples"], N_DENSE, 2, slab), "Dense")


def test_a_static_propagate_differs_behind_the_first_step(dense):
    """The reduction above bites: the same inputs on the frozen scene give step 1 and nothing else."""
    e = _franka_engine(dense["samples"], N_DENSE, H_DENSE, dense["obs"])
    e.propagate(dense["q_cur"])
    S = e.get_rollouts()
    e.close()
    A = dense["A"]
    for name in STEP_KEYS:
        assert np.array_equal(S[name][:, 0], A[name][:, 0]), name
    assert np.array_equal(S["qdot"], A["qdot"]) and np.array_equal(S["all_traj"][:, 1], A["all_traj"][:, 1])
    share = float((S["closest_dist_all"][:, 1:] != A["closest_dist_all"][:, 1:]).any(axis=1).mean())
    print("rollouts whose distances behind step 1 differ from the frozen scene's:", share)
    assert share >= 0.5


@pytest.mark.parametrize("route", ["emit", "unfused", "dense_tanh"])
def test_other_franka_routes_reduce_to_the_static_path(route):
    """Emit: 16 x 294 = 4 704 pairs; Unfused: OMDS_FLAG_UNFUSED_STEP at N = 32; a tanh network (never Emit: Dense at N = 16)."""
    from optimalmodulationds_amd import _lib as L, scenes
    N, H = (32, 3) if route == "unfused" else (16, 3)
    kind = "franka_tanh" if route == "dense_tanh" else "franka"
    flags = L.FLAG_UNFUSED_STEP if route == "unfused" else 0
    obs = scenes.shelf_scene()
    assert N * obs.shape[0] <= 24576
    q_cur, samples = _inputs(N, seed=12)
    e = _franka_engine(samples, N, H, obs, kind=kind, flags=flags)
    e.set_obstacle_motion(_velocities(obs.shape[0], seed=4))
    table, mode = e.get_obstacle_horizon()
    e.prof_enable(1)
    e.propagate(q_cur)
    A = e.get_rollouts()
    kernel = e.prof_read_ex()[3]
    e.close()
    assert mode == 1 and kernel == "k_pass1", kernel
    assert (A["closest_dist_all"][:, 1:] != A["closest_dist_all"][:, :1]).any()
    _assert_reduces_to_static(A, table, lambda slab: _franka_engine(samples, N, 2, slab, kind=kind, flags=flags), route)


def test_small_scene_route_reduces_to_the_static_path():
    """k_step_small on the planar-7 set-up of tests/test_gpu_small_step.py (N = 64, H = 3, O = 8, k = 2).  planar7.npz takes x, y AND
    z (dims[0] = 30 = 3 (7 + 3)): it is no planar-point network, so vz moves the spheres like vx and vy and the table is the full
    prediction.  The planar-point rule (dims[0] = 3 (n + 2): vz ignored) is the toy network's, in the test below."""
    from test_gpu_small_step import _engine, _policy
    N, H, O, k, K = 64, 3, 8, 2, 6

    def make(Hh, scene=None):
        e, m, obs, q0, qf = _engine(N, Hh, O, k)
        if scene is not None:
            e.set_obstacles(scene)
        rng = np.random.RandomState(3)
        mu_c, sg_c, al_c = _policy(rng, q0, qf, K)
        e.sample_policy(mu_c, sg_c, al_c, 0.0, 0.0, 0.75, K, seed=21)
        return e, obs, q0

    e, obs, q0 = make(H)
    vel = _velocities(O, seed=6)
    e.set_obstacle_motion(vel)
    table, mode = e.get_obstacle_horizon()
    e.prof_enable(1)
    e.propagate(q0)
    A = e.get_rollouts()
    kernel = e.prof_read_ex()[3]
    e.close()
    assert mode == 1 and kernel == "k_step_small", kernel
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    want = predict_obstacle_horizon(obs, vel, H, 0.3)     # _engine's dt
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    assert (table[1, :, :3] != obs[:, :3]).any(axis=0).all(), "x, y and z all move"
    _assert_reduces_to_static(A, table, lambda slab: make(2, slab)[0], "SmallScene")


def test_planar_point_network_ignores_vz():
    """The toy network reads planar obstacle points (dims[0] = 12 = 3 (2 + 2)): vz is ignored as z is -- the table keeps every z and
    moves x and y by the host's formula -- and every step reduces to the static path on its slab (set-up of tests/test_toy_variant.py:
    the 20-sphere arc, 100 rollouts, no policy kernels)."""
    from helpers import load
    from test_toy_variant import _engine, _obs4
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    fx = load("toy2_arc_K0")
    N, H = int(fx["N"]), 3
    obs = _obs4(fx)
    obs[:, 2] = np.linspace(-0.5, 0.5, obs.shape[0], dtype=np.float32)     # a z for the table to keep
    samples = (fx["it0_mu_tmp"], fx["it0_sigma_tmp"], fx["it0_alpha_tmp"])

    def make(Hh, scene):
        e = _engine(fx, N, Hh)
        e.set_obstacles(scene)
        e.set_policy_samples(*samples)
        return e

    vel = _velocities(obs.shape[0], seed=7)
    e = make(H, obs)
    e.set_obstacle_motion(vel)
    table, mode = e.get_obstacle_horizon()
    e.propagate(fx["it0_q_cur"])
    A = e.get_rollouts()
    e.close()
    want = predict_obstacle_horizon(obs, vel * np.array([1, 1, 0], np.float32), H, float(fx["dt"]))
    assert mode == 1 and np.array_equal(table.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(table[:, :, 2].view(np.uint32), np.tile(obs[:, 2], (H, 1)).view(np.uint32)) and (vel[:, 2] != 0).all()
    assert (table[1, :, :2] != obs[:, :2]).any(axis=0).all()
    _assert_reduces_to_static(A, table, lambda slab: make(2, slab), "planar points")


def test_explicit_table_equals_the_motion_it_was_read_from(dense):
    e = _franka_engine(dense["samples"], N_DENSE, H_DENSE, dense["obs"])
    e.set_obstacle_horizon(dense["table"])
    table, mode = e.get_obstacle_horizon()
    assert mode == 2 and np.array_equal(table.view(np.uint32), dense["table"].view(np.uint32))
    e.propagate(dense["q_cur"])
    _same(e.get_rollouts(), dense["A"], "explicit table")
    # slab 0 is the current scene bit for bit, or the table is refused -- and the horizon in force stays
    from optimalmodulationds_amd._lib import OmdsError
    bad = dense["table"].copy()
    bad.view(np.uint32)[0, 7, 1] ^= 1
    with pytest.raises(OmdsError, match="omds error 1.*slab 0"):
        e.set_obstacle_horizon(bad)
    with pytest.raises(OmdsError, match="omds error 1.*n_obs"):
        e.set_obstacle_horizon(dense["table"][:, :-1])
    assert e.get_obstacle_horizon()[1] == 2
    e.close()


def test_explicit_table_with_growing_radii_reduces_to_the_static_path():
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    N, H = 16, 3
    obs = scenes.shelf_scene()
    q_cur, samples = _inputs(N, seed=13)
    table = predict_obstacle_horizon(obs, _velocities(obs.shape[0], seed=5), H, DT)
    table[:, :, 3] += (np.float32(0.01) * np.arange(H, dtype=np.float32))[:, None]
    e = _franka_engine(samples, N, H, obs)
    e.set_obstacle_horizon(table)
    e.propagate(q_cur)
    A = e.get_rollouts()
    back, mode = e.get_obstacle_horizon()
    e.close()
    assert mode == 2 and np.array_equal(back.view(np.uint32), table.view(np.uint32))
    _assert_reduces_to_static(A, table, lambda slab: _franka_engine(samples, N, 2, slab), "explicit radii")


def test_life_cycle():
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd._lib import OmdsError
    from optimalmodulationds_amd.engine import Engine, predict_obstacle_horizon
    N, H = 16, 3
    obs = scenes.shelf_scene()
    O = obs.shape[0]
    vel = _velocities(O, seed=8)
    q_cur, samples = _inputs(N, seed=14)

    def rollouts(e):
        e.propagate(q_cur)
        return e.get_rollouts()

    e = _franka_engine(samples, N, H, obs)
    static = rollouts(e)
    e.set_obstacle_motion(vel)
    moving = rollouts(e)
    assert not np.array_equal(moving["closest_dist_all"], static["closest_dist_all"])
    # params.dt between two propagates: the table follows
    e.params.dt = 0.25
    e.push_params()
    slow = rollouts(e)
    table, mode = e.get_obstacle_horizon()
    assert mode == 1 and np.array_equal(table.view(np.uint32), predict_obstacle_horizon(obs, vel, H, 0.25).view(np.uint32))
    assert not np.array_equal(slow["closest_dist_all"], moving["closest_dist_all"])
    e.params.dt = DT
    e.push_params()
    _same(rollouts(e), moving, "dt restored")
    # set_obstacles clears the horizon
    e.set_obstacles(obs)
    table, mode = e.get_obstacle_horizon()
    assert mode == 0 and np.array_equal(table, np.tile(obs, (H, 1, 1)))
    _same(rollouts(e), static, "after set_obstacles")
    e.set_obstacle_motion(vel)
    e.set_obstacle_motion(None)
    assert e.get_obstacle_horizon()[1] == 0
    _same(rollouts(e), static, "after set_obstacle_motion(None)")
    e.close()

    # more spheres than max_obs, the tables already allocated for the smaller capacity: they grow with the other obstacle buffers
    g = _franka_engine(samples, N, H, obs[:40], max_obs=64)
    g.set_obstacle_motion(vel[:40])
    assert np.isfinite(rollouts(g)["all_traj"]).all()
    g.set_obstacles(obs)
    g.set_obstacle_motion(vel)
    _same(rollouts(g), moving, "grown past max_obs")
    g.close()

    # set_mlp after the motion: the feature slabs are derived again (the planar-7 network first: other weights behind the same slots)
    s = _franka_engine(samples, N, H, obs, kind="planar7")
    s.set_obstacle_motion(vel)
    rollouts(s)
    m = orc.Mlp.from_npz(weights_path("franka"))
    s.set_mlp(m.W, m.b)
    _same(rollouts(s), moving, "set_mlp after set_obstacle_motion")
    s.close()

    # a setter before any scene
    n = Engine(7, N, H, K_CLOSEST, max_obs=64)
    with pytest.raises(OmdsError, match="omds error 4"):
        n.set_obstacle_motion(vel)
    with pytest.raises(OmdsError, match="omds error 4"):
        n.set_obstacle_horizon(np.zeros((H, O, 4), np.float32))
    n.close()

    # a network wider than 256: the propagate says it cannot, and can again once the horizon is cleared
    rng = np.random.RandomState(1)
    dims = [30, 257, 257, 9]
    Ws = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32) for i in range(3)]
    bs = [(0.1 * rng.standard_normal(dims[i + 1])).astype(np.float32) for i in range(3)]
    w = Engine(7, N, H, K_CLOSEST, max_obs=512)
    w.set_mlp(Ws, bs)
    w.set_obstacles(obs)
    w.set_ds(scenes.FRANKA_QF)
    w.set_policy_samples(*samples)
    w.set_obstacle_motion(vel)
    with pytest.raises(OmdsError, match="omds error 5"):
        w.propagate(q_cur)
    w.set_obstacle_motion(None)
    w.propagate(q_cur)
    w.close()


def test_screening_stands_aside_while_a_horizon_is_set(dense):
    e = _franka_engine(dense["samples"], N_DENSE, H_DENSE, dense["obs"])
    e.set_screening(1)
    assert e.screen_stats()["active"]
    e.set_obstacle_motion(dense["vel"])
    assert not e.screen_stats()["active"]
    e.propagate(dense["q_cur"])
    _same(e.get_rollouts(), dense["A"], "screening requested, horizon set")
    st = e.screen_stats()
    assert not st["active"] and st["calibrations"] == 0
    e.set_obstacle_motion(None)
    e.propagate(dense["q_cur"])
    st = e.screen_stats()
    assert st["active"] and st["calibrations"] == 1, "the screened step runs again (its first propagate calibrates)"
    e.close()


def test_facade_update_obstacles_with_velocities():
    """MPPI.update_obstacles(obs, velocities=v) + propagate() = the Engine with set_obstacle_motion(v); without velocities the
    reference's static scene, and an unchanged parameter set (_push skips it) does not lose the motion."""
    import torch
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    N, H = 16, 4
    obs = scenes.shelf_scene()
    vel = _velocities(obs.shape[0])
    q_cur, samples = _inputs(N)
    e = _franka_engine(samples, N, H, obs)
    static = (e.propagate(q_cur), e.get_rollouts())[1]
    e.set_obstacle_motion(vel)
    moving = (e.propagate(q_cur), e.get_rollouts())[1]
    e.close()
    assert not np.array_equal(static["closest_dist_all"], moving["closest_dist_all"])

    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    mppi = MPPI(torch.tensor(q_cur), q_f, dh, torch.tensor(obs), DT, H, N, [LinDS(q_f)], dh[:, 2], nn_model, K_CLOSEST)
    mppi.dst_thr = 0.01
    mppi.Policy.n_kernels = K_POLICY
    mppi.Policy.set_samples(*samples)
    keys = ("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations")
    for want, v in ((moving, vel), (moving, vel), (static, None)):
        assert mppi.update_obstacles(torch.tensor(obs), velocities=v) == 0
        got = mppi.propagate()
        for name, t in zip(keys, got):
            assert np.array_equal(t.numpy(), want[name]), name
        assert np.array_equal(mppi.qdot.numpy(), want["qdot"])
    mppi.update_obstacles(obs, vel)          # positional, as the reference passes obs
    assert np.array_equal(mppi.propagate()[1].numpy(), moving["closest_dist_all"])
