"""Screening under an obstacle horizon (omds_set_screening_horizon; csrc/screening.hip, propagate.hip, k_obstacle_horizon_features'
fp16 slab tables, k_audit_slabs).  The all-fp32 step with a horizon is pinned to the static path step by step by
tests/test_gpu_obstacle_horizon.py; here every comparison is BIT FOR BIT (np.array_equal on all seven outputs) between two contexts
with the same inputs and the same horizon: one on set_screening(0), the other on set_screening(1) + set_screening_horizon(True).
There are no tolerances.

A fallback redoes a propagate in fp32 and would make such a comparison pass vacuously, so _Pair.propagate reads screen_stats()
around every screened propagate: one that counted no fallback must have run k_screen (prof_read_ex) and listed candidates; over a
whole test at most one propagate may fall back, none of them by error, and at least one must really have been screened.

Conventions of tests/test_gpu_obstacle_horizon.py (helpers copied, not imported): Franka weights, the shelf scene (O = 294), dt = 0.5,
k = 5, injected policy samples with K = 3, ignored_links = 0b111, velocities uniform in +-0.2 m/s per axis; KEYS of
tests/test_gpu_screen.py."""
import numpy as np
import pytest

from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

K_CLOSEST, K_POLICY, DT = 5, 3, 0.5
KEYS = ("all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal")


def _inputs(N, seed=11, n=7, q0=None, spread=0.2):
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(seed)
    q0 = np.asarray(scenes.FRANKA_Q0 if q0 is None else q0, np.float32)
    q_cur = (q0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    mu = (q_cur + spread * rng.standard_normal((N, K_POLICY, n))).astype(np.float32)
    samples = (mu, np.ones((N, K_POLICY), np.float32), rng.standard_normal((N, K_POLICY, n)).astype(np.float32))
    return q_cur, samples


def _velocities(O, seed=3):
    return np.random.RandomState(seed).uniform(-0.2, 0.2, (O, 3)).astype(np.float32)


def _franka_engine(samples, N, H, obs, kind="franka", flags=0, max_obs=512, lib=None):
    """A Franka context with one of the weight sets under tests/golden/weights (activation and skip layout from the file)."""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import Engine
    m = orc.Mlp.from_npz(weights_path(kind))
    e = Engine(7, N, H, K_CLOSEST, max_obs=max(max_obs, obs.shape[0]), flags=flags, lib=lib)
    e.set_mlp(m.W, m.b, act=m.act, skip_after=m.skip_after)
    e.set_obstacles(obs)
    e.params.dt = DT
    e.params.dst_thr = 0.01
    e.params.ignored_links = 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_policy_samples(*samples)
    return e


class _Pair:
    """fp32 / screened-over-the-horizon twins of one context recipe, and the bookkeeping that keeps the comparison honest."""

    def __init__(self, make):
        self.e0, self.e1 = make(), make()
        self.e0.set_screening(0)
        self.e1.set_screening(1)
        self.e1.set_screening_horizon(True)
        self.e1.prof_enable(1)
        self.screened = self.fell = 0

    def both(self, fn):
        fn(self.e0)
        fn(self.e1)

    def propagate(self, q, what):
        self.e0.propagate(q)
        a = self.e0.get_rollouts()
        before = self.e1.screen_stats()
        self.e1.prof_reset()
        self.e1.propagate(q)
        b = self.e1.get_rollouts()
        st = self.e1.screen_stats()
        kernel = self.e1.prof_read_ex()[3]
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), (what, key, float(np.nanmax(np.abs(a[key] - b[key]))))
        if st["fallbacks"] == before["fallbacks"]:   # really screened
            assert kernel == "k_screen" and st["candidates_per_rollout_step"] > 0, (what, kernel, st)
            self.screened += 1
        else:
            self.fell += 1
        print(what, "kernel", kernel, {k: st[k] for k in ("eps", "max_err_seen", "audit_max_err", "candidates_per_rollout_step", "fallbacks",
                                                          "fallbacks_by_slack", "fallbacks_by_overflow", "calibrations")})
        return st

    def finish(self):
        st = self.e1.screen_stats()
        assert self.fell <= 1 and st["fallbacks_by_error"] == 0 and self.screened >= 1, (self.fell, self.screened, st)
        self.e0.close()
        self.e1.close()
        return st


def _shelf():
    from optimalmodulationds_amd import scenes
    return scenes.shelf_scene()


# ---- 1. motion horizon, ReLU ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H", [(96, 4), (320, 3)])
def test_motion_horizon_is_screened_bit_for_bit(N, H):
    """96 x 294 = 28 224 pairs: fewer rollouts than CUs, and 294 = 9 * 32 + 6 leaves a partial wave per rollout; at N = 320 some
    persistent workgroups of k_screen own two rollouts.  Four iterations of a scene that keeps translating: the start state drifts,
    set_obstacles + set_obstacle_motion again each iteration with the scene advanced by v dt."""
    from optimalmodulationds_amd import scenes
    obs, vel = _shelf(), _velocities(294)
    q_cur, samples = _inputs(N)
    p = _Pair(lambda: _franka_engine(samples, N, H, obs))
    rng = np.random.RandomState(21)
    q, scene = q_cur.copy(), obs.copy()
    for it in range(4):
        p.both(lambda e: (e.set_obstacles(scene), e.set_obstacle_motion(vel)))
        assert p.e1.screen_stats()["active"] and p.e1.get_screening_horizon() == (True, True)
        assert not p.e0.screen_stats()["active"] and p.e0.get_screening_horizon() == (False, False)
        p.propagate(q, f"motion N={N} it={it}")
        q = (q + 0.04 * (scenes.FRANKA_QF - scenes.FRANKA_Q0) + 0.02 * rng.standard_normal(7)).astype(np.float32)
        scene = scene.copy()
        scene[:, :3] += np.float32(DT) * vel
    st = p.finish()
    assert st["active"] and st["calibrations"] >= 1
    assert st["max_err_seen"] <= 0.5 * st["eps"] and st["audit_max_err"] <= 0.5 * st["eps"], st


# ---- 2. explicit table ------------------------------------------------------------------------------------------------------------
def test_explicit_table_with_radii_per_slab_is_screened_bit_for_bit():
    """Mode 2, the radii inflated per slab (r (1 + 0.1 h)): the per-slab radius reaches k_screen, k_exact and the tail."""
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    N, H = 96, 4
    obs = _shelf()
    table = predict_obstacle_horizon(obs, _velocities(294, seed=5), H, DT)
    table[:, :, 3] *= (1 + np.float32(0.1) * np.arange(H, dtype=np.float32))[:, None]
    q_cur, samples = _inputs(N, seed=13)
    p = _Pair(lambda: _franka_engine(samples, N, H, obs))
    p.both(lambda e: e.set_obstacle_horizon(table))
    assert p.e1.get_obstacle_horizon()[1] == 2 and p.e1.get_screening_horizon() == (True, True)
    p.propagate(q_cur, "explicit table")
    p.propagate((q_cur + np.float32(0.05)).astype(np.float32), "explicit table, second start state")
    p.finish()


# ---- 3. moving frame --------------------------------------------------------------------------------------------------------------
def test_moving_frame_is_screened_bit_for_bit():
    from optimalmodulationds_amd._lib import OmdsError
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    N, H = 96, 4
    obs, vel = _shelf(), _velocities(294, seed=6)
    q_cur, samples = _inputs(N, seed=15)
    p = _Pair(lambda: _franka_engine(samples, N, H, obs))
    p.both(lambda e: (e.set_obstacle_motion(vel), e.set_obstacle_frame(True)))
    assert p.e1.get_obstacle_frame()[2] and p.e0.get_obstacle_frame()[2]
    plain = _franka_engine(samples, N, H, obs)       # the same motion in the world frame: the frame does change the rollouts
    plain.set_obstacle_motion(vel)
    plain.propagate(q_cur)
    world = plain.get_rollouts()
    plain.close()
    p.propagate(q_cur, "moving frame")
    assert not np.array_equal(world["all_traj"], p.e1.get_rollouts()["all_traj"])
    p.propagate((q_cur - np.float32(0.05)).astype(np.float32), "moving frame, second start state")
    # an explicit table carries no velocities: the propagate still says so, screened or not
    p.e1.set_obstacle_horizon(predict_obstacle_horizon(obs, vel, H, DT))
    with pytest.raises(OmdsError, match="omds error 5"):
        p.e1.propagate(q_cur)
    p.finish()


# ---- 4. other networks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["franka_tanh", "franka_skip"])
def test_tanh_and_skip_networks_are_screened_bit_for_bit(kind):
    """tanh: k_exact's derivative hand-over; skip: the concatenation operand of k_screen per slab (MlpDev::scrP)."""
    N, H = 64, 4
    obs, vel = _shelf(), _velocities(294, seed=7)
    q_cur, samples = _inputs(N, seed=16)
    p = _Pair(lambda: _franka_engine(samples, N, H, obs, kind=kind))
    p.both(lambda e: e.set_obstacle_motion(vel))
    p.propagate(q_cur, kind)
    p.propagate((q_cur + np.float32(0.04)).astype(np.float32), kind + ", second start state")
    st = p.finish()
    assert st["max_err_seen"] <= 0.5 * st["eps"] and st["audit_max_err"] <= 0.5 * st["eps"], st


@pytest.mark.parametrize("kind,n,k", [("planar7", 7, 1), ("planar7", 7, 3), ("planar2", 2, 2)])
def test_planar_networks_are_screened_bit_for_bit(kind, n, k):
    """The planar robots' networks on the cloud of 700 discs of tests/test_gpu_screen.py's planar test, the discs drifting at up to
    1 unit/s per axis (the scene is 15 units wide); the 2- and 7-DoF tails, other k."""
    from optimalmodulationds_amd.engine import Engine
    m = orc.Mlp.from_npz(weights_path(kind))
    rng = np.random.RandomState(12)
    reach = 6.5 if n == 2 else 7.5
    obs = np.c_[rng.uniform(-reach, reach, (700, 2)), np.zeros(700), rng.uniform(0.2, 0.6, 700)].astype(np.float32)
    vel = (5 * _velocities(700, seed=9)).astype(np.float32)
    q0 = np.zeros(n, np.float32); q0[0] = np.pi / 2
    qf = np.zeros(n, np.float32); qf[0] = -np.pi / 2
    N, H = 128, 4
    q_cur, samples = _inputs(N, seed=17, n=n, q0=q0, spread=0.3)

    def make():
        e = Engine(n, N, H, k, max_obs=1024)
        e.set_mlp(m.W, m.b)
        e.set_obstacles(obs)
        e.params.dt, e.params.dst_thr, e.params.ignored_links = 0.3, 0.25, 0
        e.push_params()
        e.set_ds(qf)
        e.set_policy_samples(*samples)
        return e

    p = _Pair(make)
    p.both(lambda e: e.set_obstacle_motion(vel))
    q = q_cur.copy()
    for it in range(2):
        p.propagate(q, f"{kind} k={k} it={it}")
        q = (q + 0.1 * (qf - q0)).astype(np.float32)
    p.finish()


# ---- 5. long rows -----------------------------------------------------------------------------------------------------------------
def test_long_rows_are_screened_bit_for_bit_on_the_matrix():
    """O = 6000 (the scene of test_rows_longer_than_a_workgroups_result_buffer_take_the_matrix_route): omds_screen_can_select is
    false, k_screen writes the matrix of the step's slab and k_select does the selection."""
    rng = np.random.RandomState(8)
    pts = rng.uniform([-0.3, -0.8, 0.0], [1.0, 0.8, 1.2], (6000, 3))
    obs = np.c_[pts, rng.uniform(0.01, 0.04, 6000)].astype(np.float32)
    N, H = 96, 3
    q_cur, samples = _inputs(N, seed=18)
    p = _Pair(lambda: _franka_engine(samples, N, H, obs, max_obs=6000))
    p.both(lambda e: e.set_obstacle_motion(_velocities(6000, seed=10)))
    p.propagate(q_cur, "O = 6000")
    st = p.finish()
    assert st["audit_rows_per_rollout_step"] > 10, st


# ---- 6. the audit and the sweep read the step's slab ------------------------------------------------------------------------------
def test_audit_and_sweep_read_the_slab_of_their_step():
    """At +-0.2 m/s the last of six slabs lies up to 0.5 m from slab 0, against an eps of about 0.016: a k_audit or a sweep that read
    slab 0 for the later steps would measure decimetres and fall back by error."""
    N, H = 96, 6
    obs, vel = _shelf(), _velocities(294, seed=4)
    q_cur, samples = _inputs(N, seed=19)
    p = _Pair(lambda: _franka_engine(samples, N, H, obs))
    p.e1.set_screening_audit(4)
    p.e1.set_screening_sweep(1, all_steps=True)
    p.both(lambda e: e.set_obstacle_motion(vel))
    table = p.e1.get_obstacle_horizon()[0]
    assert np.abs(table[H - 1, :, :3] - table[0, :, :3]).max() > 0.4
    p.propagate(q_cur, "audit 1 in 4, all-steps sweep")
    p.propagate((q_cur + np.float32(0.03)).astype(np.float32), "audit 1 in 4, all-steps sweep, second start state")
    hist = p.e1.sweep_hist()
    st = p.finish()
    assert st["audit_rows_per_rollout_step"] > 0 and st["sweeps"] == 2 * H, st
    assert hist["above_half_eps"] == 0 and hist["non_candidates"] > 0, hist
    assert st["audit_max_err"] <= 0.5 * st["eps"] and st["sweep_max_err"] <= 0.5 * st["eps"] and st["fallbacks"] == 0, st


# ---- 7. a damaged later slab is caught --------------------------------------------------------------------------------------------
def test_a_damaged_later_slab_is_caught_by_the_audit():
    """The fp16 table of the LAST slab sees one sphere 1.5 m away from where it is (omds_test_screen_corrupt_slab): with every
    unevaluated pair audited the propagate falls back by error and returns the fp32 numbers.  The sphere is the one nearest to the
    start state, so the shift moves it away from the robot: its screening values rise, it is no candidate any more, and only the
    audit rows can notice.  Without audit and sweep nobody does: no fallback is counted."""
    from optimalmodulationds_amd import _lib
    lib = _lib.load_test_hooks()
    N, H = 64, 4
    obs, vel = _shelf(), _velocities(294, seed=3)
    q_cur, samples = _inputs(N, seed=20)
    make = lambda: _franka_engine(samples, N, H, obs, lib=lib)
    probe = make()
    victim = int(np.argmin(probe.dist_grad(q_cur[None], want_mindist=True)[2][0]))
    probe.close()

    p = _Pair(make)
    p.e1.set_screening_audit(1)
    p.both(lambda e: e.set_obstacle_motion(vel))
    st = p.propagate(q_cur, "clean")
    assert st["fallbacks"] == 0
    p.e1.test_screen_corrupt_slab(H - 1, victim, 1.5)
    st = p.propagate(q_cur, "last slab damaged")       # still the fp32 context's outputs, bit for bit
    assert st["fallbacks"] == 1 and st["fallbacks_by_error"] == 1, st
    p.e0.close()
    p.e1.close()

    blind = make()
    blind.set_screening(1)
    blind.set_screening_horizon(True)
    blind.set_screening_audit(0)
    blind.set_screening_sweep(0)
    with pytest.raises(_lib.OmdsError, match="omds error 4"):
        blind.test_screen_corrupt_slab(H - 1, victim, 1.5)      # no fp16 slab tables yet
    blind.set_obstacle_motion(vel)
    blind.propagate(q_cur)
    blind.test_screen_corrupt_slab(H - 1, victim, 1.5)
    blind.propagate(q_cur)
    st = blind.screen_stats()
    blind.close()
    assert st["active"] and st["fallbacks"] == 0, st


# ---- 8. the calibration rule ------------------------------------------------------------------------------------------------------
def test_calibration_follows_the_last_slab():
    N, H = 96, 4
    obs, vel = _shelf(), _velocities(294, seed=3)
    q_cur, samples = _inputs(N, seed=22)
    assert np.abs(2 * (H - 1) * DT * vel).max() > 0.1      # reversing the velocities moves the last slab by more than the threshold
    p = _Pair(lambda: _franka_engine(samples, N, H, obs))
    assert p.propagate(q_cur, "static")["calibrations"] == 1
    p.both(lambda e: e.set_obstacle_motion(vel))
    assert p.propagate(q_cur, "motion set: a bound measured without a horizon does not stand")["calibrations"] == 2
    p.both(lambda e: e.set_obstacle_motion(vel))
    assert p.propagate(q_cur, "the same motion")["calibrations"] == 2
    p.both(lambda e: e.set_obstacle_motion(-vel))
    assert p.propagate(q_cur, "velocities reversed: another last slab")["calibrations"] == 3
    p.both(lambda e: e.set_obstacle_motion(None))
    assert p.propagate(q_cur, "horizon cleared: measured under a horizon, covers the static scene")["calibrations"] == 3
    p.finish()


def test_a_fixed_bound_is_never_recalibrated():
    N, H = 96, 4
    obs, vel = _shelf(), _velocities(294, seed=3)
    q_cur, samples = _inputs(N, seed=22)
    p = _Pair(lambda: _franka_engine(samples, N, H, obs))
    p.e1.set_screening(1, eps=0.05)
    for what, v in (("static", None), ("motion", vel), ("reversed", -vel), ("cleared", None)):
        p.both(lambda e: e.set_obstacle_motion(v))
        assert p.propagate(q_cur, "eps = 0.05, " + what)["calibrations"] == 0
    p.finish()


# ---- 9. off means today -----------------------------------------------------------------------------------------------------------
def test_off_is_the_all_fp32_step_and_slab_0_is_the_static_table():
    N, H = 96, 4
    obs, vel = _shelf(), _velocities(294, seed=3)
    q_cur, samples = _inputs(N, seed=23)
    ref = _franka_engine(samples, N, H, obs)
    ref.set_screening(0)
    ref.set_obstacle_motion(vel)
    ref.propagate(q_cur)
    want = ref.get_rollouts()
    ref.close()

    e = _franka_engine(samples, N, H, obs)
    e.set_screening(1)
    q = (q_cur + 0.1 * np.random.RandomState(2).standard_normal((32, 7))).astype(np.float32)
    static_values = e.screen_mindist(q)
    assert e.get_screening_horizon() == (False, False) and e.screen_stats()["active"]
    e.set_obstacle_motion(vel)
    assert e.get_screening_horizon() == (False, False) and not e.screen_stats()["active"]
    e.set_screening_horizon(True)
    assert e.get_screening_horizon() == (True, True) and e.screen_stats()["active"]
    e.get_obstacle_horizon()                      # builds the fp16 slab tables
    # the batch entry points keep reading the static tables, which slab 0 repeats
    assert np.array_equal(e.screen_mindist(q).view(np.uint32), static_values.view(np.uint32))
    e.set_screening_horizon(False)
    assert e.get_screening_horizon() == (False, False) and not e.screen_stats()["active"]
    e.propagate(q_cur)
    got = e.get_rollouts()
    st = e.screen_stats()
    for key in KEYS:
        assert np.array_equal(want[key], got[key]), key
    assert not st["active"] and st["calibrations"] == 0 and st["candidates_per_rollout_step"] == 0, st
    e.close()


def test_slab_0_of_a_screened_horizon_is_the_static_screened_step():
    """Slab 0 of the fp16 slab tables holds the bits of the static fp16 table: with H = 1 a screened propagate under a horizon lists
    the candidates a static screened propagate lists (the same count per rollout and step, the same largest candidate error), and
    with zero velocities every slab does."""
    N = 96
    obs = _shelf()
    q_cur, samples = _inputs(N, seed=24)
    stats = []
    for H, vel in ((1, None), (1, _velocities(294, seed=3)), (3, None), (3, np.zeros((294, 3), np.float32))):
        e = _franka_engine(samples, N, H, obs)
        e.set_screening(1, eps=0.02)                # the same bound on both sides: the candidate lists depend on it
        e.set_screening_horizon(True)
        if vel is not None:
            e.set_obstacle_motion(vel)
        e.propagate(q_cur)
        st = e.screen_stats()
        assert st["active"] and st["fallbacks"] == 0 and st["candidates_per_rollout_step"] > 0, st
        stats.append((st["candidates_per_rollout_step"], st["max_err_seen"], st["audit_max_err"], e.get_rollouts()))
        e.close()
    for a, b in ((stats[0], stats[1]), (stats[2], stats[3])):
        assert a[:3] == b[:3], (a[:3], b[:3])
        for key in KEYS:
            assert np.array_equal(a[3][key], b[3][key]), key


# ---- the facade -------------------------------------------------------------------------------------------------------------------
def test_facade_set_screening_over_the_horizon():
    """MPPI.set_screening(mode, eps, over_horizon) is a pass-through to the engine; with velocities the propagate is screened and
    returns what the all-fp32 facade returns."""
    import torch
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    N, H = 96, 4
    obs, vel = _shelf(), _velocities(294)
    q_cur, samples = _inputs(N)
    outs = []
    for over in (False, True):
        nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
        nn_model.load_weights(weights_path("franka"), {})
        dh = torch.tensor(scenes.franka_dh_params())
        q_f = torch.tensor(scenes.FRANKA_QF)
        mppi = MPPI(torch.tensor(q_cur), q_f, dh, torch.tensor(obs), DT, H, N, [LinDS(q_f)], dh[:, 2], nn_model, K_CLOSEST)
        mppi.dst_thr = 0.01
        mppi.Policy.n_kernels = K_POLICY
        mppi.Policy.set_samples(*samples)
        mppi.set_screening(1, over_horizon=over)
        assert mppi.update_obstacles(torch.tensor(obs), velocities=vel) == 0
        assert mppi._engine.get_screening_horizon() == (over, over)
        outs.append([np.asarray(t) for t in mppi.propagate()])
        st = mppi._engine.screen_stats()
        assert st["active"] == over and st["fallbacks"] == 0 and (st["candidates_per_rollout_step"] > 0) == over, st
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
