"""The scene from a depth point cloud on the device (include/omds.h: omds_set_obstacles_from_cloud, csrc/cloud_kernels.hip) against
its host definition (omds_point_cloud_spheres, checked on its own in tests/test_cloud_cpu.py) and, for the self-filter, against the
CPU oracle's pass-1 distances -- all bit for bit: the voxel arithmetic is one source for host and kernels, the compaction is ordered
by construction, and the device's pass-1 values are the oracle's bits.

Shapes: a compaction block is 1 024 cells and a counting workgroup 256 points.  P = 1; 5 003 points in 16 x 16 x 8 (two whole blocks);
70 001 points in 40 x 40 x 41 = 65 600 cells (65 blocks, the last one 64 cells; 274 counting workgroups, the last one 113 points;
about 39 000 spheres, so the block offsets matter and the obstacle buffers grow); 37 x 29 x 1 = 1 073 cells (one whole block and 49
cells).  The self-filter's candidates: 793 (16-row pass-1 tiles), 5 435 (32-row tiles) and the 39 000 of the large case (64-row
tiles): every tile height the one-state launch can take below max_spheres."""
import functools

import numpy as np
import pytest

from cloud_cases import F32, edge_points, spec_of
from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

K = 5
PAD = (10.0, 10.0, 10.0, 0.0)      # cloud_spec's default pad sphere
ERR_INVALID_ARG, ERR_NOT_INITIALISED, ERR_UNSUPPORTED = 1, 4, 5


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def host_list(pts, spec):
    from optimalmodulationds_amd.engine import point_cloud_spheres
    return point_cloud_spheres(pts, spec, cap=65536)


@functools.lru_cache(maxsize=None)
def _net(kind):
    return orc.Mlp.from_npz(weights_path(kind))


def _q0():
    from optimalmodulationds_amd import scenes
    return np.asarray(scenes.FRANKA_Q0, F32)


def _engine(kind="franka", N=32, H=3, k=K, max_obs=64, ignored=0):
    from optimalmodulationds_amd.engine import Engine
    n = {"franka": 7, "toy2": 2, "planar2": 2, None: 7}[kind]
    e = Engine(n, N, H, k, max_obs=max_obs)
    if kind is not None:
        m = _net(kind)
        e.set_mlp(m.W, m.b, act=m.act)
    e.params.ignored_links = ignored
    e.push_params()
    return e


def scene_of(e, n_spheres):
    """the scene in force, split into the real spheres and the padding"""
    got = e.get_obstacles()
    assert got.shape == (e.n_obs, 4) and e.n_obs == max(n_spheres, e.k)
    return got[:n_spheres], got[n_spheres:]


# ---- device equals definition -------------------------------------------------------------------------------------------------
def _definition_case(name):
    rng = np.random.RandomState(21)
    if name == "one-point":
        return spec_of((-0.5, -0.25, 0.0), 0.0625, (16, 16, 8)), np.array([[0.3, 0.2, 0.1]], F32)
    if name in ("5003-min1", "5003-min3"):
        spec = spec_of((-0.5, -0.25, 0.0), 0.0625, (16, 16, 8), min_points=3 if name.endswith("3") else 1)
        edge = edge_points(spec)
        lattice = (rng.randint((-560, -300, -50), (560, 820, 560), (5003 - len(edge), 3)) / 1024.0).astype(F32)      # 2^-10 lattice
        return spec, np.concatenate([lattice, edge])
    if name == "70001":
        spec = spec_of((-1.0, -1.0, -0.5), 0.05, (40, 40, 41), max_spheres=65536)
        edge = edge_points(spec)
        return spec, np.concatenate([rng.uniform((-1.05, -1.05, -0.55), (1.05, 1.05, 1.6), (70001 - len(edge), 3)).astype(F32), edge])
    if name == "37x29x1":
        spec = spec_of((-0.5, 0.25, 1.0), 0.0625, (37, 29, 1), radius=0.07)
        edge = edge_points(spec)
        cloud = rng.uniform((-0.6, 0.2, 0.95), (1.9, 2.1, 1.1), (3001 - len(edge), 3)).astype(F32)
        return spec, np.concatenate([cloud, edge])
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one-point", "5003-min1", "5003-min3", "70001", "37x29x1"])
def test_device_list_is_the_definition(name):
    """q = None on a context without a network: the scene is the host definition's list (plus padding), whatever the order of the
    points and wherever they live"""
    import torch
    spec, pts = _definition_case(name)
    want = host_list(pts, spec)
    assert len(pts) == {"one-point": 1, "5003-min1": 5003, "5003-min3": 5003, "70001": 70001, "37x29x1": 3001}[name]
    assert len(want) >= (1 if name == "one-point" else 100)
    e = _engine(None)
    n_spheres, n_occ = e.set_obstacles_from_cloud(pts, spec)
    assert (n_spheres, n_occ) == (len(want), len(want))
    real, pad = scene_of(e, n_spheres)
    assert np.array_equal(bits(real), bits(want)), f"{name}: the device list is not the definition's"
    assert (pad == F32(PAD)).all()
    assert e.max_obs >= e.n_obs
    shuffled = pts[np.random.RandomState(5).permutation(len(pts))]
    assert e.set_obstacles_from_cloud(shuffled, spec) == (n_spheres, n_occ)
    assert np.array_equal(bits(scene_of(e, n_spheres)[0]), bits(want)), f"{name}: the list depends on the order of the points"
    on_dev = torch.from_numpy(np.ascontiguousarray(shuffled)).to(f"cuda:{e.device}")
    assert e.set_obstacles_from_cloud(on_dev, spec) == (n_spheres, n_occ)
    assert np.array_equal(bits(scene_of(e, n_spheres)[0]), bits(want)), f"{name}: a device-resident cloud gives another list"
    e.close()


# ---- self-filter --------------------------------------------------------------------------------------------------------------
def _filter_spec(margin):
    from optimalmodulationds_amd.engine import cloud_spec
    return cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), max_spheres=8192, self_margin=margin)


@functools.lru_cache(maxsize=None)
def _filter_case():
    """the cloud of the issue, its candidates, and the oracle's distance of every candidate for both sets of ignored links"""
    lo, ext = np.array((-0.8, -0.8, -0.1), F32), np.array((32, 32, 28)) * 0.05
    pts = (lo + np.random.RandomState(7).uniform(0, 1, (6000, 3)) * ext).astype(F32)
    cand = host_list(pts, _filter_spec(0.0))
    assert len(cand) == 5435
    d = {ign: orc.pass1_mindist(_net("franka"), _q0()[None], cand, links)[1][0] for ign, links in ((0, []), (0b111, [0, 1, 2]))}
    return pts, cand, d


def kept_by(d, margin):
    return ~(d <= F32(margin))


@pytest.mark.parametrize("ignored", [0, 0b111])
@pytest.mark.parametrize("margin", [0.0, 0.03, 0.1])
def test_self_filter_keeps_exactly_the_oracles_set(margin, ignored):
    pts, cand, d = _filter_case()
    keep = kept_by(d[ignored], margin)
    assert keep.sum() >= 10 and (~keep).sum() >= 10
    e = _engine("franka", ignored=ignored)
    n_spheres, n_occ = e.set_obstacles_from_cloud(pts, _filter_spec(margin), q=_q0())
    assert (n_spheres, n_occ) == (int(keep.sum()), 5435)
    assert np.array_equal(bits(scene_of(e, n_spheres)[0]), bits(cand[keep]))
    e.close()


def test_self_filter_counts_of_the_issue():
    """the table of the issue, from the oracle alone"""
    _, _, d = _filter_case()
    assert [int((~kept_by(d[0], mg)).sum()) for mg in (0.0, 0.03, 0.1)] == [85, 133, 315]
    assert int((~kept_by(d[0b111], 0.03)).sum()) == 82


@pytest.mark.parametrize("ignored", [0, 0b111])
def test_self_filter_distances_are_those_of_dist_grad(ignored):
    """a fresh context with the candidates as its scene: the pass-1 row of omds_dist_grad at q is the oracle's, so the set the filter
    kept is the set of that row"""
    _, cand, d = _filter_case()
    e = _engine("franka", max_obs=8192, ignored=ignored)
    e.set_obstacles(cand)
    mind = e.dist_grad(_q0()[None], want_mindist=True)[2][0]
    assert np.array_equal(bits(mind), bits(d[ignored]))
    e.close()


def test_self_filter_on_the_large_grid():
    """39 000 candidates as the obstacle rows of one state: 64-row pass-1 tiles, grown buffers, several compaction blocks twice"""
    spec, pts = _definition_case("70001")
    spec.self_margin = 0.05
    cand = host_list(pts, spec)
    keep = kept_by(orc.pass1_mindist(_net("franka"), _q0()[None], cand, [0, 1, 2])[1][0], 0.05)
    assert len(cand) > 32768 and keep.sum() >= 10 and (~keep).sum() >= 10
    e = _engine("franka", ignored=0b111)
    assert e.set_obstacles_from_cloud(pts, spec, q=_q0()) == (int(keep.sum()), len(cand))
    assert np.array_equal(bits(scene_of(e, int(keep.sum()))[0]), bits(cand[keep]))
    e.close()


@pytest.mark.parametrize("kind,q,cols,margin", [("toy2", (-5.0, 0.0), [0, 1, 3], 2.0), ("planar2", (0.4, -0.9), [0, 1, 2, 3], 1.0)])
def test_self_filter_in_the_plane(kind, q, cols, margin):
    """a grid one cell high.  toy2 is the planar-point network (3 (n + 2) inputs: the z of a sphere is not an input), planar2 the
    two-joint planar arm whose network does take z"""
    from optimalmodulationds_amd.engine import cloud_spec
    lo, dims = np.array((-8.0, -8.0, -0.25), F32), np.array((32, 32, 1))
    pts = (lo + np.random.RandomState(11).uniform(0, 1, (1500, 3)) * (dims * 0.5)).astype(F32)
    spec = cloud_spec(lo, 0.5, dims, self_margin=margin)
    cand = host_list(pts, spec)
    q = np.array(q, F32)
    keep = kept_by(orc.pass1_mindist(_net(kind), q[None], cand[:, cols], [])[1][0], margin)
    assert keep.sum() >= 10 and (~keep).sum() >= 10
    e = _engine(kind, k=2)
    assert e.set_obstacles_from_cloud(pts, spec, q=q) == (int(keep.sum()), len(cand))
    assert np.array_equal(bits(e.get_obstacles()), bits(cand[keep]))
    e.close()


# ---- the context around it ----------------------------------------------------------------------------------------------------
def _samples(N, seed=3, Kp=3):
    rng = np.random.RandomState(seed)
    mu = (_q0() + 0.2 * rng.standard_normal((N, Kp, 7))).astype(F32)
    return mu, np.ones((N, Kp), F32), rng.standard_normal((N, Kp, 7)).astype(F32)


def test_growth_keeps_handle_network_and_ds():
    from optimalmodulationds_amd import scenes
    pts, cand, d = _filter_case()
    e = _engine("franka", N=32, max_obs=64, ignored=0b111)
    e.params.dt, e.params.dst_thr = 0.5, 0.01
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_policy_samples(*_samples(32))
    handle = e.h.value
    keep = kept_by(d[0b111], 0.03)
    assert e.set_obstacles_from_cloud(pts, _filter_spec(0.03), q=_q0()) == (int(keep.sum()), 5435)
    assert e.h.value == handle and e.max_obs >= 5435 > 64 and e.n_obs == int(keep.sum())
    mind = e.dist_grad(_q0()[None], want_mindist=True)[2][0]           # the network survived: the new scene's row is the oracle's
    assert np.array_equal(bits(mind), bits(d[0b111][keep]))
    e.propagate(_q0())                                                  # ... and so did the DS and the samples
    assert np.isfinite(e.get_rollouts()["all_traj"]).all()
    e.close()


@pytest.mark.parametrize("screen", [False, True])
def test_same_scene_as_set_obstacles(screen):
    """300 spheres of the self-filtered list: through omds_set_obstacles on one context, through the cloud path (their centres as the
    cloud, the filter on) on another; one propagate each, every array of the rollouts identical.  With screening on, both contexts
    have calibrated on another scene before, so the new one goes through ScreenHost::scene_changed on both"""
    from optimalmodulationds_amd import scenes
    _, cand, d = _filter_case()
    scene = np.ascontiguousarray(cand[kept_by(d[0b111], 0.03)][:300])
    N, q = 96, _q0()
    ctxs = []
    for _ in range(2):
        e = _engine("franka", N=N, H=3, max_obs=512, ignored=0b111)
        e.params.dt, e.params.dst_thr = 0.5, 0.01
        e.push_params()
        e.set_ds(scenes.FRANKA_QF)
        e.set_policy_samples(*_samples(N))
        if screen:
            e.set_screening(1)
            e.set_obstacles(scenes.shelf_scene())
            e.propagate(q)
            assert e.screen_stats()["calibrations"] == 1
        ctxs.append(e)
    a, b = ctxs
    a.set_obstacles(scene)
    assert b.set_obstacles_from_cloud(scene[:, :3], _filter_spec(0.03), q=q) == (300, 300)
    assert np.array_equal(bits(b.get_obstacles()), bits(scene)) and np.array_equal(bits(a.get_obstacles()), bits(scene))
    a.propagate(q)
    b.propagate(q)
    ra, rb = a.get_rollouts(), b.get_rollouts()
    assert set(ra) == set(rb) and len(ra) >= 6
    for name in ra:
        assert np.array_equal(bits(ra[name]), bits(rb[name])), name
    if screen:
        sa, sb = a.screen_stats(), b.screen_stats()
        assert sa["active"] and sb["active"] and sa["calibrations"] == sb["calibrations"] and sa["eps"] == sb["eps"]
    a.close()
    b.close()


def test_horizon_is_cleared():
    from optimalmodulationds_amd import scenes
    pts, _, _ = _filter_case()
    e = _engine("franka", max_obs=512)
    obs = scenes.shelf_scene()
    e.set_obstacles(obs)
    e.set_obstacle_motion(np.full((obs.shape[0], 3), 0.1, F32))
    assert e.get_obstacle_horizon()[1] == 1
    e.set_obstacles_from_cloud(pts, _filter_spec(0.0))
    table, mode = e.get_obstacle_horizon()
    assert mode == 0 and np.array_equal(bits(table[-1]), bits(e.get_obstacles()))
    e.close()


def test_padding_up_to_n_closest():
    from optimalmodulationds_amd.engine import cloud_spec
    pad = (3.0, -2.0, 1.5, 0.25)
    spec = cloud_spec((0.0, 0.0, 0.0), 0.25, (4, 4, 4), pad=pad)
    e = _engine("franka", k=5)
    for pts, n in ((np.zeros((0, 3), F32), 0), (np.array([[0.3, 0.3, 0.3]] * 2, F32), 1)):
        assert e.set_obstacles_from_cloud(pts, spec) == (n, n)
        real, fill = scene_of(e, n)
        assert e.n_obs == 5 and len(fill) == 5 - n and (fill == F32(pad)).all()
        if n:
            assert np.array_equal(real[0], np.array([0.375, 0.375, 0.375, 0.8660254 * 0.25], F32))
    e.close()


@pytest.mark.parametrize("case", ["one-kept", "three-of-four", "all-dropped", "one-dropped"])
def test_self_filter_with_fewer_candidates_or_survivors_than_n_closest(case):
    """the filter's pass 1 over 1 .. 4 obstacle rows, and lists of 0 .. 3 survivors that are filled up with the pad sphere; one point
    sits on the arm at FRANKA_Q0 (on the segment between two of its link end points), the others far from it"""
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import cloud_spec
    ends = orc.link_endpoints(_q0(), scenes.franka_dh_params())
    on_arm = (0.5 * (ends[3] + ends[4])).astype(F32)
    far = np.array([[0.6, 0.6, 1.2], [-0.7, 0.5, 0.2], [0.1, -0.75, 1.0]], F32)
    pts, margin = {"one-kept": (far[:1], 0.03), "three-of-four": (np.concatenate([far, on_arm[None]]), 0.03),
                   "all-dropped": (np.concatenate([far, on_arm[None]]), 10.0), "one-dropped": (on_arm[None], 0.03)}[case]
    pad = (3.0, -2.0, 1.5, 0.25)
    spec = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), self_margin=margin, pad=pad)
    cand = host_list(pts, spec)
    keep = kept_by(orc.pass1_mindist(_net("franka"), _q0()[None], cand, [0, 1, 2])[1][0], margin)
    assert (len(cand), int(keep.sum())) == {"one-kept": (1, 1), "three-of-four": (4, 3), "all-dropped": (4, 0), "one-dropped": (1, 0)}[case]
    e = _engine("franka", k=5, ignored=0b111)
    assert e.set_obstacles_from_cloud(pts, spec, q=_q0()) == (int(keep.sum()), len(cand))
    real, fill = scene_of(e, int(keep.sum()))
    assert e.n_obs == 5 and np.array_equal(bits(real), bits(cand[keep])) and (fill == F32(pad)).all()
    e.close()


def _code(err):
    return int(str(err.value).split("omds error ")[1].split(":")[0])


def test_errors():
    from optimalmodulationds_amd import _lib as L, scenes
    from optimalmodulationds_amd.engine import cloud_spec
    pts, _, _ = _filter_case()
    # a joint state without a network
    e = _engine(None)
    with pytest.raises(L.OmdsError) as err:
        e.set_obstacles_from_cloud(pts, _filter_spec(0.0), q=_q0())
    assert _code(err) == ERR_NOT_INITIALISED and e.n_obs == 0
    e.close()
    # ... on a network wider than 256; without the joint state the same context takes the cloud
    rng = np.random.RandomState(1)
    dims = [30, 512, 512, 9]
    W = [rng.uniform(-0.1, 0.1, (dims[i + 1], dims[i])).astype(F32) for i in range(3)]
    e = _engine(None)
    e.set_mlp(W, [np.zeros(dims[i + 1], F32) for i in range(3)])
    with pytest.raises(L.OmdsError) as err:
        e.set_obstacles_from_cloud(pts, _filter_spec(0.0), q=_q0())
    assert _code(err) == ERR_UNSUPPORTED
    assert e.set_obstacles_from_cloud(pts, _filter_spec(0.0)) == (5435, 5435) and e.n_obs == 5435
    e.close()
    # more occupied cells than max_spheres: the scene stays, the count comes back
    e = _engine("franka", max_obs=512)
    obs = scenes.shelf_scene()
    e.set_obstacles(obs)
    small = cloud_spec((-0.8, -0.8, -0.1), 0.05, (32, 32, 28), max_spheres=5434)
    for q in (None, _q0()):
        with pytest.raises(L.OmdsError) as err:
            e.set_obstacles_from_cloud(pts, small, q=q)
        assert _code(err) == ERR_INVALID_ARG and err.value.n_occupied == 5435
        assert e.n_obs == obs.shape[0] and np.array_equal(bits(e.get_obstacles()), bits(obs))
    small.max_spheres = 5435
    assert e.set_obstacles_from_cloud(pts, small) == (5435, 5435)
    with pytest.raises(L.OmdsError) as err:                                    # a bad spec is refused before anything runs
        e.set_obstacles_from_cloud(pts, cloud_spec((0, 0, 0), 0.0, (4, 4, 4)))
    assert _code(err) == ERR_INVALID_ARG and e.n_obs == 5435
    e.close()


def test_facade_updates_the_scene_from_a_cloud():
    import torch
    from optimalmodulationds_amd import MPPI, LinDS, RobotSdfCollisionNet, scenes
    pts, cand, d = _filter_case()
    nn_model = RobotSdfCollisionNet(in_channels=10, out_channels=9, layers=[256] * 4, skips=[])
    nn_model.load_weights(weights_path("franka"), {})
    dh = torch.tensor(scenes.franka_dh_params())
    q_f = torch.tensor(scenes.FRANKA_QF)
    mppi = MPPI(torch.tensor(_q0()), q_f, dh, torch.tensor(scenes.shelf_scene()), 0.5, 3, 32, [LinDS(q_f)], dh[:, 2], nn_model, K)
    mppi.dst_thr = 0.01
    lo, hi = (-0.8, -0.8, -0.1), (0.8, 0.8, 1.3)
    mppi.update_obstacles(scenes.shelf_scene(), velocities=np.zeros((294, 3), F32), moving_frame=True)
    assert mppi._engine.get_obstacle_frame()[0] is True
    assert mppi.ignored_links == [0, 1, 2]
    want = cand[kept_by(d[0b111], 0.03)]
    assert mppi.update_obstacles_from_cloud(pts, 0.05, lo, hi, self_margin=0.03, max_spheres=8192) == (len(want), 5435)
    assert mppi.n_obs == len(want) and np.array_equal(bits(mppi.obs.numpy()), bits(want))
    assert mppi._engine.get_obstacle_frame()[0] is False and mppi._engine.get_obstacle_horizon()[1] == 0      # as update_obstacles(obs) leaves it
    out = mppi.propagate()
    assert np.isfinite(out[0].numpy()).all()
    assert mppi.update_obstacles_from_cloud(torch.tensor(pts), 0.05, lo, hi, max_spheres=8192) == (5435, 5435)      # no filter
    assert np.array_equal(bits(mppi.obs.numpy()), bits(cand))
