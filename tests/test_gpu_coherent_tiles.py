"""Block-ordered pass-1 tiles (csrc/tile_order.hip, propagate.hip: enqueue_dense): every full launch of the compacting kernel forms
its tiles from 16 (8) rollouts x 4 obstacles that are neighbours in a key order, so that the rows of a tile fire alike.  A row's
bits do not depend on its tile-mates: every tensor of get_rollouts() equals the natural order's (OMDS_FLAG_NATURAL_TILES), the
pass-1 matrix keeps the caller's obstacle index (ties of the top-k by lower index), and the block order executes fewer chunks.
Through the hooks of include/omds_test_tiles.h (test library only): both orders are permutations, and the whole pass-1 matrix of
the last step equals the natural launch's bit for bit -- the same matrix under the unchanged top-k gives the same indices."""
import numpy as np
import pytest

from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

K_CLOSEST, K_POLICY = 5, 3


@pytest.fixture(scope="module")
def franka():
    return orc.Mlp.from_npz(weights_path("franka"))


def _run(m, obs, N, H, q, seed, flags=None, vel=None):
    """One propagate on the dense route, on the test library; returns (rollouts, skip statistics, last step's Dmin [N, O],
    (rperm, operm) of a block-ordered run | None)."""
    from optimalmodulationds_amd import _lib as L, scenes
    from optimalmodulationds_amd.engine import Engine
    flags = L.FLAG_BLOCK_TILES if flags is None else flags     # the block order at these small batches (by itself: from 262 144 pairs on)
    O = obs.shape[0]
    assert N * O > 24576, "the Dense route (k_pass1 + k_tail) runs above the Emit route's 24 576 pairs"
    rng = np.random.RandomState(seed)
    q0 = np.asarray(q, np.float32).reshape(-1, 7)[0]
    mu = (q0 + 0.2 * rng.standard_normal((N, K_POLICY, 7))).astype(np.float32)
    samples = (mu, np.ones((N, K_POLICY), np.float32), rng.standard_normal((N, K_POLICY, 7)).astype(np.float32))
    e = Engine(7, N, H, K_CLOSEST, max_obs=512, flags=flags, lib=L.load_test_hooks())
    e.set_mlp(m.W, m.b)
    e.set_obstacles(obs)
    if vel is not None:
        e.set_obstacle_motion(vel)
    e.params.dt = 0.5
    e.params.dst_thr = 0.01
    e.params.ignored_links = 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    e.set_policy_samples(*samples)
    e.propagate(q)
    got = e.get_rollouts()
    st = e.pass1_skip_stats()
    dmin = e.test_read_dmin()
    orders = None if flags & L.FLAG_NATURAL_TILES else e.test_tile_orders()
    e.close()
    return got, st, dmin, orders


def _check_orders(orders, N, O):
    rperm, operm = orders
    assert np.array_equal(np.sort(rperm), np.arange(N)), "rperm is not a permutation of the rollouts"
    assert np.array_equal(np.sort(operm), np.arange(O)), "operm is not a permutation of the obstacles"


def _topk(dmin, k=K_CLOSEST):
    """topk_row's selection: ascending, ties by lower index"""
    return np.argsort(dmin, axis=1, kind="stable")[:, :k]


def _q_cur(seed):
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(seed)
    return (np.asarray(scenes.FRANKA_Q0, np.float32) + 0.1 * rng.standard_normal(7)).astype(np.float32)


def _same(a, b, what):
    for name in a:
        assert np.array_equal(a[name], b[name]), f"{what}: {name} differs between the block order and the natural order"


def _total_chunks(st):
    return sum(st["chunks"]) * st["tiles"]


@pytest.mark.parametrize("N", [100, 132])
def test_remainders(franka, N):
    """100 = 12 x 8 + 4 rollouts on 32-row tiles, 132 = 8 x 16 + 4 on 64-row tiles with one 8-block behind them; 294 = 73 x 4 + 2
    obstacles.  The tile counts are those of the block grid: the block-ordered kernel ran."""
    from optimalmodulationds_amd import _lib as L, scenes
    obs = scenes.shelf_scene()
    assert obs.shape[0] == 294
    q = _q_cur(11)
    blk, st_b, d_b, orders = _run(franka, obs, N, 3, q, 5)
    nat, st_n, d_n, _ = _run(franka, obs, N, 3, q, 5, flags=L.FLAG_NATURAL_TILES)
    _check_orders(orders, N, 294)
    assert not np.array_equal(orders[0], np.arange(N)) and not np.array_equal(orders[1], np.arange(294)), "the orders ordered nothing"
    assert np.array_equal(d_b, d_n), "the pass-1 matrix differs from the natural launch's"
    assert np.ptp(blk["all_traj"][:, 1], axis=0).max() > 0, "the rollouts must part after the first step"
    _same(blk, nat, f"N = {N}")
    # two full launches (steps 2 and 3; step 1 is the shared 294-row launch on 16-row tiles, which keep no statistics)
    blocks = (N // 16 * 74 + -(-(N % 16) // 8) * 74) if N * 294 >= 32768 else -(-N // 8) * 74
    rows = N * 294 // 64 + -(-(N * 294 % 64) // 32) if N * 294 >= 32768 else -(-N * 294 // 32)
    assert (st_b["tiles"], st_n["tiles"]) == (2 * blocks, 2 * rows)
    print(N, "tiles", st_b["tiles"], st_n["tiles"], "chunks", _total_chunks(st_b), _total_chunks(st_n))


def test_per_rollout_start(franka):
    """per_rollout = 1 with N distinct states: step 1 is a full launch already, so the key units are picked and the order formed there."""
    from optimalmodulationds_amd import _lib as L, scenes
    N = 96
    obs = scenes.shelf_scene()
    rng = np.random.RandomState(3)
    q = (_q_cur(11) + 0.3 * rng.standard_normal((N, 7))).astype(np.float32)
    blk, st_b, d_b, orders = _run(franka, obs, N, 3, q, 6)
    nat, st_n, d_n, _ = _run(franka, obs, N, 3, q, 6, flags=L.FLAG_NATURAL_TILES)
    _same(blk, nat, "per-rollout start")
    _check_orders(orders, N, 294)
    assert np.array_equal(d_b, d_n), "the pass-1 matrix differs from the natural launch's"
    assert (st_b["tiles"], st_n["tiles"]) == (3 * 12 * 74, 3 * 882), "all three steps are full launches: 12 x 74 blocks, 28 224 / 32 tiles"


def test_duplicate_spheres_keep_the_lower_index(franka):
    """Exact duplicates of spheres, inside one block of four (neighbours in any key order: their keys are equal) and across blocks
    (a dozen copies of one sphere): their pass-1 values tie, and the selected indices must be the lower ones as in the natural order
    -- the matrix keeps the caller's obstacle index."""
    from optimalmodulationds_amd import _lib as L, scenes
    obs = scenes.shelf_scene().copy()
    N = 100
    q = _q_cur(11)
    base, *_ = _run(franka, obs, N, 2, q, 7, flags=L.FLAG_NATURAL_TILES)
    # the sphere closest to the start state's rollouts decides the outputs: duplicate the spheres of that neighbourhood
    from optimalmodulationds_amd.engine import Engine
    e = Engine(7, 1, 1, K_CLOSEST, max_obs=512)
    e.set_mlp(franka.W, franka.b)
    e.set_obstacles(obs)
    e.params.ignored_links = 0b111
    e.push_params()
    _, _, _, idx = e.dist_grad(q[None], want_mindist=True, want_idx=True)
    e.close()
    near = [int(i) for i in np.asarray(idx).reshape(-1)[:3]]
    obs[200:212] = obs[near[0]]          # a dozen copies across blocks
    obs[20:22] = obs[near[1]]            # a pair
    obs[290:294] = obs[near[2]]          # the last (partial) blocks
    blk, _, d_b, orders = _run(franka, obs, N, 2, q, 7)
    nat, _, d_n, _ = _run(franka, obs, N, 2, q, 7, flags=L.FLAG_NATURAL_TILES)
    _same(blk, nat, "duplicate spheres")
    _check_orders(orders, N, 294)
    assert np.array_equal(d_b[:, 200:212], np.repeat(d_b[:, 200:201], 12, axis=1)), "duplicates must tie bit for bit"
    assert np.array_equal(d_b[:, 290:294], np.repeat(d_b[:, 290:291], 4, axis=1)) and np.array_equal(d_b[:, 20], d_b[:, 21])
    assert np.array_equal(d_b, d_n), "the pass-1 matrix differs: the obstacle index of an entry moved"
    sel = _topk(d_b)
    assert np.array_equal(sel, _topk(d_n))
    dup = np.zeros(294, bool); dup[201:212] = True; dup[21] = True; dup[291:294] = True     # the higher-index copies
    assert np.isin(sel, [200, 20, 290]).any(), "no duplicated sphere is among the selected: the case checks nothing"
    # a selected higher copy is only ever selected together with every lower copy of its sphere
    for t in range(N):
        for first, last in ((200, 212), (20, 22), (290, 294)):
            got = sorted(o for o in sel[t] if first <= o < last)
            assert got == list(range(first, first + len(got))), f"rollout {t}: copies {got} selected, not the lowest of {first}..{last - 1}"
    assert not all(np.array_equal(blk[k], base[k]) for k in blk), "the duplicates were meant to change the scene"


def test_obstacle_horizon_reads_every_slab_under_slab_zeros_order(franka):
    """A moving scene: step i reads slab i - 1 of the obstacle horizon under the order formed on slab 0."""
    from optimalmodulationds_amd import _lib as L, scenes
    obs = scenes.shelf_scene()
    rng = np.random.RandomState(9)
    vel = (0.2 * rng.standard_normal((obs.shape[0], 3))).astype(np.float32)
    q = _q_cur(11)
    blk, _, d_b, orders = _run(franka, obs, 100, 4, q, 8, vel=vel)
    nat, _, d_n, _ = _run(franka, obs, 100, 4, q, 8, flags=L.FLAG_NATURAL_TILES, vel=vel)
    still, *_ = _run(franka, obs, 100, 4, q, 8, flags=L.FLAG_NATURAL_TILES)
    _same(blk, nat, "obstacle horizon")
    _check_orders(orders, 100, 294)
    assert np.array_equal(d_b, d_n), "the pass-1 matrix of slab 3 differs from the natural launch's"
    assert not np.array_equal(nat["closest_dist_all"], still["closest_dist_all"]), "the motion was meant to change the distances"


def test_block_order_executes_fewer_chunks(franka):
    """omds_pass1_skip_stats after one propagate at N = 128, H = 6: the block order multiplies strictly fewer chunks in total."""
    from optimalmodulationds_amd import _lib as L, scenes
    obs = scenes.shelf_scene()
    q = _q_cur(11)
    blk, st_b, _, _ = _run(franka, obs, 128, 6, q, 4)
    nat, st_n, _, _ = _run(franka, obs, 128, 6, q, 4, flags=L.FLAG_NATURAL_TILES)
    _same(blk, nat, "N = 128, H = 6")
    cb, cn = _total_chunks(st_b), _total_chunks(st_n)
    print("chunks executed: block order", cb, st_b, "natural", cn, st_n, "ratio", cb / cn)
    assert st_b["tiles"] > 0 and st_n["tiles"] > 0
    assert cb < cn, f"the block order executed {cb} chunks, the natural order {cn}"
