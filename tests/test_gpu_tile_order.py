"""The ordering launches of the block-ordered pass 1 (csrc/tile_order.hip: k_share_stats, k_tile_pick, k_order_keys, k_order_rank),
looked at through the hook of include/omds_test_tiles.h (omds_test_tile_state, test library only): the results equal the natural
order's bit for bit, the orders are the stable sort of the keys with the last-ranked row in the padding, the key units, their
weights and constants are what a float64 restatement from the tables gives, the key bits are the signs of that restatement
wherever it is not marginal, the unit pick is the nearest-to-N/2 rule up to marginal rows, two fresh contexts agree, and a second
propagate on the same context (other samples, another start) still orders correctly.

Shapes: every new kernel runs several workgroups with a ragged last one -- row groups of 32 (k_share_stats), 64 rows
(k_order_keys), 16 entries (k_order_rank): N = 300, 1029, 97 and O = 294, 500 are multiples of none of them.  (The third shape is
N = 97 and not 96 = 3 x 32: 96 would fill its last row group.)  The per-rollout start keeps N = 96, whole groups on the rollout
side, ragged ones on the obstacle side.

Margins: a key bit or a firing rollout is compared only where the float64 pre-activation is at least 1e-4 from zero, roughly 10 x
the float32 error of a 21-term chain of O(1) weights plus a few ulp of sin / cos; at most 2 % of the bits may be that close (measured
on these seeds with the CPU oracle's rollouts: at most 0.2 % on any case)."""
import functools

import numpy as np
import pytest

from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

K_CLOSEST, K_POLICY, H = 5, 3, 3
KEY_UNITS, SLOTS, MARGIN = 12, 32, 1e-4


def order_pad(n):
    return ((n + 15) & ~15) + 16


@functools.lru_cache(maxsize=None)
def _franka():
    return orc.Mlp.from_npz(weights_path("franka"))


def _scene(O):
    from optimalmodulationds_amd import scenes
    obs = scenes.shelf_scene()
    assert obs.shape[0] == 294
    if O == 294:
        return obs
    far = obs.copy()
    far[:, :3] += np.float32(0.045)          # the shelf plus a shifted copy, truncated
    return np.ascontiguousarray(np.concatenate((obs, far))[:O])


def _q_cur(seed, N=None):
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(seed)
    q = (np.asarray(scenes.FRANKA_Q0, np.float32) + 0.1 * rng.standard_normal(7)).astype(np.float32)
    if N is not None:                        # per-rollout starts
        q = (q + 0.3 * rng.standard_normal((N, 7))).astype(np.float32)
    return q


def _engine(obs, N, flags):
    from optimalmodulationds_amd import _lib as L, scenes
    from optimalmodulationds_amd.engine import Engine
    m = _franka()
    assert N * obs.shape[0] > 24576, "the Dense route (k_pass1 + k_tail) runs above the Emit route's 24 576 pairs"
    e = Engine(7, N, H, K_CLOSEST, max_obs=512, flags=flags, lib=L.load_test_hooks())
    e.set_mlp(m.W, m.b)
    e.set_obstacles(obs)
    e.params.dt = 0.5
    e.params.dst_thr = 0.01
    e.params.ignored_links = 0b111
    e.push_params()
    e.set_ds(scenes.FRANKA_QF)
    return e


def _propagate(e, q, seed, block):
    """One propagate with the policy samples of `seed`: the rollouts, the last step's Dmin, the ordering state of a block-ordered run"""
    rng = np.random.RandomState(seed)
    q0 = np.asarray(q, np.float32).reshape(-1, 7)[0]
    mu = (q0 + 0.2 * rng.standard_normal((e.N, K_POLICY, 7))).astype(np.float32)
    e.set_policy_samples(mu, np.ones((e.N, K_POLICY), np.float32), rng.standard_normal((e.N, K_POLICY, 7)).astype(np.float32))
    e.propagate(q)
    return dict(got=e.get_rollouts(), dmin=e.test_read_dmin(), state=e.test_tile_state() if block else None)


# name -> (N, O, flags of the block-ordered run (None: FLAG_BLOCK_TILES), per-rollout start)
CASES = {"300x294": (300, 294, None, False), "1029x294-default": (1029, 294, 0, False), "97x500": (97, 500, None, False),
         "96x294-per-rollout": (96, 294, None, True)}
SHAPES = ["300x294", "1029x294-default", "97x500"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything the tests of a case look at, computed once and not modified: two propagates on one block-ordered context, the same two
    on a natural-order context, and the first again on a fresh block-ordered context."""
    from optimalmodulationds_amd import _lib as L
    N, O, flags, per = CASES[name]
    flags = L.FLAG_BLOCK_TILES if flags is None else flags
    obs = _scene(O)
    qs = [_q_cur(11, N if per else None), _q_cur(12, N if per else None)]
    seeds = [5, 6]
    out = dict(N=N, O=O, obs=obs, per=per)
    e = _engine(obs, N, flags)
    out["blk"] = [_propagate(e, qs[0], seeds[0], True)]
    out["stats_blk"] = e.pass1_skip_stats()
    out["blk"].append(_propagate(e, qs[1], seeds[1], True))
    e.close()
    e = _engine(obs, N, L.FLAG_NATURAL_TILES)
    out["nat"] = [_propagate(e, qs[0], seeds[0], False)]
    out["stats_nat"] = e.pass1_skip_stats()
    out["nat"].append(_propagate(e, qs[1], seeds[1], False))
    e.close()
    e = _engine(obs, N, flags)
    out["again"] = _propagate(e, qs[0], seeds[0], True)
    e.close()
    return out


def _check_same_as_natural(blk, nat, what):
    assert set(blk["got"]) == {"all_traj", "closest_dist_all", "kernel_val_all", "dot_products", "kernel_activations", "qdot", "normal"}
    for k in blk["got"]:
        assert np.array_equal(blk["got"][k], nat["got"][k]), f"{what}: {k} differs between the block order and the natural order"
    assert np.array_equal(blk["dmin"], nat["dmin"]), f"{what}: the last step's pass-1 matrix differs from the natural launch's"
    assert np.ptp(blk["got"]["all_traj"][:, H - 1], axis=0).max() > 0, "the rollouts must have parted"


def _check_orders(st, N, O, what):
    for key, perm, n in ((st["rkey"], st["rperm"], N), (st["okey"], st["operm"], O)):
        assert key.shape == (n,) and perm.shape == (order_pad(n),)
        assert np.array_equal(key & np.uint32(0xfffff), np.arange(n, dtype=np.uint32)), f"{what}: a key's low 20 bits are not its index"
        assert np.array_equal(perm[:n], np.argsort(key, kind="stable")), f"{what}: the order is not the ascending order of the keys"
        assert np.all(perm[n:] == perm[n - 1]), f"{what}: the padding does not name the last-ranked row"
        assert not np.array_equal(perm[:n], np.arange(n)), f"{what}: the order ordered nothing"


def _tables(c, q_states):
    """float64: the rollout shares [N, 256] of the states, the obstacle shares [O, 256], the rollout / obstacle rows in the 32 slots"""
    m = _franka()
    W1 = m.W[0].astype(np.float64)
    assert W1.shape == (256, 30)
    q, p = q_states.astype(np.float64), c["obs"][:, :3].astype(np.float64)
    xq, xp = np.zeros((q.shape[0], SLOTS)), np.zeros((p.shape[0], SLOTS))
    for part, fn in enumerate((lambda v: v, np.sin, np.cos)):
        xq[:, part * 10:part * 10 + 7] = fn(q)
        xp[:, part * 10 + 7:part * 10 + 10] = fn(p)
    return xq[:, :30] @ W1.T, xp[:, :30] @ W1.T, xq, xp


def _pick_states(c, run):
    """the states the key units were picked on: those of the first full launch (step 2 of a shared start, step 1 of per-rollout starts)"""
    return run["got"]["all_traj"][:, 0 if c["per"] else 1]


@pytest.mark.parametrize("name", list(CASES))
def test_same_results_as_the_natural_order(name):
    c = _case(name)
    _check_same_as_natural(c["blk"][0], c["nat"][0], name)


@pytest.mark.parametrize("name", list(CASES))
def test_orders_are_the_stable_sort_of_the_keys(name):
    c = _case(name)
    _check_orders(c["blk"][0]["state"], c["N"], c["O"], name)


def test_default_flags_chose_the_block_order():
    """1029 x 294 = 302 526 pairs >= OMDS_BLOCK_TILES_MIN_PAIRS: the tile counts of the two full launches (steps 2 and 3; step 1 is the
    shared 294-row launch on 16-row tiles, which keep no statistics) are those of the block grid.  From 65 536 pairs on a launch ends
    on 32-row tiles: the block grid over its last ceil(256 / 74) * 16 rollouts (60 x 74 blocks of 16 x 4, then 9 x 74 of 8 x 4), the
    natural launch over the rows of its last 256 64-row tiles."""
    c = _case("1029x294-default")
    N, O = c["N"], c["O"]
    assert N * O >= 65536
    ncb = -(-O // 4)
    nrb16 = max(N // 16 - -(-256 // ncb), 0)
    blocks = nrb16 * ncb + -(-(N - nrb16 * 16) // 8) * ncb
    big = max(N * O // 64 - 256, 0)
    rows = big + -(-(N * O - big * 64) // 32)
    assert (blocks, rows) == (5106, 4984)
    assert (c["stats_blk"]["tiles"], c["stats_nat"]["tiles"]) == (2 * blocks, 2 * rows)


@pytest.mark.parametrize("name", SHAPES)
def test_tile_keys_are_consistent(name):
    c = _case(name)
    m = _franka()
    st = c["blk"][0]["state"]
    unit = st["unit"]
    assert len(set(unit.tolist())) == KEY_UNITS and unit.min() >= 0 and unit.max() < 256
    assert np.array_equal(st["W"][:, :30], m.W[0][unit, :]), "W[j] is not the first layer's weights of unit[j]"
    assert np.all(st["W"][:, 30:] == 0), "padded slots of W must be zero"
    shR, shO, _, _ = _tables(c, _pick_states(c, c["blk"][0]))
    b1 = m.b[0].astype(np.float64)
    cR64, cO64 = (b1 + shO.mean(axis=0))[unit], (b1 + shR.mean(axis=0))[unit]
    print(name, "max |cR - float64|", np.abs(st["cR"] - cR64).max(), "max |cO - float64|", np.abs(st["cO"] - cO64).max())
    assert np.abs(st["cR"] - cR64).max() <= 1e-5 and np.abs(st["cO"] - cO64).max() <= 1e-5


@pytest.mark.parametrize("name", SHAPES)
def test_key_bits_against_float64(name):
    c = _case(name)
    st = c["blk"][0]["state"]
    _, _, xq, xp = _tables(c, c["blk"][0]["got"]["all_traj"][:, H - 1])      # the state entering the last step
    W = st["W"].astype(np.float64)
    for what, x, cst, key in (("rollout", xq, st["cR"], st["rkey"]), ("obstacle", xp, st["cO"], st["okey"])):
        s = cst.astype(np.float64)[None, :] + x @ W.T
        bits = ((key[:, None] >> np.uint32(20)) >> np.arange(KEY_UNITS, dtype=np.uint32)[None, :]) & np.uint32(1)
        assert np.all(key >> np.uint32(20 + KEY_UNITS) == 0)
        clear = np.abs(s) >= MARGIN
        print(name, what, "marginal bits", int((~clear).sum()), "of", clear.size)
        assert (~clear).mean() <= 0.02, f"{what}: too many marginal bits for the comparison to mean anything"
        assert np.array_equal(bits[clear] != 0, s[clear] > 0), f"{what}: {int(((bits != 0) != (s > 0))[clear].sum())} key bits differ from float64"


@pytest.mark.parametrize("name", SHAPES)
def test_pick_rule(name):
    """Every picked unit is at least as near N / 2 as every unpicked one, each side given the benefit of its marginal rollouts."""
    c = _case(name)
    m = _franka()
    N = c["N"]
    unit = c["blk"][0]["state"]["unit"]
    shR, shO, _, _ = _tables(c, _pick_states(c, c["blk"][0]))
    s = shR + (m.b[0].astype(np.float64) + shO.mean(axis=0))[None, :]
    c64, marg = (s > 0).sum(axis=0), (np.abs(s) < MARGIN).sum(axis=0)
    picked = np.zeros(256, bool)
    picked[unit] = True
    worst_in = (np.abs(2 * c64 - N) - 2 * marg)[picked].max()
    best_out = (np.abs(2 * c64 - N) + 2 * marg)[~picked].min()
    print(name, "picked", sorted(unit.tolist()), "largest picked distance", worst_in, "smallest unpicked", best_out)
    assert worst_in <= best_out


@pytest.mark.parametrize("name", SHAPES)
def test_two_fresh_contexts_agree(name):
    c = _case(name)
    a, b = c["blk"][0]["state"], c["again"]["state"]
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{name}: {k} differs between two fresh contexts with the same inputs"


@pytest.mark.parametrize("name", SHAPES)
def test_second_propagate_reuses_the_buffers(name):
    c = _case(name)
    _check_same_as_natural(c["blk"][1], c["nat"][1], name + ", second propagate")
    _check_orders(c["blk"][1]["state"], c["N"], c["O"], name + ", second propagate")
    assert not np.array_equal(c["blk"][1]["state"]["rkey"], c["blk"][0]["state"]["rkey"]), "the second propagate was meant to differ"
