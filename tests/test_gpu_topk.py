"""The selection of the k closest obstacles (csrc/topk_device.h: topk_row) against tests/policy_ref.py::topk_ref, index by index (run
on a real MI355X: ``pytest -m gpu``).  topk_row has two implementations -- rows of up to 512 entries on 64-bit keys in registers,
longer rows on a float loop -- and the rule at the top of the header holds for both: order by (value, index), -0 equal to +0, a NaN
never picked, +-inf ordinary values, index 0 once a row has run dry.

  a. directly, through the test hook omds_test_topk (the production launcher on given rows): O on both sides of 64 and of 512,
     k in {1, 5, 64}, B = 9 (the last workgroup holds one row); distinct values, ties, constant rows, descending rows, the minimum in
     every lane slot that matters, NaNs, infinities, fewer than k pickable entries.
  b. through omds_dist_grad and omds_propagate with the Franka network on scenes of 64 .. 1100 spheres whose nearest spheres are
     duplicated verbatim (what a padded sensed scene holds): closest_idx is topk_ref of the device's own min-distance row, that row is
     the oracle's bit for bit, and the step's distance is the oracle's bit for bit on the default, unfused and tail-forward routes.

The scenes of b have 64 spheres or more: none of them runs the in-wave selection of k_step_small (scenes of up to 32 spheres)."""
import functools

import numpy as np
import pytest

import policy_ref as pr
from helpers import weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu
F32 = np.float32
B = 9
SIZES = (1, 5, 63, 64, 65, 511, 512, 513, 1024, 1500)
CASES = [(O, k) for O in SIZES for k in (1, 5, 64) if k <= O]


def _select(rows, k):
    from optimalmodulationds_amd import _lib
    return _lib.select_topk(rows, k)


def _check(rows, k, what):
    rows = np.ascontiguousarray(rows, F32)
    got = _select(rows, k)
    for b, row in enumerate(rows):
        want = pr.topk_ref(row, k)
        assert np.array_equal(got[b], want), f"{what}, O {rows.shape[1]} k {k} row {b}: {got[b][:12]} != {want[:12]} (first difference at position {int(np.argmax(got[b] != want))})"


def _row_kinds(O, k, rng):
    """name -> rows [B, O]"""
    kinds = {}
    kinds["distinct"] = np.stack([rng.permutation(O) for _ in range(B)]).astype(F32) * F32(0.37) - F32(11)
    kinds["four values"] = rng.choice(np.array([-1.0, -0.0, 0.0, 0.5], F32), size=(B, O))
    kinds["all equal"] = np.repeat(np.array([0.0, -0.0, 1.5, -2.0, np.inf, -np.inf, 3e38, 1e-45, -1e-45], F32)[:, None], O, axis=1)
    kinds["descending"] = np.repeat(np.arange(O, 0, -1, dtype=F32)[None], B, axis=0) * rng.uniform(0.5, 2, (B, 1)).astype(F32)
    rows = rng.uniform(1, 2, (B, O)).astype(F32)
    for b, o in enumerate((0, 63, 64, 511, 512, O - 1, O // 2, 65, 513)):
        rows[b, min(o, O - 1)] = -5
    kinds["minimum placed"] = rows
    rows = rng.standard_normal((B, O)).astype(F32)
    rows[rng.rand(B, O) < 0.3] = np.nan
    rows[::2, 0] = np.nan
    kinds["NaNs"] = rows
    rows = rng.standard_normal((B, O)).astype(F32)
    u = rng.rand(B, O)
    rows[u < 0.2], rows[u > 0.8] = -np.inf, np.inf
    kinds["infinities"] = rows
    rows = np.full((B, O), np.nan, F32)                    # fewer than k pickable entries, +inf among them at an index above 0
    for b in range(B):
        n_ok = min(O, max(0, k - 1 - b % 3))
        where = rng.permutation(O)[:n_ok]
        rows[b, where] = rng.standard_normal(n_ok).astype(F32)
        if n_ok and b % 2 == 0:
            rows[b, where.max()] = np.inf
    kinds["fewer than k pickable"] = rows
    return kinds


@pytest.mark.parametrize("O,k", CASES)
def test_topk_rows(O, k):
    rng = np.random.RandomState(1000 * O + k)
    for name, rows in _row_kinds(O, k, rng).items():
        _check(rows, k, name)


@pytest.mark.parametrize("O", [11, 512, 513, 600])
def test_a_dry_row_repeats_index_zero_not_an_infinity(O):
    """[NaN, NaN, NaN, 7, NaN, ..., +inf at 10], k = 4 -> [3, 10, 0, 0] on both paths (the float loop used to pick the +inf again:
    after a dry round its previous pick was (+inf, 0), and the +inf at index 10 came "after" it)."""
    row = np.full(O, np.nan, F32)
    row[3], row[10] = 7, np.inf
    rows = np.repeat(row[None], B, axis=0)
    assert pr.topk_ref(row, 4).tolist() == [3, 10, 0, 0]
    assert _select(rows, 4).tolist() == [[3, 10, 0, 0]] * B


def test_hook_rejects_bad_arguments():
    from optimalmodulationds_amd import _lib
    lib = _lib.load_test_hooks()
    rows, idx = np.zeros((2, 8), F32), np.zeros((2, 9), np.int32)
    for args in ((None, 2, 8, 1, idx.ctypes.data), (rows.ctypes.data, 2, 8, 1, None), (rows.ctypes.data, 0, 8, 1, idx.ctypes.data),
                 (rows.ctypes.data, 2, 8, 9, idx.ctypes.data), (rows.ctypes.data, 2, 8, 0, idx.ctypes.data)):
        assert lib.omds_test_topk(*args) != 0


# ---- b. through the real entry points, with the Franka network ----------------------------------------------------------------------
IGN = [0, 1, 2]
NB = 8


def _states():
    from optimalmodulationds_amd import scenes
    return (scenes.FRANKA_Q0 + 0.15 * np.random.RandomState(8).standard_normal((NB, 7))).astype(F32)


@functools.lru_cache(maxsize=None)
def _net():
    return orc.Mlp.from_npz(weights_path("franka"))


@functools.lru_cache(maxsize=None)
def _scene(O):
    """The shelf and jittered copies of it, O spheres; then the 20 spheres nearest to the states are copied verbatim over other
    spheres: half of them 64 places on (the same lane of the wave, the next register or the next turn of the loop), half of them
    512 places on (on the other side of the register path's row length) where the scene is that long.  -> (scene, min-distance matrix
    of the oracle [NB, O])."""
    from optimalmodulationds_amd import scenes
    rng = np.random.RandomState(O)
    shelf = scenes.shelf_scene()
    parts = [shelf]
    while sum(p.shape[0] for p in parts) < O:
        jit = shelf.copy()
        jit[:, :3] += rng.uniform(-0.06, 0.06, (shelf.shape[0], 3)).astype(F32)
        parts.append(jit)
    obs = np.vstack(parts)[:O].astype(F32).copy()
    _, mind = orc.pass1_mindist(_net(), _states(), obs, IGN)
    src = np.argsort(mind.mean(axis=0), kind="stable")[:20]
    taken = set(src.tolist())
    for i, s in enumerate(src):
        d = (int(s) + (512 if (i % 2 and O > 512) else 64 if O > 64 else 32)) % O       # (64 spheres: the other half of the wave)
        for tries in range(O):
            if d not in taken:
                break
            d = (d + (64 if O > 64 and tries < 8 else 1)) % O
        taken.add(d)
        obs[d] = obs[s]
    _, mind = orc.pass1_mindist(_net(), _states(), obs, IGN)
    return obs, mind


def _engine(O, k, N, H, flags=0):
    from optimalmodulationds_amd import scenes
    from optimalmodulationds_amd.engine import Engine
    m = _net()
    eng = Engine(7, N, H, k, max_obs=O, flags=flags)
    eng.set_mlp(m.W, m.b)
    eng.set_obstacles(_scene(O)[0])
    eng.params.dt, eng.params.dst_thr, eng.params.ignored_links = 0.5, 0.01, 0b111
    eng.push_params()
    eng.set_ds(scenes.FRANKA_QF)
    return eng


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("O", [64, 512, 513, 1100])
def test_closest_idx_on_scenes_with_duplicates(O, k):
    obs, omind = _scene(O)
    eng = _engine(O, k, NB, 1)
    _, _, mind, idx = eng.dist_grad(_states(), want_mindist=True, want_idx=True)
    eng.close()
    assert np.array_equal(mind.view(np.uint32), omind.view(np.uint32)), "pass-1 matrix: not the oracle's bits"
    ties = 0
    for b in range(NB):
        want = pr.topk_ref(mind[b], k)
        assert np.array_equal(idx[b], want), f"O {O} k {k} state {b}: {idx[b]} != {want}"
        ties += int((np.diff(mind[b][want]) == 0).sum())
    assert k == 1 or ties > 0, "the scene was built to put exact ties among the k closest"


@pytest.mark.parametrize("flags", [0, 1, 4], ids=["default", "unfused", "tail_forward"])
@pytest.mark.parametrize("O", [512, 513, 1100])
def test_propagate_on_scenes_with_duplicates(O, flags):
    from optimalmodulationds_amd import scenes
    obs, _ = _scene(O)
    N, H, k = NB, 2, 5
    eng = _engine(O, k, N, H, flags)
    eng.set_policy_samples(np.zeros((N, 0, 7), F32), np.zeros((N, 0), F32), np.zeros((N, 0, 7), F32))
    eng.propagate(_states())
    r = eng.get_rollouts()
    eng.close()
    empty = (np.zeros((N, 0, 7), F32), np.zeros((N, 0), F32), np.zeros((N, 0, 7), F32))
    prm = orc.Params(dst_thr=0.01)
    for h in range(H):       # every step re-derived by the oracle from the device's own state
        q = r["all_traj"][:, h]
        d, g, _, _ = orc.distance_repulsion_nn(_net(), q, obs, k, IGN)
        want = (d - F32(0.01)).astype(F32)
        assert np.array_equal(r["closest_dist_all"][:, h].view(np.uint32), want.view(np.uint32)), f"step {h}: distance not the oracle's bits"
        st = orc.modulation_step(q, scenes.FRANKA_QF, d, g, *empty, prm)
        e = np.abs(r["normal"][:, h].astype(np.float64) - st["ghat"]).max() / max(1.0, float(np.abs(st["ghat"]).max()))
        assert e <= 2e-5, f"step {h}: normal {e:.2e}"
