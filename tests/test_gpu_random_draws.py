"""The device's random draws against the host restatement (tests/philox_ref.py), value by value (run on a real MI355X:
``pytest -m gpu``).  k_sample and k_sdf_data are pure functions of (seed, counters), so the host can say what every output must be:

  a. philox4x32_10 itself, through the test hook omds_test_philox: the published known-answer vectors, 65 536 random (counter, key)
     pairs with all-zero and all-ones words mixed in, one counter word stepped 0 .. 1023 -- the host's bits.
  b. omds_sample_policy at N = 300 (two workgroups, the second partial), n = 1 .. 7, K = 3 and K = n_kernel_max, three different
     non-zero scales: every element against float64 under the rounding bar below; seeds above 2^32, rollout offsets across 2^32,
     shards bit for bit, the mean rollout, K = 0, and one scale at a time set to zero.
  c. TensorPolicyMPPI.sample_policy with seed = 5000: the keys (5000 << 20) + 1 and + 2, beyond 32 bits.
  d. dataset.generate on four specs x four row shapes x two seeds x two cfg0 (across 2^32): bit for bit the rows of
     dataset.from_draws on the host's draws, and q and the uniform points bit for bit the host's values directly.

The bar of b (philox_ref.policy_samples): |z_dev - z_ref| <= 8 2^-24 (r + |z_ref|) per normal, r the Box-Muller radius; for
v = z s + c it is |s| times that plus 2^-23 |v_ref|.  It is derived from the 1 - 2 ulp bounds of logf, sincosf, sqrtf and the
product's rounding (about 4 ulp of the r scale, doubled), measured against float64 and never against the device.  No element is
left out.  Largest |err| / bar measured on an MI355X: 0.43 over all of b and c (per n = 1 .. 7: 0.28 0.38 0.39 0.39 0.43 0.40 0.38;
K = 50: 0.41; the facade: 0.36) -- the tests print it.  The whole module takes under 3 s there."""
import numpy as np
import pytest

import philox_ref as pr

pytestmark = pytest.mark.gpu
N = 300
SCALES = (0.5, 0.25, 3.0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- a. the generator's words -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooks():
    from optimalmodulationds_amd import _lib
    return _lib.load_test_hooks()


def _dev_philox(lib, ctr, key):
    ctr = np.ascontiguousarray(ctr, np.uint32).reshape(-1, 4)
    key = np.ascontiguousarray(key, np.uint32).reshape(-1, 2)
    assert ctr.shape[0] == key.shape[0]
    out = np.full_like(ctr, 0xDEADBEEF)
    assert lib.omds_test_philox(ctr.ctypes.data, key.ctypes.data, out.ctypes.data, ctr.shape[0]) == 0
    return out


def test_generator_bits(hooks):
    kat_c, kat_k, kat_o = (np.array([k[i] for k in pr.KAT], np.uint32) for i in range(3))
    assert np.array_equal(_dev_philox(hooks, kat_c, kat_k), kat_o)
    rng = np.random.RandomState(17)
    full = rng.randint(0, 2 ** 32, size=(65536, 6), dtype=np.uint64).astype(np.uint32)
    edge = rng.rand(65536, 6)
    full[edge < 0.1] = 0
    full[edge > 0.9] = 0xFFFFFFFF
    got = _dev_philox(hooks, full[:, :4], full[:, 4:])
    want = pr.philox4x32_10(full[:, :4], full[:, 4:])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of 65536 pairs differ, first: ctr {full[bad[0], :4]} key {full[bad[0], 4:]}: {got[bad[0]]} != {want[bad[0]]}"
    for word in range(4):     # one counter word stepped, the others fixed
        ctr = np.tile(np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], np.uint32), (1024, 1))
        ctr[:, word] = np.arange(1024, dtype=np.uint32)
        key = np.tile(np.array([0xA4093822, 0x299F31D0], np.uint32), (1024, 1))
        assert np.array_equal(_dev_philox(hooks, ctr, key), pr.philox4x32_10(ctr, key)), word
    assert hooks.omds_test_philox(None, None, None, 0) == 0 and hooks.omds_test_philox(None, None, None, 1) != 0


# ---- b. the policy sampler ---------------------------------------------------------------------------------------------------------
def _means(n, K, seed=3):
    rng = np.random.RandomState(seed + 10 * n)
    return (rng.standard_normal((K, n)).astype(np.float32), (1 + rng.rand(K)).astype(np.float32),
            rng.standard_normal((K, n)).astype(np.float32))


def _sample(eng, means, scales, K, seed, off):
    eng.sample_policy(*means, *scales, K, seed=seed, rollout_offset=off)
    return eng.get_policy_samples()


def _ratio(got, ref):
    """Largest |err| / bar of one run against philox_ref.policy_samples; asserts every element (a bar of 0 demands equality)."""
    worst = 0.0
    for name, g, r, bar in zip(("mu", "sigma", "alpha"), got, ref[:3], ref[3:]):
        assert g.shape == r.shape and np.isfinite(g).all(), name
        err = np.abs(g.astype(np.float64) - r)
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err == 0, 0.0, np.inf))
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio[i] <= 1.0, f"{name}{list(i)}: device {g[i]!r}, host {r[i]!r}, |err| {err[i]:.3e} = {ratio[i]:.3g} x the bar {bar[i]:.3e}"
        worst = max(worst, float(ratio[i]))
    return worst


@pytest.mark.parametrize("n", range(1, 8))
def test_policy_sampler_exact_layout(n):
    from optimalmodulationds_amd.engine import Engine
    K = 3
    eng = Engine(n, N, 2, 1, max_obs=8)
    means = _means(n, K)
    mu_c, sg_c, al_c = means
    worst = 0.0
    runs = {}
    for seed, off in ((42, 0), (42 + 2 ** 32, 0), ((1234 << 20) + 1, 0), (42, 2 ** 32 - 100), (42, 150)):
        runs[seed, off] = got = _sample(eng, means, SCALES, K, seed, off)
        worst = max(worst, _ratio(got, pr.policy_samples(N, n, K, means, SCALES, seed, off)))
    mu, sg, al = runs[42, 0]
    # the global rollout 0, and only it, carries alpha_c; its mu and sigma are noised like every other row's
    assert _same_bits(al[0], al_c) and np.all(mu[0] != mu_c) and np.all(sg[0] != sg_c)
    assert np.all(al[1:] != al_c[None])
    # the seed's upper word is part of the key
    assert all(not np.array_equal(a, b) for a, b in zip(runs[42 + 2 ** 32, 0], runs[42, 0]))
    # rollout_offset = 2^32 - 100: row 100 is global rollout 2^32 (low word 0, high word 1), a noised row, and rows 100 .. are not
    # the rows 0 .. of shard 0
    hmu, hsg, hal = runs[42, 2 ** 32 - 100]
    assert np.all(hal[100] != al_c) and np.all(hal[99] != al_c)
    assert np.abs(hmu[100:] - mu[:200]).mean() > 0.1 and np.abs(hsg[100:] - sg[:200]).mean() > 0.1   # independent: 0.56, 0.28
    # a shard is a window of the one stream, bit for bit
    assert all(_same_bits(a[:150], b[150:]) for a, b in zip(runs[42, 150], runs[42, 0]))
    # one scale at a time set to 0: that array is its mean, the other two keep their bits -- the three arrays use separate normals
    for i, mean in enumerate((mu_c[None], sg_c[None], al_c[None])):
        sc = list(SCALES)
        sc[i] = 0.0
        got = _sample(eng, means, sc, K, 42, 0)
        assert _same_bits(got[i], np.broadcast_to(mean, got[i].shape)), i
        assert all(_same_bits(got[j], runs[42, 0][j]) for j in range(3) if j != i), i
    # K = 0: no kernels, OK, and nothing is read back
    eng.sample_policy(None, None, None, 0.0, 0.0, 0.0, 0, seed=42, rollout_offset=0)
    assert eng.K == 0 and eng.get_policy_samples()[0].shape == (N, 0, n)
    sentinel = [np.full(s, 7.0, np.float32) for s in ((N, K, n), (N, K), (N, K, n))]
    assert eng.lib.omds_get_policy_samples(eng.h, *(s.ctypes.data for s in sentinel)) == 0
    assert all(np.all(s == 7.0) for s in sentinel)
    # ... and sampling afterwards is the same stream again
    assert all(_same_bits(a, b) for a, b in zip(_sample(eng, means, SCALES, K, 42, 0), runs[42, 0]))
    eng.close()
    print(f"policy sampler n = {n}: largest |err| / bar = {worst:.4f}")


def test_policy_sampler_every_kernel_slot():
    """n = 7 with K = n_kernel_max: the widest draw (15 normals, four blocks, the last one used for three) on every kernel slot."""
    from optimalmodulationds_amd.engine import Engine
    n = 7
    eng = Engine(n, N, 2, 1, max_obs=8)
    K = eng.Kmax
    assert K == 50
    means = _means(n, K, seed=8)
    worst = _ratio(_sample(eng, means, SCALES, K, 42, 0), pr.policy_samples(N, n, K, means, SCALES, 42, 0))
    eng.close()
    print(f"policy sampler n = 7, K = {K}: largest |err| / bar = {worst:.4f}")


# ---- c. the facade's key ----------------------------------------------------------------------------------------------------------
def test_facade_key_beyond_32_bits():
    import torch

    from optimalmodulationds_amd.engine import Engine
    from optimalmodulationds_amd.policy import TensorPolicyMPPI
    n, K = 7, 2
    eng = Engine(n, N, 2, 1, max_obs=8)
    pol = TensorPolicyMPPI(N, n, engine=eng, seed=5000)
    mu_c, sg_c, al_c = _means(n, K, seed=5)
    pol.mu_c[:K], pol.sigma_c[:K], pol.alpha_c[:K] = torch.from_numpy(mu_c), torch.from_numpy(sg_c), torch.from_numpy(al_c)
    pol.mu_s, pol.sigma_s, pol.alpha_s = (torch.tensor(s) for s in SCALES)
    pol.n_kernels = K
    assert (5000 << 20) + 1 > 2 ** 32
    worst, seen = 0.0, []
    for draw in (1, 2):
        pol.sample_policy()
        got = eng.get_policy_samples()
        seen.append(got)
        worst = max(worst, _ratio(got, pr.policy_samples(N, n, K, (mu_c, sg_c, al_c), SCALES, (5000 << 20) + draw, 0)))
        assert _same_bits(pol.mu_tmp.numpy()[:, :K], got[0])
    assert all(np.abs(a[1:] - b[1:]).mean() > 0.1 for a, b in zip(*seen))      # two draws, two keys
    eng.close()
    print(f"facade key: largest |err| / bar = {worst:.4f}")


# ---- d. the data generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pr.SDF_SHAPES, ids=lambda s: f"{s[0]}+{s[1]}")
@pytest.mark.parametrize("name", pr.SDF_NAMES)
def test_data_generator_bit_for_bit(name, shape):
    from optimalmodulationds_amd import dataset
    nu, nn = shape
    spec = pr.sdf_specs(nu, nn)[name]
    n, pd, m, R = spec.n_dof, spec.point_dims, pr.SDF_M, nu + nn
    seen = {}
    for seed in pr.SDF_SEEDS:
        for cfg0 in pr.SDF_CFG0:
            q, pu, po = pr.sdf_draws(spec, seed, cfg0, m)
            rows = dataset.generate(spec, seed=seed, cfg0=cfg0, n_cfg=m)
            assert rows.shape == (m * R, spec.cols) and np.isfinite(rows).all()
            blk = rows.reshape(m, R, -1)
            what = f"{name} {shape} seed {seed:#x} cfg0 {cfg0:#x}"
            # the host's values directly: every row's q, and the uniform points
            assert _same_bits(blk[:, :, :n], np.broadcast_to(q[:, None, :], (m, R, n))), what + ": q"
            assert _same_bits(blk[:, :nu, n:n + pd], pu), what + ": uniform points"
            # the same device arithmetic behind the host's draws: all columns, near points and labels included
            want = dataset.from_draws(spec, q, pu, po)
            bad = np.argwhere(_bits(rows) != _bits(want))
            assert bad.size == 0, f"{what}: {bad.shape[0]} values differ from from_draws, first at (row, column) {bad[0]} (row {bad[0][0] % R} of its configuration)"
            seen[seed, cfg0] = rows
    a, b = seen[pr.SDF_SEEDS[0], 0], seen[pr.SDF_SEEDS[1], 0]
    assert not np.any(np.all(a[:, :n] == b[:, :n], axis=1))                     # the seed's upper word is part of the key
    lo, hi = seen[pr.SDF_SEEDS[0], 0], seen[pr.SDF_SEEDS[0], pr.SDF_CFG0[1]]
    assert not np.any(np.all(hi[2 * R:, :n] == lo[:3 * R, :n], axis=1))         # configurations 2^32 .. are not configurations 0 ..
