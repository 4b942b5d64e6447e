"""The host reference of the device's random draws (tests/philox_ref.py) checked on its own, without a GPU: the published
known-answer vectors of Philox4x32-10, a scalar plain-int restatement, Box-Muller's corner inputs, the single rounding of the data
generator's lo + w u against exact rational arithmetic on every case tests/test_gpu_random_draws.py runs, and the moments of the
policy samples (a sanity check of the reference, loose bounds)."""
from fractions import Fraction

import numpy as np
import pytest

import philox_ref as pr


def _philox_scalar(ctr, key, rounds=10):
    """Philox4x32 on Python ints, from the paper's round function (independent of the vectorised one: no numpy)."""
    c0, c1, c2, c3 = (int(x) for x in ctr)
    k0, k1 = (int(x) for x in key)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
    return c0, c1, c2, c3


def test_known_answer_vectors():
    for ctr, key, out in pr.KAT:
        assert tuple(int(x) for x in pr.philox4x32_10(ctr, key)) == out
        assert _philox_scalar(ctr, key) == out
    got = pr.philox4x32_10([k[0] for k in pr.KAT], [k[1] for k in pr.KAT])           # and as one batch
    assert np.array_equal(got, np.array([k[2] for k in pr.KAT], np.uint32))
    assert tuple(int(x) for x in pr.philox4x32_10(pr.KAT[2][0], pr.KAT[2][1], rounds=9)) != pr.KAT[2][2]


def test_vectorised_against_scalar():
    rng = np.random.RandomState(11)
    ctr = rng.randint(0, 2 ** 32, size=(4000, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.randint(0, 2 ** 32, size=(4000, 2), dtype=np.uint64).astype(np.uint32)
    edge = rng.rand(4000, 6)
    full = np.concatenate((ctr, key), axis=1)
    full[edge < 0.1] = 0
    full[edge > 0.9] = 0xFFFFFFFF
    ctr, key = full[:, :4], full[:, 4:]
    got = pr.philox4x32_10(ctr, key)
    want = np.array([_philox_scalar(c, k) for c, k in zip(ctr.tolist(), key.tolist())], np.uint32)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    # broadcasting a single key over many counters is the same function
    assert np.array_equal(pr.philox4x32_10(ctr, key[0]), np.array([_philox_scalar(c, key[0]) for c in ctr.tolist()], np.uint32))


def test_words64():
    lo, hi = pr.words64(np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 5 + (7 << 32)], dtype=object))
    assert lo.tolist() == [0, 1, 0xFFFFFFFF, 0, 0xFFFFFFFF, 5] and hi.tolist() == [0, 0, 0, 1, 0xFFFFFFFF, 7]


def test_box_muller_corners():
    A = np.array([0, 1, 2 ** 32 - 2, 2 ** 32 - 1], np.uint32)
    B = np.array([0, 2 ** 31, 2 ** 32 - 1], np.uint32)
    a, b = np.meshgrid(A, B, indexing="ij")
    u1 = (a.astype(np.float32) + np.float32(1)) * np.float32(2.0 ** -32)
    assert np.all(u1 > 0) and np.all(u1 <= 1)
    z0, z1, r = pr.box_muller(a, b)
    assert np.isfinite(r).all() and np.isfinite(z0).all() and np.isfinite(z1).all()
    assert r.max() <= 6.67 and r.min() >= 0
    assert np.all(r[3] == 0) and np.all(z0[3] == 0) and np.all(z1[3] == 0)          # a = 2^32 - 1: u1 = 1
    assert np.all(r[2] == 0)                                                        # 2^32 - 2 rounds to 2^32 in fp32 as well
    assert r[0, 0] == np.sqrt(-2.0 * np.log(2.0 ** -32))                            # a = 0: the largest radius, 6.66
    assert np.all(z0[:, 0] == r[:, 0]) and np.all(z1[:, 0] == 0)                    # b = 0: angle 0
    assert np.all(z0[:2, 1] < 0) and np.all(np.abs(z0[:, 1] + r[:, 1]) <= 1e-6 * r[:, 1] + 0)   # b = 2^31: angle fl32(pi)
    assert np.all(np.abs(z0 ** 2 + z1 ** 2 - r ** 2) <= 1e-12 * (1 + r ** 2))


def _round_f32_exact(x):
    """The fp32 nearest to the rational x (ties to even), by integer arithmetic."""
    if x == 0:
        return np.float32(0)
    ax = abs(x)                                  # the denominator is a power of two: ax in [2^k, 2^(k+1)), k = the bit lengths' difference
    e = max(ax.numerator.bit_length() - ax.denominator.bit_length() - 23, -149)
    m = round(ax / Fraction(2) ** e)             # Fraction.__round__: half to even; m <= 2^24
    v = np.float32(float(m) * 2.0 ** e)          # exact in float64, exact in fp32
    return -v if x < 0 else v


def _fma_exact(lo, w, u):
    return np.array([_round_f32_exact(Fraction(float(a)) + Fraction(float(b)) * Fraction(float(c)))
                     for a, b, c in zip(np.ravel(lo), np.ravel(w), np.ravel(u))], np.float32)


def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic: random boxes, and sums built to land half way between two fp32 values after the float64
    rounding, where a float64 evaluation followed by a cast goes wrong."""
    rng = np.random.RandomState(2)
    lo = rng.uniform(-20, 20, 20000).astype(np.float32)
    w = rng.uniform(0, 40, 20000).astype(np.float32)
    u = pr.u01(rng.randint(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32))
    got, _ = pr.fma32(lo, w, u)
    assert np.array_equal(got.view(np.uint32), _fma_exact(lo, w, u).view(np.uint32))
    # lo = 2^24 + 2 (ulp 2): w u = 1 +- 2^-46 puts the exact sum next to the tie 2^24 + 3, which the float64 sum rounds ONTO
    lo = np.float32([2 ** 24 + 2, 2 ** 24 + 2, 2 ** 24 + 2, -(2 ** 24 + 2)])
    w = np.float32([1 + 2 ** -23, 1 - 2 ** -24, 1.0, 1 + 2 ** -23])
    u = np.float32([1 - 2 ** -23, 1 - 2 ** -24, 1.0, -(1 - 2 ** -23)])
    got, steps = pr.fma32(lo, w, u)
    want = _fma_exact(lo, w, u)
    assert np.array_equal(got, want) and steps >= 2, (got, want, steps)
    naive = (lo.astype(np.float64) + w.astype(np.float64) * u.astype(np.float64)).astype(np.float32)
    assert not np.array_equal(naive, want)       # the cases do separate one rounding from two


def test_sdf_specs_are_the_dataset_tests_specs():
    import dataclasses

    import test_gpu_dataset
    full = test_gpu_dataset._specs()
    small = pr.sdf_specs(5, 3)
    assert list(full) == pr.SDF_NAMES == list(small)
    for name in full:
        for f in dataclasses.fields(full[name]):
            if f.name in ("n_uniform", "n_near", "_keep"):
                continue
            a, b = getattr(full[name], f.name), getattr(small[name], f.name)
            assert np.array_equal(np.asarray(a, dtype=object if a is None else None), np.asarray(b, dtype=object if b is None else None)), (name, f.name)
        assert (small[name].n_uniform, small[name].n_near) == (5, 3)


@pytest.mark.parametrize("name", pr.SDF_NAMES)
def test_sdf_draws_round_once_on_every_gpu_case(name):
    """Every spec, shape, seed and cfg0 of the GPU test: the values sdf_draws returns are the exactly rounded lo + w u (so the host
    side of the bit-for-bit comparison carries no double rounding), they lie in their boxes, and the configurations past 2^32 are not
    those of the low word alone."""
    for nu, nn in pr.SDF_SHAPES:
        spec = pr.sdf_specs(nu, nn)[name]
        n, pd = spec.n_dof, spec.point_dims
        qlo, qw, plo, pw, olo, ow = pr.sdf_boxes(spec)
        for seed in pr.SDF_SEEDS:
            slo, shi = pr.words64(seed)
            key = np.array([slo, shi], np.uint32)
            for cfg0 in pr.SDF_CFG0:
                q, pu, po = pr.sdf_draws(spec, seed, cfg0, pr.SDF_M)
                assert q.shape == (pr.SDF_M, n) and pu.shape == (pr.SDF_M, nu, pd) and po.shape == (pr.SDF_M, nn, pd)
                assert all(x.dtype == np.float32 for x in (q, pu, po))
                for b in range(pr.SDF_M):              # an independent walk over the documented counters, exact arithmetic
                    clo, chi = (cfg0 + b) & 0xFFFFFFFF, (cfg0 + b) >> 32
                    words = lambda s, j: pr.u01(np.array(_philox_scalar((clo, chi, s, j), key.tolist()), np.uint32))
                    uq = np.array([words(0, t >> 2)[t & 3] for t in range(n)], np.float32)
                    assert np.array_equal(q[b].view(np.uint32), _fma_exact(qlo, qw, uq).view(np.uint32))
                    rows = sorted({0, 1, nu // 2, nu - 1} & set(range(nu))) if nu > 16 else range(nu)
                    for j in rows:
                        assert np.array_equal(pu[b, j].view(np.uint32), _fma_exact(plo, pw, words(1, j)[:pd]).view(np.uint32))
                    rows = sorted({0, 1, nn // 2, nn - 1} & set(range(nn))) if nn > 16 else range(nn)
                    for j in rows:
                        assert np.array_equal(po[b, j].view(np.uint32), _fma_exact(olo, ow, words(2, j)[:pd]).view(np.uint32))
                # all elements: exactly rounded given the vectorised generator's words
                for lo_, w_, got, s, nd in ((plo, pw, pu, 1, nu), (olo, ow, po, 2, nn)):
                    if nd == 0:
                        continue
                    ctr = np.zeros((pr.SDF_M, nd, 4), np.uint32)
                    cl, ch = pr.words64(np.array([cfg0 + b for b in range(pr.SDF_M)], dtype=object))
                    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = cl[:, None], ch[:, None], s, np.arange(nd, dtype=np.uint32)
                    u = pr.u01(pr.philox4x32_10(ctr, key))[..., :pd]
                    want = _fma_exact(np.broadcast_to(lo_, u.shape), np.broadcast_to(w_, u.shape), u).reshape(u.shape)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
                assert np.all(q >= qlo) and np.all(q <= qlo + qw + 1e-6)
                assert np.all(pu >= plo) and np.all(po >= olo - 1e-7)
        if (nu, nn) == (5, 3):
            hi = pr.sdf_draws(spec, pr.SDF_SEEDS[0], 2 ** 32 - 2, pr.SDF_M)
            lo = pr.sdf_draws(spec, pr.SDF_SEEDS[0], 0, 3)
            assert not np.array_equal(hi[0][2:], lo[0])                         # cfg 2^32 .. 2^32 + 2 are not cfg 0 .. 2
            other = pr.sdf_draws(spec, pr.SDF_SEEDS[1], 0, 3)
            assert not np.array_equal(other[0], lo[0])                          # the seed's upper word matters


def test_policy_samples_moments_and_layout():
    N, n, K = 2048, 7, 4
    rng = np.random.RandomState(0)
    means = (rng.standard_normal((K, n)), 1 + rng.rand(K), rng.standard_normal((K, n)))
    scales = (0.5, 0.25, 3.0)
    ps = pr.policy_samples(N, n, K, means, scales, seed=42, rollout_offset=0)
    mc, sc, ac = (np.asarray(m, np.float32).astype(np.float64) for m in means)
    assert np.array_equal(ps.alpha[0], ac) and np.all(ps.bar_alpha[0] == 0)      # the mean rollout; its mu and sigma are noised
    assert np.all(ps.mu[0] != mc) and np.all(ps.sigma[0] != sc)
    z = np.concatenate([((ps.mu - mc) / 0.5).reshape(N, -1), ((ps.sigma - sc) / 0.25).reshape(N, -1),
                        ((ps.alpha - ac) / 3.0).reshape(N, -1)], axis=1)[1:].reshape(-1)
    assert z.size > 100000
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    assert abs(np.mean(z ** 3)) < 0.03 and abs(np.mean(z ** 4) - 3) < 0.08
    zz = np.concatenate([(ps.mu - mc) / 0.5, ((ps.sigma - sc) / 0.25)[..., None], (ps.alpha - ac) / 3.0], axis=2)[1:]
    cc = np.corrcoef(zz.reshape(-1, 2 * n + 1).T)                                # the 15 normals of a (rollout, kernel) are distinct draws
    assert np.abs(cc - np.eye(2 * n + 1)).max() < 0.05
    assert ps.bar_mu.max() < 1e-5 and ps.bar_alpha.max() < 3e-5
    # shards: rows 150 .. of the offset-0 run are the offset-150 run; offset 2^32 - 100 changes the high word at row 100
    sh = pr.policy_samples(300, n, K, means, scales, seed=42, rollout_offset=150)
    assert all(np.array_equal(a[:150], b[150:300]) for a, b in zip(sh[:3], ps[:3]))
    hi = pr.policy_samples(300, 2, 1, (mc[:1, :2], sc[:1], ac[:1, :2]), scales, seed=42, rollout_offset=2 ** 32 - 100)
    lo = pr.policy_samples(300, 2, 1, (mc[:1, :2], sc[:1], ac[:1, :2]), scales, seed=42, rollout_offset=0)
    assert not np.array_equal(hi.alpha[100], ac[:1, :2]) and not np.array_equal(hi.mu[100:], lo.mu[:200])
    up = pr.policy_samples(300, 2, 1, (mc[:1, :2], sc[:1], ac[:1, :2]), scales, seed=42 + 2 ** 32, rollout_offset=0)
    assert not np.array_equal(up.mu, lo.mu)
