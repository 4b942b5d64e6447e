"""Host restatement of the device's random draws, plain numpy, no GPU: what k_sample (csrc/rollout_kernels.hip) and k_sdf_data
(csrc/dataset_kernels.hip) must produce for given (seed, counters).  Both kernels are pure functions of them, so
tests/test_gpu_random_draws.py compares the device with these functions value by value; tests/test_philox_cpu.py checks the
functions themselves (published known-answer vectors, a scalar plain-int Philox, exact rational arithmetic).

philox4x32_10 is written from the definition in Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC 2011),
section 3.3 / figure 2 of the Philox bijection, not from csrc/philox_device.h:
    one round maps (c0, c1, c2, c3) under the round key (k0, k1) to
        (mulhi(M1, c2) ^ c1 ^ k0,  mullo(M1, c2),  mulhi(M0, c0) ^ c3 ^ k1,  mullo(M0, c0))
    with M0 = 0xD2511F53, M1 = 0xCD9E8D57; the round key starts as the key and is bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85)
    before every round but the first; ten rounds.
The layouts are the documented ones (include/omds.h at omds_sample_policy and omds_sdf_data_generate)."""
from collections import namedtuple

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# (counter, key, output) for 10 rounds: the known-answer vectors published with the paper's reference implementation
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def philox4x32_10(ctr, key, rounds=10):
    """ctr [..., 4], key [..., 2] (broadcast against each other in the leading axes) -> uint32 [..., 4]."""
    ctr, key = np.asarray(ctr, np.uint32), np.asarray(key, np.uint32)
    lead = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], lead).astype(np.uint64) for i in range(4)]
    k = [np.broadcast_to(key[..., i], lead).astype(np.uint64) for i in range(2)]
    m0, m1, mask = np.uint64(M0), np.uint64(M1), np.uint64(MASK32)
    s32 = np.uint64(32)
    for r in range(rounds):
        if r:
            k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
        p0, p1 = m0 * c[0], m1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def words64(v):
    """(low, high) 32-bit words of 64-bit values (Python ints or an integer array), as uint32 arrays."""
    v = np.asarray(v, dtype=object)
    lo = np.asarray(np.frompyfunc(lambda x: int(x) & MASK32, 1, 1)(v)).astype(np.uint32)
    hi = np.asarray(np.frompyfunc(lambda x: (int(x) >> 32) & MASK32, 1, 1)(v)).astype(np.uint32)
    return lo, hi


# ---- the policy sampler ---------------------------------------------------------------------------------------------------------
TWO_PI_F32 = np.float32(6.2831855)
INV32 = np.float32(2.0 ** -32)


def box_muller(a, b):
    """(r cos t, r sin t, r) in float64 for 32-bit words a, b.  The inputs of the transcendentals are formed in fp32, each step rounded
    as on the device: u1 = (float(a) + 1) 2^-32 in (0, 1], u2 = float(b) 2^-32, t = 6.2831855f u2; r = sqrt(-2 ln u1)."""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    u1 = (a.astype(np.float32) + np.float32(1)) * INV32
    u2 = b.astype(np.float32) * INV32
    t = (TWO_PI_F32 * u2).astype(np.float32)
    assert u1.dtype == np.float32 and t.dtype == np.float32
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    t = t.astype(np.float64)
    return r * np.cos(t), r * np.sin(t), r


def normals(seed, g, kernel, count):
    """z, r [..., count]: the first `count` normals of (seed, global rollout g, kernel) and the radius each one came from.  Block c
    = counter (g lo, g hi, kernel, c) gives z[4c .. 4c+3]: cos and sin of words (0, 1), then cos and sin of words (2, 3)."""
    glo, ghi = words64(g)
    kernel = np.asarray(kernel, np.uint32)
    lead = np.broadcast_shapes(glo.shape, kernel.shape)
    nblk = (count + 3) // 4
    ctr = np.zeros(lead + (nblk, 4), np.uint32)
    ctr[..., 0], ctr[..., 1], ctr[..., 2] = glo[..., None], ghi[..., None], np.broadcast_to(kernel, lead)[..., None]
    ctr[..., 3] = np.arange(nblk, dtype=np.uint32)
    slo, shi = words64(int(seed) & (2 ** 64 - 1))
    w = philox4x32_10(ctr, np.array([slo, shi], np.uint32))
    z0, z1, ra = box_muller(w[..., 0], w[..., 1])
    z2, z3, rb = box_muller(w[..., 2], w[..., 3])
    z = np.stack((z0, z1, z2, z3), axis=-1).reshape(lead + (4 * nblk,))
    r = np.stack((ra, ra, rb, rb), axis=-1).reshape(lead + (4 * nblk,))
    return z[..., :count], r[..., :count]


PolicySamples = namedtuple("PolicySamples", "mu sigma alpha bar_mu bar_sigma bar_alpha")
Z_ULPS = 8.0      # the bar on one normal, in units of 2^-24 (r + |z|): twice the ~4 ulp of logf, sqrtf, sincosf and the product


def policy_samples(N, n, K, means, scales, seed, rollout_offset=0):
    """omds_sample_policy restated: float64 mu [N, K, n], sigma [N, K], alpha [N, K, n] and the rounding bar of every element.
    means = (mu_c [K, n], sigma_c [K], alpha_c [K, n]), scales = (mu_s, sigma_s, alpha_s), both taken as the fp32 values the device
    sees.  mu_j = z[j] mu_s + mu_c[j], sigma = z[n] sigma_s + sigma_c, alpha_j = z[n+1+j] alpha_s + alpha_c[j]; the global rollout
    0 (rollout_offset + row == 0), and only it, carries alpha = alpha_c.  Bar of v = z s + c: |s| 8 2^-24 (r + |z|) + 2^-23 |v|."""
    mu_c, sg_c, al_c = (np.asarray(m, np.float32).astype(np.float64) for m in means)
    mu_c, sg_c, al_c = mu_c.reshape(K, n), sg_c.reshape(K), al_c.reshape(K, n)
    mu_s, sg_s, al_s = (float(np.float32(s)) for s in scales)
    g = np.array([int(rollout_offset) + t for t in range(N)], dtype=object)
    z, r = normals(seed, g[:, None], np.arange(K, dtype=np.uint32)[None, :], 2 * n + 1)     # [N, K, 2n+1]

    def scaled(zz, rr, s, c):
        v = zz * s + c
        return v, abs(s) * Z_ULPS * 2.0 ** -24 * (rr + np.abs(zz)) + 2.0 ** -23 * np.abs(v)

    mu, bar_mu = scaled(z[..., :n], r[..., :n], mu_s, mu_c[None])
    sg, bar_sg = scaled(z[..., n], r[..., n], sg_s, sg_c[None])
    al, bar_al = scaled(z[..., n + 1:], r[..., n + 1:], al_s, al_c[None])
    mean_rollout = np.array([int(x) == 0 for x in g])
    al[mean_rollout] = al_c
    bar_al[mean_rollout] = 0.0
    return PolicySamples(mu, sg, al, bar_mu, bar_sg, bar_al)


# ---- the SDF data generator -------------------------------------------------------------------------------------------------------
def fma32(lo, w, u):
    """fl32(lo + w u) for fp32 inputs, rounded ONCE like the device's fused multiply-add.  w u is exact in float64 (24 x 24 bits); the
    float64 sum may not be, and casting it would then round twice.  That matters only when the rounded sum lies exactly half way
    between two fp32 values; there the sign of the sum's exact error (TwoSum) says which side the true value is on, and the sum is
    moved one float64 step to that side before the cast.  Returns (values, number of elements that needed the step)."""
    lo, w, u = (np.asarray(x, np.float32).astype(np.float64) for x in (lo, w, u))
    p = w * u
    s = lo + p
    bb = s - lo
    err = (lo - (s - bb)) + (p - bb)                        # lo + p = s + err exactly
    f = s.astype(np.float32)
    d = s - f.astype(np.float64)                            # exact: f is the fp32 next to s
    other = np.nextafter(f, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    tie = (d != 0) & (np.abs(d) == np.abs(other - s))
    fix = tie & (err != 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32), int(fix.sum())


def u01(r):
    """(r >> 8) 2^-24 in [0, 1): exact in fp32."""
    return ((np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def sdf_boxes(spec):
    """(qlo, qw, plo, pw, olo, ow) in fp32, each operation rounded on its own, as omds_sdf_data_resolve forms them."""
    f = lambda v: np.asarray(v, np.float32).reshape(-1)
    qmin, qmax, pmin, pmax, ns = f(spec.q_min), f(spec.q_max), f(spec.p_min), f(spec.p_max), np.float32(spec.near_scale)
    olo = (ns * pmin).astype(np.float32)
    ow = ((ns * pmax).astype(np.float32) - olo).astype(np.float32)
    return qmin, (qmax - qmin).astype(np.float32), pmin, (pmax - pmin).astype(np.float32), olo, ow


def sdf_draws(spec, seed, cfg0, m, stats=None):
    """The draws of configurations cfg0 .. cfg0 + m - 1: q [m, n], p_uniform [m, n_uniform, pd], near_offsets [m, n_near, pd] in
    fp32, the arguments of dataset.from_draws.  Counter (cfg lo, cfg hi, stream, draw), key (seed lo, seed hi); stream 0 = joints
    (joint t: draw t >> 2, word t & 3), 1 = uniform points (draw = row j, words 0 .. pd-1), 2 = near offsets (draw = near row jn);
    value = lo + w u with u = (word >> 8) 2^-24, one fused multiply-add.  stats (a dict) receives the count of fma32 steps."""
    n, pd, nu, nn = spec.n_dof, spec.point_dims, spec.n_uniform, spec.n_near
    qlo, qw, plo, pw, olo, ow = sdf_boxes(spec)
    clo, chi = words64(np.array([int(cfg0) + b for b in range(m)], dtype=object))
    slo, shi = words64(int(seed) & (2 ** 64 - 1))
    key = np.array([slo, shi], np.uint32)

    def stream(s, ndraw):
        ctr = np.zeros((m, ndraw, 4), np.uint32)
        ctr[..., 0], ctr[..., 1], ctr[..., 2] = clo[:, None], chi[:, None], s
        ctr[..., 3] = np.arange(ndraw, dtype=np.uint32)
        return u01(philox4x32_10(ctr, key))                                   # [m, ndraw, 4]

    steps = 0
    uq = stream(0, (n + 3) // 4).reshape(m, -1)[:, :n]                        # joint t = word t & 3 of draw t >> 2
    q, k = fma32(qlo, qw, uq)
    steps += k
    pu, k = fma32(plo, pw, stream(1, nu)[..., :pd])
    steps += k
    po, k = fma32(olo, ow, stream(2, nn)[..., :pd])
    steps += k
    if stats is not None:
        stats["fma32_steps"] = stats.get("fma32_steps", 0) + steps
    return q, pu, po


# ---- the cases of the data-generator test, shared by the CPU and the GPU half -----------------------------------------------------
SDF_SHAPES = [(300, 341), (5, 3), (7, 0), (0, 7)]      # (n_uniform, n_near): 641 rows = a full 512-row round + a partial one, ...
SDF_SEEDS = [5, 5 + (7 << 32)]
SDF_CFG0 = [0, 2 ** 32 - 2]                            # five configurations from 2^32 - 2 straddle the 32-bit boundary
SDF_M = 5
SDF_NAMES = ["planar7", "planar2", "toy2", "franka"]


def sdf_specs(n_uniform, n_near):
    """The four specs of test_gpu_dataset._specs() with the row counts shrunk through the constructors' keywords."""
    from optimalmodulationds_amd.dataset import SdfDataSpec
    kw = dict(n_uniform=n_uniform, n_near=n_near)
    return {"planar7": SdfDataSpec.gen_dataset_planar(7, **kw), "planar2": SdfDataSpec.gen_dataset_planar(2, link_len=3.0, **kw),
            "toy2": SdfDataSpec.gen_dataset_2dtoy(**kw), "franka": SdfDataSpec.franka(**kw)}
