"""The encoding's sin / cos on the device (run on a real MI355X: ``pytest -m gpu``): csrc/trig_device.h as the kernels inline it,
through the test hooks omds_test_trig / omds_test_trig_sweep (include/omds_test.h), against the digests and the host build of
tests/test_trig_cpu.py; and the product's feature kernels (raw forward / vjp, Jacobian, trainer, wide networks) through an identity
network whose outputs are the encoded features themselves.  Bit parity with the host and the oracle is by construction for |x| < 125;
above, the double-precision sin / cos rounded to float (ocml on the device, libm on the host) are compared to each other and to
float64."""
import ctypes as C

import numpy as np
import pytest

from helpers import TRIG_B125, host_cos, host_sin, host_trig_digest, trig_band, trig_edges_in_range, ulp_err
from oracle import chain
from test_trig_cpu import TRIG_DIGEST_NEG, TRIG_DIGEST_POS

pytestmark = pytest.mark.gpu
NEG = 0x80000000


@pytest.fixture(scope="module")
def lib():
    from optimalmodulationds_amd import _lib
    return _lib.load_test_hooks()


def _dev(lib, x):
    x = np.ascontiguousarray(x, np.float32)
    s, c = np.empty_like(x), np.empty_like(x)
    assert lib.omds_test_trig(x.ctypes.data, s.ctypes.data, c.ctypes.data, x.size) == 0
    return s, c


def _dev_digest(lib, lo, hi):
    out = (C.c_uint64 * 2)()
    assert lib.omds_test_trig_sweep(int(lo), int(hi), out) == 0
    return int(out[0]), int(out[1])


def _f(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _first_difference(lib, lo, hi):
    """Bisects [lo, hi) by device vs host digests down to 2^16 bit patterns, then compares those in array mode: the first input whose
    device bits differ from the host build's, as text (None if the digests agree everywhere)."""
    while hi - lo > 1 << 16:
        step = (hi - lo + 15) // 16
        for a in range(lo, hi, step):
            b = min(hi, a + step)
            if _dev_digest(lib, a, b) != host_trig_digest(a, b):
                lo, hi = a, b
                break
        else:
            return None
    x = _f(np.arange(lo, hi, dtype=np.uint64).astype(np.uint32))
    s, c = _dev(lib, x)
    hs, hc = host_sin(x), host_cos(x)
    bad = np.nonzero((_bits(s) != _bits(hs)) | (_bits(c) != _bits(hc)))[0]
    if not bad.size:
        return None
    i = int(bad[0])
    return (f"x = {x[i]!r} ({int(_bits(x[i])):#010x}): device sin {s[i]!r} cos {c[i]!r}, host sin {hs[i]!r} cos {hc[i]!r} "
            f"({bad.size} of {x.size} inputs in [{lo:#x}, {hi:#x}) differ)")


def test_sweep_every_float_below_125(lib):
    """Every float with |x| < 125 on the device: the digests pinned in tests/test_trig_cpu.py (= the host build's and the oracle's)."""
    for lo, want in ((0, TRIG_DIGEST_POS), (NEG, TRIG_DIGEST_NEG)):
        got = _dev_digest(lib, lo, lo + TRIG_B125)
        if got != want:
            pytest.fail(f"device digests {got} != pinned {want} on [{lo:#x}, {lo + TRIG_B125:#x}); first difference: "
                        f"{_first_difference(lib, lo, lo + TRIG_B125)}")


def test_edges_and_quadrant_boundaries(lib):
    """±0, subnormals, the last float below 125 and ±1..±2000 ulps around every k pi / 2 (k <= 79): the host build's bits.
    ±inf and NaN: NaN."""
    x = np.concatenate([trig_edges_in_range(), trig_band()])
    s, c = _dev(lib, x)
    for name, dev, host in (("sin", s, host_sin(x)), ("cos", c, host_cos(x))):
        bad = np.nonzero(_bits(dev) != _bits(host))[0]
        assert bad.size == 0, (f"{name}: {bad.size} of {x.size} inputs are not the host build's bits, first x = {x[bad[0]]!r}: "
                               f"device {dev[bad[0]]!r}, host {host[bad[0]]!r}")
    z = np.array([0.0, -0.0], np.float32)
    s, c = _dev(lib, z)
    assert np.array_equal(_bits(s), _bits(z)) and np.array_equal(_bits(c), _bits(np.ones(2, np.float32)))
    s, c = _dev(lib, np.array([np.inf, -np.inf, np.nan, -np.nan], np.float32))
    assert np.isnan(s).all() and np.isnan(c).all()


def test_fallback_above_125(lib):
    """|x| >= 125 (the double sin / cos rounded to float, ocml on the device, libm in the oracle): on every 4099th finite float above
    125, both signs, and the edges 125, 1e4, 1e30, FLT_MAX: the oracle's bits and within 0.5 ulp of float64.  (Before the fallback
    was written this way it was the hardware's v_sin_f32 / v_cos_f32: 0.02 % of these inputs had the oracle's bits, some were 2 off.)"""
    x = _f(np.arange(TRIG_B125, 0x7F800000, 4099, dtype=np.uint64).astype(np.uint32))
    x = np.concatenate([x, -x, np.array([125.0, -125.0, 1e4, 1e30, np.finfo(np.float32).max], np.float32)])
    s, c = _dev(lib, x)
    x64 = x.astype(np.float64)
    es, ec = ulp_err(s, np.sin(x64)), ulp_err(c, np.cos(x64))
    same_s, same_c = _bits(s) == _bits(chain.sin(x)), _bits(c) == _bits(chain.cos(x))
    print(f"fallback |x| >= 125, {x.size} inputs: device vs float64 {es.max():.7f} / {ec.max():.7f} ulp (sin / cos); "
          f"identical to the oracle {100 * same_s.mean():.4f} % / {100 * same_c.mean():.4f} %")
    assert same_s.all() and same_c.all(), f"first input where the device is not the oracle's bits: {x[~(same_s & same_c)][0]!r}"
    assert es.max() <= 0.5 and ec.max() <= 0.5, (float(es.max()), float(ec.max()))


# ---- the product's feature kernels produce the hook's bits --------------------------------------------------------------------
# Identity network on planar-2 shapes: 5 inputs -> 15 features [x, sin x, cos x] -> W1 = [I; -I], ReLU -> W2 = [I, -I], zero biases:
# output j = relu(f_j) - relu(-f_j) = f_j exactly (one term is zero), out_div = 1.  -0 comes back as +0; no inf / NaN here (inf * 0
# poisons every unit) and no subnormals (they go through the GEMMs, not through the encoding's sin / cos).
D, F = 5, 15


def _identity_net(hidden=2 * F):
    W1 = np.zeros((hidden, F), np.float32)
    W2 = np.zeros((F, hidden), np.float32)
    W1[np.arange(F), np.arange(F)] = 1.0
    W1[F + np.arange(F), np.arange(F)] = -1.0
    W2[np.arange(F), np.arange(F)] = 1.0
    W2[np.arange(F), F + np.arange(F)] = -1.0
    return [W1, W2], [np.zeros(hidden, np.float32), np.zeros(F, np.float32)]


def _rows():
    """inputs as [B, 5] rows: around every k pi / 2 (±200 ulps), uniform [-10, 10], normal edges (no subnormals), both signs"""
    e = trig_edges_in_range()
    e = e[(e == 0) | (np.abs(e) >= np.finfo(np.float32).tiny)]
    x = np.concatenate([trig_band(width=200), np.random.RandomState(5).uniform(-10, 10, 5000).astype(np.float32), e])
    x = np.concatenate([x, np.zeros(-x.size % D, np.float32)])
    return x.reshape(-1, D)


def _features(lib, x):
    s, c = _dev(lib, x)
    return np.concatenate([x, s, c], axis=1) + np.float32(0)     # + 0: -0 -> +0


def _assert_features(y, want, what):
    y = y + np.float32(0)
    bad = _bits(y) != _bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} features are not the hook's bits, first at column {np.argwhere(bad)[0]}"


ROWS = 1024   # the engine's batch of raw rows: n_traj * n_closest


def _engine(W, b):
    from optimalmodulationds_amd.engine import Engine
    eng = Engine(2, ROWS, 1, 1, max_obs=8)
    eng.set_mlp(W, b, act="relu", out_div=1.0)
    return eng


def _batched(fn, x):
    """fn over ROWS rows at a time, outputs concatenated"""
    outs = [fn(x[r:r + ROWS]) for r in range(0, x.shape[0], ROWS)]
    return [np.concatenate(o) for o in zip(*outs)]


@pytest.mark.parametrize("hidden", [2 * F, 384])
def test_forward_vjp_features(lib, hidden):
    """omds_mlp_forward_vjp: the fused feature kernels + pass 2 (hidden 30) and k_wide_encode_raw + the GEMMs (hidden 384)."""
    x = _rows()
    eng = _engine(*_identity_net(hidden))
    y, _, _ = _batched(eng.mlp_forward_vjp, x)
    eng.close()
    _assert_features(y, _features(lib, x), f"mlp_forward_vjp, hidden {hidden}")


def test_jacobian_sin_cos_columns(lib):
    """omds_mlp_jacobian through the encoding's backward (pe_chain_rule, pass2_device.h): d sin x_j / d x_j = cos x_j and d cos x_j / d x_j = -sin x_j,
    the hook's bits (x = ±0 left out: sin 0 = 0 switches both ReLU units of that feature off)."""
    x = _rows()
    eng = _engine(*_identity_net())
    y, J = _batched(lambda xb: eng.mlp_jacobian(xb, list(range(F))), x)
    eng.close()
    _assert_features(y, _features(lib, x), "mlp_jacobian outputs")
    s, c = _dev(lib, x)
    j = np.arange(D)
    nz = x != 0
    assert np.array_equal(_bits(J[:, j, D + j][nz]), _bits(c[nz])), "d sin / dx is not the hook's cos"
    assert np.array_equal(_bits(J[:, j, 2 * D + j][nz] + np.float32(0)), _bits((-s[nz]) + np.float32(0))), "d cos / dx is not -(the hook's sin)"
    assert (J[:, j, j][nz] == 1).all()


def test_trainer_eval_features(lib):
    """SdfTrainer.eval(want_pred=True): k_encode + the trainer's GEMMs."""
    from optimalmodulationds_amd.trainer import SdfTrainer
    x = _rows()
    W, b = _identity_net()
    tr = SdfTrainer([F, 2 * F, F], "relu")
    tr.set_weights(W, b)
    tr.set_data(x, np.zeros((x.shape[0], F), np.float32))
    _, pred = tr.eval(want_pred=True)
    tr.close()
    _assert_features(pred, _features(lib, x), "trainer eval")
