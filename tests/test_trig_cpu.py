"""The encoding's sin / cos on the host: optimalmodulationds_amd/csrc/trig_device.h compiled by g++ (helpers.trig_host) against
oracle/chain_arith.c's copy, float64, the edges and torch.sin / torch.cos (MKL VML: the reference's own sine).  CPU only.

trig_device.h restates SLEEF's 1-ulp xsinf_u1 / xcosf_u1 for |x| < 125 and rounds the double sin / cos above; the kernels
inline it at every feature rebuild, the oracle has its own copy.  The device's bits are held to the digests pinned here by
tests/test_gpu_trig.py."""
import numpy as np
import torch

from helpers import (TRIG_B125, host_cos, host_sin, host_trig_digest, trig_band, trig_edges_in_range, ulp_err)
from oracle import chain

NEG = 0x80000000
# (sin, cos) digests over every float with 0 <= x < 125 (bit patterns [0, bits(125))) and with -125 < x <= -0 ([2^31, 2^31 +
# bits(125))): the sum mod 2^64 of splitmix64(bits(x) << 32 | bits(f(x))).  Computed by this project's host build and oracle; an
# edit of the algorithm (a constant, an operation, the order of one) changes them and must change them here on purpose.
TRIG_DIGEST_POS = (1160618282966584539, 333351564960202835)
TRIG_DIGEST_NEG = (8557348273489436334, 1461957385355272659)


def _f(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _dense():
    """every 997th float with |x| < 125, both signs (2.3e6 values)"""
    x = _f(np.arange(0, TRIG_B125, 997, dtype=np.uint64).astype(np.uint32))
    return np.concatenate([x, -x])


def test_exhaustive_digest_host_build_equals_oracle():
    """Every one of the 2 247 360 512 floats with |x| < 125: the host build of trig_device.h and oracle/chain_arith.c give the
    same bits, and both give the pinned digests."""
    for lo, want in ((0, TRIG_DIGEST_POS), (NEG, TRIG_DIGEST_NEG)):
        assert host_trig_digest(lo, lo + TRIG_B125) == want, f"trig_device.h (host build), range from {lo:#x}"
        assert chain.trig_digest(lo, lo + TRIG_B125) == want, f"oracle/chain_arith.c, range from {lo:#x}"


def test_small_range_arrays_equal_oracle():
    """The array entry points (what the oracle's network and the device tests use) against each other, bit for bit."""
    x = np.concatenate([_dense(), trig_band(), trig_edges_in_range()])
    assert np.array_equal(_bits(host_sin(x)), _bits(chain.sin(x)))
    assert np.array_equal(_bits(host_cos(x)), _bits(chain.cos(x)))


def test_accuracy_against_float64():
    """At most 1 ulp from float64 sin / cos (measured: 0.76 / 0.93 on the dense sample, 0.90 / 0.89 around k pi / 2)."""
    for x in (_dense(), trig_band()):
        x64 = x.astype(np.float64)
        es, ec = ulp_err(host_sin(x), np.sin(x64)), ulp_err(host_cos(x), np.cos(x64))
        assert es.max() <= 1.0, (float(es.max()), float(x[np.argmax(es)]))
        assert ec.max() <= 1.0, (float(ec.max()), float(x[np.argmax(ec)]))


def test_edges():
    b125 = _f(TRIG_B125)
    below, above = _f(TRIG_B125 - 1), _f(TRIG_B125 + 1)
    # signed zeros
    z = np.array([0.0, -0.0], np.float32)
    assert np.array_equal(_bits(host_sin(z)), _bits(z)), "sin(+-0) = +-0"
    assert np.array_equal(host_cos(z), np.ones(2, np.float32)) and not np.signbit(host_cos(z)).any(), "cos(+-0) = +1"
    # subnormals and the smallest normals: sin x = x, cos x = 1 (a translation unit that flushes denormals fails here)
    sub = _f([1, 2, 3, 0x12345, 0x007FFFFF, 0x00800000, 0x00800001])
    sub = np.concatenate([sub, -sub])
    assert np.array_equal(_bits(host_sin(sub)), _bits(sub)), "sin of a subnormal is the subnormal"
    assert (host_cos(sub) == 1.0).all()
    # both sides of the switch to the platform's sinf / cosf at 125, and large finite values: float64 to 1 ulp, oracle's bits
    x = np.array([below, b125, above, 1e4, 1e30, np.finfo(np.float32).max], np.float32)
    x = np.concatenate([x, -x])
    x64 = x.astype(np.float64)
    assert ulp_err(host_sin(x), np.sin(x64)).max() <= 1.0 and ulp_err(host_cos(x), np.cos(x64)).max() <= 1.0
    assert np.array_equal(_bits(host_sin(x)), _bits(chain.sin(x))) and np.array_equal(_bits(host_cos(x)), _bits(chain.cos(x)))
    # non-finite inputs
    nf = np.array([np.inf, -np.inf, np.nan, -np.nan], np.float32)
    for f in (host_sin, host_cos, chain.sin, chain.cos):
        assert np.isnan(f(nf)).all(), f


def _ulp_apart(a, b):
    """distance in representable floats (both finite, same sign or zero)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_against_torch():
    """torch.sin / torch.cos (the reference's sine, MKL VML) and the restatement: never more than 1 ulp apart, identical on at least
    the shares measured (rounded down): uniform [-10, 10] 97.83 / 97.84 %, dense 99.87 / 99.09 %, around k pi / 2 95.70 / 95.99 %.
    If torch's sine changes, this says so first."""
    u = np.random.RandomState(0).uniform(-10, 10, 10 ** 6).astype(np.float32)
    for name, x, floor_s, floor_c in (("uniform [-10, 10]", u, 97.5, 97.5), ("dense", _dense(), 99.8, 99.0),
                                      ("around k pi / 2", trig_band(), 95.5, 95.5)):
        for fn, mine, floor in (("sin", host_sin(x), floor_s), ("cos", host_cos(x), floor_c)):
            ref = getattr(torch, fn)(torch.from_numpy(x)).numpy()
            assert _ulp_apart(mine, ref).max() <= 1, (name, fn)
            same = 100.0 * float(np.mean(mine == ref))
            assert same >= floor, f"{name}: {fn} identical to torch's on {same:.2f} % of the inputs (floor {floor} %)"


def test_fallback_above_125():
    """|x| >= 125 goes to the double-precision sin / cos rounded to float (trig_device.h and the oracle alike): on every 4099th finite
    float above 125, both signs, within 0.5 ulp of float64 (measured 0.499998 / 0.499999: correctly rounded) and the oracle's bits."""
    x = _f(np.arange(TRIG_B125, 0x7F800000, 4099, dtype=np.uint64).astype(np.uint32))
    x = np.concatenate([x, -x])
    x64 = x.astype(np.float64)
    es, ec = ulp_err(host_sin(x), np.sin(x64)), ulp_err(host_cos(x), np.cos(x64))
    assert es.max() <= 0.5 and ec.max() <= 0.5, (float(es.max()), float(ec.max()))
    assert np.array_equal(_bits(host_sin(x)), _bits(chain.sin(x))) and np.array_equal(_bits(host_cos(x)), _bits(chain.cos(x)))
