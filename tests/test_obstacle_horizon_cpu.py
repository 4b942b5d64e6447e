"""The host definition of constant-velocity obstacle prediction (omds_obstacle_horizon_predict, include/omds.h): no GPU, no context.
out[h][o][c] = fmaf(vel[o][c], (float)h * dt, xyzr[o][c]) for c < 3, radii kept, slab 0 the input itself."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def test_prediction_is_one_product_and_one_fmaf(lib):
    """O = 5, H = 4, dt = 0.5: slab 0 and every radius are the input's bits; every other entry lies within
    2^-23 (|p| + |h dt v|) of the float64 value -- one rounding of h * dt (relative 2^-24 of |h dt v|) plus one of the fmaf (2^-24
    of |result| <= |p| + |h dt v|), doubled."""
    from optimalmodulationds_amd.engine import predict_obstacle_horizon
    rng = np.random.RandomState(5)
    O, H, dt = 5, 4, 0.5
    obs = np.c_[rng.uniform(-1.5, 1.5, (O, 3)), rng.uniform(0.02, 0.3, O)].astype(np.float32)
    vel = rng.uniform(-0.2, 0.2, (O, 3)).astype(np.float32)
    out = predict_obstacle_horizon(obs, vel, H, dt)
    assert out.shape == (H, O, 4) and out.dtype == np.float32
    assert np.array_equal(out[0].view(np.uint32), obs.view(np.uint32))
    for h in range(H):
        assert np.array_equal(out[h, :, 3].view(np.uint32), obs[:, 3].view(np.uint32))
    p, v = obs[:, :3].astype(np.float64), vel.astype(np.float64)
    moved = False
    for h in range(1, H):
        shift = h * float(np.float32(dt)) * v
        bound = 2.0 ** -23 * (np.abs(p) + np.abs(shift))
        err = np.abs(out[h, :, :3].astype(np.float64) - (p + shift))
        print(f"slab {h}: worst error / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (h, float((err / bound).max()))
        moved = moved or bool((out[h, :, :3] != obs[:, :3]).any())
    assert moved


def test_prediction_rejects_null_arguments_and_empty_sizes(lib):
    from optimalmodulationds_amd import _lib as L
    obs = np.zeros((2, 4), np.float32)
    vel = np.zeros((2, 3), np.float32)
    out = np.zeros((3, 2, 4), np.float32)
    f = lib.omds_obstacle_horizon_predict
    assert f(L.fptr(obs), L.fptr(vel), 2, 3, 0.5, L.fptr(out)) == 0
    for args in ((None, L.fptr(vel), 2, 3, 0.5, L.fptr(out)), (L.fptr(obs), None, 2, 3, 0.5, L.fptr(out)),
                 (L.fptr(obs), L.fptr(vel), 2, 3, 0.5, None), (L.fptr(obs), L.fptr(vel), 0, 3, 0.5, L.fptr(out)),
                 (L.fptr(obs), L.fptr(vel), 2, 0, 0.5, L.fptr(out)), (L.fptr(obs), L.fptr(vel), -1, 3, 0.5, L.fptr(out))):
        assert f(*args) == 1, args                    # OMDS_ERR_INVALID_ARG
        assert b"omds_obstacle_horizon_predict" in lib.omds_last_error(None)
