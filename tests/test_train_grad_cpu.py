"""The checker of tests/test_gpu_train_grad.py, checked without a GPU: the float64 reference against central differences, the
lr = 0 / betas = (0, 0) probe on the numpy restatement of k_adam, four seeded faults that the gradient bar must catch, and the bars
of the Adam step on two honest fp32 evaluations (numpy, torch)."""
import numpy as np
import pytest

import train_reference as R
from oracle import train_oracle as tro

F32 = np.float32


def _case(seed, dims, B, act="relu"):
    rng = np.random.RandomState(seed)
    W, b = R.random_network(rng, dims)
    x = R.relu_safe_rows(W, b, rng, B) if act == "relu" else rng.uniform(-2.0, 2.0, (B, dims[0] // 3)).astype(F32)
    y = rng.uniform(0.0, 3.0, (B, dims[-1])).astype(F32)
    return W, b, x, y


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_reference_gradient_is_the_central_difference_of_the_float64_loss(act):
    import torch
    dims, B = [15, 64, 129, 2], 65
    W, b, x, y = _case(11, dims, B, act)
    ref = R.reference_grads(W, b, x, y, act, torch.float64)
    P = [w.astype(np.float64) for w in W] + [v.astype(np.float64) for v in b]
    nl = len(W)

    def loss_at(params):
        with torch.no_grad():
            Wt = [torch.from_numpy(p) for p in params[:nl]]
            bt = [torch.from_numpy(p) for p in params[nl:]]
            pred = R._forward(Wt, bt, x, act, torch.float64)[0]
            return float(((pred - torch.from_numpy(y.astype(np.float64))) ** 2).mean())

    rng = np.random.RandomState(5)
    h = 1e-6
    for j, (name, g) in enumerate(zip(R.tensor_names(nl), ref["dW"] + ref["db"])):
        scale = float(np.abs(g).max())
        for flat in rng.choice(g.size, size=min(20, g.size), replace=False):
            idx = np.unravel_index(int(flat), g.shape)
            keep = P[j][idx]
            P[j][idx] = keep + h
            up = loss_at(P)
            P[j][idx] = keep - h
            dn = loss_at(P)
            P[j][idx] = keep
            fd = (up - dn) / (2 * h)
            assert abs(fd - g[idx]) <= 1e-6 * scale, (name, idx, fd, float(g[idx]), scale)


def test_probe_step_leaves_the_weights_and_returns_the_gradient():
    """lr = 0, betas = (0, 0), eps = 1e-8 from a zero state: m = g exactly, v = g g, the weights do not move (numpy restatement)."""
    W, b, x, y = _case(12, [15, 64, 129, 2], 65)
    st = tro.TrainState(W, b)
    tro.train_step(st, x, y, lr=0.0, beta1=0.0, beta2=0.0, eps=1e-8)
    for got, was in zip(st.W + st.b, W + b):
        assert np.array_equal(got, was)
    g = _oracle_grads(W, b, x, y)
    for m, v, gi in zip(st.m, st.v, g):
        assert np.array_equal(m, gi) and np.array_equal(v, (gi * gi).astype(F32))
    assert st.t == 1


C3_DIMS, C3_B = [12, 256, 256, 4], 300


def _oracle_grads(W, b, x, y, fault=None):
    """train_oracle.train_step's backward (the same numpy expressions on train_oracle.forward's activations), with one seeded fault."""
    st = tro.TrainState(W, b)
    H = tro.forward(st, x)
    L = len(W)
    G = (F32(2.0 / y.size) * (H[L] - y)).astype(F32)
    gW, gb = [None] * L, [None] * L
    for i in range(L - 1, -1, -1):
        gW[i] = (G.T @ H[i]).astype(F32)
        gb[i] = G.sum(axis=0).astype(F32)
        if i == 1 and fault == "last batch row left out of dW[1]":
            gW[i] = (G[:-1].T @ H[i][:-1]).astype(F32)
        if i == 1 and fault == "one 64-row chunk left out of db[1]":
            gb[i] = (G[:64].sum(axis=0) + G[128:].sum(axis=0)).astype(F32)
        if i == 1 and fault == "columns 128..129 of dW[1] zero":
            gW[i][:, 128:130] = 0
        if i > 0:
            G = (G @ st.W[i]).astype(F32)
            h = H[i + 1] if (i == 1 and fault == "ReLU mask of the wrong layer") else H[i]
            G = (G * (h > 0).astype(F32)).astype(F32)
    return gW + gb


FAULTS = ["last batch row left out of dW[1]", "one 64-row chunk left out of db[1]", "columns 128..129 of dW[1] zero", "ReLU mask of the wrong layer"]


@pytest.fixture(scope="module")
def c3():
    import torch
    W, b, x, y = _case(3, C3_DIMS, C3_B)
    ref64 = R.reference_grads(W, b, x, y, "relu", torch.float64)
    ref32 = R.reference_grads(W, b, x, y, "relu", torch.float32)
    bar = R.DEVICE_FACTOR * R.yardstick(ref32, ref64)[0]
    return W, b, x, y, ref64, bar


def _worst(g, ref64):
    return max(e for e, _ in R.grad_errors(g, ref64["dW"] + ref64["db"]))


def test_the_undamaged_oracle_passes_the_gradient_bar(c3):
    W, b, x, y, ref64, bar = c3
    g = _oracle_grads(W, b, x, y)
    st = tro.TrainState(W, b)
    tro.train_step(st, x, y, lr=0.0, beta1=0.0, beta2=0.0)
    for a, c in zip(g, st.m):                       # the faults below are seeded into the oracle's own gradients
        assert np.array_equal(a, c)
    assert _worst(g, ref64) <= bar, (_worst(g, ref64), bar)


@pytest.mark.parametrize("fault", FAULTS)
def test_a_seeded_fault_exceeds_the_gradient_bar_tenfold(c3, fault):
    W, b, x, y, ref64, bar = c3
    err = _worst(_oracle_grads(W, b, x, y, fault), ref64)
    print(f"{fault}: {err:.2e} against the bar {bar:.2e} ({err / bar:.0f} x)")
    assert err >= 10.0 * bar, (fault, err, bar)


def test_adam_bars_hold_for_numpy_and_torch_fp32_and_catch_a_wrong_step_count():
    """The bars of train_reference.adam_expected on two honest fp32 evaluations of the step, from C3's gradients: the numpy
    restatement of k_adam and torch.optim.Adam itself; and they do not hold for a bias correction one step off."""
    W, b, x, y = _case(3, C3_DIMS, C3_B)
    g = _oracle_grads(W, b, x, y)
    rng = np.random.RandomState(9)
    m0, v0 = R.adam_state(rng, [a.shape for a in g])
    lr, betas, eps = R.adam_hyper()
    st = tro.TrainState(W, b)
    st.m, st.v, st.t = [a.copy() for a in m0], [a.copy() for a in v0], 999
    tro.train_step(st, x, y, lr=F32(lr), beta1=F32(betas[0]), beta2=F32(betas[1]), eps=eps)
    off = 0.0
    for j, (p, gi) in enumerate(zip(W + b, g)):
        exp = R.adam_expected(p, gi, m0[j], v0[j], 1000, lr, betas, eps)
        R.adam_check(f"numpy tensor {j}", (st.W + st.b)[j], st.m[j], st.v[j], exp)
        tp, tm, tv, tstep = R.torch_adam_step(p, gi, m0[j], v0[j], 1000, lr, betas, eps)
        R.adam_check(f"torch tensor {j}", tp, tm, tv, exp)
        assert tstep == 1000.0
        wrong = R.torch_adam_step(p, gi, m0[j], v0[j], 999, lr, betas, eps)[0]
        off = max(off, float((np.abs(wrong - exp["p"]) / exp["bar_p"]).max()))
    assert off >= 10.0, off
