"""GPU tests of the trainer's gradients and Adam step (csrc/train.hip), tensor by tensor against float64.

A gradient is read without a hook: from a zero optimizer state, ``step(lr=0, betas=(0, 0), eps=1e-8)`` makes k_adam compute
m = 0 + (g - 0) * 1 = g and v = g g and leaves p - 0 * (m / denom) = p, so ``optimizer_state_dict()["state"][i]["exp_avg"]`` is the
gradient bit for bit (include/omds.h at omds_trainer_step).  Both facts are asserted as preconditions of every probe.

The reference is tests/train_reference.py: torch-CPU autograd at float64 on the same fp32 inputs.  ReLU cases take inputs on which
no unit sits within 1e-4 of its kink in float64 (relu_safe_rows), so the fp32 and the float64 masks are the same; every element of
every gradient on those inputs is compared.  The bar on max |dev - ref64| / max |ref64| per tensor is 8 x the error of torch-CPU
float32 autograd on the same inputs (the maximum over the case's tensors, floored at 2^-22): the device sums fmaf chains of
B / splits rows and then up to 256 partials one after the other where torch sums in blocks -- another constant in front of
eps sqrt(n), the same order.  The yardstick is 2.4e-7 (its floor) to 9e-7 on the random networks, 3.4e-6 at 49 153 rows on one host, 6.6e-5 on the trained franka weights (activations up to 350); the
device has been seen at 2.1 x the yardstick at most (EXPERIMENTS.md R13).  One dropped row of 3001 is 3e-4, of 49 153 2e-5; the
faults seeded in tests/test_train_grad_cpu.py exceed the bar 3 800-fold and more.

Routes: which kernel multiplies a layer's forward, weight gradient and input gradient, and how the batch is split, is stated in
optimalmodulationds_amd/csrc/train_plan_def.h and nowhere else.  The cases below name what each reaches;
tests/test_train_plan_cpu.py holds every case to the routes it names and pins the split numbers.  Every case is also run with every product on k_gemm (the test library's
omds_debug_trainer_general_gemm) and must give the same bits: the bit-for-bit claim of tests/test_gpu_train.py at every shape here."""
import functools

import numpy as np
import pytest

import train_reference as R
from helpers import RTOL, weights_path
from oracle import omds_oracle as orc

pytestmark = pytest.mark.gpu

SHIPPED = [30, 256, 256, 256, 256, 9]
# (id, dims, act, B, weights)
CASES = (
    # C1: the shipped shape -- thin forward (30 -> 256), three tall layers each way, thin-out (256 -> 9), k_wgrad_thin<32> (T = 30) and <12>
    # (T = 9), thin input gradient (K = 9); B = 1: one split, half the units dead; B = 65: two chunks of 48 and 17 rows; B = 257: rsplit 1;
    # B = 3001: 47 chunks of 64 rows, rsplit 11
    [(f"C1-{act}-B{B}", SHIPPED, act, B, "random") for act in ("relu", "tanh") for B in (1, 63, 65, 257, 3001)]
    + [
        # C2: k_wgrad_thin<16> (T = 15) and <4> (T = 2), thin-out with N = 2, thin input gradient with K = 2
        ("C2-planar2", [15, 256, 256, 256, 256, 2], "relu", 257, "planar2"),
        # C3: k_wgrad_thin<12> in its first-layer form (T = 12), <4> with T = 4
        ("C3", [12, 256, 256, 4], "relu", 300, "random"),
        # C4: k_gemm_tall forward (256 -> N) and input gradient (N <- 256) with N < 256: N = 200 keeps 16-byte stores up to the edge
        # kq + 3 < N, N = 131 / 129 have ldc % 4 != 0 (scalar stores); K = 200 / 131 / 129 on k_gemm (N -> 256 forward, 256 -> N backward)
        ("C4-200", [30, 256, 200, 256, 9], "relu", 257, "random"),
        ("C4-131", [30, 256, 131, 256, 9], "relu", 257, "random"),
        ("C4-129", [30, 256, 129, 256, 9], "relu", 257, "random"),
        # C5: a hidden bottleneck: thin forward 20 -> 256, thin input gradient 256 <- 20, k_wgrad_thin<32> (T = 20) in both forms
        ("C5", [30, 256, 20, 256, 9], "tanh", 193, "random"),
        # C6: 769 row tiles on 256 CUs: a persistent k_gemm_tall workgroup runs 3 to 4 tiles, both LDS buffers turn from parked
        # output to next input; 237 chunks of 208 rows (the last one 65), rsplit 192
        ("C6", SHIPPED, "relu", 3 * 64 * 256 + 1, "random"),
        # C7: in = 33 > THIN_KMAX and out = 17 > THINN_NMAX on k_gemm; k_wgrad_thin<32> with T = 17; thin input gradient K = 17, N = 200
        ("C7", [33, 130, 200, 17], "relu", 257, "random"),
        # C8: thin forward at its lower edge N = 64; N = 63 on k_gemm; thin-out N = 16 with K = 63 (no float4 path); k_wgrad_thin<16>
        # with T = 16; width 300: three column tiles of k_gemm, 2 x 3 and (300 -> 257) 3 x 3 weight-gradient tiles, two wide blocks of
        # k_wgrad_thin
        ("C8-64-63-16", [30, 64, 63, 16], "relu", 129, "random"),
        ("C8-300-129", [30, 300, 129, 9], "relu", 129, "random"),
        ("C8-300-257", [30, 300, 257, 9], "relu", 129, "random"),
        # C9: trained weights with dead units, y = net(x) + 5 randn as in tests/test_gpu_train.py
        ("C9-franka", SHIPPED, "relu", 3001, "franka"),
    ]
)
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    """Weights, inputs and the two CPU evaluations of a case: computed once, shared by its tests, never written to."""
    import torch
    _, dims, act, B, kind = CASES[IDS.index(cid)]
    rng = np.random.RandomState(1000 + IDS.index(cid))
    if kind == "random":
        W, b = R.random_network(rng, dims)
    else:
        m = orc.Mlp.from_npz(weights_path(kind))
        W, b = [np.array(w, np.float32) for w in m.W], [np.array(v, np.float32) for v in m.b]
        assert [W[0].shape[1]] + [w.shape[0] for w in W] == dims
    x = R.relu_safe_rows(W, b, rng, B) if act == "relu" else rng.uniform(-2.0, 2.0, (B, dims[0] // 3)).astype(np.float32)
    if kind == "franka":
        y = (orc.mlp_forward(m, x) + 5.0 * rng.standard_normal((B, dims[-1]))).astype(np.float32)
    else:
        y = rng.uniform(0.0, 3.0, (B, dims[-1])).astype(np.float32)
    ref64 = R.reference_grads(W, b, x, y, act, torch.float64)
    if act == "relu":
        assert ref64["margin"].min() >= R.MARGIN
    ref32 = R.reference_grads(W, b, x, y, act, torch.float32)
    for a in W + b + [x, y]:
        a.setflags(write=False)
    return dict(dims=dims, act=act, B=B, W=W, b=b, x=x, y=y, ref64=ref64, yard=R.yardstick(ref32, ref64))


def _probe(tr, W, b):
    """The gradient of the trainer's data set at (W, b), read through the optimizer state; asserts the probe's two preconditions."""
    tr.set_weights(W, b)                                 # also a zero optimizer state, step 0
    loss = tr.step(lr=0.0, betas=(0.0, 0.0), eps=1e-8)
    W1, b1 = tr.get_weights()
    for got, was in zip(W1 + b1, list(W) + list(b)):
        assert np.array_equal(got, was), "the probe step moved a weight"
    st = tr.optimizer_state_dict()["state"]
    nl = len(W)
    g = [st[2 * i]["exp_avg"].numpy().copy() for i in range(nl)] + [st[2 * i + 1]["exp_avg"].numpy().copy() for i in range(nl)]
    v = [st[2 * i]["exp_avg_sq"].numpy() for i in range(nl)] + [st[2 * i + 1]["exp_avg_sq"].numpy() for i in range(nl)]
    for gi, vi in zip(g, v):
        assert np.array_equal(vi, (gi * gi).astype(np.float32)), "exp_avg_sq is not exp_avg squared: exp_avg is not the gradient"
    assert float(st[0]["step"]) == 1.0
    return loss, g


@functools.lru_cache(maxsize=None)
def _device(cid):
    """The product library's forward, loss and two probes of a case."""
    from optimalmodulationds_amd.trainer import SdfTrainer
    c = _inputs(cid)
    tr = SdfTrainer(c["dims"], c["act"])
    try:
        tr.set_weights(c["W"], c["b"])
        tr.set_data(c["x"], c["y"])
        _, pred = tr.eval(want_pred=True)
        loss, g = _probe(tr, c["W"], c["b"])
        loss2, g2 = _probe(tr, c["W"], c["b"])
    finally:
        tr.close()
    return dict(pred=pred, loss=loss, g=g, loss2=loss2, g2=g2)


@pytest.mark.parametrize("cid", IDS)
def test_gradients_against_float64(cid):
    c, dev = _inputs(cid), _device(cid)
    ref, (yard, yard_per) = c["ref64"], c["yard"]
    nl = len(c["W"])
    names = R.tensor_names(nl)
    # 1. forward, 2. loss
    pscale = float(np.abs(ref["pred"]).max())
    perr = float(np.abs(dev["pred"] - ref["pred"]).max()) / pscale
    lerr = abs(dev["loss"] - ref["loss"]) / ref["loss"]
    print(f"{cid}: forward {perr:.2e}, loss {lerr:.2e} (bar {RTOL:.0e}); gradient yardstick {yard:.2e}, bar {R.DEVICE_FACTOR * yard:.2e}")
    assert perr <= RTOL, (cid, perr)
    assert lerr <= RTOL, (cid, dev["loss"], ref["loss"])
    # 3. every gradient, every element
    errs = R.grad_errors(dev["g"], ref["dW"] + ref["db"])
    for name, (e, at), y32 in zip(names, errs, yard_per):
        print(f"  {name:6s} device {e:.2e}  torch-fp32 {y32:.2e}  device / yardstick {e / yard:.2f}")
    for name, (e, at) in zip(names, errs):
        assert e <= R.DEVICE_FACTOR * yard, f"{cid} {name}: {e:.3e} of max |ref| off float64 at {at}; the bar is 8 x {yard:.3e}"
    # 4. a unit that is off on every row has an exactly zero row of dW and entry of db
    if c["act"] == "relu":
        ndead = 0
        for i, dead in enumerate(ref["dead"]):
            ndead += int(dead.sum())
            assert not np.any(dev["g"][i][dead]) and not np.any(dev["g"][nl + i][dead]), f"{cid}: a dead unit of layer {i} has a gradient"
        print(f"  dead units: {ndead}")
    # 6. a second probe from the same state
    assert dev["loss2"] == dev["loss"]
    for name, a, a2 in zip(names, dev["g"], dev["g2"]):
        assert np.array_equal(a, a2), f"{cid} {name}: two probes from the same state differ"


@pytest.mark.parametrize("cid", IDS)
def test_every_route_gives_the_general_kernels_bits(cid):
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.trainer import SdfTrainer
    c, dev = _inputs(cid), _device(cid)
    lib = L.load_test_hooks()
    assert lib.omds_debug_trainer_general_gemm(1) == 0
    try:
        tr = SdfTrainer(c["dims"], c["act"], lib=lib)
        try:
            tr.set_weights(c["W"], c["b"])
            tr.set_data(c["x"], c["y"])
            _, pred = tr.eval(want_pred=True)
            loss, g = _probe(tr, c["W"], c["b"])
        finally:
            tr.close()
    finally:
        lib.omds_debug_trainer_general_gemm(0)
    assert np.array_equal(pred, dev["pred"]), f"{cid}: predictions differ from k_gemm's"
    assert loss == dev["loss"], (cid, loss, dev["loss"])
    for name, a, a2 in zip(R.tensor_names(len(c["W"])), g, dev["g"]):
        assert np.array_equal(a, a2), f"{cid} {name}: differs from k_gemm's bits at {np.argwhere(a != a2)[:4].tolist()}"


@pytest.mark.parametrize("cid", ["C3", "C1-relu-B257"])
def test_adam_step_against_float64_and_torch(cid):
    """k_adam, the bias corrections and the step count: one step (lr 2e-4, betas (0.9, 0.999), eps 1e-8) from a loaded state at step
    999 -- exp_avg in +-1e-2, exp_avg_sq over 1e-18 .. 1e-2 -- against the formulas above k_adam in float64 at t = 1000 on the
    device's own gradient, and against torch.optim.Adam (CPU, fp32) fed the same gradient and state.  Bars: train_reference.adam_expected.
    torch's own m, v and p are held to the same bars against float64; between the device and torch the bar of p carries a whole
    ulp(p) instead of half of one, since both sides round their final subtraction.
    The hyperparameters are the float32 values the C ABI carries, in the float64 formulas and in the torch run alike."""
    import torch
    from optimalmodulationds_amd.trainer import SdfTrainer
    c, dev = _inputs(cid), _device(cid)
    nl = len(c["W"])
    g = dev["g"]
    m0, v0 = R.adam_state(np.random.RandomState(9), [a.shape for a in g])
    lr, betas, eps = R.adam_hyper(2e-4, (0.9, 0.999), 1e-8)
    order = [k for i in range(nl) for k in (i, nl + i)]        # state_dict order: weight 0, bias 0, weight 1, ...
    tr = SdfTrainer(c["dims"], c["act"])
    try:
        tr.set_weights(c["W"], c["b"])
        tr.set_data(c["x"], c["y"])
        tr.load_optimizer_state_dict({"state": {j: {"step": torch.tensor(999.0), "exp_avg": m0[k], "exp_avg_sq": v0[k]} for j, k in enumerate(order)}})
        tr.step(lr=lr, betas=betas, eps=eps)
        W1, b1 = tr.get_weights()
        st = tr.optimizer_state_dict()["state"]
    finally:
        tr.close()
    p0, p1 = list(c["W"]) + list(c["b"]), W1 + b1
    worst = dict(m=0.0, v=0.0, p=0.0, tm=0.0, tv=0.0, tp=0.0)
    for j, k in enumerate(order):
        assert float(st[j]["step"]) == 1000.0
        dm, dv = st[j]["exp_avg"].numpy(), st[j]["exp_avg_sq"].numpy()
        exp = R.adam_expected(p0[k], g[k], m0[k], v0[k], 1000, lr, betas, eps)
        for key, val in R.adam_check(f"{cid} {R.tensor_names(nl)[k]}", p1[k], dm, dv, exp).items():
            worst[key] = max(worst[key], val)
        tp, tm, tv, tstep = R.torch_adam_step(p0[k], g[k], m0[k], v0[k], 1000, lr, betas, eps)
        assert tstep == 1000.0
        R.adam_check(f"{cid} {R.tensor_names(nl)[k]} (torch)", tp, tm, tv, exp)
        for key, a, t_ in (("m", dm, tm), ("v", dv, tv), ("p", p1[k], tp)):
            r = float((np.abs(a.astype(np.float64) - t_.astype(np.float64)) / exp["bar_p_pair" if key == "p" else "bar_" + key]).max())
            worst["t" + key] = max(worst["t" + key], r)
            assert r <= 1.0, f"{cid} {R.tensor_names(nl)[k]}: {key} is {r:.2f} x its bar from torch.optim.Adam's"
    print(f"{cid}: worst error / bar against float64 m {worst['m']:.2f} v {worst['v']:.2f} p {worst['p']:.2f}; "
          f"against torch m {worst['tm']:.2f} v {worst['tv']:.2f} p {worst['tp']:.2f}")
