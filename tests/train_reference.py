"""The float64 reference of one training step's gradients (csrc/train.hip: forward through [x, sin x, cos x] -> Linear + act ... ->
Linear, F.mse_loss(reduction='mean'), backward), for tests/test_train_grad_cpu.py and tests/test_gpu_train_grad.py.  Plain torch
autograd on the CPU at the dtype asked for: float64 is the reference, float32 the yardstick an honest fp32 evaluation is held to.
Nothing of the trainer's blocking, splitting or summation order is restated here."""
import numpy as np

MARGIN = 1e-4                 # smallest |pre-activation| a ReLU row may have: far above any fp32 forward's error (1e-6 of O(1) values)
YARDSTICK_FLOOR = 2.0 ** -22  # so that one lucky fp32 tensor cannot make the bar unreachable
DEVICE_FACTOR = 8.0           # the device may be this many times the torch-fp32 yardstick (another summation order, the same order of error)


def _forward(Wt, bt, x, act, dtype):
    import torch
    import torch.nn.functional as F
    xt = torch.tensor(np.asarray(x, np.float32), dtype=dtype)
    h = torch.cat((xt, torch.sin(xt), torch.cos(xt)), dim=1)
    margin = torch.full((xt.shape[0],), float("inf"), dtype=dtype)
    dead = []
    for i in range(len(Wt)):
        h = F.linear(h, Wt[i], bt[i])
        if i + 1 < len(Wt):
            with torch.no_grad():
                margin = torch.minimum(margin, h.abs().min(dim=1).values)
                dead.append((h <= 0).all(dim=0).numpy())
            h = torch.relu(h) if act == "relu" else torch.tanh(h)
    return h, margin.numpy().astype(np.float64), dead


def reference_grads(W, b, x, y, act, dtype):
    """Loss, predictions, every dW / db, and per row the smallest |pre-activation| over all hidden units (the row's margin), of the
    network (W, b) on the fp32 inputs x [B, d] and targets y [B, C], evaluated by torch on the CPU at ``dtype``.  ``dead[i]`` marks
    the units of hidden layer i whose pre-activation is <= 0 on every row."""
    import torch
    import torch.nn.functional as F
    Wt = [torch.tensor(np.asarray(w, np.float32), dtype=dtype, requires_grad=True) for w in W]
    bt = [torch.tensor(np.asarray(v, np.float32), dtype=dtype, requires_grad=True) for v in b]
    h, margin, dead = _forward(Wt, bt, x, act, dtype)
    loss = F.mse_loss(h, torch.tensor(np.asarray(y, np.float32), dtype=dtype), reduction="mean")
    loss.backward()
    return dict(loss=float(loss.item()), pred=h.detach().numpy(), dW=[w.grad.numpy() for w in Wt], db=[v.grad.numpy() for v in bt],
                margin=margin, dead=dead)


def row_margins(W, b, x, act="relu"):
    """The float64 margin of every row of x (the forward pass of reference_grads alone)."""
    import torch
    with torch.no_grad():
        Wt = [torch.tensor(np.asarray(w, np.float32), dtype=torch.float64) for w in W]
        bt = [torch.tensor(np.asarray(v, np.float32), dtype=torch.float64) for v in b]
        return _forward(Wt, bt, x, act, torch.float64)[1]


def relu_safe_rows(W, b, rng, B, margin=MARGIN):
    """B input rows, uniform(-2, 2), on which no ReLU of the network sits within ``margin`` of its kink in float64 -- no unit's mask can
    then differ between an fp32 and a float64 forward, and the two gradients are gradients of the same smooth piece.  ceil(1.5 B) rows
    are drawn and the first B safe ones kept; at most 25 % of the drawn rows may be unsafe.  The filter chooses inputs; every element
    of every gradient on those inputs is still compared."""
    d = np.asarray(W[0]).shape[1] // 3
    n = int(np.ceil(1.5 * B))
    x = rng.uniform(-2.0, 2.0, (n, d)).astype(np.float32)
    safe = row_margins(W, b, x) >= margin
    dropped = 1.0 - float(safe.mean())
    assert dropped <= 0.25, f"{100 * dropped:.1f} % of the drawn rows are within {margin:g} of a ReLU kink"
    keep = np.flatnonzero(safe)[:B]
    assert keep.size == B, (keep.size, B)
    return x[keep]


def random_network(rng, dims):
    """W = uniform(-1, 1) * 1.7 / sqrt(fan_in), b = uniform(-1, 1) / sqrt(fan_in)."""
    W = [(rng.uniform(-1.0, 1.0, (dims[i + 1], dims[i])) * 1.7 / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    b = [(rng.uniform(-1.0, 1.0, dims[i + 1]) / np.sqrt(dims[i])).astype(np.float32) for i in range(len(dims) - 1)]
    return W, b


def grad_errors(got, ref64):
    """Per tensor: (max |got - ref| / max |ref|, index of the worst element).  A reference that is zero everywhere admits only zeros."""
    out = []
    for g, r in zip(got, ref64):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape, (g.shape, r.shape)
        assert np.isfinite(g).all(), "non-finite gradient"
        d = np.abs(g - r)
        worst = np.unravel_index(int(d.argmax()), d.shape)
        scale = float(np.abs(r).max())
        out.append(((float(d.max()) / scale) if scale > 0 else (0.0 if d.max() == 0 else float("inf")), tuple(int(v) for v in worst)))
    return out


def yardstick(ref32, ref64):
    """The error of torch-CPU float32 autograd against float64 on the same inputs: the maximum over the case's tensors, floored."""
    per = [e for e, _ in grad_errors(ref32["dW"] + ref32["db"], ref64["dW"] + ref64["db"])]
    return max(max(per), YARDSTICK_FLOOR), per


def tensor_names(L):
    return [f"dW[{i}]" for i in range(L)] + [f"db[{i}]" for i in range(L)]


# ---- one Adam step (k_adam of csrc/train.hip, torch.optim.Adam's single-tensor arithmetic) in float64 -------------------------------
def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def adam_hyper(lr=2e-4, betas=(0.9, 0.999), eps=1e-8):
    """The hyperparameters as the C ABI passes them: rounded to float32, returned as Python floats.  The kernel forms 1 - beta from the
    rounded value (1 - 0.999f is 1.3e-5 below 0.001), so the float64 formulas and the torch run take the same rounded numbers."""
    f = lambda v: float(np.float32(v))
    return f(lr), (f(betas[0]), f(betas[1])), f(eps)


def adam_expected(p, g, m, v, t, lr, betas, eps):
    """m, v and p after step t, in float64, from the formulas above k_adam:
        m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g g;  denom = sqrt(v') / sqrt(1 - b2^t) + eps;  p' = p - lr / (1 - b1^t) * m' / denom
    and the bars an fp32 evaluation is held to, each a count of the roundings in the kernel's expression (0.5 ulp of the value rounded):
      m'  m + (g - m) (1 - b1): three roundings, of g - m, of its product and of the sum: 4 ulp, the ulp taken at the largest of
          |m|, |(1 - b1)(g - m)| and |m'| -- when b1 m and (1 - b1) g cancel, m' is far smaller than what was rounded on the way to it,
          and torch's own lerp_ is thousands of ulp(m') from the float64 value on such elements;
      v'  a sum of non-negative terms, four roundings: 4 ulp(v');
      p'  0.5 ulp(p') for the final subtraction + 4 * 2^-24 |dp| for sqrt, two divisions, the sum and the product behind dp, + the
          bar of m' carried through dp = step_size * m' / denom."""
    b1, b2 = betas
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m64 = m + (g - m) * (1.0 - b1)
    v64 = v * b2 + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    den = np.sqrt(v64) / np.sqrt(1.0 - b2 ** t) + eps
    dp = step_size * (m64 / den)
    p64 = p - dp
    bar_m = 4.0 * _ulp32(np.maximum(np.maximum(np.abs(m), np.abs((1.0 - b1) * (g - m))), np.abs(m64)))
    bar_v = 4.0 * _ulp32(v64)
    bar_p = 0.5 * _ulp32(p64) + 4.0 * 2.0 ** -24 * np.abs(dp) + (step_size / den) * bar_m
    # between two fp32 evaluations: both round their final subtraction, so they may sit a whole ulp(p') apart
    return dict(m=m64, v=v64, p=p64, dp=dp, bar_m=bar_m, bar_v=bar_v, bar_p=bar_p, bar_p_pair=bar_p + 0.5 * _ulp32(p64))


def adam_state(rng, shapes):
    """exp_avg uniform in +-1e-2; exp_avg_sq log-uniform over 1e-18 .. 1e-2: eps = 1e-8 decides the denominator of some elements,
    sqrt(v) that of others."""
    m = [rng.uniform(-1e-2, 1e-2, s).astype(np.float32) for s in shapes]
    v = [(10.0 ** rng.uniform(-18.0, -2.0, s)).astype(np.float32) for s in shapes]
    return m, v


def torch_adam_step(p, g, m, v, t, lr, betas, eps):
    """One step of torch.optim.Adam on the CPU in fp32 from the state (m, v, step t - 1) with gradient g: the new (p, m, v, step)."""
    import torch
    tp = torch.nn.Parameter(torch.from_numpy(np.array(p, np.float32)))
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps)
    opt.state[tp] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(np.array(m, np.float32)),
                         exp_avg_sq=torch.from_numpy(np.array(v, np.float32)))
    tp.grad = torch.from_numpy(np.array(g, np.float32))
    opt.step()
    st = opt.state[tp]
    return tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), float(st["step"])


def adam_check(what, got_p, got_m, got_v, exp):
    """Asserts one tensor's (p, m, v) against adam_expected's values and bars; returns the worst error / bar of each."""
    out = {}
    for k, got in (("m", got_m), ("v", got_v), ("p", got_p)):
        r = np.abs(np.asarray(got, np.float64) - exp[k]) / exp["bar_" + k]
        out[k] = float(r.max())
        i = np.unravel_index(int(r.argmax()), r.shape)
        assert out[k] <= 1.0, f"{what}: {k} at {i} is {out[k]:.2f} x its bar from the float64 value ({np.asarray(got)[i]!r} vs {exp[k][i]!r})"
    return out
