"""GPU tests of SDF training on the device (csrc/train.hip, SURVEY 8 f4 / mlp_learn/train_sdf.py:96-151): the loss of every
epoch and the weights it moves, against (a) the run of the reference's own model class + torch.optim.Adam captured in
tests/golden/train_sdf_planar2.npz (tools/make_golden_train.py), (b) the numpy oracle, (c) a plain torch-CPU fp32 loop of the
same ops at the shipped network size (30 -> 256 x 4 -> 9).  Bars: loss 1e-5 relative at every epoch; weight DELTAS (what the
training moved) relative to the largest delta: 1e-4 after 10 epochs, 2e-3 after 100 -- Adam divides by sqrt(v): where a
gradient is at rounding level two fp32 evaluations step in different directions, and the numpy restatement itself is
9e-4 from the torch run after 100 epochs (tests/test_oracle_golden.py).  These are bars on whole training runs; the bars on a single
gradient (every dW and db against float64, on every kernel route) and on a single Adam step are in tests/test_gpu_train_grad.py."""
import numpy as np
import pytest

from helpers import load, weights_path
from oracle import omds_oracle as orc
from oracle import train_oracle as tro

pytestmark = pytest.mark.gpu


def _delta_err(W, W0, Wref):
    dmax = max(float(np.abs(r - w0).max()) for r, w0 in zip(Wref, W0))
    return max(float(np.abs(w - r).max()) for w, r in zip(W, Wref)) / dmax


def test_training_reproduces_the_reference_run():
    from optimalmodulationds_amd.trainer import SdfTrainer
    fx = load("train_sdf_planar2")
    nl = len([k for k in fx if k.startswith("W0_")])
    W0, b0 = [fx[f"W0_{i}"] for i in range(nl)], [fx[f"b0_{i}"] for i in range(nl)]
    dims = [W0[0].shape[1]] + [w.shape[0] for w in W0]
    tr = SdfTrainer(dims, "relu")
    tr.set_weights(W0, b0)
    tr.set_data(fx["x"], fx["y"])
    st = tro.TrainState(W0, b0)
    losses, olosses = [], []
    for e in range(int(fx["epochs"])):
        losses.append(tr.step(lr=float(fx["lr"])))
        olosses.append(tro.train_step(st, fx["x"], fx["y"], lr=float(fx["lr"])))
        if e + 1 in (10, 100):
            W, b = tr.get_weights()
            Wref, bref = [fx[f"W{e + 1}_{i}"] for i in range(nl)], [fx[f"b{e + 1}_{i}"] for i in range(nl)]
            bar = 1e-4 if e + 1 == 10 else 2e-3
            assert _delta_err(W, W0, Wref) <= bar, (e + 1, _delta_err(W, W0, Wref))
            assert _delta_err(b, b0, bref) <= bar, (e + 1, _delta_err(b, b0, bref))
            assert _delta_err(W, W0, st.W) <= bar and _delta_err(b, b0, st.b) <= bar      # and the numpy oracle
    rel = np.abs(np.asarray(losses) - fx["losses"]) / fx["losses"]
    assert rel.max() <= 1e-5, float(rel.max())
    assert (np.abs(np.asarray(losses) - np.asarray(olosses)) / np.asarray(olosses)).max() <= 1e-5
    assert abs(tr.eval() - float(fx["final_eval"])) <= 1e-5 * float(fx["final_eval"])
    assert losses[-1] < 0.1 * losses[0]                                                   # and it does train
    tr.close()


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_training_at_the_shipped_network_size_against_torch_cpu(act):
    """30 -> 256 x 4 -> 9 (the Franka network's shape; ragged batch, not a multiple of any tile) from the shipped weights: 30
    epochs beside the same ops in plain torch on the CPU -- MLPRegression.forward's NeRF features, F.mse_loss, torch.optim.Adam."""
    import torch
    import torch.nn.functional as F
    from optimalmodulationds_amd.trainer import SdfTrainer
    m = orc.Mlp.from_npz(weights_path("franka"))
    rng = np.random.RandomState(4)
    B = 3001
    x = rng.uniform(-2.0, 2.0, (B, 10)).astype(np.float32)
    y = (orc.mlp_forward(m, x) + 5.0 * rng.standard_normal((B, 9))).astype(np.float32)   # targets the net does not fit yet
    dims = [30, 256, 256, 256, 256, 9]
    tr = SdfTrainer(dims, act)
    tr.set_weights(m.W, m.b)
    tr.set_data(x, y)
    Wt = [torch.tensor(w.copy(), requires_grad=True) for w in m.W]
    bt = [torch.tensor(v.copy(), requires_grad=True) for v in m.b]
    opt = torch.optim.Adam(Wt + bt, lr=2e-4)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    worst = 0.0
    for e in range(30):
        h = torch.cat((xt, torch.sin(xt), torch.cos(xt)), dim=1)
        for i in range(5):
            h = F.linear(h, Wt[i], bt[i])
            if i < 4:
                h = torch.relu(h) if act == "relu" else torch.tanh(h)
        loss = F.mse_loss(h, yt, reduction='mean')
        loss.backward()
        opt.step()
        opt.zero_grad()
        got = tr.step(lr=2e-4)
        # the loss BEFORE any update is the forward pass alone: 1e-5.  From the second update on, the trained ReLU weights' rounding-level
        # gradients (below) have moved some weights by +-lr in opposite directions in the two runs, and the loss follows: 2e-5 (every
        # product of the trainer sums in ascending k like torch's sgemm: seen 0.9e-5 over 30 epochs; the printed `worst` is the record)
        worst = max(worst, abs(got - loss.item()) / loss.item())
        assert abs(got - loss.item()) <= (1e-5 if (e < 2 or act == "tanh") else 2e-5) * loss.item(), (e, got, loss.item())
        if e + 1 in (5, 30):
            # Trained weights carry units whose gradient is at rounding level (near-dead ReLUs); Adam's first steps are
            # lr * g / |g| whatever |g| is, so two fp32 evaluations move such a weight by +-lr in different directions.
            # Hence: all but 0.5 % of the elements within the bar (seen: 0.26 % after 30 epochs), nobody further than sign flips explain
            W, b = tr.get_weights()
            bar = 1e-4 if e + 1 == 5 else 1e-3
            for got_l, ref_l, w0_l in ((W, [w.detach().numpy() for w in Wt], m.W), (b, [v.detach().numpy() for v in bt], m.b)):
                dmax = max(float(np.abs(r - w0).max()) for r, w0 in zip(ref_l, w0_l))
                err = np.concatenate([np.abs(g - r).ravel() for g, r in zip(got_l, ref_l)])
                assert (err > bar * dmax).mean() <= 5e-3, (e + 1, float((err > bar * dmax).mean()), dmax)
                assert err.max() <= 2.0 * 2e-4 * (e + 1), (e + 1, float(err.max()))
    print(f"{act}: largest relative loss difference over 30 epochs {worst:.2e}")
    tr.close()


def test_trained_weights_round_trip_through_the_reference_checkpoint_format(tmp_path):
    """train -> the checkpoint dictionary train_sdf.py:130-138 saves -> RobotSdfCollisionNet.load_weights -> the rollout engine's
    forward (omds_mlp_forward_vjp) gives the trainer's own predictions; ReduceLROnPlateau follows torch's schedule."""
    import torch
    from optimalmodulationds_amd import RobotSdfCollisionNet
    from optimalmodulationds_amd.engine import Engine
    from optimalmodulationds_amd.trainer import ReduceLROnPlateau, SdfTrainer, checkpoint_dict, planar_link_distances
    rng = np.random.RandomState(1)
    x, y = planar_link_distances(rng, 1500, n_links=2, link_len=3.0)
    x = np.concatenate((x, np.zeros((x.shape[0], 1), np.float32)), axis=1)       # planar point + z = 0: the 2-DoF planner net takes 5 inputs
    net0 = orc.Mlp.from_npz(weights_path("planar2"))
    dims = [15, 256, 256, 256, 256, 2]
    tr = SdfTrainer(dims, "relu")
    tr.set_weights(net0.W, net0.b)
    tr.set_data(x, y)
    # (with the script's own eps = 1e-4 the schedule never leaves 2e-4 -- halving it changes the rate by exactly eps, which is
    # not "more than eps" -- so the plateau case runs with eps = 1e-8; the script's setting is checked at the end)
    sched = ReduceLROnPlateau(2e-4, factor=0.5, patience=3, threshold=0.01, eps=1e-8)
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.Adam([p], lr=2e-4)
    tsched = torch.optim.lr_scheduler.ReduceLROnPlateau(topt, mode='min', factor=0.5, patience=3, threshold=0.01, threshold_mode='rel', eps=1e-8)
    for e in range(12):
        tr.step(lr=sched.lr)
        val = tr.eval() if e < 6 else 1.0 + 0.001 * e                          # a plateau from epoch 6 on: the rate must halve
        sched.step(val)
        tsched.step(val)
        assert abs(sched.lr - topt.param_groups[0]["lr"]) < 1e-12
    assert sched.lr < 2e-4
    ref_cfg = ReduceLROnPlateau(2e-4, factor=0.5, patience=2, threshold=0.01, eps=1e-4)   # train_sdf.py:85-87 (patience shortened)
    for e in range(10):
        ref_cfg.step(1.0)
    assert ref_cfg.lr == 2e-4
    mse, pred = tr.eval(want_pred=True)
    W, b = tr.get_weights()
    path = str(tmp_path / "2dof_sdf_256x5_trained.pt")
    torch.save(checkpoint_dict(12, W, b, 5, 2), path)
    nn = RobotSdfCollisionNet(5, 2, [], [256] * 4)
    nn.load_weights(path, {'device': 'cpu', 'dtype': torch.float32})
    eng = Engine(2, 256, 2, 1, max_obs=8)
    eng.set_mlp(nn.model.W, nn.model.b)
    yy, _, _ = eng.mlp_forward_vjp(x[:200])
    assert np.abs(yy - pred[:200]).max() <= 1e-5 * max(1.0, float(np.abs(pred).max()))
    eng.close()
    tr.close()


def test_validation_split_and_optimizer_state_round_trip():
    """(a) One trainer holds the training and the validation split (train_sdf.py:84-86, 117-121): ``eval(val=True)`` equals a second
    trainer given the same weights and the validation rows as its data.  (b) The optimizer state leaves and re-enters in
    torch.optim.Adam's own state_dict() shape: a run interrupted after 5 epochs, saved as the reference's checkpoint dictionary and
    resumed in a NEW trainer continues bit for bit like the uninterrupted one; torch's Adam accepts the dictionary."""
    import torch
    from optimalmodulationds_amd.trainer import SdfTrainer, checkpoint_dict
    rng = np.random.RandomState(4)
    dims = [15, 64, 64, 2]
    W0 = [(0.3 * rng.standard_normal((dims[i + 1], dims[i]))).astype(np.float32) for i in range(3)]
    b0 = [(0.1 * rng.standard_normal(dims[i + 1])).astype(np.float32) for i in range(3)]
    x, y = rng.uniform(-2, 2, (3000, 5)).astype(np.float32), rng.uniform(0, 3, (3000, 2)).astype(np.float32)
    xv, yv = rng.uniform(-2, 2, (5000, 5)).astype(np.float32), rng.uniform(0, 3, (5000, 2)).astype(np.float32)   # larger than the training set
    a = SdfTrainer(dims, "relu")
    a.set_weights(W0, b0)
    a.set_data(x, y)
    a.set_val_data(xv, yv)
    losses_a = [a.step(lr=1e-3) for _ in range(5)]
    v_a, pred_a = a.eval(want_pred=True, val=True)
    ref = SdfTrainer(dims, "relu")
    ref.set_weights(*a.get_weights())
    ref.set_data(xv, yv)
    v_ref, pred_ref = ref.eval(want_pred=True)
    assert v_a == v_ref and np.array_equal(pred_a, pred_ref) and pred_a.shape == (5000, 2)
    assert a.eval() == pytest.approx(losses_a[-1], rel=0.2)                  # the training set is still in place
    # interrupted after 5 epochs -> checkpoint -> a new trainer
    ck = checkpoint_dict(5, *a.get_weights(), 5, 2, a.optimizer_state_dict())
    st = ck["optimizer_state_dict"]
    assert sorted(st["state"]) == list(range(6)) and float(st["state"][0]["step"]) == 5.0 and st["param_groups"][0]["lr"] == 1e-3
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for pair in zip(*a.get_weights()) for p in pair]   # weight 0, bias 0, weight 1, ...
    torch.optim.Adam(params, lr=1e-3).load_state_dict(st)                    # torch takes it as its own
    b_ = SdfTrainer(dims, "relu")
    b_.set_weights([ck["model_state_dict"][f"layers.0.{i}.0.weight"].numpy() for i in range(3)],
                   [ck["model_state_dict"][f"layers.0.{i}.0.bias"].numpy() for i in range(3)])
    b_.load_optimizer_state_dict(st)
    b_.set_data(x, y)
    cont_a = [a.step(lr=1e-3) for _ in range(5)]
    cont_b = [b_.step(lr=1e-3) for _ in range(5)]
    assert cont_a == cont_b
    for wa, wb in zip(a.get_weights()[0] + a.get_weights()[1], b_.get_weights()[0] + b_.get_weights()[1]):
        assert np.array_equal(wa, wb)
    fresh = SdfTrainer(dims, "relu")                                          # without the state the resumed run differs (bias correction restarts)
    fresh.set_weights([ck["model_state_dict"][f"layers.0.{i}.0.weight"].numpy() for i in range(3)],
                      [ck["model_state_dict"][f"layers.0.{i}.0.bias"].numpy() for i in range(3)])
    fresh.set_data(x, y)
    fresh.step(lr=1e-3)
    assert not np.array_equal(fresh.get_weights()[0][0], np.zeros(1)) and fresh.optimizer_state_dict()["state"][0]["step"] == 1.0
    for t in (a, b_, ref, fresh):
        t.close()


@pytest.mark.parametrize("act,B", [("relu", 20011), ("tanh", 4099)])
def test_special_shape_kernels_are_the_general_kernel_bit_for_bit(act, B):
    """k_gemm_tall (persistent, LDS-DMA rows, parked outputs), k_gemm_thin*, k_wgrad_thin against the general k_gemm -- six
    training steps from the same start on a batch that is NOT a multiple of the 64-row tile, weights and Adam state array-equal.  The
    test library's hook (include/omds_test.h: omds_debug_trainer_general_gemm) puts every product on the general kernel; every kernel
    sums in ascending k from zero, so a difference would be a bug (a race on the parked outputs, a wrong k permutation), not rounding."""
    from optimalmodulationds_amd import _lib as L
    from optimalmodulationds_amd.trainer import SdfTrainer
    lib = L.load_test_hooks()
    m = orc.Mlp.from_npz(weights_path("franka"))
    rng = np.random.RandomState(4)
    x = rng.uniform(-2.0, 2.0, (B, 10)).astype(np.float32)
    y = (orc.mlp_forward(m, x) + 5.0 * rng.standard_normal((B, 9))).astype(np.float32)
    outs = []
    for general in (1, 0):
        assert lib.omds_debug_trainer_general_gemm(general) == 0
        tr = SdfTrainer([30, 256, 256, 256, 256, 9], act, lib=lib)
        tr.set_weights(m.W, m.b)
        tr.set_data(x, y)
        losses = [tr.step(lr=2e-4) for _ in range(6)]
        W, b = tr.get_weights()
        st = tr.optimizer_state_dict()["state"]
        outs.append((losses, W, b, [st[i]["exp_avg"].numpy().copy() for i in st], [st[i]["exp_avg_sq"].numpy().copy() for i in st]))
        tr.close() if hasattr(tr, "close") else None
    lib.omds_debug_trainer_general_gemm(0)
    (l0, W0, b0, m0, v0), (l1, W1, b1, m1, v1) = outs
    assert l0 == l1, (l0, l1)
    for a, c in zip(W0 + b0 + m0 + v0, W1 + b1 + m1 + v1):
        assert np.array_equal(a, c)
