"""How far is a pass-1 tile's union of firing units above what its rows need, and what does sorting the rows buy? (EXPERIMENTS.md R9)

k_pass1_dyn compacts every tile to the hidden units that fire in ANY of its rows (the exact zero-skip) and multiplies
ceil(T / 8) of 32 k-chunks per hidden->hidden layer, ceil(T / 16) of 16 for the last layer, T = the tile's firing units of the level
in front.  This restates that rule in numpy on the oracle -- shelf scene, shipped franka weights, real rollouts from orc.propagate --
for several ways of forming the tiles of one launch (one horizon step's N x O pairs):

    natural     rows t * O + o in order: what the device runs under OMDS_FLAG_NATURAL_PASS1
    single      one row per tile: the floor
    random      a random permutation of the pairs
    key-B       pairs sorted by the sign bits of B layer-1 pre-activations (csrc/tile_order.hip): the key units are the B units
                whose firing rate on the rows of horizon step --key-step is closest to 1/2, kept for the later steps
    weights-B   the same with key units chosen from the weights alone (smallest |b| / ||w||)

Per order and horizon step: executed / dense FLOP of the launch and the mean firing units per tile and level, to set beside the
device's omds_pass1_skip_stats for the same N.

    python tools/studies/tile_coherence.py [--tile 64] [--bits 12] [--n 1024] [--horizon 12] [--steps 2 5 11] [--key-step 2]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import omds_oracle as orc          # noqa: E402
from optimalmodulationds_amd import scenes     # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--tile", type=int, default=64, help="rows per tile")
ap.add_argument("--bits", type=int, default=12, help="key width")
ap.add_argument("--n", type=int, default=1024, help="rollouts")
ap.add_argument("--horizon", type=int, default=12)
ap.add_argument("--steps", type=int, nargs="*", default=[2, 5, 11], help="horizon steps (1-based) whose launch is analysed")
ap.add_argument("--key-step", type=int, default=2, help="horizon step whose rows choose the key units")
args = ap.parse_args()
N, H, MT, B = args.n, args.horizon, args.tile, args.bits

m = orc.Mlp.from_npz(os.path.join(ROOT, "tests", "golden", "weights", "franka.npz"))
obs = scenes.shelf_scene()
O = obs.shape[0]
rng = np.random.RandomState(0)
q0, qf = np.array(scenes.FRANKA_Q0, np.float32), np.array(scenes.FRANKA_QF, np.float32)
K = 10
s = (np.arange(K) + 0.5) / K
mu_c = (q0 + s[:, None] * (qf - q0) + 0.15 * rng.standard_normal((K, 7))).astype(np.float32)
mu = np.repeat(mu_c[None], N, 0)
sg = np.ones((N, K), np.float32)
al = (rng.standard_normal((K, 7)) + 3.0 * rng.standard_normal((N, K, 7))).astype(np.float32)
out = orc.propagate(m, q0, qf, obs, N=N, H=H, dt=0.5, k=5, ignored_links=[0, 1, 2], mu_tmp=mu, sigma_tmp=sg, alpha_tmp=al, prm=orc.Params(dst_thr=0.01))
traj = out.all_traj                                # [N, H, 7]: all_traj[:, i - 1] are the states horizon step i evaluates
NL = len(m.W) - 1                                  # hidden levels
WIDTH = m.W[0].shape[0]


def levels_of(states):
    """(z1 [N*O, WIDTH] layer-1 pre-activations, alive [NL][N*O, WIDTH] bool) of one launch, rows in the natural order"""
    x = np.concatenate([np.repeat(states, O, 0), np.tile(obs[:, :3], (states.shape[0], 1))], 1).astype(np.float32)
    h = orc.positional_encoding(x)
    z1, alive = None, []
    for i in range(NL):
        z = h @ m.W[i].T + m.b[i]
        z1 = z if i == 0 else z1
        h = np.maximum(z, 0)
        alive.append(h > 0)
    return z1, alive


def cost(alive, perm, tile):
    """executed / dense FLOP and firing units per tile and level under the kernel's chunk rule"""
    R = perm.shape[0]
    nt = (R + tile - 1) // tile
    pad = np.concatenate([perm, np.full(nt * tile - R, -1)])
    units, exe, dense = [], 32.0 * WIDTH, 32.0 * WIDTH                       # layer 1 is a dense K = 32 product
    for L in range(NL):
        a = np.concatenate([alive[L], np.zeros((1, WIDTH), bool)])[pad].reshape(nt, tile, WIDTH).any(1)
        T = a.sum(1)
        units.append(T.mean())
        last = L == NL - 1
        cols = 16 if last else WIDTH                                          # the last layer's channels are padded to 16
        exe += (np.ceil(T / 16) * 16 if last else np.ceil(T / 8) * 8).mean() * cols
        dense += WIDTH * cols
    return exe / dense, units


def key_order(z1, units):
    key = ((z1[:, units] > 0) << np.arange(len(units))).sum(1)
    return np.argsort(key, kind="stable")


z_key, _ = levels_of(traj[:, args.key_step - 1])
rate = (z_key > 0).mean(0)
units_rate = np.lexsort((np.arange(WIDTH), np.abs(rate - 0.5)))[:B]
units_w = np.argsort(np.abs(m.b[0]) / np.linalg.norm(m.W[0], axis=1), kind="stable")[:B]
print(f"shelf scene O = {O}, N = {N}, {N * O} rows per launch, tile {MT} rows, key {B} bits; key units from step {args.key_step}: {sorted(units_rate.tolist())}")
print(f"{'order':12s} {'step':>4s}  executed/dense   units alive per tile, levels 1..{NL}")
for step in args.steps:
    z1, alive = levels_of(traj[:, step - 1])
    R = N * O
    orders = {"natural": (np.arange(R), MT), "single": (np.arange(R), 1), "random": (rng.permutation(R), MT),
              f"key-{B}": (key_order(z1, units_rate), MT), f"weights-{B}": (key_order(z1, units_w), MT)}
    for name, (perm, tile) in orders.items():
        f, u = cost(alive, perm, tile)
        print(f"{name:12s} {step:4d}  {f:14.3f}   " + " / ".join(f"{x:5.1f}" for x in u))
