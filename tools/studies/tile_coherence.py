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
    blocks      what the device forms (csrc/tile_order.hip, k_pass1_dyn_blk), restated exactly: a row's layer-1 pre-activation is
                the rollout share r[t, u] = W1[u, joint features] . enc(q_t), plus the obstacle share p[o, u] = W1[u, point features]
                . enc(x_o), plus b1[u].  Key units: the B units u whose count of rollouts with r[t, u] + b1[u] + mean_o p[o, u] > 0
                on the rollouts of step --key-step is nearest N / 2 (|2 count - N|, ties by lower unit index), kept for the later
                steps.  Rollout key: bit j = r[t, u_j] + b1 + mean_o p > 0, from the step's own states; obstacle key: bit j =
                p[o, u_j] + b1 + mean_t r > 0 with the mean over the rollouts of step --key-step.  Both orders: by key, ties by
                lower index.  Tiles: 16 consecutive rollouts x 4 consecutive obstacles of the two orders (64 rows); a launch of
                >= 65 536 pairs ends on 8 x 4 blocks (32 rows) over its last ceil(256 / ceil(O / 4)) * 16 rollouts, one of
                >= 32 768 pairs puts N mod 16 rollouts into 8 x 4 blocks, smaller ones run 8 x 4 blocks only; a partial block
                repeats its last row.  Its line also gives the mean chunks per tile and level, the figure omds_pass1_skip_stats
                reports (bench.py --full: roofline.zero_skip.mean_chunks).
    blk-RxC     R consecutive rollouts x C consecutive obstacles of the same two orders, 64 rows, no 32-row tiles
    rollouts / obstacles-only   16 x 4 blocks with only the one order applied

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


def shares(states):
    """(r [N, WIDTH], p [O, WIDTH]): the rollout and the obstacle share of every layer-1 pre-activation (their sum + b1 is the row's)"""
    d = 10
    jq = np.concatenate([part * d + np.arange(7) for part in range(3)])
    jp = np.concatenate([part * d + 7 + np.arange(3) for part in range(3)])
    eq = orc.positional_encoding(np.concatenate([states, np.zeros((states.shape[0], 3), np.float32)], 1).astype(np.float32))[:, jq]
    ep = orc.positional_encoding(np.concatenate([np.zeros((O, 7), np.float32), obs[:, :3]], 1).astype(np.float32))[:, jp]
    return (eq @ m.W[0][:, jq].T).astype(np.float32), (ep @ m.W[0][:, jp].T).astype(np.float32)


def device_keys(states_key):
    """the device's key units and the constants of its two keys (k_tile_pick), from the rollouts of the key step"""
    r, p = shares(states_key)
    c_r = m.b[0] + p.mean(0)
    away = np.abs(2 * (r + c_r > 0).sum(0) - r.shape[0])
    units = np.lexsort((np.arange(WIDTH), away))[:B]
    return units, c_r[units], (m.b[0] + r.mean(0))[units], np.argsort((((p[:, units] + (m.b[0] + r.mean(0))[units]) > 0) << np.arange(B)).sum(1), kind="stable")


def block_perm(rperm, operm, rb, cb, mixed):
    """rows (t * O + o) of the device's launch in tile order, as (perm, tile) pieces; partial blocks repeat their last row"""
    ncb = -(-O // cb)
    oblk = np.minimum(np.arange(ncb * cb), O - 1).reshape(ncb, cb)
    pieces = []
    total = N * O
    nrb_big = (max(N // 16 - -(-256 // ncb), 0) if total >= 65536 else N // 16 if total >= 32768 else 0) if mixed else -(-N // rb)
    def tiles(r0, n, h):
        nb = -(-n // h)
        rblk = rperm[np.minimum(r0 + np.arange(nb * h), N - 1)].reshape(nb, h)
        return (rblk[:, None, :, None] * O + operm[oblk][None, :, None, :]).reshape(-1), h * cb
    if nrb_big:
        pieces.append(tiles(0, min(nrb_big * rb, N), rb))
    if mixed and nrb_big * 16 < N:
        pieces.append(tiles(nrb_big * 16, N - nrb_big * 16, 8))
    return pieces


def cost_pieces(alive, pieces):
    """cost() over several (perm, tile) pieces: executed / dense of the launch, units and chunks per tile and level"""
    exe = np.zeros(NL + 1)
    un, ch, nt_all = np.zeros(NL), np.zeros(NL), 0
    for perm, tile in pieces:
        nt = perm.shape[0] // tile
        nt_all += nt
        exe[0] += nt * tile * 32.0 * WIDTH
        for L in range(NL):
            T = alive[L][perm].reshape(nt, tile, WIDTH).any(1).sum(1)
            last = L == NL - 1
            c = np.ceil(T / 16) if last else np.ceil(T / 8)
            un[L] += T.sum(); ch[L] += c.sum()
            exe[L + 1] += (c * (16 if last else 8)).sum() * tile * (16 if last else WIDTH)
    dense = N * O * (32.0 * WIDTH + (NL - 1) * WIDTH * WIDTH + WIDTH * 16)
    return exe.sum() / dense, un / nt_all, ch / nt_all


z_key, _ = levels_of(traj[:, args.key_step - 1])
dev_units, dev_cr, dev_co, dev_operm = device_keys(traj[:, args.key_step - 1])
rate = (z_key > 0).mean(0)
units_rate = np.lexsort((np.arange(WIDTH), np.abs(rate - 0.5)))[:B]
units_w = np.argsort(np.abs(m.b[0]) / np.linalg.norm(m.W[0], axis=1), kind="stable")[:B]
print(f"shelf scene O = {O}, N = {N}, {N * O} rows per launch, tile {MT} rows, key {B} bits; key units from step {args.key_step}: {sorted(units_rate.tolist())}")
print(f"device key units (k_tile_pick): {dev_units.tolist()}")
print(f"{'order':12s} {'step':>4s}  executed/dense   units alive per tile, levels 1..{NL}")
for step in args.steps:
    z1, alive = levels_of(traj[:, step - 1])
    R = N * O
    orders = {"natural": (np.arange(R), MT), "single": (np.arange(R), 1), "random": (rng.permutation(R), MT),
              f"key-{B}": (key_order(z1, units_rate), MT), f"weights-{B}": (key_order(z1, units_w), MT)}
    for name, (perm, tile) in orders.items():
        f, u = cost(alive, perm, tile)
        print(f"{name:12s} {step:4d}  {f:14.3f}   " + " / ".join(f"{x:5.1f}" for x in u))
    r, _ = shares(traj[:, step - 1])
    rperm = np.argsort((((r[:, dev_units] + dev_cr) > 0) << np.arange(B)).sum(1), kind="stable")
    ident_r, ident_o = np.arange(N), np.arange(O)
    forms = {"blocks": block_perm(rperm, dev_operm, 16, 4, True), "blk-16x4": block_perm(rperm, dev_operm, 16, 4, False),
             "blk-8x8": block_perm(rperm, dev_operm, 8, 8, False), "blk-32x2": block_perm(rperm, dev_operm, 32, 2, False),
             "blk-64x1": block_perm(rperm, dev_operm, 64, 1, False), "rollouts-only": block_perm(rperm, ident_o, 16, 4, False),
             "obstacles-only": block_perm(ident_r, dev_operm, 16, 4, False), "unsorted-16x4": block_perm(ident_r, ident_o, 16, 4, False)}
    for name, pieces in forms.items():
        f, u, c = cost_pieces(alive, pieces)
        print(f"{name:14s} {step:2d}  {f:14.3f}   " + " / ".join(f"{x:5.1f}" for x in u) + ("   chunks " + " / ".join(f"{x:5.2f}" for x in c) if name == "blocks" else ""))
