"""Where does the block order of the pass-1 tiles start to pay?  (EXPERIMENTS.md R12; the lines of profiles/r12_coherent_tiles_ab.txt)

Propagate time of the shelf workload (H = 32, K = 10 kernels, fixed policy samples, no update) at shard sizes, in ONE library: the
block order forced (OMDS_FLAG_BLOCK_TILES) against the natural order (OMDS_FLAG_NATURAL_TILES), alternating, 5 x 20 propagates each,
with the mean chunks per tile and level of both.  It brackets OMDS_BLOCK_TILES_MIN_PAIRS; it does not locate it.

    python tools/studies/block_tiles_threshold.py [N ...]      (on the GPU)"""
import sys, time
import numpy as np
import os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import omds_oracle as orc
from helpers import weights_path
from optimalmodulationds_amd import _lib as L, scenes
from optimalmodulationds_amd.engine import Engine

m = orc.Mlp.from_npz(weights_path("franka"))
obs = scenes.shelf_scene()
H, K = 32, 10
def engine(N, flags):
    rng = np.random.RandomState(0)
    q0, qf = np.array(scenes.FRANKA_Q0, np.float32), np.array(scenes.FRANKA_QF, np.float32)
    s = (np.arange(K) + 0.5) / K
    mu_c = (q0 + s[:, None] * (qf - q0) + 0.15 * rng.standard_normal((K, 7))).astype(np.float32)
    mu = np.repeat(mu_c[None], N, 0).astype(np.float32)
    al = (rng.standard_normal((K, 7)) + 3.0 * rng.standard_normal((N, K, 7))).astype(np.float32)
    e = Engine(7, N, H, 5, max_obs=512, flags=flags)
    e.set_mlp(m.W, m.b); e.set_obstacles(obs)
    e.params.dt = 0.5; e.params.dst_thr = 0.01; e.params.ignored_links = 0b111; e.push_params()
    e.set_ds(scenes.FRANKA_QF); e.set_policy_samples(mu, np.ones((N, K), np.float32), al)
    return e, q0
for N in ([int(a) for a in sys.argv[1:]] or (128, 256, 512, 768, 1024)):
    eng = {name: engine(N, fl) for name, fl in (("natural", L.FLAG_NATURAL_TILES), ("blocks", L.FLAG_BLOCK_TILES))}
    res = {k: [] for k in eng}
    for rep in range(5):
        for name, (e, q0) in eng.items():
            for _ in range(3): e.propagate(q0)
            t = time.perf_counter()
            for _ in range(20): e.propagate(q0)
            res[name].append((time.perf_counter() - t) / 20 * 1e3)
    st = {name: e.pass1_skip_stats() for name, (e, _) in eng.items()}
    for name in eng:
        v = res[name]
        print(f"N={N} {name:8s} ms/propagate median {np.median(v):.4f} min {min(v):.4f} max {max(v):.4f}  chunks {[round(c, 2) for c in st[name]['chunks']]} tiles {st[name]['tiles']}", flush=True)
    print(f"N={N} blocks/natural time {np.median(res['blocks']) / np.median(res['natural']):.4f}", flush=True)
    for e, _ in eng.values(): e.close()
