"""States, sphere lists and the numpy restatement of the velocity filter's definition (include/omds.h: omds_velocity_filter_step) that
tests/test_velocity_filter_cpu.py and tests/test_gpu_velocity_filter.py share.

The restatement follows the header's text: float32 throughout with the header's operation order, one numpy operation per named
operation (numpy's float32 +, -, *, / and its int64 -> float32 conversion are correctly rounded), integer sums in int64, libm's fmaf
for the fused steps and ``np.rint`` for the record."""
import numpy as np

from cloud_cases import F32, spec_of
from cloud_flow_cases import fmaf, track_of

SCALE = F32(1.52587890625e-5)          # 2^-16
GRIDS = ((12, 10, 9), (7, 5, 3))


def filt_of(alpha=0.3, alpha_object=0.0, max_jump=0.0):
    from optimalmodulationds_amd.engine import velocity_filter_spec
    return velocity_filter_spec(alpha, alpha_object, max_jump)


def grid_spec(dims, voxel=0.0625, origin=(-0.5, 0.25, 1.0)):
    return spec_of(origin, voxel, dims)


def cell_of(dims, ix, iy, iz):
    return (iz * dims[1] + iy) * dims[0] + ix


def _still(track, v):
    still = F32(track.still)
    if still > 0:
        s2 = fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0]))
        if s2 < still * still:
            return np.zeros(3, F32)
    return v


def _predecessor(dims, reach, state, c):
    """(S [3] int64, t, h) of the sphere in cell c; h = 0: an empty window"""
    ix, iy, iz = c % dims[0], (c // dims[0]) % dims[1], c // (dims[0] * dims[1])
    best, S, t, h = None, np.zeros(3, np.int64), 0, 0
    for z in range(max(iz - reach, 0), min(iz + reach, dims[2] - 1) + 1):
        for y in range(max(iy - reach, 0), min(iy + reach, dims[1] - 1) + 1):
            for x in range(max(ix - reach, 0), min(ix + reach, dims[0] - 1) + 1):
                q = state[cell_of(dims, x, y, z)]
                if q[3] < 1:
                    continue
                d2 = (x - ix) ** 2 + (y - iy) ** 2 + (z - iz) ** 2
                if best is None or d2 < best:
                    best, S, t, h = d2, np.zeros(3, np.int64), 0, int(q[3])
                if d2 == best:
                    S, t, h = S + q[:3], t + 1, min(h, int(q[3]))
    return S, t, h


def restate_step(spec, track, filt, state_in, cell, raw, live=None, group=None):
    """-> (vel [n, 3] float32, state_out [cells, 4] int32, (with history, restarts, groups with history))"""
    dims = [int(d) for d in spec.dims]
    n_cells, reach = dims[0] * dims[1] * dims[2], int(track.reach)
    alpha, max_jump = F32(filt.alpha), F32(filt.max_jump)
    alpha_object = F32(filt.alpha_object) if filt.alpha_object > 0 else alpha
    state = np.zeros((n_cells, 4), np.int64) if state_in is None else np.asarray(state_in, np.int64).reshape(n_cells, 4)
    cell, raw = np.asarray(cell, np.int64).reshape(-1), np.asarray(raw, F32).reshape(-1, 3)
    n = len(cell)
    live = np.ones(n, np.int64) if live is None else np.asarray(live, np.int64)
    group = np.full(n, -1, np.int64) if group is None else np.asarray(group, np.int64)
    pred = [_predecessor(dims, reach, state, int(c)) for c in cell]
    groups = {}
    for i in range(n):
        S, t, h = pred[i]
        if live[i] and group[i] >= 0 and h > 0:
            G = groups.setdefault(int(group[i]), [np.zeros(3, np.int64), 0, h])
            G[0], G[1], G[2] = G[0] + S, G[1] + t, min(G[2], h)
    vel, out = np.zeros((n, 3), F32), np.zeros((n_cells, 4), np.int32)
    with_history = restarts = 0
    for i in range(n):
        if not live[i]:
            continue
        grouped = group[i] >= 0
        S, t, h = groups.get(int(group[i]), (np.zeros(3, np.int64), 0, 0)) if grouped else pred[i]
        v, hits = raw[i].copy(), 1
        if h > 0:
            with_history += 1
            with np.errstate(all="ignore"):
                p = (np.asarray(S, np.int64).astype(F32) / np.int64(t).astype(F32)) * SCALE
                a = np.fmax(alpha_object if grouped else alpha, F32(1.0) / np.int64(h + 1).astype(F32))
                d = raw[i] - p
                j2 = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]))
                assert p.dtype == F32 and d.dtype == F32 and a.dtype == F32
                if max_jump > 0 and j2 > max_jump * max_jump:
                    restarts += 1
                else:
                    if not a >= F32(1.0):
                        v = np.array([fmaf(a, d[c], p[c]) for c in range(3)], F32)
                    hits = min(h + 1, 255)
        with np.errstate(all="ignore"):
            q = np.rint(np.fmin(np.fmax(v, F32(-1024.0)), F32(1024.0)) * F32(65536.0))
        out[cell[i], :3] = q.astype(np.int64)
        out[cell[i], 3] = hits
        vel[i] = _still(track, v)
    return vel, out, (with_history, restarts, len(groups))


# ---- the cases of the issue; each -> dict(spec, track, filt, state_in, cell, raw, live, group) --------------------------------------
def case(dims, track, filt, state_in, cell, raw, live=None, group=None):
    order = np.argsort(np.asarray(cell))
    pick = lambda a: None if a is None else np.asarray(a)[order]
    return dict(spec=grid_spec(dims), track=track, filt=filt, state_in=None if state_in is None else np.asarray(state_in, np.int32),
                cell=np.asarray(cell, np.int32)[order], raw=np.asarray(raw, F32).reshape(-1, 3)[order],
                live=None if live is None else pick(live).astype(np.int32), group=None if group is None else pick(group).astype(np.int32))


def random_state(rng, dims, fill, hits=(1, 2, 3, 17, 254, 255)):
    n_cells = dims[0] * dims[1] * dims[2]
    state = np.zeros((n_cells, 4), np.int32)
    on = rng.rand(n_cells) < fill
    state[on, :3] = rng.randint(-3 * 65536, 3 * 65536, (int(on.sum()), 3))
    state[on, 3] = rng.choice(hits, int(on.sum()))
    return state


def face_cells(dims):
    """the eight corners, the centre of every face and the centre: every way a window is clipped"""
    along = [(0, d // 2, d - 1) for d in dims]
    return sorted({cell_of(dims, x, y, z) for x in along[0] for y in along[1] for z in along[2]})


def random_case(seed, dims, reach, fill=0.15, n_extra=120, alpha=0.3, alpha_object=0.0, max_jump=0.0, still=0.0, groups=0):
    """a random state and a list of the 27 face / corner / centre cells plus random ones, with random velocities, a few dead spheres
    and, with ``groups``, that many groups of spheres sharing one raw velocity"""
    rng = np.random.RandomState(seed)
    n_cells = dims[0] * dims[1] * dims[2]
    cells = sorted(set(face_cells(dims)) | set(rng.choice(n_cells, min(n_extra, n_cells), replace=False).tolist()))
    n = len(cells)
    raw = (rng.uniform(-2.5, 2.5, (n, 3))).astype(F32)
    live = (rng.rand(n) < 0.9).astype(np.int32)
    raw[live == 0] = 0
    group = np.full(n, -1, np.int32)
    for k in range(groups):
        members = np.arange(n)[k::max(groups + 2, 1)][: 5 + 3 * k]
        members = members[live[members] == 1]
        if len(members):
            group[members] = cells[members[0]]
            raw[members] = raw[members[0]]
    return case(dims, track_of(reach, 0.1, still), filt_of(alpha, alpha_object, max_jump), random_state(rng, dims, fill), cells, raw, live,
                group if groups else None)


def single(dims, at, state_cells, raw, reach=2, **filt):
    """one sphere in cell ``at`` (ix, iy, iz) against a state of ``state_cells`` {(ix, iy, iz): (qx, qy, qz, hits)}"""
    state = np.zeros((dims[0] * dims[1] * dims[2], 4), np.int32)
    for c, q in state_cells.items():
        state[cell_of(dims, *c)] = q
    return case(dims, track_of(reach, 0.1, filt.pop("still", 0.0)), filt_of(**filt), state, [cell_of(dims, *at)], [raw])


def tie():
    """two state cells at equal d2 on either side, q of opposite sign and different size: the average matters"""
    return single(GRIDS[0], (5, 5, 4), {(4, 5, 4): (3 * 65536, -65536, 40000, 3), (6, 5, 4): (-65536, 65536, 40001, 7),
                                        (5, 5, 6): (9 * 65536, 9 * 65536, 9 * 65536, 1)}, (0.5, 0.25, -1.0))


def own_cell():
    """the own cell holds history: it alone is the predecessor, whatever the neighbours hold"""
    return single(GRIDS[0], (5, 5, 4), {(5, 5, 4): (65536, 0, -32768, 4), (4, 5, 4): (9 * 65536, 9 * 65536, 9 * 65536, 1),
                                        (6, 5, 4): (-9 * 65536, 0, 0, 2)}, (0.5, 0.25, -1.0))


def hits_case(h, alpha=0.3):
    return single(GRIDS[1], (3, 2, 1), {(3, 2, 1): (65536 + 7, -3 * 65536 + 1, 11, h)} if h else {}, (0.7, -2.9, 0.3), alpha=alpha)


def jump_case(above):
    """p = 0, max_jump = 0.75 (its square exact, one ulp 2^-24): raw = (0.75, 0, 0) has j2 = max_jump^2 exactly, raw = (0.75, 2^-12, 0)
    one ulp more"""
    return single(GRIDS[1], (3, 2, 1), {(3, 2, 1): (0, 0, 0, 5)}, (0.75, 2.0 ** -12 if above else 0.0, 0.0), max_jump=0.75)


def clamp_and_ties():
    """velocities beyond +-1024 m/s, and v 2^16 exactly between two integers (ties to even), without history: v = raw"""
    dims = GRIDS[1]
    raw = [(2000.0, -5000.0, 1024.0), (0.5 / 65536, 1.5 / 65536, 2.5 / 65536), (-0.5 / 65536, -1.5 / 65536, -2.5 / 65536),
           (np.inf, -np.inf, -1024.0), (1023.99999, -1023.99999, 3.5 / 65536)]
    return case(dims, track_of(1, 0.1), filt_of(), None, [3, 17, 40, 41, 104], raw)


def group_case(history=True):
    """five spheres of one object (one raw velocity, label = their smallest cell) whose predecessors differ -- two with their own cell,
    one with a tie, one with an empty window -- beside a free sphere; without ``history`` the state is empty"""
    dims = GRIDS[0]
    members = [(2, 2, 2), (3, 2, 2), (4, 2, 2), (9, 8, 7), (2, 3, 2)]
    state = np.zeros((dims[0] * dims[1] * dims[2], 4), np.int32)
    if history:
        state[cell_of(dims, 2, 2, 2)] = (65536, 100, -7, 3)
        state[cell_of(dims, 3, 2, 2)] = (2 * 65536, -100, 9, 9)
        state[cell_of(dims, 5, 2, 2)] = (-65536, 65536 // 3, 1, 2)           # (4, 2, 2) finds (3, 2, 2) and this one at d2 = 1
        state[cell_of(dims, 6, 6, 3)] = (7, 7, 7, 255)                       # the free sphere's
    cells = [cell_of(dims, *m) for m in members] + [cell_of(dims, 6, 6, 4)]
    raw = [(0.4, -0.2, 0.1)] * 5 + [(1.0, 1.0, 1.0)]
    return case(dims, track_of(1, 0.1), filt_of(0.3, 0.6), state, cells, raw, [1] * 6, [min(cells[:5])] * 5 + [-1])


def still_case():
    """the blend lands below the still bar: the output is +0, the stored q is not"""
    return single(GRIDS[1], (3, 2, 1), {(3, 2, 1): (6554, 0, 0, 200)}, (0.12, 0.0, 0.0), still=0.2, alpha=0.5)
