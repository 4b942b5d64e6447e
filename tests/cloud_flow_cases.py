"""Cloud pairs, specs and the numpy restatement of the sphere-velocity definition (include/omds.h: omds_point_cloud_flow) that
tests/test_cloud_flow_cpu.py and tests/test_gpu_cloud_flow.py share.

The restatement follows the header's text: float32 throughout with the header's operation order, one numpy operation per named
operation (numpy's float32 +, -, *, / and its int64 -> float32 conversion are correctly rounded), integer sums in int64, and libm's
fmaf for the one fused chain (the speed under ``still``)."""
import ctypes
import ctypes.util
import functools

import numpy as np

from cloud_cases import F32, spec_of

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def fmaf(a, b, c):
    return F32(_libm.fmaf(float(a), float(b), float(c)))


def track_of(reach, dt_frame, still=0.0):
    from optimalmodulationds_amd.engine import cloud_track_spec
    return cloud_track_spec(reach, dt_frame, still)


def records(spec, pts):
    """per cell (n, s_x, s_y, s_z) as int64 [cells, 4]"""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    origin, voxel, dims = np.array(list(spec.origin), F32), F32(spec.voxel), np.array(list(spec.dims), np.int64)
    inv = F32(1.0) / voxel
    with np.errstate(all="ignore"):
        u = (pts - origin) * inv
        f = np.floor(u)
        keep = np.isfinite(pts).all(1) & (f >= F32(0)).all(1) & (f < dims.astype(F32)).all(1)
    u, f = u[keep], f[keep]
    r = u - f
    k = (r * F32(256.0)).astype(np.int64)           # truncation of a value in [0, 256)
    assert ((k >= 0) & (k <= 255)).all()
    i = f.astype(np.int64)
    cell = (i[:, 2] * dims[1] + i[:, 1]) * dims[0] + i[:, 0]
    rec = np.zeros((int(dims.prod()), 4), np.int64)
    np.add.at(rec[:, 0], cell, 1)
    for c in range(3):
        np.add.at(rec[:, 1 + c], cell, k[:, c])
    return rec


def restate_flow(spec, track, prev, now, with_mask=False):
    """-> (occupied NOW cells ascending, vel [count, 3] float32, matched, whole [count, 3] float32); with_mask: and which of the
    cells are matched [count] bool"""
    dims = np.array(list(spec.dims), np.int64)
    mp = max(int(spec.min_points), 1)
    voxel, dt, still, reach = F32(spec.voxel), F32(track.dt_frame), F32(track.still), int(track.reach)
    rn, rp = records(spec, now), records(spec, prev)
    occ = np.nonzero(rn[:, 0] >= mp)[0]
    idx = np.stack([occ % dims[0], (occ // dims[0]) % dims[1], occ // (dims[0] * dims[1])], 1)
    BIG = 1 << 30
    offs = [(kx, ky, kz) for kz in range(-reach, reach + 1) for ky in range(-reach, reach + 1) for kx in range(-reach, reach + 1)]

    def seen(k):
        j = idx + np.array(k, np.int64)
        inside = ((j >= 0) & (j < dims)).all(1)
        cj = np.where(inside, (j[:, 2] * dims[1] + j[:, 1]) * dims[0] + j[:, 0], 0)
        return inside & (rp[cj, 0] >= mp), cj

    best = np.full(len(occ), BIG, np.int64)
    for k in offs:
        ok, _ = seen(k)
        best = np.where(ok, np.minimum(best, k[0] ** 2 + k[1] ** 2 + k[2] ** 2), best)
    t, A, P, N = np.zeros(len(occ), np.int64), np.zeros((len(occ), 3), np.int64), np.zeros((len(occ), 3), np.int64), np.zeros(len(occ), np.int64)
    for k in offs:
        ok, cj = seen(k)
        ok &= best == k[0] ** 2 + k[1] ** 2 + k[2] ** 2
        t += ok
        A -= ok[:, None] * np.array(k, np.int64)
        P += ok[:, None] * rp[cj, 1:]
        N += ok * rp[cj, 0]
    matched = best < BIG
    vel, whole_all = np.zeros((len(occ), 3), F32), np.zeros((len(occ), 3), F32)
    m = matched
    with np.errstate(all="ignore"):
        whole = A[m].astype(F32) / t[m].astype(F32)[:, None]
        a = rn[occ[m], 1:].astype(F32) / rn[occ[m], 0].astype(F32)[:, None]
        b = P[m].astype(F32) / N[m].astype(F32)[:, None]
        diff = a - b
        sub = diff * F32(0.00390625)
        cells = whole + sub
        metres = cells * voxel
        v = metres / dt
    assert v.dtype == F32
    if still > 0:
        bar = still * still
        for row in v:
            s2 = fmaf(row[2], row[2], fmaf(row[1], row[1], row[0] * row[0]))
            if s2 < bar:
                row[:] = 0
    vel[m], whole_all[m] = v, whole
    return (occ, vel, int(matched.sum()), whole_all) + ((matched,) if with_mask else ())


def cell_points(spec, cell, offsets):
    """points at in-cell ``offsets`` [n, 3] (in cells, exact for a dyadic grid) of cell (i_x, i_y, i_z)"""
    o, v = np.array(list(spec.origin), F32), F32(spec.voxel)
    return (o + v * (np.array(cell, F32) + np.asarray(offsets, F32))).astype(F32)


# ---- the cases of the issue; each -> (spec, prev, now) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slab():
    """a one-cell-thick slab at i_x = 4, 5 points per cell at offsets that are multiples of 1/64 in [1/8, 1/2], moved 2.25 cells in x.
    The x offsets of every cell are a permutation of (8, 12, 16, 20, 24) / 64, so that their mean is exact in float32"""
    spec = spec_of((0.0, 0.0, 0.0), 0.0625, (16, 12, 8))
    rng = np.random.RandomState(31)
    prev = []
    for iy in range(2, 9):
        for iz in range(1, 6):
            off = np.stack([rng.permutation([8, 12, 16, 20, 24]), rng.randint(8, 33, 5), rng.randint(8, 33, 5)], 1) / 64.0
            prev.append(cell_points(spec, (4, iy, iz), off))
    prev = np.concatenate(prev)
    now = (prev + np.array([2.25 * 0.0625, 0, 0], F32)).astype(F32)
    return spec, prev, now


def ties(n):
    """one NOW cell at (5, 5, 5), every point at offset 1/2; 2 / 4 / 8 PREV cells at equal d2 one cell below in z (2, 4) or around (8)"""
    spec = spec_of((0.0, 0.0, 0.0), 0.0625, (12, 12, 12))
    where = {2: [(4, 5, 4), (6, 5, 4)], 4: [(4, 4, 4), (6, 4, 4), (4, 6, 4), (6, 6, 4)],
             8: [(5 + a, 5 + b, 5 + c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]}[n]
    half = [[0.5, 0.5, 0.5]] * 2
    prev = np.concatenate([cell_points(spec, c, half) for c in where])
    return spec, prev, cell_points(spec, (5, 5, 5), half)


def random_pair(seed, dims, n_prev, n_now, shift=(0.4, -1.3, 2.0), min_points=1, voxel=0.0625, origin=(-0.5, 0.25, 1.0), max_spheres=65536,
                fill=1.0):
    """a random cloud in the lower ``fill`` part of the box (along x) and an independent one moved by ``shift`` cells; both reach
    past the faces, so that the crop takes part"""
    spec = spec_of(origin, voxel, dims, min_points=min_points, max_spheres=max_spheres)
    rng = np.random.RandomState(seed)
    o, ext = np.array(origin, F32), np.array(dims) * voxel
    prev = (o + rng.uniform(-0.05, 1.05, (n_prev, 3)) * ext * np.array([fill, 1, 1])).astype(F32)
    now = (o + rng.uniform(-0.05, 1.05, (n_now, 3)) * ext * np.array([fill, 1, 1]) + np.array(shift) * voxel).astype(F32)
    return spec, prev, now


def corners():
    """the eight corner cells now, their inward diagonal neighbours before: every window is clipped on three faces"""
    spec = spec_of((-0.5, 0.25, 1.0), 0.0625, (6, 5, 4))
    d = np.array((6, 5, 4))
    rng = np.random.RandomState(33)
    prev, now = [], []
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                c = np.array((cx, cy, cz)) * (d - 1)
                inward = c + np.where(c == 0, 1, -1)
                now.append(cell_points(spec, c, rng.randint(1, 64, (3, 3)) / 64.0))
                prev.append(cell_points(spec, inward, rng.randint(1, 64, (4, 3)) / 64.0))
    return spec, np.concatenate(prev), np.concatenate(now)


@functools.lru_cache(maxsize=None)
def heavy():
    """70 000 points in one cell with k = 255 on every axis (s = 17 850 000 > 2^24), against a neighbour cell that held 70 001 such
    points and a second one at the same d2 (pooled s_x = 17 850 255 + 12, odd: its conversion to float32 rounds)"""
    spec = spec_of((0.0, 0.0, 0.0), 0.0625, (4, 4, 4))
    top = [[255.5 / 256] * 3]
    now = cell_points(spec, (1, 1, 1), top * 70000)
    prev = np.concatenate([cell_points(spec, (2, 1, 1), top * 70001), cell_points(spec, (1, 2, 1), [[4 / 256, 77 / 256, 0.5]] * 3)])
    return spec, prev, now


def few_spheres(n):
    """n NOW cells in a row (partial workgroups of the velocity kernel), the same surface one cell and a bit further in y before"""
    spec = spec_of((0.0, 0.0, 0.0), 0.0625, (8, 8, 8))
    rng = np.random.RandomState(40 + n)
    now = np.concatenate([cell_points(spec, (1 + i, 3, 2), rng.randint(0, 64, (3, 3)) / 64.0) for i in range(n)])
    prev = np.concatenate([cell_points(spec, (1 + i, 4 + i % 2, 2), rng.randint(0, 64, (2, 3)) / 64.0) for i in range(n)])
    return spec, prev, now
