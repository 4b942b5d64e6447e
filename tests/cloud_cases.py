"""Clouds, specs and the numpy restatement of the point-cloud definition (include/omds.h: omds_point_cloud_spheres) that
tests/test_cloud_cpu.py and tests/test_gpu_cloud.py share."""
import numpy as np

F32 = np.float32


def spec_of(origin, voxel, dims, radius=0.0, min_points=1, max_spheres=4096):
    from optimalmodulationds_amd.engine import cloud_spec
    return cloud_spec(origin, voxel, dims, radius, min_points, max_spheres)


def restate(spec, pts):
    """The header's text in numpy float32 -> (occupied cell indices ascending, spheres [count, 4] with the centres formed in float32,
    product rounded before the sum, float64 centres [count, 3] with the product exact)"""
    pts = np.asarray(pts, F32).reshape(-1, 3)
    origin, voxel, dims = np.array(list(spec.origin), F32), F32(spec.voxel), np.array(list(spec.dims), np.int64)
    inv = F32(1.0) / voxel
    with np.errstate(all="ignore"):
        f = np.floor((pts - origin) * inv)
        keep = np.isfinite(pts).all(1) & (f >= F32(0)).all(1) & (f < dims.astype(F32)).all(1)
    i = f[keep].astype(np.int64)
    cell = (i[:, 2] * dims[1] + i[:, 1]) * dims[0] + i[:, 0]
    cnt = np.bincount(cell, minlength=int(dims.prod()))
    occ = np.nonzero(cnt >= max(int(spec.min_points), 1))[0]
    idx = np.stack([occ % dims[0], (occ // dims[0]) % dims[1], occ // (dims[0] * dims[1])], 1)
    centre = ((idx.astype(F32) + F32(0.5)) * voxel).astype(F32) + origin
    centre64 = (idx.astype(np.float64) + 0.5) * np.float64(voxel) + origin.astype(np.float64)
    radius = F32(spec.radius) if spec.radius > 0 else F32(0.8660254) * voxel
    return occ, np.concatenate([centre.astype(F32), np.full((len(occ), 1), radius, F32)], 1), centre64


def cells_of(spec, spheres):
    """cell index of every returned sphere, from its centre (exact: a centre lies half a cell inside)"""
    origin, voxel, dims = np.array(list(spec.origin), np.float64), float(spec.voxel), np.array(list(spec.dims), np.int64)
    i = np.floor((spheres[:, :3].astype(np.float64) - origin) / voxel).astype(np.int64)
    return (i[:, 2] * dims[1] + i[:, 1]) * dims[0] + i[:, 0]


def lattice_cloud(seed, n, lo, hi):
    """points on the 2^-10 lattice, uniform in [lo, hi)"""
    rng = np.random.RandomState(seed)
    return (rng.randint(int(lo * 1024), int(hi * 1024), (n, 3)) / 1024.0).astype(F32)


def edge_points(spec):
    """Points on cell faces (they belong to the cell above), on the box's upper faces and just below them, outside on every side, with
    +-inf / NaN coordinates, and duplicates: three copies of one point, two of another."""
    o, v, d = np.array(list(spec.origin), F32), F32(spec.voxel), np.array(list(spec.dims))
    top = (o + v * d.astype(F32)).astype(F32)
    inside = (o + v * F32(0.5)).astype(F32)
    pts = [o.copy(), inside, (o + v).astype(F32) if (d > 1).all() else inside]                 # the lower corner; a face of cell (1, 1, 1)
    for c in range(3):
        p = inside.copy(); p[c] = top[c]; pts.append(p)                                       # on an upper face: excluded
        p = inside.copy(); p[c] = np.nextafter(top[c], F32(-np.inf)); pts.append(p)           # the last float below it
        p = inside.copy(); p[c] = np.nextafter(o[c], F32(-np.inf)); pts.append(p)             # the last float below the lower face
        p = inside.copy(); p[c] = o[c] - F32(100); pts.append(p)
        p = inside.copy(); p[c] = top[c] + F32(1e30); pts.append(p)
        for bad in (np.inf, -np.inf, np.nan):
            p = inside.copy(); p[c] = bad; pts.append(p)
    dup3 = (o + v * ((d - 1).astype(F32) + F32(0.25))).astype(F32)                            # in the last cell
    dup2 = inside.copy(); dup2[0] = o[0] + v * F32(min(2, d[0] - 1) + 0.5)
    pts += [dup3] * 3 + [dup2] * 2
    return np.array(pts, F32)
