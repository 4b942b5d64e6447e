"""The lens model of include/omds.h (THE LENS OF A DEPTH CAMERA) in float64, for tests/depth_lens_cases.py and the lens tests: the
forward model, a Newton inverse of it (not the library's fixed-point iteration), images rendered through that inverse, and the mirror of
a scene-memory verdict.  Coefficients ``k``: 8 floats in OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6."""
import numpy as np

F64 = np.float64


def coeffs(lens):
    """the 8 coefficients of an ``OmdsDepthLens`` (or a sequence of 4, 5 or 8) as float64"""
    k = [float(v) for v in (lens.k if hasattr(lens, "k") else lens)]
    return np.array(k + [0.0] * (8 - len(k)), F64)


def forward(k, a, b):
    """undistorted normalised (a, b) -> distorted (ad, bd) and the radial factor s"""
    k1, k2, p1, p2, k3, k4, k5, k6 = coeffs(k)
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    r2 = a * a + b * b
    s = (1 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    ad = a * s + 2 * p1 * a * b + p2 * (r2 + 2 * a * a)
    bd = b * s + p1 * (r2 + 2 * b * b) + 2 * p2 * a * b
    return ad, bd, s


def project(cam, k, a, b):
    """the pixel (uf, vf) that the ray (a, b) falls on"""
    ad, bd, _ = forward(k, a, b)
    return F64(cam.fx) * ad + F64(cam.cx), F64(cam.fy) * bd + F64(cam.cy)


def inverse(k, xd, yd, rounds=60, tol=1e-13):
    """Newton on forward(a, b) = (xd, yd) from (xd, yd), the Jacobian by central differences, each step halved until the residual
    falls.  -> (a, b, ok): ok where the residual ended below ``tol`` and s > 0"""
    xd, yd = np.asarray(xd, F64), np.asarray(yd, F64)
    a, b = xd.copy(), yd.copy()
    h = 1e-6

    def res(a, b):
        ad, bd, _ = forward(k, a, b)
        return ad - xd, bd - yd

    with np.errstate(all="ignore"):
        for _ in range(rounds):
            fx, fy = res(a, b)
            ax1, ay1 = forward(k, a + h, b)[:2]
            ax0, ay0 = forward(k, a - h, b)[:2]
            bx1, by1 = forward(k, a, b + h)[:2]
            bx0, by0 = forward(k, a, b - h)[:2]
            j11, j21, j12, j22 = (ax1 - ax0) / (2 * h), (ay1 - ay0) / (2 * h), (bx1 - bx0) / (2 * h), (by1 - by0) / (2 * h)
            det = j11 * j22 - j12 * j21
            da, db = (j22 * fx - j12 * fy) / det, (j11 * fy - j21 * fx) / det
            norm = np.hypot(fx, fy)
            step = np.ones_like(a)
            for _ in range(8):
                gx, gy = res(a - step * da, b - step * db)
                worse = ~(np.hypot(gx, gy) < norm)
                step = np.where(worse, step * 0.5, step)
            good = np.isfinite(da) & np.isfinite(db)
            a, b = np.where(good, a - step * da, a), np.where(good, b - step * db, b)
        fx, fy = res(a, b)
        s = forward(k, a, b)[2]
        ok = (np.hypot(fx, fy) < tol) & (s > 0)
    return a, b, ok


def pixel_rays(cam, k):
    """(a, b, ok) [H, W] float64: the undistorted ray of every pixel centre of the full image"""
    u, v = np.meshgrid(np.arange(cam.width, dtype=F64), np.arange(cam.height, dtype=F64))
    return inverse(k, (u - F64(cam.cx)) / F64(cam.fx), (v - F64(cam.cy)) / F64(cam.fy))


def render(cam, k, spheres=(), planes=(), far=0.0):
    """depth along the optical axis [H, W] float64 of the nearest hit of every pixel's ray -- through the lens -- with ``spheres``
    (cx, cy, cz, r) and ``planes`` (n [3], d: n . x = d) in the world frame; ``far`` where nothing is hit or the pixel has no ray"""
    a, b, ok = pixel_rays(cam, k)
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    o, d = p[:, 3], np.stack([a, b, np.ones_like(a)], -1) @ p[:, :3].T
    best = np.full(a.shape, np.inf)
    with np.errstate(all="ignore"):
        for s in spheres:
            c, r = np.asarray(s[:3], F64), float(s[3])
            oc = o - c
            A, B, Cc = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - r * r
            disc = B * B - 4 * A * Cc
            tt = (-B - np.sqrt(disc)) / (2 * A)
            best = np.minimum(best, np.where((disc >= 0) & (tt > 0), tt, np.inf))
        for n, dd in planes:
            n = np.asarray(n, F64)
            den = d @ n
            tt = (dd - o @ n) / den
            best = np.minimum(best, np.where((np.abs(den) > 1e-12) & (tt > 0), tt, np.inf))
    return np.where(np.isfinite(best) & ok, best, far)


def verdict(cam, k, r2_max, image_z, sm_margin, footprint, centre):
    """the float64 mirror of one camera's verdict on a cell centre (scene_memory_def.h with a lens): -> (free, near_tie): ``image_z``
    [H, W] float64 the depths of the image as the definition reads them (NaN: no return); near_tie: the projection lies within 1e-3
    visited pixels of a rounding tie or a depth within 1e-5 m of lim, where fp32 and float64 may disagree"""
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    pc = p[:, :3].T @ (np.asarray(centre, F64) - p[:, 3])
    step = max(int(cam.step), 1)
    nu, nv = -(-int(cam.width) // step), -(-int(cam.height) // step)
    if not (F64(cam.z_min) <= pc[2] <= F64(cam.z_max)):
        return False, min(abs(pc[2] - F64(cam.z_min)), abs(pc[2] - F64(cam.z_max))) < 1e-5
    a, b = pc[0] / pc[2], pc[1] / pc[2]
    if k is not None and not (a * a + b * b <= F64(r2_max)):
        return False, abs(a * a + b * b - F64(r2_max)) < 1e-6
    uf, vf = project(cam, k, a, b) if k is not None else (F64(cam.fx) * a + F64(cam.cx), F64(cam.fy) * b + F64(cam.cy))
    us, vs = uf / step, vf / step
    tie = min(abs(us - np.floor(us) - 0.5), abs(vs - np.floor(vs) - 0.5)) < 1e-3
    ju, jv = int(np.rint(us)), int(np.rint(vs))
    if not (0 <= ju < nu and 0 <= jv < nv):
        return False, tie
    lim = pc[2] + F64(sm_margin)
    free = True
    for y in range(max(jv - footprint, 0), min(jv + footprint, nv - 1) + 1):
        for x in range(max(ju - footprint, 0), min(ju + footprint, nu - 1) + 1):
            z = image_z[y * step, x * step]
            if not np.isfinite(z):
                free = False
            else:
                tie = tie or abs(z - lim) < 1e-5
                free = free and z > lim
    return free, tie
