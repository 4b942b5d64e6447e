"""Cameras, images and the numpy restatement of the depth-image definition (include/omds.h: omds_depth_points) that
tests/test_depth_cpu.py and tests/test_gpu_depth.py share.

The restatement follows the header's text.  Up to xc, yc and z every operation is ONE float32 operation, which numpy float32 restates
bit for bit (raw -> z, the range gate, a, b, xc, yc).  numpy has no fused multiply-add, so the three nested fmaf of a world
coordinate are restated in float64: exact where every intermediate is a float32 (the exact case proves that of itself), otherwise a
reference within the bound of tests/test_depth_cpu.py."""
import numpy as np

F32, F64 = np.float32, np.float64
U16, FLT = 0, 1      # omds.h: OMDS_DEPTH_U16, OMDS_DEPTH_F32

LOOK_ALONG_X = np.array([[0, 0, 1], [-1, 0, 0], [0, -1, 0]], F64)      # camera z -> world x, image right -> world -y, image down -> world -z


def cam_of(width, height, fx, fy, cx, cy, pose=None, fmt=U16, depth_scale=0.001, z_min=0.1, z_max=10.0, step=1, pitch=0):
    from optimalmodulationds_amd.engine import depth_camera
    return depth_camera(width, height, fx, fy, cx, cy, pose, fmt, depth_scale, z_min, z_max, step, pitch)


def pose_of(R, t):
    return np.concatenate([np.asarray(R, F64), np.asarray(t, F64).reshape(3, 1)], 1).astype(F32)


def quat_pose(q, t):
    """[R | t] of the unit quaternion q = (w, x, y, z) / |q|"""
    w, x, y, z = np.asarray(q, F64) / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return pose_of(R, t)


def restate(cam, image):
    """image [H, W] (any row stride) -> dict over the visited pixels in row-major order:
    keep [V] (float32 gate), z32 [V], and in float64 a, b, xc, yc [V], t3, t2, w [V, 3] (the fmaf chain from the inside out: t3 =
    p2 z + p3, t2 = p1 yc + t3, w = p0 xc + t2) and S [V, 3] = |p0 xc| + |p1 yc| + |p2 z| + |p3|.  Dropped pixels carry z = 1."""
    step = max(int(cam.step), 1)
    us, vs = np.arange(0, cam.width, step), np.arange(0, cam.height, step)
    raw = np.asarray(image)[np.ix_(vs, us)].reshape(-1)
    u, v = np.tile(us, len(vs)), np.repeat(vs, len(us))
    with np.errstate(all="ignore"):
        if cam.format == U16:
            assert raw.dtype == np.uint16
            z32 = raw.astype(F32) * F32(cam.depth_scale)
            keep = raw != 0
        else:
            assert raw.dtype == F32
            z32 = raw.copy()
            keep = np.ones(len(raw), bool)
        keep &= (z32 >= F32(cam.z_min)) & (z32 <= F32(cam.z_max))
    ifx, ify = F32(1) / F32(cam.fx), F32(1) / F32(cam.fy)
    a32 = (u.astype(F32) - F32(cam.cx)) * ifx
    b32 = (v.astype(F32) - F32(cam.cy)) * ify
    z = np.where(keep, z32, F32(1)).astype(F64)
    a = (u.astype(F64) - F64(cam.cx)) * F64(ifx)
    b = (v.astype(F64) - F64(cam.cy)) * F64(ify)
    xc, yc = a * z, b * z
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    t3 = p[:, 2][None] * z[:, None] + p[:, 3][None]
    t2 = p[:, 1][None] * yc[:, None] + t3
    w = p[:, 0][None] * xc[:, None] + t2
    S = np.abs(p[:, 0][None] * xc[:, None]) + np.abs(p[:, 1][None] * yc[:, None]) + np.abs(p[:, 2][None] * z[:, None]) + np.abs(p[:, 3])[None]
    return dict(keep=keep, z32=z32, a32=a32, b32=b32, a=a, b=b, xc=xc, yc=yc, z=z, t3=t3, t2=t2, w=w, S=S, ifx=ifx, ify=ify)


def points_of(r):
    """the restatement's points as omds_depth_points writes them: float32, a dropped pixel three NaNs"""
    out = r["w"].astype(F32)
    out[~r["keep"]] = np.nan
    return out


def exact_camera(width=32, height=24, step=1, pitch=0, t=(0.25, -0.5, 0.75), z_min=2.0 ** -10, z_max=4.0):
    """power-of-two intrinsics, integer principal point, depth_scale 2^-10, a signed permutation looking along world x, t on the
    2^-6 lattice: with raw depths <= 4095 every intermediate of the definition is a float32"""
    return cam_of(width, height, 64.0, 32.0, 16.0, 8.0, pose_of(LOOK_ALONG_X, t), U16, 2.0 ** -10, z_min, z_max, step, pitch)


def exact_image(seed, width=32, height=24):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 4096, (height, width)).astype(np.uint16)
    img[rng.rand(height, width) < 0.1] = 0
    return img


def general_camera(fmt, width=64, height=48, step=1):
    return cam_of(width, height, 615.3, 614.9, width / 2 - 0.37, height / 2 + 0.21, quat_pose((0.8, 0.1, -0.5, 0.3), (0.31, -0.12, 0.93)), fmt,
                  0.001, 0.3, 4.0, step)


def general_image(seed, fmt, width=64, height=48):
    rng = np.random.RandomState(seed)
    metres = rng.uniform(0.1, 5.0, (height, width))
    if fmt == U16:
        img = np.round(metres * 1000).astype(np.uint16)
        img[rng.rand(height, width) < 0.1] = 0
        return img
    img = metres.astype(F32)
    img[rng.rand(height, width) < 0.1] = np.nan
    return img


# ---- rendered scenes for the device tests ------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """[R | t] of a camera at ``eye`` whose optical axis points at ``target`` (image x to the right, image y down)"""
    eye, target = np.asarray(eye, F64), np.asarray(target, F64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.asarray(up, F64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return pose_of(np.stack([x, y, z], 1), eye)



def rays(cam):
    """(origin [3], directions [H, W, 3] with unit depth along the optical axis) in the world frame, float64"""
    p = np.array(list(cam.pose), F64).reshape(3, 4)
    u, v = np.meshgrid(np.arange(cam.width, dtype=F64), np.arange(cam.height, dtype=F64))
    d_cam = np.stack([(u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, np.ones_like(u)], -1)
    return p[:, 3], d_cam @ p[:, :3].T


def render(cam, spheres=(), planes=(), far=0.0):
    """depth along the optical axis [H, W] float64 of the nearest hit of every pixel's ray with ``spheres`` (cx, cy, cz, r) and
    ``planes`` (n [3], d: n . x = d); ``far`` where nothing is hit"""
    o, d = rays(cam)
    best = np.full(d.shape[:2], np.inf)
    for s in spheres:
        c, r = np.asarray(s[:3], F64), float(s[3])
        oc = o - c
        A, B, Cc = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - r * r
        disc = B * B - 4 * A * Cc
        with np.errstate(invalid="ignore"):
            tt = (-B - np.sqrt(disc)) / (2 * A)
        tt = np.where((disc >= 0) & (tt > 0), tt, np.inf)
        best = np.minimum(best, tt)
    for n, dd in planes:
        n = np.asarray(n, F64)
        den = d @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = (dd - o @ n) / den
        tt = np.where((np.abs(den) > 1e-12) & (tt > 0), tt, np.inf)
        best = np.minimum(best, tt)
    return np.where(np.isfinite(best), best, far)


def to_u16(depth, scale=0.001):
    return np.clip(np.round(depth / scale), 0, 65535).astype(np.uint16)
