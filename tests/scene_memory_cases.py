"""Grids, frames and the numpy restatement of the scene memory of the depth route (include/omds.h: omds_depth_scene_memory) that
tests/test_scene_memory_cpu.py and tests/test_gpu_scene_memory.py share.

The restatement follows the header's text on top of depth_cases.restate (the points of an image) and cloud_cases.restate (the occupied
cells).  Every line of step 3 that is ONE float32 operation is restated by the same numpy float32 operation (the differences d_r, the
quotient 1 / zc, xc * iz, uf * istep, rint, lim).  numpy has no fused multiply-add: an fmaf is restated as the float64 expression
rounded to float32 once, which IS the fmaf wherever the float64 expression is exact -- on the exact camera (power-of-two intrinsics,
signed-permutation R, lattice t and lattice grids) it is, and the test asserts the stronger precondition that the rotated coordinates
xc, yc, zc and the cell centres are float32 values before any rounding.  On a general camera the restatement is not used."""
import numpy as np

import depth_cases as dc
from cloud_cases import restate as cloud_restate, spec_of
from depth_cases import F32, F64, FLT, U16

FLT_MAX = F32(3.402823466e+38)


def mem_of(max_age=0, clear_margin=0.0, footprint=0):
    from optimalmodulationds_amd.engine import scene_memory_spec
    return scene_memory_spec(max_age, clear_margin, footprint)


def is_f32(x):
    return np.array_equal(np.asarray(x, F64).astype(F32).astype(F64), np.asarray(x, F64))


def n_cells_of(spec):
    return int(spec.dims[0]) * int(spec.dims[1]) * int(spec.dims[2])


def cell_index(spec, ix, iy, iz):
    return (int(iz) * int(spec.dims[1]) + int(iy)) * int(spec.dims[0]) + int(ix)


def centres_of(spec, cells):
    """float32 centres [K, 3] of ``cells``: the three fmaf of the cell's sphere (float64, rounded once)"""
    dims = np.array(list(spec.dims), np.int64)
    cells = np.asarray(cells, np.int64)
    idx = np.stack([cells % dims[0], (cells // dims[0]) % dims[1], cells // (dims[0] * dims[1])], 1)
    return ((idx.astype(F64) + 0.5) * F64(spec.voxel) + np.array(list(spec.origin), F64)).astype(F32)


def clear_margin_of(spec, mem):
    radius = F32(spec.radius) if spec.radius > 0 else F32(0.8660254) * F32(spec.voxel)
    return F32(mem.clear_margin) if mem.clear_margin > 0 else radius


def project(cam, p, exact=None):
    """step 3 up to the pixel for points p [K, 3] float32 -> dict(zc, uf, vf, us, vs, ju, jv, gate, inside); ``exact``: a list that
    takes the names of the intermediates that were NOT float32 before rounding (the exact case's precondition)"""
    pose = np.array(list(cam.pose), F32).reshape(3, 4)
    d = (p - pose[:, 3][None]).astype(F32)
    out = {}
    for name, col in (("xc", 0), ("yc", 1), ("zc", 2)):
        last = (pose[2, col] * d[:, 2]).astype(F32)
        inner = pose[1, col].astype(F64) * d[:, 1].astype(F64) + last.astype(F64)
        full = pose[0, col].astype(F64) * d[:, 0].astype(F64) + inner.astype(F32).astype(F64)
        if exact is not None and not (is_f32(inner) and is_f32(full)):
            exact.append(name)
        out[name] = full.astype(F32)
    zc = out["zc"]
    with np.errstate(all="ignore"):
        gate = (zc >= F32(cam.z_min)) & (zc <= F32(cam.z_max))
        zs = np.where(gate, zc, F32(1))
        iz = F32(1) / zs
        xn, yn = out["xc"] * iz, out["yc"] * iz
        uf = (xn.astype(F64) * F64(cam.fx) + F64(cam.cx)).astype(F32)
        vf = (yn.astype(F64) * F64(cam.fy) + F64(cam.cy)).astype(F32)
        step = max(int(cam.step), 1)
        istep = F32(1) / F32(step)
        us, vs = uf * istep, vf * istep
        ju, jv = np.rint(us), np.rint(vs)
        nu, nv = -(-cam.width // step), -(-cam.height // step)
        inside = (ju >= 0) & (ju < F32(nu)) & (jv >= 0) & (jv < F32(nv))
    out.update(uf=uf, vf=vf, us=us, vs=vs, ju=ju, jv=jv, gate=gate, inside=inside, nu=nu, nv=nv, step=step)
    return out


def verdict(cam, image, p, margin, footprint, exact=None):
    """FREE [K] bool of one camera for the points p [K, 3]"""
    r = project(cam, p, exact)
    ok = r["gate"] & r["inside"]
    iu, iv = np.where(ok, r["ju"], 0).astype(np.int64), np.where(ok, r["jv"], 0).astype(np.int64)
    lim = (r["zc"] + F32(margin)).astype(F32)
    img = np.asarray(image)
    free = ok.copy()
    for b in range(-footprint, footprint + 1):
        for a in range(-footprint, footprint + 1):
            x, y = iu + a, iv + b
            window = (x >= 0) & (x < r["nu"]) & (y >= 0) & (y < r["nv"])
            raw = img[np.where(window, y, 0) * r["step"], np.where(window, x, 0) * r["step"]]
            with np.errstate(all="ignore"):
                if cam.format == U16:
                    z = raw.astype(F32) * F32(cam.depth_scale)
                    passes = (raw != 0) & (np.abs(z) <= FLT_MAX) & (z > lim)
                else:
                    z = raw.astype(F32)
                    passes = (np.abs(z) <= FLT_MAX) & (z > lim)
            free &= ~window | passes
    return free


def seen_cells(spec, cams, images):
    pts = np.concatenate([dc.points_of(dc.restate(c, im)) for c, im in zip(cams, images)])
    return cloud_restate(spec, pts)[0]


def restate(spec, mem, cams, images, mem_in=None, exact=None):
    """(words [cells] uint32, (seen, remembered, cleared, expired)) of one call, steps 1 - 5"""
    n = n_cells_of(spec)
    m = np.zeros(n, np.uint32) if mem_in is None else np.asarray(mem_in, np.uint32)
    seen = np.zeros(n, bool)
    seen[seen_cells(spec, cams, images)] = True
    out = np.zeros(n, np.uint32)
    out[seen] = 1
    cand = np.nonzero(~seen & (m != 0))[0]
    p = centres_of(spec, cand)
    margin = clear_margin_of(spec, mem)
    free = np.zeros(len(cand), bool)
    for c, im in zip(cams, images):
        free |= verdict(c, im, p, margin, int(mem.footprint), exact)
    rest = cand[~free]
    older = np.minimum(m[rest].astype(np.uint64) + 1, 0xFFFFFFFF)
    expired = (older > int(mem.max_age) + 1) if mem.max_age >= 1 else np.zeros(len(rest), bool)
    out[rest] = np.where(expired, 0, older).astype(np.uint32)
    return out, (int(seen.sum()), int((~expired).sum()), int(free.sum()), int(expired.sum()))


# ---- cameras, grids and frames -----------------------------------------------------------------------------------------------------
def exact_cam(fmt=U16, width=32, height=24, step=1, t=(0.25, -0.5, 0.75), z_max=4.0):
    """depth_cases.exact_camera, in either format (F32: metres on the 2^-10 lattice)"""
    return dc.cam_of(width, height, 64.0, 32.0, 16.0, 8.0, dc.pose_of(dc.LOOK_ALONG_X, t), fmt, 2.0 ** -10 if fmt == U16 else 1.0, 2.0 ** -10, z_max, step)


def frame(cam, metres, border=0):
    """an image of ``cam`` with depth ``metres`` everywhere but a border of ``border`` pixels without a return (metres None / 0: no
    return anywhere: raw 0, F32: NaN)"""
    shape = (cam.height, cam.width)
    blind = 0 if cam.format == U16 else np.nan
    img = np.full(shape, blind, np.uint16 if cam.format == U16 else F32)
    if metres:
        val = np.uint16(round(metres / cam.depth_scale)) if cam.format == U16 else F32(metres)
        img[border:shape[0] - border, border:shape[1] - border] = val
    return img


def put(img, cam, metres, rows, cols):
    """``img`` with ``metres`` (a float32 for F32 cameras, metres rounded to raw units for U16) over rows x cols (slices)"""
    out = img.copy()
    out[rows, cols] = np.uint16(round(float(metres) / cam.depth_scale)) if cam.format == U16 else F32(metres)
    return out


GRID_SMALL = dict(origin=(1.125, -1.125, -0.25), voxel=0.125, dims=(13, 11, 9))      # 1 287 cells around the exact camera's wall at 2 m
GRID_LARGE = dict(origin=(1.0, -1.5, -0.75), voxel=0.0625, dims=(40, 40, 40))        # 64 000 cells


def grid(kind=GRID_SMALL, max_spheres=4096, min_points=1, **over):
    g = dict(kind, **over)
    return spec_of(g["origin"], g["voxel"], g["dims"], 0.0, min_points, max_spheres)


def grid_around(points, voxel, dims, max_spheres=4096):
    """a grid of ``dims`` cells centred on the kept ``points`` (for cameras whose view is wherever their pose puts it)"""
    pts = points[~np.isnan(points).any(1)]
    centre = pts.mean(0)
    origin = np.round((centre - 0.5 * voxel * np.asarray(dims)) / voxel) * voxel
    return spec_of(tuple(float(v) for v in origin), voxel, dims, 0.0, 1, max_spheres)


def sequence(cam, wall=2.0, plate=1.0, far=3.0, border=2):
    """five frames of one camera: the wall, a plate over the left half in front of it, the plate gone, a blind frame, the wall gone (a
    return from behind where it was)"""
    w = frame(cam, wall, border)
    half = slice(0, cam.width // 2)
    return [w, put(w, cam, plate, slice(None), half), w.copy(), frame(cam, None), frame(cam, far)]
