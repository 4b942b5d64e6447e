"""Cases of the lens tests (tests/test_depth_lens_cpu.py, tests/test_gpu_depth_lens.py): small cameras, at most 67 x 50, grids of at
most 32^3 cells.  The lenses are the two whose convergence include/omds.h states -- a plumb-bob one and a Kinect-NFOV-like rational
one -- scaled to the image (fx = fy = 40 at 64 x 48 spans the normalised field of view of fx = 600 at 960 x 720), a zero lens, and one
whose outer pixels get no ray.  The images are rendered in float64 through the Newton inverse of tests/lens_ref.py."""
import numpy as np

import depth_cases as dc
import lens_ref as lr
from cloud_cases import spec_of
from depth_cases import F32, F64, FLT, U16

PLUMB = (-0.3, 0.1, 1e-3, -5e-4)
NFOV = (5.07, 3.25, 0.0, 0.0, 0.166, 5.40, 4.96, 0.90)
ZERO = (0.0, 0.0, 0.0, 0.0)


def lens_of(k, **kw):
    from optimalmodulationds_amd.engine import depth_lens
    return depth_lens(k, **kw)


def partial_lens():
    """two rounds of the inverse: the outer pixels of the plumb-bob camera have not arrived within 0.01 pixels and get no ray"""
    return lens_of(PLUMB, iters=2)


LOOK = dc.pose_of(dc.LOOK_ALONG_X, (0.0, 0.0, 0.5))      # at (0, 0, 0.5), looking along world x


def camera(width=64, height=48, fmt=U16, step=1, pitch=0, pose=None, focal=None, z_max=4.0, centre=None):
    f = 40.0 * width / 64 if focal is None else focal
    cx, cy = ((width - 1) / 2 + 0.3, (height - 1) / 2 - 0.2) if centre is None else centre
    return dc.cam_of(width, height, f, f, cx, cy, LOOK if pose is None else pose, fmt, 0.001, 0.2, z_max, step, pitch)


# every camera shape of the issue's list: (name, width, height, format, step, pitch)
SHAPES = [("64x48", 64, 48, U16, 1, 0), ("67x50 f32", 67, 50, FLT, 1, 0), ("67x50 step 2", 67, 50, U16, 2, 0), ("61x47 step 2 f32", 61, 47, FLT, 2, 0),
          ("pitch 71", 67, 50, U16, 1, 71), ("3x5", 3, 5, U16, 1, 0), ("9x1", 9, 1, FLT, 1, 0), ("1x1", 1, 1, U16, 1, 0)]
LENSES = [("plumb", PLUMB, {}), ("nfov", NFOV, {}), ("zero", ZERO, {}), ("partial", PLUMB, dict(iters=2))]


def shape_camera(name):
    _, w, h, fmt, step, pitch = next(s for s in SHAPES if s[0] == name)
    # a tiny image keeps the focal length of the 64-wide one and lies off the optical axis, so that its pixels sit where the lens bends
    return camera(w, h, fmt, step, pitch, focal=40.0 if w < 16 else None, centre=(-20.3, -12.2) if w < 16 else None)


WALL_X = 1.6
BOX = dict(origin=(0.0, -1.6, -1.1), voxel=0.1, dims=(20, 32, 32))       # 20 480 cells: the wall, the sphere and the plane below


def as_image(cam, depth):
    """float64 depths [H, W] (0: no return) as the camera's format, laid out by its pitch -> (what to pass as the image, [H, W] view)"""
    h, w, pitch = int(cam.height), int(cam.width), int(cam.pitch) or int(cam.width)
    if cam.format == U16:
        img = dc.to_u16(depth, cam.depth_scale)
    else:
        img = np.where(depth > 0, depth, np.nan).astype(F32)
    flat = np.zeros((h - 1) * pitch + w, img.dtype)
    view = np.lib.stride_tricks.as_strided(flat, (h, w), (pitch * img.itemsize, img.itemsize))
    view[:] = img
    return view


def sphere_scene(cam, k, t=0.0):
    """a sphere of radius 0.25 m at (0.9, 0.1 + t, 0.5) in front of a wall at x = WALL_X"""
    return as_image(cam, lr.render(cam, k, spheres=[(0.9, 0.1 + t, 0.5, 0.25)], planes=[((1.0, 0.0, 0.0), WALL_X)]))


PLANE = (np.array([0.8, 0.6, 0.0]), 1.2)      # a tilted plane 0.8 x + 0.6 y = 1.2 in front of the camera


def plane_scene(cam, k):
    return as_image(cam, lr.render(cam, k, planes=[PLANE]))


def z_of(cam, view):
    """the depths the definition reads from an image, float64, NaN: no return"""
    if cam.format == U16:
        return np.where(view == 0, np.nan, view.astype(F32) * F32(cam.depth_scale)).astype(F64)
    return view.astype(F64)


def flat_of(cam, view):
    """the (H - 1) pitch + W elements behind a view that as_image made"""
    n = (int(cam.height) - 1) * (int(cam.pitch) or int(cam.width)) + int(cam.width)
    return np.lib.stride_tricks.as_strided(view, (n,), (view.itemsize,))
