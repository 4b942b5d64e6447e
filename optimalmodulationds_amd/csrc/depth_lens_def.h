// The DEFINITION of the lens of a depth camera (omds.h: omds_depth_lens, omds_depth_lens_rays), stated once for the host entry points,
// the kernel k_depth_rays and the lens forms of the counting kernels and of k_scene_memory in depth_kernels.hip and scene_memory_kernels.hip, and the stand-alone
// host build of tests/depth_lens_host.cpp.  Like depth_def.h, which it builds on and leaves as it is: plain fp32, every operation of
// omds.h its own statement (one rounding each; the translation units that include this are compiled without contraction across
// statements), fmaf written out.  The quotients num / den and den / num are the IEEE-rounded ones on both sides, as 1.0f / zc is in
// scene_memory_def.h: no fast division, no reciprocal intrinsic.
//   The model is OpenCV's rational Brown-Conrady one, coefficients in OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6 (plumb-bob: k4 = k5 =
//   k6 = 0).  FORWARD, undistorted normalised (a, b) -> distorted (ad, bd), is closed form; the pixel is (fx ad + cx, fy bd + cy).
//   INVERSE, the ray of a visited pixel, is a fixed number of rounds of the fixed-point step followed by one forward evaluation that
//   decides whether the rounds arrived: a pixel whose ray did not converge has NO ray, stored as (NaN, NaN).
//   The ray of a pixel is a property of the camera, not of the frame: it depends on width, height, step, fx, fy, cx, cy and the lens,
//   never on the pose or the image.  depth_lens_rays is the table of a camera's visited pixels, row-major.
#pragma once
#include "depth_def.h"

// an omds_depth_lens behind its checks: what the kernels take by value.  model 0: no lens, pinhole arithmetic
struct DepthLens {
    int model;
    float k[8];             // k1 k2 p1 p2 k3 k4 k5 k6
    int iters;              // 1 .. 64
    float max_residual;     // pixels; finite, > 0
};

constexpr int DEPTH_LENS_ITERS = 20, DEPTH_LENS_MAX_ITERS = 64;
constexpr float DEPTH_LENS_RESIDUAL = 0.01f;

// lens == nullptr: no lens.  Values iters < 1 and max_residual <= 0 select the defaults
inline int depth_lens_resolve(const omds_depth_lens* l, DepthLens* out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    *out = DepthLens{0, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, DEPTH_LENS_ITERS, DEPTH_LENS_RESIDUAL};
    if (!l || l->model == 0) return OMDS_OK;
    if (l->model != 1) return fail("depth lens: model must be 0 (none) or 1 (rational Brown-Conrady)");
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(l->k[i])) return fail("depth lens: a coefficient is not finite");
    if (l->iters > DEPTH_LENS_MAX_ITERS) return fail("depth lens: iters must be <= 64 (< 1: the default, 20)");
    if (!std::isfinite(l->max_residual))
        return fail("depth lens: max_residual must be finite (<= 0: the default, 0.01 pixels)");
    out->model = 1;
    for (int i = 0; i < 8; ++i) out->k[i] = l->k[i];
    if (l->iters >= 1) out->iters = l->iters;
    if (l->max_residual > 0.f) out->max_residual = l->max_residual;
    return OMDS_OK;
}

// numerator and denominator of the radial factor at r2, in Horner form
OMDS_CLOUD_FN float depth_lens_num(const DepthLens& l, float r2) {
    const float h2 = fmaf(r2, l.k[4], l.k[1]);
    const float h1 = fmaf(r2, h2, l.k[0]);
    return fmaf(r2, h1, 1.0f);
}
OMDS_CLOUD_FN float depth_lens_den(const DepthLens& l, float r2) {
    const float h2 = fmaf(r2, l.k[7], l.k[6]);
    const float h1 = fmaf(r2, h2, l.k[5]);
    return fmaf(r2, h1, 1.0f);
}
// the tangential terms at (x, y): dx = 2 p1 x y + p2 (r2 + 2 x^2), dy = p1 (r2 + 2 y^2) + 2 p2 x y
OMDS_CLOUD_FN void depth_lens_tangential(const DepthLens& l, float x, float y, float r2, float* dx, float* dy) {
    const float xy = x * y;
    const float xx = x * x;
    const float yy = y * y;
    const float tx = fmaf(2.0f, xx, r2);
    const float ty = fmaf(2.0f, yy, r2);
    const float p1_2 = 2.0f * l.k[2];
    const float p2_2 = 2.0f * l.k[3];
    const float ex = l.k[3] * tx;
    const float ey = l.k[2] * ty;
    *dx = fmaf(p1_2, xy, ex);
    *dy = fmaf(p2_2, xy, ey);
}
OMDS_CLOUD_FN float depth_lens_r2(float a, float b) {
    const float bb = b * b;
    return fmaf(a, a, bb);
}

// FORWARD: (a, b) -> (ad, bd); returns the radial factor s
OMDS_CLOUD_FN float depth_lens_forward(const DepthLens& l, float a, float b, float* ad, float* bd) {
    const float r2 = depth_lens_r2(a, b);
    const float num = depth_lens_num(l, r2);
    const float den = depth_lens_den(l, r2);
    const float s = num / den;
    float dx, dy;
    depth_lens_tangential(l, a, b, r2, &dx, &dy);
    *ad = fmaf(a, s, dx);
    *bd = fmaf(b, s, dy);
    return s;
}

// INVERSE: the ray (a, b) of pixel (u, v); false: the pixel has no ray, and (a, b) = (NaN, NaN).  fx, fy are the camera's (DepthCam
// keeps their reciprocals only)
OMDS_CLOUD_FN bool depth_lens_ray(const DepthCam& c, float fx, float fy, const DepthLens& l, int u, int v, float* a, float* b) {
    const float x0 = ((float)u - c.cx) * c.ifx;
    const float y0 = ((float)v - c.cy) * c.ify;
    float x = x0, y = y0;
    for (int i = 0; i < l.iters; ++i) {
        const float r2 = depth_lens_r2(x, y);
        const float num = depth_lens_num(l, r2);
        const float den = depth_lens_den(l, r2);
        const float ic = den / num;
        float dx, dy;
        depth_lens_tangential(l, x, y, r2, &dx, &dy);
        const float ex = x0 - dx;
        const float ey = y0 - dy;
        x = ex * ic;
        y = ey * ic;
    }
    float ad, bd;
    const float s = depth_lens_forward(l, x, y, &ad, &bd);
    const float qx = ad - x0;
    const float qy = bd - y0;
    const float rx = qx * fx;
    const float ry = qy * fy;
    const bool ok = s > 0.f && fabsf(rx) <= l.max_residual && fabsf(ry) <= l.max_residual;   // NaN fails the comparisons
    *a = ok ? x : __builtin_nanf("");
    *b = ok ? y : __builtin_nanf("");
    return ok;
}

// the point at depth z along the ray (a, b), in the frame of the voxel grid: depth_point with the ray in place of the pinhole one
OMDS_CLOUD_FN void depth_point_ray(const DepthCam& c, float a, float b, float z, float* w) {
    const float xc = a * z;
    const float yc = b * z;
    for (int r = 0; r < 3; ++r)
        w[r] = fmaf(c.pose[4 * r], xc, fmaf(c.pose[4 * r + 1], yc, fmaf(c.pose[4 * r + 2], z, c.pose[4 * r + 3])));
}

// what a memory verdict needs of a camera's lens: ab == nullptr: no lens, pinhole arithmetic.  Also the entry of the by-value lens
// table the lens forms of the counting kernels take (they read ab alone)
struct DepthLensCam {
    DepthLens lens;
    float r2_max;           // the largest fmaf(a, a, b * b) over the valid rays of the table: beyond it the polynomial may fold back
    const float* ab;        // [nv * nu][2] the table, row-major over the visited pixels
};
struct DepthLensTable {
    DepthLensCam cam[OMDS_DEPTH_MAX_CAMERAS];
};

// the table of camera c under lens l: ab [nv * nu][2], its r2_max and the number of pixels without a ray.  A loop on the host; on the
// device (k_depth_rays) the maximum is an integer one on the floats' bits, which are non-negative and therefore order preserving
inline void depth_lens_table_host(const DepthCam& c, float fx, float fy, const DepthLens& l, float* ab, float* r2_max, int64_t* n_invalid) {
    float most = 0.f;
    int64_t invalid = 0;
    float* out = ab;
    for (int iv = 0; iv < c.nv; ++iv)
        for (int iu = 0; iu < c.nu; ++iu, out += 2) {
            if (!depth_lens_ray(c, fx, fy, l, iu * c.step, iv * c.step, out, out + 1)) { ++invalid; continue; }
            const float r2 = depth_lens_r2(out[0], out[1]);
            if (r2 > most) most = r2;
        }
    *r2_max = most;
    *n_invalid = invalid;
}

// omds_depth_lens_rays without its argument messages.  lens == nullptr or model 0: the pinhole rays, every one valid
inline int depth_lens_rays_host(const omds_depth_camera* cam, const omds_depth_lens* lens, float* ab_out, float* r2_max_out, int64_t* n_invalid_out,
                                std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    DepthCam c;
    DepthLens l;
    if (int rc = depth_resolve_camera(cam, &c, err)) return rc;
    if (int rc = depth_lens_resolve(lens, &l, err)) return rc;
    if (!ab_out) return fail("omds_depth_lens_rays: null ab_out");
    float r2_max = 0.f;
    int64_t n_invalid = 0;
    depth_lens_table_host(c, cam->fx, cam->fy, l, ab_out, &r2_max, &n_invalid);
    if (r2_max_out) *r2_max_out = r2_max;
    if (n_invalid_out) *n_invalid_out = n_invalid;
    return OMDS_OK;
}
