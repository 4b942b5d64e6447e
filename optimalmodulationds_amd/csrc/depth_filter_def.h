// The DEFINITION of the depth filter (omds.h: omds_depth_points_filtered), stated once for the host entry points, the kernels
// k_depth_count_filt / k_depth_count_filt_rec of depth_kernels.hip and the stand-alone host build of tests/depth_filter_host.cpp.
// Like depth_def.h, which it builds on and leaves as it is: plain fp32, every operation of omds.h its own statement (one rounding
// each; the translation units that include this are compiled without contraction across statements), fmaf written out.
//   A visited pixel (ju, jv) that omds_depth_points keeps at depth z stays iff at least min_support OTHER pixels of its window of
//   (2 radius + 1)^2 visited pixels hold a return z_n with fabsf(z_n - z) <= tol, tol = fmaf(edge_rel, z, edge_abs).
//   - A neighbour is a RETURN, not a kept pixel: it is deliberately NOT range-gated.  A surface just beyond z_max (or nearer than
//     z_min) still supports the pixel beside it, for the same reason the scene memory's z_pix is not gated.
//   - A window position outside [0, nu) x [0, nv) gives no support: a corner pixel at radius 1 has 3 possible supporters, a border
//     pixel 5; an image smaller than the window has as many as it has other pixels.
//   - "No return" (U16 raw 0) and "outside the image" are both written as z_n = NaN, and an F32 NaN element is one already: NaN fails
//     the one comparison, which is the whole test for either format.
#pragma once
#include "depth_lens_def.h"

// an omds_depth_filter_spec behind its checks: what the kernels take by value
struct DepthFilter {
    int radius;             // 1 .. 3
    int min_support;        // 1 .. (2 radius + 1)^2 - 1
    float edge_abs, edge_rel;
};

constexpr int DEPTH_FILTER_MAX_RADIUS = 3;

inline int depth_filter_resolve(const omds_depth_filter_spec* s, DepthFilter* out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!s) return fail("depth filter: null filter spec");
    if (s->radius < 1 || s->radius > DEPTH_FILTER_MAX_RADIUS) return fail("depth filter: radius must be 1 .. 3");
    const int window = (2 * s->radius + 1) * (2 * s->radius + 1);
    if (s->min_support < 1 || s->min_support > window - 1) return fail("depth filter: min_support must be 1 .. (2 radius + 1)^2 - 1");
    if (!std::isfinite(s->edge_abs) || !(s->edge_abs >= 0.f)) return fail("depth filter: edge_abs must be finite and >= 0");
    if (!std::isfinite(s->edge_rel) || !(s->edge_rel >= 0.f)) return fail("depth filter: edge_rel must be finite and >= 0");
    out->radius = s->radius;
    out->min_support = s->min_support;
    out->edge_abs = s->edge_abs;
    out->edge_rel = s->edge_rel;
    return OMDS_OK;
}

// z_n of a raw element: NaN where a U16 element is no return
OMDS_CLOUD_FN float depth_filter_z_u16(const DepthCam& c, unsigned d) {
    float z;
    return depth_z_u16(c, d, &z) ? z : __builtin_nanf("");
}
// z_n of the element at index `at` of the image, whatever its format
OMDS_CLOUD_FN float depth_filter_z(const DepthCam& c, const void* image, long long at) {
    return c.format == OMDS_DEPTH_U16 ? depth_filter_z_u16(c, static_cast<const uint16_t*>(image)[at]) : static_cast<const float*>(image)[at];
}

// the verdict on a kept pixel at depth z.  z_n(a, b): the z_n of window position (a, b), NaN where it is outside the image.  `radius`
// is f.radius (the kernels pass it as a constant)
template <class At>
OMDS_CLOUD_FN bool depth_filter_keep(const DepthFilter& f, int radius, float z, const At& z_n) {
    const float tol = fmaf(f.edge_rel, z, f.edge_abs);
    int s = 0;
    for (int b = -radius; b <= radius; ++b)
        for (int a = -radius; a <= radius; ++a) {
            if (a == 0 && b == 0) continue;
            const float diff = z_n(a, b) - z;
            if (fabsf(diff) <= tol) ++s;
        }
    return s >= f.min_support;
}

// Visited pixel (iu, iv) of a host image: 0 = omds_depth_points drops it, 1 = kept (its point in w), 2 = kept there and rejected by the
// filter (w untouched).  f == nullptr: no filter.  rays (depth_lens_def.h: the table of the camera's lens; nullptr: no lens): the point
// lies on the pixel's ray, and 3 = kept by both but the pixel has no ray (w untouched)
inline int depth_filtered_pixel(const DepthCam& c, const DepthFilter* f, const void* image, int iu, int iv, float* w, const float* rays = nullptr) {
    const int u = iu * c.step, v = iv * c.step;
    const float z = depth_filter_z(c, image, (long long)v * c.pitch + u);
    if (!depth_gate(c, z)) return 0;   // NaN: a U16 0 fails here like every other value the gate drops
    if (f) {
        const bool keep = depth_filter_keep(*f, f->radius, z, [&](int a, int b) {
            const int x = iu + a, y = iv + b;
            if (x < 0 || x >= c.nu || y < 0 || y >= c.nv) return __builtin_nanf("");
            return depth_filter_z(c, image, (long long)y * c.step * c.pitch + (long long)x * c.step);
        });
        if (!keep) return 2;
    }
    if (rays) {
        const float* ab = rays + 2 * ((long long)iv * c.nu + iu);
        if (ab[0] != ab[0]) return 3;
        depth_point_ray(c, ab[0], ab[1], z, w);
        return 1;
    }
    depth_point(c, u, v, z, w);
    return 1;
}

// omds_depth_points_filtered without its argument messages.  filt == nullptr: depth_points_host, and *n_rejected_out (when given) = 0
inline int depth_points_filtered_host(const omds_depth_camera* cam, const omds_depth_filter_spec* filt, const void* image, float* xyz_out,
                                      int64_t cap_points, int64_t* n_valid_out, int64_t* n_rejected_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!filt) {
        const int rc = depth_points_host(cam, image, xyz_out, cap_points, n_valid_out, err);
        if (rc == OMDS_OK && n_rejected_out) *n_rejected_out = 0;
        return rc;
    }
    DepthCam c;
    DepthFilter f;
    if (int rc = depth_resolve_camera(cam, &c, err)) return rc;
    if (int rc = depth_filter_resolve(filt, &f, err)) return rc;
    if (!image || !xyz_out || !n_valid_out || !n_rejected_out) return fail("omds_depth_points_filtered: null image, xyz_out, n_valid_out or n_rejected_out");
    if (cap_points < depth_visited(c)) return fail("omds_depth_points_filtered: cap_points is smaller than the visited pixels, ceil(H / step) * ceil(W / step)");
    const float nan = std::nanf("");
    int64_t valid = 0, rejected = 0;
    float* out = xyz_out;
    for (int iv = 0; iv < c.nv; ++iv)
        for (int iu = 0; iu < c.nu; ++iu, out += 3) {
            const int what = depth_filtered_pixel(c, &f, image, iu, iv, out);
            if (what == 1) { ++valid; continue; }
            if (what == 2) ++rejected;
            out[0] = out[1] = out[2] = nan;
        }
    *n_valid_out = valid;
    *n_rejected_out = rejected;
    return OMDS_OK;
}

// omds_depth_points_lens without its argument messages: depth_points_filtered_host with xc = a z, yc = b z from the pixel's ray.  A
// pixel that passes the gate and the filter but has no ray is three NaNs, neither valid nor rejected.  lens == nullptr or model 0:
// depth_points_filtered_host itself
inline int depth_points_lens_host(const omds_depth_camera* cam, const omds_depth_lens* lens, const omds_depth_filter_spec* filt, const void* image,
                                  float* xyz_out, int64_t cap_points, int64_t* n_valid_out, int64_t* n_rejected_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    DepthLens l;
    if (int rc = depth_lens_resolve(lens, &l, err)) return rc;
    if (l.model == 0) return depth_points_filtered_host(cam, filt, image, xyz_out, cap_points, n_valid_out, n_rejected_out, err);
    DepthCam c;
    DepthFilter f;
    if (int rc = depth_resolve_camera(cam, &c, err)) return rc;
    if (filt)
        if (int rc = depth_filter_resolve(filt, &f, err)) return rc;
    if (!image || !xyz_out || !n_valid_out || (filt && !n_rejected_out))
        return fail("omds_depth_points_lens: null image, xyz_out or n_valid_out (with a filter: or n_rejected_out)");
    if (cap_points < depth_visited(c)) return fail("omds_depth_points_lens: cap_points is smaller than the visited pixels, ceil(H / step) * ceil(W / step)");
    std::vector<float> rays((size_t)depth_visited(c) * 2);
    float r2_max;
    int64_t n_invalid;
    depth_lens_table_host(c, cam->fx, cam->fy, l, rays.data(), &r2_max, &n_invalid);
    const float nan = std::nanf("");
    int64_t valid = 0, rejected = 0;
    float* out = xyz_out;
    for (int iv = 0; iv < c.nv; ++iv)
        for (int iu = 0; iu < c.nu; ++iu, out += 3) {
            const int what = depth_filtered_pixel(c, filt ? &f : nullptr, image, iu, iv, out, rays.data());
            if (what == 1) { ++valid; continue; }
            if (what == 2) ++rejected;
            out[0] = out[1] = out[2] = nan;
        }
    *n_valid_out = valid;
    if (n_rejected_out) *n_rejected_out = rejected;
    return OMDS_OK;
}
