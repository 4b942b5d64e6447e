// The DEFINITION of the points of a depth image (omds.h: omds_depth_points), stated once for the host entry point, the kernels
// k_depth_count / k_depth_count_rec of depth_kernels.hip and the stand-alone host build of tests/depth_host.cpp.  Like
// point_cloud_def.h, which it builds on and leaves as it is: plain fp32, every operation of omds.h its own statement (one rounding
// each; the translation units that include this are compiled without contraction across statements), fmaf written out.
#pragma once
#include "point_cloud_def.h"

// an omds_depth_camera behind its checks: what the kernels take by value
struct DepthCam {
    int width, height;      // pixels
    long long pitch;        // elements between row starts (the camera's, or width)
    int format;             // OMDS_DEPTH_U16 | OMDS_DEPTH_F32
    int step;               // >= 1
    int nu, nv;             // visited columns and rows: ceil(width / step), ceil(height / step)
    float cx, cy;
    float ifx, ify;         // 1.0f / fx, 1.0f / fy (one division each, on the host)
    float depth_scale;
    float z_min, z_max;
    float pose[12];
};

inline int depth_resolve_camera(const omds_depth_camera* c, DepthCam* out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!c) return fail("depth image: null camera");
    if (c->width < 1 || c->height < 1) return fail("depth image: width and height must be >= 1");
    if (c->pitch != 0 && c->pitch < c->width) return fail("depth image: pitch must be 0 (= width) or >= width, in elements");
    if (c->format != OMDS_DEPTH_U16 && c->format != OMDS_DEPTH_F32) return fail("depth image: format must be 0 (uint16 raw units) or 1 (float32 metres)");
    if (!std::isfinite(c->fx) || !std::isfinite(c->fy) || c->fx == 0.f || c->fy == 0.f) return fail("depth image: fx and fy must be finite and != 0");
    if (!std::isfinite(c->cx) || !std::isfinite(c->cy)) return fail("depth image: cx and cy must be finite");
    if (c->format == OMDS_DEPTH_U16 && (!std::isfinite(c->depth_scale) || !(c->depth_scale > 0.f)))
        return fail("depth image: depth_scale must be finite and > 0");
    if (!std::isfinite(c->z_min) || !std::isfinite(c->z_max) || !(c->z_min > 0.f) || !(c->z_min <= c->z_max))
        return fail("depth image: need 0 < z_min <= z_max, both finite");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(c->pose[i])) return fail("depth image: pose is not finite");
    out->width = c->width; out->height = c->height;
    out->pitch = c->pitch == 0 ? c->width : c->pitch;
    out->format = c->format;
    out->step = c->step < 1 ? 1 : c->step;
    out->nu = (int)(((long long)c->width + out->step - 1) / out->step);
    out->nv = (int)(((long long)c->height + out->step - 1) / out->step);
    out->cx = c->cx; out->cy = c->cy;
    out->ifx = 1.0f / c->fx;
    out->ify = 1.0f / c->fy;
    out->depth_scale = c->depth_scale;
    out->z_min = c->z_min; out->z_max = c->z_max;
    for (int i = 0; i < 12; ++i) out->pose[i] = c->pose[i];
    return OMDS_OK;
}

inline int64_t depth_visited(const DepthCam& c) { return (int64_t)c.nu * c.nv; }

// elements of the image that the definition may read: the last visited row ends the buffer
inline int64_t depth_extent(const DepthCam& c) { return (int64_t)(c.height - 1) * c.pitch + c.width; }

// depth along the optical axis of a raw U16 value; false: no return
OMDS_CLOUD_FN bool depth_z_u16(const DepthCam& c, unsigned d, float* z) {
    if (d == 0u) return false;
    *z = (float)d * c.depth_scale;
    return true;
}

// the range gate: NaN, +-inf, negative values and -0 fail by the comparison
OMDS_CLOUD_FN bool depth_gate(const DepthCam& c, float z) { return z >= c.z_min && z <= c.z_max; }

// the point of pixel (u, v) at depth z in the frame of the voxel grid
OMDS_CLOUD_FN void depth_point(const DepthCam& c, int u, int v, float z, float* w) {
    const float a = ((float)u - c.cx) * c.ifx;
    const float b = ((float)v - c.cy) * c.ify;
    const float xc = a * z;
    const float yc = b * z;
    for (int r = 0; r < 3; ++r)
        w[r] = fmaf(c.pose[4 * r], xc, fmaf(c.pose[4 * r + 1], yc, fmaf(c.pose[4 * r + 2], z, c.pose[4 * r + 3])));
}

// one raw element -> kept or not, and its point
OMDS_CLOUD_FN bool depth_pixel_u16(const DepthCam& c, int u, int v, unsigned d, float* w) {
    float z;
    if (!depth_z_u16(c, d, &z) || !depth_gate(c, z)) return false;
    depth_point(c, u, v, z, w);
    return true;
}
OMDS_CLOUD_FN bool depth_pixel_f32(const DepthCam& c, int u, int v, float z, float* w) {
    if (!depth_gate(c, z)) return false;
    depth_point(c, u, v, z, w);
    return true;
}

// omds_depth_points without its argument messages
inline int depth_points_host(const omds_depth_camera* cam, const void* image, float* xyz_out, int64_t cap_points, int64_t* n_valid_out,
                             std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    DepthCam c;
    if (int rc = depth_resolve_camera(cam, &c, err)) return rc;
    if (!image || !xyz_out || !n_valid_out) return fail("omds_depth_points: null image, xyz_out or n_valid_out");
    if (cap_points < depth_visited(c)) return fail("omds_depth_points: cap_points is smaller than the visited pixels, ceil(H / step) * ceil(W / step)");
    const float nan = std::nanf("");
    int64_t valid = 0;
    float* out = xyz_out;
    for (int iv = 0; iv < c.nv; ++iv) {
        const int v = iv * c.step;
        const int64_t row = (int64_t)v * c.pitch;
        for (int iu = 0; iu < c.nu; ++iu, out += 3) {
            const int u = iu * c.step;
            const bool kept = c.format == OMDS_DEPTH_U16 ? depth_pixel_u16(c, u, v, static_cast<const uint16_t*>(image)[row + u], out)
                                                         : depth_pixel_f32(c, u, v, static_cast<const float*>(image)[row + u], out);
            if (kept) ++valid;
            else out[0] = out[1] = out[2] = nan;
        }
    }
    *n_valid_out = valid;
    return OMDS_OK;
}
