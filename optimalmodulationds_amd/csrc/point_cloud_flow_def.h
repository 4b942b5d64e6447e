// The DEFINITION of the sphere velocities of two successive point clouds (omds.h: omds_point_cloud_flow), stated once for the host
// entry point, the kernels of cloud_track_kernels.hip and the stand-alone host build of tests/cloud_flow_host.cpp.  Like point_cloud_def.h,
// which it builds on and leaves as it is: plain fp32, every operation of omds.h its own statement (one rounding each; the
// translation units that include this are compiled without contraction across statements), every sum an integer.
#pragma once
#include <algorithm>

#include "point_cloud_def.h"

constexpr int OMDS_CLOUD_MAX_REACH = 4;
constexpr unsigned OMDS_CLOUD_NO_MATCH = 0xffffffffu;   // "best d2" of an empty window

// omds_cloud_track_spec behind its checks
struct CloudTrack {
    int reach;        // 1 .. OMDS_CLOUD_MAX_REACH
    float dt_frame;   // finite, > 0
    float still;      // finite; <= 0: off
};

inline int cloud_resolve_track(const omds_cloud_track_spec* t, CloudTrack* out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!t) return fail("point cloud flow: null track spec");
    if (t->reach < 1 || t->reach > OMDS_CLOUD_MAX_REACH) return fail("point cloud flow: reach must be 1 .. 4 cells");
    if (!std::isfinite(t->dt_frame) || !(t->dt_frame > 0.f)) return fail("point cloud flow: dt_frame must be finite and > 0");
    if (!std::isfinite(t->still)) return fail("point cloud flow: still is not finite");
    out->reach = t->reach;
    out->dt_frame = t->dt_frame;
    out->still = t->still;
    return OMDS_OK;
}

// cloud_cell with the point's place inside its cell: k[c] = (int)((u_c - floorf(u_c)) * 256) in 0 .. 255.  The cell is cloud_cell's
// (the same expressions in the same order); k is written only for a kept point
OMDS_CLOUD_FN int cloud_cell_sub(const CloudGrid& g, float x, float y, float z, unsigned* k) {
    const float big = 3.402823466e+38f;
    if (!(fabsf(x) <= big) || !(fabsf(y) <= big) || !(fabsf(z) <= big)) return -1;
    const float ux = (x - g.ox) * g.inv, uy = (y - g.oy) * g.inv, uz = (z - g.oz) * g.inv;
    const float fx = floorf(ux), fy = floorf(uy), fz = floorf(uz);
    if (!(fx >= 0.f && fx < (float)g.dx && fy >= 0.f && fy < (float)g.dy && fz >= 0.f && fz < (float)g.dz)) return -1;
    const float rx = ux - fx, ry = uy - fy, rz = uz - fz;   // exact, in [0, 1)
    k[0] = (unsigned)(int)(rx * 256.0f);
    k[1] = (unsigned)(int)(ry * 256.0f);
    k[2] = (unsigned)(int)(rz * 256.0f);
    return ((int)fz * g.dy + (int)fy) * g.dx + (int)fx;
}

// What the window search of one NOW cell adds up, all integers: over the cells at the smallest d2 seen so far
struct CloudFlowSums {
    unsigned d2;              // the smallest d2, OMDS_CLOUD_NO_MATCH while the window is empty
    unsigned t;               // cells at that d2
    int A[3];                 // - sum of their offsets k_c
    unsigned long long P[3];  // sum of their s'_c
    unsigned long long N;     // sum of their n'
};

OMDS_CLOUD_FN void cloud_flow_clear(CloudFlowSums& a) {
    a.d2 = OMDS_CLOUD_NO_MATCH;
    a.t = 0u;
    a.N = 0ull;
    for (int c = 0; c < 3; ++c) { a.A[c] = 0; a.P[c] = 0ull; }
}

// one occupied PREVIOUS cell at offset (kx, ky, kz) with record (n', s')
OMDS_CLOUD_FN void cloud_flow_add(CloudFlowSums& a, int kx, int ky, int kz, unsigned n, unsigned sx, unsigned sy, unsigned sz) {
    const unsigned d2 = (unsigned)(kx * kx + ky * ky + kz * kz);
    if (d2 > a.d2) return;
    if (d2 < a.d2) { cloud_flow_clear(a); a.d2 = d2; }
    a.t += 1u;
    a.A[0] -= kx; a.A[1] -= ky; a.A[2] -= kz;
    a.P[0] += sx; a.P[1] += sy; a.P[2] += sz;
    a.N += n;
}

// the `still` rule on a finished velocity (shared with point_cloud_objects_def.h): a speed below the bar is exactly +0
OMDS_CLOUD_FN void cloud_flow_still(const CloudTrack& tr, float* v) {
    if (tr.still > 0.f) {
        const float xx = v[0] * v[0];
        const float s2 = fmaf(v[2], v[2], fmaf(v[1], v[1], xx));
        const float bar = tr.still * tr.still;
        if (s2 < bar) v[0] = v[1] = v[2] = 0.f;
    }
}

// the fp32 lines of the definition: the NOW record (n, s) and the sums of a non-empty window -> vel[3]
OMDS_CLOUD_FN void cloud_flow_velocity(const CloudGrid& g, const CloudTrack& tr, unsigned n, const unsigned* s, const CloudFlowSums& a,
                                       float* vel) {
    float v[3];
    for (int c = 0; c < 3; ++c) {
        const float whole = (float)a.A[c] / (float)a.t;
        const float now = (float)s[c] / (float)n;
        const float prev = (float)a.P[c] / (float)a.N;
        const float diff = now - prev;
        const float sub = diff * 0.00390625f;
        const float cells = whole + sub;
        const float metres = cells * g.voxel;
        v[c] = metres / tr.dt_frame;
    }
    cloud_flow_still(tr, v);
    vel[0] = v[0]; vel[1] = v[1]; vel[2] = v[2];
}

// the records of one frame: rec [n_cells][4] = (n, s_x, s_y, s_z)
inline void cloud_records_host(const CloudGrid& g, const float* xyz, int64_t n_points, std::vector<uint32_t>& rec) {
    rec.assign((size_t)g.n_cells * 4, 0u);
    for (int64_t i = 0; i < n_points; ++i) {
        unsigned k[3];
        const int cell = cloud_cell_sub(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], k);
        if (cell < 0) continue;
        uint32_t* r = &rec[(size_t)cell * 4];
        r[0] += 1u; r[1] += k[0]; r[2] += k[1]; r[3] += k[2];
    }
}

// the velocity of the occupied NOW cell c with record r against the PREVIOUS records: true when its window was not empty, else vel = 0
inline bool cloud_flow_cell_host(const CloudGrid& g, const CloudTrack& tr, const uint32_t* r, const std::vector<uint32_t>& prev, int c, float* vel) {
    const int ix = c % g.dx, iy = (c / g.dx) % g.dy, iz = c / (g.dx * g.dy);
    CloudFlowSums a;
    cloud_flow_clear(a);
    for (int z = std::max(iz - tr.reach, 0); z <= std::min(iz + tr.reach, g.dz - 1); ++z)
        for (int y = std::max(iy - tr.reach, 0); y <= std::min(iy + tr.reach, g.dy - 1); ++y)
            for (int x = std::max(ix - tr.reach, 0); x <= std::min(ix + tr.reach, g.dx - 1); ++x) {
                const uint32_t* p = &prev[((size_t)(z * g.dy + y) * g.dx + x) * 4];
                if (p[0] >= g.min_points) cloud_flow_add(a, x - ix, y - iy, z - iz, p[0], p[1], p[2], p[3]);
            }
    if (a.d2 == OMDS_CLOUD_NO_MATCH) {
        vel[0] = vel[1] = vel[2] = 0.f;
        return false;
    }
    cloud_flow_velocity(g, tr, r[0], r + 1, a, vel);
    return true;
}

// omds_point_cloud_flow without its argument messages
inline int cloud_flow_host(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const float* xyz_prev, int64_t n_prev,
                           const float* xyz_now, int64_t n_now, float* xyzr_out, float* vel_out, int32_t cap, int32_t* count_out,
                           int32_t* matched_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    CloudGrid g;
    CloudTrack tr;
    if (int rc = cloud_resolve_spec(spec, &g, err)) return rc;
    if (int rc = cloud_resolve_track(track, &tr, err)) return rc;
    if (!count_out || !matched_out) return fail("omds_point_cloud_flow: null count_out or matched_out");
    if (n_prev < 0 || n_prev > OMDS_CLOUD_MAX_POINTS || (n_prev > 0 && !xyz_prev) || n_now < 0 || n_now > OMDS_CLOUD_MAX_POINTS || (n_now > 0 && !xyz_now))
        return fail("omds_point_cloud_flow: need 0 <= n_prev, n_now <= 16 777 216 and non-null xyz_prev, xyz_now [P,3]");
    if (cap < 0 || (cap > 0 && (!xyzr_out || !vel_out))) return fail("omds_point_cloud_flow: need cap >= 0 and non-null xyzr_out [cap,4], vel_out [cap,3]");
    std::vector<uint32_t> now, prev;
    cloud_records_host(g, xyz_now, n_now, now);
    int64_t occupied = 0;
    for (int c = 0; c < g.n_cells; ++c) occupied += now[(size_t)c * 4] >= g.min_points;
    *count_out = (int32_t)occupied;
    if (occupied > g.max_spheres || occupied > cap) return fail("omds_point_cloud_flow: more occupied cells than max_spheres (or cap); count_out holds their number");
    cloud_records_host(g, xyz_prev, n_prev, prev);
    int32_t w = 0, matched = 0;
    for (int c = 0; c < g.n_cells; ++c) {
        const uint32_t* r = &now[(size_t)c * 4];
        if (r[0] < g.min_points) continue;
        cloud_sphere(g, c, xyzr_out + (size_t)4 * w);
        matched += cloud_flow_cell_host(g, tr, r, prev, c, vel_out + (size_t)3 * w++);
    }
    *matched_out = matched;
    return OMDS_OK;
}
