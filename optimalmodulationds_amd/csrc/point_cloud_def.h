// The DEFINITION of the obstacle spheres of a depth point cloud (omds.h: omds_point_cloud_spheres), stated once for the host entry
// point, the kernels of cloud_kernels.hip and its sister files and the stand-alone host build of tests/cloud_host.cpp.  Nothing here needs a HIP header:
// every function is plain fp32 arithmetic in which each operation named in omds.h is one rounding (the translation units that
// include this are compiled without contraction across statements, csrc/Makefile).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "omds.h"

#if defined(__HIPCC__)
#define OMDS_CLOUD_FN __host__ __device__ inline
#else
#define OMDS_CLOUD_FN inline
#endif

constexpr int64_t OMDS_CLOUD_MAX_CELLS = (int64_t)1 << 22;
constexpr int64_t OMDS_CLOUD_MAX_POINTS = (int64_t)1 << 24;
constexpr int32_t OMDS_CLOUD_MAX_SPHERES = 65536;
constexpr int32_t OMDS_CLOUD_DEFAULT_SPHERES = 4096;

// an omds_cloud_spec with its defaults resolved: what the kernels take by value
struct CloudGrid {
    float ox, oy, oz;       // origin
    float voxel, inv;       // edge length and 1.0f / voxel (one division, on the host)
    float radius;           // the spec's, or 0.8660254f * voxel
    int dx, dy, dz;         // cells per axis
    unsigned min_points;    // >= 1
    int max_spheres;        // 1 .. OMDS_CLOUD_MAX_SPHERES
    int n_cells;            // dx * dy * dz
};

// the checks every entry point runs before it touches a device; fills *g and returns 0, or a message and OMDS_ERR_INVALID_ARG
inline int cloud_resolve_spec(const omds_cloud_spec* s, CloudGrid* g, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!s) return fail("point cloud: null spec");
    if (!(s->voxel > 0.f) || !std::isfinite(s->voxel)) return fail("point cloud: voxel must be a finite edge length > 0");
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(s->origin[c])) return fail("point cloud: origin is not finite");
        if (s->dims[c] < 1 || s->dims[c] > OMDS_CLOUD_MAX_CELLS) return fail("point cloud: dims must be >= 1 with a product <= 4 194 304");
    }
    const int64_t cells = (int64_t)s->dims[0] * s->dims[1] * s->dims[2];   // each factor <= 2^22: no overflow
    if (cells > OMDS_CLOUD_MAX_CELLS) return fail("point cloud: dims must be >= 1 with a product <= 4 194 304");
    if (s->max_spheres > OMDS_CLOUD_MAX_SPHERES) return fail("point cloud: max_spheres is at most 65 536");
    if (s->radius != s->radius) return fail("point cloud: radius is not a number");
    g->ox = s->origin[0]; g->oy = s->origin[1]; g->oz = s->origin[2];
    g->voxel = s->voxel;
    g->inv = 1.0f / s->voxel;
    g->radius = s->radius > 0.f ? s->radius : 0.8660254f * s->voxel;
    g->dx = s->dims[0]; g->dy = s->dims[1]; g->dz = s->dims[2];
    g->min_points = s->min_points < 1 ? 1u : (unsigned)s->min_points;
    g->max_spheres = s->max_spheres < 1 ? OMDS_CLOUD_DEFAULT_SPHERES : s->max_spheres;
    g->n_cells = (int)cells;
    return OMDS_OK;
}

// cell of a point, -1 when it is dropped: a coordinate that is not finite, or a cell index outside the grid (compared as floats,
// so that no out-of-range value is ever converted)
OMDS_CLOUD_FN int cloud_cell(const CloudGrid& g, float x, float y, float z) {
    const float big = 3.402823466e+38f;
    if (!(fabsf(x) <= big) || !(fabsf(y) <= big) || !(fabsf(z) <= big)) return -1;
    const float fx = floorf((x - g.ox) * g.inv), fy = floorf((y - g.oy) * g.inv), fz = floorf((z - g.oz) * g.inv);
    if (!(fx >= 0.f && fx < (float)g.dx && fy >= 0.f && fy < (float)g.dy && fz >= 0.f && fz < (float)g.dz)) return -1;
    return ((int)fz * g.dy + (int)fy) * g.dx + (int)fx;
}

// the sphere of a cell: its centre (one fmaf per axis) and the grid's radius
OMDS_CLOUD_FN void cloud_sphere(const CloudGrid& g, int cell, float* out4) {
    const int ix = cell % g.dx, iy = (cell / g.dx) % g.dy, iz = cell / (g.dx * g.dy);
    out4[0] = fmaf((float)ix + 0.5f, g.voxel, g.ox);
    out4[1] = fmaf((float)iy + 0.5f, g.voxel, g.oy);
    out4[2] = fmaf((float)iz + 0.5f, g.voxel, g.oz);
    out4[3] = g.radius;
}

// the self-filter's rule: a candidate whose link distance is at most the margin is the robot's own body; a NaN distance keeps it
OMDS_CLOUD_FN bool cloud_keep(float d, float self_margin) { return !(d <= self_margin); }

// omds_point_cloud_spheres without its argument messages: counts per cell, then the occupied cells in ascending cell order
inline int cloud_spheres_host(const omds_cloud_spec* spec, const float* xyz, int64_t n_points, float* xyzr_out, int32_t cap,
                              int32_t* count_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    CloudGrid g;
    if (int rc = cloud_resolve_spec(spec, &g, err)) return rc;
    if (!count_out) return fail("omds_point_cloud_spheres: null count_out");
    *count_out = 0;
    if (n_points < 0 || n_points > OMDS_CLOUD_MAX_POINTS || (n_points > 0 && !xyz)) return fail("omds_point_cloud_spheres: need 0 <= n_points <= 16 777 216 and a non-null xyz [P,3]");
    if (cap < 0 || (cap > 0 && !xyzr_out)) return fail("omds_point_cloud_spheres: need cap >= 0 and a non-null xyzr_out [cap,4]");
    std::vector<uint32_t> count((size_t)g.n_cells, 0u);
    for (int64_t i = 0; i < n_points; ++i) {
        const int cell = cloud_cell(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        if (cell >= 0) count[(size_t)cell]++;
    }
    int64_t occupied = 0;
    for (int c = 0; c < g.n_cells; ++c) occupied += count[(size_t)c] >= g.min_points;
    *count_out = (int32_t)occupied;
    if (occupied > g.max_spheres || occupied > cap) return fail("omds_point_cloud_spheres: more occupied cells than max_spheres (or cap); count_out holds their number");
    int32_t w = 0;
    for (int c = 0; c < g.n_cells; ++c)
        if (count[(size_t)c] >= g.min_points) cloud_sphere(g, c, xyzr_out + (size_t)4 * w++);
    return OMDS_OK;
}
