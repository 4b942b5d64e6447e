// The DEFINITION of the object velocities of two successive point clouds (omds.h: omds_point_cloud_object_flow), stated once for the
// host entry point, the kernels of cloud_track_kernels.hip and the stand-alone host build of tests/cloud_objects_host.cpp.  It builds on
// point_cloud_flow_def.h (the records, the per-cell fallback, the `still` rule): every sum an integer, the centroids and their
// distance in fp64 and the velocity in fp32 with every operation of omds.h its own statement (one rounding each; the translation
// units that include this are compiled without contraction across statements).
#pragma once
#include "point_cloud_flow_def.h"

constexpr int OMDS_CLOUD_MAX_LINK = 2;

// omds_cloud_object_spec behind its checks
struct CloudObjects {
    int link;             // 1 .. OMDS_CLOUD_MAX_LINK
    unsigned min_cells;   // >= 1
};

inline int cloud_resolve_objects(const omds_cloud_object_spec* o, CloudObjects* out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!o) return fail("point cloud objects: null object spec");
    if (o->link < 1 || o->link > OMDS_CLOUD_MAX_LINK) return fail("point cloud objects: link must be 1 .. 2 cells");
    out->link = o->link;
    out->min_cells = o->min_cells < 1 ? 1u : (unsigned)o->min_cells;
    return OMDS_OK;
}

// the record of one component, all integers: Q_c < 2^54 (i_c < 2^22, P <= 2^24 points)
struct CloudComp {
    int label;                // the smallest cell index of the component
    unsigned m;               // cells
    unsigned long long N;     // sum of their n
    unsigned long long Q[3];  // sum of 256 i_c n + s_c: the points' coordinates in 1/256 cell
};

// what the cell with index i_c on an axis and record (n, s_c) adds to Q_c
OMDS_CLOUD_FN unsigned long long cloud_comp_q(int i, unsigned n, unsigned s) { return 256ull * (unsigned long long)i * n + s; }

// The cells a cell links to that have a SMALLER index than its own: the lower half of its (2 link + 1)^3 window, clipped to the grid
// (at most 62); the upper half is the other cell's business.  visit(cell, implied) -> whether that cell is kept.  implied: a kept
// cell of the same row at most link cells to the left was visited just before -- the two are linked by the right one's own visit, so
// a union with this one adds nothing to the components (a dense scene needs 5 unions per cell instead of 13 at link 1, 13 of 62 at 2)
template <class F>
OMDS_CLOUD_FN void cloud_lower_neighbours(const CloudGrid& g, int link, int cell, F&& visit) {
    const int ix = cell % g.dx, iy = (cell / g.dx) % g.dy, iz = cell / (g.dx * g.dy);
    const int z0 = iz - link < 0 ? 0 : iz - link, y0 = iy - link < 0 ? 0 : iy - link, x0 = ix - link < 0 ? 0 : ix - link;
    const int y1 = iy + link > g.dy - 1 ? g.dy - 1 : iy + link, x1 = ix + link > g.dx - 1 ? g.dx - 1 : ix + link;
    for (int z = z0; z <= iz; ++z)
        for (int y = y0; y <= (z < iz ? y1 : iy); ++y) {
            int last = -2 * OMDS_CLOUD_MAX_LINK;   // x of the last kept cell of this row: none yet
            for (int x = x0; x <= x1; ++x) {
                const int j = (z * g.dy + y) * g.dx + x;
                if (j >= cell) break;
                if (visit(j, x - last <= link)) last = x;
            }
        }
}

// the centroid of a component in 1/256 cell: one conversion each, one division
OMDS_CLOUD_FN void cloud_comp_centroid(const CloudComp& c, double* cen) {
    const double n = (double)c.N;
    for (int a = 0; a < 3; ++a) {
        const double q = (double)c.Q[a];
        cen[a] = q / n;
    }
}

// squared distance of two centroids: three products and two sums
OMDS_CLOUD_FN double cloud_object_d2(const double* now, const double* prev) {
    const double dx = now[0] - prev[0];
    const double dy = now[1] - prev[1];
    const double dz = now[2] - prev[2];
    const double xx = dx * dx;
    const double yy = dy * dy;
    const double zz = dz * dz;
    const double xy = xx + yy;
    return xy + zz;
}

// the order of the candidates: the smaller d2, ties to the smaller label
OMDS_CLOUD_FN bool cloud_object_closer(double d2, int label, double best_d2, int best_label) {
    return d2 < best_d2 || (d2 == best_d2 && label < best_label);
}

// the two gates of a match: the centroid moved at most reach cells, and neither component has more than twice the other's cells
OMDS_CLOUD_FN bool cloud_object_accept(const CloudTrack& tr, unsigned m_now, unsigned m_prev, double d2) {
    const double bar = 256.0 * (double)tr.reach;
    const double bar2 = bar * bar;
    const unsigned long long lo = m_now < m_prev ? m_now : m_prev, hi = m_now < m_prev ? m_prev : m_now;
    return d2 <= bar2 && 2ull * lo >= hi;
}

// the velocity of an accepted object: the centroid's displacement (fp64) to cells (fp32), then the lines of cloud_flow_velocity
OMDS_CLOUD_FN void cloud_object_velocity(const CloudGrid& g, const CloudTrack& tr, const double* now, const double* prev, float* vel) {
    float v[3];
    for (int c = 0; c < 3; ++c) {
        const double d = now[c] - prev[c];
        const double scaled = d * 0.00390625;
        const float cells = (float)scaled;
        const float metres = cells * g.voxel;
        v[c] = metres / tr.dt_frame;
    }
    cloud_flow_still(tr, v);
    vel[0] = v[0]; vel[1] = v[1]; vel[2] = v[2];
}

// One NOW object against a PREVIOUS table (ascending labels): the candidate over the components of at least min_cells cells, the
// gates, the velocity.  True when the match is accepted.  The kernel strides the same statements over the lanes of a wave
inline bool cloud_object_match_host(const CloudGrid& g, const CloudTrack& tr, const CloudObjects& ob, const CloudComp& now,
                                    const std::vector<CloudComp>& prev, float* vel) {
    double cn[3], cp[3], best_d2 = 0.0;
    int best = -1;
    cloud_comp_centroid(now, cn);
    for (size_t j = 0; j < prev.size(); ++j) {
        if (prev[j].m < ob.min_cells) continue;
        cloud_comp_centroid(prev[j], cp);
        const double d2 = cloud_object_d2(cn, cp);
        if (best < 0 || cloud_object_closer(d2, prev[j].label, best_d2, prev[best].label)) { best = (int)j; best_d2 = d2; }
    }
    if (best < 0 || !cloud_object_accept(tr, now.m, prev[(size_t)best].m, best_d2)) return false;
    cloud_comp_centroid(prev[(size_t)best], cp);
    cloud_object_velocity(g, tr, cn, cp, vel);
    return true;
}

// The components of one frame over its kept cells: cells [S] ascending -> root [S] (list index of the component's smallest cell) and
// the table in ascending label order.  A union-find that hooks the larger root under the smaller, as the kernel does
inline void cloud_components_host(const CloudGrid& g, const CloudObjects& ob, const std::vector<uint32_t>& rec, const std::vector<int>& cells,
                                  std::vector<int>& root, std::vector<CloudComp>& table) {
    const int S = (int)cells.size();
    std::vector<int> slot((size_t)g.n_cells, -1), parent((size_t)S);
    for (int i = 0; i < S; ++i) { slot[(size_t)cells[(size_t)i]] = i; parent[(size_t)i] = i; }
    auto find = [&](int x) {
        while (parent[(size_t)x] != x) x = parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
        return x;
    };
    for (int i = 0; i < S; ++i)
        cloud_lower_neighbours(g, ob.link, cells[(size_t)i], [&](int cell, bool implied) {
            const int j = slot[(size_t)cell];
            if (j < 0) return false;
            if (implied) return true;
            const int a = find(i), b = find(j);
            if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);
            return true;
        });
    root.resize((size_t)S);
    std::vector<int> comp((size_t)S, -1);
    table.clear();
    for (int i = 0; i < S; ++i) {
        const int r = root[(size_t)i] = find(i);
        if (r == i) {   // a root comes before every other cell of its component
            comp[(size_t)i] = (int)table.size();
            table.push_back(CloudComp{cells[(size_t)i], 0u, 0ull, {0ull, 0ull, 0ull}});
        }
        const int cell = cells[(size_t)i];
        const int idx[3] = {cell % g.dx, (cell / g.dx) % g.dy, cell / (g.dx * g.dy)};
        const uint32_t* r4 = &rec[(size_t)cell * 4];
        CloudComp& c = table[(size_t)comp[(size_t)r]];
        c.m += 1u;
        c.N += r4[0];
        for (int a = 0; a < 3; ++a) c.Q[a] += cloud_comp_q(idx[a], r4[0], r4[1 + a]);
    }
}

// the kept occupied cells of a frame, ascending; keep [occupied cells] or NULL = all
inline void cloud_kept_cells_host(const CloudGrid& g, const std::vector<uint32_t>& rec, const uint8_t* keep, std::vector<int>& cells) {
    cells.clear();
    size_t o = 0;
    for (int c = 0; c < g.n_cells; ++c)
        if (rec[(size_t)c * 4] >= g.min_points) {
            if (!keep || keep[o]) cells.push_back(c);
            ++o;
        }
}

// omds_point_cloud_object_flow without its argument messages
inline int cloud_objects_host(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const omds_cloud_object_spec* obj,
                              const float* xyz_prev, int64_t n_prev, const uint8_t* keep_prev, const float* xyz_now, int64_t n_now,
                              const uint8_t* keep_now, float* xyzr_out, float* vel_out, int32_t* label_out, int32_t* object_out, int32_t cap,
                              int32_t* count_out, int32_t* matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    CloudGrid g;
    CloudTrack tr;
    CloudObjects ob;
    if (int rc = cloud_resolve_spec(spec, &g, err)) return rc;
    if (int rc = cloud_resolve_track(track, &tr, err)) return rc;
    if (int rc = cloud_resolve_objects(obj, &ob, err)) return rc;
    if (!count_out || !matched_out) return fail("omds_point_cloud_object_flow: null count_out or matched_out");
    if (n_prev < 0 || n_prev > OMDS_CLOUD_MAX_POINTS || (n_prev > 0 && !xyz_prev) || n_now < 0 || n_now > OMDS_CLOUD_MAX_POINTS || (n_now > 0 && !xyz_now))
        return fail("omds_point_cloud_object_flow: need 0 <= n_prev, n_now <= 16 777 216 and non-null xyz_prev, xyz_now [P,3]");
    if (cap < 0 || (cap > 0 && (!xyzr_out || !vel_out || !label_out || !object_out)))
        return fail("omds_point_cloud_object_flow: need cap >= 0 and non-null xyzr_out [cap,4], vel_out [cap,3], label_out, object_out [cap]");
    std::vector<uint32_t> now, prev;
    cloud_records_host(g, xyz_now, n_now, now);
    int64_t occupied = 0;
    for (int c = 0; c < g.n_cells; ++c) occupied += now[(size_t)c * 4] >= g.min_points;
    *count_out = (int32_t)occupied;
    if (occupied > g.max_spheres || occupied > cap)
        return fail("omds_point_cloud_object_flow: more occupied cells than max_spheres (or cap); count_out holds their number");
    cloud_records_host(g, xyz_prev, n_prev, prev);
    std::vector<int> cells_now, cells_prev, root_now, root_prev;
    std::vector<CloudComp> table_now, table_prev;
    cloud_kept_cells_host(g, now, keep_now, cells_now);
    cloud_kept_cells_host(g, prev, keep_prev, cells_prev);
    cloud_components_host(g, ob, now, cells_now, root_now, table_now);
    cloud_components_host(g, ob, prev, cells_prev, root_prev, table_prev);
    // one match per NOW object; comp_of[root] = its row in the table
    std::vector<int> comp_of(cells_now.size(), -1);
    std::vector<float> obj_vel(table_now.size() * 3, 0.f);
    std::vector<uint8_t> accepted(table_now.size(), 0);
    int32_t n_objects = 0, n_accepted = 0;
    for (size_t k = 0, i = 0; i < cells_now.size(); ++i)
        if (root_now[i] == (int)i) comp_of[i] = (int)k++;
    for (size_t k = 0; k < table_now.size(); ++k) {
        if (table_now[k].m < ob.min_cells) continue;
        ++n_objects;
        accepted[k] = cloud_object_match_host(g, tr, ob, table_now[k], table_prev, &obj_vel[k * 3]);
        n_accepted += accepted[k];
    }
    int32_t matched = 0;
    for (size_t i = 0; i < cells_now.size(); ++i) {
        const int c = cells_now[i], k = comp_of[(size_t)root_now[i]];
        cloud_sphere(g, c, xyzr_out + 4 * i);
        label_out[i] = table_now[(size_t)k].label;
        object_out[i] = accepted[(size_t)k];
        float* vel = vel_out + 3 * i;
        if (accepted[(size_t)k]) {
            for (int a = 0; a < 3; ++a) vel[a] = obj_vel[(size_t)k * 3 + a];
            ++matched;
        } else {
            matched += cloud_flow_cell_host(g, tr, &now[(size_t)c * 4], prev, c, vel);
        }
    }
    *matched_out = matched;
    if (n_objects_out) *n_objects_out = n_objects;
    if (n_objects_matched_out) *n_objects_matched_out = n_accepted;
    return OMDS_OK;
}
