// The DEFINITION of the velocity filter (omds.h: omds_velocity_filter_step), stated once for the host entry point, the kernels
// k_vel_pred / k_vel_group / k_vel_blend of velocity_filter_kernels.hip and the stand-alone host build of tests/velocity_filter_host.cpp.
// Like point_cloud_flow_def.h, which it builds on and leaves as it is: plain fp32, every operation of omds.h its own statement (one
// rounding each; the translation units that include this are compiled without contraction across statements), every sum an integer.
//   THE STATE: per grid cell four int32 (q_x, q_y, q_z, hits); hits == 0: no history; else q the smoothed velocity in 2^-16 m/s and
//   hits the frames behind it, saturating at 255.
//   1. the PREDECESSOR of a sphere: the state cells with hits >= 1 of its window (the track spec's reach) at the smallest d2, their q
//      added up (S, int64), their number t and the smallest of their hits h; an empty window: h = 0.
//   2. a GROUP (the live spheres that move with one accepted object) adds the predecessors of its members with h > 0 up: every member
//      then blends against (G, Gt, Gh), and since the members of an object share one raw velocity each receives the same one.
//   3. the BLEND of a live sphere: p = (S / t) 2^-16;  a = max(alpha, 1 / (h + 1)): a running mean over the first frames, so that the
//      filter converges at the rate of the data;  v = p + a (raw - p), unless |raw - p| exceeds max_jump: then the history restarts.
//   4. state_out[cell] = (rint(clamp(v, +-1024) 2^16), hits'); the output is v behind the still rule of the track spec.
#pragma once
#include <map>
#include <vector>

#include "point_cloud_flow_def.h"

constexpr int VEL_FILTER_MAX_HITS = 255;

// an omds_velocity_filter_spec behind its checks: what the kernels take by value.  Compared bitwise as part of the state's key
struct VelFilter {
    float alpha;          // (0, 1]
    float alpha_object;   // (0, 1]: the spec's, or alpha where the spec's is <= 0
    float max_jump;       // <= 0: no jump test
};

inline int velocity_filter_resolve(const omds_velocity_filter_spec* s, VelFilter* out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!s) return fail("velocity filter: null filter spec");
    if (!std::isfinite(s->alpha) || !(s->alpha > 0.f && s->alpha <= 1.f)) return fail("velocity filter: alpha must be in (0, 1]");
    if (std::isnan(s->alpha_object) || s->alpha_object > 1.f) return fail("velocity filter: alpha_object must be <= 0 (alpha) or in (0, 1]");
    if (std::isnan(s->max_jump)) return fail("velocity filter: max_jump is NaN");
    out->alpha = s->alpha;
    out->alpha_object = s->alpha_object > 0.f ? s->alpha_object : s->alpha;
    out->max_jump = s->max_jump;
    return OMDS_OK;
}

// What the window search of one sphere adds up over the state cells at the smallest d2 seen so far, all integers
struct VelPredSums {
    unsigned d2;          // OMDS_CLOUD_NO_MATCH while the window is empty
    long long S[3];       // sum of their q_c
    long long t;          // cells at that d2
    int h;                // the smallest of their hits; 0 while the window is empty
};

// ... and what k_vel_pred leaves per sphere for k_vel_group and k_vel_blend: 32 bytes
struct VelPred {
    long long S[3];
    int t, h;
};
constexpr int VEL_GROUP_ACC = 4;                // int64 words of a group's sums: G[3], Gt
constexpr int VEL_NO_HISTORY = 0x7fffffff;      // Gh while no member has added

OMDS_CLOUD_FN void vel_pred_clear(VelPredSums& a) {
    a.d2 = OMDS_CLOUD_NO_MATCH;
    a.t = 0;
    a.h = 0;
    for (int c = 0; c < 3; ++c) a.S[c] = 0;
}

// one state cell with history (hits >= 1) at offset (kx, ky, kz)
OMDS_CLOUD_FN void vel_pred_add(VelPredSums& a, int kx, int ky, int kz, int qx, int qy, int qz, int hits) {
    const unsigned d2 = (unsigned)(kx * kx + ky * ky + kz * kz);
    if (d2 > a.d2) return;
    if (d2 < a.d2) { vel_pred_clear(a); a.d2 = d2; }
    a.t += 1;
    a.S[0] += qx; a.S[1] += qy; a.S[2] += qz;
    a.h = a.h == 0 ? hits : (hits < a.h ? hits : a.h);
}

// the fp32 lines of a LIVE sphere: raw and the predecessor (S, t, h) it blends against -> v (in front of the still rule) and hits';
// true: the history restarted at the jump test
OMDS_CLOUD_FN bool vel_filter_blend(const VelFilter& f, bool grouped, const float* raw, const long long* S, long long t, int h, float* v,
                                    int* hits) {
    v[0] = raw[0]; v[1] = raw[1]; v[2] = raw[2];
    *hits = 1;
    if (h == 0) return false;
    float p[3], d[3];
    const float ft = (float)t;
    for (int c = 0; c < 3; ++c) {
        const float fs = (float)S[c];
        const float mean = fs / ft;
        p[c] = mean * 1.52587890625e-5f;
    }
    const float steps = (float)(h + 1);
    const float inv = 1.0f / steps;
    const float a = fmaxf(grouped ? f.alpha_object : f.alpha, inv);
    for (int c = 0; c < 3; ++c) d[c] = raw[c] - p[c];
    const float xx = d[0] * d[0];
    const float j2 = fmaf(d[2], d[2], fmaf(d[1], d[1], xx));
    const float bar = f.max_jump * f.max_jump;
    if (f.max_jump > 0.f && j2 > bar) return true;
    if (!(a >= 1.0f))
        for (int c = 0; c < 3; ++c) v[c] = fmaf(a, d[c], p[c]);
    *hits = h + 1 < VEL_FILTER_MAX_HITS ? h + 1 : VEL_FILTER_MAX_HITS;
    return false;
}

// the record a live sphere leaves at its cell
OMDS_CLOUD_FN void vel_filter_record(const float* v, int hits, int* rec) {
    for (int c = 0; c < 3; ++c) {
        const float lo = fmaxf(v[c], -1024.f);
        const float cl = fminf(lo, 1024.f);
        const float scaled = cl * 65536.0f;
        rec[c] = (int)rintf(scaled);
    }
    rec[3] = hits;
}

// the predecessor of the sphere in cell c on the host: the window over state [n_cells][4]
inline void vel_pred_host(const CloudGrid& g, int reach, const int32_t* state, int c, VelPredSums& a) {
    vel_pred_clear(a);
    if (!state) return;
    const int ix = c % g.dx, iy = (c / g.dx) % g.dy, iz = c / (g.dx * g.dy);
    for (int z = std::max(iz - reach, 0); z <= std::min(iz + reach, g.dz - 1); ++z)
        for (int y = std::max(iy - reach, 0); y <= std::min(iy + reach, g.dy - 1); ++y)
            for (int x = std::max(ix - reach, 0); x <= std::min(ix + reach, g.dx - 1); ++x) {
                const int32_t* q = &state[((size_t)(z * g.dy + y) * g.dx + x) * 4];
                if (q[3] >= 1) vel_pred_add(a, x - ix, y - iy, z - iz, q[0], q[1], q[2], q[3]);
            }
}

// omds_velocity_filter_step without its argument messages.  Every predecessor is taken before anything is written: state_in and
// state_out may be the same array
inline int velocity_filter_step_host(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const omds_velocity_filter_spec* filt,
                                     const int32_t* state_in, const int32_t* cell, const float* raw, const int32_t* live, const int32_t* group,
                                     int32_t n, float* vel_out, int32_t* state_out, int32_t* stats_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    CloudGrid g;
    CloudTrack tr;
    VelFilter f;
    if (int rc = cloud_resolve_spec(spec, &g, err)) return rc;
    if (int rc = cloud_resolve_track(track, &tr, err)) return rc;
    if (int rc = velocity_filter_resolve(filt, &f, err)) return rc;
    if (n < 0 || (n > 0 && (!cell || !raw || !vel_out))) return fail("omds_velocity_filter_step: need n >= 0 and non-null cell [n], raw [n,3], vel_out [n,3]");
    if (!state_out) return fail("omds_velocity_filter_step: null state_out [cells,4]");
    for (int32_t i = 0; i < n; ++i) {
        if (cell[i] < 0 || cell[i] >= g.n_cells || (i > 0 && cell[i] <= cell[i - 1]))
            return fail("omds_velocity_filter_step: cell [n] must be ascending and inside the grid");
        if (group && (group[i] < -1 || group[i] >= g.n_cells)) return fail("omds_velocity_filter_step: group [n] must be -1 or a cell of the grid");
    }
    struct Group { long long G[3] = {0, 0, 0}, Gt = 0; int Gh = 0; };
    std::vector<VelPredSums> pred((size_t)n);
    std::map<int32_t, Group> groups;
    for (int32_t i = 0; i < n; ++i) {
        VelPredSums& a = pred[(size_t)i];
        vel_pred_host(g, tr.reach, state_in, cell[i], a);
        if ((live && !live[i]) || !group || group[i] < 0 || a.h == 0) continue;
        Group& G = groups[group[i]];
        for (int c = 0; c < 3; ++c) G.G[c] += a.S[c];
        G.Gt += a.t;
        G.Gh = G.Gh == 0 ? a.h : std::min(G.Gh, a.h);
    }
    std::fill(state_out, state_out + (size_t)g.n_cells * 4, 0);
    int32_t with_history = 0, restarts = 0;
    const Group none;
    for (int32_t i = 0; i < n; ++i) {
        float* out = vel_out + (size_t)3 * i;
        out[0] = out[1] = out[2] = 0.f;
        if (live && !live[i]) continue;
        const VelPredSums& a = pred[(size_t)i];
        const bool grouped = group && group[i] >= 0;
        const Group* G = &none;
        if (grouped && groups.count(group[i])) G = &groups[group[i]];
        const int h = grouped ? G->Gh : a.h;
        float v[3];
        int hits;
        restarts += vel_filter_blend(f, grouped, raw + (size_t)3 * i, grouped ? G->G : a.S, grouped ? G->Gt : a.t, h, v, &hits);
        with_history += h > 0;
        vel_filter_record(v, hits, state_out + (size_t)cell[i] * 4);
        cloud_flow_still(tr, v);
        out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
    }
    if (stats_out) {
        stats_out[0] = with_history;
        stats_out[1] = restarts;
        stats_out[2] = (int32_t)groups.size();   // a group is entered at its first member with history
    }
    return OMDS_OK;
}
