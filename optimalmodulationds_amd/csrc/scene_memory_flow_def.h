// The DEFINITION of the depth route that keeps the scene memory AND the sphere velocities in one call (omds.h:
// omds_depth_scene_memory_flow), stated once for the host entry point, the kernels of scene_memory_kernels.hip (SeenSrc, k_scene_memory_flow)
// and the stand-alone host build of tests/scene_memory_flow_host.cpp.  It builds on scene_memory_def.h (the words), point_cloud_flow_def.h
// (the records and the per-cell velocities) and point_cloud_objects_def.h (the components and the object velocities) and leaves them
// as they are: it adds no arithmetic of its own, only which sphere keeps which result.
//   T, the SEEN SUBLIST: the final spheres whose cell was counted now (n[c] >= min_points), in cell order.  On T everything is what
//   the tracked / objects depth call gives on the same images and the same stored frame and table; the memory adds spheres around T.
#pragma once
#include "point_cloud_objects_def.h"
#include "scene_memory_def.h"

// THE RULE of the last step, per final sphere: true = the sphere stands still whatever the flow or an accepted object says -- velocity
// exactly +0, not matched, no object.  A sphere outside T is remembered: nothing was measured.  A sphere of T whose STORED word was
// >= 2 was occupied and unseen at the previous memory call: the previous frame has no record of it, and what the window search finds
// around it is its neighbours, not its past (the uncovered wall that "moves" one cell sideways).
OMDS_CLOUD_FN bool scene_memory_flow_still(bool seen_now, unsigned m_stored) { return !seen_now || m_stored >= 2u; }

// the points of the images of one frame, one after the other (a dropped pixel: three NaNs, which the records drop)
inline int scene_memory_flow_points(const omds_depth_filter_spec* filt, const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                    std::vector<float>& xyz, std::string* err, const omds_depth_lens* lenses = nullptr) {
    xyz.clear();
    for (int i = 0; i < n_cams; ++i) {
        DepthCam c;
        if (int rc = depth_resolve_camera(cams + i, &c, err)) return rc;
        const size_t at = xyz.size(), visited = (size_t)depth_visited(c);
        xyz.resize(at + visited * 3);
        int64_t valid = 0, rejected = 0;
        if (int rc = depth_points_lens_host(cams + i, lenses ? lenses + i : nullptr, filt, images[i], xyz.data() + at, (int64_t)visited, &valid, &rejected, err))
            return rc;
    }
    return OMDS_OK;
}

// the checks of one frame's cameras and images, before anything is written
inline int scene_memory_flow_check_frame(const omds_depth_camera* cams, const void* const* images, int32_t n_cams, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (n_cams < 1 || n_cams > OMDS_DEPTH_MAX_CAMERAS || !cams || !images)
        return fail("omds_depth_scene_memory_flow: need 1 <= n_cams <= 8 and non-null cams, images [n_cams] per frame");
    int64_t visited = 0;
    for (int i = 0; i < n_cams; ++i) {
        DepthCam c;
        if (int rc = depth_resolve_camera(cams + i, &c, err)) return rc;
        if (!images[i]) return fail("omds_depth_scene_memory_flow: a null image");
        visited += depth_visited(c);
    }
    if (visited > OMDS_CLOUD_MAX_POINTS) return fail("omds_depth_scene_memory_flow: more than 16 777 216 visited pixels in all");
    return OMDS_OK;
}

// omds_depth_scene_memory_flow[_lens] without its argument messages (lenses_prev [n_cams_prev], lenses [n_cams]: the lenses of
// depth_lens_def.h, nullptr: none).  A composition: scene_memory_lens_host for the words, depth_points[_filtered | _lens]
// for the points of both frames, cloud_objects_host / cloud_flow_cell_host on T, then the rule above per final sphere
inline int scene_memory_flow_host(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_cloud_track_spec* track,
                                  const omds_cloud_object_spec* obj, const omds_depth_filter_spec* filt, const omds_depth_camera* cams_prev,
                                  const void* const* images_prev, int32_t n_cams_prev, const uint8_t* keep_prev, const omds_depth_camera* cams,
                                  const void* const* images, int32_t n_cams, const uint8_t* keep_now, const uint32_t* mem_in, uint32_t* mem_out,
                                  int32_t* counts_out, float* xyzr_out, float* vel_out, int32_t* age_out, int32_t* label_out,
                                  int32_t* object_out, int32_t cap, int32_t* count_out, int32_t* n_matched_out, int32_t* n_objects_out,
                                  int32_t* n_objects_matched_out, std::string* err, const omds_depth_lens* lenses_prev = nullptr,
                                  const omds_depth_lens* lenses = nullptr) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    CloudGrid g;
    SceneMem sm;
    CloudTrack tr;
    CloudObjects ob{1, 1u};
    DepthFilter f;
    if (int rc = cloud_resolve_spec(spec, &g, err)) return rc;
    if (int rc = scene_memory_resolve(mem_spec, g, &sm, err)) return rc;
    if (int rc = cloud_resolve_track(track, &tr, err)) return rc;
    if (obj)
        if (int rc = cloud_resolve_objects(obj, &ob, err)) return rc;
    if (filt)
        if (int rc = depth_filter_resolve(filt, &f, err)) return rc;
    if (int rc = scene_memory_flow_check_frame(cams, images, n_cams, err)) return rc;
    const bool have_prev = cams_prev != nullptr;
    if (have_prev)
        if (int rc = scene_memory_flow_check_frame(cams_prev, images_prev, n_cams_prev, err)) return rc;
    if (!mem_out || !count_out) return fail("omds_depth_scene_memory_flow: null mem_out or count_out");
    if (cap < 0 || (cap > 0 && (!xyzr_out || !vel_out || !age_out || !label_out || !object_out)))
        return fail("omds_depth_scene_memory_flow: need cap >= 0 and non-null xyzr_out [cap,4], vel_out [cap,3], age_out, label_out, object_out [cap]");

    // 1, 2: the words, into a buffer of this call (mem_out may be mem_in, and a refusal below must leave it alone)
    std::vector<uint32_t> words((size_t)g.n_cells);
    int32_t counts[SCENE_MEM_COUNTS] = {0, 0, 0, 0, 0};
    if (int rc = scene_memory_lens_host(spec, mem_spec, filt, lenses, cams, images, n_cams, mem_in, words.data(), counts, err)) return rc;
    const int64_t candidates = (int64_t)counts[SCENE_MEM_SEEN] + counts[SCENE_MEM_REMEMBERED];
    if (candidates > g.max_spheres || candidates > cap) {
        *count_out = (int32_t)candidates;
        if (counts_out)
            for (int k = 0; k < SCENE_MEM_COUNTS; ++k) counts_out[k] = counts[k];
        return fail("omds_depth_scene_memory_flow: more seen and remembered cells than max_spheres (or cap); count_out holds their number");
    }
    // the self-filter's stand-in: a candidate it drops leaves the memory
    std::vector<int> final_cells;
    {
        size_t o = 0;
        for (int c = 0; c < g.n_cells; ++c) {
            if (words[(size_t)c] == 0u) continue;
            if (keep_now && !keep_now[o]) {
                words[(size_t)c] = 0u;
                ++counts[SCENE_MEM_FORGOTTEN];
            } else {
                final_cells.push_back(c);
            }
            ++o;
        }
    }
    // 3: T and what the tracked / objects call gives on it
    std::vector<float> xyz_now, xyz_prev;
    if (int rc = scene_memory_flow_points(filt, cams, images, n_cams, xyz_now, err, lenses)) return rc;
    if (have_prev)
        if (int rc = scene_memory_flow_points(filt, cams_prev, images_prev, n_cams_prev, xyz_prev, err, lenses_prev)) return rc;
    std::vector<uint32_t> now, prev;
    cloud_records_host(g, xyz_now.data(), (int64_t)(xyz_now.size() / 3), now);
    cloud_records_host(g, xyz_prev.data(), (int64_t)(xyz_prev.size() / 3), prev);
    std::vector<uint8_t> keep_seen;      // one flag per occupied cell of this frame: whether it is in the final list
    std::vector<int> seen_at;            // T: index into the final list
    for (size_t i = 0; i < final_cells.size(); ++i)
        if (now[(size_t)final_cells[i] * 4] >= g.min_points) seen_at.push_back((int)i);
    for (int c = 0; c < g.n_cells; ++c)
        if (now[(size_t)c * 4] >= g.min_points) keep_seen.push_back(words[(size_t)c] != 0u ? 1 : 0);
    const size_t n_seen = seen_at.size(), n_room = std::max(keep_seen.size(), (size_t)1);
    std::vector<float> t_xyzr(n_room * 4), t_vel(n_room * 3, 0.f);
    std::vector<int32_t> t_label(n_room, -1), t_object(n_room, 0);
    std::vector<uint8_t> t_matched(n_room, 0);
    int32_t n_objects = 0, n_accepted = 0;
    if (obj) {
        int32_t occupied = 0, matched = 0;
        // (the occupied cells are at most the candidates, which passed the refusal above)
        if (int rc = cloud_objects_host(spec, track, obj, xyz_prev.data(), (int64_t)(xyz_prev.size() / 3), keep_prev, xyz_now.data(),
                                        (int64_t)(xyz_now.size() / 3), keep_seen.data(), t_xyzr.data(), t_vel.data(), t_label.data(),
                                        t_object.data(), (int32_t)n_room, &occupied, &matched, &n_objects, &n_accepted, err))
            return rc;
    }
    for (size_t j = 0; j < n_seen; ++j) {
        const int c = final_cells[(size_t)seen_at[j]];
        float v[3];
        const bool found = have_prev && cloud_flow_cell_host(g, tr, &now[(size_t)c * 4], prev, c, v);
        if (obj && t_object[j]) {
            t_matched[j] = 1;            // an accepted object's sphere: cloud_objects_host left the object's velocity
        } else {
            t_matched[j] = found ? 1 : 0;
            for (int a = 0; a < 3; ++a) t_vel[3 * j + a] = found ? v[a] : 0.f;
        }
    }
    if (!have_prev)
        for (size_t j = 0; j < n_seen; ++j) t_object[j] = 0;
    // 4, 5: per final sphere, last
    int32_t matched = 0;
    size_t j = 0;
    for (size_t i = 0; i < final_cells.size(); ++i) {
        const int c = final_cells[i];
        const bool seen_now = j < n_seen && seen_at[j] == (int)i;
        const bool still = scene_memory_flow_still(seen_now, mem_in ? mem_in[c] : 0u);
        cloud_sphere(g, c, xyzr_out + 4 * i);
        age_out[i] = (int32_t)(words[(size_t)c] - 1u);
        for (int a = 0; a < 3; ++a) vel_out[3 * i + a] = still ? 0.f : t_vel[3 * j + a];
        label_out[i] = seen_now && obj ? t_label[j] : -1;
        object_out[i] = still ? 0 : t_object[j];
        matched += !still && t_matched[j];
        if (seen_now) ++j;
    }
    for (int c = 0; c < g.n_cells; ++c) mem_out[c] = words[(size_t)c];
    if (counts_out)
        for (int k = 0; k < SCENE_MEM_COUNTS; ++k) counts_out[k] = counts[k];
    *count_out = (int32_t)final_cells.size();
    if (n_matched_out) *n_matched_out = have_prev ? matched : -1;
    if (n_objects_out) *n_objects_out = obj ? n_objects : 0;
    if (n_objects_matched_out) *n_objects_matched_out = obj && have_prev ? n_accepted : -1;
    return OMDS_OK;
}
