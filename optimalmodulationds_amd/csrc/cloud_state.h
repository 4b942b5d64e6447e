// What a context keeps for the scene from a point cloud or from depth images (scene_cloud.hip): omds_ctx::cloud, and for the obstacle
// focus (obstacle_focus.hip): omds_ctx::focus.  Included by
// omds_internal.h behind DevBuf.  Every buffer is allocated at the first call of the route that needs it and grown with the spec: a
// route is a choice of flags over scene_from_cloud's one list of stages, and each flag reserves its own group of buffers.
#pragma once
#include <cstring>

#include "point_cloud_objects_def.h"
#include "scene_memory_def.h"
#include "velocity_filter_def.h"

// Two buffers, one of which holds what the last successful call stored while the other is written; commit() swaps them
template <class T>
struct Flip {
    DevBuf<T> buf[2];
    int stored = 0;
    DevBuf<T>& kept() { return buf[stored]; }
    DevBuf<T>& next() { return buf[1 - stored]; }
    void commit() { stored = 1 - stored; }
};

// the grid of the stored frame; the floats are compared bitwise
struct CloudFrameKey {
    bool have = false;            // a frame is stored (a tracked call succeeded since creation / omds_cloud_track_reset)
    float origin[3] = {0.f, 0.f, 0.f}, voxel = 0.f;
    int dims[3] = {0, 0, 0};
    unsigned min_points = 0;
    bool same(const CloudGrid& g) const {
        return have && std::memcmp(origin, &g.ox, 12) == 0 && std::memcmp(&voxel, &g.voxel, 4) == 0 && dims[0] == g.dx && dims[1] == g.dy &&
               dims[2] == g.dz && min_points == g.min_points;
    }
    void set(const CloudGrid& g) {
        have = true;
        std::memcpy(origin, &g.ox, 12);
        voxel = g.voxel;
        dims[0] = g.dx; dims[1] = g.dy; dims[2] = g.dz;
        min_points = g.min_points;
    }
};

// the object spec the stored component table was built under, and its rows
struct CloudTableKey {
    bool have = false;            // a table is stored: an objects call succeeded and no reset / plain tracked call came after it
    int link = 0;
    unsigned min_cells = 0;
    int n = 0;                    // components in the stored table
    bool same(const CloudObjects& ob) const { return have && link == ob.link && min_cells == ob.min_cells; }
    void set(const CloudObjects& ob, int n_comp) { have = true; link = ob.link; min_cells = ob.min_cells; n = n_comp; }
};

// the grid and the memory spec the stored scene memory was built under (omds_set_obstacles_from_depth_memory); floats bitwise
struct SceneMemKey {
    CloudFrameKey grid;           // grid.have: a memory is stored (a memory call succeeded since creation / omds_scene_memory_reset)
    int max_age = 0, footprint = 0;
    float clear_margin = 0.f;
    int n_cells = 0;
    bool same(const CloudGrid& g, const SceneMem& sm) const {
        return grid.same(g) && max_age == sm.max_age && footprint == sm.footprint && std::memcmp(&clear_margin, &sm.clear_margin, 4) == 0;
    }
    void set(const CloudGrid& g, const SceneMem& sm) {
        grid.set(g);
        max_age = sm.max_age; footprint = sm.footprint; clear_margin = sm.clear_margin;
        n_cells = g.n_cells;
    }
};

// the grid and the filter spec the stored velocity-filter state was built under (omds_set_velocity_filter); floats bitwise
struct VelFilterKey {
    CloudFrameKey grid;           // grid.have: a state is stored (a filtered call with a previous frame succeeded; nothing emptied it since)
    VelFilter f = {};
    int n_cells = 0;
    bool same(const CloudGrid& g, const VelFilter& o) const { return grid.same(g) && std::memcmp(&f, &o, sizeof(f)) == 0; }
    void set(const CloudGrid& g, const VelFilter& o) { grid.set(g); f = o; n_cells = g.n_cells; }
};

// One camera slot of the context's lenses (omds_set_depth_lenses) and the ray table built for it.  The table is a CACHE under a bitwise
// key of what a ray depends on -- the visited pixels, the intrinsics and the lens, never the pose or the image -- built by the first
// depth call that needs it and rebuilt only when the key changes; it outlives the lens being turned off and comes back into use when
// the same camera and lens return
struct DepthLensSlot {
    bool on = false;              // camera i of a depth call has this lens
    DepthLens lens = {};          // behind its checks, while on
    bool have = false;            // a table is stored, built under the key below
    int width = 0, height = 0, step = 0;
    float intr[4] = {0.f, 0.f, 0.f, 0.f};   // fx, fy, cx, cy
    DepthLens built = {};
    DevBuf<float> ab;             // [entries][2]
    int64_t entries = 0;          // nv * nu
    float r2_max = 0.f;           // ... fetched behind the build
    int64_t n_invalid = 0;
    bool same(const DepthCam& c, const float* k, const DepthLens& l) const {
        return have && width == c.width && height == c.height && step == c.step && std::memcmp(intr, k, 16) == 0 &&
               std::memcmp(&built, &l, sizeof(l)) == 0;
    }
};

// What a context keeps for the obstacle focus (obstacle_focus.hip): omds_ctx::focus.  While `on`, the scene in force is a subset of the
// MASTER stored here, and idx says which.  Every buffer is allocated at the first focus call and grown with the master.
struct FocusState {
    bool on = false;                  // set by omds_focus_obstacles, cleared by install_obstacles (every scene setter ends in it)
    int n_master = 0;
    bool moving = false;              // the master carried motion velocities (horizon mode 1)
    bool labelled = false;            // ... and the labels of an objects call
    DevBuf<float4> master;            // [n_master]
    DevBuf<float> vel;                // [n_master][3] while moving
    std::vector<float> h_master, h_vel;          // the same on the host (what omds_clear_obstacle_focus installs again)
    std::vector<int32_t> label, flag;            // [n_master] while labelled
    int obj_count = 0;
    std::vector<int32_t> idx;                    // [n_obs] master index of every sphere in force, ascending
    DevBuf<unsigned> keys, sums, res;            // [n_master], [compaction blocks + 1], [4]
    DevBuf<float4> kept;                         // [n_master] the emission: spheres,
    DevBuf<int> keptIdx;                         // ... their master indices
    DevBuf<float> keptVel;                       // ... and [n_master][3] their velocities
    // ... a focus along a path (omds_focus_obstacles_path), allocated at the first such call
    DevBuf<unsigned> best, pass, bars;           // [n_master] nearest key, [n_master] passed in some state, [chunk] the bar of every row
    DevBuf<float> time;                          // [n_states] lookahead + ahead of every state
};

struct CloudState {
    DevBuf<float> xyz;                // [P][3] the points of a host cloud
    DevBuf<unsigned char> depthImg;   // the host images of a depth call, one after the other, each from a multiple of 16 bytes on
    DevBuf<unsigned> count;           // [cells rounded up to whole compaction blocks] points per cell
    DevBuf<unsigned> sums;            // [compaction blocks + 1] occupied items per block, scanned in place; the last word: their total
    DevBuf<float4> cand;              // [max_spheres] candidate spheres in cell order
    DevBuf<float4> kept;              // [max_spheres] ... and those the self-filter keeps
    // ... tracked (omds_set_obstacles_from_cloud_tracked): per cell the record (n, s_x, s_y, s_z) of point_cloud_flow_def.h.  One of
    // the two buffers holds the stored frame, the other is counted into; a successful tracked call makes its own the stored one
    Flip<uint4> rec;                  // [cells rounded up to whole compaction blocks] each, allocated when first counted into
    CloudFrameKey frame;
    DevBuf<int> candCell;             // [max_spheres] cell index of every candidate, in step with cand
    DevBuf<int> keptCell;             // [max_spheres] ... and of every kept one
    DevBuf<float4> vel;               // [max_spheres] velocity of every final sphere; .w: 1 where its window was not empty (k_cloud_flow)
    // ... objects (omds_set_obstacles_from_cloud_objects): the components of the final list, point_cloud_objects_def.h
    DevBuf<int> slot;                 // [cells rounded up to whole compaction blocks] list index of every final sphere's cell, else -1
    DevBuf<int> parent;               // [max_spheres] the union-find; after the flatten the root (list index) of every sphere
    DevBuf<int> label;                // [max_spheres] label (smallest cell of the component) of every sphere
    DevBuf<int> object;               // [max_spheres] 1 where the sphere's component is an accepted object
    DevBuf<int> compOf;               // [max_spheres] at a root: the row of its component in the table
    DevBuf<unsigned long long> acc;   // [max_spheres][5] at a root: m, N, Q_x, Q_y, Q_z of its component
    Flip<CloudComp> table;            // [max_spheres] each, ascending labels; one of the two is the stored table
    CloudTableKey tab;
    DevBuf<float4> objVel;            // [max_spheres] per component: the object's velocity; .w: 0 no object, 1 object, 2 accepted
    std::vector<int32_t> obj_label, obj_flag;   // [n_obs] of the scene in force when the objects call installed it, else empty
    int obj_count = 0;                // its objects
    // ... scene memory (omds_set_obstacles_from_depth_memory[_tracked]: the memory flag of scene_from_cloud): per cell the word of
    // scene_memory_def.h.  One of the two buffers holds the stored memory, the other is written; a successful memory call makes its
    // own the stored one
    Flip<unsigned> mem;               // [cells rounded up to whole compaction blocks] each, allocated when first written
    SceneMemKey memKey;
    DevBuf<int> age;                  // [max_spheres] m' - 1 of every final sphere's cell
    DevBuf<unsigned> memCounts;       // [SCENE_MEM_COUNTS] seen, remembered, cleared, expired, self-forgotten of the call under way
    std::vector<int32_t> mem_age;     // [n_obs] of the scene in force when the memory call installed it (padding: -1), else empty
    // ... memory and tracked in one call (omds_set_obstacles_from_depth_memory_tracked; memory_velocities): the seen sublist T of the
    // final list, on which the tracked / objects stages run, and their results carried back to the whole list
    DevBuf<int> seenCell, seenIdx;    // [max_spheres] cell of every sphere of T; its index in the final list
    DevBuf<float4> velAll;            // [max_spheres] velocity of every final sphere behind scene_memory_flow_still; .w as vel's
    DevBuf<int> labelAll, objectAll;  // [max_spheres] ... its label (-1 outside T) and whether it moves with an accepted object
    // ... the depth filter (omds_set_depth_filter): context state that every depth call consults; no key of anything stored
    bool filter_on = false;
    DepthFilter filter = {};          // behind its checks, while filter_on
    DevBuf<unsigned> filtCounts;      // [2] pixels the filter kept and rejected in the call under way
    int64_t filter_stats[2] = {0, 0}; // ... of the last depth call that reached its counting pass; 0, 0 when no filter ran
    // ... the lenses (omds_set_depth_lenses): context state that every depth call consults; no key of anything stored
    DepthLensSlot lens[OMDS_DEPTH_MAX_CAMERAS];
    DevBuf<unsigned> lensRed;         // [2] the bits of r2_max and the pixels without a ray of the table being built
    // ... the velocity filter (omds_set_velocity_filter): context state that every velocity route consults, and per cell the record
    // (q_x, q_y, q_z, hits) of velocity_filter_def.h.  One of the two buffers holds the stored state, the other is written; a
    // successful filtered call with a previous frame makes its own the stored one.  A buffer is all zero outside the cells it last
    // held: those are listed beside it, and one launch empties them in front of the next write
    bool vfilter_on = false;
    VelFilter vfilter = {};           // behind its checks, while vfilter_on
    omds_velocity_filter_spec vfilter_spec = {};   // ... as it was given (omds_get_velocity_filter)
    Flip<int4> vstate;                // [cells] each, allocated (and cleared) when first written
    DevBuf<int> vcells[2];            // [max_spheres] the cells vstate.buf[side] last held,
    int vn[2] = {0, 0};               // ... and their number
    VelFilterKey vkey;
    DevBuf<VelPred> vpred;            // [max_spheres] the predecessor of every final sphere (k_vel_pred)
    DevBuf<unsigned long long> vgroup;   // [max_spheres][VEL_GROUP_ACC] at the list index of a label's cell: G_x, G_y, G_z, Gt of the group
    DevBuf<int> vgroupH;              // [max_spheres] ... and Gh, VEL_NO_HISTORY while no member has added
    DevBuf<float4> velOut;            // [max_spheres] the filtered velocity of every final sphere; .w as vel's
    DevBuf<unsigned> vcounts;         // [3] live spheres with history, restarts, groups with history of the call under way
    bool vf_have = false;             // the scene in force was installed by a filtered call:
    std::vector<float> vf_raw;        // ... [n_obs][3] its unfiltered velocities (padding: 0),
    std::vector<int32_t> vf_live;     // ... [n_obs] its matched flags
    int32_t vf_stats[3] = {0, 0, 0};  // ... and its counts

    void forget_tracking() { frame.have = false; tab.have = false; vkey.grid.have = false; }   // omds_cloud_track_reset
    // another setter installed the scene in force
    void forget_labels() { obj_label.clear(); obj_flag.clear(); mem_age.clear(); vf_have = false; }
};
