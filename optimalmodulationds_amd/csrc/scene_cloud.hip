// The scene from a depth point cloud or from depth images (omds.h: omds_set_obstacles_from_cloud[_tracked|_objects],
// omds_set_obstacles_from_depth[_memory[_tracked]], omds_set_depth_filter), as host stages over the launchers of cloud_kernels.h; the state between calls is omds_ctx::cloud
// (cloud_state.h).  One body, scene_from_cloud, for every route: it alone says which stage follows which, one flag per line.  A route is
// a choice of four things (CloudCall): tracked or not, objects or not (objects need tracked), the scene memory or not (memory needs
// the images), and where the points come from.
//   plain   : count per cell -> ordered compaction of the occupied cells -> the robot self-filter as ONE fp32 pass-1 launch over one
//             state with the candidates as its obstacle rows, and a second compaction of those it keeps -> the final list to the host
//             (a few thousand x 16 bytes) and in through install_obstacles, the body of omds_set_obstacles (context.hip)
//   tracked : the same steps in the same order on the record buffer that is NOT the stored frame, the cell indices carried through both
//             compactions, then the velocities of the final list against the stored frame, in through omds_set_obstacle_motion
//   objects : the tracked one with the components of the final list, into the table that is NOT the stored one, their match against
//             the stored table and the object velocities over the spheres', between the velocities and the install
//   depth   : any of the three with the images of up to eight cameras as the point source: no point is ever written
//   memory  : the plain depth route with one word per cell kept between calls: occluded cells stay, cells a camera looked through
//             leave.  k_scene_memory, into the buffer that is NOT the stored memory, stands between the counting pass and the
//             compaction, which is then of the words that are not 0; the cells the self-filter drops leave the memory; the ages
//   memory + tracked / objects : both in one call (the definition: scene_memory_flow_def.h).  ONE counting pass, into records, and
//             ONE staging copy serve both halves: the memory's words out of the records' counts, and the tracked / objects stages
//             on T, the spheres of the final list whose cell was counted now, carried back to the whole list by one launch
//   filter  : while the context has a depth filter, the counting pass of every depth call above is the filtered one
//             (depth_filter_def.h): another kernel in the same place, and two counters fetched behind it
//   lens    : while the context has lenses (depth_lens_def.h), a depth call in which some camera has one stages that camera's ray table
//             (a cache of the context, built by k_depth_rays when its key changes) beside the images, and its counting pass and its
//             memory pass are the lens forms of the same kernels; a call in which no camera has one enqueues what it always did
//   smoothed: while the context has a velocity filter, every tracked route above blends its velocities against the state kept per
//             cell (velocity_filter_def.h): one stage between the velocity stages and the install, which run unchanged
#include "capi_internal.h"
#include "cloud_kernels.h"

namespace {

// Where the points of a call come from: an array xyz [n_points][3] (host or device), or the depth images of up to eight cameras
struct DepthSource {
    DepthCam cam[OMDS_DEPTH_MAX_CAMERAS];   // behind their checks
    const void* const* images;
    int n_cams;
    int on_device;
    const DepthFilter* filt;                // the context's depth filter while it is on, else nullptr
    float intr[OMDS_DEPTH_MAX_CAMERAS][4];  // fx, fy, cx, cy as the caller gave them (cam keeps 1 / fx and 1 / fy): the key of a ray table
    bool lensed;                            // some camera of the call has a lens of the context's
};
struct PointSource {
    const float* xyz;
    int64_t n_points;
    int xyz_on_device;
};

// every pointer of the caller's that a call may write: five counts, and counts [5], the cells of a memory call in place of
// n_occupied.  A route leaves those of the routes above it alone
struct CloudOuts {
    int32_t *n_spheres, *n_occupied, *n_matched, *n_objects, *n_objects_matched, *counts;
};

// One call behind the checks of its specs: the route and the caller's pointers
struct CloudCall {
    const char* who;
    const omds_cloud_spec* spec;
    CloudGrid g;
    bool tracked, objects, memory, images;   // images: the points are those of depth, not of src
    CloudTrack tr;      // while tracked
    CloudObjects ob;    // while objects
    SceneMem sm;        // while memory,
    SceneMemCams ks;    // ... and what its verdicts need of depth's cameras
    PointSource src;
    DepthSource depth;
    const float* q_now;
    CloudOuts out;
    const VelFilter* vfilt = nullptr;   // while tracked: the context's velocity filter while it is on
    const DepthFilter* filter() const { return images ? depth.filt : nullptr; }
};

// What the stages of one call hand on
struct CloudWork {
    const float* d_xyz = nullptr;   // the points on the device, or
    DepthTable depth;               // ... the camera table of a depth call,
    DepthLensTable lens;            // ... and while depth.lensed the lens table beside it
    int occupied = 0;               // cells with min_points points and more
    const float4* d_list = nullptr; // the final list so far: the candidates, behind the self-filter those it keeps
    const int* d_cell = nullptr;    // tracked or memory: the cell of every sphere of d_list, else nullptr
    const float4* d_vel = nullptr;  // where install_scene fetches the velocities of d_list from; nullptr: cloud.vel
    int n_list = 0, n_final = 0;    // spheres of d_list; of the installed scene (filled up to n_closest)
    bool have_prev = false, have_table = false;   // there is a stored frame on this grid; and a stored table under this object spec
    int n_comp = 0, matched = 0;
    unsigned filt_counts[2] = {0u, 0u};           // pixels the depth filter kept and rejected, fetched behind the counting pass
    std::vector<float> vel4, obj_vel;             // [n_list][4] of cloud.vel, [n_comp][4] of cloud.objVel
    std::vector<int32_t> label, object;           // [n_final]
    const unsigned* mem_stored = nullptr;         // memory: the stored words while they are of this grid and memory spec, else nullptr:
                                                  // from empty memory, and whatever is stored stays until the commit
    unsigned counts[SCENE_MEM_COUNTS] = {0u, 0u, 0u, 0u, 0u};   // ... the cells of this call, the last fetched behind the self-filter
    std::vector<int32_t> age;                     // ... [n_final], padding spheres: -1
    std::vector<float> raw4;                      // velocity filter: [n_list][4] the velocities in front of it (vel4 holds the filtered ones)
    unsigned vcounts[3] = {0u, 0u, 0u};           // ... spheres with history, restarts, groups with history, fetched with the velocities
};

// spec, then track when the route is tracked, then obj when it has objects: each behind its checks, in that order
int resolve_call(omds_ctx* ctx, const char* who, const omds_cloud_spec* spec, bool tracked, const omds_cloud_track_spec* track, bool objects,
                 const omds_cloud_object_spec* obj, CloudCall* c) {
    *c = CloudCall{who, spec, CloudGrid{}, tracked, objects};
    if (int rc = cloud_resolve_spec(spec, &c->g, &ctx->err)) return rc;
    REQUIRE(!objects || tracked, OMDS_ERR_INVALID_ARG, std::string(who) + ": an object spec needs a track spec (the objects route is a tracked one)");
    if (tracked)
        if (int rc = cloud_resolve_track(track, &c->tr, &ctx->err)) return rc;
    if (objects)
        if (int rc = cloud_resolve_objects(obj, &c->ob, &ctx->err)) return rc;
    if (tracked && ctx->cloud.vfilter_on) c->vfilt = &ctx->cloud.vfilter;
    return OMDS_OK;
}

// ---- reserve: one function per group of buffers.  A group that has a buffer too small synchronises the stream first (enqueued work
// may still read what a reallocation frees); reserve() leaves a buffer that is large enough alone
int reserve_base(omds_ctx* ctx, const CloudCall& c) {
    CloudState& s = ctx->cloud;
    const size_t cells = c.tracked ? 0 : cloud_padded_cells(c.g), m = (size_t)c.g.max_spheres;   // a tracked call counts into records
    if (s.count.count() < cells || s.sums.count() < (size_t)CLOUD_MAX_BLOCKS + 1 || s.cand.count() < m || s.kept.count() < m)
        CK(hipStreamSynchronize(ctx->stream));
    CK(s.count.reserve(cells));
    CK(s.sums.reserve((size_t)CLOUD_MAX_BLOCKS + 1));
    CK(s.cand.reserve(m));
    CK(s.kept.reserve(m));
    if (c.filter()) CK(s.filtCounts.reserve(2));
    return OMDS_OK;
}
int reserve_tracked(omds_ctx* ctx, const CloudCall& c) {
    CloudState& s = ctx->cloud;
    const size_t cells = cloud_padded_cells(c.g), m = (size_t)c.g.max_spheres;
    if (s.rec.next().count() < cells || s.candCell.count() < m || s.keptCell.count() < m || s.vel.count() < m)
        CK(hipStreamSynchronize(ctx->stream));
    CK(s.rec.next().reserve(cells));   // counted into; the stored frame is the other one
    CK(s.candCell.reserve(m));
    CK(s.keptCell.reserve(m));
    CK(s.vel.reserve(m));
    return OMDS_OK;
}
int reserve_objects(omds_ctx* ctx, const CloudCall& c) {
    CloudState& s = ctx->cloud;
    const size_t cells = cloud_padded_cells(c.g), m = (size_t)c.g.max_spheres;
    if (s.slot.count() < cells || s.parent.count() < m || s.label.count() < m || s.object.count() < m || s.compOf.count() < m ||
        s.acc.count() < m * OBJ_ACC || s.objVel.count() < m || s.table.next().count() < m)
        CK(hipStreamSynchronize(ctx->stream));
    CK(s.slot.reserve(cells));
    CK(s.parent.reserve(m));
    CK(s.label.reserve(m));
    CK(s.object.reserve(m));
    CK(s.compOf.reserve(m));
    CK(s.acc.reserve(m * OBJ_ACC));
    CK(s.objVel.reserve(m));
    CK(s.table.next().reserve(m));     // written; the stored table is the other one
    return OMDS_OK;
}
int reserve_memory(omds_ctx* ctx, const CloudCall& c) {
    CloudState& s = ctx->cloud;
    const size_t cells = cloud_padded_cells(c.g), m = (size_t)c.g.max_spheres;
    if (s.mem.next().count() < cells || s.candCell.count() < m || s.keptCell.count() < m || s.age.count() < m || s.memCounts.count() < SCENE_MEM_COUNTS)
        CK(hipStreamSynchronize(ctx->stream));
    CK(s.mem.next().reserve(cells));   // written; the stored memory is the other one
    CK(s.candCell.reserve(m));
    CK(s.keptCell.reserve(m));
    CK(s.age.reserve(m));
    CK(s.memCounts.reserve(SCENE_MEM_COUNTS));
    return OMDS_OK;
}
int reserve_memory_flow(omds_ctx* ctx, const CloudCall& c) {
    CloudState& s = ctx->cloud;
    const size_t m = (size_t)c.g.max_spheres;
    if (s.seenCell.count() < m || s.seenIdx.count() < m || s.velAll.count() < m || s.labelAll.count() < m || s.objectAll.count() < m)
        CK(hipStreamSynchronize(ctx->stream));
    CK(s.seenCell.reserve(m));
    CK(s.seenIdx.reserve(m));
    CK(s.velAll.reserve(m));
    CK(s.labelAll.reserve(m));
    CK(s.objectAll.reserve(m));
    return OMDS_OK;
}
// the velocity filter: the state buffer that is not the stored one, the list of the cells it holds, and the scratch of the stage.  A
// state buffer is all zero outside its listed cells: a new allocation of either starts cleared, with an empty list
int reserve_vfilter(omds_ctx* ctx, const CloudCall& c) {
    CloudState& s = ctx->cloud;
    const size_t cells = (size_t)c.g.n_cells, m = (size_t)c.g.max_spheres;
    const int side = 1 - s.vstate.stored;
    const bool fresh = s.vstate.next().count() < cells || s.vcells[side].count() < m;
    if (fresh || s.vpred.count() < m || s.vgroup.count() < m * VEL_GROUP_ACC || s.vgroupH.count() < m || s.velOut.count() < m)
        CK(hipStreamSynchronize(ctx->stream));
    CK(s.vstate.next().reserve(cells));   // written; the stored state is the other one
    CK(s.vcells[side].reserve(m));
    CK(s.vpred.reserve(m));
    CK(s.vgroup.reserve(m * VEL_GROUP_ACC));
    CK(s.vgroupH.reserve(m));
    CK(s.velOut.reserve(m));
    CK(s.vcounts.reserve(3));
    if (fresh) {
        CK(hipMemsetAsync(s.vstate.next(), 0, s.vstate.next().bytes(), ctx->stream));
        s.vn[side] = 0;
    }
    return OMDS_OK;
}

// the ray table of a camera under the lens of slot t: built on the context's stream when the slot holds none under this key, and then
// r2_max and the pixels without a ray fetched behind it (synchronises; a one-off per camera and lens)
int lens_table(omds_ctx* ctx, const DepthCam& cam, const float* intr, DepthLensSlot& t) {
    CloudState& s = ctx->cloud;
    if (t.same(cam, intr, t.lens)) return OMDS_OK;
    const size_t n = (size_t)depth_visited(cam);
    if (t.ab.count() < n * 2 || s.lensRed.count() < 2) CK(hipStreamSynchronize(ctx->stream));
    t.have = false;
    CK(t.ab.reserve(n * 2));
    CK(s.lensRed.reserve(2));
    CK(hipMemsetAsync(s.lensRed, 0, 2 * 4, ctx->stream));
    omds_launch_depth_rays(ctx->stream, cam, intr[0], intr[1], t.lens, t.ab, s.lensRed);
    CK(hipGetLastError());
    unsigned red[2] = {0u, 0u};
    CK(hipMemcpyAsync(red, s.lensRed, 2 * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    std::memcpy(&t.r2_max, &red[0], 4);
    t.n_invalid = (int64_t)red[1];
    t.entries = (int64_t)n;
    t.width = cam.width; t.height = cam.height; t.step = cam.step;
    std::memcpy(t.intr, intr, 16);
    t.built = t.lens;
    t.have = true;
    return OMDS_OK;
}

// ---- stage the points: the caller's device memory as it is, host memory through a staging buffer of the context (a host array by
// one asynchronous copy, host images by one each)
int stage_points(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    if (!c.images) {
        const size_t n = (size_t)c.src.n_points;
        w.d_xyz = c.src.xyz;
        if (c.src.xyz_on_device || n == 0) return OMDS_OK;
        if (s.xyz.count() < n * 3) {
            CK(hipStreamSynchronize(ctx->stream));
            CK(s.xyz.alloc(n * 3));
        }
        CK(hipMemcpyAsync(s.xyz, c.src.xyz, n * 12, hipMemcpyHostToDevice, ctx->stream));
        w.d_xyz = s.xyz;
        return OMDS_OK;
    }
    const DepthSource& src = c.depth;
    size_t offset[OMDS_DEPTH_MAX_CAMERAS], bytes[OMDS_DEPTH_MAX_CAMERAS], total = 0;
    for (int i = 0; i < src.n_cams; ++i) {
        bytes[i] = (size_t)depth_extent(src.cam[i]) * (src.cam[i].format == OMDS_DEPTH_U16 ? 2 : 4);
        offset[i] = total;
        total += (bytes[i] + 15) & ~(size_t)15;
    }
    if (!src.on_device && s.depthImg.count() < total) {
        CK(hipStreamSynchronize(ctx->stream));
        CK(s.depthImg.alloc(total));
    }
    std::memset(static_cast<void*>(&w.depth), 0, sizeof(w.depth));
    for (int i = 0; i < src.n_cams; ++i) {
        DepthCamDev& d = w.depth.cam[i];
        d.c = src.cam[i];
        d.image = src.images[i];
        if (src.on_device) continue;
        CK(hipMemcpyAsync(s.depthImg.get() + offset[i], src.images[i], bytes[i], hipMemcpyHostToDevice, ctx->stream));
        d.image = s.depthImg.get() + offset[i];
    }
    if (!src.lensed) return OMDS_OK;
    std::memset(static_cast<void*>(&w.lens), 0, sizeof(w.lens));   // ab == nullptr: pinhole
    for (int i = 0; i < src.n_cams; ++i) {
        DepthLensSlot& t = s.lens[i];
        if (!t.on) continue;
        if (int rc = lens_table(ctx, src.cam[i], src.intr[i], t)) return rc;
        w.lens.cam[i] = DepthLensCam{t.lens, t.r2_max, t.ab.get()};
    }
    return OMDS_OK;
}

// the number of items the compaction of n items that was just enqueued kept.  Synchronises.
int compaction_total(omds_ctx* ctx, int n, int* total_out) {
    *total_out = 0;
    if (n <= 0) return OMDS_OK;
    CK(hipGetLastError());
    unsigned total = 0;
    CK(hipMemcpyAsync(&total, ctx->cloud.sums + cloud_compaction_blocks(n), 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    *total_out = (int)total;
    return OMDS_OK;
}

// ---- count and compact the cells: the candidates in cell order, their cell indices when tracked or memory, and w.occupied (with
// memory: seen + remembered).  The depth filter's counters go round the counting pass of a depth call: cleared in front of it, fetched
// behind the compaction, read after the synchronisation; without a filter the call leaves the stats at 0, 0
void compact_counted(omds_ctx* ctx, const CloudCall& c, const unsigned* count) {
    omds_launch_cloud_compact_cells(ctx->stream, count, c.g, ctx->cloud.cand, ctx->cloud.sums);
}
void compact_counted(omds_ctx* ctx, const CloudCall& c, const uint4* rec) {
    omds_launch_cloud_compact_cells(ctx->stream, rec, c.g, ctx->cloud.cand, ctx->cloud.candCell, ctx->cloud.sums);
}
template <class T>   // unsigned: counts, uint4: records
int count_into(omds_ctx* ctx, const CloudCall& c, CloudWork& w, T* into) {
    CloudState& s = ctx->cloud;
    int rc;
    CK(hipMemsetAsync(into, 0, cloud_padded_cells(c.g) * sizeof(T), ctx->stream));
    if (c.memory) CK(hipMemsetAsync(s.memCounts, 0, SCENE_MEM_COUNTS * 4, ctx->stream));
    const DepthLensTable* lens = c.depth.lensed ? &w.lens : nullptr;
    if (!c.images) omds_launch_cloud_count(ctx->stream, w.d_xyz, (long long)c.src.n_points, c.g, into);
    else if (!c.filter()) omds_launch_cloud_count(ctx->stream, w.depth, lens, c.depth.n_cams, c.g, into);
    else omds_launch_cloud_count_filtered(ctx->stream, w.depth, lens, c.depth.n_cams, c.g, *c.filter(), into, s.filtCounts);
    if (!c.memory) {
        compact_counted(ctx, c, into);
        return OMDS_OK;
    }
    w.mem_stored = s.memKey.same(c.g, c.sm) ? s.mem.kept().get() : nullptr;
    if ((rc = prof_begin(ctx))) return rc;   // omds_prof_enable: a memory route's dominant kernel is k_scene_memory
    omds_launch_scene_memory(ctx->stream, w.depth, lens, c.ks, c.depth.n_cams, c.g, c.sm, into, w.mem_stored, s.mem.next(), s.memCounts);
    if ((rc = prof_end(ctx, c.g.n_cells, 0.0, "k_scene_memory"))) return rc;
    omds_launch_cloud_compact_cells(ctx->stream, s.mem.next().get(), c.g, s.cand, s.candCell, s.sums);
    return OMDS_OK;
}
int filter_stats_begin(omds_ctx* ctx, const CloudCall& c) {
    CloudState& s = ctx->cloud;
    if (c.images) s.filter_stats[0] = s.filter_stats[1] = 0;
    if (c.filter()) CK(hipMemsetAsync(s.filtCounts, 0, 2 * 4, ctx->stream));
    return OMDS_OK;
}
void filter_stats_done(omds_ctx* ctx, const CloudCall& c, const CloudWork& w) {
    if (!c.filter()) return;
    ctx->cloud.filter_stats[0] = (int64_t)w.filt_counts[0];
    ctx->cloud.filter_stats[1] = (int64_t)w.filt_counts[1];
}
int count_cells(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    int rc;
    if ((rc = filter_stats_begin(ctx, c))) return rc;
    if ((rc = c.tracked ? count_into(ctx, c, w, s.rec.next().get()) : count_into(ctx, c, w, s.count.get()))) return rc;
    w.d_list = s.cand;
    if (c.tracked || c.memory) w.d_cell = s.candCell;
    if (c.filter()) CK(hipMemcpyAsync(w.filt_counts, s.filtCounts, 2 * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (c.memory) CK(hipMemcpyAsync(w.counts, s.memCounts, 4 * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = compaction_total(ctx, c.g.n_cells, &w.occupied))) return rc;
    filter_stats_done(ctx, c, w);
    return OMDS_OK;
}

// ---- self-filter: the candidates become the obstacle rows of one state.  From here on the tables of the old scene are overwritten:
// the context holds no scene, and no horizon of one, until install_scene has put the new one in
int self_filter(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    const int n = ctx->cfg.n_dof, occupied = w.occupied;
    if (int rc = reserve_obstacle_capacity(ctx, occupied)) return rc;
    ctx->n_obs = 0;
    clear_obstacle_horizon(ctx);
    CK(hipMemcpyAsync(ctx->d_qcur, c.q_now, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_qcur, 1, 1, ctx->d_Fq);
    omds_launch_obstacle_features(ctx->stream, ctx->mlp, reinterpret_cast<const float*>(w.d_list), occupied, ctx->d_Fp, ctx->d_radius);
    omds_launch_pass1(ctx->stream, ctx->mlp, ctx->d_Fq, ctx->d_Fp, ctx->d_radius, occupied, 1, ctx->prm.ignored_links, ctx->d_Dmin);
    CK(hipGetLastError());
    omds_launch_cloud_compact_kept(ctx->stream, ctx->d_Dmin, w.d_list, w.d_cell, occupied, c.spec->self_margin, c.g.max_spheres, s.kept, s.keptCell,
                                   s.sums);
    w.d_list = s.kept;
    if (w.d_cell) w.d_cell = s.keptCell;
    if (int rc = compaction_total(ctx, occupied, &w.n_list)) return rc;
    if (!c.memory) return OMDS_OK;
    // ... and the cells of the candidates it drops leave the memory; their number is on the host after the next synchronisation
    omds_launch_scene_memory_forget(ctx->stream, ctx->d_Dmin, s.candCell, occupied, c.spec->self_margin, s.mem.next(), s.memCounts);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(w.counts + SCENE_MEM_FORGOTTEN, s.memCounts + SCENE_MEM_FORGOTTEN, 4, hipMemcpyDeviceToHost, ctx->stream));
    return OMDS_OK;
}

// ---- sphere velocities: the final list against the stored frame, if there is one on this grid
int sphere_velocities(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    w.have_prev = s.frame.same(c.g);
    if (!w.have_prev || w.n_list == 0) return OMDS_OK;
    w.vel4.resize((size_t)w.n_list * 4);
    omds_launch_cloud_flow(ctx->stream, c.g, c.tr, s.rec.next(), s.rec.kept(), w.d_cell, w.n_list, s.vel);
    CK(hipGetLastError());
    return OMDS_OK;
}

// ---- objects: the components of the final list, their match against the stored table and the velocities of the accepted objects
int object_velocities(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    const int n = w.n_list;
    w.have_table = w.have_prev && s.tab.same(c.ob);
    w.label.assign((size_t)w.n_final, -1);   // padding spheres: label -1, no object
    w.object.assign((size_t)w.n_final, 0);
    if (n == 0) return OMDS_OK;
    omds_launch_cloud_components(ctx->stream, c.g, c.ob.link, s.rec.next(), w.d_cell, n, s.slot, s.parent, s.label, s.acc);
    CK(hipGetLastError());
    omds_launch_cloud_compact_roots(ctx->stream, s.parent, w.d_cell, s.acc, n, c.g.max_spheres, s.table.next(), s.compOf, s.sums);
    if (int rc = compaction_total(ctx, n, &w.n_comp)) return rc;
    omds_launch_cloud_match(ctx->stream, c.g, c.tr, c.ob, s.table.next(), w.n_comp, s.table.kept(), w.have_table ? s.tab.n : 0, s.objVel);
    if (w.have_table) {
        omds_launch_cloud_apply(ctx->stream, s.parent, s.compOf, s.objVel, n, s.vel, s.object);
        CK(hipMemcpyAsync(w.object.data(), s.object, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    CK(hipGetLastError());
    w.obj_vel.resize((size_t)w.n_comp * 4);
    CK(hipMemcpyAsync(w.obj_vel.data(), s.objVel, (size_t)w.n_comp * 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemcpyAsync(w.label.data(), s.label, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    return OMDS_OK;
}

// ---- memory: the calls since the cell of every final sphere was last counted
int memory_ages(omds_ctx* ctx, const CloudCall&, CloudWork& w) {
    CloudState& s = ctx->cloud;
    w.age.assign((size_t)w.n_final, -1);
    if (w.n_list == 0) return OMDS_OK;
    omds_launch_scene_memory_age(ctx->stream, s.mem.next(), w.d_cell, w.n_list, s.age);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(w.age.data(), s.age, (size_t)w.n_list * 4, hipMemcpyDeviceToHost, ctx->stream));
    return OMDS_OK;
}

// ---- memory and tracked: the ordered compaction of the final list to T, the spheres whose cell was counted now -> the two stages
// above on T as their final list, unchanged -> one launch carries T's results back to the whole list under scene_memory_flow_still,
// which reads the STORED words.  t is the caller's: copies to its vectors are under way until install_scene synchronises
int memory_velocities(omds_ctx* ctx, const CloudCall& c, CloudWork& w, CloudWork& t) {
    CloudState& s = ctx->cloud;
    int rc;
    w.label.assign((size_t)w.n_final, -1);   // padding spheres: label -1, no object
    w.object.assign((size_t)w.n_final, 0);
    w.have_prev = s.frame.same(c.g);
    if (w.n_list == 0) {
        w.have_table = c.objects && w.have_prev && s.tab.same(c.ob);
        return OMDS_OK;
    }
    omds_launch_cloud_compact_seen(ctx->stream, s.rec.next(), c.g, w.d_cell, w.n_list, s.seenCell, s.seenIdx, s.sums);
    if ((rc = compaction_total(ctx, w.n_list, &t.n_list))) return rc;
    t.d_cell = s.seenCell;
    t.n_final = t.n_list;
    if ((rc = sphere_velocities(ctx, c, t))) return rc;
    if (c.objects && (rc = object_velocities(ctx, c, t))) return rc;
    const bool flowed = t.have_prev && t.n_list > 0, labelled = c.objects && t.n_list > 0;
    omds_launch_scene_memory_flow(ctx->stream, s.rec.next(), c.g, w.mem_stored, w.d_cell, w.n_list, s.seenIdx, t.n_list,
                                  flowed ? s.vel.get() : nullptr, labelled ? s.label.get() : nullptr,
                                  labelled && t.have_table ? s.object.get() : nullptr, s.velAll, s.labelAll, s.objectAll);
    CK(hipGetLastError());
    if (c.objects) {
        CK(hipMemcpyAsync(w.label.data(), s.labelAll, (size_t)w.n_list * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(w.object.data(), s.objectAll, (size_t)w.n_list * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (w.have_prev) {
        w.vel4.resize((size_t)w.n_list * 4);
        w.d_vel = s.velAll;
    }
    w.have_table = t.have_table;   // what commit_objects takes of T: the table is of its components
    w.n_comp = t.n_comp;
    w.obj_vel = std::move(t.obj_vel);
    return OMDS_OK;
}

// ---- the velocity filter: the velocities of the final list, wherever the stages above left them, against the stored state while it is
// of this grid and filter spec, into velOut, which install_scene then fetches; the records into the state buffer that is not the
// stored one, emptied first of the cells it last held.  Without a previous frame there are no velocities: commit_vfilter empties the
// history.  The labels and object flags are the route's: of the whole list behind k_scene_memory_flow, else of object_velocities
int filter_velocities(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    if (!w.have_prev) return OMDS_OK;
    const int n = w.n_list, side = 1 - s.vstate.stored;
    omds_launch_vel_clear(ctx->stream, s.vcells[side], s.vn[side], s.vstate.next());
    s.vn[side] = 0;
    CK(hipGetLastError());
    if (n == 0) return OMDS_OK;
    const float4* raw = w.d_vel ? w.d_vel : s.vel.get();
    const bool grouped = c.objects && w.have_table;
    const int* label = !grouped ? nullptr : c.memory ? s.labelAll.get() : s.label.get();
    const int* object = !grouped ? nullptr : c.memory ? s.objectAll.get() : s.object.get();
    w.raw4.resize((size_t)n * 4);
    CK(hipMemcpyAsync(w.raw4.data(), raw, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipMemsetAsync(s.vcounts, 0, 3 * 4, ctx->stream));
    omds_launch_vel_filter(ctx->stream, c.g, c.tr, *c.vfilt, s.vkey.same(c.g, *c.vfilt) ? s.vstate.kept().get() : nullptr, w.d_cell, n, raw, label,
                           object, s.vpred, s.vgroup, s.vgroupH, s.vstate.next(), s.vcells[side], s.velOut, s.vcounts);
    CK(hipGetLastError());
    s.vn[side] = n;   // what k_vel_blend lists
    CK(hipMemcpyAsync(w.vcounts, s.vcounts, 3 * 4, hipMemcpyDeviceToHost, ctx->stream));
    w.d_vel = s.velOut;
    return OMDS_OK;
}

// ---- install: the list to the host, filled up to n_closest with the spec's pad sphere, and in as omds_set_obstacles puts a list in;
// then the velocities, if any sphere moves: a scene whose every sphere stands still keeps the cleared horizon, and the propagate that
// follows is the static one
int install_scene(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    const int n_list = w.n_list, n_final = w.n_final;
    if (!w.vel4.empty())
        CK(hipMemcpyAsync(w.vel4.data(), w.d_vel ? w.d_vel : ctx->cloud.vel.get(), (size_t)n_list * 16, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<float> list((size_t)n_final * 4);
    if (n_list > 0) CK(hipMemcpyAsync(list.data(), w.d_list, (size_t)n_list * 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    for (int i = n_list; i < n_final; ++i) std::memcpy(&list[(size_t)i * 4], c.spec->pad, 16);
    if (int rc = install_obstacles(ctx, list.data(), n_final)) return rc;
    if (c.out.n_spheres) *c.out.n_spheres = n_list;
    if (w.vel4.empty()) return OMDS_OK;
    std::vector<float> vel((size_t)n_final * 3, 0.f);   // padding spheres stand still
    bool moving = false;
    for (size_t i = 0; i * 4 < w.vel4.size(); ++i) {
        for (int k = 0; k < 3; ++k) {
            vel[i * 3 + k] = w.vel4[i * 4 + k];
            moving |= w.vel4[i * 4 + k] != 0.f;
        }
        w.matched += w.vel4[i * 4 + 3] != 0.f;
    }
    return moving ? omds_set_obstacle_motion(ctx, vel.data()) : OMDS_OK;
}

// ---- commit, behind everything that can fail: what was counted is the stored frame now ...
void commit_frame(omds_ctx* ctx, const CloudCall& c, const CloudWork& w) {
    CloudState& s = ctx->cloud;
    s.rec.commit();
    s.frame.set(c.g);
    s.tab.have = false;   // a plain tracked call stores its records and no table: the next objects call has nothing to match
    if (c.out.n_matched) *c.out.n_matched = w.have_prev ? (int32_t)w.matched : -1;
}
// ... and what was written the stored table, with the labels of the scene in force
void commit_objects(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    int32_t n_objects = 0, n_accepted = 0;
    for (int i = 0; i < w.n_comp; ++i) {
        n_objects += w.obj_vel[(size_t)i * 4 + 3] >= 1.f;
        n_accepted += w.obj_vel[(size_t)i * 4 + 3] == 2.f;
    }
    s.table.commit();
    s.tab.set(c.ob, w.n_comp);
    s.obj_label = std::move(w.label);
    s.obj_flag = std::move(w.object);
    s.obj_count = n_objects;
    if (c.out.n_objects) *c.out.n_objects = n_objects;
    if (c.out.n_objects_matched) *c.out.n_objects_matched = w.have_table ? n_accepted : -1;
}

// ... and what the velocity filter wrote the stored state, with the unfiltered velocities and flags of the scene in force.  A call
// without a previous frame leaves an empty history
void commit_vfilter(omds_ctx* ctx, const CloudCall& c, const CloudWork& w) {
    CloudState& s = ctx->cloud;
    s.vkey.grid.have = false;
    if (w.have_prev) {
        s.vstate.commit();
        s.vkey.set(c.g, *c.vfilt);
    }
    s.vf_have = true;
    s.vf_raw.assign((size_t)w.n_final * 3, 0.f);   // padding spheres stand still
    s.vf_live.assign((size_t)w.n_final, 0);
    for (size_t i = 0; i * 4 < w.raw4.size(); ++i) {
        for (int k = 0; k < 3; ++k) s.vf_raw[i * 3 + k] = w.raw4[i * 4 + k];
        s.vf_live[i] = w.raw4[i * 4 + 3] != 0.f;
    }
    for (int k = 0; k < 3; ++k) s.vf_stats[k] = (int32_t)w.vcounts[k];
}

// ... and, first of the three, what was written the stored memory, with the ages of the scene in force
void commit_memory(omds_ctx* ctx, const CloudCall& c, CloudWork& w) {
    CloudState& s = ctx->cloud;
    if (c.out.counts) c.out.counts[SCENE_MEM_FORGOTTEN] = (int32_t)w.counts[SCENE_MEM_FORGOTTEN];
    s.mem_age = std::move(w.age);
    s.mem.commit();
    s.memKey.set(c.g, c.sm);
}

// THE sequence of every route.  A refusal and every failure in front of the commits leave what is stored as it was: each Flip was
// written in the buffer that is not the stored one.  Without `tracked` no line touches the records, the frame key or the table key
int scene_from_cloud(omds_ctx* ctx, const CloudCall& c) {
    const std::string me(c.who);
    int rc;
    REQUIRE(c.images || (c.src.n_points >= 0 && c.src.n_points <= OMDS_CLOUD_MAX_POINTS && (c.src.n_points == 0 || c.src.xyz)),
            OMDS_ERR_INVALID_ARG, me + ": need 0 <= n_points <= 16 777 216 and a non-null xyz [P,3]");
    if (c.q_now) {
        REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, me + ": the self-filter needs the distance network (omds_set_mlp)");
        REQUIRE(!ctx->wide.on, OMDS_ERR_UNSUPPORTED, me + ": no self-filter on networks wider than 256 (no obstacle tables)");
    }
    CK(hipSetDevice(ctx->dev));
    CloudWork w, t;   // t: with memory and tracked, the seen sublist as the final list of the velocity stages
    if ((rc = reserve_base(ctx, c))) return rc;
    if (c.tracked && (rc = reserve_tracked(ctx, c))) return rc;
    if (c.objects && (rc = reserve_objects(ctx, c))) return rc;
    if (c.memory && (rc = reserve_memory(ctx, c))) return rc;
    if (c.memory && c.tracked && (rc = reserve_memory_flow(ctx, c))) return rc;
    if (c.vfilt && (rc = reserve_vfilter(ctx, c))) return rc;
    if ((rc = stage_points(ctx, c, w))) return rc;
    if ((rc = count_cells(ctx, c, w))) return rc;
    if (c.out.n_occupied) *c.out.n_occupied = w.occupied;
    if (c.out.counts)
        for (int k = 0; k < SCENE_MEM_COUNTS; ++k) c.out.counts[k] = (int32_t)w.counts[k];
    REQUIRE(w.occupied <= c.g.max_spheres, OMDS_ERR_INVALID_ARG,
            me + (!c.memory   ? ": more occupied cells than max_spheres (n_occupied_out holds their number); the scene is unchanged"
                  : !c.tracked ? ": more seen and remembered cells than max_spheres (counts_out holds their numbers); the scene and the memory are "
                                 "unchanged"
                               : ": more seen and remembered cells than max_spheres (counts_out holds their numbers); the scene, the memory, the "
                                 "record frame and the component table are unchanged"));
    w.n_list = w.occupied;
    if (c.q_now && w.occupied > 0 && (rc = self_filter(ctx, c, w))) return rc;
    w.n_final = std::max(w.n_list, ctx->cfg.n_closest);
    if (c.memory && (rc = memory_ages(ctx, c, w))) return rc;
    if (c.tracked && !c.memory && (rc = sphere_velocities(ctx, c, w))) return rc;
    if (c.objects && !c.memory && (rc = object_velocities(ctx, c, w))) return rc;
    if (c.tracked && c.memory && (rc = memory_velocities(ctx, c, w, t))) return rc;
    if (c.vfilt && (rc = filter_velocities(ctx, c, w))) return rc;
    if ((rc = install_scene(ctx, c, w))) return rc;
    if (c.memory) commit_memory(ctx, c, w);
    if (c.tracked) commit_frame(ctx, c, w);
    if (c.vfilt) commit_vfilter(ctx, c, w);
    if (c.objects) commit_objects(ctx, c, w);
    return OMDS_OK;
}

// a cloud entry point behind resolve_call: the caller's array as the point source
int scene_from_points(omds_ctx* ctx, CloudCall& c, const float* xyz, int64_t n_points, int xyz_on_device, const float* q_now, const CloudOuts& out) {
    c.src = PointSource{xyz, n_points, xyz_on_device};
    c.q_now = q_now;
    c.out = out;
    return scene_from_cloud(ctx, c);
}

// the checks of a depth call's cameras and images, into depth (whose images, n_cams and on_device the caller has set)
int resolve_depth_source(omds_ctx* ctx, const char* me, const omds_depth_camera* cams, DepthSource& depth) {
    REQUIRE(depth.n_cams >= 1 && depth.n_cams <= OMDS_DEPTH_MAX_CAMERAS && cams && depth.images, OMDS_ERR_INVALID_ARG,
            std::string(me) + ": need 1 <= n_cams <= 8 and non-null cams, images [n_cams]");
    int64_t visited = 0;
    for (int i = 0; i < depth.n_cams; ++i) {
        if (int rc = depth_resolve_camera(cams + i, &depth.cam[i], &ctx->err)) return rc;
        REQUIRE(depth.images[i], OMDS_ERR_INVALID_ARG, std::string(me) + ": a null image");
        visited += depth_visited(depth.cam[i]);   // each < 2^62 / 8: no overflow
    }
    REQUIRE(visited <= OMDS_CLOUD_MAX_POINTS, OMDS_ERR_INVALID_ARG, std::string(me) + ": more than 16 777 216 visited pixels in all");
    return OMDS_OK;
}

// a depth entry point behind resolve_call: the images, with the context's filter, as the point source; with `memory` the route with
// the scene memory, mem_spec behind its checks in front of the cameras'
int scene_from_images(omds_ctx* ctx, CloudCall& c, bool memory, const omds_scene_memory_spec* mem_spec, const omds_depth_camera* cams,
                      const void* const* images, int32_t n_cams, int images_on_device, const float* q_now, const CloudOuts& out) {
    if (memory)
        if (int rc = scene_memory_resolve(mem_spec, c.g, &c.sm, &ctx->err)) return rc;
    c.images = true;
    c.memory = memory;
    c.depth.images = images;
    c.depth.n_cams = n_cams;
    c.depth.on_device = images_on_device;
    c.depth.filt = ctx->cloud.filter_on ? &ctx->cloud.filter : nullptr;
    if (int rc = resolve_depth_source(ctx, c.who, cams, c.depth)) return rc;
    for (int i = 0; memory && i < n_cams; ++i) c.ks.k[i] = scene_memory_camera(cams[i], c.depth.cam[i]);
    c.depth.lensed = false;
    for (int i = 0; i < n_cams; ++i) {
        const float intr[4] = {cams[i].fx, cams[i].fy, cams[i].cx, cams[i].cy};
        std::memcpy(c.depth.intr[i], intr, 16);
        if (ctx->cloud.lens[i].on) c.depth.lensed = true;
    }
    c.q_now = q_now;
    c.out = out;
    return scene_from_cloud(ctx, c);
}

}  // namespace

extern "C" {

int omds_point_cloud_spheres(const omds_cloud_spec* spec, const float* xyz, int64_t n_points, float* xyzr_out, int32_t cap,
                             int32_t* count_out) {
    return cloud_spheres_host(spec, xyz, n_points, xyzr_out, cap, count_out, &g_create_err);
}

int omds_point_cloud_flow(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const float* xyz_prev, int64_t n_prev,
                          const float* xyz_now, int64_t n_now, float* xyzr_out, float* vel_out, int32_t cap, int32_t* count_out,
                          int32_t* matched_out) {
    return cloud_flow_host(spec, track, xyz_prev, n_prev, xyz_now, n_now, xyzr_out, vel_out, cap, count_out, matched_out, &g_create_err);
}

int omds_point_cloud_object_flow(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const omds_cloud_object_spec* obj,
                                 const float* xyz_prev, int64_t n_prev, const uint8_t* keep_prev, const float* xyz_now, int64_t n_now,
                                 const uint8_t* keep_now, float* xyzr_out, float* vel_out, int32_t* label_out, int32_t* object_out, int32_t cap,
                                 int32_t* count_out, int32_t* matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out) {
    return cloud_objects_host(spec, track, obj, xyz_prev, n_prev, keep_prev, xyz_now, n_now, keep_now, xyzr_out, vel_out, label_out, object_out,
                              cap, count_out, matched_out, n_objects_out, n_objects_matched_out, &g_create_err);
}

int omds_depth_points(const omds_depth_camera* cam, const void* image, float* xyz_out, int64_t cap_points, int64_t* n_valid_out) {
    return depth_points_host(cam, image, xyz_out, cap_points, n_valid_out, &g_create_err);
}

int omds_depth_points_filtered(const omds_depth_camera* cam, const omds_depth_filter_spec* filt, const void* image, float* xyz_out,
                               int64_t cap_points, int64_t* n_valid_out, int64_t* n_rejected_out) {
    return depth_points_filtered_host(cam, filt, image, xyz_out, cap_points, n_valid_out, n_rejected_out, &g_create_err);
}

int omds_depth_lens_rays(const omds_depth_camera* cam, const omds_depth_lens* lens, float* ab_out, float* r2_max_out, int64_t* n_invalid_out) {
    return depth_lens_rays_host(cam, lens, ab_out, r2_max_out, n_invalid_out, &g_create_err);
}

int omds_depth_points_lens(const omds_depth_camera* cam, const omds_depth_lens* lens, const omds_depth_filter_spec* filt, const void* image,
                           float* xyz_out, int64_t cap_points, int64_t* n_valid_out, int64_t* n_rejected_out) {
    return depth_points_lens_host(cam, lens, filt, image, xyz_out, cap_points, n_valid_out, n_rejected_out, &g_create_err);
}

int omds_depth_scene_memory_lens(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_filter_spec* filt,
                                 const omds_depth_lens* lenses, const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                 const uint32_t* mem_in, uint32_t* mem_out, int32_t counts_out[4]) {
    return scene_memory_lens_host(spec, mem_spec, filt, lenses, cams, images, n_cams, mem_in, mem_out, counts_out, &g_create_err);
}

int omds_depth_scene_memory_flow_lens(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_cloud_track_spec* track,
                                      const omds_cloud_object_spec* obj, const omds_depth_filter_spec* filt, const omds_depth_lens* lenses_prev,
                                      const omds_depth_camera* cams_prev, const void* const* images_prev, int32_t n_cams_prev,
                                      const uint8_t* keep_prev, const omds_depth_lens* lenses, const omds_depth_camera* cams,
                                      const void* const* images, int32_t n_cams, const uint8_t* keep_now, const uint32_t* mem_in, uint32_t* mem_out,
                                      int32_t counts_out[5], float* xyzr_out, float* vel_out, int32_t* age_out, int32_t* label_out,
                                      int32_t* object_out, int32_t cap, int32_t* count_out, int32_t* n_matched_out, int32_t* n_objects_out,
                                      int32_t* n_objects_matched_out) {
    return scene_memory_flow_host(spec, mem_spec, track, obj, filt, cams_prev, images_prev, n_cams_prev, keep_prev, cams, images, n_cams, keep_now,
                                  mem_in, mem_out, counts_out, xyzr_out, vel_out, age_out, label_out, object_out, cap, count_out, n_matched_out,
                                  n_objects_out, n_objects_matched_out, &g_create_err, lenses_prev, lenses);
}

int omds_set_depth_lenses(omds_ctx* ctx, const omds_depth_lens* lenses, int32_t n) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudState& s = ctx->cloud;
    REQUIRE(n >= 0 && n <= OMDS_DEPTH_MAX_CAMERAS, OMDS_ERR_INVALID_ARG, "omds_set_depth_lenses: need 0 <= n <= 8");
    if (!lenses) n = 0;
    DepthLens l[OMDS_DEPTH_MAX_CAMERAS];
    for (int i = 0; i < n; ++i)
        if (int rc = depth_lens_resolve(lenses + i, &l[i], &ctx->err)) return rc;   // the stored lenses stay as they were
    for (int i = 0; i < OMDS_DEPTH_MAX_CAMERAS; ++i) {
        s.lens[i].on = i < n && l[i].model != 0;
        if (s.lens[i].on) s.lens[i].lens = l[i];
    }
    return OMDS_OK;
}

int omds_get_depth_lens_table(omds_ctx* ctx, int32_t i, float* ab_out, float* r2_max_out, int64_t* n_invalid_out, int64_t* n_entries_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(i >= 0 && i < OMDS_DEPTH_MAX_CAMERAS, OMDS_ERR_INVALID_ARG, "omds_get_depth_lens_table: need 0 <= i < 8");
    const DepthLensSlot& t = ctx->cloud.lens[i];
    if (n_entries_out) *n_entries_out = t.have ? t.entries : 0;
    if (r2_max_out) *r2_max_out = t.have ? t.r2_max : 0.f;
    if (n_invalid_out) *n_invalid_out = t.have ? t.n_invalid : 0;
    if (ab_out && t.have && t.entries > 0) {
        CK(hipSetDevice(ctx->dev));
        CK(hipMemcpyAsync(ab_out, t.ab.get(), (size_t)t.entries * 8, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

int omds_set_depth_filter(omds_ctx* ctx, const omds_depth_filter_spec* spec) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudState& s = ctx->cloud;
    if (!spec) {
        s.filter_on = false;
        return OMDS_OK;
    }
    DepthFilter f;
    if (int rc = depth_filter_resolve(spec, &f, &ctx->err)) return rc;   // the stored filter stays as it was
    s.filter = f;
    s.filter_on = true;
    return OMDS_OK;
}

int omds_get_depth_filter_stats(omds_ctx* ctx, int64_t out[2]) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(out, OMDS_ERR_INVALID_ARG, "omds_get_depth_filter_stats: null out");
    out[0] = ctx->cloud.filter_stats[0];
    out[1] = ctx->cloud.filter_stats[1];
    return OMDS_OK;
}

int omds_set_obstacles_from_cloud(omds_ctx* ctx, const omds_cloud_spec* spec, const float* xyz, int64_t n_points, int xyz_on_device,
                                  const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudCall c;
    if (int rc = resolve_call(ctx, "omds_set_obstacles_from_cloud", spec, false, nullptr, false, nullptr, &c)) return rc;
    return scene_from_points(ctx, c, xyz, n_points, xyz_on_device, q_now, {n_spheres_out, n_occupied_out, nullptr, nullptr, nullptr});
}

int omds_set_obstacles_from_cloud_tracked(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const float* xyz,
                                          int64_t n_points, int xyz_on_device, const float* q_now, int32_t* n_spheres_out,
                                          int32_t* n_occupied_out, int32_t* n_matched_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudCall c;
    if (int rc = resolve_call(ctx, "omds_set_obstacles_from_cloud_tracked", spec, true, track, false, nullptr, &c)) return rc;
    return scene_from_points(ctx, c, xyz, n_points, xyz_on_device, q_now, {n_spheres_out, n_occupied_out, n_matched_out, nullptr, nullptr});
}

int omds_set_obstacles_from_cloud_objects(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track,
                                          const omds_cloud_object_spec* obj, const float* xyz, int64_t n_points, int xyz_on_device,
                                          const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out, int32_t* n_matched_out,
                                          int32_t* n_objects_out, int32_t* n_objects_matched_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudCall c;
    if (int rc = resolve_call(ctx, "omds_set_obstacles_from_cloud_objects", spec, true, track, true, obj, &c)) return rc;
    return scene_from_points(ctx, c, xyz, n_points, xyz_on_device, q_now,
                             {n_spheres_out, n_occupied_out, n_matched_out, n_objects_out, n_objects_matched_out});
}

int omds_set_obstacles_from_depth(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track,
                                  const omds_cloud_object_spec* obj, const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                  int images_on_device, const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out,
                                  int32_t* n_matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudCall c;
    if (int rc = resolve_call(ctx, "omds_set_obstacles_from_depth", spec, track != nullptr, track, obj != nullptr, obj, &c)) return rc;
    return scene_from_images(ctx, c, false, nullptr, cams, images, n_cams, images_on_device, q_now,
                             {n_spheres_out, n_occupied_out, n_matched_out, n_objects_out, n_objects_matched_out, nullptr});
}

int omds_depth_scene_memory(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_camera* cams,
                            const void* const* images, int32_t n_cams, const uint32_t* mem_in, uint32_t* mem_out, int32_t counts_out[4]) {
    return scene_memory_host(spec, mem_spec, cams, images, n_cams, mem_in, mem_out, counts_out, &g_create_err);
}

int omds_depth_scene_memory_filtered(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_filter_spec* filt,
                                     const omds_depth_camera* cams, const void* const* images, int32_t n_cams, const uint32_t* mem_in,
                                     uint32_t* mem_out, int32_t counts_out[4]) {
    return scene_memory_host(spec, mem_spec, filt, cams, images, n_cams, mem_in, mem_out, counts_out, &g_create_err);
}

int omds_set_obstacles_from_depth_memory(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec,
                                         const omds_depth_camera* cams, const void* const* images, int32_t n_cams, int images_on_device,
                                         const float* q_now, int32_t* n_spheres_out, int32_t counts_out[5]) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudCall c;
    if (int rc = resolve_call(ctx, "omds_set_obstacles_from_depth_memory", spec, false, nullptr, false, nullptr, &c)) return rc;
    return scene_from_images(ctx, c, true, mem_spec, cams, images, n_cams, images_on_device, q_now,
                             {n_spheres_out, nullptr, nullptr, nullptr, nullptr, counts_out});
}

int omds_depth_scene_memory_flow(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_cloud_track_spec* track,
                                 const omds_cloud_object_spec* obj, const omds_depth_filter_spec* filt, const omds_depth_camera* cams_prev,
                                 const void* const* images_prev, int32_t n_cams_prev, const uint8_t* keep_prev, const omds_depth_camera* cams,
                                 const void* const* images, int32_t n_cams, const uint8_t* keep_now, const uint32_t* mem_in, uint32_t* mem_out,
                                 int32_t counts_out[5], float* xyzr_out, float* vel_out, int32_t* age_out, int32_t* label_out,
                                 int32_t* object_out, int32_t cap, int32_t* count_out, int32_t* n_matched_out, int32_t* n_objects_out,
                                 int32_t* n_objects_matched_out) {
    return scene_memory_flow_host(spec, mem_spec, track, obj, filt, cams_prev, images_prev, n_cams_prev, keep_prev, cams, images, n_cams, keep_now,
                                  mem_in, mem_out, counts_out, xyzr_out, vel_out, age_out, label_out, object_out, cap, count_out, n_matched_out,
                                  n_objects_out, n_objects_matched_out, &g_create_err);
}

int omds_set_obstacles_from_depth_memory_tracked(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec,
                                                 const omds_cloud_track_spec* track, const omds_cloud_object_spec* obj,
                                                 const omds_depth_camera* cams, const void* const* images, int32_t n_cams, int images_on_device,
                                                 const float* q_now, int32_t* n_spheres_out, int32_t counts_out[5], int32_t* n_matched_out,
                                                 int32_t* n_objects_out, int32_t* n_objects_matched_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudCall c;
    if (int rc = resolve_call(ctx, "omds_set_obstacles_from_depth_memory_tracked", spec, true, track, obj != nullptr, obj, &c)) return rc;
    return scene_from_images(ctx, c, true, mem_spec, cams, images, n_cams, images_on_device, q_now,
                             {n_spheres_out, nullptr, n_matched_out, n_objects_out, n_objects_matched_out, counts_out});
}

int omds_scene_memory_reset(omds_ctx* ctx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    ctx->cloud.memKey.grid.have = false;
    return OMDS_OK;
}

int omds_get_scene_memory(omds_ctx* ctx, int32_t* age, uint32_t* grid, int32_t* n_cells_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudState& s = ctx->cloud;
    const bool have = s.memKey.grid.have;
    if (n_cells_out) *n_cells_out = have ? s.memKey.n_cells : 0;
    if (age && ctx->n_obs > 0) {
        if (s.mem_age.size() == (size_t)ctx->n_obs) std::memcpy(age, s.mem_age.data(), (size_t)ctx->n_obs * 4);
        else std::fill(age, age + ctx->n_obs, -1);
    }
    if (grid && have) {
        CK(hipSetDevice(ctx->dev));
        CK(hipMemcpyAsync(grid, s.mem.kept(), (size_t)s.memKey.n_cells * 4, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

int omds_get_cloud_objects(omds_ctx* ctx, int32_t* label, int32_t* object, int32_t* n_objects_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const CloudState& s = ctx->cloud;
    REQUIRE(ctx->n_obs > 0 && s.obj_label.size() == (size_t)ctx->n_obs, OMDS_ERR_NOT_INITIALISED,
            "omds_get_cloud_objects: the scene in force was not installed by omds_set_obstacles_from_cloud_objects");
    if (label) std::memcpy(label, s.obj_label.data(), (size_t)ctx->n_obs * 4);
    if (object) std::memcpy(object, s.obj_flag.data(), (size_t)ctx->n_obs * 4);
    if (n_objects_out) *n_objects_out = s.obj_count;
    return OMDS_OK;
}

int omds_velocity_filter_step(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const omds_velocity_filter_spec* filt,
                              const int32_t* state_in, const int32_t* cell, const float* raw, const int32_t* live, const int32_t* group, int32_t n,
                              float* vel_out, int32_t* state_out, int32_t stats_out[3]) {
    return velocity_filter_step_host(spec, track, filt, state_in, cell, raw, live, group, n, vel_out, state_out, stats_out, &g_create_err);
}

int omds_set_velocity_filter(omds_ctx* ctx, const omds_velocity_filter_spec* spec) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudState& s = ctx->cloud;
    if (!spec) {
        s.vfilter_on = false;
        s.vkey.grid.have = false;   // the history goes with the filter
        return OMDS_OK;
    }
    VelFilter f;
    if (int rc = velocity_filter_resolve(spec, &f, &ctx->err)) return rc;   // the stored filter stays as it was
    s.vfilter = f;
    s.vfilter_spec = *spec;
    s.vfilter_on = true;
    return OMDS_OK;
}

int omds_get_velocity_filter(omds_ctx* ctx, omds_velocity_filter_spec* spec_out, int32_t* on_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const CloudState& s = ctx->cloud;
    if (spec_out) *spec_out = s.vfilter_on ? s.vfilter_spec : omds_velocity_filter_spec{0.f, 0.f, 0.f};
    if (on_out) *on_out = s.vfilter_on ? 1 : 0;
    return OMDS_OK;
}

int omds_get_velocity_filter_frame(omds_ctx* ctx, float* raw, int32_t* live, int32_t stats[3]) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const CloudState& s = ctx->cloud;
    REQUIRE(ctx->n_obs > 0 && s.vf_have && s.vf_live.size() == (size_t)ctx->n_obs, OMDS_ERR_NOT_INITIALISED,
            "omds_get_velocity_filter_frame: the scene in force was not installed by a call under a velocity filter");
    if (raw) std::memcpy(raw, s.vf_raw.data(), (size_t)ctx->n_obs * 12);
    if (live) std::memcpy(live, s.vf_live.data(), (size_t)ctx->n_obs * 4);
    for (int k = 0; stats && k < 3; ++k) stats[k] = s.vf_stats[k];
    return OMDS_OK;
}

int omds_get_velocity_filter_state(omds_ctx* ctx, int32_t* grid, int32_t* n_cells_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudState& s = ctx->cloud;
    const bool have = s.vkey.grid.have;
    if (n_cells_out) *n_cells_out = have ? s.vkey.n_cells : 0;
    if (grid && have) {
        CK(hipSetDevice(ctx->dev));
        CK(hipMemcpyAsync(grid, s.vstate.kept(), (size_t)s.vkey.n_cells * 16, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipStreamSynchronize(ctx->stream));
    }
    return OMDS_OK;
}

int omds_cloud_track_reset(omds_ctx* ctx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    ctx->cloud.forget_tracking();
    return OMDS_OK;
}

}  // extern "C"
