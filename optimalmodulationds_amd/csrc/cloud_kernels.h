// What the host stages of the scene from a point cloud or from depth images (scene_cloud.hip) need of the cloud kernel files
// (cloud_kernels.hip, depth_kernels.hip, scene_memory_kernels.hip, cloud_track_kernels.hip, velocity_filter_kernels.hip; what they
// share on the device: cloud_device.h): the sizes they reserve buffers by, the camera table of the depth counting pass, and the
// launchers, each defined beside its kernel.  A launcher takes a stream and raw pointers, enqueues, and waits for nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "depth_def.h"
#include "point_cloud_objects_def.h"
#include "scene_memory_def.h"
#include "scene_memory_flow_def.h"
#include "velocity_filter_def.h"

constexpr int CLOUD_NT = 256;                          // lanes of every workgroup here
constexpr int CLOUD_ITEMS = 4;                         // consecutive items per lane of a compaction block
constexpr int CLOUD_BLOCK = CLOUD_NT * CLOUD_ITEMS;    // items per compaction block
constexpr int CLOUD_MAX_BLOCKS = (int)(OMDS_CLOUD_MAX_CELLS / CLOUD_BLOCK);   // 4096: what the one workgroup of k_compact_scan takes
static_assert(CLOUD_MAX_BLOCKS * CLOUD_BLOCK == OMDS_CLOUD_MAX_CELLS, "k_compact_scan takes every grid the spec allows");
constexpr int OBJ_ACC = 5;                             // uint64 words of a component's sums: m, N, Q[3]

inline int cloud_compaction_blocks(int n) { return (n + CLOUD_BLOCK - 1) / CLOUD_BLOCK; }
// the cells of a grid rounded up to whole compaction blocks: what the per-cell buffers (counts, records, slots) hold
inline size_t cloud_padded_cells(const CloudGrid& g) { return (size_t)cloud_compaction_blocks(g.n_cells) * CLOUD_BLOCK; }

struct DepthCamDev {
    DepthCam c;
    const void* image;     // device memory, element (0, 0)
    int runs;              // items per visited row: ceil(nu / DEPTH_RUN)       (these two are the launcher's to fill; the filtered
    long long items;       // runs * nv                                          pass: tiles per tile row, and the camera's tiles)
};
struct DepthTable {
    DepthCamDev cam[OMDS_DEPTH_MAX_CAMERAS];
};

// The counting pass, from P points xyz [P][3] or from the images of tab.cam[0 .. n_cams), into counts [cells] or into records [cells]
// (both cleared by the caller).  lt (depth_lens_def.h): nullptr when no camera of the call has a lens -- the pinhole kernels; else
// lt->cam[i] beside tab.cam[i], its ab the camera's ray table on the device or nullptr (pinhole arithmetic) -- the lens forms
void omds_launch_cloud_count(hipStream_t s, const float* xyz, long long P, const CloudGrid& g, unsigned* count);
void omds_launch_cloud_count(hipStream_t s, const float* xyz, long long P, const CloudGrid& g, uint4* rec);
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, unsigned* count);
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, uint4* rec);
// ... from the pixels of the images the depth filter f keeps (depth_filter_def.h); counters [2], cleared by the caller, takes the pixels
// the filter kept and those it rejected
void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, const DepthFilter& f,
                                      unsigned* count, unsigned* counters);
void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, const DepthFilter& f,
                                      uint4* rec, unsigned* counters);
// The ray table of camera c (fx, fy: the camera's) under lens l: ab [nv * nu][2]; red [2], cleared by the caller, takes the bits of the
// largest r2 of a valid ray and the pixels without a ray
void omds_launch_depth_rays(hipStream_t s, const DepthCam& c, float fx, float fy, const DepthLens& l, float* ab, unsigned* red);

// The ordered compactions, one per item space: the kept items to out (and what goes with them) in item order, at most cap of them
// written; sums [blocks of the item space + 1] is scratch, and sums[cloud_compaction_blocks(n)] holds the number of kept items after.
// ... the cells of g with min_points points and more (count / rec padded with zeros to cloud_padded_cells): their spheres, cap = g.max_spheres
void omds_launch_cloud_compact_cells(hipStream_t s, const unsigned* count, const CloudGrid& g, float4* out, unsigned* sums);
void omds_launch_cloud_compact_cells(hipStream_t s, const uint4* rec, const CloudGrid& g, float4* out, int* cell, unsigned* sums);
// ... the cells of g whose scene-memory word is not 0 (mem padded with zeros like count): their spheres and their cell indices
void omds_launch_cloud_compact_cells(hipStream_t s, const unsigned* mem, const CloudGrid& g, float4* out, int* cell, unsigned* sums);
// ... the n candidates the self-filter keeps at their pass-1 distances d [n]; with candCell their cell indices go to cell beside them
void omds_launch_cloud_compact_kept(hipStream_t s, const float* d, const float4* cand, const int* candCell, int n, float margin, int cap,
                                    float4* out, int* cell, unsigned* sums);
// ... the roots among the n spheres (root, acc: what omds_launch_cloud_components left): the component table, compOf[root] = its row
void omds_launch_cloud_compact_roots(hipStream_t s, const int* root, const int* cells, const unsigned long long* acc, int n, int cap,
                                     CloudComp* table, int* compOf, unsigned* sums);

// ... the spheres of a master scene the obstacle focus keeps (keys [n], res [4]: what omds_launch_focus_select left), in ascending
// master index: the sphere to out, its index to idx, and with vel [n][3] its velocity to velOut [cap][3]
void omds_launch_focus_compact(hipStream_t s, const unsigned* keys, const unsigned* res, const float4* master, const float* vel, int n, int cap,
                               float4* out, int* idx, float* velOut, unsigned* sums);
// The obstacle focus (obstacle_focus_kernels.hip).  keys [n]: the keys (obstacle_focus_def.h) of the reaches of distances d [n] and
// velocities vel [n][3] (nullptr: the distances themselves; dims < 3: v_z = 0)
void omds_launch_focus_keys(hipStream_t s, const float* d, const float* vel, int dims, float lookahead, int n, unsigned* keys);
// res [4]: kept, passing, the key of the last kept sphere of the order, the index up to which a sphere with that key is kept.  One workgroup
void omds_launch_focus_select(hipStream_t s, const unsigned* keys, int n, int n_closest, float margin, bool all_pass, int max_keep, unsigned* res);
// ... along a path, one chunk of C states: rows [C][n], pass 1's distances, become the keys of their reaches in place (time [C]:
// lookahead + ahead per state, read with vel); bars [C] is scratch; best [n] and pass [n], set to ~0 and 0 before the first chunk,
// take the nearest key of every sphere and whether it passed in some row
void omds_launch_focus_path_chunk(hipStream_t s, float* rows, const float* vel, int dims, const float* time, int C, int n, int n_closest, float margin,
                                  bool all_pass, unsigned* bars, unsigned* best, unsigned* pass);
// ... after the last chunk: sel [n] = the nearest key of a passing sphere, ~0 for the others, and res [4] as omds_launch_focus_select
// leaves it, for omds_launch_focus_compact on sel
void omds_launch_focus_path_select(hipStream_t s, const unsigned* best, const unsigned* pass, int n, int n_closest, int max_keep, unsigned* sel,
                                   unsigned* res);

// The scene memory (scene_memory_def.h).  mem_out [cloud_padded_cells]: the words of this call from the counts count and the stored
// words mem_in (both padded with zeros; mem_in == nullptr: all empty); counters [SCENE_MEM_COUNTS], cleared by the caller, takes the
// seen, remembered, cleared and expired cells.  lt as above: with it the verdicts of a camera with a lens go through its forward model
void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const DepthLensTable* lt, const SceneMemCams& ks, int n_cams, const CloudGrid& g,
                              const SceneMem& sm, const unsigned* count, const unsigned* mem_in, unsigned* mem_out, unsigned* counters);
// ... the same pass with the counts read out of the records rec (the .x of each; padded with zeros like count)
void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const DepthLensTable* lt, const SceneMemCams& ks, int n_cams, const CloudGrid& g,
                              const SceneMem& sm, const uint4* rec, const unsigned* mem_in, unsigned* mem_out, unsigned* counters);
// Memory and velocities in one call (scene_memory_flow_def.h).  One more ordered compaction: of the n spheres of the final list (their
// cells in cells) those whose cell has min_points points and more in the records now, in list order: the cell to cell, the index in
// the final list to idx; sums as above
void omds_launch_cloud_compact_seen(hipStream_t s, const uint4* now, const CloudGrid& g, const int* cells, int n, int* cell, int* idx,
                                    unsigned* sums);
// ... and the results of those n_seen spheres (velT as omds_launch_cloud_flow / omds_launch_cloud_apply left it, labelT, objectT; each
// may be nullptr: zeros, -1, 0) to their places in vel, label, object [n] under scene_memory_flow_still, which reads the STORED words
// mem_in (nullptr: all empty); the spheres outside them get velocity 0, label -1, object 0
void omds_launch_scene_memory_flow(hipStream_t s, const uint4* now, const CloudGrid& g, const unsigned* mem_in, const int* cells, int n,
                                   const int* idx, int n_seen, const float4* velT, const int* labelT, const int* objectT, float4* vel, int* label,
                                   int* object);
// ... mem[cell[i]] = 0 for every candidate i of n the self-filter drops at its pass-1 distance d[i]; counters[SCENE_MEM_FORGOTTEN] += them
void omds_launch_scene_memory_forget(hipStream_t s, const float* d, const int* cell, int n, float margin, unsigned* mem, unsigned* counters);
// ... age[i] = mem[cell[i]] - 1 for the n final spheres
void omds_launch_scene_memory_age(hipStream_t s, const unsigned* mem, const int* cell, int n, int* age);

// vel [n]: the velocity of every final sphere (its cell in cells) from the records of this frame and the previous one
void omds_launch_cloud_flow(hipStream_t s, const CloudGrid& g, const CloudTrack& tr, const uint4* now, const uint4* prev, const int* cells, int n,
                            float4* vel);
// the components of the n final spheres: slot [cloud_padded_cells] and acc [n][OBJ_ACC] are cleared here; after it parent [n] is
// every sphere's root, label [n] its component's label and acc the sums at the roots
void omds_launch_cloud_components(hipStream_t s, const CloudGrid& g, int link, const uint4* now, const int* cells, int n, int* slot, int* parent,
                                  int* label, unsigned long long* acc);
// objVel [n_now]: every component of the table now against the table prev (n_prev = 0: nothing to match)
void omds_launch_cloud_match(hipStream_t s, const CloudGrid& g, const CloudTrack& tr, const CloudObjects& ob, const CloudComp* now, int n_now,
                             const CloudComp* prev, int n_prev, float4* objVel);
// the velocities of the accepted objects over vel [n], object [n] = 1 on their spheres
void omds_launch_cloud_apply(hipStream_t s, const int* root, const int* compOf, const float4* objVel, int n, float4* vel, int* object);

// The velocity filter (velocity_filter_def.h).  state[cells[i]] = no history for the n cells the buffer last held (n = 0: no launch)
void omds_launch_vel_clear(hipStream_t s, const int* cells, int n, int4* state);
// ... the stage on the n > 0 final spheres (their cells in cells, ascending): vel [n] as the velocity stages left it (.w: the matched
// flag) against the stored state state_in [cells] (nullptr: an empty history) -> out [n] the filtered velocities, .w kept, and
// state_out [cells] (all zero before the call) the records of the live spheres; held [n] = cells, for the next omds_launch_vel_clear
// of that buffer.  label, object [n]: the spheres with object = 1 blend as the group of their label (object == nullptr: no groups,
// and no group launch); pred [n], group [n][VEL_GROUP_ACC] and groupH [n] are scratch.  counters [3], cleared by the caller, takes the
// live spheres with history, the restarts and the groups with history
void omds_launch_vel_filter(hipStream_t s, const CloudGrid& g, const CloudTrack& tr, const VelFilter& f, const int4* state_in, const int* cells,
                            int n, const float4* vel, const int* label, const int* object, VelPred* pred, unsigned long long* group, int* groupH,
                            int4* state_out, int* held, float4* out, unsigned* counters);
