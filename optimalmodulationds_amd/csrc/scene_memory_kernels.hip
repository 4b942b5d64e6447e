// The scene memory of the depth route (the layout of the cloud kernel files: cloud_kernels.hip; the launchers: cloud_kernels.h).
// One more pass over the cells behind the counting pass (scene_memory_def.h; k_scene_memory), the cells with a word as an item space
// of the ordered compaction (MemSrc) and two small launches over the candidates (k_scene_memory_forget, k_scene_memory_age).  Memory
// and velocities in one call (scene_memory_flow_def.h): the same pass reading the counts out of the records (k_scene_memory<uint4>),
// the seen sublist as another item space (SeenSrc), and one launch that carries its results back to the final list
// (k_scene_memory_flow).
#include <algorithm>

#include "cloud_device.h"

namespace {

// ---- the scene memory of the depth route (scene_memory_def.h) ----------------------------------------------------------------------
// One pass over the cells behind the counting pass: a lane owns 4 consecutive cells (one 16-byte load of the counts, one of the stored
// words, one 16-byte store of the new words) and the workgroups stride over the padded cells, so the padding comes out 0 too.  A lane
// whose four stored words are 0 -- nearly every lane of a large grid -- projects nothing and reads no image.  The others ask the
// cameras of the table, which travels by value like the counting pass's; every camera is asked, so the table index stays uniform.
// The lanes of a wave diverge there (accepted: a few thousand remembered cells against millions of empty ones).  A streaming kernel:
// no LDS, no barrier.  The counters are integers, reduced per wave before one atomic each: no order can change them
struct TableCams {
    const DepthTable& t;
    __device__ const DepthCam& cam(int i) const { return t.cam[i].c; }
    __device__ const void* image(int i) const { return t.cam[i].image; }
};
constexpr unsigned MEM_MAX_BLOCKS = 2048;
// the counts of the four cells from base on: one 16-byte load of the plain counting pass's counts, or the .x of four consecutive
// 16-byte records of the tracked one's (the combined route: the same counting pass serves the memory and the velocities)
__device__ inline uint4 scene_memory_counts(const unsigned* count, int base) { return *reinterpret_cast<const uint4*>(count + base); }
__device__ inline uint4 scene_memory_counts(const uint4* rec, int base) {
    return make_uint4(rec[base].x, rec[base + 1].x, rec[base + 2].x, rec[base + 3].x);
}
// The KERNEL is the template: k_scene_memory<unsigned> compiles to the instructions the memory route's kernel had before there was a
// second form; the body as a __device__ function called by two kernels did not (the compiler unrolled the camera loop another way).
// The LENS FORM (depth_lens_def.h), launched only when some camera of the call has a lens, is the same template with the lens table of
// the call by value as a trailing parameter pack LT = {DepthLensTable}: the verdicts through scene_memory_cell<true>.  The pack is
// TRAILING so that the pinhole instantiations (LT empty) keep the kernel arguments, and with them the instructions, they had as the
// only form (717 / 720 instructions; the lens instantiations 774 / 777, what k_scene_memory_lens was).  Both tables in one struct by
// value took the lens kernels to about 1 980 instructions on a scratch copy (EXPERIMENTS R34)
__device__ inline const DepthLensTable* lens_of() { return nullptr; }
__device__ inline const DepthLensTable* lens_of(const DepthLensTable& lt) { return &lt; }
template <class N, class... LT>   // N = unsigned: counts, uint4: records
__global__ __launch_bounds__(CLOUD_NT) void k_scene_memory(DepthTable tab, SceneMemCams ks, int n_cams, CloudGrid g, SceneMem sm,
                                                           const N* __restrict__ count, const unsigned* __restrict__ mem_in,
                                                           unsigned* __restrict__ mem_out, int groups, unsigned* __restrict__ counters, LT... lt) {
    const TableCams cams{tab};
    unsigned tally[4] = {0u, 0u, 0u, 0u};
    for (int i = blockIdx.x * CLOUD_NT + threadIdx.x; i < groups; i += gridDim.x * CLOUD_NT) {
        const int base = i * CLOUD_ITEMS;
        const uint4 n4 = scene_memory_counts(count, base);
        const uint4 m4 = mem_in ? *reinterpret_cast<const uint4*>(mem_in + base) : make_uint4(0u, 0u, 0u, 0u);
        const unsigned n[CLOUD_ITEMS] = {n4.x, n4.y, n4.z, n4.w}, m[CLOUD_ITEMS] = {m4.x, m4.y, m4.z, m4.w};
        unsigned out[CLOUD_ITEMS];
        if ((m4.x | m4.y | m4.z | m4.w) == 0u) {
            for (int j = 0; j < CLOUD_ITEMS; ++j) {
                out[j] = (base + j < g.n_cells && n[j] >= g.min_points) ? 1u : 0u;
                tally[SCENE_MEM_SEEN] += out[j];
            }
        } else {
            for (int j = 0; j < CLOUD_ITEMS; ++j) {
                int what = -1;
                out[j] = base + j < g.n_cells
                             ? scene_memory_cell<sizeof...(LT) != 0>(g, sm, cams, ks, n_cams, base + j, n[j], m[j], &what, lens_of(lt...))
                             : 0u;
                for (int k = 0; k < 4; ++k) tally[k] += what == k ? 1u : 0u;
            }
        }
        *reinterpret_cast<uint4*>(mem_out + base) = make_uint4(out[0], out[1], out[2], out[3]);
    }
    for (int k = 0; k < 4; ++k) {
        const unsigned sum = wave_sum(tally[k]);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(counters + k, sum);
    }
}

// the candidates the self-filter drops (cloud_keep's rule at the same distances the second compaction reads) leave the memory
__global__ __launch_bounds__(CLOUD_NT) void k_scene_memory_forget(const float* __restrict__ d, const int* __restrict__ cell, int n, float margin,
                                                                  unsigned* __restrict__ mem, unsigned* __restrict__ counters) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    const bool drop = i < n && !cloud_keep(d[i], margin);
    if (drop) mem[cell[i]] = 0u;
    const unsigned sum = wave_sum(drop ? 1u : 0u);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(counters + SCENE_MEM_FORGOTTEN, sum);
}

__global__ __launch_bounds__(CLOUD_NT) void k_scene_memory_age(const unsigned* __restrict__ mem, const int* __restrict__ cell, int n,
                                                               int* __restrict__ age) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (i < n) age[i] = (int)(mem[cell[i]] - 1u);
}

// ---- memory and velocities in one call (scene_memory_flow_def.h) -------------------------------------------------------------------
// T, the final spheres whose cell was counted now, as one more item space of the ordered compaction: items = the final list; each
// kept one leaves its cell and its index in the final list.  T is in cell order like the list, which the union-find relies on
struct SeenSrc {
    const uint4* now;
    const int* cells;
    unsigned min_points;
    int* cell;
    int* idx;
    __device__ unsigned flags(int base, int n) const {
        unsigned f = 0;
        for (int j = 0; j < CLOUD_ITEMS; ++j)
            if (base + j < n && now[cells[base + j]].x >= min_points) f |= 1u << j;
        return f;
    }
    __device__ void emit(int item, unsigned pos) const {
        cell[pos] = cells[item];
        idx[pos] = item;
    }
};

// T's results back to the final list under scene_memory_flow_still: one lane per final sphere, every output written by exactly one
// lane.  Lane j < n_seen carries T sphere j to its place idx[j]; lane i whose own sphere is not in T writes the remembered sphere's
// values at i (a sphere in T is written by the lane that carries it, wherever that lane is).  vel.w stays the matched flag k_cloud_flow
// and k_obj_apply left, 0 where the rule overrides, so the host still counts.  velT / labelT / objectT == nullptr: no previous frame /
// no object spec / no stored table
__global__ __launch_bounds__(CLOUD_NT) void k_scene_memory_flow(const uint4* __restrict__ now, unsigned min_points, const unsigned* __restrict__ mem_in,
                                                                const int* __restrict__ cells, int n, const int* __restrict__ idx, int n_seen,
                                                                const float4* __restrict__ velT, const int* __restrict__ labelT,
                                                                const int* __restrict__ objectT, float4* __restrict__ vel,
                                                                int* __restrict__ label, int* __restrict__ object) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (i >= n) return;
    if (i < n_seen) {
        const int at = idx[i];
        const bool still = scene_memory_flow_still(true, mem_in ? mem_in[cells[at]] : 0u);
        vel[at] = (still || !velT) ? make_float4(0.f, 0.f, 0.f, 0.f) : velT[i];
        label[at] = labelT ? labelT[i] : -1;
        object[at] = (still || !objectT) ? 0 : objectT[i];
    }
    if (scene_memory_flow_still(now[cells[i]].x >= min_points, 0u)) {
        vel[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        label[i] = -1;
        object[i] = 0;
    }
}

// the cells with a memory word as an item space of the ordered compaction: the candidates of a memory call, with their cell indices
struct MemSrc {             // items = cells; mem is zero-padded to whole blocks like count, kept are the words that are not 0
    const unsigned* mem;
    CloudGrid g;
    float4* out;
    int* cell;
    __device__ unsigned flags(int base, int) const {
        const uint4 m = *reinterpret_cast<const uint4*>(mem + base);
        return (m.x ? 1u : 0u) | (m.y ? 2u : 0u) | (m.z ? 4u : 0u) | (m.w ? 8u : 0u);
    }
    __device__ void emit(int item, unsigned pos) const {
        float s[4];
        cloud_sphere(g, item, s);
        out[pos] = make_float4(s[0], s[1], s[2], s[3]);
        cell[pos] = item;
    }
};

// one launcher of both count forms; lt == nullptr: the pinhole instantiation
template <class N>
void launch_scene_memory(hipStream_t s, const DepthTable& tab, const DepthLensTable* lt, const SceneMemCams& ks, int n_cams, const CloudGrid& g,
                         const SceneMem& sm, const N* count, const unsigned* mem_in, unsigned* mem_out, unsigned* counters) {
    const int groups = (int)(cloud_padded_cells(g) / CLOUD_ITEMS);   // a multiple of CLOUD_NT
    const dim3 blocks(std::min((unsigned)(groups / CLOUD_NT), MEM_MAX_BLOCKS));
    if (lt)
        hipLaunchKernelGGL((k_scene_memory<N, DepthLensTable>), blocks, dim3(CLOUD_NT), 0, s, tab, ks, n_cams, g, sm, count, mem_in, mem_out, groups,
                           counters, *lt);
    else hipLaunchKernelGGL(k_scene_memory<N>, blocks, dim3(CLOUD_NT), 0, s, tab, ks, n_cams, g, sm, count, mem_in, mem_out, groups, counters);
}

}  // namespace

void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const DepthLensTable* lt, const SceneMemCams& ks, int n_cams, const CloudGrid& g,
                              const SceneMem& sm, const unsigned* count, const unsigned* mem_in, unsigned* mem_out, unsigned* counters) {
    launch_scene_memory(s, tab, lt, ks, n_cams, g, sm, count, mem_in, mem_out, counters);
}
void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const DepthLensTable* lt, const SceneMemCams& ks, int n_cams, const CloudGrid& g,
                              const SceneMem& sm, const uint4* rec, const unsigned* mem_in, unsigned* mem_out, unsigned* counters) {
    launch_scene_memory(s, tab, lt, ks, n_cams, g, sm, rec, mem_in, mem_out, counters);
}
void omds_launch_cloud_compact_seen(hipStream_t s, const uint4* now, const CloudGrid& g, const int* cells, int n, int* cell, int* idx,
                                    unsigned* sums) {
    compact(s, SeenSrc{now, cells, g.min_points, cell, idx}, n, g.max_spheres, sums);
}
void omds_launch_scene_memory_flow(hipStream_t s, const uint4* now, const CloudGrid& g, const unsigned* mem_in, const int* cells, int n,
                                   const int* idx, int n_seen, const float4* velT, const int* labelT, const int* objectT, float4* vel, int* label,
                                   int* object) {
    if (n > 0)
        hipLaunchKernelGGL(k_scene_memory_flow, dim3((n + CLOUD_NT - 1) / CLOUD_NT), dim3(CLOUD_NT), 0, s, now, g.min_points, mem_in, cells, n, idx,
                           n_seen, velT, labelT, objectT, vel, label, object);
}
void omds_launch_scene_memory_forget(hipStream_t s, const float* d, const int* cell, int n, float margin, unsigned* mem, unsigned* counters) {
    if (n > 0) hipLaunchKernelGGL(k_scene_memory_forget, dim3((n + CLOUD_NT - 1) / CLOUD_NT), dim3(CLOUD_NT), 0, s, d, cell, n, margin, mem, counters);
}
void omds_launch_scene_memory_age(hipStream_t s, const unsigned* mem, const int* cell, int n, int* age) {
    if (n > 0) hipLaunchKernelGGL(k_scene_memory_age, dim3((n + CLOUD_NT - 1) / CLOUD_NT), dim3(CLOUD_NT), 0, s, mem, cell, n, age);
}

void omds_launch_cloud_compact_cells(hipStream_t s, const unsigned* mem, const CloudGrid& g, float4* out, int* cell, unsigned* sums) {
    compact(s, MemSrc{mem, g, out, cell}, g.n_cells, g.max_spheres, sums);
}
