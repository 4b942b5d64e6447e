// The velocities of a tracked scene call (the layout of the cloud kernel files: cloud_kernels.hip; the launchers: cloud_kernels.h).
// k_cloud_flow evaluates point_cloud_flow_def.h against the records of the previous tracked frame with one wave per final sphere.  The
// objects form adds the launches of point_cloud_objects_def.h: slot map, union-find, flatten, component sums, the component table by
// the ordered compaction (RootSrc), one wave per component for the match against the stored table, and the object velocities over
// k_cloud_flow's.
#include "cloud_device.h"

namespace {

// The velocity of every final sphere (point_cloud_flow_def.h): one wave per sphere, four per workgroup, no barrier.  A first probe
// of the sphere's own cell in the previous frame settles the common case (d2 = 0 is the unique minimum).  Otherwise the lanes stride
// over the window clipped to the grid, x innermost; each keeps the sums of its own cells at its own smallest d2, the wave takes the
// minimum, lanes above it drop their sums, and the rest is added up by shuffles -- integers throughout, so the schedule cannot change
// a bit.  Lane 0 then evaluates the fp32 lines of the definition; vel[sphere].w = 1 where the window was not empty (the host counts
// them: one counter for all spheres would serialise 30 000 atomics on one address, 0.34 ms at the scene of EXPERIMENTS R18).
__global__ __launch_bounds__(CLOUD_NT) void k_cloud_flow(CloudGrid g, CloudTrack tr, const uint4* __restrict__ now, const uint4* __restrict__ prev,
                                                         const int* __restrict__ cells, int n_spheres, float4* __restrict__ vel) {
    const int lane = threadIdx.x & 63, sphere = blockIdx.x * FLOW_WAVES + (threadIdx.x >> 6);
    if (sphere >= n_spheres) return;   // a whole wave
    const int cell = cells[sphere];
    CloudFlowSums a;
    cloud_flow_clear(a);
    const uint4 own = prev[cell];
    if (own.x >= g.min_points) {
        cloud_flow_add(a, 0, 0, 0, own.x, own.y, own.z, own.w);
    } else {
        const int ix = cell % g.dx, iy = (cell / g.dx) % g.dy, iz = cell / (g.dx * g.dy);
        const int x0 = max(ix - tr.reach, 0), y0 = max(iy - tr.reach, 0), z0 = max(iz - tr.reach, 0);
        const int wx = min(ix + tr.reach, g.dx - 1) - x0 + 1, wy = min(iy + tr.reach, g.dy - 1) - y0 + 1, wz = min(iz + tr.reach, g.dz - 1) - z0 + 1;
        for (int i = lane; i < wx * wy * wz; i += 64) {
            const int x = x0 + i % wx, y = y0 + (i / wx) % wy, z = z0 + i / (wx * wy);
            const uint4 p = prev[(z * g.dy + y) * g.dx + x];
            if (p.x >= g.min_points) cloud_flow_add(a, x - ix, y - iy, z - iz, p.x, p.y, p.z, p.w);
        }
        const unsigned best = wave_min(a.d2);
        if (a.d2 != best) cloud_flow_clear(a);
        a.d2 = best;
        a.t = wave_sum(a.t);
        a.N = wave_sum(a.N);
        for (int c = 0; c < 3; ++c) {
            a.A[c] = wave_sum(a.A[c]);
            a.P[c] = wave_sum(a.P[c]);
        }
    }
    if (lane != 0) return;
    float v[3] = {0.f, 0.f, 0.f};
    const bool matched = a.d2 != OMDS_CLOUD_NO_MATCH;
    if (matched) {
        const uint4 r = now[cell];
        const unsigned s[3] = {r.y, r.z, r.w};
        cloud_flow_velocity(g, tr, r.x, s, a, v);
    }
    vel[sphere] = make_float4(v[0], v[1], v[2], matched ? 1.f : 0.f);
}

// ---- the objects of the final list (point_cloud_objects_def.h) ---------------------------------------------------------------------
// slot[cell] = list index of the final sphere in that cell (the rest of the grid was cleared to -1), and every sphere its own root
__global__ __launch_bounds__(CLOUD_NT) void k_obj_slot(const int* __restrict__ cells, int n, int* __restrict__ slot, int* __restrict__ parent) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (i >= n) return;
    slot[cells[i]] = i;
    parent[i] = i;
}

// The union-find.  Invariants: parent[x] <= x, and an entry that has stopped being a root (parent[x] != x) never becomes one again.
// Loads and stores are relaxed device-scope atomics, so that no lane works on a cached copy of another workgroup's hook.
__device__ inline int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void uf_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see; x strictly decreases, so the loop ends after at most x steps.  Path halving: the
// grandparent of a non-root is one of its ancestors and stays one, whatever is hooked meanwhile (hooks only act on roots)
__device__ inline int uf_find(int* parent, int x) {
    for (;;) {
        const int p = uf_load(parent + x);
        if (p == x) return x;
        const int gp = uf_load(parent + p);
        if (gp != p) uf_store(parent + x, gp);
        x = p;
    }
}

// Unite the components of a and b: hook the larger root under the smaller by compare-and-swap.  A swap that fails means another
// lane has hooked that root in the meantime; the search resumes from there, and max(a, b) is strictly smaller than before: the loop
// ends on this lane's own progress and waits for nobody.  Returns the root both are under now
__device__ inline int uf_unite(int* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return b;
    }
}

// one lane per sphere: unite with every final sphere in the lower half of its window (the upper half is the other sphere's).  The
// list is in cell order, so hooking larger under smaller leaves the component's smallest cell as its root
__global__ __launch_bounds__(CLOUD_NT) void k_obj_union(CloudGrid g, int link, const int* __restrict__ cells, int n, const int* __restrict__ slot,
                                                        int* parent) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (i >= n) return;
    int mine = i;   // an ancestor of i: where the next search for its root starts
    cloud_lower_neighbours(g, link, cells[i], [&](int cell, bool implied) {
        const int j = slot[cell];
        if (j < 0) return false;
        if (!implied) mine = uf_unite(parent, mine, j);
        return true;
    });
}

// the root of x by a walk that stores nothing
__device__ inline int uf_root(const int* parent, int x) {
    for (;;) {
        const int p = uf_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// parent[i] = root of i, label[i] = the root's cell.  INVARIANT: in this launch entry i is stored to by lane i alone, once, and the
// value is the root -- the searches here halve no path (a halving store of another lane, landing late, could put a mere ancestor
// back over the root).  A concurrent walk reads either the old ancestor or the root at i: both lead to the root.  After this launch
// parent[] IS the root of every sphere, which is what k_obj_sums, RootSrc and k_obj_apply take it for
__global__ __launch_bounds__(CLOUD_NT) void k_obj_flatten(const int* __restrict__ cells, int n, int* parent, int* __restrict__ label) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (i >= n) return;
    const int r = uf_root(parent, i);
    if (r != i) uf_store(parent + i, r);
    label[i] = cells[r];
}

// The component sums m, N, Q[3] at acc[root][5], all uint64.  A dense scene is one or two huge components: every sphere's five atomics
// would land on the same five words, and atomics from different waves on one word cost 80 ns and more each (EXPERIMENTS R19).  So
// equal roots are combined before memory is touched, in three steps: the list is in cell order, so every run of equal roots inside a
// wave is added up by a segmented shuffle scan; the runs of the wave's DOMINANT root (that of its first lane: the huge component,
// whose runs small components interrupt) are added up by a shuffle sum; and the dominant sums of the sixteen waves of the workgroup
// meet in LDS, from where each distinct root goes to memory once.  What is left for the atomics is one set per workgroup for a huge
// component and one per run for the small ones.  Integers throughout: no order can change a bit
__global__ __launch_bounds__(SUMS_NT) void k_obj_sums(CloudGrid g, const uint4* __restrict__ now, const int* __restrict__ cells,
                                                      const int* __restrict__ root, int n, unsigned long long* __restrict__ acc) {
    __shared__ int key[SUMS_WAVES];
    __shared__ unsigned long long part[SUMS_WAVES][OBJ_ACC];
    const int i = blockIdx.x * SUMS_NT + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int r = -1;
    unsigned long long v[OBJ_ACC] = {0ull, 0ull, 0ull, 0ull, 0ull};
    if (i < n) {
        r = root[i];
        const int cell = cells[i];
        const uint4 rec = now[cell];
        v[0] = 1ull;
        v[1] = rec.x;
        v[2] = cloud_comp_q(cell % g.dx, rec.x, rec.y);
        v[3] = cloud_comp_q((cell / g.dx) % g.dy, rec.x, rec.z);
        v[4] = cloud_comp_q(cell / (g.dx * g.dy), rec.x, rec.w);
    }
    const int before = __shfl_up(r, 1, 64);
    const bool head = lane == 0 || before != r;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run_end = above ? lane + __ffsll((long long)above) : 64;   // the next head, exclusive end of this lane's run
    for (int d = 1; d < 64; d <<= 1)
        for (int k = 0; k < OBJ_ACC; ++k) {
            const unsigned long long o = __shfl_down(v[k], d, 64);
            if (lane + d < run_end) v[k] += o;
        }
    const int dominant = __shfl(r, 0, 64);   // -1: the whole wave lies past the list
    const bool first = head && r >= 0, joins = first && r == dominant;
    for (int k = 0; k < OBJ_ACC; ++k) {
        const unsigned long long d = wave_sum(joins ? v[k] : 0ull);
        if (lane == 0) part[wave][k] = d;
    }
    if (lane == 0) key[wave] = dominant;
    if (first && !joins)
        for (int k = 0; k < OBJ_ACC; ++k) atomicAdd(acc + (size_t)r * OBJ_ACC + k, v[k]);
    __syncthreads();
    if (threadIdx.x >= SUMS_WAVES || key[threadIdx.x] < 0) return;
    const int mine = key[threadIdx.x];
    for (int w = 0; w < (int)threadIdx.x; ++w)
        if (key[w] == mine) return;   // an earlier wave speaks for this root
    for (int k = 0; k < OBJ_ACC; ++k) {
        unsigned long long s = 0ull;
        for (int w = threadIdx.x; w < SUMS_WAVES; ++w)
            if (key[w] == mine) s += part[w][k];
        atomicAdd(acc + (size_t)mine * OBJ_ACC + k, s);
    }
}

// the roots as an item space of the ordered compaction: the component table in ascending label order
struct RootSrc {
    const int* root;
    const int* cells;
    const unsigned long long* acc;
    CloudComp* table;
    int* compOf;
    __device__ unsigned flags(int base, int n) const {
        unsigned f = 0;
        for (int j = 0; j < CLOUD_ITEMS; ++j)
            if (base + j < n && root[base + j] == base + j) f |= 1u << j;
        return f;
    }
    __device__ void emit(int item, unsigned pos) const {
        const unsigned long long* a = acc + (size_t)item * OBJ_ACC;
        table[pos] = CloudComp{cells[item], (unsigned)a[0], a[1], {a[2], a[3], a[4]}};
        compOf[item] = (int)pos;
    }
};

// One wave per NOW component.  A component of fewer than min_cells cells is no object (.w = 0).  Else the lanes stride over the
// previous table in the definition's fp64 statements, the wave takes the minimum of (d2, label), and lane 0 applies the gates and the
// velocity lines: .w = 2 with the object's velocity when accepted, else .w = 1
__global__ __launch_bounds__(CLOUD_NT) void k_obj_match(CloudGrid g, CloudTrack tr, CloudObjects ob, const CloudComp* __restrict__ now, int n_now,
                                                        const CloudComp* __restrict__ prev, int n_prev, float4* __restrict__ objVel) {
    const int lane = threadIdx.x & 63, comp = blockIdx.x * FLOW_WAVES + (threadIdx.x >> 6);
    if (comp >= n_now) return;   // a whole wave
    const CloudComp c = now[comp];
    if (c.m < ob.min_cells) {
        if (lane == 0) objVel[comp] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    double cn[3], cp[3], best_d2 = 0.0;
    int best = -1, best_label = 0;
    cloud_comp_centroid(c, cn);
    for (int j = lane; j < n_prev; j += 64) {
        const CloudComp p = prev[j];
        if (p.m < ob.min_cells) continue;
        cloud_comp_centroid(p, cp);
        const double d2 = cloud_object_d2(cn, cp);
        if (best < 0 || cloud_object_closer(d2, p.label, best_d2, best_label)) { best = j; best_d2 = d2; best_label = p.label; }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const double o_d2 = __shfl_xor(best_d2, d, 64);
        const int o_best = __shfl_xor(best, d, 64), o_label = __shfl_xor(best_label, d, 64);
        if (o_best >= 0 && (best < 0 || cloud_object_closer(o_d2, o_label, best_d2, best_label))) { best = o_best; best_d2 = o_d2; best_label = o_label; }
    }
    if (lane != 0) return;
    float v[3] = {0.f, 0.f, 0.f};
    float state = 1.f;
    if (best >= 0) {
        const CloudComp p = prev[best];
        if (cloud_object_accept(tr, c.m, p.m, best_d2)) {
            cloud_comp_centroid(p, cp);
            cloud_object_velocity(g, tr, cn, cp, v);
            state = 2.f;
        }
    }
    objVel[comp] = make_float4(v[0], v[1], v[2], state);
}

// every sphere of an accepted object takes the object's velocity over k_cloud_flow's and counts as matched
__global__ __launch_bounds__(CLOUD_NT) void k_obj_apply(const int* __restrict__ root, const int* __restrict__ compOf, const float4* __restrict__ objVel,
                                                        int n, float4* __restrict__ vel, int* __restrict__ object) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (i >= n) return;
    const float4 o = objVel[compOf[root[i]]];
    const bool accepted = o.w == 2.f;
    if (accepted) vel[i] = make_float4(o.x, o.y, o.z, 1.f);
    object[i] = accepted ? 1 : 0;
}

}  // namespace

void omds_launch_cloud_flow(hipStream_t s, const CloudGrid& g, const CloudTrack& tr, const uint4* now, const uint4* prev, const int* cells, int n,
                            float4* vel) {
    hipLaunchKernelGGL(k_cloud_flow, dim3((n + FLOW_WAVES - 1) / FLOW_WAVES), dim3(CLOUD_NT), 0, s, g, tr, now, prev, cells, n, vel);
}

void omds_launch_cloud_components(hipStream_t s, const CloudGrid& g, int link, const uint4* now, const int* cells, int n, int* slot, int* parent,
                                  int* label, unsigned long long* acc) {
    const int blocks = (n + CLOUD_NT - 1) / CLOUD_NT;
    (void)hipMemsetAsync(slot, 0xff, cloud_padded_cells(g) * 4, s);   // -1.  (A failure is the caller's hipGetLastError, like a launch's)
    (void)hipMemsetAsync(acc, 0, (size_t)n * OBJ_ACC * 8, s);
    hipLaunchKernelGGL(k_obj_slot, dim3(blocks), dim3(CLOUD_NT), 0, s, cells, n, slot, parent);
    hipLaunchKernelGGL(k_obj_union, dim3(blocks), dim3(CLOUD_NT), 0, s, g, link, cells, n, (const int*)slot, parent);
    hipLaunchKernelGGL(k_obj_flatten, dim3(blocks), dim3(CLOUD_NT), 0, s, cells, n, parent, label);
    hipLaunchKernelGGL(k_obj_sums, dim3((n + SUMS_NT - 1) / SUMS_NT), dim3(SUMS_NT), 0, s, g, now, cells, (const int*)parent, n, acc);
}

void omds_launch_cloud_match(hipStream_t s, const CloudGrid& g, const CloudTrack& tr, const CloudObjects& ob, const CloudComp* now, int n_now,
                             const CloudComp* prev, int n_prev, float4* objVel) {
    hipLaunchKernelGGL(k_obj_match, dim3((n_now + FLOW_WAVES - 1) / FLOW_WAVES), dim3(CLOUD_NT), 0, s, g, tr, ob, now, n_now, prev, n_prev, objVel);
}

void omds_launch_cloud_apply(hipStream_t s, const int* root, const int* compOf, const float4* objVel, int n, float4* vel, int* object) {
    hipLaunchKernelGGL(k_obj_apply, dim3((n + CLOUD_NT - 1) / CLOUD_NT), dim3(CLOUD_NT), 0, s, root, compOf, objVel, n, vel, object);
}

void omds_launch_cloud_compact_roots(hipStream_t s, const int* root, const int* cells, const unsigned long long* acc, int n, int cap,
                                     CloudComp* table, int* compOf, unsigned* sums) {
    compact(s, RootSrc{root, cells, acc, table, compOf}, n, cap, sums);
}
