// The scene from a depth point cloud (omds.h: omds_point_cloud_spheres, omds_set_obstacles_from_cloud): the workspace crop and the
// voxel down-sample as one counting pass over the points (k_cloud_count, integer atomics) and an ordered compaction of the occupied
// cells (k_compact_sums -> k_compact_scan -> k_compact_emit), the robot self-filter as ONE fp32 pass-1 launch over one state with the
// candidates as its obstacle rows (the launch the shared first step of a propagate uses) and a second compaction of those it keeps.
// The arithmetic of a cell and of its sphere is point_cloud_def.h's, shared with the host definition.  The final list goes to the host
// (a few thousand x 16 bytes) and from there through install_obstacles, the body of omds_set_obstacles (context.hip).
// The tracked form (omds_set_obstacles_from_cloud_tracked) counts into records of 16 bytes per cell (k_cloud_count_rec), carries each
// candidate's cell index through both compactions, and evaluates point_cloud_flow_def.h against the records of the previous tracked
// frame with one wave per final sphere (k_cloud_flow); the velocities then go in through omds_set_obstacle_motion.
// The objects form (omds_set_obstacles_from_cloud_objects) is the tracked one with the launches of point_cloud_objects_def.h between
// k_cloud_flow and the install: slot map, union-find, flatten, component sums, the component table by the same ordered compaction, one
// wave per component for the match against the stored table, and the object velocities over k_cloud_flow's.
// The depth form (omds_set_obstacles_from_depth) is any of the three with another POINT SOURCE: the counting pass deprojects the
// pixels of up to eight depth images itself (depth_def.h; k_depth_count, k_depth_count_rec) and no point is ever written.
#include "capi_internal.h"
#include "depth_def.h"
#include "point_cloud_objects_def.h"

namespace {

constexpr int CLOUD_NT = 256;                          // lanes of every workgroup here
constexpr int CLOUD_ITEMS = 4;                         // consecutive items per lane of a compaction block
constexpr int CLOUD_BLOCK = CLOUD_NT * CLOUD_ITEMS;    // items per compaction block
constexpr int CLOUD_MAX_BLOCKS = (int)(OMDS_CLOUD_MAX_CELLS / CLOUD_BLOCK);   // 4096: what the one workgroup of k_compact_scan takes

// one pass over the points: the crop is cloud_cell's range test, the down-sample the count per cell
__global__ __launch_bounds__(CLOUD_NT) void k_cloud_count(const float* __restrict__ xyz, long long P, CloudGrid g, unsigned* __restrict__ count) {
    for (long long i = (long long)blockIdx.x * CLOUD_NT + threadIdx.x; i < P; i += (long long)gridDim.x * CLOUD_NT) {
        const int cell = cloud_cell(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
        if (cell >= 0) atomicAdd(&count[cell], 1u);
    }
}

// ... of the tracked call: the same crop, and per kept point the record (n, s_x, s_y, s_z) of its cell, four integer atomics
__global__ __launch_bounds__(CLOUD_NT) void k_cloud_count_rec(const float* __restrict__ xyz, long long P, CloudGrid g, uint4* __restrict__ rec) {
    for (long long i = (long long)blockIdx.x * CLOUD_NT + threadIdx.x; i < P; i += (long long)gridDim.x * CLOUD_NT) {
        unsigned k[3];
        const int cell = cloud_cell_sub(g, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], k);
        if (cell < 0) continue;
        unsigned* r = reinterpret_cast<unsigned*>(rec + cell);
        atomicAdd(r, 1u);
        atomicAdd(r + 1, k[0]);
        atomicAdd(r + 2, k[1]);
        atomicAdd(r + 3, k[2]);
    }
}

// exclusive prefix of v over the 256 lanes of the workgroup in lane order, and their sum: a shuffle scan inside each wave, the four
// wave sums through LDS
__device__ inline unsigned block_exclusive_scan(unsigned v, unsigned* wsum, unsigned* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned pre = 0, tot = 0;
    for (int i = 0; i < CLOUD_NT / 64; ++i) {
        const unsigned s = wsum[i];
        if (i < w) pre += s;
        tot += s;
    }
    __syncthreads();   // wsum may be written again
    *total = tot;
    return pre + inc - v;
}

// The two item spaces that are compacted.  flags(base, n): bit j set when item base + j is kept; emit(item, pos): its sphere to out[pos]
struct CellSrc {            // items = cells; count is zero-padded to whole blocks, so no lane reads past it
    const unsigned* count;
    CloudGrid g;
    float4* out;
    __device__ unsigned flags(int base, int) const {
        const uint4 c = *reinterpret_cast<const uint4*>(count + base);
        return (c.x >= g.min_points ? 1u : 0u) | (c.y >= g.min_points ? 2u : 0u) | (c.z >= g.min_points ? 4u : 0u) | (c.w >= g.min_points ? 8u : 0u);
    }
    __device__ void emit(int item, unsigned pos) const {
        float s[4];
        cloud_sphere(g, item, s);
        out[pos] = make_float4(s[0], s[1], s[2], s[3]);
    }
};
struct KeepSrc {            // items = candidates; d [n] their pass-1 distances at the robot's state
    const float* d;
    const float4* cand;
    float margin;
    float4* out;
    __device__ unsigned flags(int base, int n) const {
        unsigned f = 0;
        for (int j = 0; j < CLOUD_ITEMS; ++j)
            if (base + j < n && cloud_keep(d[base + j], margin)) f |= 1u << j;
        return f;
    }
    __device__ void emit(int item, unsigned pos) const { out[pos] = cand[item]; }
};
// ... and those of the tracked call, which also write every kept item's cell index beside its sphere
struct RecSrc {             // items = cells; rec is zero-padded to whole blocks like count, occupancy is its .x
    const uint4* rec;
    CloudGrid g;
    float4* out;
    int* cell;
    __device__ unsigned flags(int base, int) const {
        unsigned f = 0;
        for (int j = 0; j < CLOUD_ITEMS; ++j)
            if (rec[base + j].x >= g.min_points) f |= 1u << j;
        return f;
    }
    __device__ void emit(int item, unsigned pos) const {
        float s[4];
        cloud_sphere(g, item, s);
        out[pos] = make_float4(s[0], s[1], s[2], s[3]);
        cell[pos] = item;
    }
};
struct KeepCellSrc {
    KeepSrc keep;
    const int* candCell;
    int* cell;
    __device__ unsigned flags(int base, int n) const { return keep.flags(base, n); }
    __device__ void emit(int item, unsigned pos) const {
        keep.emit(item, pos);
        cell[pos] = candCell[item];
    }
};

template <class Src>
__global__ __launch_bounds__(CLOUD_NT) void k_compact_sums(Src src, int n, unsigned* __restrict__ sums) {
    __shared__ unsigned wsum[CLOUD_NT / 64];
    const int base = (blockIdx.x * CLOUD_NT + threadIdx.x) * CLOUD_ITEMS;
    unsigned total;
    (void)block_exclusive_scan((unsigned)__popc(src.flags(base, n)), wsum, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums [nb] -> their exclusive prefixes in place, sums[nb] = the total
__global__ __launch_bounds__(CLOUD_NT) void k_compact_scan(unsigned* __restrict__ sums, int nb) {
    __shared__ unsigned wsum[CLOUD_NT / 64];
    const int per = (nb + CLOUD_NT - 1) / CLOUD_NT;
    const int lo = min((int)threadIdx.x * per, nb), hi = min(lo + per, nb);
    unsigned s = 0;
    for (int i = lo; i < hi; ++i) s += sums[i];
    unsigned total;
    unsigned run = block_exclusive_scan(s, wsum, &total);
    for (int i = lo; i < hi; ++i) {
        const unsigned v = sums[i];
        sums[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) sums[nb] = total;
}

// every kept item to out[offset of its block + its rank in the block]: the output is in item order whatever the schedule; positions
// from cap on are not written (the host has the total and refuses the call)
template <class Src>
__global__ __launch_bounds__(CLOUD_NT) void k_compact_emit(Src src, int n, const unsigned* __restrict__ sums, unsigned cap) {
    __shared__ unsigned wsum[CLOUD_NT / 64];
    const int base = (blockIdx.x * CLOUD_NT + threadIdx.x) * CLOUD_ITEMS;
    const unsigned f = src.flags(base, n);
    unsigned total;
    unsigned pos = block_exclusive_scan((unsigned)__popc(f), wsum, &total) + sums[blockIdx.x];
    for (int j = 0; j < CLOUD_ITEMS; ++j)
        if (f >> j & 1u) {
            if (pos < cap) src.emit(base + j, pos);
            ++pos;
        }
}

__device__ inline unsigned wave_min(unsigned v) {
    for (int d = 32; d > 0; d >>= 1) v = min(v, (unsigned)__shfl_xor(v, d, 64));
    return v;
}
template <class T>
__device__ inline T wave_sum(T v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ---- the counting pass over depth images (depth_def.h) -----------------------------------------------------------------------------
// ONE launch for all cameras: the table goes by value in the kernel arguments, blockIdx.y is the camera (so every index into the table
// is uniform over the workgroup) and blockIdx.x strides over that camera's items.  An ITEM is a run of DEPTH_RUN consecutive visited
// pixels of one visited row: with step 1 a lane's loads are 8 bytes of a U16 row (two dwords where the run's address is a multiple of
// 4, else four shorts: a base aligned to the element size only, an odd pitch) or 16 bytes of an F32 row.  The loop bound is the same
// for all lanes of a workgroup, so every wave reaches the cross-lane steps below whole.
constexpr int DEPTH_RUN = 4;
constexpr int DEPTH_ROUNDS = 8;       // wave rounds before the lanes that are left issue their own atomics
constexpr unsigned DEPTH_MAX_BLOCKS = 2048;

struct DepthCamDev {
    DepthCam c;
    const void* image;     // device memory, element (0, 0)
    int runs;              // items per visited row: ceil(nu / DEPTH_RUN)
    long long items;       // runs * nv
};
struct DepthTable {
    DepthCamDev cam[OMDS_DEPTH_MAX_CAMERAS];
};

// the cells of item `item` of camera d: cell[t] (-1: no point) and, when REC, k[t][3] of cloud_cell_sub
template <bool REC>
__device__ inline void depth_item_cells(const DepthCamDev& d, const CloudGrid& g, long long item, int* cell, unsigned (*k)[3]) {
    const DepthCam& c = d.c;
    const int iv = (int)(item / d.runs), j0 = (int)(item % d.runs) * DEPTH_RUN;
    const int v = iv * c.step;
    const long long first = (long long)v * c.pitch + (long long)j0 * c.step;
    const bool whole = c.step == 1 && j0 + DEPTH_RUN <= c.nu;
    float z[DEPTH_RUN];
    bool have[DEPTH_RUN];
    if (c.format == OMDS_DEPTH_U16) {
        const uint16_t* p = static_cast<const uint16_t*>(d.image) + first;
        unsigned raw[DEPTH_RUN] = {0u, 0u, 0u, 0u};
        if (whole && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
            const unsigned* q = reinterpret_cast<const unsigned*>(p);
            const unsigned w0 = q[0], w1 = q[1];
            raw[0] = w0 & 0xffffu; raw[1] = w0 >> 16; raw[2] = w1 & 0xffffu; raw[3] = w1 >> 16;
        } else {
            for (int t = 0; t < DEPTH_RUN; ++t)
                if (j0 + t < c.nu) raw[t] = p[(long long)t * c.step];
        }
        for (int t = 0; t < DEPTH_RUN; ++t) {
            z[t] = 0.f;
            have[t] = depth_z_u16(c, raw[t], &z[t]);   // a column past the row holds raw 0: no return
        }
    } else {
        const float* p = static_cast<const float*>(d.image) + first;
        if (whole && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            const float4 w = *reinterpret_cast<const float4*>(p);
            z[0] = w.x; z[1] = w.y; z[2] = w.z; z[3] = w.w;
            for (int t = 0; t < DEPTH_RUN; ++t) have[t] = true;
        } else {
            for (int t = 0; t < DEPTH_RUN; ++t) {
                have[t] = j0 + t < c.nu;
                z[t] = have[t] ? p[(long long)t * c.step] : 0.f;
            }
        }
    }
    for (int t = 0; t < DEPTH_RUN; ++t) {
        cell[t] = -1;
        if (!have[t] || !depth_gate(c, z[t])) continue;
        float w[3];
        depth_point(c, (j0 + t) * c.step, v, z[t], w);
        if (REC) cell[t] = cloud_cell_sub(g, w[0], w[1], w[2], k[t]);
        else cell[t] = cloud_cell(g, w[0], w[1], w[2]);
    }
}

// what one lane adds to a cell: the count alone, or the record (n, s_x, s_y, s_z) packed in 16-bit fields.  A wave's sum of one cell
// is at most 64 lanes x DEPTH_RUN pixels = 256 points and 255 x 256 = 65 280 per offset sum: no field carries into the next
template <bool REC> struct DepthAcc;
template <> struct DepthAcc<false> {
    typedef unsigned T;
    __device__ static T one(const unsigned*) { return 1u; }
    __device__ static void add(void* buf, int cell, T v) { atomicAdd(static_cast<unsigned*>(buf) + cell, v); }
};
template <> struct DepthAcc<true> {
    typedef unsigned long long T;
    __device__ static T one(const unsigned* k) {
        return 1ull | (unsigned long long)k[0] << 16 | (unsigned long long)k[1] << 32 | (unsigned long long)k[2] << 48;
    }
    __device__ static void add(void* buf, int cell, T v) {
        unsigned* r = reinterpret_cast<unsigned*>(static_cast<uint4*>(buf) + cell);
        atomicAdd(r, (unsigned)(v & 0xffffu));
        atomicAdd(r + 1, (unsigned)(v >> 16 & 0xffffu));
        atomicAdd(r + 2, (unsigned)(v >> 32 & 0xffffu));
        atomicAdd(r + 3, (unsigned)(v >> 48));
    }
};

// The lane first merges equal cells of its run in registers; then the wave merges across lanes -- the first lane that still holds a
// cell names it, the lanes that hold the same cell hand their sums to a wave reduction (zeros from the others) and drop it, the naming
// lane issues the one atomic (four when REC) -- for at most DEPTH_ROUNDS rounds; what is left after that goes out lane by lane, so an
// image in which every lane holds other cells does not serialise 64 rounds.  Integer sums: no order can change a bit.  No atomic
// returns a value and nothing waits for one.  (The plain form, one atomic per kept pixel, was 0.02-0.06 ms slower per tracked call
// at 640 x 480: EXPERIMENTS R20.)
template <bool REC>
__device__ inline void depth_count(const DepthTable& tab, const CloudGrid& g, void* buf) {
    typedef DepthAcc<REC> Acc;
    typedef typename Acc::T T;
    const DepthCamDev& d = tab.cam[blockIdx.y];
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * CLOUD_NT; base < d.items; base += (long long)gridDim.x * CLOUD_NT) {
        const long long item = base + threadIdx.x;
        int cell[DEPTH_RUN] = {-1, -1, -1, -1};
        unsigned k[DEPTH_RUN][3] = {};
        if (item < d.items) depth_item_cells<REC>(d, g, item, cell, k);
        T acc[DEPTH_RUN];
        for (int t = 0; t < DEPTH_RUN; ++t) acc[t] = Acc::one(k[t]);
        for (int t = 1; t < DEPTH_RUN; ++t)
            for (int s = 0; s < t; ++s)
                if (cell[t] >= 0 && cell[t] == cell[s]) {
                    acc[s] += acc[t];
                    cell[t] = -1;
                }
        for (int round = 0; round < DEPTH_ROUNDS; ++round) {
            const int mine = cell[0] >= 0 ? cell[0] : cell[1] >= 0 ? cell[1] : cell[2] >= 0 ? cell[2] : cell[3];
            const unsigned long long pending = __ballot(mine >= 0);
            if (!pending) break;   // the same for every lane of the wave
            const int namer = __ffsll((long long)pending) - 1;
            const int named = __shfl(mine, namer, 64);
            T part = 0;
            for (int t = 0; t < DEPTH_RUN; ++t)
                if (cell[t] == named) {
                    part = acc[t];
                    cell[t] = -1;
                }
            const T sum = wave_sum(part);
            if (lane == namer) Acc::add(buf, named, sum);
        }
        for (int t = 0; t < DEPTH_RUN; ++t)
            if (cell[t] >= 0) Acc::add(buf, cell[t], acc[t]);
    }
}

__global__ __launch_bounds__(CLOUD_NT) void k_depth_count(DepthTable tab, CloudGrid g, unsigned* __restrict__ count) {
    depth_count<false>(tab, g, count);
}
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_rec(DepthTable tab, CloudGrid g, uint4* __restrict__ rec) {
    depth_count<true>(tab, g, rec);
}

// The velocity of every final sphere (point_cloud_flow_def.h): one wave per sphere, four per workgroup, no barrier.  A first probe
// of the sphere's own cell in the previous frame settles the common case (d2 = 0 is the unique minimum).  Otherwise the lanes stride
// over the window clipped to the grid, x innermost; each keeps the sums of its own cells at its own smallest d2, the wave takes the
// minimum, lanes above it drop their sums, and the rest is added up by shuffles -- integers throughout, so the schedule cannot change
// a bit.  Lane 0 then evaluates the fp32 lines of the definition; vel[sphere].w = 1 where the window was not empty (the host counts
// them: one counter for all spheres would serialise 30 000 atomics on one address, 0.34 ms at the scene of EXPERIMENTS R18).
constexpr int FLOW_WAVES = CLOUD_NT / 64;
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
constexpr int OBJ_ACC = 5;
constexpr int SUMS_NT = 1024, SUMS_WAVES = SUMS_NT / 64;
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

// the roots as a third item space of the ordered compaction: the component table in ascending label order
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

inline int compaction_blocks(int n) { return (n + CLOUD_BLOCK - 1) / CLOUD_BLOCK; }

// the ordered compaction of n items of src into src.out (at most cap spheres written); *total_out = kept items.  Synchronises.
template <class Src>
int compact(omds_ctx* ctx, const Src& src, int n, int cap, int* total_out) {
    *total_out = 0;
    if (n <= 0) return OMDS_OK;
    const int nb = compaction_blocks(n);
    unsigned* sums = ctx->d_cloudSums;
    hipLaunchKernelGGL((k_compact_sums<Src>), dim3(nb), dim3(CLOUD_NT), 0, ctx->stream, src, n, sums);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(CLOUD_NT), 0, ctx->stream, sums, nb);
    hipLaunchKernelGGL((k_compact_emit<Src>), dim3(nb), dim3(CLOUD_NT), 0, ctx->stream, src, n, sums, (unsigned)cap);
    CK(hipGetLastError());
    unsigned total = 0;
    CK(hipMemcpyAsync(&total, sums + nb, 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    *total_out = (int)total;
    return OMDS_OK;
}

// What the objects call adds to the tracked one: its spec, and where its two counts go
struct ObjectsCall {
    CloudObjects ob;
    int32_t* n_objects_out;
    int32_t* n_objects_matched_out;
};

// Where the points of a call come from: an array xyz [n_points][3] (host or device), or the depth images of up to eight cameras
struct DepthSource {
    DepthCam cam[OMDS_DEPTH_MAX_CAMERAS];   // behind their checks
    const void* const* images;
    int n_cams;
    int on_device;
};
struct PointSource {
    const float* xyz;
    int64_t n_points;
    int xyz_on_device;
    const DepthSource* depth;   // != nullptr: the images, and the three fields above are unused
};

// the kernel's camera table and its grid; host images go to the context's staging buffer, one asynchronous copy each
int stage_depth(omds_ctx* ctx, const DepthSource& src, DepthTable* tab, dim3* grid) {
    size_t offset[OMDS_DEPTH_MAX_CAMERAS], total = 0;
    long long most = 1;
    for (int i = 0; i < src.n_cams; ++i) {
        const size_t bytes = (size_t)depth_extent(src.cam[i]) * (src.cam[i].format == OMDS_DEPTH_U16 ? 2 : 4);
        offset[i] = total;
        total += (bytes + 15) & ~(size_t)15;
    }
    if (!src.on_device && ctx->d_depthImg.count() < total) {
        CK(hipStreamSynchronize(ctx->stream));
        CK(ctx->d_depthImg.alloc(total));
    }
    std::memset(static_cast<void*>(tab), 0, sizeof(*tab));
    for (int i = 0; i < src.n_cams; ++i) {
        DepthCamDev& d = tab->cam[i];
        d.c = src.cam[i];
        d.image = src.images[i];
        if (!src.on_device) {
            const size_t bytes = (size_t)depth_extent(d.c) * (d.c.format == OMDS_DEPTH_U16 ? 2 : 4);
            CK(hipMemcpyAsync(ctx->d_depthImg.get() + offset[i], src.images[i], bytes, hipMemcpyHostToDevice, ctx->stream));
            d.image = ctx->d_depthImg.get() + offset[i];
        }
        d.runs = (d.c.nu + DEPTH_RUN - 1) / DEPTH_RUN;
        d.items = (long long)d.runs * d.c.nv;
        most = std::max(most, d.items);
    }
    const unsigned per_camera = std::max(DEPTH_MAX_BLOCKS / (unsigned)src.n_cams, 1u);
    *grid = dim3((unsigned)std::min<long long>((most + CLOUD_NT - 1) / CLOUD_NT, per_camera), (unsigned)src.n_cams);
    return OMDS_OK;
}

// The cloud entry points.  tr == nullptr is omds_set_obstacles_from_cloud: the count buffer, no cell indices, no velocities.  With tr
// the same steps in the same order on the record buffer that is NOT the stored frame, then k_cloud_flow over the final list; with oc
// (which needs tr) the components of the final list, into the table that is NOT the stored one, and the object velocities
int scene_from_cloud(omds_ctx* ctx, const char* who, const omds_cloud_spec* spec, const CloudGrid& g, const CloudTrack* tr, const PointSource& src,
                     const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out, int32_t* n_matched_out,
                     const ObjectsCall* oc = nullptr) {
    const std::string me(who);
    int rc;
    const float* xyz = src.xyz;
    const int64_t n_points = src.n_points;
    REQUIRE(src.depth || (n_points >= 0 && n_points <= OMDS_CLOUD_MAX_POINTS && (n_points == 0 || xyz)), OMDS_ERR_INVALID_ARG,
            me + ": need 0 <= n_points <= 16 777 216 and a non-null xyz [P,3]");
    if (q_now) {
        REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, me + ": the self-filter needs the distance network (omds_set_mlp)");
        REQUIRE(!ctx->wide.on, OMDS_ERR_UNSUPPORTED, me + ": no self-filter on networks wider than 256 (no obstacle tables)");
    }
    CK(hipSetDevice(ctx->dev));
    const int nb = compaction_blocks(g.n_cells), k = ctx->cfg.n_closest;
    static_assert(CLOUD_MAX_BLOCKS * CLOUD_BLOCK == OMDS_CLOUD_MAX_CELLS, "k_compact_scan takes every grid the spec allows");
    const size_t n_padded = (size_t)nb * CLOUD_BLOCK;
    DevBuf<uint4>* rec = tr ? &ctx->d_cloudRec[1 - ctx->cloud_stored] : nullptr;   // counted into; the stored frame is the other one
    if ((tr ? rec->count() < n_padded || ctx->d_cloudVel.count() < (size_t)g.max_spheres : ctx->d_cloudCount.count() < n_padded) ||
        ctx->d_cloudCand.count() < (size_t)g.max_spheres) {
        CK(hipStreamSynchronize(ctx->stream));
        if (tr) {
            CK(rec->reserve(n_padded));
            CK(ctx->d_cloudCandCell.reserve((size_t)g.max_spheres));
            CK(ctx->d_cloudKeptCell.reserve((size_t)g.max_spheres));
            CK(ctx->d_cloudVel.reserve((size_t)g.max_spheres));
        } else {
            CK(ctx->d_cloudCount.reserve(n_padded));
        }
        CK(ctx->d_cloudSums.reserve((size_t)CLOUD_MAX_BLOCKS + 1));
        CK(ctx->d_cloudCand.reserve((size_t)g.max_spheres));
        CK(ctx->d_cloudKept.reserve((size_t)g.max_spheres));
    }
    DevBuf<unsigned char>* table = oc ? &ctx->d_cloudTable[1 - ctx->cloud_table_stored] : nullptr;   // written; the stored table is the other one
    if (oc && (ctx->d_cloudSlot.count() < n_padded || ctx->d_cloudParent.count() < (size_t)g.max_spheres ||
               table->count() < (size_t)g.max_spheres * sizeof(CloudComp))) {
        CK(hipStreamSynchronize(ctx->stream));
        CK(ctx->d_cloudSlot.reserve(n_padded));
        CK(ctx->d_cloudParent.reserve((size_t)g.max_spheres));
        CK(ctx->d_cloudLabel.reserve((size_t)g.max_spheres));
        CK(ctx->d_cloudObject.reserve((size_t)g.max_spheres));
        CK(ctx->d_cloudCompOf.reserve((size_t)g.max_spheres));
        CK(ctx->d_cloudAcc.reserve((size_t)g.max_spheres * OBJ_ACC));
        CK(ctx->d_cloudObjVel.reserve((size_t)g.max_spheres));
        CK(table->reserve((size_t)g.max_spheres * sizeof(CloudComp)));
    }
    // the points: the caller's device array as it is, a host array through a staging buffer of the context
    const float* d_xyz = xyz;
    DepthTable depth_table;
    dim3 depth_grid;
    if (src.depth) {
        if ((rc = stage_depth(ctx, *src.depth, &depth_table, &depth_grid))) return rc;
    } else if (!src.xyz_on_device && n_points > 0) {
        if (ctx->d_cloudXyz.count() < (size_t)n_points * 3) {
            CK(hipStreamSynchronize(ctx->stream));
            CK(ctx->d_cloudXyz.alloc((size_t)n_points * 3));
        }
        CK(hipMemcpyAsync(ctx->d_cloudXyz, xyz, (size_t)n_points * 12, hipMemcpyHostToDevice, ctx->stream));
        d_xyz = ctx->d_cloudXyz;
    }
    const unsigned grid = (unsigned)std::min<long long>((n_points + CLOUD_NT - 1) / CLOUD_NT, 2048);
    int occupied = 0;
    if (tr) {
        CK(hipMemsetAsync(rec->get(), 0, n_padded * 16, ctx->stream));
        if (src.depth)
            hipLaunchKernelGGL(k_depth_count_rec, depth_grid, dim3(CLOUD_NT), 0, ctx->stream, depth_table, g, rec->get());
        else if (n_points > 0)
            hipLaunchKernelGGL(k_cloud_count_rec, dim3(grid), dim3(CLOUD_NT), 0, ctx->stream, d_xyz, (long long)n_points, g, rec->get());
        const RecSrc cells{rec->get(), g, ctx->d_cloudCand, ctx->d_cloudCandCell};
        if ((rc = compact(ctx, cells, g.n_cells, g.max_spheres, &occupied))) return rc;
    } else {
        CK(hipMemsetAsync(ctx->d_cloudCount, 0, n_padded * 4, ctx->stream));
        if (src.depth)
            hipLaunchKernelGGL(k_depth_count, depth_grid, dim3(CLOUD_NT), 0, ctx->stream, depth_table, g, ctx->d_cloudCount.get());
        else if (n_points > 0)
            hipLaunchKernelGGL(k_cloud_count, dim3(grid), dim3(CLOUD_NT), 0, ctx->stream, d_xyz, (long long)n_points, g, ctx->d_cloudCount.get());
        const CellSrc cells{ctx->d_cloudCount, g, ctx->d_cloudCand};
        if ((rc = compact(ctx, cells, g.n_cells, g.max_spheres, &occupied))) return rc;
    }
    if (n_occupied_out) *n_occupied_out = occupied;
    REQUIRE(occupied <= g.max_spheres, OMDS_ERR_INVALID_ARG,
            me + ": more occupied cells than max_spheres (n_occupied_out holds their number); the scene is unchanged");
    const float4* d_list = ctx->d_cloudCand;
    const int* d_cell = ctx->d_cloudCandCell;
    int n_list = occupied;
    if (q_now && occupied > 0) {
        // The candidates become the obstacle rows of one state.  From here on the tables of the old scene are overwritten: the context
        // holds no scene, and no horizon of one, until install_obstacles below has put the new one in
        const int n = ctx->cfg.n_dof;
        if ((rc = reserve_obstacle_capacity(ctx, occupied))) return rc;
        ctx->n_obs = 0;
        clear_obstacle_horizon(ctx);
        CK(hipMemcpyAsync(ctx->d_qcur, q_now, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        omds_launch_rollout_features(ctx->stream, ctx->mlp, ctx->d_qcur, 1, 1, ctx->d_Fq);
        omds_launch_obstacle_features(ctx->stream, ctx->mlp, reinterpret_cast<const float*>(d_list), occupied, ctx->d_Fp, ctx->d_radius);
        omds_launch_pass1(ctx->stream, ctx->mlp, ctx->d_Fq, ctx->d_Fp, ctx->d_radius, occupied, 1, ctx->prm.ignored_links, ctx->d_Dmin);
        CK(hipGetLastError());
        const KeepSrc keep{ctx->d_Dmin, d_list, spec->self_margin, ctx->d_cloudKept};
        if (tr) {
            const KeepCellSrc keep_cell{keep, d_cell, ctx->d_cloudKeptCell};
            if ((rc = compact(ctx, keep_cell, occupied, g.max_spheres, &n_list))) return rc;
            d_cell = ctx->d_cloudKeptCell;
        } else {
            if ((rc = compact(ctx, keep, occupied, g.max_spheres, &n_list))) return rc;
        }
        d_list = ctx->d_cloudKept;
    }
    // the velocities of the final list against the stored frame, if there is one on this grid
    const int n_final = std::max(n_list, k);
    const bool have_prev = tr && ctx->cloud_have_frame && std::memcmp(ctx->cloud_frame_origin, &g.ox, 12) == 0 &&
                           std::memcmp(&ctx->cloud_frame_voxel, &g.voxel, 4) == 0 && ctx->cloud_frame_dims[0] == g.dx &&
                           ctx->cloud_frame_dims[1] == g.dy && ctx->cloud_frame_dims[2] == g.dz && ctx->cloud_frame_min_points == g.min_points;
    std::vector<float> vel4;
    if (have_prev && n_list > 0) {
        vel4.resize((size_t)n_list * 4);
        hipLaunchKernelGGL(k_cloud_flow, dim3((n_list + FLOW_WAVES - 1) / FLOW_WAVES), dim3(CLOUD_NT), 0, ctx->stream, g, *tr,
                           (const uint4*)rec->get(), (const uint4*)ctx->d_cloudRec[ctx->cloud_stored].get(), d_cell, n_list,
                           ctx->d_cloudVel.get());
        CK(hipGetLastError());
    }
    // the components of the final list, their match against the stored table and the velocities of the accepted objects
    const bool have_table = oc && have_prev && ctx->cloud_have_table && ctx->cloud_table_link == oc->ob.link &&
                            ctx->cloud_table_min_cells == oc->ob.min_cells;
    int n_comp = 0;
    std::vector<int32_t> label((size_t)n_final, -1), object((size_t)n_final, 0);   // padding spheres: label -1, no object
    std::vector<float> obj_vel;
    if (oc && n_list > 0) {
        const int blocks = (n_list + CLOUD_NT - 1) / CLOUD_NT;
        CloudComp* d_table = reinterpret_cast<CloudComp*>(table->get());
        CK(hipMemsetAsync(ctx->d_cloudSlot, 0xff, n_padded * 4, ctx->stream));   // -1
        CK(hipMemsetAsync(ctx->d_cloudAcc, 0, (size_t)n_list * OBJ_ACC * 8, ctx->stream));
        hipLaunchKernelGGL(k_obj_slot, dim3(blocks), dim3(CLOUD_NT), 0, ctx->stream, d_cell, n_list, ctx->d_cloudSlot.get(), ctx->d_cloudParent.get());
        hipLaunchKernelGGL(k_obj_union, dim3(blocks), dim3(CLOUD_NT), 0, ctx->stream, g, oc->ob.link, d_cell, n_list,
                           (const int*)ctx->d_cloudSlot.get(), ctx->d_cloudParent.get());
        hipLaunchKernelGGL(k_obj_flatten, dim3(blocks), dim3(CLOUD_NT), 0, ctx->stream, d_cell, n_list, ctx->d_cloudParent.get(), ctx->d_cloudLabel.get());
        hipLaunchKernelGGL(k_obj_sums, dim3((n_list + SUMS_NT - 1) / SUMS_NT), dim3(SUMS_NT), 0, ctx->stream, g, (const uint4*)rec->get(), d_cell,
                           (const int*)ctx->d_cloudParent.get(), n_list, ctx->d_cloudAcc.get());
        CK(hipGetLastError());
        const RootSrc roots{ctx->d_cloudParent, d_cell, ctx->d_cloudAcc, d_table, ctx->d_cloudCompOf};
        if ((rc = compact(ctx, roots, n_list, g.max_spheres, &n_comp))) return rc;
        hipLaunchKernelGGL(k_obj_match, dim3((n_comp + FLOW_WAVES - 1) / FLOW_WAVES), dim3(CLOUD_NT), 0, ctx->stream, g, *tr, oc->ob,
                           (const CloudComp*)d_table, n_comp,
                           (const CloudComp*)reinterpret_cast<const CloudComp*>(ctx->d_cloudTable[ctx->cloud_table_stored].get()),
                           have_table ? ctx->cloud_table_n : 0, ctx->d_cloudObjVel.get());
        if (have_table) {
            hipLaunchKernelGGL(k_obj_apply, dim3(blocks), dim3(CLOUD_NT), 0, ctx->stream, (const int*)ctx->d_cloudParent.get(),
                               (const int*)ctx->d_cloudCompOf.get(), (const float4*)ctx->d_cloudObjVel.get(), n_list, ctx->d_cloudVel.get(),
                               ctx->d_cloudObject.get());
            CK(hipMemcpyAsync(object.data(), ctx->d_cloudObject, (size_t)n_list * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        CK(hipGetLastError());
        obj_vel.resize((size_t)n_comp * 4);
        CK(hipMemcpyAsync(obj_vel.data(), ctx->d_cloudObjVel, (size_t)n_comp * 16, hipMemcpyDeviceToHost, ctx->stream));
        CK(hipMemcpyAsync(label.data(), ctx->d_cloudLabel, (size_t)n_list * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!vel4.empty()) CK(hipMemcpyAsync(vel4.data(), ctx->d_cloudVel, (size_t)n_list * 16, hipMemcpyDeviceToHost, ctx->stream));
    // to the host, filled up to n_closest with the spec's pad sphere, and in as omds_set_obstacles puts a list in
    std::vector<float> list((size_t)n_final * 4);
    if (n_list > 0) CK(hipMemcpyAsync(list.data(), d_list, (size_t)n_list * 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    for (int i = n_list; i < n_final; ++i) std::memcpy(&list[(size_t)i * 4], spec->pad, 16);
    if ((rc = install_obstacles(ctx, list.data(), n_final))) return rc;
    if (n_spheres_out) *n_spheres_out = n_list;
    if (!tr) return OMDS_OK;
    // a scene whose every sphere stands still keeps the cleared horizon: the propagate that follows is the static one
    std::vector<float> vel((size_t)n_final * 3, 0.f);   // padding spheres stand still
    int matched = 0;
    bool moving = false;
    for (size_t i = 0; i * 4 < vel4.size(); ++i) {
        for (int c = 0; c < 3; ++c) {
            vel[i * 3 + c] = vel4[i * 4 + c];
            moving |= vel4[i * 4 + c] != 0.f;
        }
        matched += vel4[i * 4 + 3] != 0.f;
    }
    if (moving && (rc = omds_set_obstacle_motion(ctx, vel.data()))) return rc;
    ctx->cloud_stored = 1 - ctx->cloud_stored;   // what was counted is the stored frame now
    ctx->cloud_have_frame = true;
    std::memcpy(ctx->cloud_frame_origin, &g.ox, 12);
    ctx->cloud_frame_voxel = g.voxel;
    ctx->cloud_frame_dims[0] = g.dx; ctx->cloud_frame_dims[1] = g.dy; ctx->cloud_frame_dims[2] = g.dz;
    ctx->cloud_frame_min_points = g.min_points;
    if (n_matched_out) *n_matched_out = have_prev ? (int32_t)matched : -1;
    ctx->cloud_have_table = false;   // a plain tracked call stores its records and no table: the next objects call has nothing to match
    if (!oc) return OMDS_OK;
    int32_t n_objects = 0, n_accepted = 0;
    for (int c = 0; c < n_comp; ++c) {
        n_objects += obj_vel[(size_t)c * 4 + 3] >= 1.f;
        n_accepted += obj_vel[(size_t)c * 4 + 3] == 2.f;
    }
    ctx->cloud_table_stored = 1 - ctx->cloud_table_stored;   // what was written is the stored table now
    ctx->cloud_have_table = true;
    ctx->cloud_table_n = n_comp;
    ctx->cloud_table_link = oc->ob.link;
    ctx->cloud_table_min_cells = oc->ob.min_cells;
    ctx->cloud_obj_label = std::move(label);
    ctx->cloud_obj_flag = std::move(object);
    ctx->cloud_obj_count = n_objects;
    if (oc->n_objects_out) *oc->n_objects_out = n_objects;
    if (oc->n_objects_matched_out) *oc->n_objects_matched_out = have_table ? n_accepted : -1;
    return OMDS_OK;
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

int omds_set_obstacles_from_cloud(omds_ctx* ctx, const omds_cloud_spec* spec, const float* xyz, int64_t n_points, int xyz_on_device,
                                  const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudGrid g;
    if (int rc = cloud_resolve_spec(spec, &g, &ctx->err)) return rc;
    return scene_from_cloud(ctx, "omds_set_obstacles_from_cloud", spec, g, nullptr, PointSource{xyz, n_points, xyz_on_device, nullptr}, q_now,
                            n_spheres_out, n_occupied_out, nullptr);
}

int omds_set_obstacles_from_cloud_tracked(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const float* xyz,
                                          int64_t n_points, int xyz_on_device, const float* q_now, int32_t* n_spheres_out,
                                          int32_t* n_occupied_out, int32_t* n_matched_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudGrid g;
    CloudTrack tr;
    if (int rc = cloud_resolve_spec(spec, &g, &ctx->err)) return rc;
    if (int rc = cloud_resolve_track(track, &tr, &ctx->err)) return rc;
    return scene_from_cloud(ctx, "omds_set_obstacles_from_cloud_tracked", spec, g, &tr, PointSource{xyz, n_points, xyz_on_device, nullptr}, q_now,
                            n_spheres_out, n_occupied_out, n_matched_out);
}

int omds_point_cloud_object_flow(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const omds_cloud_object_spec* obj,
                                 const float* xyz_prev, int64_t n_prev, const uint8_t* keep_prev, const float* xyz_now, int64_t n_now,
                                 const uint8_t* keep_now, float* xyzr_out, float* vel_out, int32_t* label_out, int32_t* object_out, int32_t cap,
                                 int32_t* count_out, int32_t* matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out) {
    return cloud_objects_host(spec, track, obj, xyz_prev, n_prev, keep_prev, xyz_now, n_now, keep_now, xyzr_out, vel_out, label_out, object_out,
                              cap, count_out, matched_out, n_objects_out, n_objects_matched_out, &g_create_err);
}

int omds_set_obstacles_from_cloud_objects(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track,
                                          const omds_cloud_object_spec* obj, const float* xyz, int64_t n_points, int xyz_on_device,
                                          const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out, int32_t* n_matched_out,
                                          int32_t* n_objects_out, int32_t* n_objects_matched_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudGrid g;
    CloudTrack tr;
    ObjectsCall oc{{0, 0u}, n_objects_out, n_objects_matched_out};
    if (int rc = cloud_resolve_spec(spec, &g, &ctx->err)) return rc;
    if (int rc = cloud_resolve_track(track, &tr, &ctx->err)) return rc;
    if (int rc = cloud_resolve_objects(obj, &oc.ob, &ctx->err)) return rc;
    return scene_from_cloud(ctx, "omds_set_obstacles_from_cloud_objects", spec, g, &tr, PointSource{xyz, n_points, xyz_on_device, nullptr}, q_now,
                            n_spheres_out, n_occupied_out, n_matched_out, &oc);
}

int omds_depth_points(const omds_depth_camera* cam, const void* image, float* xyz_out, int64_t cap_points, int64_t* n_valid_out) {
    return depth_points_host(cam, image, xyz_out, cap_points, n_valid_out, &g_create_err);
}

int omds_set_obstacles_from_depth(omds_ctx* ctx, const omds_cloud_spec* spec, const omds_cloud_track_spec* track,
                                  const omds_cloud_object_spec* obj, const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                  int images_on_device, const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out,
                                  int32_t* n_matched_out, int32_t* n_objects_out, int32_t* n_objects_matched_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    const char* me = "omds_set_obstacles_from_depth";
    CloudGrid g;
    CloudTrack tr;
    ObjectsCall oc{{0, 0u}, n_objects_out, n_objects_matched_out};
    if (int rc = cloud_resolve_spec(spec, &g, &ctx->err)) return rc;
    REQUIRE(!obj || track, OMDS_ERR_INVALID_ARG, std::string(me) + ": an object spec needs a track spec (the objects route is a tracked one)");
    if (track)
        if (int rc = cloud_resolve_track(track, &tr, &ctx->err)) return rc;
    if (obj)
        if (int rc = cloud_resolve_objects(obj, &oc.ob, &ctx->err)) return rc;
    REQUIRE(n_cams >= 1 && n_cams <= OMDS_DEPTH_MAX_CAMERAS && cams && images, OMDS_ERR_INVALID_ARG,
            std::string(me) + ": need 1 <= n_cams <= 8 and non-null cams, images [n_cams]");
    DepthSource depth;
    depth.images = images;
    depth.n_cams = n_cams;
    depth.on_device = images_on_device;
    int64_t visited = 0;
    for (int i = 0; i < n_cams; ++i) {
        if (int rc = depth_resolve_camera(cams + i, &depth.cam[i], &ctx->err)) return rc;
        REQUIRE(images[i], OMDS_ERR_INVALID_ARG, std::string(me) + ": a null image");
        visited += depth_visited(depth.cam[i]);   // each < 2^62 / 8: no overflow
    }
    REQUIRE(visited <= OMDS_CLOUD_MAX_POINTS, OMDS_ERR_INVALID_ARG, std::string(me) + ": more than 16 777 216 visited pixels in all");
    return scene_from_cloud(ctx, me, spec, g, track ? &tr : nullptr, PointSource{nullptr, 0, 0, &depth}, q_now, n_spheres_out, n_occupied_out,
                            n_matched_out, obj ? &oc : nullptr);
}

int omds_get_cloud_objects(omds_ctx* ctx, int32_t* label, int32_t* object, int32_t* n_objects_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    REQUIRE(ctx->n_obs > 0 && ctx->cloud_obj_label.size() == (size_t)ctx->n_obs, OMDS_ERR_NOT_INITIALISED,
            "omds_get_cloud_objects: the scene in force was not installed by omds_set_obstacles_from_cloud_objects");
    if (label) std::memcpy(label, ctx->cloud_obj_label.data(), (size_t)ctx->n_obs * 4);
    if (object) std::memcpy(object, ctx->cloud_obj_flag.data(), (size_t)ctx->n_obs * 4);
    if (n_objects_out) *n_objects_out = ctx->cloud_obj_count;
    return OMDS_OK;
}

int omds_cloud_track_reset(omds_ctx* ctx) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    ctx->cloud_have_frame = false;
    ctx->cloud_have_table = false;
    return OMDS_OK;
}

}  // extern "C"
