// The kernels of the scene from a depth point cloud (the host stages: scene_cloud.hip; the launchers of all the files below:
// cloud_kernels.h).  The workspace crop and the voxel down-sample are one counting pass over the points (k_cloud_count, integer
// atomics) and an ordered compaction of the occupied cells (cloud_device.h: k_compact_sums -> k_compact_scan -> k_compact_emit); the
// same compaction keeps the candidates the self-filter lets through.  The arithmetic of a cell and of its sphere is
// point_cloud_def.h's, shared with the host definition.  The tracked form counts into records of 16 bytes per cell
// (k_cloud_count_rec) and carries each candidate's cell index through both compactions.
// What else a scene call launches, one concern per file (each says its own): depth_kernels.hip, the depth images as another POINT
// SOURCE of the counting pass; scene_memory_kernels.hip; cloud_track_kernels.hip, the velocities and the objects of the tracked form;
// velocity_filter_kernels.hip.  Here also: FocusSrc, the item space of the obstacle focus (obstacle_focus_kernels.hip).
#include <algorithm>

#include "cloud_device.h"

namespace {

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

// The two item spaces of the cloud call (cloud_device.h: what flags and emit are); emit(item, pos): the item's sphere to out[pos]
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

// the spheres of a master scene as one more item space (the obstacle focus, obstacle_focus_kernels.hip): kept are the keys below
// res[2] and, of the keys equal to it, those at indices up to res[3]; each goes out with its master index and its velocity
struct FocusSrc {
    const unsigned* keys;
    const unsigned* res;
    const float4* master;
    const float* vel;       // [n][3] or nullptr
    float4* out;
    int* idx;
    float* velOut;          // [cap][3], written when vel is given
    __device__ unsigned flags(int base, int n) const {
        const unsigned last = res[2], cut = res[3];
        unsigned f = 0;
        for (int j = 0; j < CLOUD_ITEMS; ++j)
            if (base + j < n) {
                const unsigned key = keys[base + j];
                if (key < last || (key == last && (unsigned)(base + j) <= cut)) f |= 1u << j;
            }
        return f;
    }
    __device__ void emit(int item, unsigned pos) const {
        out[pos] = master[item];
        idx[pos] = item;
        if (vel)
            for (int c = 0; c < 3; ++c) velOut[3 * (size_t)pos + c] = vel[3 * (size_t)item + c];
    }
};

inline dim3 point_blocks(long long P) { return dim3((unsigned)std::min<long long>((P + CLOUD_NT - 1) / CLOUD_NT, 2048)); }

}  // namespace

void omds_launch_cloud_count(hipStream_t s, const float* xyz, long long P, const CloudGrid& g, unsigned* count) {
    if (P > 0) hipLaunchKernelGGL(k_cloud_count, point_blocks(P), dim3(CLOUD_NT), 0, s, xyz, P, g, count);
}
void omds_launch_cloud_count(hipStream_t s, const float* xyz, long long P, const CloudGrid& g, uint4* rec) {
    if (P > 0) hipLaunchKernelGGL(k_cloud_count_rec, point_blocks(P), dim3(CLOUD_NT), 0, s, xyz, P, g, rec);
}

void omds_launch_cloud_compact_cells(hipStream_t s, const unsigned* count, const CloudGrid& g, float4* out, unsigned* sums) {
    compact(s, CellSrc{count, g, out}, g.n_cells, g.max_spheres, sums);
}
void omds_launch_cloud_compact_cells(hipStream_t s, const uint4* rec, const CloudGrid& g, float4* out, int* cell, unsigned* sums) {
    compact(s, RecSrc{rec, g, out, cell}, g.n_cells, g.max_spheres, sums);
}

void omds_launch_cloud_compact_kept(hipStream_t s, const float* d, const float4* cand, const int* candCell, int n, float margin, int cap,
                                    float4* out, int* cell, unsigned* sums) {
    const KeepSrc keep{d, cand, margin, out};
    if (candCell) compact(s, KeepCellSrc{keep, candCell, cell}, n, cap, sums);
    else compact(s, keep, n, cap, sums);
}

void omds_launch_focus_compact(hipStream_t s, const unsigned* keys, const unsigned* res, const float4* master, const float* vel, int n, int cap,
                               float4* out, int* idx, float* velOut, unsigned* sums) {
    compact(s, FocusSrc{keys, res, master, vel, out, idx, velOut}, n, cap, sums);
}
