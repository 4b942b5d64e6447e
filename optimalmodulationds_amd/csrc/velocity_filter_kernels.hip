// The velocity filter of a tracked scene call (velocity_filter_def.h; the layout of the cloud kernel files: cloud_kernels.hip; the
// launchers: cloud_kernels.h): the predecessor of every final sphere in the stored state, the group sums of the accepted objects,
// and the blend.
#include "cloud_device.h"

namespace {

// state[cells[i]] = no history for the n cells a state buffer last held: behind it the buffer is all zero again
__global__ __launch_bounds__(CLOUD_NT) void k_vel_clear(const int* __restrict__ cells, int n, int4* __restrict__ state) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x;
    if (i < n) state[cells[i]] = make_int4(0, 0, 0, 0);
}

// The predecessor of every final sphere in the stored state: one wave per sphere, four per workgroup, no barrier, in the shape of
// k_cloud_flow.  The sphere's own cell first (d2 = 0 is the unique minimum); otherwise the lanes stride over the window clipped to
// the grid, each keeps the sums of its own cells at its own smallest d2, the wave takes the minimum, lanes above it drop their sums,
// and the rest is added up by shuffles -- integers throughout.  Lane 0 writes (S, t, h) and empties the sphere's group accumulator
// (group != nullptr), which k_vel_group fills in the next launch.  state == nullptr: an empty history
__global__ __launch_bounds__(CLOUD_NT) void k_vel_pred(CloudGrid g, int reach, const int4* __restrict__ state, const int* __restrict__ cells,
                                                       int n_spheres, VelPred* __restrict__ pred, unsigned long long* __restrict__ group,
                                                       int* __restrict__ groupH) {
    const int lane = threadIdx.x & 63, sphere = blockIdx.x * FLOW_WAVES + (threadIdx.x >> 6);
    if (sphere >= n_spheres) return;   // a whole wave
    VelPredSums a;
    vel_pred_clear(a);
    if (state) {
        const int cell = cells[sphere];
        const int4 own = state[cell];
        if (own.w >= 1) {
            vel_pred_add(a, 0, 0, 0, own.x, own.y, own.z, own.w);
        } else {
            const int ix = cell % g.dx, iy = (cell / g.dx) % g.dy, iz = cell / (g.dx * g.dy);
            const int x0 = max(ix - reach, 0), y0 = max(iy - reach, 0), z0 = max(iz - reach, 0);
            const int wx = min(ix + reach, g.dx - 1) - x0 + 1, wy = min(iy + reach, g.dy - 1) - y0 + 1, wz = min(iz + reach, g.dz - 1) - z0 + 1;
            for (int i = lane; i < wx * wy * wz; i += 64) {
                const int x = x0 + i % wx, y = y0 + (i / wx) % wy, z = z0 + i / (wx * wy);
                const int4 q = state[(z * g.dy + y) * g.dx + x];
                if (q.w >= 1) vel_pred_add(a, x - ix, y - iy, z - iz, q.x, q.y, q.z, q.w);
            }
            const unsigned best = wave_min(a.d2);
            if (a.d2 != best) vel_pred_clear(a);
            a.d2 = best;
            a.t = wave_sum(a.t);
            for (int c = 0; c < 3; ++c) a.S[c] = wave_sum(a.S[c]);
            const unsigned h = wave_min(a.h == 0 ? 0xffffffffu : (unsigned)a.h);   // the lanes without a cell at the minimum stay out
            a.h = h == 0xffffffffu ? 0 : (int)h;
        }
    }
    if (lane != 0) return;
    pred[sphere] = VelPred{{a.S[0], a.S[1], a.S[2]}, (int)a.t, a.h};
    if (!group) return;
    for (int k = 0; k < VEL_GROUP_ACC; ++k) group[(size_t)sphere * VEL_GROUP_ACC + k] = 0ull;
    groupH[sphere] = VEL_NO_HISTORY;
}

// the list index of the sphere in cell `cell`: the list is in ascending cell order.  -1: not in the list
__device__ inline int vel_group_slot(const int* __restrict__ cells, int n, int cell) {
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, c = cells[mid];
        if (c == cell) return mid;
        if (c < cell) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// The group sums G[3], Gt (int64, added as their two's complement) and Gh at the list index of the label's cell: one lane per sphere;
// a sphere adds when it moves with an accepted object, is live and has a predecessor.  A dense scene is one or two huge objects, and
// atomics from different waves on one word serialise (EXPERIMENTS R19), so equal labels are combined before memory is touched, in the
// three steps of k_obj_sums: the list is in cell order, so every run of equal labels inside a wave is added up by a segmented shuffle
// scan; the runs of the wave's DOMINANT label (that of its first adding lane) by a shuffle sum; and the dominant sums of the sixteen
// waves of the workgroup meet in LDS, from where each distinct label goes to memory once, behind one binary search for its
// accumulator.  Integers throughout: no order can change a bit
__global__ __launch_bounds__(SUMS_NT) void k_vel_group(const int* __restrict__ cells, int n, const float4* __restrict__ vel,
                                                       const int* __restrict__ label, const int* __restrict__ object,
                                                       const VelPred* __restrict__ pred, unsigned long long* __restrict__ group,
                                                       int* __restrict__ groupH) {
    __shared__ int key_of[SUMS_WAVES], h_of[SUMS_WAVES];
    __shared__ unsigned long long part[SUMS_WAVES][VEL_GROUP_ACC];
    const int i = blockIdx.x * SUMS_NT + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int key = -1, h = VEL_NO_HISTORY;
    unsigned long long v[VEL_GROUP_ACC] = {0ull, 0ull, 0ull, 0ull};
    if (i < n && object[i] == 1 && vel[i].w != 0.f) {
        const VelPred p = pred[i];
        if (p.h > 0) {
            key = label[i];
            h = p.h;
            for (int c = 0; c < 3; ++c) v[c] = (unsigned long long)p.S[c];
            v[3] = (unsigned long long)p.t;
        }
    }
    const int before = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || before != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int run_end = above ? lane + __ffsll((long long)above) : 64;   // the next head, exclusive end of this lane's run
    for (int d = 1; d < 64; d <<= 1) {
        const int oh = __shfl_down(h, d, 64);
        if (lane + d < run_end) h = min(h, oh);
        for (int k = 0; k < VEL_GROUP_ACC; ++k) {
            const unsigned long long o = __shfl_down(v[k], d, 64);
            if (lane + d < run_end) v[k] += o;
        }
    }
    const unsigned long long adding = __ballot(key >= 0);
    const int dominant = adding ? __shfl(key, __ffsll((long long)adding) - 1, 64) : -1;   // -1: no lane of the wave adds
    const bool first = head && key >= 0, joins = first && key == dominant;
    for (int k = 0; k < VEL_GROUP_ACC; ++k) {
        const unsigned long long d = wave_sum(joins ? v[k] : 0ull);
        if (lane == 0) part[wave][k] = d;
    }
    const unsigned dh = wave_min(joins ? (unsigned)h : (unsigned)VEL_NO_HISTORY);
    if (lane == 0) {
        key_of[wave] = dominant;
        h_of[wave] = (int)dh;
    }
    if (first && !joins) {
        const int at = vel_group_slot(cells, n, key);
        if (at >= 0) {   // a label is the cell of a sphere of the list
            for (int k = 0; k < VEL_GROUP_ACC; ++k) atomicAdd(group + (size_t)at * VEL_GROUP_ACC + k, v[k]);
            atomicMin(groupH + at, h);
        }
    }
    __syncthreads();
    if (threadIdx.x >= SUMS_WAVES || key_of[threadIdx.x] < 0) return;
    const int mine = key_of[threadIdx.x];
    for (int w = 0; w < (int)threadIdx.x; ++w)
        if (key_of[w] == mine) return;   // an earlier wave speaks for this label
    const int at = vel_group_slot(cells, n, mine);
    if (at < 0) return;
    int hm = VEL_NO_HISTORY;
    for (int k = 0; k < VEL_GROUP_ACC; ++k) {
        unsigned long long sum = 0ull;
        for (int w = threadIdx.x; w < SUMS_WAVES; ++w)
            if (key_of[w] == mine) sum += part[w][k];
        atomicAdd(group + (size_t)at * VEL_GROUP_ACC + k, sum);
    }
    for (int w = threadIdx.x; w < SUMS_WAVES; ++w)
        if (key_of[w] == mine) hm = min(hm, h_of[w]);
    atomicMin(groupH + at, hm);
}

// The blend (velocity_filter_def.h): one lane per sphere.  A live sphere takes the fp32 lines of the definition against its own
// predecessor, or its group's (object != nullptr and its flag set), leaves its record by one 16-byte store and its velocity behind the
// still rule; .w stays the matched flag the velocity stages left, so the host still counts.  Every lane lists its cell for the launch
// that empties the buffer again.  counters [3]: live spheres with history, restarts, groups with history -- summed per wave
__global__ __launch_bounds__(CLOUD_NT) void k_vel_blend(VelFilter f, CloudTrack tr, const int* __restrict__ cells, int n,
                                                        const float4* __restrict__ vel, const int* __restrict__ label,
                                                        const int* __restrict__ object, const VelPred* __restrict__ pred,
                                                        const unsigned long long* __restrict__ group, const int* __restrict__ groupH,
                                                        int4* __restrict__ state, int* __restrict__ held, float4* __restrict__ out,
                                                        unsigned* __restrict__ counters) {
    const int i = blockIdx.x * CLOUD_NT + threadIdx.x, lane = threadIdx.x & 63;
    bool with_history = false, restart = false, group_here = false;
    if (i < n) {
        const int cell = cells[i];
        const float4 r = vel[i];
        float v[3] = {0.f, 0.f, 0.f};
        held[i] = cell;
        if (r.w != 0.f) {
            const VelPred own = pred[i];
            long long S[3] = {own.S[0], own.S[1], own.S[2]}, t = own.t;
            int h = own.h;
            const bool grouped = object && object[i] == 1;
            if (grouped) {
                const int at = vel_group_slot(cells, n, label[i]);
                h = 0;
                if (at >= 0 && groupH[at] != VEL_NO_HISTORY) {
                    for (int c = 0; c < 3; ++c) S[c] = (long long)group[(size_t)at * VEL_GROUP_ACC + c];
                    t = (long long)group[(size_t)at * VEL_GROUP_ACC + 3];
                    h = groupH[at];
                }
            }
            const float raw[3] = {r.x, r.y, r.z};
            int hits, rec[4];
            restart = vel_filter_blend(f, grouped, raw, S, t, h, v, &hits);
            with_history = h > 0;
            vel_filter_record(v, hits, rec);
            state[cell] = make_int4(rec[0], rec[1], rec[2], rec[3]);
            cloud_flow_still(tr, v);
        }
        out[i] = make_float4(v[0], v[1], v[2], r.w);
        group_here = object && groupH[i] != VEL_NO_HISTORY;
    }
    const unsigned a = (unsigned)__popcll(__ballot(with_history)), b = (unsigned)__popcll(__ballot(restart)),
                   c = (unsigned)__popcll(__ballot(group_here));
    if (lane != 0) return;
    if (a) atomicAdd(counters, a);
    if (b) atomicAdd(counters + 1, b);
    if (c) atomicAdd(counters + 2, c);
}

}  // namespace

void omds_launch_vel_clear(hipStream_t s, const int* cells, int n, int4* state) {
    if (n > 0) hipLaunchKernelGGL(k_vel_clear, dim3((n + CLOUD_NT - 1) / CLOUD_NT), dim3(CLOUD_NT), 0, s, cells, n, state);
}

void omds_launch_vel_filter(hipStream_t s, const CloudGrid& g, const CloudTrack& tr, const VelFilter& f, const int4* state_in, const int* cells,
                            int n, const float4* vel, const int* label, const int* object, VelPred* pred, unsigned long long* group, int* groupH,
                            int4* state_out, int* held, float4* out, unsigned* counters) {
    const int blocks = (n + CLOUD_NT - 1) / CLOUD_NT;
    if (!object) group = nullptr, groupH = nullptr;
    hipLaunchKernelGGL(k_vel_pred, dim3((n + FLOW_WAVES - 1) / FLOW_WAVES), dim3(CLOUD_NT), 0, s, g, tr.reach, state_in, cells, n, pred, group, groupH);
    if (object && state_in)   // without a history no sphere has a predecessor to add
        hipLaunchKernelGGL(k_vel_group, dim3((n + SUMS_NT - 1) / SUMS_NT), dim3(SUMS_NT), 0, s, cells, n, vel, label, object, (const VelPred*)pred,
                           group, groupH);
    hipLaunchKernelGGL(k_vel_blend, dim3(blocks), dim3(CLOUD_NT), 0, s, f, tr, cells, n, vel, label, object, (const VelPred*)pred,
                       (const unsigned long long*)group, (const int*)groupH, state_out, held, out, counters);
}
