// The device pieces that several of the cloud kernel files need (cloud_kernels.hip, depth_kernels.hip, scene_memory_kernels.hip,
// cloud_track_kernels.hip, velocity_filter_kernels.hip): the wave reductions, the workgroup scan and the ordered compaction over an
// ITEM SPACE -- a struct Src with flags(base, n): bit j set when item base + j is kept, and emit(item, pos): what goes out for it at
// pos.  A source struct lives in the file of the concern that owns it; compact<Src> below is instantiated there.  Everything here is
// in the unnamed namespace of the file that includes it.
#pragma once
#include "cloud_kernels.h"

namespace {

constexpr int FLOW_WAVES = CLOUD_NT / 64;               // one wave per sphere or component: k_cloud_flow, k_obj_match, k_vel_pred
constexpr int SUMS_NT = 1024, SUMS_WAVES = SUMS_NT / 64;   // the workgroup of k_obj_sums and k_vel_group

__device__ inline unsigned wave_min(unsigned v) {
    for (int d = 32; d > 0; d >>= 1) v = min(v, (unsigned)__shfl_xor(v, d, 64));
    return v;
}
template <class T>
__device__ inline T wave_sum(T v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ inline unsigned wave_max(unsigned v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, (unsigned)__shfl_xor(v, d, 64));
    return v;
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

// the ordered compaction of n items of src (at most cap written); the number of kept items is left at sums[blocks of n]
template <class Src>
void compact(hipStream_t s, const Src& src, int n, int cap, unsigned* sums) {
    if (n <= 0) return;
    const int nb = cloud_compaction_blocks(n);
    hipLaunchKernelGGL((k_compact_sums<Src>), dim3(nb), dim3(CLOUD_NT), 0, s, src, n, sums);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(CLOUD_NT), 0, s, sums, nb);
    hipLaunchKernelGGL((k_compact_emit<Src>), dim3(nb), dim3(CLOUD_NT), 0, s, src, n, sums, (unsigned)cap);
}

}  // namespace
