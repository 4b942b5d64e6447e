// The kernels of the scene from a depth point cloud or from depth images (the host stages: scene_cloud.hip).  The workspace crop and
// the voxel down-sample are one counting pass over the points (k_cloud_count, integer atomics) and an ordered compaction of the
// occupied cells (k_compact_sums -> k_compact_scan -> k_compact_emit); the same compaction keeps the candidates the self-filter lets
// through.  The arithmetic of a cell and of its sphere is point_cloud_def.h's, shared with the host definition.
// The tracked form counts into records of 16 bytes per cell (k_cloud_count_rec), carries each candidate's cell index through both
// compactions, and evaluates point_cloud_flow_def.h against the records of the previous tracked frame with one wave per final sphere
// (k_cloud_flow).
// The objects form adds the launches of point_cloud_objects_def.h: slot map, union-find, flatten, component sums, the component table
// by the same ordered compaction, one wave per component for the match against the stored table, and the object velocities over
// k_cloud_flow's.
// The depth form is another POINT SOURCE of the counting pass: it deprojects the pixels of up to eight depth images itself
// (depth_def.h; k_depth_count, k_depth_count_rec) and no point is ever written.
// The scene memory of the depth route (scene_memory_def.h) is one more pass over the cells behind that counting pass (k_scene_memory),
// a fifth item space of the compaction (MemSrc) and two small launches over the candidates (k_scene_memory_forget, k_scene_memory_age).
// Memory and velocities in one call (scene_memory_flow_def.h): the same pass reading the counts out of the records (k_scene_memory<uint4>),
// the seen sublist as a sixth item space (SeenSrc), and one launch that carries its results back to the final list (k_scene_memory_flow).
#include <algorithm>
#include <type_traits>

#include "cloud_kernels.h"

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

// the cell of pixel (u, v) at a depth z behind the range gate (-1: outside the grid) and, when REC, k[3] of cloud_cell_sub: the one
// deprojection of every depth kernel here
template <bool REC>
__device__ inline int depth_pixel_cell(const DepthCam& c, const CloudGrid& g, int u, int v, float z, unsigned* k) {
    float w[3];
    depth_point(c, u, v, z, w);
    if (REC) return cloud_cell_sub(g, w[0], w[1], w[2], k);
    return cloud_cell(g, w[0], w[1], w[2]);
}

// ... and of a pixel with the ray (a, b) of its camera's lens (depth_lens_def.h), which the caller has found valid
template <bool REC>
__device__ inline int depth_ray_cell(const DepthCam& c, const CloudGrid& g, float a, float b, float z, unsigned* k) {
    float w[3];
    depth_point_ray(c, a, b, z, w);
    if (REC) return cloud_cell_sub(g, w[0], w[1], w[2], k);
    return cloud_cell(g, w[0], w[1], w[2]);
}

// the cells of item `item` of camera d: cell[t] (-1: no point) and, when REC, k[t][3] of cloud_cell_sub.  LENS: lc is the camera's
// entry of the lens table; with lc->ab the run's four rays come from it -- entry iv * nu + j0 + t, 8 bytes each: two 16-byte loads
// where a pair starts at an even entry and lies whole inside the row, else 8-byte loads of the entries inside the row (the last run of
// the last row ends the table) -- and a pixel without a ray gives no point
template <bool REC, bool LENS = false>
__device__ inline void depth_item_cells(const DepthCamDev& d, const CloudGrid& g, long long item, int* cell, unsigned (*k)[3],
                                        const DepthLensCam* lc = nullptr) {
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
    if (LENS && lc->ab) {
        const long long e0 = (long long)iv * c.nu + j0;
        const float2* rp = reinterpret_cast<const float2*>(lc->ab) + e0;
        float2 ray[DEPTH_RUN];
        for (int t = 0; t < DEPTH_RUN; t += 2) {
            ray[t] = ray[t + 1] = make_float2(0.f, 0.f);
            if (j0 + t + 1 < c.nu && ((e0 + t) & 1) == 0) {
                const float4 w = *reinterpret_cast<const float4*>(rp + t);
                ray[t] = make_float2(w.x, w.y);
                ray[t + 1] = make_float2(w.z, w.w);
            } else {
                if (j0 + t < c.nu) ray[t] = rp[t];
                if (j0 + t + 1 < c.nu) ray[t + 1] = rp[t + 1];
            }
        }
        for (int t = 0; t < DEPTH_RUN; ++t) {
            cell[t] = -1;
            if (!have[t] || !depth_gate(c, z[t]) || ray[t].x != ray[t].x) continue;
            cell[t] = depth_ray_cell<REC>(c, g, ray[t].x, ray[t].y, z[t], k[t]);
        }
        return;
    }
    for (int t = 0; t < DEPTH_RUN; ++t) {
        cell[t] = -1;
        if (!have[t] || !depth_gate(c, z[t])) continue;
        cell[t] = depth_pixel_cell<REC>(c, g, (j0 + t) * c.step, v, z[t], k[t]);
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
// THE MERGE STANDS TWICE: here, inside depth_count's loop, and as depth_add_cells below it for the filtered pass (why: there).  A
// change to the rounds, to DepthAcc or to the field bound is a change to both; the contention extremes of tests/test_gpu_depth.py (every
// pixel in one cell, two cells, more cells in a wave than rounds) go through this one there and through the other in
// tests/test_gpu_depth_filter.py.
template <bool REC, bool LENS = false>   // LENS: lt is the lens table of the call, beside tab
__device__ inline void depth_count(const DepthTable& tab, const CloudGrid& g, void* buf, const DepthLensTable* lt = nullptr) {
    typedef DepthAcc<REC> Acc;
    typedef typename Acc::T T;
    const DepthCamDev& d = tab.cam[blockIdx.y];
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * CLOUD_NT; base < d.items; base += (long long)gridDim.x * CLOUD_NT) {
        const long long item = base + threadIdx.x;
        int cell[DEPTH_RUN] = {-1, -1, -1, -1};
        unsigned k[DEPTH_RUN][3] = {};
        if (item < d.items) depth_item_cells<REC, LENS>(d, g, item, cell, k, LENS ? &lt->cam[blockIdx.y] : nullptr);
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

// ... and the merge of depth_count as a function, for the filtered pass below: reached by every lane of a wave (the cross-lane steps
// need it whole), uses cell[] up.  depth_count keeps its own text: calling this from there changes the instructions of k_depth_count
// and k_depth_count_rec (the compiler unrolls the rounds), and those two stay the kernels they were
template <bool REC>
__device__ inline void depth_add_cells(int* cell, const unsigned (*k)[3], void* buf) {
    typedef DepthAcc<REC> Acc;
    typedef typename Acc::T T;
    const int lane = threadIdx.x & 63;
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

// ---- the counting pass behind the depth filter (depth_filter_def.h) ----------------------------------------------------------------
// The same launch shape -- one launch, the table by value, blockIdx.y the camera, a lane a run of DEPTH_RUN visited pixels of a row --
// but a workgroup owns a TILE of FILT_TW x FILT_TH visited pixels: FILT_TW / DEPTH_RUN = 8 runs across, 32 rows down.  It stages the
// tile with a halo of R as z_n into LDS, one float per visited pixel, NaN for "no return" and for "outside the image" alike (which
// makes the support test the definition's one comparison for either format); every raw element is read from global memory once per
// tile.  One barrier per tile: the tiles alternate between two LDS images, and a lane that stages image i has passed the barrier of
// tile i - 1, behind which no lane reads image i - 2 = i any more.  The tile loop's bound is the same for every lane of the workgroup.
//   TILE SHAPE: the halo reads (TW + 2R)(TH + 2R) / (TW TH) of the tile: 32 x 32: 1.13 (R = 1), 1.41 (R = 3); 64 x 16: 1.16, 1.50;
//   128 x 8: 1.27, 1.83.  32 x 32 is the smallest overhead and also the shape whose run reads have no bank conflict:
//   ROW STRIDE: the support test is ds_read_b32 / ds_read2_b32 traffic, banked (address / 4) mod 32 over each 32-lane half of a wave.  A half holds 4
//   rows of 8 runs; at window offset (a, b) its lanes read the dwords row * S + 4 run + const.  4 run covers the banks = 0 (mod 4), so
//   the four rows must differ mod 4: S = 1 (mod 4), the smallest such S >= TW + 2R -- 37, 37, 41 -- puts the 32 lanes on 32 banks.
//   (With 16 runs to a row, a 64-wide tile, lanes run and run + 8 of ONE row are 32 dwords apart: 2-way whatever the stride.)
constexpr int FILT_TW = 32, FILT_TH = 32, FILT_RUNS = FILT_TW / DEPTH_RUN;
static_assert(FILT_RUNS * FILT_TH == CLOUD_NT, "one lane per run of the tile");
constexpr int filt_stride(int R) { return (FILT_TW + 2 * R + 2) / 4 * 4 + 1; }
static_assert(filt_stride(1) == 37 && filt_stride(2) == 37 && filt_stride(3) == 41, "the smallest stride = 1 (mod 4) that holds a staged row");

// one aligned load of a group: 4 bytes = 2 U16 elements, 16 bytes = 4 F32 elements
__device__ inline void filt_load_group(const uint16_t* p, uint16_t* raw) {
    const unsigned w = *reinterpret_cast<const unsigned*>(p);
    raw[0] = (uint16_t)(w & 0xffffu);
    raw[1] = (uint16_t)(w >> 16);
}
__device__ inline void filt_load_group(const float* p, float* raw) {
    const float4 w = *reinterpret_cast<const float4*>(p);
    raw[0] = w.x; raw[1] = w.y; raw[2] = w.z; raw[3] = w.w;
}

// step == 1 (nu = width, nv = height): the rows of the staged region by the aligned loads of depth_item_cells -- a GROUP is G elements
// whose first address is a multiple of G elements (4 bytes of a U16 row, 16 of an F32 row), whatever the base, the pitch and the tile's
// first column; a lane takes one group of one row.  A group that lies whole inside its image row is one load; the groups on the row's
// ends load their inside elements one by one (the next row, or the end of the buffer, lies behind them).  Elements of a group outside
// the region are not stored; region positions outside the image hold NaN
template <int R, class E, int G, class Z>
__device__ inline void filt_stage_rows(const DepthCam& c, const E* image, int x0, int y0, float* tile, const Z& z_of) {
    constexpr int RW = FILT_TW + 2 * R, RH = FILT_TH + 2 * R, S = filt_stride(R), NG = (RW + 2 * G - 2) / G;   // groups that touch a region row
    const float nan = __builtin_nanf("");
    const long long e0 = (long long)(reinterpret_cast<uintptr_t>(image) / sizeof(E));   // the image's address in elements
    for (int i = threadIdx.x; i < NG * RH; i += CLOUD_NT) {
        const int ry = i / NG, gi = i - ry * NG, y = y0 + ry;
        const bool row_in = y >= 0 && y < c.nv;
        const long long row = (long long)y * c.pitch;
        const int lead = (int)((e0 + row + x0) & (long long)(G - 1));   // elements between the group boundary and the region's first column
        const int xg = x0 - lead + gi * G;                              // column of the group's first element
        float z[G];
        for (int e = 0; e < G; ++e) z[e] = nan;
        if (row_in && xg >= 0 && xg + G <= c.width) {
            E raw[G];
            filt_load_group(image + row + xg, raw);
            for (int e = 0; e < G; ++e) z[e] = z_of(raw[e]);
        } else if (row_in) {
            for (int e = 0; e < G; ++e)
                if (xg + e >= 0 && xg + e < c.width) z[e] = z_of(image[row + xg + e]);
        }
        for (int e = 0; e < G; ++e) {
            const int rx = xg + e - x0;
            if (rx >= 0 && rx < RW) tile[ry * S + rx] = z[e];
        }
    }
}

// the region of visited pixels [tu0 - R, tu0 + FILT_TW + R) x [tv0 - R, tv0 + FILT_TH + R) as z_n into tile [FILT_TH + 2R][stride]
template <int R>
__device__ inline void filt_stage(const DepthCam& c, const void* image, int tu0, int tv0, float* tile) {
    constexpr int RW = FILT_TW + 2 * R, RH = FILT_TH + 2 * R, S = filt_stride(R);
    const int x0 = tu0 - R, y0 = tv0 - R;
    if (c.step == 1) {
        if (c.format == OMDS_DEPTH_U16)
            filt_stage_rows<R, uint16_t, 2>(c, static_cast<const uint16_t*>(image), x0, y0, tile, [&](uint16_t d) { return depth_filter_z_u16(c, d); });
        else
            filt_stage_rows<R, float, 4>(c, static_cast<const float*>(image), x0, y0, tile, [](float z) { return z; });
        return;
    }
    for (int i = threadIdx.x; i < RW * RH; i += CLOUD_NT) {
        const int ry = i / RW, rx = i - ry * RW, x = x0 + rx, y = y0 + ry;
        float z = __builtin_nanf("");
        if (x >= 0 && x < c.nu && y >= 0 && y < c.nv) z = depth_filter_z(c, image, (long long)y * c.step * c.pitch + (long long)x * c.step);
        tile[ry * S + rx] = z;
    }
}

// counters[0] += pixels the filter keeps, counters[1] += pixels it rejects: integers, reduced per wave, one atomic each
// LENS: lt is the lens table of the call; a pixel the filter keeps whose camera has a lens takes its ray from the table (entry
// jv * nu + ju: a kept pixel lies inside the image) and, when it has none, gives no point and is counted neither as kept nor as rejected
template <bool REC, int R, bool LENS = false>
__device__ inline void depth_count_filt(const DepthTable& tab, const CloudGrid& g, const DepthFilter& f, void* buf, unsigned* counters,
                                        const DepthLensTable* lt = nullptr) {
    constexpr int S = filt_stride(R), RH = FILT_TH + 2 * R;
    __shared__ float tile[2][RH * S];
    const DepthCamDev& d = tab.cam[blockIdx.y];
    const DepthCam& c = d.c;
    const int ly = threadIdx.x / FILT_RUNS, lx = threadIdx.x % FILT_RUNS * DEPTH_RUN;   // this lane's row and first column in the tile
    unsigned kept = 0, rejected = 0;
    int flip = 0;
    for (long long t = blockIdx.x; t < d.items; t += gridDim.x, flip ^= 1) {   // items: the camera's tiles, runs of them to a tile row
        const int tv0 = (int)(t / d.runs) * FILT_TH, tu0 = (int)(t % d.runs) * FILT_TW;
        filt_stage<R>(c, d.image, tu0, tv0, tile[flip]);
        __syncthreads();
        const float* own = tile[flip] + (ly + R) * S + lx + R;
        int cell[DEPTH_RUN] = {-1, -1, -1, -1};
        unsigned k[DEPTH_RUN][3] = {};
        for (int j = 0; j < DEPTH_RUN; ++j) {
            const float z = own[j];                // NaN: no return, or a column / row past the image
            if (!depth_gate(c, z)) continue;
            const float* at = own + j;
            if (!depth_filter_keep(f, R, z, [&](int a, int b) { return at[b * S + a]; })) {
                ++rejected;
                continue;
            }
            if (LENS && lt->cam[blockIdx.y].ab) {
                const float2 ray = reinterpret_cast<const float2*>(lt->cam[blockIdx.y].ab)[(long long)(tv0 + ly) * c.nu + tu0 + lx + j];
                if (ray.x != ray.x) continue;
                ++kept;
                cell[j] = depth_ray_cell<REC>(c, g, ray.x, ray.y, z, k[j]);
                continue;
            }
            ++kept;
            cell[j] = depth_pixel_cell<REC>(c, g, (tu0 + lx + j) * c.step, (tv0 + ly) * c.step, z, k[j]);
        }
        depth_add_cells<REC>(cell, k, buf);
    }
    kept = wave_sum(kept);
    rejected = wave_sum(rejected);
    if ((threadIdx.x & 63) == 0) {
        if (kept) atomicAdd(counters, kept);
        if (rejected) atomicAdd(counters + 1, rejected);
    }
}

template <int R>
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_filt(DepthTable tab, CloudGrid g, DepthFilter f, unsigned* __restrict__ count,
                                                               unsigned* __restrict__ counters) {
    depth_count_filt<false, R>(tab, g, f, count, counters);
}
template <int R>
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_filt_rec(DepthTable tab, CloudGrid g, DepthFilter f, uint4* __restrict__ rec,
                                                                   unsigned* __restrict__ counters) {
    depth_count_filt<true, R>(tab, g, f, rec, counters);
}

__global__ __launch_bounds__(CLOUD_NT) void k_depth_count(DepthTable tab, CloudGrid g, unsigned* __restrict__ count) {
    depth_count<false>(tab, g, count);
}
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_rec(DepthTable tab, CloudGrid g, uint4* __restrict__ rec) {
    depth_count<true>(tab, g, rec);
}

// ---- the lens of a depth camera (depth_lens_def.h) -------------------------------------------------------------------------------------
// The four counting kernels again, with the lens table of the call by value beside the camera table: launched only when some camera of
// the call has a lens, so that the kernels above stay the kernels they are.  A camera without a lens (ab == nullptr; the branch is
// uniform over the workgroup, blockIdx.y being the camera) runs the pinhole arithmetic
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_lens(DepthTable tab, DepthLensTable lt, CloudGrid g, unsigned* __restrict__ count) {
    depth_count<false, true>(tab, g, count, &lt);
}
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_rec_lens(DepthTable tab, DepthLensTable lt, CloudGrid g, uint4* __restrict__ rec) {
    depth_count<true, true>(tab, g, rec, &lt);
}
template <int R>
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_filt_lens(DepthTable tab, DepthLensTable lt, CloudGrid g, DepthFilter f,
                                                                    unsigned* __restrict__ count, unsigned* __restrict__ counters) {
    depth_count_filt<false, R, true>(tab, g, f, count, counters, &lt);
}
template <int R>
__global__ __launch_bounds__(CLOUD_NT) void k_depth_count_filt_rec_lens(DepthTable tab, DepthLensTable lt, CloudGrid g, DepthFilter f,
                                                                        uint4* __restrict__ rec, unsigned* __restrict__ counters) {
    depth_count_filt<true, R, true>(tab, g, f, rec, counters, &lt);
}

// The ray table of one camera: one lane per visited pixel runs the definition and makes one 8-byte store; a pixel without a ray is
// (NaN, NaN).  red[0] takes the largest r2 of a valid ray as an integer maximum on the float's bits (non-negative, so the order of the
// bits is the order of the values), red[1] the pixels without a ray: both reduced per wave, then one integer atomic each.  Every lane
// reaches the cross-lane steps
__device__ inline unsigned wave_max(unsigned v) {
    for (int d = 32; d > 0; d >>= 1) v = max(v, (unsigned)__shfl_xor(v, d, 64));
    return v;
}
__global__ __launch_bounds__(CLOUD_NT) void k_depth_rays(DepthCam c, float fx, float fy, DepthLens l, float2* __restrict__ ab, long long n,
                                                         unsigned* __restrict__ red) {
    const long long i = (long long)blockIdx.x * CLOUD_NT + threadIdx.x;
    unsigned bits = 0u, invalid = 0u;
    if (i < n) {
        const int iv = (int)(i / c.nu), iu = (int)(i % c.nu);
        float a, b;
        if (depth_lens_ray(c, fx, fy, l, iu * c.step, iv * c.step, &a, &b)) bits = __float_as_uint(depth_lens_r2(a, b));
        else invalid = 1u;
        ab[i] = make_float2(a, b);
    }
    bits = wave_max(bits);
    invalid = wave_sum(invalid);
    if ((threadIdx.x & 63) == 0) {
        if (bits) atomicMax(red, bits);
        if (invalid) atomicAdd(red + 1, invalid);
    }
}

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
// second form; the body as a __device__ function called by two kernels did not (the compiler unrolled the camera loop another way)
template <class N>   // unsigned: counts, uint4: records
__global__ __launch_bounds__(CLOUD_NT) void k_scene_memory(DepthTable tab, SceneMemCams ks, int n_cams, CloudGrid g, SceneMem sm,
                                                           const N* __restrict__ count, const unsigned* __restrict__ mem_in,
                                                           unsigned* __restrict__ mem_out, int groups, unsigned* __restrict__ counters) {
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
                out[j] = base + j < g.n_cells ? scene_memory_cell(g, sm, cams, ks, n_cams, base + j, n[j], m[j], &what) : 0u;
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

// ... and its lens form (depth_lens_def.h), launched only when some camera of the call has a lens: the same pass with the lens table by
// value beside the camera table, the verdicts through scene_memory_cell<true>.  A kernel of its own for the reason above
template <class N>
__global__ __launch_bounds__(CLOUD_NT) void k_scene_memory_lens(DepthTable tab, DepthLensTable lt, SceneMemCams ks, int n_cams, CloudGrid g, SceneMem sm,
                                                                const N* __restrict__ count, const unsigned* __restrict__ mem_in,
                                                                unsigned* __restrict__ mem_out, int groups, unsigned* __restrict__ counters) {
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
                out[j] = base + j < g.n_cells ? scene_memory_cell<true>(g, sm, cams, ks, n_cams, base + j, n[j], m[j], &what, &lt) : 0u;
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

// ---- the velocity filter (velocity_filter_def.h) -------------------------------------------------------------------------------------
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

// the spheres of a master scene as a fourth item space (the obstacle focus, obstacle_focus_kernels.hip): kept are the keys below
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

// the ordered compaction of n items of src (at most cap written); the number of kept items is left at sums[blocks of n]
template <class Src>
void compact(hipStream_t s, const Src& src, int n, int cap, unsigned* sums) {
    if (n <= 0) return;
    const int nb = cloud_compaction_blocks(n);
    hipLaunchKernelGGL((k_compact_sums<Src>), dim3(nb), dim3(CLOUD_NT), 0, s, src, n, sums);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(CLOUD_NT), 0, s, sums, nb);
    hipLaunchKernelGGL((k_compact_emit<Src>), dim3(nb), dim3(CLOUD_NT), 0, s, src, n, sums, (unsigned)cap);
}

inline dim3 point_blocks(long long P) { return dim3((unsigned)std::min<long long>((P + CLOUD_NT - 1) / CLOUD_NT, 2048)); }

// the items of every camera into the table; the grid: blockIdx.y the camera, DEPTH_MAX_BLOCKS workgroups over all of them
dim3 depth_blocks(DepthTable& tab, int n_cams) {
    long long most = 1;
    for (int i = 0; i < n_cams; ++i) {
        DepthCamDev& d = tab.cam[i];
        d.runs = (d.c.nu + DEPTH_RUN - 1) / DEPTH_RUN;
        d.items = (long long)d.runs * d.c.nv;
        most = std::max(most, d.items);
    }
    const unsigned per_camera = std::max(DEPTH_MAX_BLOCKS / (unsigned)n_cams, 1u);
    return dim3((unsigned)std::min<long long>((most + CLOUD_NT - 1) / CLOUD_NT, per_camera), (unsigned)n_cams);
}

// ... of the filtered pass: an item is a tile, `runs` of them to a tile row
dim3 depth_filt_blocks(DepthTable& tab, int n_cams) {
    long long most = 1;
    for (int i = 0; i < n_cams; ++i) {
        DepthCamDev& d = tab.cam[i];
        d.runs = (d.c.nu + FILT_TW - 1) / FILT_TW;
        d.items = (long long)d.runs * ((d.c.nv + FILT_TH - 1) / FILT_TH);
        most = std::max(most, d.items);
    }
    const unsigned per_camera = std::max(DEPTH_MAX_BLOCKS / (unsigned)n_cams, 1u);
    return dim3((unsigned)std::min<long long>(most, per_camera), (unsigned)n_cams);
}

// the radius as a constant of the kernel (the window loops unroll): f(std::integral_constant<int, radius>)
template <class F>
void with_radius(int radius, const F& f) {
    if (radius == 1) f(std::integral_constant<int, 1>{});
    else if (radius == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}

}  // namespace

void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, int n_cams, const CloudGrid& g, const DepthFilter& f, unsigned* count,
                                      unsigned* counters) {
    const dim3 grid = depth_filt_blocks(tab, n_cams);
    with_radius(f.radius, [&](auto R) {
        hipLaunchKernelGGL((k_depth_count_filt<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, g, f, count, counters);
    });
}
void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, int n_cams, const CloudGrid& g, const DepthFilter& f, uint4* rec,
                                      unsigned* counters) {
    const dim3 grid = depth_filt_blocks(tab, n_cams);
    with_radius(f.radius, [&](auto R) {
        hipLaunchKernelGGL((k_depth_count_filt_rec<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, g, f, rec, counters);
    });
}

void omds_launch_cloud_count(hipStream_t s, const float* xyz, long long P, const CloudGrid& g, unsigned* count) {
    if (P > 0) hipLaunchKernelGGL(k_cloud_count, point_blocks(P), dim3(CLOUD_NT), 0, s, xyz, P, g, count);
}
void omds_launch_cloud_count(hipStream_t s, const float* xyz, long long P, const CloudGrid& g, uint4* rec) {
    if (P > 0) hipLaunchKernelGGL(k_cloud_count_rec, point_blocks(P), dim3(CLOUD_NT), 0, s, xyz, P, g, rec);
}
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, int n_cams, const CloudGrid& g, unsigned* count) {
    const dim3 grid = depth_blocks(tab, n_cams);
    hipLaunchKernelGGL(k_depth_count, grid, dim3(CLOUD_NT), 0, s, tab, g, count);
}
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, int n_cams, const CloudGrid& g, uint4* rec) {
    const dim3 grid = depth_blocks(tab, n_cams);
    hipLaunchKernelGGL(k_depth_count_rec, grid, dim3(CLOUD_NT), 0, s, tab, g, rec);
}

// the lens forms: the same grids, the lens table beside the camera table
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, const DepthLensTable& lt, int n_cams, const CloudGrid& g, unsigned* count) {
    const dim3 grid = depth_blocks(tab, n_cams);
    hipLaunchKernelGGL(k_depth_count_lens, grid, dim3(CLOUD_NT), 0, s, tab, lt, g, count);
}
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, const DepthLensTable& lt, int n_cams, const CloudGrid& g, uint4* rec) {
    const dim3 grid = depth_blocks(tab, n_cams);
    hipLaunchKernelGGL(k_depth_count_rec_lens, grid, dim3(CLOUD_NT), 0, s, tab, lt, g, rec);
}
void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, const DepthLensTable& lt, int n_cams, const CloudGrid& g, const DepthFilter& f,
                                      unsigned* count, unsigned* counters) {
    const dim3 grid = depth_filt_blocks(tab, n_cams);
    with_radius(f.radius, [&](auto R) {
        hipLaunchKernelGGL((k_depth_count_filt_lens<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, lt, g, f, count, counters);
    });
}
void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, const DepthLensTable& lt, int n_cams, const CloudGrid& g, const DepthFilter& f,
                                      uint4* rec, unsigned* counters) {
    const dim3 grid = depth_filt_blocks(tab, n_cams);
    with_radius(f.radius, [&](auto R) {
        hipLaunchKernelGGL((k_depth_count_filt_rec_lens<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, lt, g, f, rec, counters);
    });
}
void omds_launch_depth_rays(hipStream_t s, const DepthCam& c, float fx, float fy, const DepthLens& l, float* ab, unsigned* red) {
    const long long n = depth_visited(c);
    hipLaunchKernelGGL(k_depth_rays, dim3((unsigned)((n + CLOUD_NT - 1) / CLOUD_NT)), dim3(CLOUD_NT), 0, s, c, fx, fy, l, reinterpret_cast<float2*>(ab), n,
                       red);
}

void omds_launch_cloud_compact_cells(hipStream_t s, const unsigned* count, const CloudGrid& g, float4* out, unsigned* sums) {
    compact(s, CellSrc{count, g, out}, g.n_cells, g.max_spheres, sums);
}
void omds_launch_cloud_compact_cells(hipStream_t s, const uint4* rec, const CloudGrid& g, float4* out, int* cell, unsigned* sums) {
    compact(s, RecSrc{rec, g, out, cell}, g.n_cells, g.max_spheres, sums);
}
void omds_launch_cloud_compact_cells(hipStream_t s, const unsigned* mem, const CloudGrid& g, float4* out, int* cell, unsigned* sums) {
    compact(s, MemSrc{mem, g, out, cell}, g.n_cells, g.max_spheres, sums);
}

void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const SceneMemCams& ks, int n_cams, const CloudGrid& g, const SceneMem& sm,
                              const unsigned* count, const unsigned* mem_in, unsigned* mem_out, unsigned* counters) {
    const int groups = (int)(cloud_padded_cells(g) / CLOUD_ITEMS);   // a multiple of CLOUD_NT
    const unsigned blocks = std::min((unsigned)(groups / CLOUD_NT), MEM_MAX_BLOCKS);
    hipLaunchKernelGGL(k_scene_memory<unsigned>, dim3(blocks), dim3(CLOUD_NT), 0, s, tab, ks, n_cams, g, sm, count, mem_in, mem_out, groups, counters);
}
void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const SceneMemCams& ks, int n_cams, const CloudGrid& g, const SceneMem& sm,
                              const uint4* rec, const unsigned* mem_in, unsigned* mem_out, unsigned* counters) {
    const int groups = (int)(cloud_padded_cells(g) / CLOUD_ITEMS);   // a multiple of CLOUD_NT
    const unsigned blocks = std::min((unsigned)(groups / CLOUD_NT), MEM_MAX_BLOCKS);
    hipLaunchKernelGGL(k_scene_memory<uint4>, dim3(blocks), dim3(CLOUD_NT), 0, s, tab, ks, n_cams, g, sm, rec, mem_in, mem_out, groups, counters);
}
void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const DepthLensTable& lt, const SceneMemCams& ks, int n_cams, const CloudGrid& g,
                              const SceneMem& sm, const unsigned* count, const unsigned* mem_in, unsigned* mem_out, unsigned* counters) {
    const int groups = (int)(cloud_padded_cells(g) / CLOUD_ITEMS);   // a multiple of CLOUD_NT
    const unsigned blocks = std::min((unsigned)(groups / CLOUD_NT), MEM_MAX_BLOCKS);
    hipLaunchKernelGGL(k_scene_memory_lens<unsigned>, dim3(blocks), dim3(CLOUD_NT), 0, s, tab, lt, ks, n_cams, g, sm, count, mem_in, mem_out, groups,
                       counters);
}
void omds_launch_scene_memory(hipStream_t s, DepthTable tab, const DepthLensTable& lt, const SceneMemCams& ks, int n_cams, const CloudGrid& g,
                              const SceneMem& sm, const uint4* rec, const unsigned* mem_in, unsigned* mem_out, unsigned* counters) {
    const int groups = (int)(cloud_padded_cells(g) / CLOUD_ITEMS);   // a multiple of CLOUD_NT
    const unsigned blocks = std::min((unsigned)(groups / CLOUD_NT), MEM_MAX_BLOCKS);
    hipLaunchKernelGGL(k_scene_memory_lens<uint4>, dim3(blocks), dim3(CLOUD_NT), 0, s, tab, lt, ks, n_cams, g, sm, rec, mem_in, mem_out, groups,
                       counters);
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

void omds_launch_cloud_compact_kept(hipStream_t s, const float* d, const float4* cand, const int* candCell, int n, float margin, int cap,
                                    float4* out, int* cell, unsigned* sums) {
    const KeepSrc keep{d, cand, margin, out};
    if (candCell) compact(s, KeepCellSrc{keep, candCell, cell}, n, cap, sums);
    else compact(s, keep, n, cap, sums);
}
void omds_launch_cloud_compact_roots(hipStream_t s, const int* root, const int* cells, const unsigned long long* acc, int n, int cap,
                                     CloudComp* table, int* compOf, unsigned* sums) {
    compact(s, RootSrc{root, cells, acc, table, compOf}, n, cap, sums);
}

void omds_launch_focus_compact(hipStream_t s, const unsigned* keys, const unsigned* res, const float4* master, const float* vel, int n, int cap,
                               float4* out, int* idx, float* velOut, unsigned* sums) {
    compact(s, FocusSrc{keys, res, master, vel, out, idx, velOut}, n, cap, sums);
}

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
