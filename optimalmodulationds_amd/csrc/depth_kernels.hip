// The depth form of the scene call's counting pass (the layout of the cloud kernel files: cloud_kernels.hip; the launchers:
// cloud_kernels.h): the pixels of up to eight depth images deprojected into the counts or the records of the grid, no point ever
// written (depth_def.h; k_depth_count, k_depth_count_rec); the same pass behind the depth filter, a workgroup to a tile in LDS
// (depth_filter_def.h; k_depth_count_filt, k_depth_count_filt_rec); the lens forms of both and the ray table of a camera's lens
// (depth_lens_def.h; k_depth_rays).
#include <algorithm>
#include <type_traits>

#include "cloud_device.h"

namespace {

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
// pixel in one cell, two cells, more cells in a wave than rounds) go through this one there, under a lens in
// tests/test_gpu_depth_lens.py, and through the other in tests/test_gpu_depth_filter.py.  (One function with the unroll policy of
// the rounds as a template parameter -- depth_add_cells<REC, UNROLL>, rolled in k_depth_count[_lens], unrolled elsewhere -- leaves
// the twelve filtered kernels as they are and the four unfiltered ones within 3 instructions; it was built and not kept, the lens call
// came out 0.0002 ms over its bound: EXPERIMENTS R34.)
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

// lt == nullptr: no camera of the call has a lens, and the pinhole kernel runs; else the lens form, *lt by value beside the table
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, unsigned* count) {
    const dim3 grid = depth_blocks(tab, n_cams);
    if (lt) hipLaunchKernelGGL(k_depth_count_lens, grid, dim3(CLOUD_NT), 0, s, tab, *lt, g, count);
    else hipLaunchKernelGGL(k_depth_count, grid, dim3(CLOUD_NT), 0, s, tab, g, count);
}
void omds_launch_cloud_count(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, uint4* rec) {
    const dim3 grid = depth_blocks(tab, n_cams);
    if (lt) hipLaunchKernelGGL(k_depth_count_rec_lens, grid, dim3(CLOUD_NT), 0, s, tab, *lt, g, rec);
    else hipLaunchKernelGGL(k_depth_count_rec, grid, dim3(CLOUD_NT), 0, s, tab, g, rec);
}
void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, const DepthFilter& f,
                                      unsigned* count, unsigned* counters) {
    const dim3 grid = depth_filt_blocks(tab, n_cams);
    with_radius(f.radius, [&](auto R) {
        if (lt) hipLaunchKernelGGL((k_depth_count_filt_lens<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, *lt, g, f, count, counters);
        else hipLaunchKernelGGL((k_depth_count_filt<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, g, f, count, counters);
    });
}
void omds_launch_cloud_count_filtered(hipStream_t s, DepthTable tab, const DepthLensTable* lt, int n_cams, const CloudGrid& g, const DepthFilter& f,
                                      uint4* rec, unsigned* counters) {
    const dim3 grid = depth_filt_blocks(tab, n_cams);
    with_radius(f.radius, [&](auto R) {
        if (lt) hipLaunchKernelGGL((k_depth_count_filt_rec_lens<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, *lt, g, f, rec, counters);
        else hipLaunchKernelGGL((k_depth_count_filt_rec<decltype(R)::value>), grid, dim3(CLOUD_NT), 0, s, tab, g, f, rec, counters);
    });
}

void omds_launch_depth_rays(hipStream_t s, const DepthCam& c, float fx, float fy, const DepthLens& l, float* ab, unsigned* red) {
    const long long n = depth_visited(c);
    hipLaunchKernelGGL(k_depth_rays, dim3((unsigned)((n + CLOUD_NT - 1) / CLOUD_NT)), dim3(CLOUD_NT), 0, s, c, fx, fy, l, reinterpret_cast<float2*>(ab), n,
                       red);
}
