// The scene from a depth point cloud (omds.h: omds_point_cloud_spheres, omds_set_obstacles_from_cloud): the workspace crop and the
// voxel down-sample as one counting pass over the points (k_cloud_count, integer atomics) and an ordered compaction of the occupied
// cells (k_compact_sums -> k_compact_scan -> k_compact_emit), the robot self-filter as ONE fp32 pass-1 launch over one state with the
// candidates as its obstacle rows (the launch the shared first step of a propagate uses) and a second compaction of those it keeps.
// The arithmetic of a cell and of its sphere is point_cloud_def.h's, shared with the host definition.  The final list goes to the host
// (a few thousand x 16 bytes) and from there through install_obstacles, the body of omds_set_obstacles (context.hip).
#include "capi_internal.h"
#include "point_cloud_def.h"

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

}  // namespace

extern "C" {

int omds_point_cloud_spheres(const omds_cloud_spec* spec, const float* xyz, int64_t n_points, float* xyzr_out, int32_t cap,
                             int32_t* count_out) {
    return cloud_spheres_host(spec, xyz, n_points, xyzr_out, cap, count_out, &g_create_err);
}

int omds_set_obstacles_from_cloud(omds_ctx* ctx, const omds_cloud_spec* spec, const float* xyz, int64_t n_points, int xyz_on_device,
                                  const float* q_now, int32_t* n_spheres_out, int32_t* n_occupied_out) {
    if (!ctx) return OMDS_ERR_INVALID_ARG;
    CloudGrid g;
    int rc;
    if ((rc = cloud_resolve_spec(spec, &g, &ctx->err))) return rc;
    REQUIRE(n_points >= 0 && n_points <= OMDS_CLOUD_MAX_POINTS && (n_points == 0 || xyz), OMDS_ERR_INVALID_ARG,
            "omds_set_obstacles_from_cloud: need 0 <= n_points <= 16 777 216 and a non-null xyz [P,3]");
    if (q_now) {
        REQUIRE(ctx->have_mlp, OMDS_ERR_NOT_INITIALISED, "omds_set_obstacles_from_cloud: the self-filter needs the distance network (omds_set_mlp)");
        REQUIRE(!ctx->wide.on, OMDS_ERR_UNSUPPORTED, "omds_set_obstacles_from_cloud: no self-filter on networks wider than 256 (no obstacle tables)");
    }
    CK(hipSetDevice(ctx->dev));
    const int nb = compaction_blocks(g.n_cells), k = ctx->cfg.n_closest;
    static_assert(CLOUD_MAX_BLOCKS * CLOUD_BLOCK == OMDS_CLOUD_MAX_CELLS, "k_compact_scan takes every grid the spec allows");
    if (ctx->d_cloudCount.count() < (size_t)nb * CLOUD_BLOCK || ctx->d_cloudCand.count() < (size_t)g.max_spheres) {
        CK(hipStreamSynchronize(ctx->stream));
        CK(ctx->d_cloudCount.reserve((size_t)nb * CLOUD_BLOCK));
        CK(ctx->d_cloudSums.reserve((size_t)CLOUD_MAX_BLOCKS + 1));
        CK(ctx->d_cloudCand.reserve((size_t)g.max_spheres));
        CK(ctx->d_cloudKept.reserve((size_t)g.max_spheres));
    }
    // the points: the caller's device array as it is, a host array through a staging buffer of the context
    const float* d_xyz = xyz;
    if (!xyz_on_device && n_points > 0) {
        if (ctx->d_cloudXyz.count() < (size_t)n_points * 3) {
            CK(hipStreamSynchronize(ctx->stream));
            CK(ctx->d_cloudXyz.alloc((size_t)n_points * 3));
        }
        CK(hipMemcpyAsync(ctx->d_cloudXyz, xyz, (size_t)n_points * 12, hipMemcpyHostToDevice, ctx->stream));
        d_xyz = ctx->d_cloudXyz;
    }
    CK(hipMemsetAsync(ctx->d_cloudCount, 0, (size_t)nb * CLOUD_BLOCK * 4, ctx->stream));
    if (n_points > 0) {
        const unsigned grid = (unsigned)std::min<long long>((n_points + CLOUD_NT - 1) / CLOUD_NT, 2048);
        hipLaunchKernelGGL(k_cloud_count, dim3(grid), dim3(CLOUD_NT), 0, ctx->stream, d_xyz, (long long)n_points, g, ctx->d_cloudCount.get());
    }
    int occupied = 0;
    const CellSrc cells{ctx->d_cloudCount, g, ctx->d_cloudCand};
    if ((rc = compact(ctx, cells, g.n_cells, g.max_spheres, &occupied))) return rc;
    if (n_occupied_out) *n_occupied_out = occupied;
    REQUIRE(occupied <= g.max_spheres, OMDS_ERR_INVALID_ARG,
            "omds_set_obstacles_from_cloud: more occupied cells than max_spheres (n_occupied_out holds their number); the scene is unchanged");
    const float4* d_list = ctx->d_cloudCand;
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
        if ((rc = compact(ctx, keep, occupied, g.max_spheres, &n_list))) return rc;
        d_list = ctx->d_cloudKept;
    }
    // to the host, filled up to n_closest with the spec's pad sphere, and in as omds_set_obstacles puts a list in
    const int n_final = std::max(n_list, k);
    std::vector<float> list((size_t)n_final * 4);
    if (n_list > 0) CK(hipMemcpyAsync(list.data(), d_list, (size_t)n_list * 16, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    for (int i = n_list; i < n_final; ++i) std::memcpy(&list[(size_t)i * 4], spec->pad, 16);
    if ((rc = install_obstacles(ctx, list.data(), n_final))) return rc;
    if (n_spheres_out) *n_spheres_out = n_list;
    return OMDS_OK;
}

}  // extern "C"
