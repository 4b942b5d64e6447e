// The row order of the block-ordered pass 1 (k_pass1_dyn_blk, mlp_kernels.hip): which rollouts and which obstacles
// share a tile.  The exact zero-skip multiplies the UNION of the hidden units that fire in a tile, so a tile is cheaper the more
// alike its rows are.  A row's layer-1 pre-activation is a rollout share (the weights over the joint features times Fq[t]) plus an
// obstacle share (the weights over the point features times Fp[o]) plus the bias; the sign bits of OMDS_KEY_UNITS of them,
// taken with the other operand at its mean, are a key per rollout and a key per obstacle, and a tile is a block of consecutive
// rollouts x consecutive obstacles of the two key orders.  Nothing here has to be exact: every permutation of the rows computes the
// same bits, the order only decides how many chunks the products run over.
//
// Four small kernels, each written once for a table of rows and used for the rollouts (Fq) and the obstacles (Fp) alike, each spread
// over the device (a row group, a block of rows or a block of entries per workgroup):
//
//   k_share_stats   per unit the sum of the layer-1 shares of OMDS_SHARE_ROWS rows, and the number of them that fire against a
//                   constant: partial sums [groups][256], reduced by their readers in ascending group order (no float atomics)
//   k_tile_pick     the key units (the OMDS_KEY_UNITS units whose firing count over the N rollouts, obstacle share at its mean, is
//                   nearest N / 2; ties by lower unit index), their weights and the constants of both keys (TileKeys)
//   k_order_keys    key[i] = sign bits << 20 | i of the rows of a table
//   k_order_rank    perm[rank of key[i]] = i; the owner of the last rank fills the padding
//
// Once per propagate, in front of its first full launch: stats(Fp of the scene, slab 0 of an obstacle horizon), stats(Fq), pick,
// keys + rank of the obstacles, keys + rank of the rollouts; in front of every later step's pass 1: keys + rank of the rollouts.
// Both orders are the ranks of (key << 20 | index): ties by lower index, the same permutation on every run.
#include "omds_internal.h"

constexpr int OMDS_KEY_ROWS = 64;        // rows (= threads) of a workgroup of k_order_keys
constexpr int OMDS_RANK_LANES = 16;      // lanes that share the scan of one entry's rank
constexpr int OMDS_RANK_ENTRIES = 256 / OMDS_RANK_LANES;   // entries ranked by a workgroup of k_order_rank

// the partial sums of `groups` row groups, in ascending group order: every reader forms the same bits
__device__ __forceinline__ float share_total(const float* __restrict__ part, int groups, int u) {
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += part[(size_t)g * OMDS_WIDTH + u];
    return s;
}

// Thread u = hidden unit u over the rows [blockIdx.x * OMDS_SHARE_ROWS ...) of a table: sum[group][u] = the sum of the unit's shares
// (each table is zero in the other operand's slots: one 32-slot dot product serves both shares).  cnt != nullptr (the rollout
// pass): also the number of rows with share + c[u] > 0, c = b1 + the mean share of the other table, whose partial sums (prev
// [prev_groups][256] over prev_n rows) every workgroup reduces for itself.
// The workgroup's rows reach LDS with one 16-byte load per thread, all in flight at once, and are read from there as broadcasts.
__global__ __launch_bounds__(OMDS_WIDTH) void k_share_stats(const float* __restrict__ W1t, int F, const float* __restrict__ rows, int n,
                                                            const float* __restrict__ b1, const float* __restrict__ prev, int prev_groups,
                                                            int prev_n, float* __restrict__ sum, int* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) float x[OMDS_SHARE_ROWS][OMDS_FROW];
    static_assert(OMDS_SHARE_ROWS * OMDS_FROW == 4 * OMDS_WIDTH, "one float4 per thread stages the row group");
    const int u = threadIdx.x, r0 = blockIdx.x * OMDS_SHARE_ROWS, nr = min(OMDS_SHARE_ROWS, n - r0);
    {
        const int r = u / (OMDS_FROW / 4), q = u % (OMDS_FROW / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nr) v = reinterpret_cast<const float4*>(rows + (size_t)(r0 + r) * OMDS_FROW)[q];
        reinterpret_cast<float4*>(&x[r][0])[q] = v;
    }
    float w[OMDS_FROW];
#pragma unroll
    for (int f = 0; f < OMDS_FROW; ++f) w[f] = f < F ? W1t[(size_t)f * OMDS_WIDTH + u] : 0.f;
    float c = 0.f;
    if (cnt) c = b1[u] + share_total(prev, prev_groups, u) / (float)prev_n;
    __syncthreads();
    float s = 0.f;
    int fire = 0;
    for (int r = 0; r < nr; ++r) {
        float d = 0.f;
#pragma unroll
        for (int q = 0; q < OMDS_FROW / 4; ++q) {
            const float4 v = reinterpret_cast<const float4*>(&x[r][0])[q];
            d = fmaf(w[4 * q], v.x, d); d = fmaf(w[4 * q + 1], v.y, d); d = fmaf(w[4 * q + 2], v.z, d); d = fmaf(w[4 * q + 3], v.w, d);
        }
        s += d;
        fire += (d + c > 0.f) ? 1 : 0;
    }
    sum[(size_t)blockIdx.x * OMDS_WIDTH + u] = s;
    if (cnt) cnt[(size_t)blockIdx.x * OMDS_WIDTH + u] = fire;
}

// One workgroup, thread u = hidden unit u: the firing counts and both mean shares from the partial sums, the key units, TileKeys
__global__ __launch_bounds__(OMDS_WIDTH) void k_tile_pick(const float* __restrict__ W1t, const float* __restrict__ b1, int F,
                                                          const float* __restrict__ sumO, int groupsO, int O,
                                                          const float* __restrict__ sumR, const int* __restrict__ cntR, int groupsR, int N,
                                                          TileKeys* __restrict__ keys) {
    __shared__ float meanO[OMDS_WIDTH], meanR[OMDS_WIDTH];
    __shared__ int away[OMDS_WIDTH];                      // |2 firing rollouts - N| of a unit
    __shared__ int sel[OMDS_KEY_UNITS];
    const int u = threadIdx.x;
    meanO[u] = share_total(sumO, groupsO, u) / (float)O;
    meanR[u] = share_total(sumR, groupsR, u) / (float)N;
    int fire = 0;
    for (int g = 0; g < groupsR; ++g) fire += cntR[(size_t)g * OMDS_WIDTH + u];
    const int n2 = 2 * fire - N;
    away[u] = n2 < 0 ? -n2 : n2;
    __syncthreads();
    int rank = 0;
    for (int v = 0; v < OMDS_WIDTH; ++v) rank += (away[v] < away[u] || (away[v] == away[u] && v < u)) ? 1 : 0;
    if (rank < OMDS_KEY_UNITS) sel[rank] = u;
    __syncthreads();
    for (int e = u; e < OMDS_KEY_UNITS * OMDS_FROW; e += OMDS_WIDTH) {
        const int j = e / OMDS_FROW, f = e % OMDS_FROW;
        keys->W[j][f] = f < F ? W1t[(size_t)f * OMDS_WIDTH + sel[j]] : 0.f;
    }
    if (u < OMDS_KEY_UNITS) {
        const int s = sel[u];
        keys->cR[u] = b1[s] + meanO[s];
        keys->cO[u] = b1[s] + meanR[s];
        keys->unit[u] = s;
    }
}

// Thread = row i of a table: key bit j = the key unit j fires at the row with the other operand's share at its mean (an ascending-f
// fmaf chain from the constant c[j] = TileKeys::cR for the rollouts, ::cO for the obstacles), key[i] = bits << 20 | i
__global__ __launch_bounds__(OMDS_KEY_ROWS) void k_order_keys(const TileKeys* __restrict__ keys, const float* __restrict__ c,
                                                              const float* __restrict__ rows, int n, unsigned* __restrict__ key) {
    __shared__ __attribute__((aligned(16))) float Wk[OMDS_KEY_UNITS][OMDS_FROW];
    __shared__ float ck[OMDS_KEY_UNITS];
    const int tid = threadIdx.x, i = blockIdx.x * OMDS_KEY_ROWS + tid;
    for (int e = tid; e < OMDS_KEY_UNITS * OMDS_FROW; e += OMDS_KEY_ROWS) Wk[e / OMDS_FROW][e % OMDS_FROW] = keys->W[e / OMDS_FROW][e % OMDS_FROW];
    if (tid < OMDS_KEY_UNITS) ck[tid] = c[tid];
    float x[OMDS_FROW];
    if (i < n) {
        const float4* row = reinterpret_cast<const float4*>(rows + (size_t)i * OMDS_FROW);
#pragma unroll
        for (int q = 0; q < OMDS_FROW / 4; ++q) { const float4 v = row[q]; x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w; }
    } else {
#pragma unroll
        for (int f = 0; f < OMDS_FROW; ++f) x[f] = 0.f;
    }
    __syncthreads();
    unsigned bits = 0u;
#pragma unroll 1
    for (int j = 0; j < OMDS_KEY_UNITS; ++j) {
        float s = ck[j];
#pragma unroll
        for (int f = 0; f < OMDS_FROW; ++f) s = fmaf(Wk[j][f], x[f], s);
        bits |= (s > 0.f ? 1u : 0u) << j;
    }
    if (i < n) key[i] = (bits << 20) | (unsigned)i;
}

// Workgroup b ranks the entries [b * OMDS_RANK_ENTRIES ...) of key[0 .. n) (distinct values) against all n keys, held in LDS and
// padded with 0xffffffff to whole scan rounds; OMDS_RANK_LANES lanes share an entry, each counting the smaller keys of every
// OMDS_RANK_LANES-th 16-byte piece, summed over the lanes by shuffles.  perm[rank] = index; the owner of the last rank also fills
// perm[n .. npad) with its index, so that a partial block reads valid rows.
__global__ __launch_bounds__(256) void k_order_rank(const unsigned* __restrict__ key, int n, int* __restrict__ perm, int npad) {
    extern __shared__ __attribute__((aligned(16))) unsigned lkey[];   // [n rounded up to 4 * OMDS_RANK_LANES]
    const int tid = threadIdx.x, nl = (n + 4 * OMDS_RANK_LANES - 1) & ~(4 * OMDS_RANK_LANES - 1);
    for (int x = tid; x < nl; x += 256) lkey[x] = x < n ? key[x] : 0xffffffffu;
    __syncthreads();
    const int lane = tid % OMDS_RANK_LANES, i = blockIdx.x * OMDS_RANK_ENTRIES + tid / OMDS_RANK_LANES;
    const unsigned mine = lkey[min(i, n - 1)];
    int pos = 0;
    for (int x = 4 * lane; x < nl; x += 4 * OMDS_RANK_LANES) {
        const uint4 k = *reinterpret_cast<const uint4*>(lkey + x);
        pos += (k.x < mine) + (k.y < mine) + (k.z < mine) + (k.w < mine);
    }
#pragma unroll
    for (int d = 1; d < OMDS_RANK_LANES; d <<= 1) pos += __shfl_xor(pos, d, OMDS_RANK_LANES);
    if (i < n) {
        if (lane == 0) perm[pos] = i;
        if (pos == n - 1)
            for (int p = n + lane; p < npad; p += OMDS_RANK_LANES) perm[p] = i;
    }
}

static void launch_order(hipStream_t s, const TileKeys* keys, const float* c, const float* rows, int n, unsigned* key, int* perm) {
    hipLaunchKernelGGL(k_order_keys, dim3((n + OMDS_KEY_ROWS - 1) / OMDS_KEY_ROWS), dim3(OMDS_KEY_ROWS), 0, s, keys, c, rows, n, key);
    const size_t lds = (size_t)((n + 4 * OMDS_RANK_LANES - 1) & ~(4 * OMDS_RANK_LANES - 1)) * sizeof(unsigned);
    hipLaunchKernelGGL(k_order_rank, dim3((n + OMDS_RANK_ENTRIES - 1) / OMDS_RANK_ENTRIES), dim3(256), lds, s, key, n, perm, omds_order_pad(n));
}

void omds_launch_tile_pick(hipStream_t s, const MlpDev& m, const float* Fq, int N, const float* Fp, int O, const TileOrderBufs& b) {
    const int gO = omds_share_groups(O), gR = omds_share_groups(N), F = 3 * m.d;
    hipLaunchKernelGGL(k_share_stats, dim3(gO), dim3(OMDS_WIDTH), 0, s, m.W1t, F, Fp, O, m.b1, nullptr, 0, 1, b.sumO, nullptr);
    hipLaunchKernelGGL(k_share_stats, dim3(gR), dim3(OMDS_WIDTH), 0, s, m.W1t, F, Fq, N, m.b1, b.sumO, gO, O, b.sumR, b.cntR);
    hipLaunchKernelGGL(k_tile_pick, dim3(1), dim3(OMDS_WIDTH), 0, s, m.W1t, m.b1, F, b.sumO, gO, O, b.sumR, b.cntR, gR, N, b.keys);
    launch_order(s, b.keys, b.keys->cO, Fp, O, b.okey, b.operm);
}

// the kernels see a table of `count` rows that starts at the part's first row: the same two launches as for a whole batch
void omds_launch_rollout_order(hipStream_t s, const TileKeys* keys, const float* Fq, int first, int count, unsigned* rkey, int* rperm) {
    launch_order(s, keys, keys->cR, Fq + (size_t)first * OMDS_FROW, count, rkey + first, rperm);
}

void omds_launch_tile_order(hipStream_t s, const MlpDev& m, const float* Fq, int N, const float* Fp, int O, const TileOrderBufs& b,
                            bool pick) {
    if (pick) omds_launch_tile_pick(s, m, Fq, N, Fp, O, b);
    omds_launch_rollout_order(s, b.keys, Fq, 0, N, b.rkey, b.rperm);
}
