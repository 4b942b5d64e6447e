// The row order of the block-ordered pass 1 (k_pass1_dyn_blk, mlp_kernels.hip): which rollouts and which obstacles
// share a tile.  The exact zero-skip multiplies the UNION of the hidden units that fire in a tile, so a tile is cheaper the more
// alike its rows are.  A row's layer-1 pre-activation is a rollout share (the weights over the joint features times Fq[t]) plus an
// obstacle share (the weights over the point features times Fp[o]) plus the bias; the sign bits of OMDS_KEY_UNITS of them,
// taken with the other operand at its mean, are a key per rollout and a key per obstacle, and a tile is a block of consecutive
// rollouts x consecutive obstacles of the two key orders.  Nothing here has to be exact: every permutation of the rows computes the
// same bits, the order only decides how many chunks the products run over.
//
//   k_tile_pick     once per propagate, in front of its first full launch: the key units (the OMDS_KEY_UNITS units whose firing
//                   rate over the N rollouts, obstacle share at its mean, is nearest 1/2; ties by lower unit index), their
//                   weights and constants (TileKeys), and the obstacle order operm of the scene (slab 0 of an obstacle horizon)
//   k_rollout_order once per horizon step, in front of that step's pass 1: the rollout order rperm from Fq
//
// Both orders are the ranks of (key << 20 | index): ties by lower index, the same permutation on every run.
#include "omds_internal.h"

__device__ __forceinline__ float order_dot32(const float (&w)[OMDS_FROW], const float* __restrict__ row) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < OMDS_FROW / 4; ++q) {
        const float4 v = reinterpret_cast<const float4*>(row)[q];
        s = fmaf(w[4 * q], v.x, s); s = fmaf(w[4 * q + 1], v.y, s); s = fmaf(w[4 * q + 2], v.z, s); s = fmaf(w[4 * q + 3], v.w, s);
    }
    return s;
}

// rank of every entry of key[0 .. n) (distinct values; key[n .. n4) hold 0xffffffff) -> perm[rank] = index; the owner of the
// last rank also fills perm[n .. npad) with its index, so that a partial block reads valid rows
__device__ __forceinline__ void order_place(const unsigned* key, int n, int n4, int i, int* __restrict__ perm, int npad) {
    const unsigned mine = key[i];
    int pos = 0;
    for (int x = 0; x < n4; x += 4) {
        const uint4 k = *reinterpret_cast<const uint4*>(key + x);
        pos += (k.x < mine) + (k.y < mine) + (k.z < mine) + (k.w < mine);
    }
    perm[pos] = i;
    if (pos == n - 1)
        for (int p = n; p < npad; ++p) perm[p] = i;
}

__global__ __launch_bounds__(1024) void k_tile_pick(const float* __restrict__ W1t, const float* __restrict__ b1, int F,
                                                    const float* __restrict__ Fq, int N, const float* __restrict__ Fp, int O,
                                                    TileKeys* __restrict__ keys, int* __restrict__ operm, int Opad) {
    __shared__ float part[4][OMDS_WIDTH];
    __shared__ int cnt[4][OMDS_WIDTH];
    __shared__ float meanO[OMDS_WIDTH], meanR[OMDS_WIDTH];
    __shared__ int away[OMDS_WIDTH];                      // |2 firing rollouts - N| of a unit
    __shared__ int sel[OMDS_KEY_UNITS];
    __shared__ __attribute__((aligned(16))) float Wk[OMDS_KEY_UNITS][OMDS_FROW];
    __shared__ float cO[OMDS_KEY_UNITS];
    __shared__ __attribute__((aligned(16))) unsigned okey[OMDS_ORDER_MAX_OBS];
    const int tid = threadIdx.x, u = tid & (OMDS_WIDTH - 1), g = tid >> 8;   // unit u over the rows g, g + 4, ...
    float w[OMDS_FROW];
#pragma unroll
    for (int f = 0; f < OMDS_FROW; ++f) w[f] = f < F ? W1t[(size_t)f * OMDS_WIDTH + u] : 0.f;
    // mean obstacle share of every unit (each table is zero in the other operand's slots: one dot product serves both shares)
    float so = 0.f;
    for (int o = g; o < O; o += 4) so += order_dot32(w, Fp + (size_t)o * OMDS_FROW);
    part[g][u] = so;
    __syncthreads();
    if (g == 0) meanO[u] = (part[0][u] + part[1][u] + part[2][u] + part[3][u]) / (float)O;
    __syncthreads();
    // firing rate and mean rollout share of every unit
    const float c = b1[u] + meanO[u];
    float sr = 0.f;
    int fire = 0;
    for (int t = g; t < N; t += 4) {
        const float r = order_dot32(w, Fq + (size_t)t * OMDS_FROW);
        sr += r;
        fire += (r + c > 0.f) ? 1 : 0;
    }
    part[g][u] = sr;
    cnt[g][u] = fire;
    __syncthreads();
    if (g == 0) {
        meanR[u] = (part[0][u] + part[1][u] + part[2][u] + part[3][u]) / (float)N;
        const int n2 = 2 * (cnt[0][u] + cnt[1][u] + cnt[2][u] + cnt[3][u]) - N;
        away[u] = n2 < 0 ? -n2 : n2;
    }
    __syncthreads();
    if (tid < OMDS_WIDTH) {
        int rank = 0;
        for (int v = 0; v < OMDS_WIDTH; ++v) rank += (away[v] < away[u] || (away[v] == away[u] && v < u)) ? 1 : 0;
        if (rank < OMDS_KEY_UNITS) sel[rank] = u;
    }
    __syncthreads();
    if (tid < OMDS_KEY_UNITS * OMDS_FROW) {
        const int j = tid / OMDS_FROW, f = tid % OMDS_FROW;
        const float v = f < F ? W1t[(size_t)f * OMDS_WIDTH + sel[j]] : 0.f;
        Wk[j][f] = v;
        keys->W[j][f] = v;
    }
    if (tid < OMDS_KEY_UNITS) {
        const int s = sel[tid];
        keys->cR[tid] = b1[s] + meanO[s];
        keys->unit[tid] = s;
        cO[tid] = b1[s] + meanR[s];
    }
    __syncthreads();
    // the obstacle order: key bit j = unit sel[j] fires at obstacle o with the rollout share at its mean
    const int O4 = (O + 3) & ~3;
    for (int o = tid; o < O4; o += 1024) {
        unsigned key = 0xffffffffu;
        if (o < O) {
            const float4* row = reinterpret_cast<const float4*>(Fp + (size_t)o * OMDS_FROW);
            float x[OMDS_FROW];
#pragma unroll
            for (int q = 0; q < OMDS_FROW / 4; ++q) { const float4 v = row[q]; x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w; }
            unsigned bits = 0u;
#pragma unroll 1
            for (int j = 0; j < OMDS_KEY_UNITS; ++j) {
                float s = cO[j];
#pragma unroll
                for (int f = 0; f < OMDS_FROW; ++f) s = fmaf(Wk[j][f], x[f], s);
                bits |= (s > 0.f ? 1u : 0u) << j;
            }
            key = (bits << 20) | (unsigned)o;
        }
        okey[o] = key;
    }
    __syncthreads();
    for (int o = tid; o < O; o += 1024) order_place(okey, O, O4, o, operm, Opad);
}

__global__ __launch_bounds__(256) void k_rollout_order(const TileKeys* __restrict__ keys, const float* __restrict__ Fq, int N,
                                                       int* __restrict__ rperm, int Npad) {
    extern __shared__ __attribute__((aligned(16))) unsigned rkey[];   // [N rounded up to 4]: every workgroup holds all keys, and ranks 256 of them
    __shared__ __attribute__((aligned(16))) float Wk[OMDS_KEY_UNITS][OMDS_FROW];
    __shared__ float cR[OMDS_KEY_UNITS];
    const int tid = threadIdx.x;
    for (int e = tid; e < OMDS_KEY_UNITS * OMDS_FROW; e += 256) Wk[e / OMDS_FROW][e % OMDS_FROW] = keys->W[e / OMDS_FROW][e % OMDS_FROW];
    if (tid < OMDS_KEY_UNITS) cR[tid] = keys->cR[tid];
    __syncthreads();
    const int N4 = (N + 3) & ~3;
    for (int t = tid; t < N4; t += 256) {
        unsigned key = 0xffffffffu;
        if (t < N) {
            const float4* row = reinterpret_cast<const float4*>(Fq + (size_t)t * OMDS_FROW);
            float x[OMDS_FROW];
#pragma unroll
            for (int q = 0; q < OMDS_FROW / 4; ++q) { const float4 v = row[q]; x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w; }
            unsigned bits = 0u;
#pragma unroll 1
            for (int j = 0; j < OMDS_KEY_UNITS; ++j) {
                float s = cR[j];
#pragma unroll
                for (int f = 0; f < OMDS_FROW; ++f) s = fmaf(Wk[j][f], x[f], s);
                bits |= (s > 0.f ? 1u : 0u) << j;
            }
            key = (bits << 20) | (unsigned)t;
        }
        rkey[t] = key;
    }
    __syncthreads();
    const int t = blockIdx.x * 256 + tid;
    if (t < N) order_place(rkey, N, N4, t, rperm, Npad);
}

void omds_launch_tile_order(hipStream_t s, const MlpDev& m, const float* Fq, int N, const float* Fp, int O, TileKeys* keys,
                            int* rperm, int* operm, bool pick) {
    if (pick)
        hipLaunchKernelGGL(k_tile_pick, dim3(1), dim3(1024), 0, s, m.W1t, m.b1, 3 * m.d, Fq, N, Fp, O, keys, operm, omds_order_pad(O));
    hipLaunchKernelGGL(k_rollout_order, dim3((N + 255) / 256), dim3(256), (size_t)((N + 3) & ~3) * 4, s, keys, Fq, N, rperm, omds_order_pad(N));
}
