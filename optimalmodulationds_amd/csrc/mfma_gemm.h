// The fp32 MFMA GEMM cores of the distance-network kernels (32x32x2: gemm256, gemm_k32; 16x16x4: gemm16, gemm16_k32; 4-row groups: W4Ring, gemm4), their
// C-layout helpers and the tile geometry (Geo).  Included by the pass-1 and pass-2 headers, and on its own by train_kernels.hip (f32x16, LDH) and tools/ubench/gemm_loop.hip.
#pragma once
#include "omds_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define LDH OMDS_LDH

// hidden activation: ReLU (all shipped reference networks) or tanh (MATLAB-prototype style nets)
__device__ __forceinline__ float actf(float z, int act) { return act == OMDS_ACT_RELU ? fmaxf(z, 0.f) : tanhf(z); }

// ------------------------------------------------------------------------------------------------
// [MR*32 x 256] . [256 x NR*32] on v_mfma_f32_32x32x2_f32
//   A (activations) from LDS: lane l reads H[row = l&31 (+32 per row block)][8c + 4(l>>5) .. +3]
//   B (weights) from global, packed so that lane l's float4 = W[32 cb + (l&31)][8c + 4(l>>5) .. +3]
//   MFMA step m of chunk c contracts k = 8c + m (lanes 0-31) and k = 8c + 4 + m (lanes 32-63).
// ------------------------------------------------------------------------------------------------
template <int MR, int NR>
__device__ __forceinline__ void mfma_chunk(const float4 (&a)[MR], const float4 (&w)[NR], f32x16 (&acc)[MR][NR]) {
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, w[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, w[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, w[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, w[j].w, acc[i][j], 0, 0, 0);
}

// Weight fragments come through a buffer descriptor (SGPR base + per-lane byte offset + SCALAR chunk offset):
// a flat global_load needs 64-bit VALU address arithmetic per load, and VALU instructions take issue slots away
// from the MFMAs of the same SIMD -- in the isolated loop (tools/ubench/gemm_loop.hip) buffer loads issue at 65.7
// cycles per MFMA (the MFMA-only floor is 65.3), global loads at 68.7.
typedef float omds_f4 __attribute__((ext_vector_type(4)));
template <int MR, int NR>
__device__ __forceinline__ void load_chunk(const float* arow, __amdgpu_buffer_rsrc_t wrsrc, int wvoff, int c,
                                           float4 (&a)[MR], float4 (&w)[NR]) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const omds_f4 v = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wvoff, (j * (32 * 64) + c * 64) * 16, 0));
        w[j] = make_float4(v.x, v.y, v.z, v.w);
    }
#pragma unroll
    for (int i = 0; i < MR; ++i) a[i] = *reinterpret_cast<const float4*>(arow + i * 32 * LDH + 8 * c);
}

// Software-pipelined by hand: the fragments of chunk c+1 (one global_load_dwordx4 per column block,
// one ds_read_b128 per row block) are issued BEFORE the 4*MR*NR MFMAs of chunk c and pinned there
// with sched_barrier (left alone, hipcc sinks the loads next to their use and waits vmcnt(0) per chunk).
template <int MR, int NR>
__device__ __forceinline__ void gemm256(const float* __restrict__ Hw, const float4* __restrict__ Wp, int cb0,
                                        int lane, f32x16 (&acc)[MR][NR]) {
    const float* arow = Hw + (lane & 31) * LDH + 4 * (lane >> 5);
    // cb0 derives from the wave index: wave-uniform, but only readfirstlane makes that provable to the compiler
    const float4* wbase = Wp + (size_t)__builtin_amdgcn_readfirstlane(cb0) * (32 * 64);
    const __amdgpu_buffer_rsrc_t wp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(wbase), 0, NR * 32 * 64 * 16, 0x00020000);
    const int wv = lane * 16;
    float4 a0[MR], a1[MR], w0[NR], w1[NR];
    load_chunk<MR, NR>(arow, wp, wv, 0, a0, w0);
    // One load (the weight fragment first, then the LDS reads) is slotted after every MFMA of the first half
    // of a cluster via sched_group_barrier: in the isolated loop (tools/ubench/gemm_loop.hip) this issues at
    // 68.6 cycles per MFMA against 70.3 for "all loads, then the cluster" and 75 for hipcc's own schedule.
#define OMDS_INTERLEAVE()                                                             \
    _Pragma("unroll") for (int q_ = 0; q_ < NR; ++q_) {                               \
        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);                             \
    }                                                                                 \
    _Pragma("unroll") for (int q_ = 0; q_ < MR; ++q_) {                               \
        __builtin_amdgcn_sched_group_barrier(0x8, 2, 0);                              \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                            \
    }                                                                                 \
    __builtin_amdgcn_sched_group_barrier(0x8, 4 * MR * NR - NR - 2 * MR, 0);          \
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 32; c += 2) {   // fully unrolled: every LDS / buffer offset is an immediate or an SGPR, no VALU in the loop
        load_chunk<MR, NR>(arow, wp, wv, c + 1, a1, w1);
        mfma_chunk<MR, NR>(a0, w0, acc);
        OMDS_INTERLEAVE()
        load_chunk<MR, NR>(arow, wp, wv, (c + 2) & 31, a0, w0);   // last iteration re-loads chunk 0 (harmless)
        mfma_chunk<MR, NR>(a1, w1, acc);
        OMDS_INTERLEAVE()
    }
#undef OMDS_INTERLEAVE
}

// C/D layout of the 32x32 MFMA: lane l, register r -> row (r&3) + 8(r>>2) + 4(l>>5), col l&31.
__device__ __forceinline__ int crow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ------------------------------------------------------------------------------------------------
// [16 x 256] . [256 x 32] on v_mfma_f32_16x16x4_f32 -- the GEMM of the 16-row pass-2 tiles used for small batches,
// where a tile's chain of dependent GEMMs is the latency of the whole horizon step: half the rows = half the MFMA
// time per GEMM (3.4 us instead of 6.8 us on the four SIMDs of a CU).
//   Lane group g = l>>4 contracts, in steps 0..3 of chunk c, k = 16c + pa[g] + {0, 2, 8, 10} with pa = {0, 4, 1, 5}: the K
//   index of an MFMA runs over the lane groups, so the products of an output element are added in the order
//   16c + {0,4,1,5, 2,6,3,7, 8,12,9,13, 10,14,11,15} -- exactly the order of the 32-row kernels (gemm256: chunk of 8 k, step j
//   adds k = 8c'+j then 8c'+4+j).  Both MFMAs are plain fmaf chains in k order (tools/ubench/mfma_order.hip), so a row gets
//   the SAME bits from a 16-row and a 32-row tile.  A from LDS: two ds_read2_b32 per chunk; B packed alike (Wf16 / Wb16).
//   C/D: lane l, reg r -> row 4(l>>4)+r, col l&15.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pa16(int lane) { const int g = lane >> 4; return (g >> 1) + 4 * (g & 1); }
__device__ __forceinline__ float4 load_a16(const float* arow, int c) {   // arow = H + row * LDH + pa16(lane)
    return make_float4(arow[16 * c], arow[16 * c + 2], arow[16 * c + 8], arow[16 * c + 10]);
}
__device__ __forceinline__ void load_chunk16(const float* arow, __amdgpu_buffer_rsrc_t wrsrc, int wvoff, int c, float4& a, float4 (&w)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const omds_f4 v = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wvoff, (j * 16 + c) * 64 * 16, 0));
        w[j] = make_float4(v.x, v.y, v.z, v.w);
    }
    a = load_a16(arow, c);
}
__device__ __forceinline__ void mfma_chunk16(const float4& a, const float4 (&w)[2], f32x4 (&acc)[2]) {
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[0].x, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[1].x, acc[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[0].y, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[1].y, acc[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[0].z, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[1].z, acc[1], 0, 0, 0);
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[0].w, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[1].w, acc[1], 0, 0, 0);
}
// One chunk of a 16x16x4 chain on ONE accumulator: four dependent MFMAs, k in the order of the four elements of a (load_a16) and w
__device__ __forceinline__ f32x4 mfma4_16x16(float4 a, float4 w, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, acc, 0, 0, 0);
    return acc;
}
// Minimum over the 16 lanes of a DPP row -- the 16 columns of a row of the 16x16 C tile -- left in every lane of the row: xor 1 and
// xor 2 inside the quad (quad_perm [1, 0, 3, 2] and [2, 3, 0, 1]), then row_half_mirror (within 8) and row_mirror (within 16).
// A NaN never wins: v_min_f32 returns the other operand.
__device__ __forceinline__ float row16_min_f32(float v) {
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false)));
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false)));
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false)));
    v = fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false)));
    return v;
}
// Wp = pack of one layer ([16 colblk16][16 kchunk][64 lane]); wave w produces columns 32w .. 32w+31 (blocks 2w, 2w+1)
__device__ __forceinline__ void gemm16(const float* __restrict__ Hs, const float4* __restrict__ Wp, int wave, int lane, f32x4 (&acc)[2]) {
    const float* arow = Hs + (lane & 15) * LDH + pa16(lane);
    const float4* wbase = Wp + (size_t)__builtin_amdgcn_readfirstlane(wave) * (2 * 16 * 64);
    const __amdgpu_buffer_rsrc_t wp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(wbase), 0, 2 * 16 * 64 * 16, 0x00020000);
    const int wv = lane * 16;
    float4 a0, a1, w0[2], w1[2];
    load_chunk16(arow, wp, wv, 0, a0, w0);
#define OMDS_INTERLEAVE16()                                 \
    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);        \
    __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);       \
    __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);        \
    __builtin_amdgcn_sched_group_barrier(0x20, 1, 0);       \
    __builtin_amdgcn_sched_group_barrier(0x8, 2, 0);        \
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      \
    __builtin_amdgcn_sched_group_barrier(0x8, 4, 0);        \
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 16; c += 2) {
        load_chunk16(arow, wp, wv, c + 1, a1, w1);
        mfma_chunk16(a0, w0, acc);
        OMDS_INTERLEAVE16()
        load_chunk16(arow, wp, wv, (c + 2) & 15, a0, w0);
        mfma_chunk16(a1, w1, acc);
        OMDS_INTERLEAVE16()
    }
#undef OMDS_INTERLEAVE16
}

// ------------------------------------------------------------------------------------------------
// Layer 1: [rows x 32] . [32 x 256] over the tile's ENCODED INPUTS [x, sin x, cos x] (3d <= 30 features, zero-padded), which sit
// at positions 0..31 of the tile rows.  The reference computes the layer as one chain over the 3d features in their order
// [q, p, sin q, sin p, cos q, cos p] (network_macros_mod.py:139-141): joint and obstacle terms alternate along the chain, so the
// layer does NOT split into a rollout half plus an obstacle half without changing its bits -- it is a K = 32 product like
// every other layer (four k-chunks of the 32x32x2 shape, two of the 16x16x4 shape), 4 % of a launch's MFMA work.
// ------------------------------------------------------------------------------------------------
template <int MR, int NR>
__device__ __forceinline__ void gemm_k32(const float* __restrict__ Hw, const float4* __restrict__ W1f, int cb0, int lane, f32x16 (&acc)[MR][NR]) {
    const float* arow = Hw + (lane & 31) * LDH + 4 * (lane >> 5);
    const float4* wbase = W1f + (size_t)__builtin_amdgcn_readfirstlane(cb0) * (4 * 64);
    const __amdgpu_buffer_rsrc_t wp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(wbase), 0, NR * 4 * 64 * 16, 0x00020000);
    const int wv = lane * 16;
    float4 a[4][MR], w[4][NR];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const omds_f4 v = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(wp, wv, (j * (4 * 64) + c * 64) * 16, 0));
            w[c][j] = make_float4(v.x, v.y, v.z, v.w);
        }
#pragma unroll
        for (int i = 0; i < MR; ++i) a[c][i] = *reinterpret_cast<const float4*>(arow + i * 32 * LDH + 8 * c);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) mfma_chunk<MR, NR>(a[c], w[c], acc);
}
// W1f16 = [16 colblk16][2 kchunk][64 lane]; wave w produces columns 32w .. 32w+31 (blocks 2w, 2w+1)
__device__ __forceinline__ void gemm16_k32(const float* __restrict__ Hs, const float4* __restrict__ W1f16, int wave, int lane, f32x4 (&acc)[2]) {
    const float* arow = Hs + (lane & 15) * LDH + pa16(lane);
    const float4* wbase = W1f16 + (size_t)__builtin_amdgcn_readfirstlane(wave) * (2 * 2 * 64);
    const __amdgpu_buffer_rsrc_t wp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(wbase), 0, 2 * 2 * 64 * 16, 0x00020000);
    float4 a[2], w[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const omds_f4 v = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(wp, lane * 16, (j * 2 + c) * 64 * 16, 0));
            w[c][j] = make_float4(v.x, v.y, v.z, v.w);
        }
        a[c] = load_a16(arow, c);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) mfma_chunk16(a[c], w[c], acc);
}

// ------------------------------------------------------------------------------------------------
// [4 NG x 256] . [256 x 64] on v_mfma_f32_4x4x1_16B_f32 with the A operand of ONE block broadcast to all 16 blocks
// (cbsz = 4, abid = g): D[i][lane] = fmaf(A[4g + i], B[lane], C[i][lane]) -- 4 rows x 64 columns x k = 1 per instruction at
// the full fp32 MFMA rate (tools/ubench/mfma_4x4.hip: 138-142 TFLOP/s by the wall clock from ONE wave per SIMD with 3-5
// independent chains, against 144-156 for 16x16x4), one fused multiply-add per element (76800 of 76800 random elements).  A
// GEMM on 4-row groups therefore has a row granularity of 4 where the 16x16x4 / 32x32x2 shapes have 16 / 32, and with K = 1 per
// instruction the k order of the 32-row kernels (8c + {0,4,1,5,2,6,3,7}) is just the issue order: bit-identical rows again.
//   A: lane l reads H[row l][k] (one register serves up to 16 row groups; abid picks the group);
//   B: lane l holds W[k][64 cw + l], packed so that one b128 is four consecutive k (MlpDev::Wb4: [layer][4 cb][64 kq][64 lane]).
//   acc[g][i] = element (row 4 g + i, column 64 cw + lane).
// One wave per SIMD does the work (a second one would fetch the same weight fragments a second time), so nothing but its own
// lookahead hides the L2 round trip: the weights stream through a ring of PD chunks (8 k each) that runs ACROSS the layers of
// the chain -- the slot of chunk c is asked for chunk c + PD of the same layer or chunk c + PD - 32 of the next one the moment
// it has been consumed.  sched_barrier pins every request where it is written: left to itself the scheduler sinks the loads
// to their uses (measured: 7.8 us per layer instead of 4.5).  "No next layer" is a VGPR offset of 0xffffffff: out of range
// for the buffer, the load returns zeros and moves no data.
// ------------------------------------------------------------------------------------------------
constexpr int W4_LAYER_BYTES = 4 * 64 * 64 * 16;
template <int PD>
struct W4Ring {
    float4 w[PD][2];
    __amdgpu_buffer_rsrc_t rs;
    int sbase;   // this wave's column block inside a layer pack, bytes
    int vlane;   // lane * 16
    __device__ __forceinline__ void bind(const float4* pack, int nl, int cw, int lane) {
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(pack), 0, nl * W4_LAYER_BYTES, 0x00020000);
        sbase = __builtin_amdgcn_readfirstlane(cw) * (64 * 64 * 16);
        vlane = lane * 16;
    }
    // chunk C (0..31) of layer l into slot S
    template <int S, int C>
    __device__ __forceinline__ void issue(int l) {
        const int voff = l >= 0 ? vlane + l * W4_LAYER_BYTES : -1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const omds_f4 v = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, sbase + (2 * C + h) * 64 * 16, 0));
            w[S][h] = make_float4(v.x, v.y, v.z, v.w);
        }
    }
    // one half (four k) of chunk C of layer l into slot S
    template <int S, int C, int HALF>
    __device__ __forceinline__ void issue_half(int l) {
        const int voff = l >= 0 ? vlane + l * W4_LAYER_BYTES : -1;
        const omds_f4 v = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, sbase + (2 * C + HALF) * 64 * 16, 0));
        w[S][HALF] = make_float4(v.x, v.y, v.z, v.w);
    }
    template <int C = 0>
    __device__ __forceinline__ void fill(int l) {
        if constexpr (C < PD) {
            issue<C, C>(l);
            __builtin_amdgcn_sched_barrier(0);
            fill<C + 1>(l);
        }
    }
};

template <int NG, int G>
__device__ __forceinline__ void g4_step(float av, float bv, f32x4 (&acc)[NG]) {
    if constexpr (G < NG) {
        acc[G] = __builtin_amdgcn_mfma_f32_4x4x1f32(av, bv, acc[G], 4, G, 0);
        g4_step<NG, G + 1>(av, bv, acc);
    }
}
// Chunk C.  The requests that keep the pipeline full -- the two halves of the ring slot the PREVIOUS chunk has freed, the two
// LDS reads of the next chunk's A operand -- are each issued behind one group of MFMAs instead of in a cluster at the chunk
// boundary: an instruction issued in the shadow of a 2-pass MFMA costs nothing, a cluster of them between two MFMAs leaves
// the matrix pipe idle (9.7 cycles per MFMA with the cluster, against the 8.4 one wave can issue).
template <int NG, int PD, int C>
__device__ __forceinline__ void gemm4_chunks(const float* arow, W4Ring<PD>& R, int l, int l_next, float4 a_lo, float4 a_hi, f32x4 (&acc)[NG]) {
    if constexpr (C < 32) {   // chunk C = k 8C .. 8C+7, contracted in the order 8C + {0,4,1,5,2,6,3,7}
        constexpr int CP = C - 1 + PD;   // the chunk that slot (C - 1) % PD takes next
        float4 n_lo = a_lo, n_hi = a_hi;
        const float4 w_lo = R.w[C % PD][0], w_hi = R.w[C % PD][1];
        g4_step<NG, 0>(a_lo.x, w_lo.x, acc);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C >= 1) {
            if constexpr (CP < 32) R.template issue_half<(C - 1) % PD, CP, 0>(l);
            else R.template issue_half<(C - 1) % PD, CP - 32, 0>(l_next);
        }
        __builtin_amdgcn_sched_barrier(0);
        g4_step<NG, 0>(a_hi.x, w_hi.x, acc);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C >= 1) {
            if constexpr (CP < 32) R.template issue_half<(C - 1) % PD, CP, 1>(l);
            else R.template issue_half<(C - 1) % PD, CP - 32, 1>(l_next);
        }
        __builtin_amdgcn_sched_barrier(0);
        g4_step<NG, 0>(a_lo.y, w_lo.y, acc);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C + 1 < 32) n_lo = *reinterpret_cast<const float4*>(arow + 8 * (C + 1));
        __builtin_amdgcn_sched_barrier(0);
        g4_step<NG, 0>(a_hi.y, w_hi.y, acc);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C + 1 < 32) n_hi = *reinterpret_cast<const float4*>(arow + 8 * (C + 1) + 4);
        __builtin_amdgcn_sched_barrier(0);
        g4_step<NG, 0>(a_lo.z, w_lo.z, acc);
        g4_step<NG, 0>(a_hi.z, w_hi.z, acc);
        g4_step<NG, 0>(a_lo.w, w_lo.w, acc);
        g4_step<NG, 0>(a_hi.w, w_hi.w, acc);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (C == 31) {   // the last chunk's own slot: the ring is whole again for the next layer
            constexpr int CL = 31 + PD - 32;
            R.template issue_half<31 % PD, CL, 0>(l_next);
            R.template issue_half<31 % PD, CL, 1>(l_next);
            __builtin_amdgcn_sched_barrier(0);
        }
        gemm4_chunks<NG, PD, C + 1>(arow, R, l, l_next, n_lo, n_hi, acc);
    }
}
// R holds chunks 0 .. PD-1 of layer l (filled, or left by the previous call); on return those of layer l_next
template <int NG, int PD>
__device__ __forceinline__ void gemm4(const float* __restrict__ Hs, W4Ring<PD>& R, int l, int l_next, int lane, f32x4 (&acc)[NG]) {
    static_assert(NG >= 1 && NG <= 8 && 32 % PD == 0, "row groups 0..7 (abid), ring slots that divide the 32 chunks");
    const float* arow = Hs + (lane & 31) * LDH;   // lanes >= 32 re-read rows 0..31: never selected (abid < 8)
    gemm4_chunks<NG, PD, 0>(arow, R, l, l_next, *reinterpret_cast<const float4*>(arow), *reinterpret_cast<const float4*>(arow + 4), acc);
}

template <int MT, int MR, int NR>
struct Geo {
    static constexpr int WM = MT / (32 * MR);
    static constexpr int WN = OMDS_NCB / NR;
    static constexpr int NW = WM * WN;
    static constexpr int NT = NW * 64;
    static_assert(WM >= 1 && WN >= 1 && WM * 32 * MR == MT && WN * NR == OMDS_NCB, "bad tile geometry");
};
// 16-row tile on v_mfma_f32_16x16x4 (gemm16): 8 waves, wave w owns columns 32w .. 32w+31 as two 16-column blocks
template <>
struct Geo<16, 1, 1> {
    static constexpr int WM = 1, WN = 8, NW = 8, NT = 512;
};
