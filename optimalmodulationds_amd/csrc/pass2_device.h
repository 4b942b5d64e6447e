// Pass 2: forward and analytic backward on the selected rows (pass2_body, pass2_backward, the first layer's backward and the
// 4-row-group forms).  Included by mlp_kernels.hip (k_pass2), tail_kernel.hip and step_small.hip.
#pragma once
#include "mfma_gemm.h"
#include "timeline_device.h"
#include "trig_device.h"

constexpr int P2_MT = 32;
constexpr int P2_NT = 512;

struct P2Smem {
    float* Hs;        // [32][LDH]
    float* gf;        // [32][33] feature gradients
    uint16_t* maskL;  // [nhh+1][512] ReLU masks, 16 bits per thread and layer
    uint32_t* maskG4; // the same storage seen by the 4-row-group backward: [nhh+1][256 columns], bit e = row e
    int* rowT;        // [32] rollout of each row (-1: padding row)
    int* rowO;        // [32] obstacle of each row
    int* rowMin;      // [32] arg-min link of each row
    const int* rowE = nullptr;   // tanh derivative hand-over (k_tail_sel): [32] list entry whose derivative rows each backward row reads
                                 // (-1: padding row), dscr then being ExactOut::deriv with dlayer = cap * 256; nullptr: row S0 + r of dscr
};

// Geometry of the per-thread accumulator values of a pass-2 tile: ROWS = 32 uses the 32x32x2 MFMA (16 values per thread,
// one column), ROWS = 16 the 16x16x4 MFMA (two 16-column blocks -> 8 values per thread, two columns).
template <int ROWS>
struct P2Geo {
    static constexpr int NV = ROWS == 32 ? 16 : 8;
    static constexpr int NB = ROWS == 32 ? 1 : 2;    // distinct columns per thread
    static __device__ __forceinline__ int row(int r, int lane) { return ROWS == 32 ? crow(r, lane) : 4 * (lane >> 4) + (r & 3); }
    static __device__ __forceinline__ int col(int r, int wave, int lane) {
        return ROWS == 32 ? wave * 32 + (lane & 31) : wave * 32 + 16 * (r >> 2) + (lane & 15);
    }
    static __device__ __forceinline__ int blk(int r) { return ROWS == 32 ? 0 : (r >> 2); }
    // position of that column in the k-permuted tile (omds_kpos keeps groups of eight columns together)
    static __device__ __forceinline__ int pos(int r, int wave, int lane) {
        return ROWS == 32 ? wave * 32 + omds_kpos(lane & 31) : wave * 32 + 16 * (r >> 2) + omds_kpos(lane & 15);
    }
};

// One [ROWS x 256] . [256 x 256] GEMM of pass 2 (forward pack or transposed pack of layer l; l = -1: layer 1 over the encoded
// inputs at positions 0..31, K = 32); out[r] in P2Geo order.  The accumulators start at zero in every product, forward and
// backward (the reference's chains; the forward's bias is added by the caller) -- the same arithmetic as pass1_tile, so the
// forward of a row is bit-identical in pass 1 and pass 2.
template <int ROWS>
__device__ __forceinline__ void p2_gemm(const float* Hs, const MlpDev& m, int l, bool backward, int wave, int lane,
                                        float (&out)[P2Geo<ROWS>::NV]) {
    if constexpr (ROWS == 32) {
        f32x16 acc[1][1];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
        if (l < 0) gemm_k32<1, 1>(Hs, m.W1f, wave, lane, acc);
        else gemm256<1, 1>(Hs, (backward ? m.Wb : m.Wf) + (size_t)l * (OMDS_NCB * 32 * 64), wave, lane, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[r] = acc[0][0][r];
    } else {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        if (l < 0) gemm16_k32(Hs, m.W1f16, wave, lane, acc);
        else gemm16(Hs, (backward ? m.Wb16 : m.Wf16) + (size_t)l * (16 * 16 * 64), wave, lane, acc);
#pragma unroll
        for (int r = 0; r < 8; ++r) out[r] = acc[r >> 2][r & 3];
    }
}

template <int ACT, int ROWS>
__device__ __forceinline__ void pass2_backward(const MlpDev& m, const P2Smem& sm, const float* __restrict__ xyzr, int R0,
                                               int total_rows, const float* __restrict__ qT, int ldq, float* gradx, int dbase,
                                               float* __restrict__ dscr, size_t dlayer, int S0);
template <int ROWS>
__device__ __forceinline__ void p2_backward_first(const MlpDev& m, const P2Smem& sm, const float* __restrict__ xyzr, int R0,
                                                  int total_rows, const float* __restrict__ qT, int ldq, float* gradx, int dbase);

// The last layer of pass 2 on the tile in LDS (v_mfma_f32_16x16x4, waves 0 .. ROWS / 16 - 1), the arg-min over ALL raw outputs
// (robot_sdf.py:155) and the distance of that link: sm.rowMin[r], drow[dbase + r]; optionally the raw outputs, the arg-min per global
// row, and the pass-1 value of each row (d1row: min over the un-ignored links of y / out_div - radius, MPPI.py:236-242).  seed_col >= 0:
// that output column instead of the arg-min one.  Shared by pass2_body and pass2_body_g4 (32 rows there, 20 of them real).
template <int ROWS>
__device__ __forceinline__ void p2_last_layer(const MlpDev& m, const float* Hs, int* rowMin, const int* rowO, const float* __restrict__ radius,
                                              int R0, int total_rows, float* drow, int dbase, float* __restrict__ yraw,
                                              int32_t* __restrict__ minidx, float* d1row, uint32_t ignored, int seed_col) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (wave < ROWS / 16) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* arow = Hs + (wave * 16 + (lane & 15)) * LDH + pa16(lane);
        const int j = lane & 15;
        const float bj = m.bl[j];
        // all 16 weight fragments in flight at once: the MFMA chain below is latency-bound otherwise
        {
            float4 wl[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) wl[c] = m.Wl[c * 64 + lane];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                acc = mfma4_16x16(load_a16(arow, c), wl[c], acc);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = wave * 16 + 4 * (lane >> 4) + reg;
            const int R = R0 + r;
            const float y = acc[reg] + bj;
            if (yraw != nullptr && R < total_rows) yraw[(size_t)R * OMDS_CPAD + j] = (j < m.C) ? y : 0.f;
            float bv = (j < m.C && (seed_col < 0 || j == seed_col)) ? y : __builtin_inff();
            int bi = j;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                if ((ov < bv) || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            if (d1row != nullptr) {
                float v = y / m.out_div - radius[rowO[r]];
                v = (j >= m.C) ? __builtin_inff() : (((ignored >> j) & 1u) ? 1e6f : v);
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) v = fminf(v, __shfl_xor(v, off));
                if (j == 0) d1row[r] = v;
            }
            if (j == 0) {
                rowMin[r] = bi;
                if (R < total_rows) {
                    drow[dbase + r] = bv / m.out_div - radius[rowO[r]];
                    if (minidx != nullptr) minidx[R] = bi;
                }
            }
        }
    }
}

// The rows' encoded inputs Fq[t] | Fp[o] (padding rows: zero), features 0 .. F-1 of each, at positions c0 .. of the k-permuted tile
template <int ROWS>
__device__ __forceinline__ void fill_encoded(float* Hs, const int* rowT, const int* rowO, const float* __restrict__ Fq,
                                             const float* __restrict__ Fp, int c0, int F) {
    for (int e = threadIdx.x; e < ROWS * 32; e += P2_NT) {
        const int r = e >> 5, f = e & 31;
        if (f < F) {
            const int t = rowT[r];
            uint32_t v = 0u;
            if (t >= 0) v = __builtin_bit_cast(uint32_t, Fq[(size_t)t * OMDS_FROW + f]) | __builtin_bit_cast(uint32_t, Fp[(size_t)rowO[r] * OMDS_FROW + f]);
            reinterpret_cast<uint32_t*>(Hs)[r * LDH + omds_kpos(c0 + f)] = v;
        }
    }
}

// Body of pass 2 for the ROWS rows described by sm.rowT / sm.rowO (already in LDS, barrier done by the
// caller).  R0 = global index of row 0 (tanh scratch, yraw, minidx); outputs go to
// gradx[(dbase + row) * d + j] and drow[dbase + row] (global memory or LDS).
template <int ACT, int ROWS = 32>
__device__ __forceinline__ void pass2_body(const MlpDev& m, const P2Smem& sm, const float* __restrict__ Fq,
                                           const float* __restrict__ Fp, const float* __restrict__ radius,
                                           const float* __restrict__ xyzr, int R0, int total_rows,
                                           const float* __restrict__ qT, int ldq, float* gradx, float* drow, int dbase,
                                           float* __restrict__ yraw, int32_t* __restrict__ minidx,
                                           float* __restrict__ dscr, size_t dlayer, int S0,
                                           float* d1row = nullptr, uint32_t ignored = 0, int seed_col = -1) {
    // seed_col >= 0: the backward starts from that output column instead of the arg-min one (one Jacobian column,
    // robot_sdf.py:92-100); minidx / drow then describe that column
    // d1row (optional, [ROWS]): the pass-1 value of each row, min over the un-ignored links of y / out_div - radius
    // (MPPI.py:236-242), computed from the same last-layer outputs -- bit-identical to pass1_tile's Dmin for 32-row tiles
    // S0 = first row of this workgroup's private slot in the tanh scratch
    using G = P2Geo<ROWS>;
    constexpr int NV = G::NV;
    float* Hs = sm.Hs;
    uint16_t* maskL = sm.maskL;
    int* rowT = sm.rowT;
    int* rowO = sm.rowO;
    int* rowMin = sm.rowMin;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr bool relu = ACT == OMDS_ACT_RELU;

    float bnext[G::NB];   // bias of the layer about to be multiplied, fetched one layer ahead (no L2 round trip in front of its epilogue)
#pragma unroll
    for (int jb = 0; jb < G::NB; ++jb) bnext[jb] = m.b1[G::col(4 * jb, wave, lane)];
    // ---- the rows' encoded inputs [x, sin x, cos x] at positions 0..31: Fq[t] | Fp[o] (padding rows: zero) ----------------
    fill_encoded<ROWS>(Hs, rowT, rowO, Fq, Fp, 0, 32);
    __syncthreads();
    // skip-connection networks: the encoded input of each row behind the activations of `level` (MlpDev::skip_mask)
    auto inject = [&](int level) {
        fill_encoded<ROWS>(Hs, rowT, rowO, Fq, Fp, m.skip_col[level], 3 * m.d);
        __syncthreads();
    };

    // ---- forward: layer 1 (l = -1) and the hidden -> hidden layers, each the reference's product (from zero, ascending k, bias
    //      last); level l + 1 of the masks / derivatives ---------------------------------------------------------------------
    for (int l = -1; l < m.nhh; ++l) {
        float bv[G::NB];
#pragma unroll
        for (int jb = 0; jb < G::NB; ++jb) bv[jb] = bnext[jb];
        if (l + 1 < m.nhh) {
#pragma unroll
            for (int jb = 0; jb < G::NB; ++jb) bnext[jb] = m.bh[(l + 1) * OMDS_WIDTH + G::col(4 * jb, wave, lane)];
        }
        float acc[NV];
        p2_gemm<ROWS>(Hs, m, l, false, wave, lane, acc);
        __syncthreads();
        uint32_t bits = 0;
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const int row = G::row(r, lane), col = G::col(r, wave, lane);
            const float z = acc[r] + bv[G::blk(r)];
            bits |= (z > 0.f ? 1u : 0u) << r;
            const float h = actf(z, ACT);
            Hs[row * LDH + G::pos(r, wave, lane)] = h;
            if (!relu) dscr[(l + 1) * dlayer + (size_t)(S0 + row) * OMDS_WIDTH + col] = 1.f - h * h;
        }
        maskL[(l + 1) * P2_NT + tid] = (uint16_t)bits;
        __syncthreads();
        if ((m.skip_mask >> (l + 1)) & 1u) inject(l + 1);
    }

    // ---- last layer, arg-min over ALL raw outputs (robot_sdf.py:155), distance of that link -------
    p2_last_layer<ROWS>(m, Hs, rowMin, rowO, radius, R0, total_rows, drow, dbase, yraw, minidx, d1row, ignored, seed_col);
    __syncthreads();
    pass2_backward<ACT, ROWS>(m, sm, xyzr, R0, total_rows, qT, ldq, gradx, dbase, dscr, dlayer, S0);
}

// 1 - h^2 of (row, col) at one hidden level: from the workgroup's own scratch rows (pass 2 behind its own forward) or, with
// sm.rowE, from the derivative rows k_exact left for the list entry of each backward row (a padding row multiplies by zero)
__device__ __forceinline__ float p2_tanh_deriv(const P2Smem& sm, const float* __restrict__ dscr, size_t level_off, int S0, int row, int col) {
    if (sm.rowE == nullptr) return dscr[level_off + (size_t)(S0 + row) * OMDS_WIDTH + col];
    const int e = sm.rowE[row];   // k_exact wrote its rows as they sit in the tile: column col at position omds_kpos(col)
    return e >= 0 ? dscr[level_off + (size_t)e * OMDS_WIDTH + omds_kpos(col)] : 0.f;
}

// The backward half of pass 2: from sm.rowMin (arg-min link of each row), the activation derivatives -- sm.maskL (ReLU:
// 16 bits per thread and layer in the MFMA C layout) or dscr (tanh) -- and sm.rowT / sm.rowO to the input gradients
// gradx[(dbase + row) * d + j].  pass2_body runs it behind its own forward; the screened step (k_tail_sel) runs it on masks
// that k_exact produced when it evaluated the candidates.
template <int ACT, int ROWS>
__device__ __forceinline__ void pass2_backward(const MlpDev& m, const P2Smem& sm, const float* __restrict__ xyzr, int R0,
                                               int total_rows, const float* __restrict__ qT, int ldq, float* gradx, int dbase,
                                               float* __restrict__ dscr, size_t dlayer, int S0) {
    using G = P2Geo<ROWS>;
    constexpr int NV = G::NV;
    float* Hs = sm.Hs;
    float* gf = sm.gf;
    uint16_t* maskL = sm.maskL;
    int* rowMin = sm.rowMin;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr bool relu = ACT == OMDS_ACT_RELU;

    // skip-connection networks: the gradient that arrives at the concatenated input columns of a level is a direct
    // contribution to the feature gradient; it is collected in gf (one owner thread per element and level)
    const int F3 = 3 * m.d;
    if (m.skip_mask) {
        for (int e = tid; e < ROWS * 33; e += P2_NT) gf[e] = 0.f;
        __syncthreads();
    }
    // ---- backward seed: dy[minIdx]/dH_last = Wlast[minIdx], masked by the last hidden layer ---------
    {
        const uint32_t bits = maskL[m.nhh * P2_NT + tid];
        const bool cap = (m.skip_mask >> m.nhh) & 1u;
        const int c0 = m.skip_col[m.nhh];
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const int row = G::row(r, lane), col = G::col(r, wave, lane);
            const float g = m.Wlraw[(size_t)rowMin[row] * OMDS_WIDTH + col];
            if (cap && col >= c0 && col < c0 + F3) gf[row * 33 + col - c0] += g;
            const float dv = relu ? (((bits >> r) & 1u) ? 1.f : 0.f) : p2_tanh_deriv(sm, dscr, m.nhh * dlayer, S0, row, col);
            Hs[row * LDH + G::pos(r, wave, lane)] = g * dv;
        }
    }
    __syncthreads();
    OMDS_TL_STAMP(4);

    // ---- backward through the hidden -> hidden layers ------------------------------------------
    for (int l = m.nhh - 1; l >= 0; --l) {
        float acc[NV];
        p2_gemm<ROWS>(Hs, m, l, true, wave, lane, acc);
        if (l == m.nhh - 1) OMDS_TL_STAMP(5);
        __syncthreads();
        if (l == m.nhh - 1) OMDS_TL_STAMP(6);
        const uint32_t bits = maskL[l * P2_NT + tid];
        const bool cap = (m.skip_mask >> l) & 1u;
        const int c0 = m.skip_col[l];
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const int row = G::row(r, lane), col = G::col(r, wave, lane);
            const float dv = relu ? (((bits >> r) & 1u) ? 1.f : 0.f) : p2_tanh_deriv(sm, dscr, l * dlayer, S0, row, col);
            if (cap && col >= c0 && col < c0 + F3) gf[row * 33 + col - c0] += acc[r];
            Hs[row * LDH + G::pos(r, wave, lane)] = acc[r] * dv;
        }
        __syncthreads();
        if (l == m.nhh - 1) OMDS_TL_STAMP(7);
    }
    OMDS_TL_STAMP(8);

    p2_backward_first<ROWS>(m, sm, xyzr, R0, total_rows, qT, ldq, gradx, dbase);
}

// d y / d x of one input from the gradients at its three encoded features, as torch's autograd accumulates them for
// x_nerf = cat(x, sin x, cos x) (network_macros_mod.py:139-140): (g_x + g_cos * (-sin x)) + g_sin * cos x, every operation rounded
// on its own (established bit for bit against the reference's gradients, tools/studies/assoc_order_study.py --vjp)
__device__ __forceinline__ float pe_chain_rule(float gx, float gsin, float gcos, float x) {
    return __fadd_rn(__fadd_rn(gx, __fmul_rn(gcos, -omds_sinf(x))), __fmul_rn(gsin, omds_cosf(x)));
}

// The first layer's backward as the reference computes it (robot_sdf.py:153-158: (g * mask) @ W1): for every (row, feature) ONE fmaf
// chain over the 256 hidden units in ascending order from zero.  [ROWS x 256] . [256 x 32] on v_mfma_f32_16x16x4: wave w owns the
// 16 x 16 block (rows 16 (w >> 1), features 16 (w & 1)) and runs the whole k range -- 64 dependent MFMAs, 1 us; splitting k over
// the waves (the round-1 form) was 0.5 us shorter and summed eight partial chains.  Hs = the gradient at the first layer's
// pre-activations (k-permuted tile, read like gemm16); out[row * 33 + f] = the chain (+ prior[row * 33 + f], the skip
// concatenations' direct contributions, when prior != nullptr; out may alias prior).
template <int ROWS>
__device__ __forceinline__ void first_layer_backward(const MlpDev& m, const float* Hs, float* out, const float* prior) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (wave < ROWS / 8) {
        const int rb = wave >> 1, jb = wave & 1;
        const float* arow = Hs + (rb * 16 + (lane & 15)) * LDH + pa16(lane);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float4 wq[16];   // all 16 weight fragments in flight at once: the chain below is latency-bound otherwise
#pragma unroll
        for (int c = 0; c < 16; ++c) wq[c] = m.W1b16[(c * 2 + jb) * 64 + lane];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            acc = mfma4_16x16(load_a16(arow, c), wq[c], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // C/D layout 16x16: column (feature) lane & 15, row 4 (lane >> 4) + r
            const int e = (rb * 16 + 4 * (lane >> 4) + r) * 33 + 16 * jb + (lane & 15);
            out[e] = prior ? acc[r] + prior[e] : acc[r];
        }
    }
}

// The tail of the pass-2 backward: from the gradient at the first layer's pre-activations (sm.Hs) to the input gradients.
template <int ROWS>
__device__ __forceinline__ void p2_backward_first(const MlpDev& m, const P2Smem& sm, const float* __restrict__ xyzr, int R0,
                                                  int total_rows, const float* __restrict__ qT, int ldq, float* gradx, int dbase) {
    float* gf = sm.gf;
    int* rowT = sm.rowT;
    int* rowO = sm.rowO;
    const int tid = threadIdx.x;
    first_layer_backward<ROWS>(m, sm.Hs, gf, m.skip_mask ? gf : nullptr);
    __syncthreads();
    // ---- positional-encoding chain rule -------------------------------------------------------------------------------
    const int d = m.d, n = m.n_dof;
    if (tid < ROWS * d) {
        const int row = tid / d, jj = tid - row * d;
        const int R = R0 + row;
        if (R < total_rows && rowT[row] >= 0) {
            const float x = (jj < n) ? qT[(size_t)jj * ldq + rowT[row]] : xyzr[rowO[row] * 4 + (jj - n)];
            gradx[(size_t)(dbase + row) * d + jj] = pe_chain_rule(gf[row * 33 + jj], gf[row * 33 + d + jj], gf[row * 33 + 2 * d + jj], x);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The hidden part of the pass-2 backward on 4-ROW GROUPS (gemm4): for workgroups whose rows do not fill a 16-row tile.  At
// N = 1024, k = 5 a CU's share is 4 rollouts = 20 rows: five groups of 4 where the 16-row shape needs two blocks (32 rows of
// matrix-pipe time) -- 10240 instead of 16384 MFMA cycles per SIMD and layer.  ReLU networks without skip concatenations;
// the same fmaf chains in the same k order as pass2_backward<ACT, 16 | 32>, so the same bits.
//   waves 0-3: columns 64 w .. +63 of ALL row groups (one wave per SIMD: a second one would fetch the same weight fragments from L2 a second time; weights through the 8-chunk ring across the layers); thread: column 64 w + lane.
// sm.maskG4[l * 256 + column]: bit e = ReLU mask of element (row e, column) at hidden level l (written by the caller BEFORE
// this call, which overwrites the tile buffer).  Leaves the gradient at the first layer's pre-activations in sm.Hs
// (32 rows, the rest 0).
// ------------------------------------------------------------------------------------------------
template <int NG>
__device__ __forceinline__ void pass2_backward_hidden_g4(const MlpDev& m, const P2Smem& sm) {
    float* Hs = sm.Hs;
    const int* rowMin = sm.rowMin;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = wave & 3, col = 64 * cw + lane, pcol = omds_kpos(col);   // the column's position in the k-permuted tile
    const bool mine = wave < 4;   // waves 4-7 take no part in the GEMMs: a second wave per SIMD would fetch the same weight fragments
                                  // from L2 a second time (0.5 B per FLOP on this shape), and that, not the matrix pipe, then bounds the layer
    constexpr int PD = 8;
    W4Ring<PD> ring;
    if (mine) {   // the first chunks of the first GEMM are on their way during the seed
        ring.bind(m.Wb4, m.nhh, cw, lane);
        ring.fill(m.nhh - 1);
    }
    // rows past the last group are zero for the first-layer backward, which runs on the whole 32-row tile
    for (int e = tid; e < (32 - 4 * NG) * OMDS_WIDTH; e += P2_NT) Hs[(4 * NG + e / OMDS_WIDTH) * LDH + (e % OMDS_WIDTH)] = 0.f;
    // ---- seed: dy[minIdx]/dH_last = Wlast[minIdx], masked by the last hidden layer
    if (mine) {
        const uint32_t bseed = sm.maskG4[m.nhh * 256 + (tid & 255)];
#pragma unroll
        for (int e = 0; e < 4 * NG; ++e) {
            const float gz = m.Wlraw[(size_t)rowMin[e] * OMDS_WIDTH + col];
            Hs[e * LDH + pcol] = ((bseed >> e) & 1u) ? gz : 0.f;
        }
    }
    __syncthreads();
    OMDS_TL_STAMP(4);
    for (int l = m.nhh - 1; l >= 0; --l) {
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (mine) gemm4<NG, PD>(Hs, ring, l, l - 1, lane, acc);
        if (l == m.nhh - 1) OMDS_TL_STAMP(5);   // the first GEMM, this wave's share
        __syncthreads();   // every wave has finished reading the tile
        if (l == m.nhh - 1) OMDS_TL_STAMP(6);
        if (mine) {
            const uint32_t bl = sm.maskG4[l * 256 + (tid & 255)];
#pragma unroll
            for (int e = 0; e < 4 * NG; ++e) Hs[e * LDH + pcol] = ((bl >> e) & 1u) ? acc[e >> 2][e & 3] : 0.f;
        }
        __syncthreads();
        if (l == m.nhh - 1) OMDS_TL_STAMP(7);
    }
    OMDS_TL_STAMP(8);
}

// ------------------------------------------------------------------------------------------------
// Pass 2 -- forward AND backward -- on 4-ROW GROUPS, for the all-fp32 tail of large batches (k_tail<ND, ACT, 4>): a workgroup
// owns 4 NG = 20 network rows (four rollouts at k = 5), so that 1024 rollouts are 256 workgroups, one per CU, each multiplying
// five groups of 4 rows per hidden layer where the 32-row tile of 171 workgroups multiplies 32 (11 264 against 16 384 matrix-
// pipe cycles per SIMD and layer, forward and backward).  ReLU networks without skip concatenations.
//   layer 1 (K = 32): the 32-row product of pass2_body on all eight waves (rows >= 4 NG are padding);
//   hidden layers: gemm4 on waves 0-3 (columns 64 w .. +63), forward weights MlpDev::Wf4 through the ring across the layers;
//     the epilogue (bias last, ReLU) leaves the level in the tile and its masks as sm.maskG4[(l + 1) * 256 + column], bit e =
//     row e -- the layout pass2_backward_hidden_g4 reads; level 0's word is read back from the tile (h > 0 <=> z > 0);
//   last layer, arg-min link, distance: as pass2_body; then pass2_backward_hidden_g4 + p2_backward_first<32>.
// The same fmaf chains in the same k order as pass2_body<ACT, 32 | 16>: the same bits per row (tests/test_gpu_screen.py runs the
// shapes against each other).
// ------------------------------------------------------------------------------------------------
// What pass2_body_g4 needs that does not depend on WHICH obstacles the rows are: requested before the caller's top-k, so that the
// kernel's first dependent round trips (a fetch from another XCD's writes takes microseconds) run side by side instead of in a row
struct P2G4Pre {
    W4Ring<8> ring;      // waves 0-3: the first chunks of the first hidden product
    float b1v, bnext;    // biases of layer 1 (this thread's column of the 32-row product) and of the first hidden product
    uint32_t q[2];       // the rollout halves of this thread's two encoded-input elements: rows (tid >> 5) and 16 + (tid >> 5), feature tid & 31
};
// t_of_row(r) = the rollout of tile row r, or -1 (what the top-k will write to sm.rowT[r])
template <typename TOfRow>
__device__ __forceinline__ void pass2_g4_prefetch(const MlpDev& m, const float* __restrict__ Fq, TOfRow t_of_row, P2G4Pre& pre) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = wave & 3, col4 = 64 * cw + lane;
    if (wave < 4) {
        pre.ring.bind(m.Wf4, m.nhh, cw, lane);
        pre.ring.fill(0);
    }
    pre.b1v = m.b1[P2Geo<32>::col(0, wave, lane)];
    pre.bnext = wave < 4 ? m.bh[col4] : 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int t = t_of_row((tid >> 5) + 16 * h);
        pre.q[h] = t >= 0 ? __builtin_bit_cast(uint32_t, Fq[(size_t)t * OMDS_FROW + (tid & 31)]) : 0u;
    }
}

template <int NG>
__device__ __forceinline__ void pass2_body_g4(const MlpDev& m, P2Smem& sm, P2G4Pre& pre, const float* __restrict__ Fp,
                                              const float* __restrict__ radius, const float* __restrict__ xyzr, int R0, int total_rows,
                                              const float* __restrict__ qT, int ldq, float* gradx, float* drow, int dbase) {
    using G = P2Geo<32>;
    float* Hs = sm.Hs;
    int* rowT = sm.rowT;
    int* rowO = sm.rowO;
    int* rowMin = sm.rowMin;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cw = wave & 3, col4 = 64 * cw + lane, pcol = omds_kpos(col4);
    const bool mine = wave < 4;
    sm.maskG4 = reinterpret_cast<uint32_t*>(sm.maskL);   // (nhh + 1) * 256 words <= the (nhh + 1) * 512 halfwords of maskL
    constexpr int PD = 8;
    W4Ring<PD>& ring = pre.ring;
    const float b1v = pre.b1v;
    float bnext = pre.bnext;
    // ---- the rows' encoded inputs at positions 0..31: Fq[t] | Fp[o] (padding rows: zero), as pass2_body; the rollout half is
    //      already here, the two obstacle halves are one round trip -----------------------------------------------------------
    {
        uint32_t pv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = (tid >> 5) + 16 * h;
            pv[h] = rowT[r] >= 0 ? __builtin_bit_cast(uint32_t, Fp[(size_t)rowO[r] * OMDS_FROW + (tid & 31)]) : 0u;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            reinterpret_cast<uint32_t*>(Hs)[((tid >> 5) + 16 * h) * LDH + omds_kpos(tid & 31)] = rowT[(tid >> 5) + 16 * h] >= 0 ? (pre.q[h] | pv[h]) : 0u;
    }
    __syncthreads();
    OMDS_TL_STAMP(3);
    // ---- layer 1 on the 32-row tile ---------------------------------------------------------------------------------------
    {
        float acc[G::NV];
        p2_gemm<32>(Hs, m, -1, false, wave, lane, acc);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < G::NV; ++r) Hs[G::row(r, lane) * LDH + G::pos(r, wave, lane)] = actf(acc[r] + b1v, OMDS_ACT_RELU);
    }
    __syncthreads();
    OMDS_TL_STAMP(17);
    if (mine) {
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 4 * NG; ++e) bits |= (Hs[e * LDH + pcol] > 0.f ? 1u : 0u) << e;
        sm.maskG4[col4] = bits;
    }
    // ---- hidden -> hidden layers on 4-row groups --------------------------------------------------------------------------
    for (int l = 0; l < m.nhh; ++l) {
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float bv = bnext;
        if (mine && l + 1 < m.nhh) bnext = m.bh[(l + 1) * OMDS_WIDTH + col4];
        if (mine) gemm4<NG, PD>(Hs, ring, l, l + 1 < m.nhh ? l + 1 : -1, lane, acc);
        __syncthreads();   // every wave has finished reading the tile
        if (mine) {
            uint32_t bits = 0;
#pragma unroll
            for (int e = 0; e < 4 * NG; ++e) {
                const float z = acc[e >> 2][e & 3] + bv;
                bits |= (z > 0.f ? 1u : 0u) << e;
                Hs[e * LDH + pcol] = actf(z, OMDS_ACT_RELU);
            }
            sm.maskG4[(l + 1) * 256 + col4] = bits;
        }
        __syncthreads();
    }
    OMDS_TL_STAMP(18);
    // ---- last layer, arg-min over ALL raw outputs (robot_sdf.py:155), distance of that link: pass2_body's ---------------------
    p2_last_layer<32>(m, Hs, rowMin, rowO, radius, R0, total_rows, drow, dbase, nullptr, nullptr, nullptr, 0u, -1);
    __syncthreads();
    pass2_backward_hidden_g4<NG>(m, sm);
    p2_backward_first<32>(m, sm, xyzr, R0, total_rows, qT, ldq, gradx, dbase);
}
