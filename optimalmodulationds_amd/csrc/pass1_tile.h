// The dense pass-1 tile: pass1_tile in all its forms (k_pass1, k_pass1e, k_exact, k_audit, k_step_small) and the divisor by
// multiplication its row bookkeeping uses.  Included by mlp_kernels.hip, screen_kernel.hip, screen_exact.hip, screen_stats.hip, step_small.hip and pass1_tile_dyn.h.
#pragma once
#include "mfma_gemm.h"
#include "timeline_device.h"

// ------------------------------------------------------------------------------------------------
// pass 1: all (rollout, obstacle) pairs -> min link distance
// ------------------------------------------------------------------------------------------------

// n / d for 0 <= n < 2^32 by multiplication (Granlund-Montgomery): q = (mulhi(mul, n) + n) >> shift with
// shift = ceil(log2 d), mul = floor(2^32 (2^shift - d) / d) + 1; n < 2^31 here, so the sum cannot overflow.
struct OmdsDivisor {
    unsigned mul;
    int shift;
    __device__ __forceinline__ unsigned div(unsigned n) const { return (__umulhi(mul, n) + n) >> shift; }
    static OmdsDivisor make(unsigned d) {
        OmdsDivisor r;
        r.shift = 0;
        while ((1ull << r.shift) < d) ++r.shift;
        r.mul = (unsigned)((((1ull << r.shift) - d) << 32) / d + 1);
        return r;
    }
};

// The forms of pass1_tile.  The arithmetic of a row is the same in all of them and independent of the other rows of the tile: bit-identical results.
enum class TileMode {
    Dmin,       // The tile covers rows row0 .. row0+MT-1 of the virtual rollout-major pair space (row = t*O + o) and writes Dmin[row].  (k_pass1,
                // k_pass1_mixed)
    List,       // Screening, screen_exact.hip: the tile covers entries row0 .. of `rowlist`, each naming a pair t*O + o; the exact value, what pass
                // 2's forward would compute for the row (pass-2 distance, arg-min link) and the ReLU masks go to ex->... per list entry, and max
                // |screening value - exact value| to *maxerr_bits.  (k_exact, ReLU)
    SmallScene, // Fused small-O step, step_small.hip: rows as in Dmin, outputs as in List but indexed by the row within the tile (ex-> pointers are
                // LDS arrays) and the masks stay in the tile's LDS block (maskS, behind rowIdx).  (k_step_small)
    ListPatch,  // Screened step of tanh networks: rows as in List; the exact value overwrites the pair's screening value in Dmin, max |screening -
                // exact| goes to *maxerr_bits, nothing else is kept.  (k_exact, tanh matrix route)
    Audit,      // Audit sample: rows as in List, the rollout index of a pair running over all horizon steps' states; no outputs but max (ex->Da[entry]
                // - exact value) into maxerr_bits[2].  With SLAB (the audit sample of a propagate with an obstacle horizon, this mode only): Fp /
                // radius hold one slab of slab_ld rows per horizon step and the pair's rollout index tt runs over all steps' states, ndiv.div(tt) = tt
                // / N being its step: the obstacle row is (tt / N) * slab_ld + o.  A template flag: without it the function is the code it was.
                // (k_audit, k_audit_slabs)
    ListDeriv,  // Screened step of tanh networks with the derivative hand-over: List with the rows' activation derivatives 1 - h^2 of every hidden
                // layer (ex->deriv[(level * cap + entry) * 256 + column]: 1 KB per entry and layer, written row-wise from the tile) in place of the
                // ReLU masks -- what pass 2's forward would have left in its scratch, so that the tail runs the backward only (k_tail_sel).  (k_exact,
                // tanh)
    EmitAll,    // The all-fp32 step without a second forward: rows and Dmin as in Dmin, and what List leaves per list entry -- pass-2 distance,
                // arg-min link, ReLU masks -- for EVERY pair, indexed by the pair (ex->dr / amin / mask [row]): the forward of the k rows a rollout
                // ends up selecting has been computed here anyway, so the tail selects from Dmin and runs the backward only.  (k_pass1e*)
};
constexpr bool tile_lists(TileMode m) { return m == TileMode::List || m == TileMode::ListPatch || m == TileMode::Audit || m == TileMode::ListDeriv; }   // rows are entries of `rowlist`
constexpr bool tile_emits_masks(TileMode m) { return m == TileMode::List || m == TileMode::SmallScene || m == TileMode::EmitAll; }   // the ReLU masks of every level are kept
constexpr bool tile_emits_deriv(TileMode m) { return m == TileMode::ListDeriv; }                                                       // ... the activation derivatives
constexpr bool tile_emits_y(TileMode m) { return tile_emits_masks(m) || tile_emits_deriv(m); }   // pass 2's distance and arg-min link per row (ex->dr, ex->amin)

// The last layer's epilogue, from links to the row's distance: a = one accumulator value of the lane (a row of the 16x16 C tile, link j = lane & 15);
// bias, out_div, the row's radius; padding links count as inf, ignored links as 1e6; minimum over the 16 links.  One row per call, everything by
// value: with the lane's four rows passed as arrays all eight k_pass1 kernels came out with other register names (EXPERIMENTS.md R16).
__device__ __forceinline__ float link_row_distance(float a, float bj, bool pad, bool ign, float out_div, float rad) {
    const float v = (a + bj) / out_div - rad;
    return row16_min_f32(pad ? __builtin_inff() : (ign ? 1e6f : v));
}
// Four consecutive rows g .. g+3 of Dmin, g a multiple of 4: one 16-byte store, guarded scalars where the row space ends inside the four.
__device__ __forceinline__ void store_dmin4(float* __restrict__ Dmin, long long g, long long total_rows, const float (&y)[4]) {
    if (g + 3 < total_rows) *reinterpret_cast<float4*>(Dmin + g) = make_float4(y[0], y[1], y[2], y[3]);
    else {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) if (g + reg < total_rows) Dmin[g + reg] = y[reg];
    }
}

template <int MT, int MR, int NR, int ACT, TileMode MODE = TileMode::Dmin, bool SLAB = false>
__device__ __forceinline__ void pass1_tile(const MlpDev& m, float* smem, const float* __restrict__ Fq,
                                           const float* __restrict__ Fp, const float* __restrict__ radius, int O,
                                           long long total_rows, uint32_t ignored, float* __restrict__ Dmin,
                                           const long long row0, const OmdsDivisor odiv,
                                           const int* __restrict__ rowlist = nullptr, unsigned* maxerr_bits = nullptr,
                                           const ExactOut* ex = nullptr, [[maybe_unused]] const OmdsDivisor ndiv = OmdsDivisor{0u, 0},
                                           [[maybe_unused]] const unsigned slab_ld = 0u) {
    static_assert(!SLAB || MODE == TileMode::Audit, "obstacle slabs per listed row: the audit sample only");
    constexpr bool LIST = tile_lists(MODE), EMIT = tile_emits_masks(MODE), DERIV = tile_emits_deriv(MODE), EMITY = tile_emits_y(MODE);
    static_assert(!DERIV || MT == 16, "the derivative hand-over is written for the 16-row tiles of k_exact");
    using G = Geo<MT, MR, NR>;
    const int nhid = m.nhh + 1;
    constexpr Pass1Lds lds(MT, 0);                              // the blocks and what each launch reserves of them: pass1_plan_def.h (nhid moves the end only)
    float* Hs = smem + lds.Hs;                                  // [MT][LDH]
    float* rowRad = smem + lds.rowRad;                          // [MT] obstacle radius of each row
    int* rowIdx = reinterpret_cast<int*>(smem + lds.rowIdx);    // [MT] LIST: pair index of each row
    uint32_t* maskS = reinterpret_cast<uint32_t*>(smem + lds.maskS);   // [MT][nhid][8] EMIT: ReLU masks of the tile's rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / G::WN, wn = wave % G::WN;
    // ListDeriv: the activation derivatives of the tile's rows at `level`, row-wise (a wave per row, one float4 per lane: 1 KB
    // coalesced) from the activations the epilogue has just left in the tile; after the barrier behind the epilogue
    [[maybe_unused]] auto emit_deriv = [&](int level) {
        if constexpr (DERIV) {
            for (int r = wave; r < MT; r += G::NW) {
                const long long e_idx = row0 + r;
                if (e_idx < total_rows && e_idx < ex->cap) {
                    const float4 h = *reinterpret_cast<const float4*>(Hs + r * LDH + 4 * lane);
                    float4 dv;
                    dv.x = 1.f - h.x * h.x; dv.y = 1.f - h.y * h.y; dv.z = 1.f - h.z * h.z; dv.w = 1.f - h.w * h.w;
                    *reinterpret_cast<float4*>(ex->deriv + ((size_t)level * ex->cap + (size_t)e_idx) * OMDS_WIDTH + 4 * lane) = dv;
                }
            }
            if ((m.skip_mask >> level) & 1u) __syncthreads();   // the concatenated inputs are about to be written into these rows
        }
    };
    OMDS_TL(0);
    OMDS_TL_HWID(7);

    const int cb0 = wn * NR;
    constexpr int NBIAS = MT == 16 ? 2 : NR;   // distinct output columns per thread
    auto bias_col = [&](int j) { return MT == 16 ? wave * 32 + 16 * j + (lane & 15) : (cb0 + j) * 32 + (lane & 31); };
    float bcur[NBIAS];   // bias of the layer about to be multiplied, fetched one layer ahead (layer 1's: in flight across the gather)
#pragma unroll
    for (int j = 0; j < NBIAS; ++j) bcur[j] = m.b1[bias_col(j)];

    // ---- the tile's encoded inputs: row r = pair (t, o) gets Fq[t] | Fp[o] (each table is zero in the other's slots) at positions
    //      0..31.  A wave fills two rows per step, one per lane half; the row bookkeeping (rollout t, obstacle o, bounds) is
    //      wave-uniform and stays on the scalar unit, the fetches are buffer loads.  Kept short on purpose: next to a co-resident
    //      workgroup that streams MFMAs these instructions issue at roughly one per MFMA slot (tools/ubench/corun.hip), and the
    //      matrix pipe idles whenever both residents of a CU are outside their GEMM loops (tools/pass1_timeline.py). ----------
    {
        constexpr int IT = MT / G::NW;                          // rows per wave
        static_assert(IT % 2 == 0, "two rows per step");
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        const unsigned row0u = (unsigned)row0;                  // the launcher keeps total_rows below 2^31
        const unsigned t0 = LIST ? 0u : odiv.div(row0u);        // row0 / O by multiplication (three scalar instructions)
        const int rows_here = (int)((total_rows - row0 < MT) ? (total_rows - row0) : MT);
        const __amdgpu_buffer_rsrc_t qr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Fq) + (size_t)t0 * OMDS_FROW, 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Fp), 0, 0x7fffffff, 0x00020000);
        const bool hi = lane >= 32;
        const int f4 = (lane & 31) * 4;
        int o = LIST ? 0 : (int)(row0u - t0 * (unsigned)O) + wv, dt = 0;   // un-listed rows: row r = wv + it * NW is pair (t0 + dt, o)
        if constexpr (!LIST) { while (o >= O) { o -= O; ++dt; } }
        float myrad = 0.f;                                      // lane it of the wave collects the radius of its row it
        int myidx = 0;
        uint32_t fv[IT / 2];
#pragma unroll
        for (int it = 0; it < IT; it += 2) {
            int offq[2], offp[2];
            bool ok[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ok[h] = wv + (it + h) * G::NW < rows_here;
                float rad = 0.f;
                int idx = 0;
                offq[h] = 0; offp[h] = 0;
                if constexpr (LIST) {
                    if (ok[h]) {
                        idx = __builtin_amdgcn_readfirstlane(rowlist[row0 + wv + (it + h) * G::NW]);
                        const unsigned tt = odiv.div((unsigned)idx);
                        int oo = (int)((unsigned)idx - tt * (unsigned)O);
                        if constexpr (SLAB) oo += (int)(ndiv.div(tt) * slab_ld);   // the row of the step's slab (wave-uniform, like tt)
                        offq[h] = (int)(tt * (OMDS_FROW * 4)); offp[h] = oo * (OMDS_FROW * 4);
                        rad = radius[oo];
                    }
                } else {
                    if (ok[h]) { offq[h] = dt * (OMDS_FROW * 4); offp[h] = o * (OMDS_FROW * 4); rad = radius[o]; }
                    o += G::NW;
                    while (o >= O) { o -= O; ++dt; }
                }
                const int rbits = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, rad));   // wave-uniform: keep it in an SGPR for the asm
                asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(myrad) : "s"(rbits), "n"(it + h));
                if constexpr (LIST) {
                    const int ib = __builtin_amdgcn_readfirstlane(idx);
                    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(myidx) : "s"(ib), "n"(it + h));
                }
            }
            const uint32_t fq = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(qr, (hi ? offq[1] : offq[0]) + f4, 0, 0);
            const uint32_t fp = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(pr, (hi ? offp[1] : offp[0]) + f4, 0, 0);
            fv[it / 2] = (hi ? ok[1] : ok[0]) ? (fq | fp) : 0u;   // rows past the end: zero inputs (their results are never stored)
        }
        OMDS_TL_WAIT("vmcnt(0)");
        OMDS_TL(8);
        uint32_t* frow = reinterpret_cast<uint32_t*>(Hs) + (wv + (hi ? G::NW : 0)) * LDH + omds_kpos(lane & 31);
#pragma unroll
        for (int it = 0; it < IT; it += 2) frow[it * G::NW * LDH] = fv[it / 2];
        if (lane < IT) rowRad[wv + lane * G::NW] = myrad;
        if constexpr (LIST) { if (lane < IT) rowIdx[wv + lane * G::NW] = myidx; }
    }
    OMDS_TL_WAIT("lgkmcnt(0)");
    OMDS_TL(9);
    __syncthreads();
    OMDS_TL(1);
    // skip-connection networks: the encoded input of each row goes behind the activations of `level` (MlpDev::skip_mask)
    auto inject = [&](int level) {
        const int c0 = m.skip_col[level], F = 3 * m.d;
        for (int e = tid; e < MT * 32; e += G::NT) {
            const int r = e >> 5, f = e & 31;
            if (f < F) {
                uint32_t v = 0u;
                if (row0 + r < total_rows) {
                    unsigned pair;
                    if constexpr (LIST) pair = (unsigned)rowIdx[r];
                    else pair = (unsigned)row0 + (unsigned)r;
                    const unsigned t = odiv.div(pair);
                    unsigned o = pair - t * (unsigned)O;
                    if constexpr (SLAB) o += ndiv.div(t) * slab_ld;
                    v = __builtin_bit_cast(uint32_t, Fq[(size_t)t * OMDS_FROW + f]) | __builtin_bit_cast(uint32_t, Fp[(size_t)o * OMDS_FROW + f]);
                }
                reinterpret_cast<uint32_t*>(Hs)[r * LDH + omds_kpos(c0 + f)] = v;
            }
        }
        __syncthreads();
    };

    // ---- layer 1 (l = -1, K = 32 over the encoded inputs) and the hidden -> hidden layers, each the reference's product: the
    //      accumulators start at ZERO, the k order is ascending (omds_kpos), the bias is added in the epilogue ----------------
    const float* Hw = Hs + (wm * MR * 32) * LDH;
    if constexpr (MT == 16) {
        const int scol0 = wave * 32 + omds_kpos(lane & 15);   // position of column wave*32 + 16 j + (lane & 15): + 16 j
        for (int l = -1; l < m.nhh; ++l) {
            f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            float bnow[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) bnow[j] = bcur[j];
            if (l + 1 < m.nhh) {
#pragma unroll
                for (int j = 0; j < 2; ++j) bcur[j] = m.bh[(l + 1) * OMDS_WIDTH + bias_col(j)];
            }
            if (l < 0) gemm16_k32(Hs, m.W1f16, wave, lane, acc);
            else gemm16(Hs, m.Wf16 + (size_t)l * (16 * 16 * 64), wave, lane, acc);
            __syncthreads();  // every wave has finished reading the tile
            if (l == 0) OMDS_TL(6);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] += bnow[j];
            if constexpr (EMIT) {   // ReLU masks of this level: row 4g + reg = ballot bits of lanes 16g .. 16g+15, columns 32 wave + 16 j + (lane & 15)
                uint32_t mw = 0;
                const int sh = 16 * ((lane & 15) >> 2);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const unsigned long long b0 = __ballot(acc[0][reg] > 0.f), b1 = __ballot(acc[1][reg] > 0.f);
                    if ((lane & 3) == reg) mw = (uint32_t)((b0 >> sh) & 0xffffu) | ((uint32_t)((b1 >> sh) & 0xffffu) << 16);
                }
                if (lane < 16) maskS[((size_t)lane * nhid + (l + 1)) * 8 + wave] = mw;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
                Hs[(4 * (lane >> 4) + (r & 3)) * LDH + scol0 + 16 * (r >> 2)] = actf(acc[r >> 2][r & 3], ACT);
            __syncthreads();
            emit_deriv(l + 1);
            if ((m.skip_mask >> (l + 1)) & 1u) inject(l + 1);
            OMDS_TL(2 + (l < 0 ? 0 : l));
        }
    } else
    for (int l = -1; l < m.nhh; ++l) {
        f32x16 acc[MR][NR];
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        float bnow[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) bnow[j] = bcur[j];
        if (l + 1 < m.nhh) {
#pragma unroll
            for (int j = 0; j < NR; ++j) bcur[j] = m.bh[(l + 1) * OMDS_WIDTH + (cb0 + j) * 32 + (lane & 31)];
        }
        if (l < 0) gemm_k32<MR, NR>(Hw, m.W1f, cb0, lane, acc);
        else gemm256<MR, NR>(Hw, m.Wf + (size_t)l * (OMDS_NCB * 32 * 64), cb0, lane, acc);
        __syncthreads();  // every wave has finished reading the tile
        if (l == 0) OMDS_TL(6);
        // one lane-dependent base address per column block; everything else of (row, col) is a compile-time offset, so the
        // 16 * MR stores of a block use immediate offsets (hipcc otherwise builds a VGPR address per row: VALU = matrix-pipe time)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            float* hb = Hs + (wm * MR * 32 + 4 * (lane >> 5)) * LDH + (cb0 + j) * 32 + omds_kpos(lane & 31);
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float z = acc[i][j][r] + bnow[j];
                    hb[(i * 32 + (r & 3) + 8 * (r >> 2)) * LDH] = actf(z, ACT);
                    if constexpr (EMIT) {   // lanes 0-31 hold row (r&3) + 8(r>>2) of this 32-column block, lanes 32-63 that row + 4
                        const unsigned long long bal = __ballot(z > 0.f);
                        if (lane == 0) {
                            const int rr = wm * MR * 32 + i * 32 + (r & 3) + 8 * (r >> 2);
                            maskS[((size_t)rr * nhid + (l + 1)) * 8 + cb0 + j] = (uint32_t)bal;
                            maskS[((size_t)(rr + 4) * nhid + (l + 1)) * 8 + cb0 + j] = (uint32_t)(bal >> 32);
                        }
                    }
                }
        }
        __syncthreads();
        if ((m.skip_mask >> (l + 1)) & 1u) inject(l + 1);
        OMDS_TL(2 + (l < 0 ? 0 : l));
    }

    // ---- last layer (256 -> C, padded to 16) on v_mfma_f32_16x16x4_f32, 16 rows per wave.  Kept short on purpose
    //      (buffer loads with constant offsets, DPP min over the 16 link lanes, one 16-byte store per 4 rows): like
    //      the layer-1 build it mostly runs starved next to the other resident workgroup's GEMM ----------------
    const __amdgpu_buffer_rsrc_t wlr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4*>(m.Wl), 0, 16 * 64 * 16, 0x00020000);
    for (int rb = __builtin_amdgcn_readfirstlane(wave); rb < MT / 16; rb += G::NW) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* arow = Hs + (rb * 16 + (lane & 15)) * LDH + pa16(lane);   // the k sequence of gemm16 (ascending k through omds_kpos)
        const int r4 = rb * 16 + 4 * (lane >> 4);
        [[maybe_unused]] float scr[4];   // LIST: the screening values of this lane's four rows (guard), in flight across the MFMA loop
        if constexpr (LIST) {
            const bool have_da = MODE == TileMode::Audit || ex->Da != nullptr;   // the pair's screening value: the copy the selection took, or k_screen's matrix
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                scr[reg] = (row0 + r4 + reg < total_rows) ? (have_da ? ex->Da[row0 + r4 + reg] : Dmin[rowIdx[r4 + reg]]) : 0.f;
        }
        // 64 dependent MFMAs on one accumulator (the k order is the row's bits): the weights must not add a trip to L2 per
        // chunk on top.  Four chunks in flight, each slot re-armed when it has been consumed; sched_barrier keeps the requests
        // where they are written (left alone the loop was load, wait, four MFMAs, sixteen times).  k_exact 37.0 -> 36.5 us; 8 or 16
        // chunks in flight need its 80-register cap lifted (two workgroups per CU instead of three) and lose what they gain.
        constexpr int LPD = 4;
        omds_f4 wq[LPD];
#pragma unroll
        for (int c = 0; c < LPD; ++c) {
            wq[c] = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(wlr, lane * 16, c * 64 * 16, 0));
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const omds_f4 w = wq[c % LPD];
            acc = mfma4_16x16(load_a16(arow, c), make_float4(w.x, w.y, w.z, w.w), acc);
            if (c + LPD < 16) wq[c % LPD] = __builtin_bit_cast(omds_f4, __builtin_amdgcn_raw_buffer_load_b128(wlr, lane * 16, (c + LPD) * 64 * 16, 0));
            __builtin_amdgcn_sched_barrier(0);
        }
#ifdef OMDS_TIMELINE
        asm volatile("s_nop 0" ::"v"(acc[0]) : "memory");
        OMDS_TL(10);
#endif
        // C/D layout 16x16: col = lane&15 (link), row = 4(lane>>4) + reg
        const int j = lane & 15;
        const float bj = m.bl[j];
        const bool pad = j >= m.C, ign = (ignored >> j) & 1u;
        const float4 rr = *reinterpret_cast<const float4*>(rowRad + r4);
        const float rad[4] = {rr.x, rr.y, rr.z, rr.w};
        float y[4];
        [[maybe_unused]] float ydr[4];
        [[maybe_unused]] int yam[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            if constexpr (EMITY) {   // pass 2's arg-min over ALL raw outputs (robot_sdf.py:155) and the distance of that link:
                // the minimum over the 16 link lanes by DPP, then the lowest lane holding it from a ballot (ties: lower link,
                // as a compare-and-swap reduction by (value, index) would give; eight dependent cross-lane shuffles shorter)
                const float yv = pad ? __builtin_inff() : acc[reg] + bj;
                const float mn = row16_min_f32(yv);
                const unsigned long long eq = __ballot(yv == mn);
                const unsigned bits = (unsigned)(eq >> (lane & 48)) & 0xffffu;
                ydr[reg] = mn / m.out_div - rad[reg];
                yam[reg] = bits ? __builtin_ctz(bits) : 0;
            }
            y[reg] = link_row_distance(acc[reg], bj, pad, ign, m.out_div, rad[reg]);
        }
        if constexpr (LIST) {
            if (j == 0) {
                float me = 0.f;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const long long e_idx = row0 + r4 + reg;
                    if (e_idx < total_rows) {
                        // candidates (List): |Da - D| -> maxerr_bits[0].  Audit sample (Audit: pairs that were NOT candidates):
                        // the one-sided Da - D the selection rule bounds by eps -> maxerr_bits[2]; a non-candidate whose
                        // screening value is too LOW is harmless, one too HIGH by more than eps could hide a top-k row
                        const float e = MODE == TileMode::Audit ? scr[reg] - y[reg] : fabsf(scr[reg] - y[reg]);   // (List, ListPatch, ListDeriv: candidates)
                        if (!(e <= me)) me = (e == e) ? e : __builtin_inff();   // a NaN screening value (fp16 overflow) counts as an infinite error
                        if constexpr (MODE == TileMode::List || MODE == TileMode::ListDeriv) {
                            if (e_idx < ex->cap) { ex->D[e_idx] = y[reg]; ex->dr[e_idx] = ydr[reg]; ex->amin[e_idx] = yam[reg]; }
                        }
                        if constexpr (MODE == TileMode::ListPatch) Dmin[rowIdx[r4 + reg]] = y[reg];   // the exact value takes the screening value's place
                    }
                }
                if (me > 0.f) atomicMax(maxerr_bits + (MODE == TileMode::Audit ? 2 : 0), __builtin_bit_cast(unsigned, me));   // non-negative floats order like their bits
            }
        } else if constexpr (MODE == TileMode::SmallScene) {
            if (j == 0) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) { ex->D[r4 + reg] = y[reg]; ex->dr[r4 + reg] = ydr[reg]; ex->amin[r4 + reg] = yam[reg]; }
            }
        } else
        if (j == 0) {
            const long long g = row0 + r4;   // row0 and r4 are multiples of 4
            if constexpr (MODE != TileMode::EmitAll) store_dmin4(Dmin, g, total_rows, y);
            else if (g + 3 < total_rows) {   // EmitAll: its three rows under ONE guard (through store_dmin4 each has its own: k_pass1e + 3 % instructions)
                *reinterpret_cast<float4*>(Dmin + g) = make_float4(y[0], y[1], y[2], y[3]);
                *reinterpret_cast<float4*>(ex->dr + g) = make_float4(ydr[0], ydr[1], ydr[2], ydr[3]);
                *reinterpret_cast<int4*>(ex->amin + g) = make_int4(yam[0], yam[1], yam[2], yam[3]);
            } else {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if (g + reg < total_rows) { Dmin[g + reg] = y[reg]; ex->dr[g + reg] = ydr[reg]; ex->amin[g + reg] = yam[reg]; }
            }
        }
    }
    if constexpr (MODE == TileMode::List || MODE == TileMode::EmitAll) {   // the tile's rows are consecutive entries (list entries / pairs): one contiguous block of masks
        __syncthreads();
        const long long words = (long long)((total_rows - row0 < MT) ? (total_rows - row0) : MT) * nhid * 8;
        for (int i = tid; i < words; i += G::NT) {
            const long long e_idx = row0 + i / (nhid * 8);
            if (e_idx < ex->cap) ex->mask[(size_t)row0 * nhid * 8 + i] = maskS[i];
        }
    }
#ifdef OMDS_TIMELINE
    __syncthreads();
    OMDS_TL(5);
#endif
}
