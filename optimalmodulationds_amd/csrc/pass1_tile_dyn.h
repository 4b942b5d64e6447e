// The compacting pass-1 tile (k_pass1_dyn, k_pass1_dyn_blk): the by-unit gather product gemm_gather and pass1_tile_dyn in
// natural and block order.  Included by mlp_kernels.hip.
#pragma once
#include "pass1_tile.h"

// ------------------------------------------------------------------------------------------------
// pass 1 with PER-TILE COMPACTION of the hidden levels (k_pass1's 32- and 64-row tiles, ReLU networks without skips).
// A hidden unit whose activation is exactly zero in every row of the tile adds fmaf(0, w, acc) = acc to every chain of the next
// layer: leaving it out changes no bit, whatever the order -- as long as the units that ARE multiplied keep their ascending order.
// So every level is stored COMPACTED: a wave ballots which of its 32 units fired in the tile, the eight masks meet in LDS at the
// barrier every layer has anyway, and a unit's position is its rank among the tile's firing units (k-permuted by omds_kpos like
// every tile); dead columns are not stored at all.  The next product runs over ceil(T / 8) chunks, T = firing units of the tile
// (164 / 195 / 146 / 130 of 256 on the shelf task), and fetches its weight fragments BY UNIT: W^T rows (one per unit, 1 KB) named by
// the position -> unit table the epilogue leaves in LDS -- four coalesced 256-byte loads per chunk instead of one 1 KB fragment.
// Exact for every input: nothing is presumed about which units fire.
// ------------------------------------------------------------------------------------------------
// an LDS location as its 32-bit byte address, and a 16-byte read from one (ds_read_b128 with an immediate offset)
// (the host pass of the compiler parses device functions too: it has no LDS address space to cast into)
__device__ __forceinline__ uint32_t omds_lds_addr(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(size_t)(const __attribute__((address_space(3))) void*)p;
#else
    return 0u;
#endif
}
__device__ __forceinline__ float4 omds_lds_f4(uint32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const omds_f4 v = *(const __attribute__((address_space(3))) omds_f4*)a;
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return make_float4(0.f, 0.f, 0.f, 0.f);
#endif
}
constexpr int OMDS_IDS = OMDS_WIDTH + 64;   // entries of the position -> unit table (the pipelines read up to four 16-position chunks ahead)

template <int MR>
__device__ __forceinline__ void gemm_gather(const float* __restrict__ Hw, const uint32_t* __restrict__ idsS, const float* __restrict__ WT, int cb0,
                                            int lane, f32x16 (&acc)[MR][1], int nch, unsigned long long* tl_first = nullptr) {
    // LDS byte addresses, as integers: the two running addresses stay two registers with immediate offsets (derived from one another
    // by the optimiser they cost three additions per chunk)
    uint32_t arow = omds_lds_addr(Hw + (lane & 31) * LDH + 4 * (lane >> 5));
    uint32_t irow = omds_lds_addr(idsS + 4 * (lane >> 5));   // this lane half's four positions of a chunk: 8c + 4h .. + 3
    const __amdgpu_buffer_rsrc_t wt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(WT) + __builtin_amdgcn_readfirstlane(cb0) * 32, 0,
                                                                        OMDS_WIDTH * OMDS_WIDTH * 4, 0x00020000);
    const int colb = (lane & 31) * 4;
    float4 a0[MR], a1[MR];
    float b0[4], b1[4];
    uint4 i0, i1;
    auto loadA = [&](uint32_t ar, float4 (&a)[MR]) {
#pragma unroll
        for (int i = 0; i < MR; ++i) a[i] = omds_lds_f4(ar + i * 32 * LDH * 4);
    };
    auto loadI = [&](uint32_t ir) { return __builtin_bit_cast(uint4, omds_lds_f4(ir)); };
    auto loadB = [&](const uint4& id, float (&b)[4]) {   // W^T[unit][column]: byte offset unit * 1024 (the table's entry) + column * 4
        b[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wt, (int)id.x + colb, 0, 0));
        b[1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wt, (int)id.y + colb, 0, 0));
        b[2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wt, (int)id.z + colb, 0, 0));
        b[3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wt, (int)id.w + colb, 0, 0));
    };
    auto mfma4 = [&](const float4 (&a)[MR], const float (&b)[4]) {
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[0], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[1], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[2], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[3], acc[i][0], 0, 0, 0);
    };
    auto mfma4_first = [&](const float4 (&a)[MR], const float (&b)[4]) {   // the chain starts here: C = 0 is the instruction's literal, no accumulator is cleared
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[0], zero, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[1], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[2], acc[i][0], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < MR; ++i) acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[3], acc[i][0], 0, 0, 0);
    };
    // three stages: the table entries of chunk c + 2 (LDS), the operands of chunk c + 1 (LDS, L2), the MFMAs of chunk c.
    // Chunk 0 is peeled so that no accumulator is cleared (a VALU instruction beside the MFMAs is not free: EXPERIMENTS.md R6.11, R6.13).
    const int n = __builtin_amdgcn_readfirstlane(nch);
    if (n == 0) {
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
        return;
    }
    i0 = loadI(irow);
    i1 = loadI(irow + 32);
    loadA(arow, a0);
    loadB(i0, b0);
    loadA(arow + 32, a1);
    loadB(i1, b1);
    i0 = loadI(irow + 64);
    __builtin_amdgcn_sched_barrier(0);
#ifdef OMDS_TIMELINE   // diagnostic build: when this product's first operands are here (tl_first: thread 0's slot)
    if (tl_first) { OMDS_TL_WAIT("vmcnt(4) lgkmcnt(1)"); *tl_first = wall_clock64(); }
#endif
    mfma4_first(a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    // now (a1, b1) is chunk 1, i0 the table entries of chunk 2
    const int npair = (n - 1) >> 1;
#pragma unroll 1
    for (int p = 0; p < npair; ++p) {
        loadA(arow + 64, a0);
        loadB(i0, b0);
        i1 = loadI(irow + 96);
        __builtin_amdgcn_sched_barrier(0);
        mfma4(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
        loadA(arow + 96, a1);
        loadB(i1, b1);
        i0 = loadI(irow + 128);
        __builtin_amdgcn_sched_barrier(0);
        mfma4(a0, b0);
        __builtin_amdgcn_sched_barrier(0);
        arow += 64;
        irow += 64;
        asm volatile("" : "+v"(arow), "+v"(irow));
    }
    if ((n - 1) & 1) mfma4(a1, b1);   // an even count: the last chunk is the one the final pair (or the prologue) fetched
}

#ifndef OMDS_DYN_PRIO_PROD
#define OMDS_DYN_PRIO_PROD 0
#endif
#ifndef OMDS_DYN_PRIO_EPI
#define OMDS_DYN_PRIO_EPI 3
#endif
#define OMDS_DYN_PRIO(p) __builtin_amdgcn_s_setprio(p)
// BLK (k_pass1_dyn_blk): the tile is a block of MT / 4 consecutive rollouts of the rollout order x 4 consecutive obstacles of the
// obstacle order (tile_order.hip) instead of MT consecutive rows: row r = rollout slot r / 4, obstacle slot r % 4.  Both orders are
// padded with their last entry, so a partial block holds copies of rows it has anyway (they add nothing to the union of firing
// units) and only the stores look at the counts.  Dmin stays [N][O] in the caller's indices: four scalars per row group.
struct TileBlock {
    const int* rp;   // the block's rollouts: MT / 4 entries of the rollout order, the first nr of them real
    const int* op;   // the block's obstacles: 4 entries of the obstacle order, the first no of them real
    int nr, no;
};
template <int MT, int MR, bool BLK = false>
__device__ __forceinline__ void pass1_tile_dyn(const MlpDev& m, float* smem, const float* __restrict__ Fq, const float* __restrict__ Fp,
                                               const float* __restrict__ radius, int O, long long total_rows, uint32_t ignored,
                                               float* __restrict__ Dmin, const long long row0, const OmdsDivisor odiv,
                                               const TileBlock blk = TileBlock{}) {
    using G = Geo<MT, MR, 1>;
    static_assert(G::NW == 8 && G::WM == 1, "eight waves, wave w owns the units 32 w .. 32 w + 31 of every level");
    constexpr Pass1DynLds lds(MT);                                 // pass1_plan_def.h
    float* Hs = smem + lds.Hs;                                     // [MT][LDH]
    float* rowRad = smem + lds.rowRad;                             // [MT]
    uint32_t* aliveS = reinterpret_cast<uint32_t*>(smem + lds.aliveS);   // [8] which of a wave's 32 units fired in this tile at the current level
    uint32_t* idsS = reinterpret_cast<uint32_t*>(smem + lds.idsS);       // [OMDS_IDS] position -> unit * 1024 of the current level
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int col = wv * 32 + (lane & 31);                         // the unit this thread's accumulators hold, at every level
    float bcur = m.b1[col];
    OMDS_DYN_PRIO(OMDS_DYN_PRIO_EPI);   // outside its products a wave's VALU / LDS work competes with the co-resident workgroup's MFMA stream for issue
    if (tid < OMDS_IDS - OMDS_WIDTH) idsS[OMDS_WIDTH + tid] = 0u;  // behind the table: valid offsets for the pipeline's look-ahead
    OMDS_TL(0);
    OMDS_TL_HWID(15);

    // ---- the tile's encoded inputs.  The natural order is pass1_tile's un-listed gather with another radius fetch (one vector load here, a v_writelane
    //      per row there, in a loop that also serves the listed forms): a copy, because a shared loop with a hook per row for that difference is longer
    if constexpr (BLK) {
        // wave wv fills rows wv + 8 it: obstacle slot wv & 3 in all of them, rollout slots (wv >> 2) + 2 it.  The ids are wave-uniform:
        // scalar loads, all of them issued before the first is used
        constexpr int IT = MT / G::NW;
        const __amdgpu_buffer_rsrc_t qr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Fq), 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Fp), 0, 0x7fffffff, 0x00020000);
        const bool hi = lane >= 32;
        const int f4 = (lane & 31) * 4;
        const int offp = blk.op[wv & 3] * (OMDS_FROW * 4);
        int offq[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) offq[it] = blk.rp[(wv >> 2) + 2 * it] * (OMDS_FROW * 4);
        const uint32_t fp = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(pr, offp + f4, 0, 0);
        uint32_t fv[IT / 2];
#pragma unroll
        for (int it = 0; it < IT; it += 2)
            fv[it / 2] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(qr, (hi ? offq[it + 1] : offq[it]) + f4, 0, 0) | fp;
        uint32_t* frow = reinterpret_cast<uint32_t*>(Hs) + (wv + (hi ? G::NW : 0)) * LDH + omds_kpos(lane & 31);
#pragma unroll
        for (int it = 0; it < IT; it += 2) frow[it * G::NW * LDH] = fv[it / 2];
        // what the last layer needs of the block: rowRad[0 .. 3] the obstacles' radii, behind them the rollout of every slot and the
        // obstacle of every slot (-1: padding, not stored)
        int* slotT = reinterpret_cast<int*>(smem + lds.slotT);
        int* slotO = reinterpret_cast<int*>(smem + lds.slotO);
        if (tid < 4) {
            const int o = blk.op[tid];
            rowRad[tid] = radius[o];
            slotO[tid] = tid < blk.no ? o : -1;
        } else if (tid >= 64 && tid < 64 + MT / 4) {
            slotT[tid - 64] = tid - 64 < blk.nr ? blk.rp[tid - 64] : -1;
        }
    } else {
        constexpr int IT = MT / G::NW;
        const unsigned row0u = (unsigned)row0;
        const unsigned t0 = odiv.div(row0u);
        const int rows_here = (int)((total_rows - row0 < MT) ? (total_rows - row0) : MT);
        const __amdgpu_buffer_rsrc_t qr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Fq) + (size_t)t0 * OMDS_FROW, 0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t pr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Fp), 0, 0x7fffffff, 0x00020000);
        const bool hi = lane >= 32;
        const int f4 = (lane & 31) * 4;
        int o = (int)(row0u - t0 * (unsigned)O) + wv, dt = 0;
        while (o >= O) { o -= O; ++dt; }
        // the radius of row wv + 8 j by lane j: one vector load (a scalar load per row is a chain of IT L2 round trips in front of the tile)
        float myrad = 0.f;
        if (lane < IT && wv + lane * G::NW < rows_here) {
            const unsigned g = row0u + (unsigned)(wv + lane * G::NW);
            myrad = radius[g - odiv.div(g) * (unsigned)O];
        }
        uint32_t fv[IT / 2];
#pragma unroll
        for (int it = 0; it < IT; it += 2) {
            int offq[2], offp[2];
            bool ok[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                ok[h] = wv + (it + h) * G::NW < rows_here;
                offq[h] = ok[h] ? dt * (OMDS_FROW * 4) : 0;
                offp[h] = ok[h] ? o * (OMDS_FROW * 4) : 0;
                o += G::NW;
                while (o >= O) { o -= O; ++dt; }
            }
            const uint32_t fq = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(qr, (hi ? offq[1] : offq[0]) + f4, 0, 0);
            const uint32_t fp = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(pr, (hi ? offp[1] : offp[0]) + f4, 0, 0);
            fv[it / 2] = (hi ? ok[1] : ok[0]) ? (fq | fp) : 0u;
        }
        uint32_t* frow = reinterpret_cast<uint32_t*>(Hs) + (wv + (hi ? G::NW : 0)) * LDH + omds_kpos(lane & 31);
#pragma unroll
        for (int it = 0; it < IT; it += 2) frow[it * G::NW * LDH] = fv[it / 2];
        if (lane < IT) rowRad[wv + lane * G::NW] = myrad;
    }
    __syncthreads();
    OMDS_TL(1);

    // ---- layer 1 (l = -1) and the hidden -> hidden layers on the compacted tile -----------------------------------------
    int T = 0;   // firing units of the level in the tile
    for (int l = -1; l < m.nhh; ++l) {
        f32x16 acc[MR][1];
        const float bnow = bcur;
        if (l + 1 < m.nhh) bcur = m.bh[(l + 1) * OMDS_WIDTH + col];
        OMDS_TLE(l, 0);
        OMDS_DYN_PRIO(OMDS_DYN_PRIO_PROD);
        if (l < 0) {
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;
            gemm_k32<MR, 1>(Hs, m.W1f, wv, lane, acc);
        }
#ifdef OMDS_TIMELINE
        else gemm_gather<MR>(Hs, idsS, m.WhT + (size_t)l * (OMDS_WIDTH * OMDS_WIDTH), wv, lane, acc, (T + 7) >> 3,
                             (m.tl && threadIdx.x == 0 && l < 3) ? m.tl + (size_t)blockIdx.x * 16 + 11 + l : nullptr);
#else
        else gemm_gather<MR>(Hs, idsS, m.WhT + (size_t)l * (OMDS_WIDTH * OMDS_WIDTH), wv, lane, acc, (T + 7) >> 3);
#endif
        OMDS_DYN_PRIO(OMDS_DYN_PRIO_EPI);
        OMDS_TL(2 + 2 * (l + 1));   // this wave's share of the product done (diagnostic build)
        OMDS_TLE(l, 1);
        // bias (last, as the reference adds it), ReLU, and which of this wave's units fired in the tile (the column of lane l and of
        // lane l + 32 is the same unit).  v_max_f32 / v_max3_f32 written out: fmaxf() would canonicalise every operand first
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float z = acc[i][0][r] + bnow;
                asm("v_max_f32_e32 %0, 0, %1" : "=v"(acc[i][0][r]) : "v"(z));
            }
        float zm = 0.f;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int r = 0; r < 16; r += 2) asm("v_max3_f32 %0, %1, %2, %3" : "=v"(zm) : "v"(zm), "v"(acc[i][0][r]), "v"(acc[i][0][r + 1]));
        const unsigned long long bal = __ballot(zm > 0.f);
        const uint32_t mine = (uint32_t)bal | (uint32_t)(bal >> 32);
        if (lane == 0) aliveS[wv] = mine;
        OMDS_TLE(l, 2);
        __syncthreads();  // every wave has finished reading the tile and the table; the eight masks are there
        OMDS_TLE(l, 3);
        const uint4 mlo = *reinterpret_cast<const uint4*>(aliveS), mhi = *reinterpret_cast<const uint4*>(aliveS + 4);
        const uint32_t mk[8] = {mlo.x, mlo.y, mlo.z, mlo.w, mhi.x, mhi.y, mhi.z, mhi.w};
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const int cnt = __builtin_popcount(__builtin_amdgcn_readfirstlane(mk[w]));
            base += w < wv ? cnt : 0;
            total += cnt;
        }
        T = total;
        if (tid == 0) {   // statistics (omds_pass1_skip_stats): chunks the consumer of this level multiplies, firing units
            atomicAdd(m.skip_stats + 1 + (l + 1), (unsigned long long)(l + 1 < m.nhh ? (T + 7) >> 3 : (T + 15) >> 4));
            atomicAdd(m.skip_stats + 1 + (OMDS_MAX_HIDDEN + 1) + (l + 1), (unsigned long long)T);
            if (l < 0) atomicAdd(m.skip_stats, 1ull);
        }
        const bool alive = (mine >> (lane & 31)) & 1u;
        const int rank = base + __builtin_popcount(mine & ((1u << (lane & 31)) - 1u));
        if (alive) {
            const int pos = omds_kpos(rank);
            float* hb = Hs + (4 * (lane >> 5)) * LDH + pos;
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) hb[(i * 32 + (r & 3) + 8 * (r >> 2)) * LDH] = acc[i][0][r];
            if (lane < 32) idsS[pos] = (uint32_t)col * (OMDS_WIDTH * 4);
        }
        // zero columns up to the next multiple of 16 positions (the chunks of both consumers are whole); their table entries: unit 0
        const int Tp = (T + 15) & ~15;
        constexpr int CPP = G::NT / MT;   // columns one pass of the workgroup clears (8 or 16 of at most 15)
#pragma unroll
        for (int it = 0; it < (15 + CPP - 1) / CPP; ++it) {
            const int pz = T + tid / MT + it * CPP;
            if (pz < Tp) {
                Hs[(tid % MT) * LDH + omds_kpos(pz)] = 0.f;
                if (tid % MT == 0) idsS[omds_kpos(pz)] = 0u;
            }
        }
        OMDS_TLE(l, 4);
        __syncthreads();
        OMDS_TLE(l, 5);
        OMDS_TL(3 + 2 * (l + 1));
    }

    // ---- last layer (256 -> C, padded to 16) on v_mfma_f32_16x16x4_f32 over the compacted level, weights by unit from WlT ----
    const __amdgpu_buffer_rsrc_t wlt = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(m.WlT), 0, OMDS_WIDTH * 16 * 4, 0x00020000);
    const int nch16 = (T + 15) >> 4;
    for (int rb = wv; rb < MT / 16; rb += G::NW) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* arow = Hs + (rb * 16 + (lane & 15)) * LDH + pa16(lane);
        const uint32_t* ir = idsS + pa16(lane);
        const int jb = (lane & 15) * 4;
        const int r4 = rb * 16 + 4 * (lane >> 4);
        constexpr int LPD = 4;
        float wq[LPD][4];
        auto loadW = [&](const uint32_t* ic, float (&w)[4]) {   // WlT[unit][link]: byte offset unit * 64 = table entry / 16
            w[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wlt, (int)(ic[0] >> 4) + jb, 0, 0));
            w[1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wlt, (int)(ic[2] >> 4) + jb, 0, 0));
            w[2] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wlt, (int)(ic[8] >> 4) + jb, 0, 0));
            w[3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wlt, (int)(ic[10] >> 4) + jb, 0, 0));
        };
        auto mfma4 = [&](const float* ac, const float (&w)[4]) {
            acc = mfma4_16x16(load_a16(ac, 0), make_float4(w[0], w[1], w[2], w[3]), acc);
        };
        // the weights run LPD chunks ahead of the chain, in a ROLLED loop of LPD chunks per trip (a guard per chunk in an unrolled
        // loop made every chunk wait for the newest fetch); the fetches behind the level read the table's look-ahead entries
#pragma unroll
        for (int c = 0; c < LPD; ++c) loadW(ir + 16 * c, wq[c]);
        __builtin_amdgcn_sched_barrier(0);
        int c = 0;
#pragma unroll 1
        for (; c + LPD <= nch16; c += LPD) {
#pragma unroll
            for (int q = 0; q < LPD; ++q) {
                mfma4(arow + 16 * q, wq[q]);
                loadW(ir + 16 * (LPD + q), wq[q]);
                __builtin_amdgcn_sched_barrier(0);
            }
            arow += 16 * LPD;
            ir += 16 * LPD;
        }
#pragma unroll
        for (int q = 0; q < LPD - 1; ++q)
            if (c + q < nch16) mfma4(arow + 16 * q, wq[q]);
        const int j = lane & 15;
        const float bj = m.bl[j];
        const bool pad = j >= m.C, ign = (ignored >> j) & 1u;
        const float4 rr = *reinterpret_cast<const float4*>(rowRad + (BLK ? 0 : r4));   // BLK: the four rows of a group are the block's four obstacles
        const float rad[4] = {rr.x, rr.y, rr.z, rr.w};
        float y[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) y[reg] = link_row_distance(acc[reg], bj, pad, ign, m.out_div, rad[reg]);
        if constexpr (BLK) {
            if (j == 0) {
                const int t = reinterpret_cast<const int*>(smem + lds.slotT)[r4 >> 2];
                if (t >= 0) {
                    const int4 oo = *reinterpret_cast<const int4*>(smem + lds.slotO);
                    float* drow = Dmin + (size_t)t * O;
                    if (oo.x >= 0) drow[oo.x] = y[0];
                    if (oo.y >= 0) drow[oo.y] = y[1];
                    if (oo.z >= 0) drow[oo.z] = y[2];
                    if (oo.w >= 0) drow[oo.w] = y[3];
                }
            }
        } else
        if (j == 0) store_dmin4(Dmin, row0 + r4, total_rows, y);
    }
#ifdef OMDS_TIMELINE
    __syncthreads();
    OMDS_TL(10);
#endif
}
