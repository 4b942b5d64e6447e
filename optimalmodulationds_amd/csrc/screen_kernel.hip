// Low-precision SCREENING of pass 1 with exact re-selection (gfx950).
//
// Pass 1 of MPPI.distance_repulsion_nn (MPPI.py:233-253) evaluates the distance network on all N*O (rollout, obstacle)
// pairs, but only feeds the sort that picks the k closest obstacles; the distance and gradient the step uses come from
// pass 2 on those k rows (MPPI.py:259-280).  So the N*O evaluations need not be fp32 as long as the SELECTED SET is the
// fp32 one.  Three kernels replace k_pass1 in the horizon step:
//
//   k_screen  : the network on all pairs in fp16 (v_mfma_f32_32x32x16_f16, fp32 accumulate) -> approximate min link
//               distance Da[t][o].
//   k_select  : per rollout, tau = (k-th smallest Da) + 1.25 eps; every obstacle with Da <= tau is a CANDIDATE.  If the rows
//               that are NOT candidates have a screening error Da - D <= eps and the exact k-th smallest candidate stays eps
//               below tau (the slack guard k_tail_sel checks from exact numbers), the exact top-k over the candidates is the
//               exact top-k over all obstacles, ties included (proof in DESIGN.md 4.3).  The candidates of a rollout take a
//               contiguous range of a compact list (range start, length and tau per rollout).
//   k_exact   : the fp32 pass-1 tile code (pass1_tile, bit-identical arithmetic per row: an MFMA output element is one
//               k-ordered fmaf chain of its own row) on the listed rows only.  Per entry it leaves the exact D and what
//               pass 2's forward would compute for the row (same arithmetic): pass-2 distance, arg-min link, ReLU masks --
//               k_tail_sel then picks the top-k by (D, obstacle) and runs only the backward.  It also records
//               max |Da - D| over all candidates (the run-time guard of eps: the host re-runs the propagate without
//               screening if the observed error ever exceeds the calibrated margin).
//
// k_screen design (MI355X-first).  fp16 MFMA is 16x the fp32 rate, so everything the fp32 kernel could hide -- LDS round
// trips of the activations, weight fragments from L2 -- would dominate.  Hence:
//   * TRANSPOSED product H'^T = W . H^T: the weights are the A operand, the activations the B operand (column = pair).
//     A wave owns 32 pairs and ALL 256 features of them, so a layer's output (C layout: lane = pair, registers =
//     features) IS the next layer's B operand after ReLU + cvt_pk -- the K order inside a dot product is free, the host
//     packs the weights in the permuted order the C layout produces.  Activations never leave registers: no LDS traffic,
//     no bank conflicts, no barrier for them.
//   * weights stream L2 -> LDS by LDS-DMA (buffer/global_load ... lds, 1 KiB = one A fragment per wave instruction) as
//     16 KB slices (32 output features x 256 k) through a 4-slot ring shared by the 8 waves of the workgroup (256 pairs):
//     128 KB per layer per 256 pairs instead of per 32, one s_barrier per slice, counted vmcnt, loads two slices ahead.
//   * layer 1 runs on the matrix pipe too: its 3(n+3) <= 32 inputs are two k-chunks, fetched as fp16 from a 64-byte row per
//     rollout and per obstacle (four 16-byte loads per lane and tile; reading the separable fp32 halves Fq[t] + Fp[o]
//     like k_pass1 does cost 36 % of the kernel, their fp16 copies still 25 %), W1 is one more slice of the ring.
//   * persistent workgroups (one per CU) loop over their tiles: the ring never drains, no refill gap between tiles.
//   * ReLU networks: a k-chunk (16 hidden units) whose activations are zero for all 32 pairs of the wave adds nothing to any
//     output, so its MFMAs are not issued (a ballot per tested chunk and layer, a scalar branch per MFMA of chunks 8-15).  The
//     host orders the units of this pack by how often they fire (screening.hip: screen_reorder), which puts the units a trained
//     network never uses -- 300 of the shipped one's 1024 -- into whole chunks: a quarter of the MFMAs go (EXPERIMENTS.md C 4.1d).
#include "pass1_tile.h"   // OmdsDivisor
#include "screen_select.h"

static_assert(SC_WIDTH == OMDS_WIDTH, "screen_plan_def.h sizes the bias table");
static_assert(SC_PW == 2 && SC_PW * SC_WAVES == 16, "a slice is 16 fragments: two LDS-DMA pieces per wave (issue)");
static_assert(SC_DIST >= 2 && SC_DIST <= SC_RING - 1 && (SC_RING & (SC_RING - 1)) == 0, "the slice DIST steps ahead overwrites a slot last read RING - DIST >= 1 steps ago");

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

// first k-chunk whose activations are tested for "all zero" before its MFMAs (ReLU networks).  Measured on the shipped network
// (variant builds, EXPERIMENTS.md; 1024 x 32 / 4096 x 32): 4: 100.0 / 365.5 us, 8: 98.0 / 357.7, 9: 96.7 / 351.2, 10: 96.1 / 349.5,
// 11: 97.0 / 351.7, 12: 97.2 / 355.3 -- its silent units begin at chunk 9-13 depending on the layer; every test and branch in front of
// them costs issue slots
constexpr int SC_TEST0 = 10;

struct ScreenArgs {
    const _Float16* Wh;      // [nhh*8 + 2 slices][16 fragments][64 lane][8 halfs], fragment order (packed by omds_set_mlp)
    const float* bias;       // [nhh + 2][256]: layer 1, hidden->hidden, the last layer's (padded with zeros)
    const _Float16* FqH;     // [4 pieces][ldFq rows][8]: fp16 network inputs of the rollouts (q, sin q, cos q at their feature slots)
    const _Float16* FpH;     // [4][ldFp][8]: obstacle points likewise (omds_screen_fidx)
    const _Float16* FqS;     // skip-connection networks: the same inputs at the slots of the CONCATENATED columns (omds_screen_sidx)
    const _Float16* FpS;
    int ldFq, ldFp;          // row capacities of the tables
    const float* radius;
    float* Dmin;
    long long total_rows;
    int unit, units_base, units_rem;   // the chunk rule's integers (screen_chunk, screen_plan_def.h)
    int B, O;
    uint32_t ignored;
    uint32_t skip_mask;      // bit L: the encoded input is concatenated behind level L (MlpDev::skip_mask)
    OmdsDivisor odiv;
    int nhh, C;
    float out_div;
    int res_tiles;           // tiles per workgroup (capacity of the result buffer in LDS)
    const SelectSink* sel;   // device memory, or nullptr.  Non-null: the flush phase selects each rollout's candidates instead of writing
                             // Dmin.  A pointer on purpose: as kernel arguments the sink's 20 dwords were loaded at entry and held in
                             // SGPRs across the tile loop (SGPR spills 36 -> 114)
};

// LDS-DMA: 16 bytes per lane from gsrc (per-lane address) to LDS [lds_dst + 16 * lane] (lds_dst wave-uniform).  Invisible
// to hipcc's s_waitcnt bookkeeping by design: completion is waited for with counted vmcnt below.
// The source is a wave-uniform base (SGPR pair) + a per-lane 32-bit byte offset + an immediate: per-lane 64-bit
// pointers would be loop-invariant VGPR pairs, one per slice, that hipcc hoists out of the tile loop and spills.
template <int IMM>
__device__ __forceinline__ void dma16(const void* gbase_uniform, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:%4\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(gbase_uniform), "s"(lds_dst), "n"(IMM)
                 : "memory");
}
// counted wait for this wave's LDS-DMA pieces + workgroup barrier; the "memory" clobber keeps hipcc from moving LDS reads
// of the slice above the barrier
template <int N>
__device__ __forceinline__ void wait_vm_barrier_n() { asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory"); }

// two fp32 pre-activations -> two fp16 activations (the next layer's B operand).  ReLU: convert, then one packed max.
// tanh: 1 - 2 / (1 + exp(2x)) in fp32 (v_exp_f32 / v_rcp_f32: +inf and 0 give the saturated values, tanh(0) = 0 exactly), then
// convert -- 7 VALU instructions per pair against 2 (EXPERIMENTS.md C 4.1b has what that costs beside the MFMAs)
template <int ACT>
__device__ __forceinline__ h2 act_pk(float a, float b) {
    if constexpr (ACT == OMDS_ACT_RELU) {
        h2 p = {(_Float16)a, (_Float16)b};                 // v_cvt_pk_f16_f32 (round to nearest even)
        const h2 z = {(_Float16)0, (_Float16)0};
        return __builtin_elementwise_max(p, z);            // v_pk_max_f16
    } else {
        // a, b arrive as 2 log2(e) x: the host scales the fp16 weights and the biases of every tanh layer by that factor
        // (build_mlp_packs, OMDS_SCREEN_TANH_SCALE), so tanh x = 1 - 2 / (1 + exp2(a)) needs no multiply here.  The add and the final
        // multiply-add are packed fp32 instructions (v_pk_add_f32 / v_pk_fma_f32: one per pair), only exp and rcp run per element:
        // 7 VALU instructions per pair (round 3: 11 -- scalar mul / add / fma; k_screen<2, tanh> 402 -> 382 us with the packed forms)
        typedef float f2 __attribute__((ext_vector_type(2)));
        const f2 e1 = f2{__builtin_amdgcn_exp2f(a), __builtin_amdgcn_exp2f(b)} + 1.f;
        const f2 r = f2{__builtin_amdgcn_rcpf(e1[0]), __builtin_amdgcn_rcpf(e1[1])};
        const f2 t = __builtin_elementwise_fma(f2{-2.f, -2.f}, r, f2{1.f, 1.f});
        return h2{(_Float16)t[0], (_Float16)t[1]};
    }
}

// A fragments of one group (4 k-chunks) of a slice
struct AGroup { h8 f[4]; };
__device__ __forceinline__ AGroup read_group(const unsigned char* slot_lane, int g) {
    AGroup r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.f[i] = *reinterpret_cast<const h8*>(slot_lane + (4 * g + i) * 1024);
    return r;
}

// pair (rollout t, obstacle o) of this lane in tile `tile` of the workgroup's chunk [p0, p1); rows past the end (also: the
// prefetch of a non-existent next tile) clamp to the chunk's last pair and are not stored.  Plain scalars on purpose: a
// struct carried around the tile loop went through scratch memory
__device__ __forceinline__ void tile_row(const ScreenArgs& a, long long p0, long long p1, int tile, int wave, int b, unsigned& t, unsigned& o) {
    long long row = p0 + (long long)tile * SC_ROWS + wave * 32 + b;
    if (row >= p1) row = p1 - 1;
    t = a.odiv.div((unsigned)row);
    o = (unsigned)row - t * (unsigned)a.O;
}

typedef unsigned u4 __attribute__((ext_vector_type(4)));

template <int NHH, int ACT, bool SKIP>
__global__ __launch_bounds__(SC_NT, 2) void k_screen(ScreenArgs a) {
    // PERSISTENT: workgroup w multiplies the tiles of its own contiguous chunk of the pair space (one workgroup per CU).
    // The weight slices keep streaming through the ring across tile boundaries (the slice sequence is periodic), the bias
    // table is loaded once, and the results wait in LDS until the end -- a store in flight would perturb the counted vmcnt
    // waits of the LDS-DMA pieces (stores and loads retire out of order with respect to each other).  Measured on the
    // one-tile-per-workgroup form (its phase timeline, EXPERIMENTS.md): of 57 kcycles per tile slot 14 were the refill gap between two
    // workgroups of a CU, 12 the layer-1 operand loads and first-slice latency, and only 29 the slice loop.
    // A chunk of WHOLE rollouts (a.sel.rowlist != nullptr) ends with every screening value of those rollouts in this
    // workgroup's LDS: the flush phase then does k_select's work from there -- k-th smallest, window, list append, audit
    // sample -- and the N x O matrix is never written or re-read (one launch and 2 x 1.2 MB less per horizon step).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // the small tables first: their ds_read offsets then fit the 16-bit immediate from ONE base register (behind the 64 KB
    // ring hipcc kept a base VGPR per 256-byte window alive across the tile loop, and spilled them)
    float* biasL = reinterpret_cast<float*>(smem_raw);                         // [NHH+2][256]: layer 1, hidden->hidden, last
    float* resL = biasL + (NHH + 2) * OMDS_WIDTH;                              // [a.res_tiles][SC_ROWS]
    unsigned char* ring = reinterpret_cast<unsigned char*>(resL + a.res_tiles * SC_ROWS);   // [SC_RING][SC_SLICE]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = lane & 31, half = lane >> 5;
    constexpr int S = NHH * 8 + 2;                 // slice steps of a tile: layer 1, 8 per hidden->hidden layer, the last layer
    const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)ring;
    const ScreenChunk chunk = screen_chunk(a.unit, a.units_base, a.units_rem, a.total_rows, (int)blockIdx.x);   // this workgroup's pairs [p0, p1)
    const long long p0 = chunk.p0, p1 = chunk.p1;
    const int my_pairs = chunk.pairs(), my_tiles = chunk.tiles();

    // slice `sl` of the network -> ring slot `slot`; this wave moves fragments PW*w .. PW*w + PW-1
    const unsigned char* wbase = reinterpret_cast<const unsigned char*>(a.Wh) + (SC_PW * wave) * 1024;   // wave-uniform
    const unsigned lane16 = lane * 16;
    auto issue = [&](int sl, int slot) {
        const unsigned char* src = wbase + (size_t)sl * SC_SLICE;
        const unsigned dst = ring_lds + (unsigned)(slot * SC_SLICE + (SC_PW * wave) * 1024);
        // the instruction offset advances the global AND the LDS address
        dma16<0>(src, lane16, dst);
        dma16<1024>(src, lane16, dst);
    };
    for (int i = tid; i < (NHH + 2) * OMDS_WIDTH; i += SC_NT) biasL[i] = a.bias[i];
    for (int i = tid; i < my_tiles * SC_ROWS; i += SC_NT) resL[i] = __builtin_inff();   // the two lane-halves of a pair min into it
    __syncthreads();   // bias table visible; nothing of the ring is in flight yet (hipcc's fence would drain it)
#pragma unroll
    for (int s0 = 0; s0 < SC_DIST; ++s0) issue(s0 % S, s0 % SC_RING);

    // network inputs of a pair as fp16 B operands: chunk cc, lane-half h, slot j <-> feature 16 cc + 8 h + j of
    // [x, sin x, cos x] (x = q then the obstacle point).  The rollout table holds the q features (zeros elsewhere), the
    // obstacle table the point features: two 16-byte loads per chunk and a bitwise OR
    // (buffer loads: SGPR descriptor + 32-bit lane offset + scalar piece offset -- no 64-bit per-lane pointers to keep alive)
    const __amdgpu_buffer_rsrc_t fq_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(a.FqH), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t fp_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(a.FpH), 0, 0x7fffffff, 0x00020000);
    auto load_inputs = [&](unsigned rt, unsigned ro, u4 (&raw)[4]) {
        unsigned hh = (unsigned)half;
        asm volatile("" : "+v"(hh));   // opaque: keeps hipcc from hoisting half * ld out of the tile loop into VGPRs it then spills
        const int vq = (int)((hh * (unsigned)a.ldFq + rt) * 16u), vp = (int)((hh * (unsigned)a.ldFp + ro) * 16u);
        raw[0] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(fq_rs, vq, 0, 0));
        raw[1] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(fp_rs, vp, 0, 0));
        raw[2] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(fq_rs, vq, a.ldFq * 32, 0));
        raw[3] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(fp_rs, vp, a.ldFp * 32, 0));
    };
    // skip-connection networks: the same encoded input at the slots of the concatenated columns.  The host packs the
    // layer behind a concatenation with those columns LAST (virtual columns 256 - 3d .. 255 = k-chunks 14 and 15, whatever
    // the width of the layer in front: the K order of a dot product is free), so the concatenation is a bitwise OR into
    // act[14], act[15] -- zeros there, the padded units of the narrower layer -- and one table serves every level
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t sq_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(SKIP ? a.FqS : a.FqH), 0, 0x7fffffff, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t sp_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(SKIP ? a.FpS : a.FpH), 0, 0x7fffffff, 0x00020000);
    auto load_skip = [&](unsigned rt, unsigned ro, u4 (&sk)[2]) {
        unsigned hh = (unsigned)half;
        asm volatile("" : "+v"(hh));
        const int vq = (int)((hh * (unsigned)a.ldFq + rt) * 16u), vp = (int)((hh * (unsigned)a.ldFp + ro) * 16u);
        sk[0] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(sq_rs, vq, 0, 0)) |
                __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(sp_rs, vp, 0, 0));
        sk[1] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(sq_rs, vq, a.ldFq * 32, 0)) |
                __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(sp_rs, vp, a.ldFp * 32, 0));
    };
    unsigned row_o;
    u4 raw[4];
    [[maybe_unused]] u4 skn[2];   // SKIP: the next tile's concatenation operands, fetched with its inputs
    float rad;
    {
        unsigned rt;
        tile_row(a, p0, p1, 0, wave, b, rt, row_o);
        load_inputs(rt, row_o, raw);
        if constexpr (SKIP) load_skip(rt, row_o, skn);
        rad = a.radius[row_o];
    }

    const unsigned char* ring_lane = ring + lane * 16;
    // accumulators start at the bias.  C layout: register r = 4j + i <-> output row 32 fb + 8 j + 4 half + i
    auto read_bias = [&](int layer, int fb) {
        f32x16 r;
        const float* bl = biasL + layer * OMDS_WIDTH + 32 * fb + 4 * half;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 bv = *reinterpret_cast<const float4*>(bl + 8 * j);
            r[4 * j] = bv.x; r[4 * j + 1] = bv.y; r[4 * j + 2] = bv.z; r[4 * j + 3] = bv.w;
        }
        return r;
    };
    auto to_act = [&](const f32x16& acc, h8& lo, h8& hi) {   // registers 0-7 are the slots of chunk 2 fb of the next layer, 8-15 of 2 fb + 1
        const h2 q0 = act_pk<ACT>(acc[0], acc[1]), q1 = act_pk<ACT>(acc[2], acc[3]), q2 = act_pk<ACT>(acc[4], acc[5]), q3 = act_pk<ACT>(acc[6], acc[7]);
        const h2 q4 = act_pk<ACT>(acc[8], acc[9]), q5 = act_pk<ACT>(acc[10], acc[11]), q6 = act_pk<ACT>(acc[12], acc[13]), q7 = act_pk<ACT>(acc[14], acc[15]);
        lo = h8{q0[0], q0[1], q1[0], q1[1], q2[0], q2[1], q3[0], q3[1]};
        hi = h8{q4[0], q4[1], q5[0], q5[1], q6[0], q6[1], q7[0], q7[1]};
    };

    // ---- the slice pipeline.  Global step sigma = it * S + s multiplies slice s (ring slot sigma % RING) in 4 groups of 4
    //      fragments; the A fragments of the next group are read while the current group's MFMAs issue.  In the middle of a
    //      step the wave waits for ITS pieces of the next slice (issued DIST-1 steps earlier) and meets the others at the
    //      barrier: after it that slice is complete and every wave has finished reading the previous one, so the slice DIST
    //      steps ahead may overwrite a slot last read RING - DIST >= 1 steps ago.  Slices keep being issued past the last
    //      tile (into free slots, never read), so the counted wait is one constant.
    wait_vm_barrier_n<SC_PW * (SC_DIST - 1)>();   // slice 0 landed (the later ones may still be in flight)
    AGroup cur = read_group(ring_lane, 0);
    int sigma0 = 0;
    for (int it = 0; it < my_tiles; ++it, sigma0 += S) {
        auto sync_and_issue = [&](int s) {
            wait_vm_barrier_n<SC_PW * (SC_DIST - 2)>();
            issue((s + SC_DIST) % S, (sigma0 + s + SC_DIST) & (SC_RING - 1));
        };
        auto slot_ptr = [&](int s) { return ring_lane + ((sigma0 + s) & (SC_RING - 1)) * SC_SLICE; };
        if (it * SC_ROWS + wave * 32 >= my_pairs) {
            // all pairs of this wave lie past the end of the chunk (the partial last tile of a chunk of whole rollouts): it keeps
            // the ring moving -- its DMA pieces, the barriers -- and issues no MFMA.  The matrix pipe is power-limited under this
            // kernel: multiplying clamped duplicates would slow the waves that have real pairs (measured: 99 -> 108 us at N = 1024)
            for (int s = 0; s < S; ++s) sync_and_issue(s);
            continue;
        }
        h8 in[2];
        [[maybe_unused]] h8 sk[2];
        {
            const u4 i0 = raw[0] | raw[1], i1 = raw[2] | raw[3];
            in[0] = __builtin_bit_cast(h8, i0);
            in[1] = __builtin_bit_cast(h8, i1);
            if constexpr (SKIP) { sk[0] = __builtin_bit_cast(h8, skn[0]); sk[1] = __builtin_bit_cast(h8, skn[1]); }
        }
        h8 act[16];
        // ReLU networks: bit cc = some pair of this wave has a non-zero activation in k-chunk cc of the layer about to be consumed.
        // A chunk whose 16 units are zero for all 32 pairs contributes exactly nothing to any output: its MFMAs are not issued.
        // (The host orders the hidden units of the screening pack by how often they fire, so that the units a trained network
        //  never uses -- a third of the shipped one's -- fill whole chunks: omds_internal.h, screen reorder.)
        unsigned alive = 0xffffu;
        auto find_alive = [&]() {
            if constexpr (ACT == OMDS_ACT_RELU && !SKIP) {
                unsigned mk = (1u << SC_TEST0) - 1u;   // the first chunks hold the units that fire most: multiplied without a test
#pragma unroll
                for (int cc = SC_TEST0; cc < 16; ++cc) {
                    const u4 v = __builtin_bit_cast(u4, act[cc]);
                    const unsigned nz = v.x | v.y | v.z | v.w;
                    mk |= (__builtin_amdgcn_ballot_w64(nz != 0u) != 0ull ? 1u : 0u) << cc;
                }
                alive = mk;
            }
        };
        auto concat = [&](int level) {   // wave-uniform test; the OR touches 8 registers
            if constexpr (SKIP) {
                if ((a.skip_mask >> level) & 1u) {
                    act[14] = __builtin_bit_cast(h8, __builtin_bit_cast(u4, act[14]) | __builtin_bit_cast(u4, sk[0]));
                    act[15] = __builtin_bit_cast(h8, __builtin_bit_cast(u4, act[15]) | __builtin_bit_cast(u4, sk[1]));
                }
            }
        };
        // ---- step 0: layer 1 on the matrix pipe.  Slice 0 = W1 as 8 row blocks x 2 k-chunks (fragment 2 fb + cc)
        {
            const unsigned char* sl = slot_ptr(0);
            const unsigned char* sl_next = slot_ptr(1);
            // group g = row blocks 2g, 2g+1 (two MFMAs each); their activation + conversion runs one group later,
            // under the next group's MFMAs; the scheduling barriers keep hipcc from batching all MFMAs first
            f32x16 pa, pb;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g == 1) sync_and_issue(0);
                const AGroup pre = (g < 3) ? read_group(sl, g + 1) : read_group(sl_next, 0);
                const f32x16 ba = read_bias(0, 2 * g), bb = read_bias(0, 2 * g + 1);
                f32x16 ca = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.f[0], in[0], ba, 0, 0, 0);
                f32x16 cb = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.f[2], in[0], bb, 0, 0, 0);
                ca = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.f[1], in[1], ca, 0, 0, 0);
                cb = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.f[3], in[1], cb, 0, 0, 0);
                if (g > 0) {
                    to_act(pa, act[4 * g - 4], act[4 * g - 3]);
                    to_act(pb, act[4 * g - 2], act[4 * g - 1]);
                }
                __builtin_amdgcn_sched_barrier(0);
                pa = ca; pb = cb;
                cur = pre;
            }
            to_act(pa, act[12], act[13]);
            to_act(pb, act[14], act[15]);
            concat(0);
            find_alive();
        }
        // ---- steps 1 .. S-1: hidden->hidden layers and the last layer
        h8 nxt[16];
        float dmin = __builtin_inff();
        f32x16 acc = read_bias(1, 0);
        unsigned nrow_o = row_o;
#pragma unroll
        for (int s = 1; s < S; ++s) {
            const int fb = (s - 1) & 7;                        // output row block of hidden->hidden layer (s - 1) >> 3 (bias row + 1)
            const bool last = s == S - 1;
            const unsigned char* sl = slot_ptr(s);
            const unsigned char* sl_next = slot_ptr(s + 1);
            f32x16 acc_next = acc;                             // the next step's start values (the bias)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g == 1) sync_and_issue(s);
                const AGroup pre = (g < 3) ? read_group(sl, g + 1) : read_group(sl_next, 0);   // (reading only the fragments that will be multiplied: 96 -> 103 us)
                if (g == 2 && !last) acc_next = (s + 1 == S - 1) ? read_bias(NHH + 1, 0) : read_bias(((s) >> 3) + 1, s & 7);
                if (s == S - 2 && g == 2) {   // the next tile's inputs, fetched under the last two steps of this one
                    unsigned nt;
                    tile_row(a, p0, p1, it + 1, wave, b, nt, nrow_o);
                    load_inputs(nt, nrow_o, raw);
                    if constexpr (SKIP) load_skip(nt, nrow_o, skn);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (4 * g + i < SC_TEST0 || ((alive >> (4 * g + i)) & 1u))
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.f[i], act[4 * g + i], acc, 0, 0, 0);
                }
                // issue order inside the group: one fragment read of the NEXT group ahead of each fragment's MFMAs (the
                // group's MFMAs = 128+ cycles of lead for the LDS latency; group 2 also carries the four bias reads of the
                // next step); everything else (the previous step's epilogue VALU) fills in behind
                if (g == 2 && !last) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    }
                }
                cur = pre;
            }
            if (!last) {
                to_act(acc, nxt[2 * fb], nxt[2 * fb + 1]);
                if (fb == 7) {
#pragma unroll
                    for (int cc = 0; cc < 16; ++cc) act[cc] = nxt[cc];
                    concat(((s - 1) >> 3) + 1);
                    find_alive();
                }
            } else {
                // last layer: the links sit on the A rows (rows >= C are zero); min over the valid, un-ignored links
#pragma unroll
                for (int r = 0; r < 8; ++r) {   // link = 4 half + (r & 3) + 8 (r >> 2); links >= 16 do not exist (OMDS_CPAD)
                    const int link = 4 * half + (r & 3) + 8 * (r >> 2);
                    float v = acc[r] / a.out_div - rad;
                    v = (link >= a.C) ? __builtin_inff() : (((a.ignored >> link) & 1u) ? 1e6f : v);
                    dmin = fminf(dmin, v);
                }
            }
            acc = acc_next;
        }
        // links 0-3, 8-11 sit in lane-half 0, the others in half 1: both min into the pair's LDS slot (ds_min_f32; a cross-lane
        // exchange would keep a lane-index VGPR alive across the whole tile loop)
        __hip_atomic_fetch_min(&resL[it * SC_ROWS + wave * 32 + b], dmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        row_o = nrow_o;
        rad = a.radius[row_o];
    }
    // ---- drain the ring (pieces issued past the last tile still target this workgroup's LDS), then flush the results
    wait_vm_barrier_n<0>();
    __syncthreads();
    if (a.sel) {
        // the chunk is whole rollouts: resL[rl * O .. +O) are the screening values of rollout t0 + rl
        SelectShared& sh = *reinterpret_cast<SelectShared*>(ring);   // the ring is drained and idle
        const SelectSink sel = *a.sel;
        const int O = a.O;
        const int t0 = (int)a.odiv.div((unsigned)p0);
        const int n_roll = my_pairs / O;
        for (int r0 = 0; r0 < n_roll; r0 += SEL_WAVES) {
            const int rl = r0 + wave;
            const bool live = rl < n_roll;
            const int rr = live ? rl : n_roll - 1;
            select_rollout(sel, sh, (const __attribute__((address_space(3))) float*)resL + rr * O, t0 + rr, live, O, lane, wave);
        }
    } else {
        for (int i = tid; i < my_pairs; i += SC_NT) a.Dmin[p0 + i] = resL[i];
    }
}

// k_select: one wave per rollout (select_rollout above), for the steps whose k_screen writes the matrix: rows too long for a
// workgroup's LDS, and the matrix route of a tanh network whose derivative hand-over buffer could not be allocated (k_exact, TileMode::ListPatch
// writes the exact values into the matrix).
struct SelectArgs {
    const float* Dmin;    // [N][O] screening values
    int N, O;
    SelectSink sel;
};
__global__ __launch_bounds__(SEL_WAVES * 64) void k_select(SelectArgs a) {
    __shared__ SelectShared sh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t_raw = blockIdx.x * SEL_WAVES + wave;
    const bool live = t_raw < a.N;                       // waves past the last rollout take part in the barriers with 0 entries
    const int t = live ? t_raw : a.N - 1;
    select_rollout(a.sel, sh, a.Dmin + (size_t)t * a.O, t, live, a.O, lane, wave);
}

template <int NHH, int ACT, bool SKIP>
static void launch_screen_t(hipStream_t s, dim3 grid, size_t lds, size_t lds_max, const ScreenArgs& a) {
    static std::atomic<uint64_t> configured{0};
    if (omds_first_use_on_device(configured))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_screen<NHH, ACT, SKIP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    hipLaunchKernelGGL((k_screen<NHH, ACT, SKIP>), grid, dim3(SC_NT), lds, s, a);
}
template <int NHH>
static void launch_screen_n(hipStream_t s, dim3 grid, size_t lds, size_t lds_max, const ScreenArgs& a, int act, bool skip) {
    if (act == OMDS_ACT_RELU) { if (skip) launch_screen_t<NHH, OMDS_ACT_RELU, true>(s, grid, lds, lds_max, a); else launch_screen_t<NHH, OMDS_ACT_RELU, false>(s, grid, lds, lds_max, a); }
    else { if (skip) launch_screen_t<NHH, OMDS_ACT_TANH, true>(s, grid, lds, lds_max, a); else launch_screen_t<NHH, OMDS_ACT_TANH, false>(s, grid, lds, lds_max, a); }
}

void omds_launch_screen(hipStream_t s, const ScreenDev& sd, const MlpDev& m, const uint16_t* FqH, int ldFq, const uint16_t* FpH,
                        int ldFp, const float* radius, int O, int B, uint32_t ignored, float* Dmin, const SelectSink* sel) {
    // sel: DEVICE pointer to this step's sink (screening.hip uploads the sinks of all horizon steps before the loop)
    const long long total = (long long)B * O;
    if (total <= 0) return;
    ScreenArgs a;
    a.Wh = reinterpret_cast<const _Float16*>(sd.Wh);
    a.bias = sd.bias;
    a.FqH = reinterpret_cast<const _Float16*>(FqH); a.FpH = reinterpret_cast<const _Float16*>(FpH);
    a.FqS = reinterpret_cast<const _Float16*>(m.scrQ); a.FpS = reinterpret_cast<const _Float16*>(m.scrP);
    a.ldFq = ldFq; a.ldFp = ldFp;
    a.radius = radius; a.Dmin = Dmin; a.B = B;
    a.total_rows = total; a.O = O; a.ignored = ignored; a.odiv = OmdsDivisor::make((unsigned)O);
    a.nhh = m.nhh; a.C = m.C; a.out_div = m.out_div;
    a.skip_mask = m.skip_mask;
    // who owns which pairs, how many workgroups and result tiles, how much LDS: screen_plan_def.h
    const ScreenLaunchPlan p = screen_plan(B, O, m.nhh, omds_cu_count(), sel != nullptr);
    a.unit = p.unit; a.units_base = p.units_base; a.units_rem = p.units_rem;
    a.res_tiles = p.res_tiles;
    a.sel = p.selects ? sel : nullptr;
    if (p.selects) a.Dmin = nullptr;
    const dim3 grid((unsigned)p.grid);
    const size_t lds = p.lds_bytes, lds_max = p.lds_max_bytes;
    const bool skip = m.skip_mask != 0;
    switch (m.nhh) {
        case 1: launch_screen_n<1>(s, grid, lds, lds_max, a, m.act, skip); break;
        case 2: launch_screen_n<2>(s, grid, lds, lds_max, a, m.act, skip); break;
        case 3: launch_screen_n<3>(s, grid, lds, lds_max, a, m.act, skip); break;
        case 4: launch_screen_n<4>(s, grid, lds, lds_max, a, m.act, skip); break;
        default: break;   // omds_screen_supported() keeps other depths on the fp32 path
    }
}

bool omds_screen_supported(const MlpDev& m) { return (m.act == OMDS_ACT_RELU || m.act == OMDS_ACT_TANH) && m.nhh >= 1 && m.nhh <= 4; }

void omds_launch_select(hipStream_t s, const float* Dmin, int B, int O, const SelectSink& sel) {
    if (B <= 0) return;
    SelectArgs a;
    a.Dmin = Dmin; a.N = B; a.O = O; a.sel = sel;
    hipLaunchKernelGGL(k_select, dim3((B + SEL_WAVES - 1) / SEL_WAVES), dim3(SEL_WAVES * 64), 0, s, a);
}
