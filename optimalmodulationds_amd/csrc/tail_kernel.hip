// Fused per-step "tail" kernel for gfx950: everything of one horizon step that is local to a rollout
// once the pass-1 min-distance matrix exists -- top-k over the obstacles (MPPI.py:245-247), forward +
// analytic backward on the k closest rows (robot_sdf.py:153-158), softmax blend, modulation / policy /
// Euler step (MPPI.py:102-223) and the encoded joint inputs [q, sin q, cos q] of the NEXT step.  A workgroup owns
// floor(ROWS/k) rollouts (<= ROWS network rows), so a horizon step is two launches: k_pass1 + k_tail.  ROWS = 32
// (v_mfma_f32_32x32x2) for large batches; ROWS = 16 (v_mfma_f32_16x16x4) when the batch has too few rows to fill the
// CUs with 32-row tiles anyway: the workgroup's chain of dependent GEMMs IS the step latency then, and it halves.
// The stand-alone kernels (k_topk, k_pass2, k_modulate, k_rollout_layer1) remain for the batch entry
// points (omds_dist_grad, omds_mlp_forward_vjp) and for n_dof / k combinations not instantiated here.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "pass2_device.h"
#include "timeline_device.h"
#include "topk_device.h"
#include "trig_device.h"
#include "step_epilogue.h"
#include "tail_plan_def.h"

static_assert(TAIL_MT == P2_MT && TAIL_NT == P2_NT && TAIL_LDH == LDH, "tail_plan_def.h restates pass 2's tile");

struct TailArgs {
    MlpDev m;
    const float* Fp;
    const float* radius;
    const float* xyzr;
    const float* Dmin;   // [N][O]
    int ldD;             // row stride of Dmin: O, or 0 when every rollout reads ONE row (the shared first step of a propagate)
    float* Fq;         // [N][OMDS_FROW] encoded joint inputs, in: this step, out: next step (rows of the workgroup's own rollouts)
    float* FqOut;      // where the next step's rows go: Fq itself, or the next slab when all steps' halves are kept
    _Float16* FqH;       // next step's states as fp16 network inputs for the screening kernel (nullptr: not screening)
    int ldF;             // row capacity of FqH
    float* dscr;         // tanh derivative scratch
    int O;
    int n_slots;         // workgroups of the launch (tanh scratch stride between layers)
    // screened step (k_tail_sel): the candidate list of k_select and what k_exact computed for its entries
    const int* rowlist;  // [entries] pair t*O + o
    const int* range;    // [N][4] start, length of each rollout's entries, tau of k_select (float bits)
    float e_bound;       // assumed bound on the screening error of the rows that were NOT re-evaluated
    unsigned* viol;      // count of rollouts whose slack tau - (exact k-th smallest) fell below e_bound
    ExactOut ex;
    StepArgs st;
};
// ... of the launch of one half of a two-part propagate: the rollouts [t0, t_end) of the batch
struct TailPartArgs : TailArgs {
    int t0, t_end;
};
template <bool PART> using TailArgsOf = std::conditional_t<PART, TailPartArgs, TailArgs>;

// The two tails' pointers into their dynamic LDS block.  Where the blocks lie and how large the launch is, is TailLdsPlan
// (tail_plan_def.h); every pointer is formed from the block's start and its offset there (k_tail does not read sel).
struct TailLds {
    P2Smem sm;
    float *gx, *dr, *feat;
    int* sel;
    __device__ __forceinline__ TailLds(float* smem, int nhid) {
        const TailLdsPlan o(nhid, true);
        sm.Hs = smem + o.Hs;
        sm.gf = smem + o.gf;
        sm.maskL = reinterpret_cast<uint16_t*>(smem + o.maskL);
        sm.rowT = reinterpret_cast<int*>(smem + o.rowT);
        sm.rowO = reinterpret_cast<int*>(smem + o.rowO);
        sm.rowMin = reinterpret_cast<int*>(smem + o.rowMin);
        gx = smem + o.gx;
        dr = smem + o.dr;
        feat = smem + o.feat;
        sel = reinterpret_cast<int*>(smem + o.sel);
    }
};

// FRAME: the modulation runs in the moving obstacle's frame (step_device.h); its own instantiation, so that the kernel of every
// other propagate is the code it was.  PART, likewise: the launch of one half of a two-part propagate (enqueue_dense), which owns the
// rollouts [a.t0, a.t_end) -- workgroup b starts at a.t0 + b RW and stops at a.t_end -- while N stays the row stride of every table.
// ReLU networks only: the tanh scratch is laid out by workgroup, and two launches at once would share it.
template <int ND, int ACT, int ROWS, bool FRAME = false, bool PART = false>
__global__ __launch_bounds__(P2_NT) void k_tail(TailArgsOf<PART> a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDev& m = a.m;
    TailLds L(smem, m.nhh + 1);
    P2Smem& sm = L.sm;
    float *const gx = L.gx, *const dr = L.dr, *const feat = L.feat;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.st.N, k = a.st.k, O = a.O;
    // ROWS = 4: forward and backward on 4-row groups (pass2_body_g4): 4 G4_NG = 20 network rows per workgroup
    static_assert(ACT == OMDS_ACT_RELU || ROWS != 4, "the 4-row-group pass 2 works on ReLU masks");
    static_assert(ACT == OMDS_ACT_RELU || !PART, "the tanh scratch is one launch's");
    constexpr int G4_NG = 5, TROWS = ROWS == 4 ? 4 * G4_NG : ROWS;
    const int RW = TROWS / k;                 // rollouts per workgroup
    int t_base = blockIdx.x * RW, T1 = N;     // the launch's rollouts start at workgroup 0's t_base and end in front of T1
    if constexpr (PART) { t_base += a.t0; T1 = a.t_end; }

    OMDS_TL_STAMP(0);
    OMDS_TL_STAMP(1);
    P2G4Pre pre;   // (ROWS = 4) everything of pass 2 that does not wait for the top-k is requested in front of it
    if constexpr (ROWS == 4)
        pass2_g4_prefetch(m, a.Fq, [&](int r) { const int rl = r / k; return (rl < RW && t_base + rl < T1) ? t_base + rl : -1; }, pre);
    // ---- top-k of each rollout's min-distance row (ascending, ties by lower obstacle index) -------
    if (tid < P2_MT) { sm.rowT[tid] = -1; sm.rowO[tid] = 0; }
    __syncthreads();
    for (int rl = wave; rl < RW; rl += 8) {
        const int t = t_base + rl;
        if (t >= T1) break;
        topk_row(a.Dmin + (size_t)t * a.ldD, O, k, lane, [&](int j, int bi) {
            sm.rowT[rl * k + j] = t;
            sm.rowO[rl * k + j] = bi;
            // screened step of a tanh network: the matrix holds exact values on the candidates and screening values (all above
            // tau) elsewhere; the k smallest are exact ones, and no unevaluated row can belong among them, as long as the k-th
            // stays e_bound below tau (the slack guard)
            if (a.range && j == k - 1 && !(__builtin_bit_cast(float, a.range[4 * t + 2]) - a.Dmin[(size_t)t * a.ldD + bi] >= a.e_bound)) atomicAdd(a.viol, 1u);
        });
    }
    __syncthreads();
    OMDS_TL_STAMP(2);

    // ---- forward + backward on the selected rows; gradients and distances stay in LDS ------------
    const float* qT = a.st.trajT + (size_t)(a.st.step - 1) * ND * N;
    if constexpr (ROWS == 4)
        pass2_body_g4<G4_NG>(m, sm, pre, a.Fp, a.radius, a.xyzr, t_base * k, T1 * k, qT, N, gx, dr, 0);
    else
        pass2_body<ACT, ROWS>(m, sm, a.Fq, a.Fp, a.radius, a.xyzr, t_base * k, T1 * k, qT, N, gx, dr, 0, nullptr, nullptr,
                              a.dscr, (size_t)a.n_slots * ROWS * OMDS_WIDTH, (int)blockIdx.x * ROWS);
    __syncthreads();
    OMDS_TL_STAMP(9);

    // ---- modulation / policy / Euler step: 16 lanes per rollout; then the encoded joint inputs of the next step -------------
    step_advance<ND, FRAME>(a.st, m, qT, N, T1, t_base, RW, k, gx, dr, sm.rowO, feat, a.FqH, a.ldF);
    OMDS_TL_STAMP(10);
    if (a.st.step >= a.st.H) return;   // last step: nothing is integrated, no next network evaluation
    __syncthreads();
    step_write_next_rows<ND, P2_NT>(a.FqOut, feat, m.d, T1, t_base, RW);
    OMDS_TL_STAMP(11);
    OMDS_TL_STAMP(19);
}

// ------------------------------------------------------------------------------------------------
// Screened step: k_screen -> k_select -> k_exact -> k_tail_sel.  k_exact has evaluated every candidate row in fp32 with
// pass 1's arithmetic, which is also pass 2's forward (same start value, same k order), and left the pass-1 value D, the
// pass-2 distance, the arg-min link and the ReLU masks per list entry.  This tail therefore needs no forward at all: top-k
// by (D, obstacle index) over each rollout's few candidates, masks of the selected entries gathered into the MFMA C layout,
// the pass-2 backward, then blend / modulation / Euler step / next-step layer 1 exactly as in k_tail.
// tanh networks (ACT = OMDS_ACT_TANH, round 4): k_exact left 1 - h^2 of every hidden unit of every candidate instead of masks
// (ExactOut::deriv, 1 KB per entry and layer); the backward reads the selected entries' rows through sm.rowE -- the same
// numbers pass 2's own forward would have written to its scratch, so the tanh tail drops its forward too.
// ------------------------------------------------------------------------------------------------
template <int ND, int ROWS, int ACT = OMDS_ACT_RELU, bool FRAME = false>
__global__ __launch_bounds__(P2_NT) void k_tail_sel(TailArgs a) {
    static_assert(ACT == OMDS_ACT_RELU || ROWS != 4, "the 4-row-group backward works on ReLU masks");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDev& m = a.m;
    TailLds L(smem, m.nhh + 1);
    P2Smem& sm = L.sm;
    float *const gx = L.gx, *const dr = L.dr, *const feat = L.feat;
    int* const sel = L.sel;
    uint32_t* maskRow = reinterpret_cast<uint32_t*>(sm.Hs);     // [32][nhid][8] gathered masks; the tile buffer is idle until the seed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.st.N, k = a.st.k, O = a.O, nhid = m.nhh + 1;
    // ROWS = 4: the backward runs on 4-row groups (pass2_backward_hidden_g4): G4_ROWS network rows per workgroup
    constexpr int G4_NG = 5, TROWS = ROWS == 4 ? 4 * G4_NG : ROWS;
    const int RW = TROWS / k;                 // rollouts per workgroup
    const int t_base = blockIdx.x * RW;

    OMDS_TL_STAMP(0);
    OMDS_TL_STAMP(1);
    // ---- top-k of each rollout's candidates by (D, obstacle index): k rounds of "smallest after the previous one" ----
    if (tid < P2_MT) { sm.rowT[tid] = -1; sm.rowO[tid] = 0; sm.rowMin[tid] = 0; sel[tid] = -1; dr[tid] = 0.f; }
    __syncthreads();
    for (int rl = wave; rl < RW; rl += 8) {
        const int t = t_base + rl;
        if (t >= N) break;
        // rowlist == nullptr: EVERY pair of the rollout is an entry and the entry index is the pair index (pass1_tile, TileMode::EmitAll: the
        // all-fp32 step); no window, no slack to check
        const bool dense = a.rowlist == nullptr;
        const int base = dense ? t * O : a.range[4 * t], cnt = dense ? O : a.range[4 * t + 1];
        const float tau = dense ? __builtin_inff() : __builtin_bit_cast(float, a.range[4 * t + 2]);
        if (lane == 0 && cnt < k && a.viol) atomicAdd(a.viol, 1u);
        if (cnt <= 64) {
            // the usual case, a few candidates: one per lane, and its rank under (D, obstacle) by comparing with every other
            // candidate's (value, obstacle) broadcast from its lane -- cnt scalar steps instead of k wave-wide reductions
            const int e = base + lane;
            const bool have = lane < cnt && e < a.ex.cap;   // list longer than k_exact's outputs: the host redoes the propagate in fp32
            const float x = have ? a.ex.D[e] : __builtin_inff();
            const int o = have ? (dense ? e : a.rowlist[e]) - t * O : 0x7fffffff;
            int rank = 0;
            for (int j = 0; j < cnt; ++j) {
                const float xj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), j));
                const int oj = __builtin_amdgcn_readlane(o, j);
                rank += ((xj < x) || (xj == x && oj < o)) ? 1 : 0;
            }
            // slack guard: every row that was not listed has a screening value above tau; with an error of at most e_bound its
            // exact value exceeds tau - e_bound, so it stays out of the k smallest as long as tau - D*_k >= e_bound
            if (have && rank == k - 1 && a.viol && !(tau - x >= a.e_bound)) atomicAdd(a.viol, 1u);   // (dense mode: tau = inf, viol = NULL)
            if (have && rank < k) {
                const int r = rl * k + rank;
                sm.rowT[r] = t;
                sm.rowO[r] = o;
                sm.rowMin[r] = a.ex.amin[e];
                dr[r] = a.ex.dr[e];
                sel[r] = e;
            }
            continue;
        }
        float pv = -__builtin_inff();
        int po = -1;
        for (int j = 0; j < k; ++j) {
            float bv = __builtin_inff();
            int bo = 0x7fffffff, be = -1;
            for (int i = lane; i < cnt; i += 64) {
                const int e = base + i;
                if (e >= a.ex.cap) break;   // list longer than k_exact's outputs: the host sees the count and redoes the propagate in fp32
                const float x = a.ex.D[e];
                const int o = (dense ? e : a.rowlist[e]) - t * O;
                const bool after = (x > pv) || (x == pv && o > po);
                if (after && ((x < bv) || (x == bv && o < bo))) { bv = x; bo = o; be = e; }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oo = __shfl_xor(bo, off);
                const int oe = __shfl_xor(be, off);
                if ((ov < bv) || (ov == bv && oo < bo)) { bv = ov; bo = oo; be = oe; }
            }
            pv = bv;
            po = bo;
            if (lane == 0 && be >= 0) {
                const int r = rl * k + j;
                sm.rowT[r] = t;
                sm.rowO[r] = bo;
                sm.rowMin[r] = a.ex.amin[be];
                dr[r] = a.ex.dr[be];
                sel[r] = be;
            }
        }
        if (lane == 0 && a.viol && !(tau - pv >= a.e_bound)) atomicAdd(a.viol, 1u);   // pv = the exact k-th smallest
    }
    __syncthreads();
    OMDS_TL_STAMP(2);
    if constexpr (ACT == OMDS_ACT_TANH) {
        sm.rowE = sel;   // the backward gathers 1 - h^2 of row r from entry sel[r] of ExactOut::deriv (written by k_exact, TileMode::ListDeriv)
    } else {
    // ---- the selected entries' masks -> LDS -> 16 bits per thread and layer in the MFMA C layout (what pass 2's forward
    //      would have left in sm.maskL): thread (wave = 32-column block, lane) owns column wave*32 + (lane&31) of rows crow(r, lane)
    for (int i = tid; i < TROWS * nhid * 8; i += P2_NT) {
        const int r = i / (nhid * 8);
        maskRow[i] = sel[r] >= 0 ? a.ex.mask[(size_t)sel[r] * nhid * 8 + (i - r * nhid * 8)] : 0u;
    }
    __syncthreads();
    if constexpr (ROWS == 4) {
        // the 4-row-group backward wants, per hidden level and COLUMN, the mask bits of all rows in one word
        sm.maskG4 = reinterpret_cast<uint32_t*>(sm.maskL);   // (nhh + 1) * 256 words <= the (nhh + 1) * 512 halfwords of maskL
        for (int i = tid; i < nhid * 256; i += P2_NT) {
            const int l = i >> 8, col = i & 255;
            uint32_t bits = 0;
#pragma unroll
            for (int e = 0; e < 4 * G4_NG; ++e) {
                const uint32_t* mr = maskRow + ((size_t)e * nhid + l) * 8;
                bits |= ((mr[col >> 5] >> (col & 31)) & 1u) << e;
            }
            sm.maskG4[i] = bits;
        }
    } else {
        using G = P2Geo<ROWS>;
        for (int l = 0; l < nhid; ++l) {
            uint32_t bits = 0;
#pragma unroll
            for (int r = 0; r < G::NV; ++r) {
                const int col = G::col(r, wave, lane);
                const uint32_t* mr = maskRow + ((size_t)G::row(r, lane) * nhid + l) * 8;
                bits |= ((mr[col >> 5] >> (col & 31)) & 1u) << r;   // one ballot half per 32-column block and level
            }
            sm.maskL[l * P2_NT + tid] = (uint16_t)bits;
        }
    }
    __syncthreads();
    }

    OMDS_TL_STAMP(3);
    // ---- backward on the selected rows; gradients stay in LDS -----------------------------------------
    const float* qT = a.st.trajT + (size_t)(a.st.step - 1) * ND * N;
    if constexpr (ROWS == 4) {
        pass2_backward_hidden_g4<G4_NG>(m, sm);
        p2_backward_first<32>(m, sm, a.xyzr, t_base * k, N * k, qT, N, gx, 0);
    } else {
        pass2_backward<ACT, ROWS>(m, sm, a.xyzr, t_base * k, N * k, qT, N, gx, 0, a.ex.deriv, (size_t)a.ex.cap * OMDS_WIDTH, 0);
    }
    __syncthreads();
    OMDS_TL_STAMP(9);

    // ---- modulation / policy / Euler step: 16 lanes per rollout; then the encoded joint inputs of the next step -------------
    step_advance<ND, FRAME>(a.st, m, qT, N, N, t_base, RW, k, gx, dr, sm.rowO, feat, a.FqH, a.ldF);
    OMDS_TL_STAMP(10);
    if (a.st.step >= a.st.H) return;   // last step: nothing is integrated, no next network evaluation
    __syncthreads();
    step_write_next_rows<ND, P2_NT>(a.FqOut, feat, m.d, N, t_base, RW);
    OMDS_TL_STAMP(11);
    OMDS_TL_STAMP(19);
}

#ifdef OMDS_TAIL_TL
// one line per workgroup: XCC / CU of thread 0 are not recorded; columns = stamps 0..11 and 19 (0 and 19: s_memrealtime, 100 MHz)
__global__ void k_tail_tl_dump(int nb) {
    for (int b = 0; b < nb && b < 1024; ++b) {
        printf("TL %d", b);
        for (int i = 0; i < 19; ++i) printf(" %llu", g_tail_tl[b][i]);   // 12..16: inside modulate_core, 17..18: pass2_body_g4
        printf(" %llu\n", g_tail_tl[b][19]);
    }
}
// prints the stamps of the third launch at horizon step OMDS_TAIL_TL_STEP (tools/tail_timeline.py)
static void tail_tl_dump(hipStream_t s, int step, int grid) {
    static int seen = 0;
    static const char* want = getenv("OMDS_TAIL_TL_STEP");
    if (want && step == atoi(want) && ++seen == 3) hipLaunchKernelGGL(k_tail_tl_dump, dim3(1), dim3(1), 0, s, grid);
}
#else
static void tail_tl_dump(hipStream_t, int, int) {}
#endif

// ---- launchers: the tile height, the key and the LDS size are tail_plan_def.h's ----------------------------------------------------
// one launch of instantiation K on tiles of ROWS rows; SEL: k_tail_sel's LDS block
template <void (*K)(TailArgs), int ROWS, bool SEL>
static void launch_tail_k(hipStream_t s, const TailArgs& a) {
    static std::atomic<uint64_t> configured{0};
    if (omds_first_use_on_device(configured)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)TailLdsPlan::bytes(OMDS_MAX_HIDDEN + 1, SEL));
    }
    const int grid = tail_workgroups(a.st.N, ROWS, a.st.k);
    hipLaunchKernelGGL(K, dim3(grid), dim3(P2_NT), TailLdsPlan::bytes(a.m.nhh + 1, SEL), s, a);
    tail_tl_dump(s, a.st.step, grid);
}

// entry i launches the kernel of TAIL_KEYS[i]: the key's four constants are the template arguments
using TailLauncher = void (*)(hipStream_t, const TailArgs&);
#define OMDS_TAIL_LAUNCHER(ND, ACT, ROWS, FRAME) launch_tail_k<k_tail<ND, ACT, ROWS, FRAME>, ROWS, false>,
#define OMDS_TAIL_SEL_LAUNCHER(ND, ACT, ROWS, FRAME) launch_tail_k<k_tail_sel<ND, ROWS, ACT, FRAME>, ROWS, true>,
static const TailLauncher TAIL_LAUNCHERS[TAIL_N_KEYS] = {OMDS_TAIL_KEYS(OMDS_TAIL_LAUNCHER)};
static const TailLauncher TAIL_SEL_LAUNCHERS[TAIL_N_KEYS] = {OMDS_TAIL_KEYS(OMDS_TAIL_SEL_LAUNCHER)};

// k_tail<.., PART>: the ReLU keys of the table again, entry i beside TAIL_KEYS[i] (nullptr: a tanh key, which has no such form)
using TailPartLauncher = void (*)(hipStream_t, const TailArgs&, int, int);
template <int ND, int ACT, int ROWS, bool FRAME>
static void launch_tail_part_k(hipStream_t s, const TailArgs& a, int t0, int t_end) {
    static std::atomic<uint64_t> configured{0};
    if (omds_first_use_on_device(configured)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_tail<ND, ACT, ROWS, FRAME, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)TailLdsPlan::bytes(OMDS_MAX_HIDDEN + 1, false));
    }
    TailPartArgs pa;
    static_cast<TailArgs&>(pa) = a;
    pa.t0 = t0; pa.t_end = t_end;
    hipLaunchKernelGGL((k_tail<ND, ACT, ROWS, FRAME, true>), dim3(tail_workgroups(t_end - t0, ROWS, a.st.k)), dim3(P2_NT),
                       TailLdsPlan::bytes(a.m.nhh + 1, false), s, pa);
}
template <int ND, int ACT, int ROWS, bool FRAME>
constexpr TailPartLauncher tail_part_launcher() {
    if constexpr (ACT == OMDS_ACT_RELU) return launch_tail_part_k<ND, ACT, ROWS, FRAME>;
    else return nullptr;
}
#define OMDS_TAIL_PART_LAUNCHER(ND, ACT, ROWS, FRAME) tail_part_launcher<ND, ACT, ROWS, FRAME>(),
static const TailPartLauncher TAIL_PART_LAUNCHERS[TAIL_N_KEYS] = {OMDS_TAIL_KEYS(OMDS_TAIL_PART_LAUNCHER)};

static void launch_tail_key(const TailLauncher* launchers, const TailKey& key, hipStream_t s, const TailArgs& a) {
    const int i = tail_key_index(key);
    // A miss cannot happen: omds_tail_supported / omds_tail_sel_supported (the routes ask them, propagate.hip) admit n_dof 7 and 2 only,
    // an activation is ReLU or tanh, the choosers return 4 only under g4_ok, which the plan keys grant to ReLU networks outside
    // the moving frame alone (frame_rows turns a 4 into 16 or 32), and 16 and 32 exist for every (n_dof, activation, frame)
    // (tests/test_tail_plan_cpu.py walks the grid).
    if (i < 0) {   // (not an assert: whatever the build's flags, a miss neither launches nothing in silence nor indexes the table)
        fprintf(stderr, "omds: no tail kernel is instantiated for n_dof %d, activation %d, %d rows, frame %d\n", key.n_dof, key.act, key.rows, (int)key.frame);
        abort();
    }
    launchers[i](s, a);
}

// The `forced` argument of the row choosers: the tile shape of the test hook omds_debug_force_tile_rows (libomds_hip_test.so,
// include/omds_test.h).  The release library has no hook: 0 = the launcher's own choice.
#ifdef OMDS_TEST_HOOKS
static std::atomic<int> g_force_sel_rows{0}, g_force_tail_rows{0};
void omds_force_tile_rows(int tail_sel_rows, int tail_rows) {
    g_force_sel_rows.store(tail_sel_rows);
    g_force_tail_rows.store(tail_rows);
}
#define OMDS_FORCED_ROWS(slot) (slot).load()
#else
#define OMDS_FORCED_ROWS(slot) 0
#endif

bool omds_tail_sel_supported(int n_dof, int k) { return (n_dof == 7 || n_dof == 2) && k >= 1 && k <= 32; }

void omds_launch_tail_sel(hipStream_t s, const MlpDev& m, const float* Fp, const float* radius, const float* xyzr,
                          float* Fq, int O, const StepArgs& st, const ExactOut& ex, const TailScreen& scr) {
    TailArgs a;
    a.e_bound = scr.e_bound;
    a.viol = scr.viol;
    a.FqH = reinterpret_cast<_Float16*>(scr.FqH);
    a.ldF = scr.ldF;
    a.n_slots = 0;
    a.m = m; a.Fp = Fp; a.radius = radius; a.xyzr = xyzr; a.Dmin = nullptr; a.ldD = O; a.Fq = Fq; a.FqOut = Fq; a.dscr = nullptr; a.O = O; a.st = st;
    a.rowlist = scr.rowlist; a.range = scr.range; a.ex = ex;
    launch_tail_key(TAIL_SEL_LAUNCHERS, tail_sel_plan_key(st.n, m.act, m.skip_mask == 0 && m.nhh >= 1, st.frame != 0, st.N, st.k, omds_cu_count(),
                                                          OMDS_FORCED_ROWS(g_force_sel_rows)), s, a);
}

bool omds_tail_supported(int n_dof, int k) { return (n_dof == 7 || n_dof == 2) && k >= 1 && k <= P2_MT; }

int omds_pass2_rows(int N, int k) { return omds_tail_rows(N, k, false, omds_cu_count(), OMDS_FORCED_ROWS(g_force_tail_rows)); }

void omds_launch_tail(hipStream_t s, const MlpDev& m, const float* Fp, const float* radius, const float* xyzr,
                      const float* Dmin, float* Fq, float* dscr, int O, const StepArgs& st, const TailScreen& scr, bool shared_row,
                      int first, int count) {
    TailArgs a;
    a.ldD = shared_row ? 0 : O;
    a.FqH = reinterpret_cast<_Float16*>(scr.FqH);
    a.ldF = scr.ldF;
    const TailKey key = tail_plan_key(st.n, m.act, m.skip_mask == 0 && m.nhh >= 1, st.frame != 0, st.N, st.k, omds_cu_count(),
                                      OMDS_FORCED_ROWS(g_force_tail_rows));
    a.n_slots = tail_workgroups(st.N, key.rows, st.k);
    a.rowlist = nullptr; a.range = scr.range; a.ex = ExactOut{}; a.e_bound = scr.e_bound; a.viol = scr.viol;
    a.m = m; a.Fp = Fp; a.radius = radius; a.xyzr = xyzr; a.Dmin = Dmin; a.Fq = Fq; a.FqOut = scr.FqOut ? scr.FqOut : Fq; a.dscr = dscr; a.O = O; a.st = st;
    if (count < 0) {
        launch_tail_key(TAIL_LAUNCHERS, key, s, a);
        return;
    }
    // a part of the batch: the key above is the whole batch's, so the part runs the tile shape its rollouts have in the whole launch
    const int i = tail_key_index(key);
    if (i < 0 || !TAIL_PART_LAUNCHERS[i]) {   // cannot happen: the plan parts the propagate of a compacting (ReLU) network only
        fprintf(stderr, "omds: no part tail kernel is instantiated for n_dof %d, activation %d, %d rows, frame %d\n", key.n_dof, key.act, key.rows, (int)key.frame);
        abort();
    }
    TAIL_PART_LAUNCHERS[i](s, a, first, first + count);
}
