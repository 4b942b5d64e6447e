// The fp32 re-evaluation of the screened step (gfx950): the pass-1 tile code (pass1_tile, bit-identical arithmetic per row) on listed
// rows -- k_exact on the candidates of every horizon step, the audit kernels on the audit sample of a whole propagate.  Grids, rounds
// are screen_plan_def.h's, the LDS sizes pass1_plan_def.h's.
#include <algorithm>

#include "pass1_tile.h"

static_assert(P1_LDH == LDH && SC_WIDTH == OMDS_WIDTH, "pass1_plan_def.h sizes the tiles of pass1_tile, screen_plan_def.h the bias table");

// k_exact: fp32 pass-1 tiles over the listed rows, 16 rows per tile (v_mfma_f32_16x16x4 fed in the k order of the 32-row
// kernels: the same bits per row, mfma_gemm.h), up to three workgroups resident per CU (78 registers).  A tile is a chain of
// dependent GEMMs on one CU, so what counts is (a) the granularity -- 9.2 candidates per rollout at N = 1024 are 590 tiles of
// 16 rows for 768 slots, where 32-row tiles were 295 for 256 CUs and the 39 left over doubled the launch time -- and (b)
// co-residency: three tiles on a CU fill each other's barrier / epilogue / last-layer gaps.  Measured at 9.9 candidates per
// rollout: 52.9 us, against 59.6 (32-row tiles, two resident), 64.1 (an equal share of 32 + 16 rows per CU, one after the
// other) and 58.0 (16-row tiles, two resident).
template <int ACT, TileMode MODE>
__global__ __launch_bounds__(512, 6) void k_exact(MlpDev m, const float* __restrict__ Fq, const float* __restrict__ Fp,
                                                  const float* __restrict__ radius, int O, uint32_t ignored,
                                                  float* __restrict__ Dmin, OmdsDivisor odiv, const int* __restrict__ rowlist,
                                                  const int* __restrict__ total, unsigned* __restrict__ maxerr_bits, ExactOut ex) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = *total;
    for (int blk = blockIdx.x; blk * 16 < n; blk += gridDim.x) {
        pass1_tile<16, 1, 1, ACT, MODE>(m, smem, Fq, Fp, radius, O, n, ignored, Dmin, (long long)blk * 16, odiv, rowlist, maxerr_bits, &ex);
        __syncthreads();   // the tile buffer is reused by the next tile
    }
}

// ReLU networks: TileMode::List -- per entry the exact value, pass 2's distance / arg-min link and the ReLU masks, for k_tail_sel.
// tanh networks: TileMode::ListDeriv -- the same with 1 - h^2 of every hidden unit (ex.deriv: 1 KB per entry and layer) in place of the masks, so
// that k_tail_sel<..., tanh> runs the backward only (round 4; 3 KB per candidate row of HBM traffic against a second forward in
// the tail).  Without ex.deriv (a matrix-mode step: rows too long for the selecting flush AND no derivative buffer), TileMode::ListPatch: the
// exact value replaces the screening value in the matrix Dmin itself and k_tail takes its top-k from the matrix and runs its own
// forward.  The grid is sized for EXACT_RESIDENT resident workgroups per CU; longer lists stride (the list length is only known
// on the device).
void omds_launch_exact(hipStream_t s, const MlpDev& m, const float* Fq, const float* Fp, const float* radius, int O,
                       int B, uint32_t ignored, float* Dmin, const int* rowlist, const int* total, unsigned* maxerr_bits,
                       const ExactOut& ex) {
    if (B <= 0) return;
    const size_t lds = exact_lds_bytes(m.nhh);
    const int ncu = omds_cu_count();
    const long long blocks_max = ((long long)B * O + 15) / 16;
    const unsigned grid = (unsigned)std::min<long long>(blocks_max, (long long)EXACT_RESIDENT * ncu);
    const OmdsDivisor od = OmdsDivisor::make((unsigned)O);
    if (m.act == OMDS_ACT_RELU)
        hipLaunchKernelGGL((k_exact<OMDS_ACT_RELU, TileMode::List>), dim3(grid), dim3(512), lds, s, m, Fq, Fp, radius, O, ignored, Dmin, od, rowlist, total, maxerr_bits, ex);
    else if (ex.deriv)   // the derivative hand-over: k_tail_sel runs the backward on what this launch leaves per entry
        hipLaunchKernelGGL((k_exact<OMDS_ACT_TANH, TileMode::ListDeriv>), dim3(grid), dim3(512), lds, s, m, Fq, Fp, radius, O, ignored, Dmin, od, rowlist, total, maxerr_bits, ex);
    else
        hipLaunchKernelGGL((k_exact<OMDS_ACT_TANH, TileMode::ListPatch>), dim3(grid), dim3(512), lds, s, m, Fq, Fp, radius, O, ignored, Dmin, od, rowlist, total, maxerr_bits, ex);
}

// k_audit: the audit sample of a whole propagate (k_select recorded (row, screening value) of a pseudo-random subset of the
// pairs that were NOT candidates) evaluated in fp32 with the pass-1 tile code -- 64-row tiles, the throughput shape of
// k_pass1, because nothing waits for this launch but the end of the propagate -- against the layer-1 table of ALL horizon
// steps' states ([H*N][256], rebuilt from the stored rollouts by k_rollout_layer1, the arithmetic of the step itself).
// Output: max (Da - D) over the sample, the one-sided error the selection rule bounds by eps (maxerr_bits[2]).
template <int ACT>
__global__ __launch_bounds__(512) void k_audit(MlpDev m, const float* __restrict__ FqAll, const float* __restrict__ Fp,
                                               const float* __restrict__ radius, int O, uint32_t ignored, OmdsDivisor odiv,
                                               const int* __restrict__ rows, const int* __restrict__ total, int cap,
                                               unsigned* __restrict__ maxerr_bits, ExactOut ex) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = min(*total, cap);
    const int G = (int)gridDim.x;
    const AuditRounds ar = audit_rounds(n, G);
    for (int r = 0; r < ar.full; ++r) {
        pass1_tile<64, 2, 1, ACT, TileMode::Audit>(m, smem, FqAll, Fp, radius, O, n, ignored, nullptr, ((long long)r * G + blockIdx.x) * 64, odiv, rows, maxerr_bits, &ex);
        __syncthreads();
    }
    if (ar.last64) {
        if (ar.in_last(blockIdx.x))
            pass1_tile<64, 2, 1, ACT, TileMode::Audit>(m, smem, FqAll, Fp, radius, O, n, ignored, nullptr, ar.last_row0(blockIdx.x), odiv, rows, maxerr_bits, &ex);
    } else if (ar.in_last(blockIdx.x)) {
        pass1_tile<32, 1, 1, ACT, TileMode::Audit>(m, smem, FqAll, Fp, radius, O, n, ignored, nullptr, ar.last_row0(blockIdx.x), odiv, rows, maxerr_bits, &ex);
    }
}
// k_audit of a propagate with an obstacle horizon: Fp / radius hold H slabs of slab_ld rows, and a listed row (step_row0 + t) * O + o
// with step_row0 = (step - 1) * N reads obstacle row (step - 1) * slab_ld + o -- the scene its step saw (ndiv divides by N;
// pass1_tile's SLAB flag).  A kernel of its own: k_audit keeps its argument list.  Still ONE launch for all steps.  The
// rounds are written out in both: through one shared device function the kernels came out up to 18 instructions shorter (EXPERIMENTS.md R26).
template <int ACT>
__global__ __launch_bounds__(512) void k_audit_slabs(MlpDev m, const float* __restrict__ FqAll, const float* __restrict__ Fp,
                                                     const float* __restrict__ radius, int O, uint32_t ignored, OmdsDivisor odiv,
                                                     const int* __restrict__ rows, const int* __restrict__ total, int cap,
                                                     unsigned* __restrict__ maxerr_bits, ExactOut ex, OmdsDivisor ndiv, unsigned slab_ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n = min(*total, cap);
    const int G = (int)gridDim.x;
    const AuditRounds ar = audit_rounds(n, G);
    for (int r = 0; r < ar.full; ++r) {
        pass1_tile<64, 2, 1, ACT, TileMode::Audit, true>(m, smem, FqAll, Fp, radius, O, n, ignored, nullptr, ((long long)r * G + blockIdx.x) * 64, odiv, rows, maxerr_bits, &ex, ndiv, slab_ld);
        __syncthreads();
    }
    if (ar.last64) {
        if (ar.in_last(blockIdx.x))
            pass1_tile<64, 2, 1, ACT, TileMode::Audit, true>(m, smem, FqAll, Fp, radius, O, n, ignored, nullptr, ar.last_row0(blockIdx.x), odiv, rows, maxerr_bits, &ex, ndiv, slab_ld);
    } else if (ar.in_last(blockIdx.x)) {
        pass1_tile<32, 1, 1, ACT, TileMode::Audit, true>(m, smem, FqAll, Fp, radius, O, n, ignored, nullptr, ar.last_row0(blockIdx.x), odiv, rows, maxerr_bits, &ex, ndiv, slab_ld);
    }
}

// one audit kernel: configured for its LDS on the first launch per device, launched on the plan's grid
template <auto KERNEL, typename... Args>
static void launch_audit_kernel(hipStream_t s, unsigned grid, Args... args) {
    static std::atomic<uint64_t> configured{0};
    if (omds_first_use_on_device(configured))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)audit_lds_bytes());
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(512), audit_lds_bytes(), s, args...);
}
void omds_launch_audit(hipStream_t s, const MlpDev& m, const float* FqAll, const float* Fp, const float* radius, int O,
                       uint32_t ignored, const int* rows, const float* da, const int* total, int cap, unsigned* maxerr_bits,
                       int N, int slab_ld) {
    if (cap <= 0) return;
    ExactOut ex{};
    ex.Da = da;
    const unsigned grid = audit_grid(cap);
    const OmdsDivisor od = OmdsDivisor::make((unsigned)O);
    const bool relu = m.act == OMDS_ACT_RELU;
    if (slab_ld > 0) {   // an obstacle horizon: the row's step picks its slab
        const OmdsDivisor nd = OmdsDivisor::make((unsigned)N);
        if (relu) launch_audit_kernel<&k_audit_slabs<OMDS_ACT_RELU>>(s, grid, m, FqAll, Fp, radius, O, ignored, od, rows, total, cap, maxerr_bits, ex, nd, (unsigned)slab_ld);
        else launch_audit_kernel<&k_audit_slabs<OMDS_ACT_TANH>>(s, grid, m, FqAll, Fp, radius, O, ignored, od, rows, total, cap, maxerr_bits, ex, nd, (unsigned)slab_ld);
    } else {
        if (relu) launch_audit_kernel<&k_audit<OMDS_ACT_RELU>>(s, grid, m, FqAll, Fp, radius, O, ignored, od, rows, total, cap, maxerr_bits, ex);
        else launch_audit_kernel<&k_audit<OMDS_ACT_TANH>>(s, grid, m, FqAll, Fp, radius, O, ignored, od, rows, total, cap, maxerr_bits, ex);
    }
}
