// Distance-network kernels for gfx950 (MI355X): exact-fp32 MFMA, activations resident in LDS.
//
// What they replace in the reference (paths relative to python_scripts/):
//   k_pass1          : MPPI.build_nn_input + model_jit.forward over all N*O (rollout, obstacle)
//                      pairs + /100, -radius, link mask, min over links
//                      (ds_mppi/functions/MPPI.py:93-95, 233-243; mlp_learn/sdf/network_macros_mod.py:137-146)
//   k_topk           : mindist_matrix.sort(dim=1)[:, :k]                       (MPPI.py:245-247)
//   k_pass2          : RobotSdfCollisionNet.functorch_vjp on the N*k closest rows: forward,
//                      arg-min link over all raw outputs, analytic backward (ReLU masks + the
//                      positional-encoding chain rule)                         (robot_sdf.py:153-158)
//   k_blend          : softmax(-10 d) blend of the k gradients                 (MPPI.py:270-280)
//
// Design (MI355X-first, not a translation):
//   * the [N*O, n+4] input matrix is never materialised: sin/cos are evaluated per rollout and per
//     obstacle (tables Fq / Fp of encoded inputs), a tile gathers its pairs' 30 inputs into LDS and
//     layer 1 is a K = 32 product like every other layer -- the reference's single chain over
//     [q, p, sin q, sin p, cos q, cos p] does not split into a rollout half plus an obstacle half;
//   * a workgroup owns MT consecutive rows of the virtual (rollout-major) row space, keeps the
//     [MT x 256] activation tile in LDS (row stride 260 floats: conflict-free ds_read_b128 of
//     MFMA A-fragments) across all layers, and streams the pre-packed weights straight from L2
//     into VGPRs as MFMA B-fragments (1 KiB fully coalesced per wave-load, no LDS round trip);
//   * v_mfma_f32_32x32x2_f32: each lane loads four consecutive positions (one ds_read_b128 /
//     buffer_load_dwordx4) and feeds four MFMA steps; the tile is stored k-permuted (omds_kpos) so
//     that the resulting chain runs over k in ASCENDING order from zero, bias added last -- the
//     arithmetic of torch-CPU's addmm, bit for bit;
//   * accumulators stay in registers until the whole layer is done, so the tile is updated in
//     place (one LDS buffer, two barriers per layer).
#include "pass1_tile.h"
#include "pass1_tile_dyn.h"
#include "pass2_device.h"
#include "topk_device.h"
#include "trig_device.h"

static_assert(P1_LDH == LDH && P1_WIDTH == OMDS_WIDTH && P1_IDS == OMDS_IDS && P1_MAX_NHID == OMDS_MAX_HIDDEN + 1, "pass1_plan_def.h restates pass 1's tile");
static_assert(TAIL_MT == P2_MT && TAIL_NT == P2_NT && TAIL_LDH == LDH, "tail_plan_def.h restates pass 2's tile");

// ------------------------------------------------------------------------------------------------
// encoded inputs [x, sin x, cos x] of the rollout states and of the obstacle points (network_macros_mod.py:139-140), each at its
// feature slot part * d + j of a 32-float row; a pair's input row is the OR of its two rows (pass1_tile, pass2_body)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rollout_features(MlpDev m, const float* __restrict__ qT, int ldq, int B,
                                                          float* __restrict__ Fq, _Float16* __restrict__ FqH, int ldF, int slab) {
    const int t = blockIdx.x * 32 + (threadIdx.x >> 3), c = threadIdx.x & 7, n = m.n_dof, d = m.d;
    if (t >= B || c >= n) return;
    const int h = slab > 0 ? t / slab : 0;   // slab > 0: row t is rollout t - h*slab of state slab h ([n][ldq] each)
    const float q = qT[((size_t)h * n + c) * ldq + (t - h * slab)];
    const float sq = omds_sinf(q), cq = omds_cosf(q);
    Fq[(size_t)t * OMDS_FROW + c] = q;
    Fq[(size_t)t * OMDS_FROW + d + c] = sq;
    Fq[(size_t)t * OMDS_FROW + 2 * d + c] = cq;
    // the screening kernel's input row of this rollout (the other slots stay zero)
    if (FqH) omds_screen_store_row(FqH, reinterpret_cast<_Float16*>(m.scrQ), c, d, t, ldF, q, sq, cq);
}

__global__ __launch_bounds__(256) void k_obstacle_features(MlpDev m, const float* __restrict__ xyzr, int O,
                                                           float* __restrict__ Fp, float* __restrict__ radius,
                                                           _Float16* __restrict__ FpH, int ldF) {
    const int o = blockIdx.x * 64 + (threadIdx.x >> 2), c = threadIdx.x & 3, n = m.n_dof, d = m.d, po = d - n;   // po = 3 (x, y, z) or 2 (toy networks)
    if (o >= O) return;
    if (c == 3) { radius[o] = xyzr[o * 4 + 3]; return; }
    if (c >= po) return;
    const float p = xyzr[o * 4 + c];
    const float sp = omds_sinf(p), cp = omds_cosf(p);
    Fp[(size_t)o * OMDS_FROW + n + c] = p;
    Fp[(size_t)o * OMDS_FROW + d + n + c] = sp;
    Fp[(size_t)o * OMDS_FROW + 2 * d + n + c] = cp;
    if (FpH) omds_screen_store_row(FpH, reinterpret_cast<_Float16*>(m.scrP), n + c, d, o, ldF, p, sp, cp);
}

// The same tables for every slab of an obstacle horizon (omds.h: omds_set_obstacle_motion / omds_set_obstacle_horizon): row
// h * ld + o of obsT / radiusT / FpT is obstacle o as step h + 1 of a propagate sees it.  vel != nullptr: the position is
// xyzr + (h dt) vel, ONE fp32 product and one fmaf (slab 0: xyzr itself), the arithmetic of omds_obstacle_horizon_predict; a
// planar-point network (po = 2) keeps z.  vel == nullptr: obsT holds the caller's spheres.
// FpHT / scrPT (optional; screening over the horizon, omds_set_screening_horizon): the fp16 tables k_obstacle_features writes, one
// per slab -- [H][4 pieces][ld][8], slab h being an omds_screen_fidx / omds_screen_sidx table of row capacity ld at element offset
// h * 32 ld -- from the same p, sin p, cos p rounded to fp16: slab 0 holds the bits of the static tables.
__global__ __launch_bounds__(256) void k_obstacle_horizon_features(MlpDev m, const float* __restrict__ xyzr, const float* __restrict__ vel,
                                                                   float dt, int H, int O, int ld, float* __restrict__ obsT,
                                                                   float* __restrict__ radiusT, float* __restrict__ FpT,
                                                                   _Float16* __restrict__ FpHT, _Float16* __restrict__ scrPT) {
    const int r = blockIdx.x * 64 + (threadIdx.x >> 2), c = threadIdx.x & 3, n = m.n_dof, d = m.d, po = d - n;
    if (r >= H * O) return;
    const int h = r / O, o = r - h * O;
    const size_t row = (size_t)h * ld + o;
    float p;
    if (vel) {
        p = xyzr[o * 4 + c];
        if (c < po && h > 0) {
            const float t = (float)h * dt;
            p = fmaf(vel[o * 3 + c], t, p);
        }
        obsT[row * 4 + c] = p;
    } else {
        p = obsT[row * 4 + c];
    }
    if (c == 3) { radiusT[row] = p; return; }
    if (c >= po) return;
    const float sp = omds_sinf(p), cp = omds_cosf(p);
    FpT[row * OMDS_FROW + n + c] = p;
    FpT[row * OMDS_FROW + d + n + c] = sp;
    FpT[row * OMDS_FROW + 2 * d + n + c] = cp;
    if (FpHT) omds_screen_store_row(FpHT + (size_t)h * 32 * ld, scrPT ? scrPT + (size_t)h * 32 * ld : nullptr, n + c, d, o, ld, p, sp, cp);
}

template <int MT, int MR, int NR, int ACT>
__global__ __launch_bounds__((Geo<MT, MR, NR>::NT)) void k_pass1(MlpDev m, const float* __restrict__ Fq,
                                                               const float* __restrict__ Fp,
                                                               const float* __restrict__ radius, int O,
                                                               long long total_rows, uint32_t ignored,
                                                               float* __restrict__ Dmin, OmdsDivisor odiv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    pass1_tile<MT, MR, NR, ACT>(m, smem, Fq, Fp, radius, O, total_rows, ignored, Dmin, (long long)blockIdx.x * MT, odiv);
}

// Mixed-granularity launch: the first n_big workgroups take 64-row tiles, the rest cover the remaining rows
// in 32-row tiles.  Workgroups are dispatched in index order, so the kernel ends on small tiles and the
// drain phase (slots idling while the last tiles finish) shrinks with the tile size.
template <int ACT>
__global__ __launch_bounds__(512) void k_pass1_mixed(const float* __restrict__ Fq, const float* __restrict__ Fp,
                                                     const float* __restrict__ radius, float* __restrict__ Dmin,
                                                     long long total_rows, int O, uint32_t ignored, int n_big,
                                                     OmdsDivisor odiv, MlpDev m) {
    // argument order: the scalars and pointers the layer-1 build needs come first so that they can be preloaded into
    // SGPRs at wave launch (-mllvm -amdgpu-kernarg-preload-count); the weight-pack descriptor is fetched behind them
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // (the rule is called where its value is used: pass1_plan_def.h says why)
    const int b = blockIdx.x;
    if (pass1_mixed_tile(b, n_big).rows == 64) pass1_tile<64, 2, 1, ACT>(m, smem, Fq, Fp, radius, O, total_rows, ignored, Dmin, pass1_mixed_tile(b, n_big).row0, odiv);
    else pass1_tile<32, 1, 1, ACT>(m, smem, Fq, Fp, radius, O, total_rows, ignored, Dmin, pass1_mixed_tile(b, n_big).row0, odiv);
}

// k_pass1 on per-tile compacted levels (pass1_tile_dyn): the same launch shape as k_pass1_mixed
__global__ __launch_bounds__(512) void k_pass1_dyn(const float* __restrict__ Fq, const float* __restrict__ Fp,
                                                   const float* __restrict__ radius, float* __restrict__ Dmin,
                                                   long long total_rows, int O, uint32_t ignored, int n_big,
                                                   OmdsDivisor odiv, MlpDev m) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x;
    if (pass1_mixed_tile(b, n_big).rows == 64) pass1_tile_dyn<64, 2>(m, smem, Fq, Fp, radius, O, total_rows, ignored, Dmin, pass1_mixed_tile(b, n_big).row0, odiv);
    else pass1_tile_dyn<32, 1>(m, smem, Fq, Fp, radius, O, total_rows, ignored, Dmin, pass1_mixed_tile(b, n_big).row0, odiv);
}

// ... on block-ordered tiles (pass1_tile_dyn<.., BLK>; tile_order.hip): workgroup b < n_big is block (b / ncb, b % ncb) of the grid of
// 16-rollout x 4-obstacle blocks over the first nrb16 * 16 entries of rperm, the rest are the 8 x 4 blocks of the remaining entries
// (pass1_block, pass1_plan_def.h)
__global__ __launch_bounds__(512) void k_pass1_dyn_blk(const float* __restrict__ Fq, const float* __restrict__ Fp,
                                                       const float* __restrict__ radius, float* __restrict__ Dmin,
                                                       const int* __restrict__ rperm, const int* __restrict__ operm, int N, int O,
                                                       uint32_t ignored, int n_big, int nrb16, OmdsDivisor cdiv, MlpDev m) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    auto block = [&] { return pass1_block(blockIdx.x, n_big, nrb16, (unsigned)(O + 3) >> 2, N, O, [&](unsigned b) { return cdiv.div(b); }); };
    auto tile_block = [&] { const Pass1Block k = block(); return TileBlock{rperm + k.r0, operm + k.o0, k.nr, k.no}; };
    if (block().big) pass1_tile_dyn<64, 2, true>(m, smem, Fq, Fp, radius, O, 0, ignored, Dmin, 0, cdiv, tile_block());
    else pass1_tile_dyn<32, 1, true>(m, smem, Fq, Fp, radius, O, 0, ignored, Dmin, 0, cdiv, tile_block());
}

// k_pass1 in pass1_tile's TileMode::EmitAll (a kernel of its own: the tuned Dmin kernels keep their argument lists and code): beside Dmin
// every pair's pass-2 distance, arg-min link and ReLU masks go to `ex`, indexed by the pair.  On 16- and 32-row tiles only: the route
// that launches it ends below the Medium class (PASS1_EMIT_MAX_PAIRS, pass1_plan_def.h).
template <int MT, int MR, int NR, int ACT>
__global__ __launch_bounds__((Geo<MT, MR, NR>::NT)) void k_pass1e(MlpDev m, const float* __restrict__ Fq,
                                                                const float* __restrict__ Fp,
                                                                const float* __restrict__ radius, int O,
                                                                long long total_rows, uint32_t ignored,
                                                                float* __restrict__ Dmin, OmdsDivisor odiv, ExactOut ex) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    pass1_tile<MT, MR, NR, ACT, TileMode::EmitAll>(m, smem, Fq, Fp, radius, O, total_rows, ignored, Dmin, (long long)blockIdx.x * MT, odiv, nullptr, nullptr, &ex);
}

// ------------------------------------------------------------------------------------------------
// top-k (ascending, ties by lower obstacle index): one wave per rollout
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_topk(const float* __restrict__ Dmin, int B, int O, int k,
                                              int32_t* __restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= B) return;
    topk_row(Dmin + (size_t)t * O, O, k, lane, [&](int j, int bi) { idx[(size_t)t * k + j] = bi; });
}

// ------------------------------------------------------------------------------------------------
// pass 2: forward + analytic backward on the N*k closest rows. 32 rows per workgroup, 8 waves,
// wave w owns output columns [32w, 32w+32). ReLU masks live in LDS as 16 bits per thread/layer
// in the MFMA C-layout (the same lane owns the same (row, col) in every layer).
// ------------------------------------------------------------------------------------------------
template <int ACT, int ROWS>
__global__ __launch_bounds__(P2_NT) void k_pass2(MlpDev m, const float* __restrict__ Fq,
                                                 const float* __restrict__ Fp, const float* __restrict__ radius,
                                                 const float* __restrict__ xyzr, const int32_t* __restrict__ idx,
                                                 int total_rows, int k, const float* __restrict__ qT, int ldq,
                                                 float* __restrict__ gradx, float* __restrict__ drow,
                                                 float* __restrict__ yraw, int32_t* __restrict__ minidx,
                                                 float* __restrict__ dscr, int seed_col) {
    // dscr (tanh only): [nhh+1][rows padded to 32][256] activation derivatives 1 - h^2, L2-resident scratch
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const TailLdsPlan o(m.nhh + 1, false);   // pass 2's six blocks (tail_plan_def.h)
    P2Smem sm;
    sm.Hs = smem + o.Hs;
    sm.gf = smem + o.gf;
    sm.maskL = reinterpret_cast<uint16_t*>(smem + o.maskL);
    sm.rowT = reinterpret_cast<int*>(smem + o.rowT);
    sm.rowO = reinterpret_cast<int*>(smem + o.rowO);
    sm.rowMin = reinterpret_cast<int*>(smem + o.rowMin);
    const int tid = threadIdx.x;
    const int R0 = blockIdx.x * ROWS;
    if (tid < ROWS) {
        const int R = R0 + tid;
        int t = -1, o = 0;
        if (R < total_rows) { t = R / k; o = idx[R]; }
        sm.rowT[tid] = t;
        sm.rowO[tid] = o;
    }
    __syncthreads();
    pass2_body<ACT, ROWS>(m, sm, Fq, Fp, radius, xyzr, R0, total_rows, qT, ldq, gradx, drow, R0, yraw, minidx, dscr,
                                 (size_t)gridDim.x * ROWS * OMDS_WIDTH, R0, nullptr, 0, seed_col);
}

// ------------------------------------------------------------------------------------------------
// blend of the k closest gradients (MPPI.py:270-280), standalone form for omds_dist_grad
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_blend(const float* __restrict__ gradx, const float* __restrict__ drow, int B,
                                               int k, int d, int n, float softmax_k, float* __restrict__ dist,
                                               float* __restrict__ nngrad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B) return;
    float mx = -__builtin_inff();
    for (int j = 0; j < k; ++j) mx = fmaxf(mx, softmax_k * drow[t * k + j]);
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += expf(softmax_k * drow[t * k + j] - mx);
    for (int c = 0; c < n; ++c) {
        float g = 0.f;
        for (int j = 0; j < k; ++j) g += gradx[(size_t)(t * k + j) * d + c] * (expf(softmax_k * drow[t * k + j] - mx) / s);
        nngrad[(size_t)t * n + c] = g;
    }
    dist[t] = drow[t * k];
}

// ------------------------------------------------------------------------------------------------
// the moving frame's two quantities, standalone form for omds_approach_rate (omds.h: omds_moving_frame_velocity; the arithmetic
// of modulate_core<.., FRAME = true>, step_device.h)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_approach_rate(const float* __restrict__ gradx, const float* __restrict__ drow,
                                                       const int32_t* __restrict__ idx, const float* __restrict__ vel, int ldv, int B,
                                                       int k, int d, int n, float softmax_k, float max_speed,
                                                       float* __restrict__ rate_out, float* __restrict__ qo_out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B) return;
    float mx = -__builtin_inff();
    for (int j = 0; j < k; ++j) mx = fmaxf(mx, softmax_k * drow[t * k + j]);
    float s = 0.f;
    for (int j = 0; j < k; ++j) s += expf(softmax_k * drow[t * k + j] - mx);
    float g[OMDS_MAX_DOF], rate = 0.f, gn2 = 0.f;
    for (int c = 0; c < n; ++c) g[c] = 0.f;
    for (int j = 0; j < k; ++j) {
        const float w = expf(softmax_k * drow[t * k + j] - mx) / s;
        const float* gr = gradx + (size_t)(t * k + j) * d;
        const float* vo = vel + (size_t)idx[t * k + j] * ldv;
        for (int c = 0; c < n; ++c) g[c] = fmaf(gr[c], w, g[c]);
        float sj = 0.f;
        for (int c = 0; c < d - n; ++c) sj = fmaf(gr[n + c], vo[c], sj);
        rate = fmaf(sj, w, rate);
    }
    for (int c = 0; c < n; ++c) gn2 = fmaf(g[c], g[c], gn2);
    const float gn = sqrtf(gn2);
    float r = rate / gn;
    if (gn == 0.f || !(fabsf(r) <= 3.402823466e+38f)) r = 0.f;
    r = fminf(fmaxf(r, -max_speed), max_speed);
    rate_out[t] = rate;
    for (int c = 0; c < n; ++c) qo_out[(size_t)t * n + c] = gn == 0.f ? 0.f : -r * (g[c] / gn);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
void omds_launch_approach_rate(hipStream_t s, const float* gradx, const float* drow, const int32_t* idx, const float* vel, int ldv,
                               int B, int k, int d, int n, float softmax_k, float max_speed, float* rate, float* qo) {
    if (B <= 0) return;
    hipLaunchKernelGGL(k_approach_rate, dim3((B + 255) / 256), dim3(256), 0, s, gradx, drow, idx, vel, ldv, B, k, d, n, softmax_k, max_speed,
                       rate, qo);
}

void omds_launch_rollout_features(hipStream_t s, const MlpDev& m, const float* qT, int ldq, int B, float* Fq, uint16_t* FqH, int ldF, int slab) {
    if (B <= 0) return;
    hipLaunchKernelGGL(k_rollout_features, dim3((B + 31) / 32), dim3(256), 0, s, m, qT, ldq, B, Fq, reinterpret_cast<_Float16*>(FqH), ldF, slab);
}

void omds_launch_obstacle_features(hipStream_t s, const MlpDev& m, const float* xyzr, int O, float* Fp, float* radius, uint16_t* FpH, int ldF) {
    if (O <= 0) return;
    hipLaunchKernelGGL(k_obstacle_features, dim3((O + 63) / 64), dim3(256), 0, s, m, xyzr, O, Fp, radius, reinterpret_cast<_Float16*>(FpH), ldF);
}

void omds_launch_obstacle_horizon_features(hipStream_t s, const MlpDev& m, const float* xyzr, const float* vel, float dt, int H, int O,
                                           int ld, float* obsT, float* radiusT, float* FpT, uint16_t* FpHT, uint16_t* scrPT) {
    if (H <= 0 || O <= 0) return;
    hipLaunchKernelGGL(k_obstacle_horizon_features, dim3((unsigned)(((long long)H * O + 63) / 64)), dim3(256), 0, s, m, xyzr, vel, dt, H, O, ld,
                       obsT, radiusT, FpT, reinterpret_cast<_Float16*>(FpHT), reinterpret_cast<_Float16*>(scrPT));
}

// one kernel with a dynamic LDS block: configured for lds_max on the first launch per device, launched with lds
template <auto KERNEL, typename... Args>
static void launch_lds_kernel(hipStream_t s, long long grid, int threads, size_t lds, size_t lds_max, const Args&... args) {
    static std::atomic<uint64_t> configured{0};
    if (omds_first_use_on_device(configured))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(threads), lds, s, args...);
}

// Grids, tile heights and LDS sizes of every launch below: pass1_plan_def.h.
// the dense launch of one tile height (Tiny, Small, Medium)
template <int MT, int MR, int NR>
static void launch_pass1_t(hipStream_t s, const MlpDev& m, const float* Fq, const float* Fp, const float* radius,
                           int O, long long total, uint32_t ignored, float* Dmin, long long tiles) {
    const size_t lds = pass1_dmin_lds_bytes(MT);
    const OmdsDivisor od = OmdsDivisor::make((unsigned)O);
    if (m.act == OMDS_ACT_RELU) launch_lds_kernel<&k_pass1<MT, MR, NR, OMDS_ACT_RELU>>(s, tiles, Geo<MT, MR, NR>::NT, lds, lds, m, Fq, Fp, radius, O, total, ignored, Dmin, od);
    else launch_lds_kernel<&k_pass1<MT, MR, NR, OMDS_ACT_TANH>>(s, tiles, Geo<MT, MR, NR>::NT, lds, lds, m, Fq, Fp, radius, O, total, ignored, Dmin, od);
}

void omds_launch_pass1(hipStream_t s, const MlpDev& m, const float* Fq, const float* Fp, const float* radius,
                       int O, int B, uint32_t ignored, float* Dmin) {
    const long long total = (long long)B * O;
    if (total <= 0) return;
    const Pass1Size size = pass1_size(total);
    const bool compact = m.compact && size != Pass1Size::Tiny;   // per-tile compaction: k_pass1_dyn has no 16-row tiles
    const Pass1Grid g = pass1_grid(total, compact);
    const OmdsDivisor od = OmdsDivisor::make((unsigned)O);
    if (compact) {
        launch_lds_kernel<&k_pass1_dyn>(s, g.workgroups(), 512, pass1_dyn_lds_bytes(), pass1_dyn_lds_bytes(), Fq, Fp, radius, Dmin, total, O, ignored, (int)g.n_big, od, m);
        return;
    }
    switch (size) {
        case Pass1Size::Large:
            if (m.act == OMDS_ACT_RELU) launch_lds_kernel<&k_pass1_mixed<OMDS_ACT_RELU>>(s, g.workgroups(), 512, pass1_mixed_lds_bytes(), pass1_mixed_lds_bytes(), Fq, Fp, radius, Dmin, total, O, ignored, (int)g.n_big, od, m);
            else launch_lds_kernel<&k_pass1_mixed<OMDS_ACT_TANH>>(s, g.workgroups(), 512, pass1_mixed_lds_bytes(), pass1_mixed_lds_bytes(), Fq, Fp, radius, Dmin, total, O, ignored, (int)g.n_big, od, m);
            break;
        case Pass1Size::Medium: launch_pass1_t<64, 2, 1>(s, m, Fq, Fp, radius, O, total, ignored, Dmin, g.workgroups()); break;
        case Pass1Size::Small: launch_pass1_t<32, 1, 1>(s, m, Fq, Fp, radius, O, total, ignored, Dmin, g.workgroups()); break;
        case Pass1Size::Tiny: launch_pass1_t<16, 1, 1>(s, m, Fq, Fp, radius, O, total, ignored, Dmin, g.workgroups()); break;
    }
}

// The block-ordered form of the compacting launch (pass1_block_grid)
bool omds_pass1_blocks_ok(const MlpDev& m, int N, int O) {
    return m.compact && pass1_size((long long)N * O) != Pass1Size::Tiny && N <= OMDS_ORDER_MAX_ROLLOUTS && O <= OMDS_ORDER_MAX_OBS;
}
void omds_launch_pass1_blocks(hipStream_t s, const MlpDev& m, const float* Fq, const float* Fp, const float* radius, int O, int N,
                              uint32_t ignored, float* Dmin, const int* rperm, const int* operm, int first) {
    const Pass1BlockGrid g = pass1_block_grid(N, O);
    // a part of the batch: the kernel addresses Fq and Dmin by the entries of rperm, which count from the part's first rollout
    Fq += (size_t)first * OMDS_FROW;
    Dmin += (size_t)first * O;
    launch_lds_kernel<&k_pass1_dyn_blk>(s, g.workgroups(), 512, pass1_dyn_lds_bytes(), pass1_dyn_lds_bytes(), Fq, Fp, radius, Dmin, rperm, operm, N, O, ignored,
                                        (int)g.n_big, g.nrb16, OmdsDivisor::make((unsigned)g.ncb), m);
}

// pass 1 that also leaves every pair's pass-2 distance, arg-min link and ReLU masks (pass1_tile, TileMode::EmitAll) -- the same tile choice as
// omds_launch_pass1, so Dmin is the same launch shape's bits (they are the same bits in every shape anyway).  ReLU networks only, and
// up to PASS1_EMIT_MAX_PAIRS pairs: Tiny and Small launches.
template <int MT, int MR, int NR>
static void launch_pass1e_t(hipStream_t s, const MlpDev& m, const float* Fq, const float* Fp, const float* radius,
                            int O, long long total, uint32_t ignored, float* Dmin, const ExactOut& ex, long long tiles) {
    launch_lds_kernel<&k_pass1e<MT, MR, NR, OMDS_ACT_RELU>>(s, tiles, Geo<MT, MR, NR>::NT, pass1_emit_lds_bytes(MT, m.nhh + 1), pass1_emit_lds_max_bytes(MT), m, Fq, Fp, radius,
                                                            O, total, ignored, Dmin, OmdsDivisor::make((unsigned)O), ex);
}
void omds_launch_pass1_emit(hipStream_t s, const MlpDev& m, const float* Fq, const float* Fp, const float* radius,
                            int O, int B, uint32_t ignored, float* Dmin, const ExactOut& ex) {
    const long long total = (long long)B * O;
    if (total <= 0) return;
    if (!pass1_emit_ok(total)) {   // cannot happen: choose_route (propagate.hip) asks the same predicate (not an assert: whatever the build's flags, no silent no-op)
        fprintf(stderr, "omds: the emitting pass 1 has no kernel for %lld pairs\n", total);
        abort();
    }
    const long long tiles = pass1_grid(total, false).workgroups();
    if (pass1_size(total) == Pass1Size::Small) launch_pass1e_t<32, 1, 1>(s, m, Fq, Fp, radius, O, total, ignored, Dmin, ex, tiles);
    else launch_pass1e_t<16, 1, 1>(s, m, Fq, Fp, radius, O, total, ignored, Dmin, ex, tiles);
}

void omds_launch_topk(hipStream_t s, const float* Dmin, int B, int O, int k, int32_t* idx) {
    if (B <= 0) return;
    hipLaunchKernelGGL(k_topk, dim3((B + 3) / 4), dim3(256), 0, s, Dmin, B, O, k, idx);
}

void omds_launch_pass2(hipStream_t s, const MlpDev& m, const float* Fq, const float* Fp, const float* radius,
                       const float* xyzr, const int32_t* idx, int B, int k, const float* qT, int ldq, float* gradx,
                       float* drow, float* yraw, int32_t* minidx, float* dscr, int seed_col) {
    const int total = B * k;
    if (total <= 0) return;
    // same tile height as the fused tail would pick for this batch, so that the batch entry points (omds_dist_grad)
    // reproduce the step path bit for bit
    const int rows = omds_pass2_rows(B, k);
#define OMDS_P2_LAUNCH(A, R)                                                                                                                        \
    launch_lds_kernel<&k_pass2<A, R>>(s, (total + rows - 1) / rows, P2_NT, TailLdsPlan::pass2_bytes(m.nhh + 1), TailLdsPlan::pass2_bytes(OMDS_MAX_HIDDEN + 1), m, Fq, \
                                      Fp, radius, xyzr, idx, total, k, qT, ldq, gradx, drow, yraw, minidx, dscr, seed_col)
    if (m.act == OMDS_ACT_RELU) { if (rows == 16) OMDS_P2_LAUNCH(OMDS_ACT_RELU, 16); else OMDS_P2_LAUNCH(OMDS_ACT_RELU, 32); }
    else { if (rows == 16) OMDS_P2_LAUNCH(OMDS_ACT_TANH, 16); else OMDS_P2_LAUNCH(OMDS_ACT_TANH, 32); }
#undef OMDS_P2_LAUNCH
}

void omds_launch_blend(hipStream_t s, const float* gradx, const float* drow, int B, int k, int d, int n,
                       float softmax_k, float* dist, float* nngrad) {
    if (B <= 0) return;
    hipLaunchKernelGGL(k_blend, dim3((B + 255) / 256), dim3(256), 0, s, gradx, drow, B, k, d, n, softmax_k, dist, nngrad);
}
