// Test hook (include/omds_test.h, libomds_hip_test.so only: the Makefile links this file into no other library): ONE horizon step of
// modulate_core (step_device.h) on caller-supplied inputs, with no network and no context, for tests/test_gpu_step_edges.py.
//   nsub = 1 : the production launcher omds_launch_modulate (k_modulate<ND, FRAME>, ND = 1..7, the SEDS branch included) as shipped
//   nsub = 16: k_modulate16 below, which calls modulate_core<ND, 16, false, FRAME> the way the fused step kernels do (step_advance, step_epilogue.h:
//              16 consecutive lanes of a wave per rollout, sub = lane & 15, whole 16-lane groups on or off by t < N), gradients and
//              distances in global memory; ND = 2 and 7, the two the fused kernels instantiate, and never with SEDS (no product kernel
//              instantiates WITH_SEDS with NSUB = 16)
// Every argument is checked on the host: a mistaken test gets OMDS_ERR_INVALID_ARG, never an out-of-range read on the device.
#include "omds_internal.h"
#include "omds_test.h"

#include "step_device.h"

template <int ND, bool FRAME>
__global__ __launch_bounds__(256) void k_modulate16(StepArgs a) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = tid >> 4, sub = tid & 15;
    if (t >= a.N) return;
    float q[ND], qn[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) q[j] = a.trajT[((size_t)(a.step - 1) * ND + j) * a.N + t];
    modulate_core<ND, 16, false, FRAME>(a, a.step, t, sub, a.gradx, a.drow, t * a.k, q, qn, a.rowObs);
}

template <int ND>
static void launch_modulate16_t(const StepArgs& a) {
    const dim3 grid((a.N + 15) / 16), block(256);
    if (a.frame) hipLaunchKernelGGL((k_modulate16<ND, true>), grid, block, 0, 0, a);
    else hipLaunchKernelGGL((k_modulate16<ND, false>), grid, block, 0, 0, a);
}

namespace {
constexpr int MT_MAX_N = 1 << 16, MT_MAX_H = 64, MT_MAX_K = 1 << 10, MT_MAX_O = 1 << 16, MT_MAX_D = 16;

bool args_ok(const omds_test_modulate_args* a) {
    if (!a) return false;
    const int n = a->n_dof;
    if (n < 1 || n > OMDS_MAX_DOF || (a->nsub != 1 && a->nsub != 16)) return false;
    if (a->N < 1 || a->N > MT_MAX_N || a->H < 1 || a->H > MT_MAX_H || a->step < 1 || a->step > a->H) return false;
    if (a->Kmax < 1 || a->Kmax > MT_MAX_K || a->K < 0 || a->K > a->Kmax) return false;
    if (a->k < 1 || a->k > 32 || !omds_tail_supported(7, a->k)) return false;   // the tails' maximum
    if (a->d < n || a->d > MT_MAX_D) return false;
    if (!a->qf || !a->q || !a->drow || !a->gradx || !a->maxact || !a->phisum0) return false;
    if (a->K > 0 && (!a->mu || !a->sigma || !a->alpha)) return false;
    if (!a->q_next || !a->qdot || !a->dist || !a->dot || !a->act || !a->normal || !a->kval) return false;
    if (!(a->prm.rbf_p > 0.f)) return false;
    if (a->seds_G != 0) {
        if (a->seds_G < 1 || a->seds_G > 64 || a->A) return false;
        if (!a->seds_mu_in || !a->seds_b || !a->seds_sigma_inv || !a->seds_A || !a->seds_prior || !a->seds_den) return false;
    }
    if (a->nsub == 16 && ((n != 2 && n != 7) || a->seds_G != 0)) return false;
    if (a->frame) {
        if (a->O < 1 || a->O > MT_MAX_O || a->ldVel < a->d - n || a->ldVel > 8 || !a->vel || !a->rowObs) return false;
        if (!(a->frame_max >= 0.f)) return false;   // fminf / fmaxf with a NaN or negative clamp is nobody's intent
        for (size_t e = 0; e < (size_t)a->N * a->k; ++e)
            if (a->rowObs[e] < 0 || a->rowObs[e] >= a->O) return false;
    }
    return true;
}
}   // namespace

#define HCK(expr) do { if ((expr) != hipSuccess) { rc = OMDS_ERR_HIP; goto done; } } while (0)

extern "C" OMDS_API int omds_test_modulate(const omds_test_modulate_args* a) {
    if (!args_ok(a)) return OMDS_ERR_INVALID_ARG;
    int rc = OMDS_OK;
    const int n = a->n_dof, N = a->N, K = a->K, Kmax = a->Kmax, k = a->k, d = a->d, H = a->H, i = a->step;
    const size_t F = sizeof(float);
    // device buffers: inputs, then outputs (the rollouts hold H + 1 slabs: slab `step` exists at step == H too, and must stay untouched)
    const size_t n_traj = (size_t)(H + 1) * n * N, n_hN = (size_t)H * N, n_hnN = (size_t)H * n * N, n_kval = (size_t)H * Kmax * N,
                 n_nN = (size_t)n * N, n_KN = (size_t)Kmax * N, n_rows = (size_t)N * k;
    float *d_traj = nullptr, *d_dist = nullptr, *d_dot = nullptr, *d_act = nullptr, *d_normal = nullptr, *d_kval = nullptr, *d_qdot = nullptr,
          *d_maxact = nullptr, *d_phisum0 = nullptr, *d_mu = nullptr, *d_sigma = nullptr, *d_alpha = nullptr, *d_gradx = nullptr,
          *d_drow = nullptr, *d_A = nullptr, *d_seds = nullptr, *d_vel = nullptr;
    int* d_rowObs = nullptr;
    StepArgs s{};
    HCK(hipMalloc(&d_traj, n_traj * F));
    HCK(hipMalloc(&d_dist, n_hN * F));
    HCK(hipMalloc(&d_dot, n_hN * F));
    HCK(hipMalloc(&d_act, n_hN * F));
    HCK(hipMalloc(&d_normal, n_hnN * F));
    HCK(hipMalloc(&d_kval, n_kval * F));
    HCK(hipMalloc(&d_qdot, n_nN * F));
    HCK(hipMalloc(&d_maxact, n_KN * F));
    HCK(hipMalloc(&d_phisum0, (size_t)Kmax * F));
    HCK(hipMalloc(&d_gradx, n_rows * d * F));
    HCK(hipMalloc(&d_drow, n_rows * F));
    // 0xFF everywhere: an output the step did not write reads back as the bit pattern 0xFFFFFFFF
    HCK(hipMemset(d_traj, 0xFF, n_traj * F));
    HCK(hipMemset(d_dist, 0xFF, n_hN * F));
    HCK(hipMemset(d_dot, 0xFF, n_hN * F));
    HCK(hipMemset(d_act, 0xFF, n_hN * F));
    HCK(hipMemset(d_normal, 0xFF, n_hnN * F));
    HCK(hipMemset(d_kval, 0xFF, n_kval * F));
    HCK(hipMemset(d_qdot, 0xFF, n_nN * F));
    HCK(hipMemcpy(d_traj + (size_t)(i - 1) * n * N, a->q, n_nN * F, hipMemcpyHostToDevice));
    HCK(hipMemcpy(d_maxact, a->maxact, n_KN * F, hipMemcpyHostToDevice));
    HCK(hipMemcpy(d_phisum0, a->phisum0, (size_t)Kmax * F, hipMemcpyHostToDevice));
    HCK(hipMemcpy(d_gradx, a->gradx, n_rows * d * F, hipMemcpyHostToDevice));
    HCK(hipMemcpy(d_drow, a->drow, n_rows * F, hipMemcpyHostToDevice));
    if (K > 0) {
        HCK(hipMalloc(&d_mu, (size_t)K * n * N * F));
        HCK(hipMalloc(&d_sigma, (size_t)K * N * F));
        HCK(hipMalloc(&d_alpha, (size_t)K * n * N * F));
        HCK(hipMemcpy(d_mu, a->mu, (size_t)K * n * N * F, hipMemcpyHostToDevice));
        HCK(hipMemcpy(d_sigma, a->sigma, (size_t)K * N * F, hipMemcpyHostToDevice));
        HCK(hipMemcpy(d_alpha, a->alpha, (size_t)K * n * N * F, hipMemcpyHostToDevice));
    }
    if (a->A) {
        HCK(hipMalloc(&d_A, (size_t)n * n * F));
        HCK(hipMemcpy(d_A, a->A, (size_t)n * n * F, hipMemcpyHostToDevice));
    }
    if (a->seds_G > 0) {
        const std::vector<float> pk = omds_pack_seds(n, a->seds_G, a->seds_mu_in, a->seds_b, a->seds_sigma_inv, a->seds_A, a->seds_prior, a->seds_den);
        HCK(hipMalloc(&d_seds, pk.size() * F));
        HCK(hipMemcpy(d_seds, pk.data(), pk.size() * F, hipMemcpyHostToDevice));
    }
    if (a->frame) {
        HCK(hipMalloc(&d_vel, (size_t)a->O * a->ldVel * F));
        HCK(hipMalloc(&d_rowObs, n_rows * sizeof(int)));
        HCK(hipMemcpy(d_vel, a->vel, (size_t)a->O * a->ldVel * F, hipMemcpyHostToDevice));
        HCK(hipMemcpy(d_rowObs, a->rowObs, n_rows * sizeof(int), hipMemcpyHostToDevice));
    }
    s.N = N; s.H = H; s.n = n; s.K = K; s.Kmax = Kmax; s.k = k; s.d = d; s.step = i;
    s.trajT = d_traj; s.distT = d_dist; s.dotT = d_dot; s.actT = d_act; s.normalT = d_normal; s.kvalT = d_kval; s.qdotT = d_qdot;
    s.maxact = d_maxact; s.phisum0 = d_phisum0;
    s.muT = d_mu; s.sigmaT = d_sigma; s.alphaT = d_alpha;
    s.gradx = d_gradx; s.drow = d_drow;
    for (int j = 0; j < n; ++j) s.qf[j] = a->qf[j];
    s.A = d_A;
    s.seds = d_seds; s.seds_G = a->seds_G; s.seds_lin_thr = a->seds_lin_thr; s.seds_thr = a->seds_thr;
    s.frame = a->frame ? 1 : 0; s.frame_max = a->frame_max; s.hzVel = d_vel; s.ldVel = a->ldVel; s.rowObs = d_rowObs;
    s.prm = a->prm;
    if (a->nsub == 1) omds_launch_modulate(0, s);
    else if (n == 2) launch_modulate16_t<2>(s);
    else launch_modulate16_t<7>(s);
    HCK(hipGetLastError());
    HCK(hipDeviceSynchronize());
    HCK(hipMemcpy(a->q_next, d_traj + (size_t)i * n * N, n_nN * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->qdot, d_qdot, n_nN * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->dist, d_dist + (size_t)(i - 1) * N, (size_t)N * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->dot, d_dot + (size_t)(i - 1) * N, (size_t)N * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->act, d_act + (size_t)(i - 1) * N, (size_t)N * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->normal, d_normal + (size_t)(i - 1) * n * N, n_nN * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->kval, d_kval + (size_t)(i - 1) * Kmax * N, n_KN * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->maxact, d_maxact, n_KN * F, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(a->phisum0, d_phisum0, (size_t)Kmax * F, hipMemcpyDeviceToHost));
done:
    for (void* p : {(void*)d_traj, (void*)d_dist, (void*)d_dot, (void*)d_act, (void*)d_normal, (void*)d_kval, (void*)d_qdot, (void*)d_maxact,
                    (void*)d_phisum0, (void*)d_mu, (void*)d_sigma, (void*)d_alpha, (void*)d_gradx, (void*)d_drow, (void*)d_A, (void*)d_seds,
                    (void*)d_vel, (void*)d_rowObs})
        if (p) (void)hipFree(p);
    return rc;
}
#undef HCK
