// The ending of a fused horizon step, once for k_tail, k_tail_sel (tail_kernel.hip) and k_step_small (step_small.hip): the modulation /
// policy / Euler step of the workgroup's rollouts on the gradients and distances its backward left in LDS, and the encoded joint
// inputs [q, sin q, cos q] of the NEXT step.  The kernels keep what lies between the two halves: their timeline stamps, the
// `step >= H` return (last step: nothing is integrated, no next network evaluation) and the barrier.
// One source for the three kernels is one arithmetic (-ffp-contract=on, Makefile): their steps are each other's bits.
#pragma once
#include "step_device.h"
#include "trig_device.h"

// 16 lanes per rollout: rollout rl = tid / 16 of the workgroup's RW (t = t_base + rl < N), state q = qT[j * ldq + t], gradient rows
// rl * k .. + k - 1 of gx / dr, their obstacles in rowObs (LDS).  feat [RW][3 ND] receives (q_next, sin, cos).  FqH != nullptr (a
// screened step; a literal nullptr folds the branch away): the same three, rounded to fp16, go to the screening kernel's input row of
// the rollout, of row capacity ldF -- unless this is the last step.
template <int ND, bool FRAME>
__device__ __forceinline__ void step_advance(const StepArgs& st, const MlpDev& m, const float* qT, int ldq, int N, int t_base, int RW, int k,
                                             const float* gx, const float* dr, const int* rowObs, float* feat, _Float16* FqH, int ldF) {
    const int tid = threadIdx.x;
    const int rl = tid >> 4, sub = tid & 15;
    const int t = t_base + rl;
    if (rl < RW && t < N) {
        float q[ND], qn[ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) q[j] = qT[(size_t)j * ldq + t];
        modulate_core<ND, 16, false, FRAME>(st, st.step, t, sub, gx, dr, rl * k, q, qn, rowObs);
        if (sub < ND) {
            float v = qn[0];
#pragma unroll
            for (int j = 1; j < ND; ++j) v = (sub == j) ? qn[j] : v;
            feat[rl * 3 * ND + sub] = v;
            feat[rl * 3 * ND + ND + sub] = omds_sinf(v);
            feat[rl * 3 * ND + 2 * ND + sub] = omds_cosf(v);
            if (FqH && st.step < st.H)   // (m.scrQ: skip-connection networks, the concatenation operand of the screening kernel)
                omds_screen_store_row(FqH, reinterpret_cast<_Float16*>(m.scrQ), sub, m.d, t, ldF, v, feat[rl * 3 * ND + ND + sub],
                                      feat[rl * 3 * ND + 2 * ND + sub]);
        }
    }
}

// the encoded joint inputs of the next step (as k_rollout_features writes them) from feat, by a workgroup of NT threads
template <int ND, int NT>
__device__ __forceinline__ void step_write_next_rows(float* FqOut, const float* feat, int d, int N, int t_base, int RW) {
    const int tid = threadIdx.x;
    for (int e = tid; e < RW * 3 * ND; e += NT) {
        const int rl = e / (3 * ND), cc = e - rl * (3 * ND), part = cc / ND, t = t_base + rl;
        if (t < N) FqOut[(size_t)t * OMDS_FROW + part * d + (cc - part * ND)] = feat[e];
    }
}
