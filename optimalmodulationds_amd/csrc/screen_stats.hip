// The screening's diagnostic kernels (gfx950): the states the error bound is calibrated on, the largest difference of two arrays, and
// the sweep histograms.  None of them runs inside a screened step (screening.hip calls their launchers).
#include <algorithm>

#include "pass1_tile.h"   // OmdsDivisor
#include "screen_select.h"

// Calibration of the screening bound on the device (screening.hip: calibrate_screen): B states -- the even ones uniform inside the
// joint box, the odd ones drawn from the rollouts of the last propagate (where the next rollouts will live), or scattered
// around the start state while there are none yet -- and the largest |screening value - fp32 value| over their B x O pairs.
struct CalibArgs {
    float* qT;             // [n][B] out
    int B, n;
    float lo[OMDS_MAX_DOF], hi[OMDS_MAX_DOF], center[OMDS_MAX_DOF];
    const float* trajT;    // [H][n][N] rollouts of the last propagate, or nullptr
    int N, H;
    unsigned seed;
};
__global__ __launch_bounds__(256) void k_calib_states(CalibArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.B) return;
    auto uni = [&](unsigned salt) { return ((omds_audit_hash((unsigned)t * 0x9E3779B1u + salt + a.seed) >> 8) + 0.5f) * (1.f / 16777216.f); };
    if ((t & 1) && a.trajT) {
        const unsigned r = omds_audit_hash((unsigned)t + 0x51ED270Bu * a.seed);
        const int tt = (int)(r % (unsigned)a.N), hh = (int)((r >> 16) % (unsigned)a.H);
        for (int j = 0; j < a.n; ++j) a.qT[(size_t)j * a.B + t] = a.trajT[((size_t)hh * a.n + j) * a.N + tt];
        return;
    }
    for (int j = 0; j < a.n; ++j) {
        float v;
        if (t & 1) {   // Box-Muller scatter (sigma 0.6 rad) around the start state, clamped to the box
            const float g = sqrtf(-2.f * logf(uni(2 * j + 1))) * cosf(6.2831853f * uni(2 * j + 2));
            v = fminf(a.hi[j], fmaxf(a.lo[j], a.center[j] + 0.6f * g));
        } else {
            v = a.lo[j] + (a.hi[j] - a.lo[j]) * uni(2 * j + 1);
        }
        a.qT[(size_t)j * a.B + t] = v;
    }
}
void omds_launch_calib_states(hipStream_t s, float* qT, int B, int n, const float* lo, const float* hi, const float* center,
                              const float* trajT, int N, int H, unsigned seed) {
    CalibArgs a;
    a.qT = qT; a.B = B; a.n = n; a.trajT = trajT; a.N = N; a.H = H; a.seed = seed;
    for (int j = 0; j < OMDS_MAX_DOF; ++j) { a.lo[j] = j < n ? lo[j] : 0.f; a.hi[j] = j < n ? hi[j] : 0.f; a.center[j] = j < n ? center[j] : 0.f; }
    hipLaunchKernelGGL(k_calib_states, dim3((B + 255) / 256), dim3(256), 0, s, a);
}
// *out_bits = max(*out_bits, max_i |x[i] - y[i]|) as float bits; a non-finite difference counts as +inf
__global__ __launch_bounds__(256) void k_max_abs_diff(const float* __restrict__ x, const float* __restrict__ y, long long n, unsigned* out_bits) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float e = fabsf(x[i] - y[i]);
        if (!(e <= m)) m = (e < __builtin_inff()) ? e : __builtin_inff();
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out_bits, __builtin_bit_cast(unsigned, m));
}
void omds_launch_max_abs_diff(hipStream_t s, const float* x, const float* y, long long n, unsigned* out_bits) {
    if (n <= 0) return;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_max_abs_diff, dim3(grid), dim3(256), 0, s, x, y, n, out_bits);
}

// Sweep statistics (omds.h, omds_screen_sweep_hist): one step's N x O screening values Da beside its N x O fp32 values D and the
// tau of every rollout (range[4 t + 2], what the selection of that step used).  x = Da - D over the pairs that are NOT candidates
// -- the population the selection rule's assumption "x <= eps" is about -- goes into histograms; max |x| over ALL pairs into
// *maxabs_bits (a non-finite difference counts as +inf) like k_max_abs_diff.  Counters are 64-bit and accumulate across launches.
__global__ __launch_bounds__(256) void k_sweep_hist(const float* __restrict__ D, const float* __restrict__ Da, const int* __restrict__ range,
                                                    int N, int O, OmdsDivisor od, float eps, unsigned long long* __restrict__ hist, unsigned* maxabs_bits) {
    __shared__ unsigned bins[OMDS_HIST_LOG_BINS * 2 + OMDS_HIST_RATIO_BINS];
    __shared__ unsigned cnt[8];
    for (int i = threadIdx.x; i < OMDS_HIST_LOG_BINS * 2 + OMDS_HIST_RATIO_BINS; i += blockDim.x) bins[i] = 0;
    if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long total = (long long)N * O;
    float mabs = 0.f, mpos = 0.f;
    unsigned n_all = 0, n_non = 0, n_half = 0, n_eps = 0, n_bad = 0;
    const float inv_eps = eps > 0.f ? 1.f / eps : 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float d = D[i], da = Da[i];
        const int t = (int)od.div((unsigned)i);
        const float tau = __builtin_bit_cast(float, range[4 * t + 2]);
        const float x = da - d, e = fabsf(x);
        ++n_all;
        if (!(e <= mabs)) mabs = (e < __builtin_inff()) ? e : __builtin_inff();
        if (screen_is_candidate(da, tau)) continue;
        ++n_non;
        if (!(e < __builtin_inff())) { ++n_bad; continue; }          // a finite Da beside a non-finite D: cannot happen with finite weights
        if (x > mpos) mpos = x;
        if (x > 0.5f * eps) ++n_half;
        if (x > eps) ++n_eps;
        // log2 bins: bin b holds 2^(b - OMDS_HIST_LOG_BINS) <= |x| < 2^(b + 1 - OMDS_HIST_LOG_BINS); bin 0 also everything smaller
        // (zero included), the last bin everything >= 1/2
        int b = (e > 0.f ? ilogbf(e) : -1000) + OMDS_HIST_LOG_BINS;
        b = b < 0 ? 0 : (b > OMDS_HIST_LOG_BINS - 1 ? OMDS_HIST_LOG_BINS - 1 : b);
        atomicAdd(&bins[(x < 0.f ? OMDS_HIST_LOG_BINS : 0) + b], 1u);
        if (x > 0.f) {   // x / eps in OMDS_HIST_RATIO_BINS linear bins over [0, 1); the last bin also everything >= 1
            int r = (int)(x * inv_eps * OMDS_HIST_RATIO_BINS);
            r = r > OMDS_HIST_RATIO_BINS - 1 ? OMDS_HIST_RATIO_BINS - 1 : r;
            atomicAdd(&bins[2 * OMDS_HIST_LOG_BINS + r], 1u);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { mabs = fmaxf(mabs, __shfl_xor(mabs, off)); mpos = fmaxf(mpos, __shfl_xor(mpos, off)); }
    atomicAdd(&cnt[0], n_all); atomicAdd(&cnt[1], n_non); atomicAdd(&cnt[2], n_half); atomicAdd(&cnt[3], n_eps); atomicAdd(&cnt[4], n_bad);
    if ((threadIdx.x & 63) == 0) {
        if (mabs > 0.f) atomicMax(maxabs_bits, __builtin_bit_cast(unsigned, mabs));
        if (mpos > 0.f) atomicMax(&hist[OMDS_HIST_MAX_POS], (unsigned long long)__builtin_bit_cast(unsigned, mpos));
        if (mabs > 0.f) atomicMax(&hist[OMDS_HIST_MAX_ABS], (unsigned long long)__builtin_bit_cast(unsigned, mabs));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&hist[OMDS_HIST_PAIRS], (unsigned long long)cnt[0]);
        atomicAdd(&hist[OMDS_HIST_NONCAND], (unsigned long long)cnt[1]);
        atomicAdd(&hist[OMDS_HIST_ABOVE_HALF], (unsigned long long)cnt[2]);
        atomicAdd(&hist[OMDS_HIST_ABOVE_EPS], (unsigned long long)cnt[3]);
        atomicAdd(&hist[OMDS_HIST_NONFINITE], (unsigned long long)cnt[4]);
    }
    for (int i = threadIdx.x; i < OMDS_HIST_LOG_BINS * 2 + OMDS_HIST_RATIO_BINS; i += blockDim.x)
        if (bins[i]) atomicAdd(&hist[OMDS_HIST_BINS0 + i], (unsigned long long)bins[i]);
}
void omds_launch_sweep_hist(hipStream_t s, const float* D, const float* Da, const int* range, int N, int O, float eps,
                            unsigned long long* hist, unsigned* maxabs_bits) {
    const long long n = (long long)N * O;
    if (n <= 0) return;
    const unsigned grid = (unsigned)std::min<long long>((n + 2047) / 2048, 512);   // few workgroups: each ends with ~200 64-bit atomics
    hipLaunchKernelGGL(k_sweep_hist, dim3(grid), dim3(256), 0, s, D, Da, range, N, O, OmdsDivisor::make((unsigned)O), eps, hist, maxabs_bits);
}
