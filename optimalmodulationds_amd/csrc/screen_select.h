// The candidate selection of the screened step (device): from a rollout's O screening values to its entries of the candidate list and
// its share of the audit sample.  Included by screen_kernel.hip (k_screen's flush phase, k_select) and screen_stats.hip (the hash of
// the calibration states, the candidate rule of the sweep statistics).
#pragma once
#include "mfma_gemm.h"

// lowbias32 (an integer hash with good avalanche): which non-candidate pairs enter the audit sample
__device__ __forceinline__ unsigned omds_audit_hash(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// The candidate rule: everything not above tau, and every non-finite value (NaN / +inf = an fp16 overflow inside the network:
// nothing is known about such a row).
__device__ __forceinline__ bool screen_is_candidate(float x, float tau) { return !(x > tau) || !(x < __builtin_inff()); }

// wave-wide minimum of a float, result uniform over the wave (NaN never wins: v_min_f32 returns the other operand): four DPP
// steps inside each row of 16 lanes (row16_min_f32, the link minimum of pass 1), then the four rows meet through SGPRs --
// ~10 instructions where a __shfl_xor butterfly is 6 dependent ds_bpermute round trips
__device__ __forceinline__ float wave_min_f32(float v) {
    v = row16_min_f32(v);
    const int iv = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return fminf(fminf(r0, r1), fminf(r2, r3));
}
// number of set bits of a wave mask below this lane
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// One wave = one rollout: from the rollout's O screening values (row: global memory or LDS) to its candidates in the list
// and its share of the audit sample.  All SEL_WAVES waves of the workgroup call it together (two barriers inside: ONE atomic on
// the list counter per workgroup -- 1024 same-address atomics, one per rollout, serialise in L2 and were half of the first
// k_select); `live` = this wave has a rollout.  Everything cross-lane is a ballot or a DPP step: this runs in the flush phase
// of k_screen, on the critical path of every horizon step, and a shuffle-based version took 9 us there.
// Each of the three passes -- the k-th smallest value, the counts, the scatter -- is written twice, for "values in registers" and for
// "values re-read": stated once over a row view they were 101-126 instructions more in every k_screen (EXPERIMENTS.md R26).
struct SelectShared { int wtot[SEL_WAVES], watot[SEL_WAVES], wbase, wabase; };
template <typename RowPtr>
__device__ __forceinline__ void select_rollout(const SelectSink& a, SelectShared& sh, RowPtr row, int t, bool live, int O, int lane, int wave) {
    constexpr int NV = 8;
    float v[NV];
    const bool in_regs = O <= 64 * NV;   // rows of up to 512 values sit in registers; longer rows are re-read
    if (in_regs) {
#pragma unroll
        for (int i = 0; i < NV; ++i) { const int o = lane + 64 * i; v[i] = (o < O) ? row[o] : __builtin_nanf(""); }   // NaN padding never wins a minimum
    }
    // k-th smallest value, multiplicities counted: at most k rounds of "smallest value above the previous one, and how many
    // entries hold it".  NaN entries (an fp16 overflow inside the network) never win a round; they are made candidates below.
    float kth = __builtin_inff(), prev = 0.f;
    int remaining = a.k;
    for (int round = 0; round < a.k; ++round) {
        float loc = __builtin_inff();
        if (in_regs) {
#pragma unroll
            for (int i = 0; i < NV; ++i) loc = (round == 0 || v[i] > prev) ? fminf(loc, v[i]) : loc;
        } else {
            for (int o = lane; o < O; o += 64) { const float x = row[o]; loc = (round == 0 || x > prev) ? fminf(loc, x) : loc; }
        }
        const float m = wave_min_f32(loc);
        int c = 0;
        if (in_regs) {
#pragma unroll
            for (int i = 0; i < NV; ++i) c += __popcll(__ballot(v[i] == m));
        } else {
            for (int o0 = 0; o0 < O; o0 += 64) { const int o = o0 + lane; c += __popcll(__ballot(o < O && row[o] == m)); }
        }
        kth = m;
        if (c >= remaining || !(m < __builtin_inff())) break;   // +inf: fewer than k finite values -- everything becomes a candidate
        remaining -= c;
        prev = m;
    }
    const float tau = kth + a.delta;
    // Candidates: screen_is_candidate.  AUDIT sample: a pseudo-random subset of the pairs that are NOT candidates -- the
    // population the selection rule makes an assumption about (screening error <= eps) -- goes with its screening value into
    // the propagate's audit list; k_audit evaluates those pairs in fp32 once the horizon loop is done.
    const int rbase = t * O;
    const bool auditing = a.audit_mask != 0xffffffffu;
    auto is_audit = [&](int o) { return auditing && (omds_audit_hash((unsigned)(rbase + o) ^ a.audit_seed) & a.audit_mask) == 0u; };
    // one ballot pair per group of 64 obstacles: totals are scalar popcounts, a lane's list position is the number of set bits
    // below it -- no scans, no shuffles.  (The order of a rollout's entries in the list is group-major; nothing depends on it.)
    unsigned long long cm[NV], am[NV];
    int wave_total = 0, wave_audit = 0;
    if (in_regs) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int o = lane + 64 * i;
            const bool c = o < O && screen_is_candidate(v[i], tau);
            cm[i] = __ballot(c);
            am[i] = __ballot(o < O && !c && is_audit(o));
            wave_total += __popcll(cm[i]);
            wave_audit += __popcll(am[i]);
        }
    } else {
        for (int o0 = 0; o0 < O; o0 += 64) {
            const int o = o0 + lane;
            const bool c = o < O && screen_is_candidate(row[o], tau);
            wave_total += __popcll(__ballot(c));
            wave_audit += __popcll(__ballot(o < O && !c && is_audit(o)));
        }
    }
    if (!live) { wave_total = 0; wave_audit = 0; }
    if (lane == 0) { sh.wtot[wave] = wave_total; sh.watot[wave] = wave_audit; }
    __syncthreads();
    // the two list counters are bumped by two different waves at once: their L2 round trips overlap
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) sum += sh.wtot[w];
        sh.wbase = atomicAdd(a.total, sum);
    } else if (threadIdx.x == 64) {
        int asum = 0;
#pragma unroll
        for (int w = 0; w < SEL_WAVES; ++w) asum += sh.watot[w];
        sh.wabase = asum ? atomicAdd(a.audit_total, asum) : 0;
    }
    __syncthreads();
    if (live) {
        int base = sh.wbase, abase = sh.wabase;
        for (int w = 0; w < wave; ++w) { base += sh.wtot[w]; abase += sh.watot[w]; }
        if (lane == 0) {
            a.range[4 * t] = base;
            a.range[4 * t + 1] = wave_total;
            a.range[4 * t + 2] = __builtin_bit_cast(int, tau);   // k_tail_sel checks the rollout's slack against it
        }
        const int arow0 = (a.step_row0 + t) * O;
        if (in_regs) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int o = lane + 64 * i;
                if ((cm[i] >> lane) & 1ull) {
                    const int pos = base + lanes_below(cm[i]);
                    a.rowlist[pos] = rbase + o;
                    if (a.listDa) a.listDa[pos] = v[i];
                } else if ((am[i] >> lane) & 1ull) {
                    const int apos = abase + lanes_below(am[i]);
                    if (apos < a.audit_cap) { a.audit_rows[apos] = arow0 + o; a.audit_da[apos] = v[i]; }
                }
                base += __popcll(cm[i]);
                abase += __popcll(am[i]);
            }
        } else {
            for (int o0 = 0; o0 < O; o0 += 64) {
                const int o = o0 + lane;
                const float x = o < O ? row[o] : 0.f;
                const bool c = o < O && screen_is_candidate(x, tau), au = o < O && !c && is_audit(o);
                const unsigned long long cmk = __ballot(c), amk = __ballot(au);
                if (c) {
                    const int pos = base + lanes_below(cmk);
                    a.rowlist[pos] = rbase + o;
                    if (a.listDa) a.listDa[pos] = x;
                } else if (au) {
                    const int apos = abase + lanes_below(amk);
                    if (apos < a.audit_cap) { a.audit_rows[apos] = arow0 + o; a.audit_da[apos] = x; }
                }
                base += __popcll(cmk);
                abase += __popcll(amk);
            }
        }
    }
    __syncthreads();   // the shared counters are reused by the workgroup's next round of rollouts
}
