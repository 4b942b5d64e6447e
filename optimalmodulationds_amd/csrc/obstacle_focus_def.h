// The DEFINITION of the obstacle focus (omds.h: omds_obstacle_focus_select), stated once for the host entry point, the kernels of
// obstacle_focus_kernels.hip and the stand-alone host build of tests/obstacle_focus_host.cpp.  Nothing here needs a HIP header: every
// function is plain fp32 arithmetic in which each operation named in omds.h is one rounding (the translation units that include this
// are compiled without contraction across statements, csrc/Makefile), and integer work on the bits of a float.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "omds.h"

#if defined(__HIPCC__)
#define OMDS_FOCUS_FN __host__ __device__ inline
#else
#define OMDS_FOCUS_FN inline
#endif

// an omds_obstacle_focus_spec behind its checks
struct FocusRule {
    float margin;       // >= 0, or +inf
    float lookahead;    // >= 0, finite
    int max_keep;       // 0: no cap, else >= n_closest
    bool all_pass;      // margin == +inf
};

inline int focus_resolve_spec(const omds_obstacle_focus_spec* s, int n_closest, FocusRule* r, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!s) return fail("obstacle focus: null spec");
    if (!(s->margin >= 0.f)) return fail("obstacle focus: margin must be >= 0 or +inf");
    if (!(s->lookahead >= 0.f) || !std::isfinite(s->lookahead)) return fail("obstacle focus: lookahead must be finite and >= 0");
    if (s->max_keep >= 1 && s->max_keep < n_closest) return fail("obstacle focus: max_keep below n_closest (< 1 is no cap)");
    r->margin = s->margin;
    r->lookahead = s->lookahead;
    r->max_keep = s->max_keep < 1 ? 0 : s->max_keep;
    r->all_pass = std::isinf(s->margin);
    return OMDS_OK;
}

OMDS_FOCUS_FN uint32_t focus_bits(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}
OMDS_FOCUS_FN float focus_float(uint32_t b) {
    float x;
    memcpy(&x, &b, 4);
    return x;
}

// the reach of a sphere at distance d that moves at (vx, vy, vz): the distance it can have after lookahead seconds of approaching
OMDS_FOCUS_FN float focus_reach(float d, float vx, float vy, float vz, float lookahead) {
    const float s2 = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
    const float speed = sqrtf(s2);
    return fmaf(-speed, lookahead, d);
}

// The key of a reach: an unsigned integer whose order is the fp32 order of the reaches, NaN as -inf and -0 as +0.  Everything the
// selection compares is a key: a < b, a == b, a <= b on reaches (NaN counted as -inf) are the same comparisons on their keys
OMDS_FOCUS_FN uint32_t focus_key(float r) {
    uint32_t b = focus_bits(r);
    if ((b & 0x7fffffffu) > 0x7f800000u) b = 0xff800000u;   // NaN -> -inf
    if (b == 0x80000000u) b = 0u;                           // -0 -> +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// ... and back: the reach a key stands for (-inf for the key of a NaN)
OMDS_FOCUS_FN float focus_key_value(uint32_t key) { return focus_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// the key every passing sphere's key is at most: that of bar = t + margin, t the reach of the n_closest-th sphere of the order
OMDS_FOCUS_FN uint32_t focus_bar_key(uint32_t kth_key, float margin) { return focus_key(focus_key_value(kth_key) + margin); }

// omds_obstacle_focus_select without its argument messages
inline int focus_select_host(const omds_obstacle_focus_spec* spec, const float* d, const float* vel, int n_obs, int n_closest, int32_t* idx_out,
                             int32_t cap, int32_t* kept_out, int32_t* passed_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    FocusRule r;
    if (n_closest < 1) return fail("omds_obstacle_focus_select: need n_closest >= 1");
    if (int rc = focus_resolve_spec(spec, n_closest, &r, err)) return rc;
    if (n_obs < n_closest) return fail("omds_obstacle_focus_select: fewer spheres than n_closest");
    if (!d || !idx_out || !kept_out || !passed_out || cap < 0) return fail("omds_obstacle_focus_select: need non-null d [O], idx_out [cap], kept_out, passed_out and cap >= 0");
    std::vector<std::pair<uint32_t, int32_t>> order((size_t)n_obs);   // (key, index): the order of the definition is the order of the pairs
    for (int o = 0; o < n_obs; ++o) {
        const float reach = vel ? focus_reach(d[o], vel[3 * (size_t)o], vel[3 * (size_t)o + 1], vel[3 * (size_t)o + 2], r.lookahead) : d[o];
        order[(size_t)o] = {focus_key(reach), o};
    }
    std::sort(order.begin(), order.end());
    int64_t passed = n_obs;
    if (!r.all_pass) {
        const uint32_t bar = focus_bar_key(order[(size_t)n_closest - 1].first, r.margin);
        passed = std::upper_bound(order.begin(), order.end(), std::make_pair(bar, INT32_MAX)) - order.begin();
    }
    const int64_t kept = r.max_keep ? std::min<int64_t>(passed, r.max_keep) : passed;
    *kept_out = (int32_t)kept;
    *passed_out = (int32_t)passed;
    if (cap < kept) return fail("omds_obstacle_focus_select: cap is smaller than the kept set (kept_out holds its size); idx_out is untouched");
    for (int64_t i = 0; i < kept; ++i) idx_out[i] = order[(size_t)i].second;
    std::sort(idx_out, idx_out + kept);
    return OMDS_OK;
}
