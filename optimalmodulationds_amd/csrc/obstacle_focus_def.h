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
OMDS_FOCUS_FN float focus_speed(float vx, float vy, float vz) {
    const float s2 = fmaf(vz, vz, fmaf(vy, vy, vx * vx));
    return sqrtf(s2);
}
OMDS_FOCUS_FN float focus_reach(float d, float vx, float vy, float vz, float lookahead) {
    const float speed = focus_speed(vx, vy, vz);
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

// The time a sphere has to approach until state b of a path is reached: lookahead + ahead_b, one rounding
OMDS_FOCUS_FN float focus_path_time(float lookahead, float ahead) { return lookahead + ahead; }
inline bool focus_ahead_ok(float a) { return a >= 0.f && std::isfinite(a); }
// the word the final selection of a path orders by: the nearest key of a passing sphere, and for the others a word above every key
// (no key exceeds 0xff800000, that of +inf)
constexpr uint32_t FOCUS_NOT_PASSING = 0xffffffffu;

// omds_obstacle_focus_select_path without its argument messages: d [n_states][n_obs], ahead [n_states] or null.  Per state the keys
// of its row, the bar of its own n_closest-th key, and into per-sphere words an OR of "passes here" and a minimum of the keys: integer
// work whose result no order of the states changes
inline int focus_select_path_host(const omds_obstacle_focus_spec* spec, const float* d, const float* ahead, const float* vel, int n_states, int n_obs,
                                  int n_closest, int32_t* idx_out, int32_t cap, int32_t* kept_out, int32_t* passed_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    FocusRule r;
    if (n_closest < 1) return fail("omds_obstacle_focus_select_path: need n_closest >= 1");
    if (int rc = focus_resolve_spec(spec, n_closest, &r, err)) return rc;
    if (n_obs < n_closest) return fail("omds_obstacle_focus_select_path: fewer spheres than n_closest");
    if (n_states < 1) return fail("omds_obstacle_focus_select_path: need n_states >= 1");
    if (!d || !idx_out || !kept_out || !passed_out || cap < 0)
        return fail("omds_obstacle_focus_select_path: need non-null d [n_states][O], idx_out [cap], kept_out, passed_out and cap >= 0");
    if (ahead)
        for (int b = 0; b < n_states; ++b)
            if (!focus_ahead_ok(ahead[b])) return fail("omds_obstacle_focus_select_path: every ahead must be finite and >= 0");
    const size_t O = (size_t)n_obs;
    std::vector<float> speed(vel ? O : 0);
    for (size_t o = 0; o < speed.size(); ++o) speed[o] = focus_speed(vel[3 * o], vel[3 * o + 1], vel[3 * o + 2]);
    std::vector<uint32_t> best(O, FOCUS_NOT_PASSING), row(O), sorted(O);
    std::vector<unsigned char> pass(O, r.all_pass ? 1 : 0);
    for (int b = 0; b < n_states; ++b) {
        const float* db = d + (size_t)b * O;
        const float time = ahead ? focus_path_time(r.lookahead, ahead[b]) : r.lookahead;
        for (size_t o = 0; o < O; ++o) row[o] = focus_key(vel ? fmaf(-speed[o], time, db[o]) : db[o]);
        uint32_t bar = FOCUS_NOT_PASSING;
        if (!r.all_pass) {
            sorted = row;
            std::nth_element(sorted.begin(), sorted.begin() + (n_closest - 1), sorted.end());
            bar = focus_bar_key(sorted[(size_t)n_closest - 1], r.margin);
        }
        for (size_t o = 0; o < O; ++o) {
            pass[o] |= row[o] <= bar;
            best[o] = std::min(best[o], row[o]);
        }
    }
    std::vector<std::pair<uint32_t, int32_t>> order;   // (nearest key, index) of the passing spheres
    for (size_t o = 0; o < O; ++o)
        if (pass[o]) order.push_back({best[o], (int32_t)o});
    std::sort(order.begin(), order.end());
    const int64_t passed = (int64_t)order.size();
    const int64_t kept = r.max_keep ? std::min<int64_t>(passed, r.max_keep) : passed;
    *kept_out = (int32_t)kept;
    *passed_out = (int32_t)passed;
    if (cap < kept) return fail("omds_obstacle_focus_select_path: cap is smaller than the kept set (kept_out holds its size); idx_out is untouched");
    for (int64_t i = 0; i < kept; ++i) idx_out[i] = order[(size_t)i].second;
    std::sort(idx_out, idx_out + kept);
    return OMDS_OK;
}
