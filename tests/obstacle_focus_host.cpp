// Stand-alone host build of the obstacle-focus definition (optimalmodulationds_amd/csrc/obstacle_focus_def.h: the body of
// omds_obstacle_focus_select) for tests/test_obstacle_focus_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it
// on its cases: the header's functions are the ones the library and its kernels use, only the compiler differs.
//   obstacle_focus_host IN OUT
// IN : int32 n_cases, then per case: omds_obstacle_focus_spec (raw), int32 n_obs, int32 n_closest, int32 cap, int32 have_vel,
//      int32 null_mask (1: spec NULL, 2: d NULL, 4: idx_out NULL, 8: kept_out NULL, 16: passed_out NULL), float d[n_obs],
//      float vel[n_obs][3] when have_vel
// OUT: per case: int32 rc, int32 kept, int32 passed, int32 written, int32 idx[written]   (written = kept when rc == 0, else 0)
// d, vel and idx_out are allocated at exactly the sizes passed, so that a read or write past either is the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/obstacle_focus_def.h"

extern "C" int omds_obstacle_focus_select(const omds_obstacle_focus_spec* spec, const float* d, const float* vel, int n_obs, int n_closest,
                                          int32_t* idx_out, int32_t cap, int32_t* kept_out, int32_t* passed_out) {
    std::string err;
    return focus_select_host(spec, d, vel, n_obs, n_closest, idx_out, cap, kept_out, passed_out, &err);
}

int main(int argc, char** argv) {
    return run_cases(argc, argv, "obstacle_focus_host", [](FILE* in, FILE* out) {
        omds_obstacle_focus_spec spec;
        int32_t n_obs = 0, n_closest = 0, cap = 0, have_vel = 0, null_mask = 0;
        if (!get(in, &spec) || !get(in, &n_obs) || !get(in, &n_closest) || !get(in, &cap) || !get(in, &have_vel) || !get(in, &null_mask)) return false;
        const size_t stored = n_obs > 0 ? (size_t)n_obs : 0;
        float* d = exactly<float>(stored);
        float* vel = have_vel ? exactly<float>(stored * 3) : nullptr;
        int32_t* idx = exactly<int32_t>(cap > 0 ? (size_t)cap : 0);
        if (stored && !get(in, d, stored)) return false;
        if (vel && stored && !get(in, vel, stored * 3)) return false;
        int32_t kept = -1, passed = -1;
        const int rc = omds_obstacle_focus_select((null_mask & 1) ? nullptr : &spec, (null_mask & 2) ? nullptr : d, vel, n_obs, n_closest,
                                                  (null_mask & 4) ? nullptr : idx, cap, (null_mask & 8) ? nullptr : &kept,
                                                  (null_mask & 16) ? nullptr : &passed);
        const int32_t head[4] = {rc, kept, passed, rc == 0 ? kept : 0};
        fwrite(head, 4, 4, out);
        if (head[3] > 0) fwrite(idx, 4, (size_t)head[3], out);
        free(d);
        free(vel);
        free(idx);
        return true;
    });
}
