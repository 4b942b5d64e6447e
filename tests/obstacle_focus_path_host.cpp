// Stand-alone host build of the definition of the obstacle focus along a path (optimalmodulationds_amd/csrc/obstacle_focus_def.h: the
// body of omds_obstacle_focus_select_path) for tests/test_obstacle_focus_path_cpu.py, which compiles it with g++
// -fsanitize=address,undefined and runs it on its cases: the header's functions are the ones the library and its kernels use, only the
// compiler differs.
//   obstacle_focus_path_host IN OUT
// IN : int32 n_cases, then per case: omds_obstacle_focus_spec (raw), int32 n_states, int32 n_obs, int32 n_closest, int32 cap,
//      int32 have_ahead, int32 have_vel, int32 null_mask (1: spec NULL, 2: d NULL, 4: idx_out NULL, 8: kept_out NULL, 16: passed_out
//      NULL), float d[n_states][n_obs], float ahead[n_states] when have_ahead, float vel[n_obs][3] when have_vel
// OUT: per case: int32 rc, int32 kept, int32 passed, int32 written, int32 idx[written]   (written = kept when rc == 0, else 0)
// d, ahead, vel and idx_out are allocated at exactly the sizes passed, so that a read or write past either is the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/obstacle_focus_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "obstacle_focus_path_host", [](FILE* in, FILE* out) {
        omds_obstacle_focus_spec spec;
        int32_t n_states = 0, n_obs = 0, n_closest = 0, cap = 0, have_ahead = 0, have_vel = 0, null_mask = 0;
        if (!get(in, &spec) || !get(in, &n_states) || !get(in, &n_obs) || !get(in, &n_closest) || !get(in, &cap) || !get(in, &have_ahead) ||
            !get(in, &have_vel) || !get(in, &null_mask))
            return false;
        const size_t O = n_obs > 0 ? (size_t)n_obs : 0, B = n_states > 0 ? (size_t)n_states : 0;
        float* d = exactly<float>(B * O);
        float* ahead = have_ahead ? exactly<float>(B) : nullptr;
        float* vel = have_vel ? exactly<float>(O * 3) : nullptr;
        int32_t* idx = exactly<int32_t>(cap > 0 ? (size_t)cap : 0);
        if (B * O && !get(in, d, B * O)) return false;
        if (ahead && B && !get(in, ahead, B)) return false;
        if (vel && O && !get(in, vel, O * 3)) return false;
        int32_t kept = -1, passed = -1;
        std::string err;
        const int rc = focus_select_path_host((null_mask & 1) ? nullptr : &spec, (null_mask & 2) ? nullptr : d, ahead, vel, n_states, n_obs, n_closest,
                                              (null_mask & 4) ? nullptr : idx, cap, (null_mask & 8) ? nullptr : &kept,
                                              (null_mask & 16) ? nullptr : &passed, &err);
        const int32_t head[4] = {rc, kept, passed, rc == 0 ? kept : 0};
        fwrite(head, 4, 4, out);
        if (head[3] > 0) fwrite(idx, 4, (size_t)head[3], out);
        free(d);
        free(ahead);
        free(vel);
        free(idx);
        return true;
    });
}
