// Stand-alone host build of the velocity filter's definition (optimalmodulationds_amd/csrc/velocity_filter_def.h: the body of
// omds_velocity_filter_step) for tests/test_velocity_filter_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs
// it on its cases: the header's functions are the ones the library and its kernels use, only the compiler differs.
//   velocity_filter_host IN OUT
// IN : int32 n_cases, then per case: omds_cloud_spec (raw), omds_cloud_track_spec (raw), omds_velocity_filter_spec (raw), int32 n,
//      int32 cells (records the state arrays are allocated for), int32 have (1: state_in, 2: live, 4: group given),
//      int32 null_mask (1: spec, 2: track, 4: filt, 8: cell, 16: raw, 32: vel_out, 64: state_out NULL),
//      int32 state_in[cells][4] if given, int32 cell[n], float raw[n][3], int32 live[n] if given, int32 group[n] if given
// OUT: per case: int32 rc, int32 stats[3], int32 written, float vel[written][3], int32 state_out[cells][4] when rc == 0
//      (written = n when rc == 0, else 0)
// Every array is allocated at exactly the size passed, so that a write or read past one is the sanitizer's to report; the outputs
// are filled with a sentinel first, and a refused call must leave it everywhere.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/velocity_filter_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "velocity_filter_host", [](FILE* in, FILE* out) {
        omds_cloud_spec spec;
        omds_cloud_track_spec track;
        omds_velocity_filter_spec filt;
        int32_t n = 0, cells = 0, have = 0, null_mask = 0;
        if (!get(in, &spec) || !get(in, &track) || !get(in, &filt) || !get(in, &n) || !get(in, &cells) || !get(in, &have) || !get(in, &null_mask))
            return false;
        const size_t sn = n > 0 ? (size_t)n : 0, sc = cells > 0 ? (size_t)cells : 0;
        int32_t* state_in = exactly<int32_t>(sc * 4);
        int32_t* cell = exactly<int32_t>(sn);
        float* raw = exactly<float>(sn * 3);
        int32_t* live = exactly<int32_t>(sn);
        int32_t* group = exactly<int32_t>(sn);
        float* vel = exactly<float>(sn * 3);
        int32_t* state_out = exactly<int32_t>(sc * 4);
        if (((have & 1) && sc && !get(in, state_in, sc * 4)) || (sn && !get(in, cell, sn)) || (sn && !get(in, raw, sn * 3)) ||
            ((have & 2) && sn && !get(in, live, sn)) || ((have & 4) && sn && !get(in, group, sn)))
            return false;
        const float vel_mark = -7.f;
        const int32_t mark = -77;
        for (size_t i = 0; i < sn * 3; ++i) vel[i] = vel_mark;
        for (size_t i = 0; i < sc * 4; ++i) state_out[i] = mark;
        int32_t stats[3] = {mark, mark, mark};
        std::string err;
        const int rc = velocity_filter_step_host((null_mask & 1) ? nullptr : &spec, (null_mask & 2) ? nullptr : &track, (null_mask & 4) ? nullptr : &filt,
                                                 (have & 1) ? state_in : nullptr, (null_mask & 8) ? nullptr : cell, (null_mask & 16) ? nullptr : raw,
                                                 (have & 2) ? live : nullptr, (have & 4) ? group : nullptr, n, (null_mask & 32) ? nullptr : vel,
                                                 (null_mask & 64) ? nullptr : state_out, stats, &err);
        if (rc != 0) {   // a refusal writes nothing
            for (size_t i = 0; i < sn * 3; ++i)
                if (vel[i] != vel_mark) return false;
            for (size_t i = 0; i < sc * 4; ++i)
                if (state_out[i] != mark) return false;
            if (stats[0] != mark || stats[1] != mark || stats[2] != mark) return false;
        }
        const int32_t head[5] = {rc, stats[0], stats[1], stats[2], rc == 0 ? n : 0};
        fwrite(head, 4, 5, out);
        if (rc == 0) {
            if (sn) fwrite(vel, 12, sn, out);
            if (sc) fwrite(state_out, 16, sc, out);
        }
        free(state_in);
        free(cell);
        free(raw);
        free(live);
        free(group);
        free(vel);
        free(state_out);
        return true;
    });
}
