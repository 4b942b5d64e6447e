// Stand-alone host build of the sphere-velocity definition (optimalmodulationds_amd/csrc/point_cloud_flow_def.h: the body of
// omds_point_cloud_flow) for tests/test_cloud_flow_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on its
// cases: the header's functions are the ones the library and its kernels use, only the compiler differs.
//   cloud_flow_host IN OUT
// IN : int32 n_cases, then per case: omds_cloud_spec (raw), omds_cloud_track_spec (raw), int64 n_prev, int64 n_now, int32 cap,
//      int32 null_mask (1: spec, 2: track, 4: xyz_prev, 8: xyz_now, 16: xyzr_out, 32: vel_out, 64: count_out, 128: matched_out NULL),
//      float xyz_prev[n_prev][3], float xyz_now[n_now][3]
// OUT: per case: int32 rc, int32 count, int32 matched, int32 written, float xyzr[written][4], float vel[written][3]
//      (written = count when rc == 0, else 0)
// Every array is allocated at exactly the size passed, so that a write or read past one is the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/point_cloud_flow_def.h"

extern "C" int omds_point_cloud_flow(const omds_cloud_spec* spec, const omds_cloud_track_spec* track, const float* xyz_prev, int64_t n_prev,
                                     const float* xyz_now, int64_t n_now, float* xyzr_out, float* vel_out, int32_t cap, int32_t* count_out,
                                     int32_t* matched_out) {
    std::string err;
    return cloud_flow_host(spec, track, xyz_prev, n_prev, xyz_now, n_now, xyzr_out, vel_out, cap, count_out, matched_out, &err);
}

int main(int argc, char** argv) {
    return run_cases(argc, argv, "cloud_flow_host", [](FILE* in, FILE* out) {
        omds_cloud_spec spec;
        omds_cloud_track_spec track;
        int64_t n_prev = 0, n_now = 0;
        int32_t cap = 0, null_mask = 0;
        if (!get(in, &spec) || !get(in, &track) || !get(in, &n_prev) || !get(in, &n_now) || !get(in, &cap) || !get(in, &null_mask)) return false;
        const size_t sp = n_prev > 0 ? (size_t)n_prev : 0, sn = n_now > 0 ? (size_t)n_now : 0, sc = cap > 0 ? (size_t)cap : 0;
        float* prev = exactly<float>(sp * 3);
        float* now = exactly<float>(sn * 3);
        float* xyzr = exactly<float>(sc * 4);
        float* vel = exactly<float>(sc * 3);
        if ((sp && !get(in, prev, sp * 3)) || (sn && !get(in, now, sn * 3))) return false;
        int32_t count = -1, matched = -1;
        const int rc = omds_point_cloud_flow((null_mask & 1) ? nullptr : &spec, (null_mask & 2) ? nullptr : &track, (null_mask & 4) ? nullptr : prev,
                                             n_prev, (null_mask & 8) ? nullptr : now, n_now, (null_mask & 16) ? nullptr : xyzr,
                                             (null_mask & 32) ? nullptr : vel, cap, (null_mask & 64) ? nullptr : &count,
                                             (null_mask & 128) ? nullptr : &matched);
        const int32_t head[4] = {rc, count, matched, rc == 0 ? count : 0};
        fwrite(head, 4, 4, out);
        if (head[3] > 0) {
            fwrite(xyzr, 16, (size_t)head[3], out);
            fwrite(vel, 12, (size_t)head[3], out);
        }
        free(prev);
        free(now);
        free(xyzr);
        free(vel);
        return true;
    });
}
