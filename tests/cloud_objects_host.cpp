// Stand-alone host build of the object-velocity definition (optimalmodulationds_amd/csrc/point_cloud_objects_def.h: the body of
// omds_point_cloud_object_flow) for tests/test_cloud_objects_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs
// it on its cases: the header's functions are the ones the library and its kernels use, only the compiler differs.
//   cloud_objects_host IN OUT
// IN : int32 n_cases, then per case: omds_cloud_spec, omds_cloud_track_spec, omds_cloud_object_spec (raw), int64 n_prev, int64 n_now,
//      int64 n_keep_prev, int64 n_keep_now (-1: NULL), int32 cap, int32 null_mask (bit 0: spec, 1: track, 2: obj, 3: xyz_prev,
//      4: xyz_now, 5: xyzr_out, 6: vel_out, 7: label_out, 8: object_out, 9: count_out, 10: matched_out, 11: n_objects_out,
//      12: n_objects_matched_out NULL), float xyz_prev[n_prev][3], float xyz_now[n_now][3], uint8 keep_prev[], uint8 keep_now[]
// OUT: per case: int32 rc, count, matched, n_objects, n_objects_matched, written, float xyzr[written][4], float vel[written][3],
//      int32 label[written], int32 object[written]   (written = kept cells when rc == 0, else 0)
// Every array is allocated at exactly the size passed, so that a write or read past one is the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/point_cloud_objects_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "cloud_objects_host", [](FILE* in, FILE* out) {
        omds_cloud_spec spec;
        omds_cloud_track_spec track;
        omds_cloud_object_spec obj;
        int64_t n_prev = 0, n_now = 0, n_kp = 0, n_kn = 0;
        int32_t cap = 0, mask = 0;
        if (!get(in, &spec) || !get(in, &track) || !get(in, &obj) || !get(in, &n_prev) || !get(in, &n_now) || !get(in, &n_kp) || !get(in, &n_kn) ||
            !get(in, &cap) || !get(in, &mask))
            return false;
        const size_t sp = n_prev > 0 ? (size_t)n_prev : 0, sn = n_now > 0 ? (size_t)n_now : 0, sc = cap > 0 ? (size_t)cap : 0;
        float* prev = exactly<float>(sp * 3);
        float* now = exactly<float>(sn * 3);
        uint8_t* kp = n_kp > 0 ? exactly<uint8_t>((size_t)n_kp) : nullptr;
        uint8_t* kn = n_kn > 0 ? exactly<uint8_t>((size_t)n_kn) : nullptr;
        float* xyzr = exactly<float>(sc * 4);
        float* vel = exactly<float>(sc * 3);
        int32_t* label = exactly<int32_t>(sc);
        int32_t* object = exactly<int32_t>(sc);
        if ((sp && !get(in, prev, sp * 3)) || (sn && !get(in, now, sn * 3)) || (kp && !get(in, kp, (size_t)n_kp)) || (kn && !get(in, kn, (size_t)n_kn)))
            return false;
        int32_t count = -1, matched = -1, n_objects = -1, n_accepted = -1;
        auto nul = [&](int bit) { return (mask >> bit & 1) != 0; };
        std::string err;
        const int rc = cloud_objects_host(nul(0) ? nullptr : &spec, nul(1) ? nullptr : &track, nul(2) ? nullptr : &obj, nul(3) ? nullptr : prev, n_prev,
                                          kp, nul(4) ? nullptr : now, n_now, kn, nul(5) ? nullptr : xyzr, nul(6) ? nullptr : vel,
                                          nul(7) ? nullptr : label, nul(8) ? nullptr : object, cap, nul(9) ? nullptr : &count,
                                          nul(10) ? nullptr : &matched, nul(11) ? nullptr : &n_objects, nul(12) ? nullptr : &n_accepted, &err);
        int32_t written = 0;
        if (rc == 0) {
            written = count;
            if (kn) {
                written = 0;
                for (int64_t i = 0; i < n_kn; ++i) written += kn[i] != 0;
            }
        }
        const int32_t head[6] = {rc, count, matched, n_objects, n_accepted, written};
        fwrite(head, 4, 6, out);
        if (written > 0) {
            fwrite(xyzr, 16, (size_t)written, out);
            fwrite(vel, 12, (size_t)written, out);
            fwrite(label, 4, (size_t)written, out);
            fwrite(object, 4, (size_t)written, out);
        }
        free(prev); free(now); free(kp); free(kn); free(xyzr); free(vel); free(label); free(object);
        return true;
    });
}
