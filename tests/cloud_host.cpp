// Stand-alone host build of the point-cloud definition (optimalmodulationds_amd/csrc/point_cloud_def.h: the body of
// omds_point_cloud_spheres) for tests/test_cloud_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on its
// edge cases: the header's functions are the ones the library and its kernels use, only the compiler differs.
//   cloud_host IN OUT
// IN : int32 n_cases, then per case: omds_cloud_spec (raw), int64 n_points, int32 cap, int32 null_mask (1: spec NULL, 2: xyz NULL,
//      4: xyzr_out NULL, 8: count_out NULL), float xyz[n_points][3]
// OUT: per case: int32 rc, int32 count, int32 written, float xyzr[written][4]   (written = count when rc == 0, else 0)
// The output array is allocated at exactly cap spheres and the points at exactly n_points, so that a write or read past either is
// the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/point_cloud_def.h"

extern "C" int omds_point_cloud_spheres(const omds_cloud_spec* spec, const float* xyz, int64_t n_points, float* xyzr_out, int32_t cap,
                                        int32_t* count_out) {
    std::string err;
    return cloud_spheres_host(spec, xyz, n_points, xyzr_out, cap, count_out, &err);
}

int main(int argc, char** argv) {
    return run_cases(argc, argv, "cloud_host", [](FILE* in, FILE* out) {
        omds_cloud_spec spec;
        int64_t n_points = 0;
        int32_t cap = 0, null_mask = 0;
        if (!get(in, &spec) || !get(in, &n_points) || !get(in, &cap) || !get(in, &null_mask)) return false;
        const size_t stored = n_points > 0 ? (size_t)n_points : 0;
        float* xyz = exactly<float>(stored * 3);
        float* xyzr = exactly<float>((cap > 0 ? (size_t)cap : 0) * 4);
        if (stored && !get(in, xyz, stored * 3)) return false;
        int32_t count = -1;
        const int rc = omds_point_cloud_spheres((null_mask & 1) ? nullptr : &spec, (null_mask & 2) ? nullptr : xyz, n_points,
                                                (null_mask & 4) ? nullptr : xyzr, cap, (null_mask & 8) ? nullptr : &count);
        const int32_t head[3] = {rc, count, rc == 0 ? count : 0};
        fwrite(head, 4, 3, out);
        if (head[2] > 0) fwrite(xyzr, 16, (size_t)head[2], out);
        free(xyz);
        free(xyzr);
        return true;
    });
}
