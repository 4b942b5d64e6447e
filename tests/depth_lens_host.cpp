// Stand-alone host build of the lens definition (optimalmodulationds_amd/csrc/depth_lens_def.h: the body of omds_depth_lens_rays, and
// through depth_filter_def.h that of omds_depth_points_lens) for tests/test_depth_lens_cpu.py, which compiles it with g++
// -fsanitize=address,undefined and runs it on its cases: the header's functions are the ones the library and its kernels use, only the
// compiler differs.
//   depth_lens_host IN OUT
// IN : int32 n_cases, then per case: omds_depth_camera (raw), omds_depth_lens (raw), int32 have_lens (0: lens NULL), omds_depth_filter_spec
//      (raw), int32 have_filter (0: filt NULL), int64 visited, int32 elem_bytes, int64 n_elems, the image (n_elems * elem_bytes bytes)
// OUT: per case: int32 rc_rays, float r2_max, int64 n_invalid, int32 rc_points, int64 n_valid, int64 n_rejected, int64 written,
//      float ab[written][2], float xyz[written][3]   (written = visited when both rc == 0, else 0)
// The image is allocated at exactly n_elems elements and the outputs at exactly the visited count, so that a read or write past any of
// them is the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/depth_filter_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "depth_lens_host", [](FILE* in, FILE* out) {
        omds_depth_camera cam;
        omds_depth_lens lens;
        omds_depth_filter_spec filt;
        int64_t visited = 0, n_elems = 0;
        int32_t have_lens = 0, have_filter = 0, elem_bytes = 0;
        if (!get(in, &cam) || !get(in, &lens) || !get(in, &have_lens) || !get(in, &filt) || !get(in, &have_filter) || !get(in, &visited) ||
            !get(in, &elem_bytes) || !get(in, &n_elems))
            return false;
        if (n_elems < 0 || visited < 0 || elem_bytes < 1 || elem_bytes > 4) return false;
        const size_t image_bytes = (size_t)n_elems * (size_t)elem_bytes;
        unsigned char* image = exactly<unsigned char>(image_bytes);
        float* ab = exactly<float>((size_t)visited * 2);
        float* xyz = exactly<float>((size_t)visited * 3);
        if (!image || !ab || !xyz) return false;
        if (image_bytes && !get(in, image, image_bytes)) return false;
        float r2_max = -1.f;
        int64_t n_invalid = -1, n_valid = -1, n_rejected = -1;
        std::string err;
        const int rc_rays = depth_lens_rays_host(&cam, have_lens ? &lens : nullptr, ab, &r2_max, &n_invalid, &err);
        const int rc_points = depth_points_lens_host(&cam, have_lens ? &lens : nullptr, have_filter ? &filt : nullptr, image, xyz, visited, &n_valid,
                                                     &n_rejected, &err);
        const int64_t written = rc_rays == 0 && rc_points == 0 ? visited : 0;
        fwrite(&rc_rays, 4, 1, out);
        fwrite(&r2_max, 4, 1, out);
        fwrite(&n_invalid, 8, 1, out);
        fwrite(&rc_points, 4, 1, out);
        fwrite(&n_valid, 8, 1, out);
        fwrite(&n_rejected, 8, 1, out);
        fwrite(&written, 8, 1, out);
        if (written > 0) {
            fwrite(ab, 8, (size_t)written, out);
            fwrite(xyz, 12, (size_t)written, out);
        }
        free(image);
        free(ab);
        free(xyz);
        return true;
    });
}
