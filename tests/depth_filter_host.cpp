// Stand-alone host build of the depth filter's definition (optimalmodulationds_amd/csrc/depth_filter_def.h: the body of
// omds_depth_points_filtered) for tests/test_depth_filter_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on
// its edge cases: the header's functions are the ones the library and its kernels use, only the compiler differs.
//   depth_filter_host IN OUT
// IN : int32 n_cases, then per case: omds_depth_camera (raw), omds_depth_filter_spec (raw), int32 have_filter (0: filt NULL),
//      int64 cap_points, int32 null_mask (1: cam NULL, 2: image NULL, 4: xyz_out NULL, 8: n_valid_out NULL, 16: n_rejected_out NULL),
//      int32 elem_bytes, int64 n_elems, the image (n_elems * elem_bytes bytes)
// OUT: per case: int32 rc, int64 n_valid, int64 n_rejected, int64 written, float xyz[written][3]   (written = cap_points when rc == 0, else 0)
// The image is allocated at exactly n_elems elements and the output at exactly cap_points points, so that a read or write past
// either -- a window that leaves the image, say -- is the sanitizer's to report.
#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/depth_filter_def.h"

int main(int argc, char** argv) {
    return run_cases(argc, argv, "depth_filter_host", [](FILE* in, FILE* out) {
        omds_depth_camera cam;
        omds_depth_filter_spec filt;
        int64_t cap = 0, n_elems = 0;
        int32_t have_filter = 0, null_mask = 0, elem_bytes = 0;
        if (!get(in, &cam) || !get(in, &filt) || !get(in, &have_filter) || !get(in, &cap) || !get(in, &null_mask) || !get(in, &elem_bytes) ||
            !get(in, &n_elems))
            return false;
        if (n_elems < 0 || elem_bytes < 1 || elem_bytes > 4) return false;
        const size_t image_bytes = (size_t)n_elems * (size_t)elem_bytes;
        unsigned char* image = exactly<unsigned char>(image_bytes);   // malloc: aligned for either element
        float* xyz = exactly<float>((cap > 0 ? (size_t)cap : 0) * 3);
        if (!image || !xyz) return false;
        if (image_bytes && !get(in, image, image_bytes)) return false;
        int64_t n_valid = -1, n_rejected = -1;
        std::string err;
        const int rc = depth_points_filtered_host((null_mask & 1) ? nullptr : &cam, have_filter ? &filt : nullptr, (null_mask & 2) ? nullptr : image,
                                                  (null_mask & 4) ? nullptr : xyz, cap, (null_mask & 8) ? nullptr : &n_valid,
                                                  (null_mask & 16) ? nullptr : &n_rejected, &err);
        const int64_t written = rc == 0 ? cap : 0;
        fwrite(&rc, 4, 1, out);
        fwrite(&n_valid, 8, 1, out);
        fwrite(&n_rejected, 8, 1, out);
        fwrite(&written, 8, 1, out);
        if (written > 0) fwrite(xyz, 12, (size_t)written, out);
        free(image);
        free(xyz);
        return true;
    });
}
