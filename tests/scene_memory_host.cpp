// Stand-alone host build of the scene-memory definition (optimalmodulationds_amd/csrc/scene_memory_def.h: the body of
// omds_depth_scene_memory) for tests/test_scene_memory_cpu.py, which compiles it with g++ -fsanitize=address,undefined and runs it on
// its cases: the header's functions are the ones the library and its kernels use, only the compiler differs.
//   scene_memory_host IN OUT
// IN : int32 n_cases, then per case: omds_cloud_spec (raw), omds_scene_memory_spec (raw), int32 n_cams (the value passed),
//      int32 n_images (cameras and images that follow), int32 null_mask (1: mem_spec NULL, 2: mem_out NULL, 4: counts_out NULL),
//      int64 n_cells, int32 have_mem_in, [uint32 mem_in[n_cells]], then per image: omds_depth_camera (raw), int32 elem_bytes,
//      int64 n_elems, the image (n_elems * elem_bytes bytes)
// OUT: per case: int32 rc, int32 counts[4], int64 written, uint32 words[written]   (written = n_cells when rc == 0, else 0)
// Every image is allocated at exactly n_elems elements and both word arrays at exactly n_cells words, so that a read or write past
// any of them is the sanitizer's to report.  A refused call must leave the output words and the counts as they were: the program
// fills them with a sentinel first and exits 3 when a refusal wrote anything.
#include <vector>

#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/scene_memory_def.h"

extern "C" int omds_depth_scene_memory(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_camera* cams,
                                       const void* const* images, int32_t n_cams, const uint32_t* mem_in, uint32_t* mem_out,
                                       int32_t counts_out[4]) {
    std::string err;
    return scene_memory_host(spec, mem_spec, cams, images, n_cams, mem_in, mem_out, counts_out, &err);
}

int main(int argc, char** argv) {
    int refusal_wrote = 0;
    const int rc_all = run_cases(argc, argv, "scene_memory_host", [&](FILE* in, FILE* out) {
        omds_cloud_spec spec;
        omds_scene_memory_spec mem;
        int32_t n_cams = 0, n_images = 0, null_mask = 0, have_in = 0;
        int64_t n_cells = 0;
        if (!get(in, &spec) || !get(in, &mem) || !get(in, &n_cams) || !get(in, &n_images) || !get(in, &null_mask) || !get(in, &n_cells) ||
            !get(in, &have_in))
            return false;
        if (n_images < 0 || n_images > OMDS_DEPTH_MAX_CAMERAS || n_cells < 0 || n_cells > OMDS_CLOUD_MAX_CELLS) return false;
        uint32_t* mem_in = exactly<uint32_t>((size_t)n_cells);
        uint32_t* mem_out = exactly<uint32_t>((size_t)n_cells);
        if (!mem_in || !mem_out) return false;
        if (have_in && n_cells && !get(in, mem_in, (size_t)n_cells)) return false;
        std::vector<omds_depth_camera> cams((size_t)n_images);
        std::vector<void*> images((size_t)n_images, nullptr);
        for (int i = 0; i < n_images; ++i) {
            int32_t elem_bytes = 0;
            int64_t n_elems = 0;
            if (!get(in, &cams[(size_t)i]) || !get(in, &elem_bytes) || !get(in, &n_elems)) return false;
            if (n_elems < 0 || elem_bytes < 1 || elem_bytes > 4) return false;
            const size_t bytes = (size_t)n_elems * (size_t)elem_bytes;
            images[(size_t)i] = exactly<unsigned char>(bytes);   // malloc: aligned for either element
            if (!images[(size_t)i] || (bytes && !get(in, static_cast<unsigned char*>(images[(size_t)i]), bytes))) return false;
        }
        const uint32_t sentinel = 0xA5A5A5A5u;
        for (int64_t c = 0; c < n_cells; ++c) mem_out[c] = sentinel;
        int32_t counts[4] = {-7, -7, -7, -7};
        const int rc = omds_depth_scene_memory(&spec, (null_mask & 1) ? nullptr : &mem, cams.data(), images.data(), n_cams, have_in ? mem_in : nullptr,
                                               (null_mask & 2) ? nullptr : mem_out, (null_mask & 4) ? nullptr : counts);
        if (rc != 0) {
            for (int64_t c = 0; c < n_cells; ++c) refusal_wrote |= mem_out[c] != sentinel;
            for (int k = 0; k < 4; ++k) refusal_wrote |= counts[k] != -7;
        }
        const int64_t written = rc == 0 ? n_cells : 0;
        fwrite(&rc, 4, 1, out);
        fwrite(counts, 4, 4, out);
        fwrite(&written, 8, 1, out);
        if (written > 0) fwrite(mem_out, 4, (size_t)written, out);
        for (void* p : images) free(p);
        free(mem_in);
        free(mem_out);
        return true;
    });
    return rc_all ? rc_all : (refusal_wrote ? 3 : 0);
}
