// Stand-alone host build of the definition of memory and velocities in one depth call (optimalmodulationds_amd/csrc/
// scene_memory_flow_def.h: the body of omds_depth_scene_memory_flow) for tests/test_scene_memory_flow_cpu.py, which compiles it with
// g++ -fsanitize=address,undefined and runs it on its cases: the header's functions are the ones the library and its kernels use,
// only the compiler differs.
//   scene_memory_flow_host IN OUT
// IN : int32 n_cases, then per case: omds_cloud_spec, omds_scene_memory_spec, omds_cloud_track_spec (raw), int32 have_obj,
//      omds_cloud_object_spec (raw), int32 have_filt, omds_depth_filter_spec (raw), int32 null_mask (1: mem_spec NULL, 2: mem_out NULL,
//      4: track NULL, 8: count_out NULL, 16: vel_out NULL), int32 cap, int64 n_cells, int32 have_mem_in, [uint32 mem_in[n_cells]],
//      then two frames, the previous one first: int32 n_cams (the value passed; previous frame: 0 = no previous frame), int32 n_images
//      (cameras and images that follow), per image: omds_depth_camera (raw), int32 elem_bytes, int64 n_elems, the image; int32 n_keep
//      (-1: NULL), uint8 keep[n_keep]
// OUT: per case: int32 rc, int32 counts[5], int32 count, n_matched, n_objects, n_objects_matched, int64 cells written, uint32
//      words[cells written], int64 spheres written, then float xyzr[4 n], float vel[3 n], int32 age[n], label[n], object[n]
// Every image is allocated at exactly n_elems elements, both word arrays at exactly n_cells words, every output array at exactly cap
// entries and every keep array at exactly n_keep bytes, so that a read or write past any of them is the sanitizer's to report.  An
// argument refusal must leave every output as it was: the program fills them with a sentinel first and exits 3 when one wrote anything
// (the too-many-cells refusal fills counts and count, as the header says, and nothing else).
#include <cstring>
#include <vector>

#include "host_io.h"

#include "../optimalmodulationds_amd/csrc/scene_memory_flow_def.h"

struct Frame {
    int32_t n_cams = 0;
    std::vector<omds_depth_camera> cams;
    std::vector<void*> images;
    int32_t n_keep = -1;
    uint8_t* keep = nullptr;
    bool read(FILE* in) {
        int32_t n_images = 0;
        if (!get(in, &n_cams) || !get(in, &n_images) || n_images < 0 || n_images > OMDS_DEPTH_MAX_CAMERAS) return false;
        cams.resize((size_t)n_images);
        images.assign((size_t)n_images, nullptr);
        for (int i = 0; i < n_images; ++i) {
            int32_t elem_bytes = 0;
            int64_t n_elems = 0;
            if (!get(in, &cams[(size_t)i]) || !get(in, &elem_bytes) || !get(in, &n_elems)) return false;
            if (n_elems < 0 || elem_bytes < 1 || elem_bytes > 4) return false;
            const size_t bytes = (size_t)n_elems * (size_t)elem_bytes;
            images[(size_t)i] = exactly<unsigned char>(bytes);
            if (!images[(size_t)i] || (bytes && !get(in, static_cast<unsigned char*>(images[(size_t)i]), bytes))) return false;
        }
        if (!get(in, &n_keep) || n_keep < -1) return false;
        if (n_keep >= 0) {
            keep = exactly<uint8_t>((size_t)n_keep);
            if (!keep || (n_keep && !get(in, keep, (size_t)n_keep))) return false;
        }
        return true;
    }
    ~Frame() {
        for (void* p : images) free(p);
        free(keep);
    }
};

int main(int argc, char** argv) {
    int refusal_wrote = 0;
    const int rc_all = run_cases(argc, argv, "scene_memory_flow_host", [&](FILE* in, FILE* out) {
        omds_cloud_spec spec;
        omds_scene_memory_spec mem;
        omds_cloud_track_spec track;
        omds_cloud_object_spec obj;
        omds_depth_filter_spec filt;
        int32_t have_obj = 0, have_filt = 0, null_mask = 0, cap = 0, have_in = 0;
        int64_t n_cells = 0;
        if (!get(in, &spec) || !get(in, &mem) || !get(in, &track) || !get(in, &have_obj) || !get(in, &obj) || !get(in, &have_filt) ||
            !get(in, &filt) || !get(in, &null_mask) || !get(in, &cap) || !get(in, &n_cells) || !get(in, &have_in))
            return false;
        if (n_cells < 0 || n_cells > OMDS_CLOUD_MAX_CELLS || cap < -1 || cap > OMDS_CLOUD_MAX_SPHERES) return false;
        uint32_t* mem_in = exactly<uint32_t>((size_t)n_cells);
        uint32_t* mem_out = exactly<uint32_t>((size_t)n_cells);
        if (!mem_in || !mem_out) return false;
        if (have_in && n_cells && !get(in, mem_in, (size_t)n_cells)) return false;
        Frame prev, now;
        if (!prev.read(in) || !now.read(in)) return false;
        const size_t room = cap > 0 ? (size_t)cap : 0;
        float* xyzr = exactly<float>(room * 4);
        float* vel = exactly<float>(room * 3);
        int32_t* age = exactly<int32_t>(room);
        int32_t* label = exactly<int32_t>(room);
        int32_t* object = exactly<int32_t>(room);
        const uint32_t sentinel = 0xA5A5A5A5u;
        for (int64_t c = 0; c < n_cells; ++c) mem_out[c] = sentinel;
        std::memset(xyzr, 0xA5, room * 16);
        std::memset(vel, 0xA5, room * 12);
        for (size_t i = 0; i < room; ++i) age[i] = label[i] = object[i] = -7;
        int32_t counts[5] = {-7, -7, -7, -7, -7}, count = -7, n_matched = -7, n_objects = -7, n_objects_matched = -7;
        std::string err;
        const int rc = scene_memory_flow_host(
            &spec, (null_mask & 1) ? nullptr : &mem, (null_mask & 4) ? nullptr : &track, have_obj ? &obj : nullptr, have_filt ? &filt : nullptr,
            prev.n_cams ? prev.cams.data() : nullptr, prev.images.data(), prev.n_cams, prev.keep, now.cams.data(), now.images.data(), now.n_cams,
            now.keep, have_in ? mem_in : nullptr, (null_mask & 2) ? nullptr : mem_out, counts, xyzr, (null_mask & 16) ? nullptr : vel, age, label,
            object, cap, (null_mask & 8) ? nullptr : &count, &n_matched, &n_objects, &n_objects_matched, &err);
        const bool too_many = rc != 0 && count != -7;
        if (rc != 0) {
            for (int64_t c = 0; c < n_cells; ++c) refusal_wrote |= mem_out[c] != sentinel;
            for (size_t i = 0; i < room; ++i) refusal_wrote |= age[i] != -7 || label[i] != -7 || object[i] != -7;
            refusal_wrote |= n_matched != -7 || n_objects != -7 || n_objects_matched != -7;
            if (!too_many)
                for (int k = 0; k < 5; ++k) refusal_wrote |= counts[k] != -7;
        }
        const int64_t cells_written = rc == 0 ? n_cells : 0, spheres = rc == 0 ? count : 0;
        fwrite(&rc, 4, 1, out);
        fwrite(counts, 4, 5, out);
        fwrite(&count, 4, 1, out);
        fwrite(&n_matched, 4, 1, out);
        fwrite(&n_objects, 4, 1, out);
        fwrite(&n_objects_matched, 4, 1, out);
        fwrite(&cells_written, 8, 1, out);
        if (cells_written > 0) fwrite(mem_out, 4, (size_t)cells_written, out);
        fwrite(&spheres, 8, 1, out);
        if (spheres > 0) {
            fwrite(xyzr, 16, (size_t)spheres, out);
            fwrite(vel, 12, (size_t)spheres, out);
            fwrite(age, 4, (size_t)spheres, out);
            fwrite(label, 4, (size_t)spheres, out);
            fwrite(object, 4, (size_t)spheres, out);
        }
        free(mem_in); free(mem_out); free(xyzr); free(vel); free(age); free(label); free(object);
        return true;
    });
    return rc_all ? rc_all : (refusal_wrote ? 3 : 0);
}
