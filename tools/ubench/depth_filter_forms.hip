// The two forms of the filtered counting pass of the depth routes (csrc/depth_kernels.hip: k_depth_count_filt[_rec]) side by side, on
// one 640 x 480 U16 image in device memory, kernel times by HIP events.  EXPERIMENTS.md R27.
//   tile   : the library's kernels -- a workgroup stages a tile of 32 x 32 visited pixels and its halo into LDS, the support test reads LDS
//   direct : the form that was NOT kept, written here only -- today's launch shape (a lane takes a run of 4 pixels of a row, 256
//            consecutive runs to a workgroup), each lane reading its (2 R + 1) rows of 4 + 2 R neighbours through the caches, no LDS,
//            no barrier; the same definition (depth_filter_keep), the same deprojection and the same merge behind it
//   plain  : k_depth_count[_rec], no filter, for scale
// Before anything is timed both forms count the image into cleared buffers, which must come out equal word for word.  The timed
// launches do not clear the buffers in between (the atomics cost the same on any value).  The legs alternate launch by launch.
// This file includes the library's kernel file: it sees the kernels and helpers of its unnamed namespace and links no library.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=on -Iinclude -o tools/ubench/depth_filter_forms tools/ubench/depth_filter_forms.hip
// Run:   tools/ubench/depth_filter_forms [launches per leg, default 200]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../optimalmodulationds_amd/csrc/depth_kernels.hip"

#define HIP_OK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e_));                        \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

namespace {

template <bool REC, int R>
__global__ __launch_bounds__(CLOUD_NT) void k_direct(DepthTable tab, CloudGrid g, DepthFilter f, void* buf, unsigned* counters) {
    const DepthCamDev& d = tab.cam[blockIdx.y];
    const DepthCam& c = d.c;
    unsigned kept = 0, rejected = 0;
    for (long long base = (long long)blockIdx.x * CLOUD_NT; base < d.items; base += (long long)gridDim.x * CLOUD_NT) {
        const long long item = base + threadIdx.x;
        int cell[DEPTH_RUN] = {-1, -1, -1, -1};
        unsigned k[DEPTH_RUN][3] = {};
        if (item < d.items) {
            const int iv = (int)(item / d.runs), j0 = (int)(item % d.runs) * DEPTH_RUN;
            float win[2 * R + 1][DEPTH_RUN + 2 * R];
            for (int b = 0; b < 2 * R + 1; ++b)
                for (int x = 0; x < DEPTH_RUN + 2 * R; ++x) {
                    const int xx = j0 - R + x, yy = iv - R + b;
                    const bool in = xx >= 0 && xx < c.nu && yy >= 0 && yy < c.nv;
                    win[b][x] = in ? depth_filter_z(c, d.image, (long long)yy * c.step * c.pitch + (long long)xx * c.step) : __builtin_nanf("");
                }
            for (int t = 0; t < DEPTH_RUN; ++t) {
                const float z = win[R][R + t];
                if (!depth_gate(c, z)) continue;
                if (!depth_filter_keep(f, R, z, [&](int a, int b) { return win[R + b][R + t + a]; })) {
                    ++rejected;
                    continue;
                }
                ++kept;
                cell[t] = depth_pixel_cell<REC>(c, g, (j0 + t) * c.step, iv * c.step, z, k[t]);
            }
        }
        depth_add_cells<REC>(cell, k, buf);
    }
    kept = wave_sum(kept);
    rejected = wave_sum(rejected);
    if ((threadIdx.x & 63) == 0) {
        if (kept) atomicAdd(counters, kept);
        if (rejected) atomicAdd(counters + 1, rejected);
    }
}

// a wall 3 m away, three discs nearer (depth edges), a smooth ripple, and one pixel in sixteen a speckle or a hole
std::vector<uint16_t> image_of(int W, int H) {
    std::vector<uint16_t> img((size_t)W * H);
    unsigned s = 12345u;
    for (int v = 0; v < H; ++v)
        for (int u = 0; u < W; ++u) {
            float z = 3.0f + 0.0002f * u + 0.0001f * v;
            const int cx[3] = {160, 330, 500}, cy[3] = {120, 260, 200}, r[3] = {60, 90, 40};
            const float zd[3] = {1.2f, 1.8f, 0.9f};
            for (int i = 0; i < 3; ++i)
                if ((u - cx[i]) * (u - cx[i]) + (v - cy[i]) * (v - cy[i]) < r[i] * r[i]) z = zd[i];
            s = s * 1664525u + 1013904223u;
            const unsigned h = s >> 16;
            if ((h & 15u) == 0) z = (h & 16u) ? 0.f : 0.5f + (h >> 5 & 1023u) * 0.003f;
            img[(size_t)v * W + u] = (uint16_t)(z * 1000.f + 0.5f);
        }
    return img;
}

template <class F>
float time_launch(hipEvent_t a, hipEvent_t b, const F& launch) {
    HIP_OK(hipEventRecord(a, nullptr));
    launch();
    HIP_OK(hipEventRecord(b, nullptr));
    HIP_OK(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, a, b));
    return ms * 1000.f;
}

float median(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

template <bool REC, int R>
void run(const DepthTable& table, const CloudGrid& g, int launches) {
    typedef typename std::conditional<REC, uint4, unsigned>::type Word;
    const size_t cells = cloud_padded_cells(g);
    const DepthFilter f{R, R == 1 ? 4 : R == 2 ? 10 : 20, 0.01f, 0.01f};
    Word *a = nullptr, *b = nullptr;
    unsigned* counters = nullptr;
    HIP_OK(hipMalloc(&a, cells * sizeof(Word)));
    HIP_OK(hipMalloc(&b, cells * sizeof(Word)));
    HIP_OK(hipMalloc(&counters, 4 * sizeof(unsigned)));
    HIP_OK(hipMemset(a, 0, cells * sizeof(Word)));
    HIP_OK(hipMemset(b, 0, cells * sizeof(Word)));
    HIP_OK(hipMemset(counters, 0, 4 * sizeof(unsigned)));
    DepthTable plain_tab = table, tile_tab = table;
    const dim3 plain_grid = depth_blocks(plain_tab, 1), tile_grid = depth_filt_blocks(tile_tab, 1);
    auto tile = [&](Word* into, unsigned* cnt) {
        if (REC) hipLaunchKernelGGL((k_depth_count_filt_rec<R>), tile_grid, dim3(CLOUD_NT), 0, nullptr, tile_tab, g, f, (uint4*)into, cnt);
        else hipLaunchKernelGGL((k_depth_count_filt<R>), tile_grid, dim3(CLOUD_NT), 0, nullptr, tile_tab, g, f, (unsigned*)into, cnt);
    };
    auto direct = [&](Word* into, unsigned* cnt) {
        hipLaunchKernelGGL((k_direct<REC, R>), plain_grid, dim3(CLOUD_NT), 0, nullptr, plain_tab, g, f, (void*)into, cnt);
    };
    auto plain = [&](Word* into) {
        if (REC) hipLaunchKernelGGL(k_depth_count_rec, plain_grid, dim3(CLOUD_NT), 0, nullptr, plain_tab, g, (uint4*)into);
        else hipLaunchKernelGGL(k_depth_count, plain_grid, dim3(CLOUD_NT), 0, nullptr, plain_tab, g, (unsigned*)into);
    };
    tile(a, counters);
    direct(b, counters + 2);
    HIP_OK(hipDeviceSynchronize());
    std::vector<Word> ha(cells), hb(cells);
    unsigned hc[4];
    HIP_OK(hipMemcpy(ha.data(), a, cells * sizeof(Word), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hb.data(), b, cells * sizeof(Word), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(hc, counters, sizeof(hc), hipMemcpyDeviceToHost));
    const bool same = std::memcmp(ha.data(), hb.data(), cells * sizeof(Word)) == 0 && hc[0] == hc[2] && hc[1] == hc[3];
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    std::vector<float> t_tile, t_direct, t_plain;
    for (int i = 0; i < launches + 5; ++i) {
        const float p = time_launch(e0, e1, [&] { plain(b); });
        const float t = time_launch(e0, e1, [&] { tile(a, counters); });
        const float d = time_launch(e0, e1, [&] { direct(b, counters + 2); });
        if (i < 5) continue;   // warm-up
        t_plain.push_back(p);
        t_tile.push_back(t);
        t_direct.push_back(d);
    }
    HIP_OK(hipGetLastError());
    printf("%-7s radius %d min_support %2d: kept %u rejected %u, tile and direct agree: %s;  median of %d launches: plain %.2f us, tile (LDS) %.2f us, "
           "direct %.2f us\n", REC ? "records" : "counts", R, f.min_support, hc[0], hc[1], same ? "yes" : "NO", launches, median(t_plain), median(t_tile),
           median(t_direct));
    if (!same) exit(3);
    HIP_OK(hipEventDestroy(e0));
    HIP_OK(hipEventDestroy(e1));
    HIP_OK(hipFree(a));
    HIP_OK(hipFree(b));
    HIP_OK(hipFree(counters));
}

}  // namespace

int main(int argc, char** argv) {
    const int launches = argc > 1 ? atoi(argv[1]) : 200;
    const int W = 640, H = 480;
    omds_depth_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.width = W; cam.height = H; cam.format = OMDS_DEPTH_U16; cam.step = 1;
    cam.fx = cam.fy = 600.f; cam.cx = 319.5f; cam.cy = 239.5f;
    cam.depth_scale = 0.001f; cam.z_min = 0.2f; cam.z_max = 6.f;
    const float pose[12] = {0, 0, 1, 0, -1, 0, 0, 0, 0, -1, 0, 0};   // the camera looks along x
    std::memcpy(cam.pose, pose, sizeof(pose));
    omds_cloud_spec spec;
    std::memset(&spec, 0, sizeof(spec));
    spec.origin[0] = -1.f; spec.origin[1] = -3.2f; spec.origin[2] = -3.2f;
    spec.voxel = 0.05f;
    spec.dims[0] = spec.dims[1] = spec.dims[2] = 128;
    spec.min_points = 1; spec.max_spheres = 16384;
    std::string err;
    DepthTable table;
    std::memset(static_cast<void*>(&table), 0, sizeof(table));
    CloudGrid g;
    if (depth_resolve_camera(&cam, &table.cam[0].c, &err) || cloud_resolve_spec(&spec, &g, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    const std::vector<uint16_t> img = image_of(W, H);
    void* d_img = nullptr;
    HIP_OK(hipMalloc(&d_img, img.size() * 2));
    HIP_OK(hipMemcpy(d_img, img.data(), img.size() * 2, hipMemcpyHostToDevice));
    table.cam[0].image = d_img;
    printf("one %d x %d U16 image in device memory, grid 128^3 x 0.05 m; kernel times by HIP events, the legs alternating\n", W, H);
    run<false, 1>(table, g, launches);
    run<false, 2>(table, g, launches);
    run<false, 3>(table, g, launches);
    run<true, 1>(table, g, launches);
    run<true, 2>(table, g, launches);
    run<true, 3>(table, g, launches);
    HIP_OK(hipFree(d_img));
    printf("depth_filter_forms: done\n");
    return 0;
}
