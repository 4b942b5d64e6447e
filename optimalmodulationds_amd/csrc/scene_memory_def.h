// The DEFINITION of the scene memory of the depth route (omds.h: omds_depth_scene_memory), stated once for the host entry point, the
// kernels k_scene_memory / k_scene_memory_forget of scene_memory_kernels.hip and the stand-alone host build of tests/scene_memory_host.cpp.
// Like depth_def.h, which it builds on and leaves as it is: plain fp32, every operation of omds.h its own statement (one rounding
// each; the translation units that include this are compiled without contraction across statements), fmaf written out.  The quotient
// 1.0f / zc is the IEEE-rounded one on both sides: no fast division, no reciprocal intrinsic.
//   m[c] == 0: cell c is empty;  m[c] == k >= 1: occupied, last counted k - 1 calls ago.
#pragma once
#include "depth_filter_def.h"

// an omds_scene_memory_spec behind its checks: what the kernels take by value
struct SceneMem {
    int max_age;            // < 1: a remembered cell never expires
    float clear_margin;     // the spec's, or the grid's sphere radius
    int footprint;          // 0 .. 3: the window of a verdict is (2 footprint + 1)^2 visited pixels
};

// what a verdict needs of a camera beside its DepthCam (which keeps 1 / fx and 1 / fy only)
struct SceneMemCam {
    float fx, fy;
    float istep;            // 1.0f / (float)step (one division, on the host)
};
struct SceneMemCams {
    SceneMemCam k[OMDS_DEPTH_MAX_CAMERAS];
};

inline int scene_memory_resolve(const omds_scene_memory_spec* s, const CloudGrid& g, SceneMem* out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!s) return fail("scene memory: null memory spec");
    if (s->clear_margin != s->clear_margin) return fail("scene memory: clear_margin is not a number");
    if (s->footprint < 0 || s->footprint > 3) return fail("scene memory: footprint must be 0 .. 3");
    out->max_age = s->max_age < 1 ? 0 : s->max_age;
    out->clear_margin = s->clear_margin > 0.f ? s->clear_margin : g.radius;
    out->footprint = s->footprint;
    return OMDS_OK;
}

inline SceneMemCam scene_memory_camera(const omds_depth_camera& c, const DepthCam& r) {
    return SceneMemCam{c.fx, c.fy, 1.0f / (float)r.step};
}

// One camera's verdict on the point p (a cell centre) that got no points this call: true = FREE, the camera looked through it; false =
// SILENT, the camera cannot tell (out of range, out of the image, no return, or a return at or before lim).  R is taken as orthonormal
// and applied transposed (camera <- grid frame); it is not checked.  The range gate is NOT applied to the pixel's depth: a return
// beyond z_max is still a return from behind the cell.
//   LENS (depth_lens_def.h), and lens->ab != nullptr: the camera has a lens.  The pixel the cell centre falls on comes from the forward
//   model at (a, b) = (xc iz, yc iz); beyond the field of view of the camera's ray table, !(fmaf(a, a, b * b) <= r2_max), the
//   polynomial may fold back and the verdict is SILENT, which never clears a cell.  From rintf on everything is the same.
template <bool LENS = false>
OMDS_CLOUD_FN bool scene_memory_camera_free(const DepthCam& c, const SceneMemCam& k, const void* image, const SceneMem& sm, const float* p,
                                            const DepthLensCam* lens = nullptr) {
    const float big = 3.402823466e+38f;
    const float d0 = p[0] - c.pose[3];
    const float d1 = p[1] - c.pose[7];
    const float d2 = p[2] - c.pose[11];
    const float x2 = c.pose[8] * d2;
    const float y2 = c.pose[9] * d2;
    const float z2 = c.pose[10] * d2;
    const float xc = fmaf(c.pose[0], d0, fmaf(c.pose[4], d1, x2));
    const float yc = fmaf(c.pose[1], d0, fmaf(c.pose[5], d1, y2));
    const float zc = fmaf(c.pose[2], d0, fmaf(c.pose[6], d1, z2));
    if (!(zc >= c.z_min && zc <= c.z_max)) return false;
    const float iz = 1.0f / zc;
    const float xn = xc * iz;
    const float yn = yc * iz;
    float uf, vf;
    if (LENS && lens->ab) {
        const float r2 = depth_lens_r2(xn, yn);
        if (!(r2 <= lens->r2_max)) return false;
        float ad, bd;
        depth_lens_forward(lens->lens, xn, yn, &ad, &bd);
        uf = fmaf(ad, k.fx, c.cx);
        vf = fmaf(bd, k.fy, c.cy);
    } else {
        uf = fmaf(xn, k.fx, c.cx);
        vf = fmaf(yn, k.fy, c.cy);
    }
    const float us = uf * k.istep;
    const float vs = vf * k.istep;
    const float ju = rintf(us);
    const float jv = rintf(vs);
    if (!(ju >= 0.f && ju < (float)c.nu && jv >= 0.f && jv < (float)c.nv)) return false;   // as floats, before any conversion
    const int iu = (int)ju, iv = (int)jv;
    const float lim = zc + sm.clear_margin;
    for (int b = -sm.footprint; b <= sm.footprint; ++b) {
        const int y = iv + b;
        if (y < 0 || y >= c.nv) continue;
        const long long row = (long long)y * c.step * c.pitch;
        for (int a = -sm.footprint; a <= sm.footprint; ++a) {
            const int x = iu + a;
            if (x < 0 || x >= c.nu) continue;
            const long long at = row + (long long)x * c.step;
            float z_pix;
            if (c.format == OMDS_DEPTH_U16) {
                if (!depth_z_u16(c, static_cast<const uint16_t*>(image)[at], &z_pix)) return false;
            } else {
                z_pix = static_cast<const float*>(image)[at];
            }
            if (!(fabsf(z_pix) <= big && z_pix > lim)) return false;
        }
    }
    return true;
}

// the word of a remembered cell that no camera cleared: one call older, saturating; 0 when that is more than max_age unseen calls
OMDS_CLOUD_FN unsigned scene_memory_older(const SceneMem& sm, unsigned m) {
    const unsigned next = m == 0xFFFFFFFFu ? m : m + 1u;
    if (sm.max_age >= 1 && next > (unsigned)sm.max_age + 1u) return 0u;
    return next;
}

enum { SCENE_MEM_SEEN = 0, SCENE_MEM_REMEMBERED = 1, SCENE_MEM_CLEARED = 2, SCENE_MEM_EXPIRED = 3, SCENE_MEM_FORGOTTEN = 4, SCENE_MEM_COUNTS = 5 };

// m' of cell `cell` with n points this call and the stored word m (steps 1 - 5 of omds.h); which of the four counters it adds to
// goes to *what (-1: none, the cell was and stays empty)
// LENS: lenses->cam[i] is the lens of camera i (ab == nullptr: none)
template <bool LENS = false, class Cams>   // cams.cam(i): the DepthCam of camera i, cams.image(i): element (0, 0) of its image
OMDS_CLOUD_FN unsigned scene_memory_cell(const CloudGrid& g, const SceneMem& sm, const Cams& cams, const SceneMemCams& ks, int n_cams, int cell,
                                         unsigned n, unsigned m, int* what, const DepthLensTable* lenses = nullptr) {
    if (n >= g.min_points) { *what = SCENE_MEM_SEEN; return 1u; }
    if (m == 0u) { *what = -1; return 0u; }
    float p[4];
    cloud_sphere(g, cell, p);
    bool is_free = false;
    for (int i = 0; i < n_cams; ++i)   // every camera is asked: the index stays uniform over a wave
        if (scene_memory_camera_free<LENS>(cams.cam(i), ks.k[i], cams.image(i), sm, p, LENS ? &lenses->cam[i] : nullptr)) is_free = true;
    if (is_free) { *what = SCENE_MEM_CLEARED; return 0u; }
    const unsigned next = scene_memory_older(sm, m);
    *what = next ? SCENE_MEM_REMEMBERED : SCENE_MEM_EXPIRED;
    return next;
}

// omds_depth_scene_memory[_filtered] without its argument messages, the one body of both: the counting pass of the depth route
// (omds_depth_points[_filtered] + cloud_cell), then steps 1 - 5 per cell.  filt == nullptr: no depth filter.  The filter changes the
// counts alone: the verdicts of step 3 read the raw images (a flying pixel is still a return).  No self-filter.  lenses [n_cams]
// (omds_depth_scene_memory_lens; nullptr: none): the counts come from the points on the rays of depth_lens_def.h, and the verdicts of
// a camera with a lens go through its forward model; a pixel without a ray is still a return for both
inline int scene_memory_lens_host(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_filter_spec* filt,
                                  const omds_depth_lens* lenses, const omds_depth_camera* cams, const void* const* images, int32_t n_cams,
                                  const uint32_t* mem_in, uint32_t* mem_out, int32_t* counts_out, std::string* err) {
    auto fail = [&](const char* m) { if (err) *err = m; return (int)OMDS_ERR_INVALID_ARG; };
    CloudGrid g;
    SceneMem sm;
    DepthFilter f;
    if (int rc = cloud_resolve_spec(spec, &g, err)) return rc;
    if (int rc = scene_memory_resolve(mem_spec, g, &sm, err)) return rc;
    if (filt)
        if (int rc = depth_filter_resolve(filt, &f, err)) return rc;
    if (n_cams < 1 || n_cams > OMDS_DEPTH_MAX_CAMERAS || !cams || !images) return fail("omds_depth_scene_memory: need 1 <= n_cams <= 8 and non-null cams, images [n_cams]");
    if (!mem_out) return fail("omds_depth_scene_memory: null mem_out");
    DepthCam cam[OMDS_DEPTH_MAX_CAMERAS];
    SceneMemCams ks;
    int64_t visited = 0;
    for (int i = 0; i < n_cams; ++i) {
        if (int rc = depth_resolve_camera(cams + i, &cam[i], err)) return rc;
        if (!images[i]) return fail("omds_depth_scene_memory: a null image");
        ks.k[i] = scene_memory_camera(cams[i], cam[i]);
        visited += depth_visited(cam[i]);
    }
    if (visited > OMDS_CLOUD_MAX_POINTS) return fail("omds_depth_scene_memory: more than 16 777 216 visited pixels in all");
    DepthLensTable lt;
    std::vector<float> rays[OMDS_DEPTH_MAX_CAMERAS];
    bool lensed = false;
    for (int i = 0; i < n_cams; ++i) {
        lt.cam[i].ab = nullptr;
        lt.cam[i].r2_max = 0.f;
        if (int rc = depth_lens_resolve(lenses ? lenses + i : nullptr, &lt.cam[i].lens, err)) return rc;
        if (lt.cam[i].lens.model == 0) continue;
        rays[i].resize((size_t)depth_visited(cam[i]) * 2);
        int64_t n_invalid;
        depth_lens_table_host(cam[i], cams[i].fx, cams[i].fy, lt.cam[i].lens, rays[i].data(), &lt.cam[i].r2_max, &n_invalid);
        lt.cam[i].ab = rays[i].data();
        lensed = true;
    }
    std::vector<uint32_t> count((size_t)g.n_cells, 0u);
    for (int i = 0; i < n_cams; ++i) {
        const DepthCam& c = cam[i];
        for (int iv = 0; iv < c.nv; ++iv)
            for (int iu = 0; iu < c.nu; ++iu) {
                float w[3];
                if (depth_filtered_pixel(c, filt ? &f : nullptr, images[i], iu, iv, w, lt.cam[i].ab) != 1) continue;
                const int cell = cloud_cell(g, w[0], w[1], w[2]);
                if (cell >= 0) count[(size_t)cell]++;
            }
    }
    struct HostCams {
        const DepthCam* c;
        const void* const* images;
        const DepthCam& cam(int i) const { return c[i]; }
        const void* image(int i) const { return images[i]; }
    } const host_cams{cam, images};
    int32_t counts[4] = {0, 0, 0, 0};
    for (int cell = 0; cell < g.n_cells; ++cell) {
        int what;
        const unsigned n = count[(size_t)cell], m = mem_in ? mem_in[cell] : 0u;
        mem_out[cell] = lensed ? scene_memory_cell<true>(g, sm, host_cams, ks, n_cams, cell, n, m, &what, &lt)
                               : scene_memory_cell(g, sm, host_cams, ks, n_cams, cell, n, m, &what);
        if (what >= 0) counts[what]++;
    }
    if (counts_out)
        for (int k = 0; k < 4; ++k) counts_out[k] = counts[k];
    return OMDS_OK;
}
inline int scene_memory_host(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_filter_spec* filt,
                             const omds_depth_camera* cams, const void* const* images, int32_t n_cams, const uint32_t* mem_in,
                             uint32_t* mem_out, int32_t* counts_out, std::string* err) {
    return scene_memory_lens_host(spec, mem_spec, filt, nullptr, cams, images, n_cams, mem_in, mem_out, counts_out, err);
}
inline int scene_memory_host(const omds_cloud_spec* spec, const omds_scene_memory_spec* mem_spec, const omds_depth_camera* cams,
                             const void* const* images, int32_t n_cams, const uint32_t* mem_in, uint32_t* mem_out, int32_t* counts_out,
                             std::string* err) {
    return scene_memory_host(spec, mem_spec, nullptr, cams, images, n_cams, mem_in, mem_out, counts_out, err);
}
