// SDF training data (include/omds.h: omds_sdf_data_*), host side: the spec's checks and the temporary device buffers around the
// generator kernel (dataset_kernels.hip).
#include "capi_internal.h"

static bool finite_box(const float* lo, const float* hi, int k) {
    for (int i = 0; i < k; ++i)
        if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || lo[i] > hi[i]) return false;
    return true;
}

static_assert(OMDS_SDF_DATA_MAX_PTS_PER_LINK == 256 && OMDS_SDF_DATA_MAX_LINK_PTS == 2048 && OMDS_MAX_DOF == 7,
              "the messages of omds_sdf_data_resolve spell these limits out");

// Everything an entry point checks before it touches a device; fills *a when non-null.
int omds_sdf_data_resolve(const omds_sdf_data_spec* sp, SdfDataArgs* a, std::string* err) {
    auto bad = [&](const char* m) { if (err) *err = std::string("omds_sdf_data: ") + m; return (int)OMDS_ERR_INVALID_ARG; };
    if (!sp) return bad("spec is NULL");
    const bool dh = sp->kind == OMDS_SDF_DATA_DH;
    if (!dh && sp->kind != OMDS_SDF_DATA_POINT) return bad("kind must be 0 (DH chain) or 1 (point robot)");
    const int n = sp->n_dof;
    if (dh && (n < 1 || n > OMDS_MAX_DOF)) return bad("a DH chain needs 1 <= n_dof <= 7");
    if (!dh && (n < 2 || n > 3)) return bad("the point robot needs n_dof = 2 or 3 point dimensions");
    if (dh && (sp->n_pts < 1 || sp->n_pts > OMDS_SDF_DATA_MAX_PTS_PER_LINK || n * sp->n_pts > OMDS_SDF_DATA_MAX_LINK_PTS))
        return bad("a DH chain needs 1 <= n_pts <= 256 and n_dof * n_pts <= 2048 (the link points one workgroup holds)");
    if (sp->n_cfg < 1) return bad("n_cfg must be >= 1");
    if (sp->n_uniform < 0 || sp->n_near < 0 || sp->n_uniform + (int64_t)sp->n_near < 1 || sp->n_uniform + (int64_t)sp->n_near > (1 << 24))
        return bad("need n_uniform, n_near >= 0 and 1 <= n_uniform + n_near <= 2^24 rows per configuration");
    if (!std::isfinite(sp->near_scale) || sp->near_scale < 0.f) return bad("near_scale must be finite and >= 0");
    if (dh && (!sp->dh_params || sp->dh_rows < n + 1)) return bad("dh_params must hold n_dof + 1 rows (link l is sampled along a_{l+1})");
    if (dh && !sp->lspan) return bad("lspan (torch.linspace(0.01, 1, n_pts)) is NULL");
    if (!sp->q_min || !sp->q_max || !sp->p_min || !sp->p_max) return bad("q_min, q_max, p_min, p_max must all be given");
    const int pd = dh ? 3 : n;
    if (!finite_box(sp->q_min, sp->q_max, n)) return bad("q_min / q_max must be finite with q_min <= q_max");
    if (!finite_box(sp->p_min, sp->p_max, pd)) return bad("p_min / p_max must be finite with p_min <= p_max");
    if (dh) {
        for (int i = 0; i < 4 * (n + 1); ++i)
            if (!std::isfinite(sp->dh_params[i])) return bad("dh_params must be finite");
        for (int k = 0; k < sp->n_pts; ++k)
            if (!std::isfinite(sp->lspan[k])) return bad("lspan must be finite");
    }
    const int64_t R = (int64_t)sp->n_uniform + sp->n_near, cols = 2 * (int64_t)n + (dh ? 3 : 1);
    if ((int64_t)sp->n_cfg > INT64_MAX / R / cols) return bad("n_cfg * (n_uniform + n_near) * cols overflows int64");
    if (!a) return OMDS_OK;
    std::memset(a, 0, sizeof(*a));
    a->kind = sp->kind; a->n = n; a->n_pts = dh ? sp->n_pts : 0; a->n_uniform = sp->n_uniform; a->n_near = sp->n_near;
    a->pd = pd; a->nin = n + pd; a->nlab = dh ? n : 1;
    if (dh) {
        std::memcpy(a->dh, sp->dh_params, sizeof(float) * 4 * (n + 1));
        std::memcpy(a->span, sp->lspan, sizeof(float) * sp->n_pts);
    }
    for (int i = 0; i < n; ++i) { a->qlo[i] = sp->q_min[i]; a->qw[i] = sp->q_max[i] - sp->q_min[i]; }
    for (int i = 0; i < pd; ++i) {
        a->plo[i] = sp->p_min[i]; a->pw[i] = sp->p_max[i] - sp->p_min[i];
        a->olo[i] = sp->near_scale * sp->p_min[i]; a->ow[i] = sp->near_scale * sp->p_max[i] - a->olo[i];
    }
    return OMDS_OK;
}

// the rows of n_cfg configurations (cfg0 ..) to host memory through a temporary device buffer on a stream of its own
static int sdf_data_run(int device, const omds_sdf_data_spec* spec, uint64_t seed, int64_t cfg0, int64_t n_cfg, const float* q,
                        const float* pu, const float* po, float* out, const char* who) {
    SdfDataArgs a;
    std::string err;
    int rc = omds_sdf_data_resolve(spec, &a, &err);
    auto bad = [&](const std::string& m) { g_create_err = std::string(who) + ": " + m; return (int)OMDS_ERR_INVALID_ARG; };
    if (rc) return bad(err);
    if (!out) return bad("out is NULL");
    const bool draws = (q != nullptr);
    if (draws && (!q || (a.n_uniform > 0 && !pu) || (a.n_near > 0 && !po))) return bad("q, p_uniform and near_offsets must be given");
    const int64_t R = (int64_t)a.n_uniform + a.n_near, cols = a.nin + a.nlab;
    if (n_cfg < 1) return bad("n_cfg must be >= 1");
    if (n_cfg > INT64_MAX / R / cols || n_cfg * R * cols > (int64_t)(SIZE_MAX / sizeof(float))) return bad("n_cfg * rows * cols overflows");
    if (n_cfg > 0x7fffffff) return bad("n_cfg must be <= 2^31 - 1 (one workgroup per configuration)");
    if (cfg0 < 0 || cfg0 > INT64_MAX - n_cfg) return bad("cfg0 must be >= 0 and cfg0 + n_cfg must fit int64");
    const size_t nfl = (size_t)(n_cfg * R * cols);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        g_create_err = std::string(who) + ": no HIP device available; this library has no CPU fallback";
        return OMDS_ERR_HIP;
    }
    if (device < 0 || device >= ndev) return bad("device ordinal out of range");
    DevBuf<float> d_out, d_draw;   // freed on return, behind the synchronisation of every path
    hipStream_t s = nullptr;
    auto fail = [&](const char* what, hipError_t err2) {
        g_create_err = std::string(who) + ": " + what + ": " + hipGetErrorString(err2);
        if (s) (void)hipStreamSynchronize(s);
        if (s) (void)hipStreamDestroy(s);
        return (int)OMDS_ERR_HIP;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = d_out.alloc(nfl)) != hipSuccess) return fail("hipMalloc", e);
    const float *qd = nullptr, *pud = nullptr, *pod = nullptr;
    if (draws) {
        const size_t nq = (size_t)n_cfg * a.n, nu = (size_t)n_cfg * a.n_uniform * a.pd, no = (size_t)n_cfg * a.n_near * a.pd;
        if ((e = d_draw.alloc(nq + nu + no)) != hipSuccess) return fail("hipMalloc", e);
        if ((e = hipMemcpyAsync(d_draw, q, nq * sizeof(float), hipMemcpyHostToDevice, s)) != hipSuccess) return fail("hipMemcpy", e);
        if (nu && (e = hipMemcpyAsync(d_draw + nq, pu, nu * sizeof(float), hipMemcpyHostToDevice, s)) != hipSuccess) return fail("hipMemcpy", e);
        if (no && (e = hipMemcpyAsync(d_draw + nq + nu, po, no * sizeof(float), hipMemcpyHostToDevice, s)) != hipSuccess)
            return fail("hipMemcpy", e);
        qd = d_draw; pud = d_draw + nq; pod = d_draw + nq + nu;
    }
    omds_launch_sdf_data(s, a, seed, cfg0, n_cfg, qd, pud, pod, d_out, nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return fail("k_sdf_data launch", e);
    if ((e = hipMemcpyAsync(out, d_out, nfl * sizeof(float), hipMemcpyDeviceToHost, s)) != hipSuccess) return fail("hipMemcpy", e);
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail("hipStreamSynchronize", e);
    (void)hipStreamDestroy(s);
    return OMDS_OK;
}

extern "C" {

int omds_sdf_data_shape(const omds_sdf_data_spec* spec, int64_t* rows, int32_t* cols) {
    SdfDataArgs a;
    std::string err;
    const int rc = omds_sdf_data_resolve(spec, &a, &err);
    if (rc) { g_create_err = "omds_sdf_data_shape: " + err; return rc; }
    if (rows) *rows = (int64_t)spec->n_cfg * (a.n_uniform + a.n_near);
    if (cols) *cols = a.nin + a.nlab;
    return OMDS_OK;
}

int omds_sdf_data_generate(int device, const omds_sdf_data_spec* spec, uint64_t seed, int64_t cfg0, int64_t n_cfg, float* out) {
    return sdf_data_run(device, spec, seed, cfg0, n_cfg, nullptr, nullptr, nullptr, out, "omds_sdf_data_generate");
}

int omds_sdf_data_from_draws(int device, const omds_sdf_data_spec* spec, const float* q, const float* p_uniform,
                             const float* near_offsets, int64_t n_cfg, float* out) {
    if (!q) { g_create_err = "omds_sdf_data_from_draws: q is NULL"; return OMDS_ERR_INVALID_ARG; }
    return sdf_data_run(device, spec, 0, 0, n_cfg, q, p_uniform, near_offsets, out, "omds_sdf_data_from_draws");
}

}  // extern "C"
