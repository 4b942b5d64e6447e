// SDF training on the device, the host side: struct omds_trainer and the omds_trainer_* C ABI (include/omds.h) over the launchers of
// train_kernels.hip.  No kernel in here.  One epoch is what mlp_learn/train_sdf.py:96-151 does: a FULL-BATCH forward of the distance
// network, F.mse_loss(reduction = 'mean'), backward through every layer and one torch.optim.Adam step.  Which kernel multiplies a
// layer, and how the contractions over the batch are split, is decided in train_plan_def.h and nowhere else: forward() and the
// backward loop of omds_trainer_step switch on the plan.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <new>
#include <vector>

#include "train_kernels.h"

struct TrainSet {                          // one data split on the device
    float* x = nullptr; float* y = nullptr;   // x [B, d], y [B, C]
    int B = 0, cap = 0;                    // rows it holds, rows x / y have room for
};

struct omds_trainer {
    int dev = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int L = 0, act = 0, d = 0;
    std::vector<int> dims;                 // [L + 1]: 3 d, hidden ..., C
    std::vector<TrainLayerPlan> plan;      // [L]: the route of every product (trainer_plan)
    bool plan_general = false;             // the test hook's state the plan was made under
    std::vector<float*> W, b, gW, gb, mW, mb, vW, vb;
    TrainSet set[2];                       // 0: the training set, 1: the validation set (omds_trainer_set_val_data)
    int cap = 0;                           // rows the activation / gradient buffers hold
    std::vector<float*> H;                 // [L + 1] activations: H[0] = encoded input ... H[L] = prediction
    float* G[2] = {nullptr, nullptr};      // gradient ping-pong [cap x max width]
    float4* pack256 = nullptr;             // MFMA fragment pack of the layer a tall GEMM is about to multiply (k_pack256), 256 KB
    float* partial = nullptr;              // split-K partials of the weight gradient / column-sum partials
    size_t partial_floats = 0;
    double* lossp = nullptr; double* h_lossp = nullptr;
    long long step = 0;
};

static thread_local std::string g_train_err;
#define TCK(expr)                                                                          \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) { tr->err = std::string(#expr) + ": " + hipGetErrorString(_e); return OMDS_ERR_HIP; } \
    } while (0)

#ifdef OMDS_TEST_HOOKS
// Test hook (include/omds_test.h, libomds_hip_test.so only): every product of the trainer on the general kernel k_gemm, so that a test
// can hold the special-shape kernels (k_gemm_tall, k_gemm_thin*, k_wgrad_thin) to its bits.  Process-wide.
static std::atomic<int> g_trainer_general{0};
extern "C" OMDS_API int omds_debug_trainer_general_gemm(int on) { g_trainer_general.store(on ? 1 : 0); return OMDS_OK; }
#define OMDS_TRAINER_GENERAL() (g_trainer_general.load() != 0)
#else
#define OMDS_TRAINER_GENERAL() false
#endif
// The routes: made at omds_trainer_create, made again at the top of forward() when the hook has flipped since
static void trainer_plan(omds_trainer* tr) {
    const bool general = OMDS_TRAINER_GENERAL();
    if (!tr->plan.empty() && general == tr->plan_general) return;
    tr->plan.resize((size_t)tr->L);
    train_plan_layers(tr->dims.data(), tr->L, general, tr->plan.data());
    tr->plan_general = general;
}

static void trainer_free_buffers(omds_trainer* tr) {   // activations and gradient ping-pong (sized by the larger data set)
    for (float* p : {tr->G[0], tr->G[1]}) if (p) (void)hipFree(p);
    tr->G[0] = tr->G[1] = nullptr;
    for (float*& p : tr->H) { if (p) (void)hipFree(p); p = nullptr; }
    tr->cap = 0;
}
static void trainer_free_data(omds_trainer* tr) {
    for (TrainSet& t : tr->set) {
        for (float* p : {t.x, t.y}) if (p) (void)hipFree(p);
        t = TrainSet();
    }
    trainer_free_buffers(tr);
}
static int trainer_reserve(omds_trainer* tr, int rows) {
    if (rows <= tr->cap) return OMDS_OK;
    trainer_free_buffers(tr);
    int wmax = 0;
    for (int v : tr->dims) wmax = std::max(wmax, v);
    for (int i = 0; i <= tr->L; ++i) TCK(hipMalloc(&tr->H[i], (size_t)rows * tr->dims[i] * 4));
    for (int i = 0; i < 2; ++i) TCK(hipMalloc(&tr->G[i], (size_t)rows * wmax * 4));
    tr->cap = rows;
    return OMDS_OK;
}
// Room for batch rows in split `which` (a grown split is empty until its caller has filled it and set B) and, in the activation
// buffers, for the larger of the two splits.  The stream is idle: every caller has synchronised it
static int trainer_reserve_set(omds_trainer* tr, int which, int batch) {
    TrainSet& t = tr->set[which];
    if (batch > t.cap) {
        for (float* p : {t.x, t.y}) if (p) (void)hipFree(p);
        t = TrainSet();
        TCK(hipMalloc(&t.x, (size_t)batch * tr->d * 4));
        TCK(hipMalloc(&t.y, (size_t)batch * tr->dims[tr->L] * 4));
        t.cap = batch;
    }
    return trainer_reserve(tr, which ? std::max(batch, tr->set[0].B) : batch);
}
// omds_trainer_set_data (which = 0) and omds_trainer_set_val_data (which = 1)
static int trainer_set_data(omds_trainer* tr, int which, const float* x, const float* y, int batch) {
    TCK(hipSetDevice(tr->dev));
    TCK(hipStreamSynchronize(tr->stream));
    if (int rc = trainer_reserve_set(tr, which, batch)) return rc;
    TrainSet& t = tr->set[which];
    TCK(hipMemcpy(t.x, x, (size_t)batch * tr->d * 4, hipMemcpyHostToDevice));
    TCK(hipMemcpy(t.y, y, (size_t)batch * tr->dims[tr->L] * 4, hipMemcpyHostToDevice));
    t.B = batch;
    return OMDS_OK;
}

static int forward(omds_trainer* tr, int B, const float* x) {
    hipStream_t s = tr->stream;
    trainer_plan(tr);
    omds_launch_train_encode(s, x, B, tr->d, tr->H[0]);
    for (int i = 0; i < tr->L; ++i) {
        const int in = tr->dims[i], out = tr->dims[i + 1];
        const int a = i + 1 < tr->L ? tr->act : -1;
        const float* H = tr->H[i];
        float* Z = tr->H[i + 1];
        switch (tr->plan[i].forward) {
        case TRAIN_THIN: omds_launch_train_thin(s, 1, H, in, tr->W[i], in, 0, Z, out, B, out, in, tr->b[i], a); break;
        case TRAIN_THIN_OUT: omds_launch_train_thin_out(s, H, in, tr->W[i], in, Z, out, B, out, in, tr->b[i], a); break;
        case TRAIN_TALL: omds_launch_train_tall(s, 1, tr->pack256, H, tr->W[i], in, 0, Z, out, B, out, tr->b[i], a); break;
        default: omds_launch_linear_forward(s, H, in, tr->W[i], tr->b[i], Z, out, B, a); break;
        }
    }
    TCK(hipGetLastError());   // an invalid launch configuration must not go on as a loss computed from stale buffers
    return OMDS_OK;
}

static int mse(omds_trainer* tr, int B, const float* y, float* G, double* loss) {
    const size_t n = (size_t)B * tr->dims[tr->L];
    const int blocks = omds_launch_train_mse(tr->stream, tr->H[tr->L], y, n, G, tr->lossp);
    TCK(hipGetLastError());
    TCK(hipMemcpyAsync(tr->h_lossp, tr->lossp, (size_t)blocks * 8, hipMemcpyDeviceToHost, tr->stream));
    TCK(hipStreamSynchronize(tr->stream));
    double sum = 0.0;
    for (int i = 0; i < blocks; ++i) sum += tr->h_lossp[i];
    *loss = sum / (double)n;
    return OMDS_OK;
}

extern "C" {

const char* omds_trainer_last_error(const omds_trainer* tr) { return tr ? tr->err.c_str() : g_train_err.c_str(); }

int omds_trainer_create(int device, int n_linear, const int32_t* dims, int act, omds_trainer** out) {
    if (!out || !dims || n_linear < 2 || n_linear > OMDS_MAX_HIDDEN + 1 || (act != OMDS_ACT_RELU && act != OMDS_ACT_TANH) || dims[0] % 3 != 0) {
        g_train_err = "omds_trainer_create: need 2 <= n_linear <= 9 Linear layers, dims[0] = 3 * (raw inputs), act RELU or TANH";
        return OMDS_ERR_INVALID_ARG;
    }
    for (int i = 0; i <= n_linear; ++i)
        if (dims[i] < 1 || dims[i] > 4096) { g_train_err = "omds_trainer_create: layer widths must be in 1 .. 4096"; return OMDS_ERR_INVALID_ARG; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_train_err = std::string("omds_trainer_create: no HIP device available (") + hipGetErrorString(e) + "); this library has no CPU fallback";
        return OMDS_ERR_HIP;
    }
    if (device < 0 || device >= ndev) { g_train_err = "omds_trainer_create: device ordinal out of range"; return OMDS_ERR_INVALID_ARG; }
    omds_trainer* tr = new (std::nothrow) omds_trainer();
    if (!tr) { g_train_err = "omds_trainer_create: out of host memory"; return OMDS_ERR_INVALID_ARG; }
    tr->dev = device; tr->L = n_linear; tr->act = act; tr->d = dims[0] / 3;
    tr->dims.assign(dims, dims + n_linear + 1);
    trainer_plan(tr);
    auto fail = [&](const char* what, hipError_t err) { g_train_err = std::string(what) + ": " + hipGetErrorString(err); omds_trainer_destroy(tr); return OMDS_ERR_HIP; };
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&tr->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    for (int i = 0; i < n_linear; ++i) {
        const size_t nw = (size_t)dims[i] * dims[i + 1], nb = dims[i + 1];
        for (auto* vec : {&tr->W, &tr->gW, &tr->mW, &tr->vW}) {
            float* p = nullptr;
            if ((e = hipMalloc(&p, nw * 4)) != hipSuccess) return fail("hipMalloc", e);
            (void)hipMemsetAsync(p, 0, nw * 4, tr->stream);
            vec->push_back(p);
        }
        for (auto* vec : {&tr->b, &tr->gb, &tr->mb, &tr->vb}) {
            float* p = nullptr;
            if ((e = hipMalloc(&p, nb * 4)) != hipSuccess) return fail("hipMalloc", e);
            (void)hipMemsetAsync(p, 0, nb * 4, tr->stream);
            vec->push_back(p);
        }
    }
    tr->H.assign(n_linear + 1, nullptr);
    tr->partial_floats = train_partial_floats(tr->dims.data(), n_linear);
    if ((e = hipMalloc(&tr->partial, tr->partial_floats * 4)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&tr->pack256, TRAIN_PACK_BYTES)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&tr->lossp, TRAIN_MSE_BLOCKS * 8)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipHostMalloc(&tr->h_lossp, TRAIN_MSE_BLOCKS * 8)) != hipSuccess) return fail("hipHostMalloc", e);
    (void)hipStreamSynchronize(tr->stream);
    *out = tr;
    return OMDS_OK;
}

void omds_trainer_destroy(omds_trainer* tr) {
    if (!tr) return;
    (void)hipSetDevice(tr->dev);
    if (tr->stream) (void)hipStreamSynchronize(tr->stream);
    trainer_free_data(tr);
    for (auto* vec : {&tr->W, &tr->b, &tr->gW, &tr->gb, &tr->mW, &tr->mb, &tr->vW, &tr->vb})
        for (float* p : *vec) if (p) (void)hipFree(p);
    if (tr->partial) (void)hipFree(tr->partial);
    if (tr->pack256) (void)hipFree(tr->pack256);
    if (tr->lossp) (void)hipFree(tr->lossp);
    if (tr->h_lossp) (void)hipHostFree(tr->h_lossp);
    if (tr->stream) (void)hipStreamDestroy(tr->stream);
    delete tr;
}

int omds_trainer_set_weights(omds_trainer* tr, const float* const* W, const float* const* b) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    if (!W || !b) { tr->err = "omds_trainer_set_weights: null argument"; return OMDS_ERR_INVALID_ARG; }
    TCK(hipSetDevice(tr->dev));
    for (int i = 0; i < tr->L; ++i) {
        const size_t nw = (size_t)tr->dims[i] * tr->dims[i + 1], nb = tr->dims[i + 1];
        TCK(hipMemcpy(tr->W[i], W[i], nw * 4, hipMemcpyHostToDevice));
        TCK(hipMemcpy(tr->b[i], b[i], nb * 4, hipMemcpyHostToDevice));
        for (float* p : {tr->mW[i], tr->vW[i]}) TCK(hipMemset(p, 0, nw * 4));   // a fresh optimizer state, like a new torch.optim.Adam
        for (float* p : {tr->mb[i], tr->vb[i]}) TCK(hipMemset(p, 0, nb * 4));
    }
    tr->step = 0;
    return OMDS_OK;
}

int omds_trainer_get_weights(omds_trainer* tr, float* const* W, float* const* b) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    if (!W || !b) { tr->err = "omds_trainer_get_weights: null argument"; return OMDS_ERR_INVALID_ARG; }
    TCK(hipSetDevice(tr->dev));
    TCK(hipStreamSynchronize(tr->stream));
    for (int i = 0; i < tr->L; ++i) {
        TCK(hipMemcpy(W[i], tr->W[i], (size_t)tr->dims[i] * tr->dims[i + 1] * 4, hipMemcpyDeviceToHost));
        TCK(hipMemcpy(b[i], tr->b[i], (size_t)tr->dims[i + 1] * 4, hipMemcpyDeviceToHost));
    }
    return OMDS_OK;
}

int omds_trainer_set_data(omds_trainer* tr, const float* x, const float* y, int batch) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    if (!x || !y || batch < 1) { tr->err = "omds_trainer_set_data: need batch >= 1 and non-null x [B, d], y [B, C]"; return OMDS_ERR_INVALID_ARG; }
    return trainer_set_data(tr, 0, x, y, batch);
}

// The validation split (train_sdf.py:84-86, 117-121) beside the training set: evaluated by omds_trainer_eval(which = 1) with the
// trainer's current weights -- no weight copy, no second trainer, the optimizer state untouched.
int omds_trainer_set_val_data(omds_trainer* tr, const float* x, const float* y, int batch) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    if (!x || !y || batch < 1) { tr->err = "omds_trainer_set_val_data: need batch >= 1 and non-null x [B, d], y [B, C]"; return OMDS_ERR_INVALID_ARG; }
    return trainer_set_data(tr, 1, x, y, batch);
}

// SDF training data made on the device straight into the training set (which = 0) or the validation set (which = 1): the rows of
// omds_sdf_data_generate, split into x [B, d] and y [B, C] by the kernel's stores, on the trainer's stream, no host copy.
int omds_trainer_generate_data(omds_trainer* tr, const omds_sdf_data_spec* spec, uint64_t seed, int64_t cfg0, int64_t n_cfg, int which) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    SdfDataArgs a;
    std::string err;
    if (omds_sdf_data_resolve(spec, &a, &err)) { tr->err = "omds_trainer_generate_data: " + err; return OMDS_ERR_INVALID_ARG; }
    if (which != 0 && which != 1) { tr->err = "omds_trainer_generate_data: which must be 0 (training set) or 1 (validation set)"; return OMDS_ERR_INVALID_ARG; }
    if (a.nin != tr->d || a.nlab != tr->dims[tr->L]) {
        tr->err = "omds_trainer_generate_data: the spec's rows have " + std::to_string(a.nin) + " inputs and " + std::to_string(a.nlab) +
                  " labels, the trainer takes " + std::to_string(tr->d) + " and " + std::to_string(tr->dims[tr->L]);
        return OMDS_ERR_INVALID_ARG;
    }
    const int64_t R = (int64_t)a.n_uniform + a.n_near;
    if (n_cfg < 1 || n_cfg > INT32_MAX / R) { tr->err = "omds_trainer_generate_data: need n_cfg >= 1 and n_cfg * (n_uniform + n_near) rows < 2^31"; return OMDS_ERR_INVALID_ARG; }
    if (cfg0 < 0 || cfg0 > INT64_MAX - n_cfg) { tr->err = "omds_trainer_generate_data: cfg0 must be >= 0 and cfg0 + n_cfg must fit int64"; return OMDS_ERR_INVALID_ARG; }
    const int batch = (int)(n_cfg * R);
    TCK(hipSetDevice(tr->dev));
    TCK(hipStreamSynchronize(tr->stream));
    if (int rc = trainer_reserve_set(tr, which, batch)) return rc;
    TrainSet& t = tr->set[which];
    omds_launch_sdf_data(tr->stream, a, seed, cfg0, n_cfg, nullptr, nullptr, nullptr, t.x, t.y);
    TCK(hipGetLastError());
    t.B = batch;
    return OMDS_OK;
}

// forward + F.mse_loss with the current weights, no update: which = 0 the training set, 1 the validation set (train_sdf.py:117-121)
int omds_trainer_eval(omds_trainer* tr, int which, float* mse_out, float* pred_out) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    if (which != 0 && which != 1) { tr->err = "omds_trainer_eval: which must be 0 (training set) or 1 (validation set)"; return OMDS_ERR_INVALID_ARG; }
    const TrainSet& t = tr->set[which];
    const int B = t.B;
    if (B < 1) { tr->err = which ? "omds_trainer_eval: no validation set (omds_trainer_set_val_data)" : "omds_trainer_eval: no data set (omds_trainer_set_data)"; return OMDS_ERR_NOT_INITIALISED; }
    TCK(hipSetDevice(tr->dev));
    int rc;
    if ((rc = trainer_reserve(tr, B))) return rc;
    if ((rc = forward(tr, B, t.x))) return rc;
    double loss = 0.0;
    if ((rc = mse(tr, B, t.y, nullptr, &loss))) return rc;
    if (mse_out) *mse_out = (float)loss;
    if (pred_out) TCK(hipMemcpy(pred_out, tr->H[tr->L], (size_t)B * tr->dims[tr->L] * 4, hipMemcpyDeviceToHost));
    return OMDS_OK;
}

// torch.optim.Adam's state (exp_avg, exp_avg_sq per parameter, the step count), for checkpoints in the reference's format
// (train_sdf.py:130-138 saves optimizer.state_dict()) and for resuming: arrays like omds_trainer_get_weights (NULL array = skip).
int omds_trainer_get_optimizer_state(omds_trainer* tr, float* const* mW, float* const* mb, float* const* vW, float* const* vb, int64_t* step) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    TCK(hipSetDevice(tr->dev));
    TCK(hipStreamSynchronize(tr->stream));
    for (int i = 0; i < tr->L; ++i) {
        const size_t nw = (size_t)tr->dims[i] * tr->dims[i + 1] * 4, nb = (size_t)tr->dims[i + 1] * 4;
        if (mW && mW[i]) TCK(hipMemcpy(mW[i], tr->mW[i], nw, hipMemcpyDeviceToHost));
        if (vW && vW[i]) TCK(hipMemcpy(vW[i], tr->vW[i], nw, hipMemcpyDeviceToHost));
        if (mb && mb[i]) TCK(hipMemcpy(mb[i], tr->mb[i], nb, hipMemcpyDeviceToHost));
        if (vb && vb[i]) TCK(hipMemcpy(vb[i], tr->vb[i], nb, hipMemcpyDeviceToHost));
    }
    if (step) *step = tr->step;
    return OMDS_OK;
}
int omds_trainer_set_optimizer_state(omds_trainer* tr, const float* const* mW, const float* const* mb, const float* const* vW,
                                     const float* const* vb, int64_t step) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    if (!mW || !mb || !vW || !vb || step < 0) { tr->err = "omds_trainer_set_optimizer_state: null argument or negative step"; return OMDS_ERR_INVALID_ARG; }
    for (int i = 0; i < tr->L; ++i)
        if (!mW[i] || !mb[i] || !vW[i] || !vb[i]) { tr->err = "omds_trainer_set_optimizer_state: null array"; return OMDS_ERR_INVALID_ARG; }
    TCK(hipSetDevice(tr->dev));
    TCK(hipStreamSynchronize(tr->stream));
    for (int i = 0; i < tr->L; ++i) {
        const size_t nw = (size_t)tr->dims[i] * tr->dims[i + 1] * 4, nb = (size_t)tr->dims[i + 1] * 4;
        TCK(hipMemcpy(tr->mW[i], mW[i], nw, hipMemcpyHostToDevice));
        TCK(hipMemcpy(tr->vW[i], vW[i], nw, hipMemcpyHostToDevice));
        TCK(hipMemcpy(tr->mb[i], mb[i], nb, hipMemcpyHostToDevice));
        TCK(hipMemcpy(tr->vb[i], vb[i], nb, hipMemcpyHostToDevice));
    }
    tr->step = step;
    return OMDS_OK;
}

// one epoch of train_sdf.py:105-113 on the whole data set: forward, mse_loss, backward, Adam step.  loss_out = the loss BEFORE the step
int omds_trainer_step(omds_trainer* tr, float lr, float beta1, float beta2, float eps, float* loss_out) {
    if (!tr) return OMDS_ERR_INVALID_ARG;
    const TrainSet& t = tr->set[0];
    if (t.B < 1) { tr->err = "omds_trainer_step: no data set (omds_trainer_set_data)"; return OMDS_ERR_NOT_INITIALISED; }
    TCK(hipSetDevice(tr->dev));
    hipStream_t s = tr->stream;
    const int B = t.B, L = tr->L;
    int rc;
    if ((rc = trainer_reserve(tr, B))) return rc;
    if ((rc = forward(tr, B, t.x))) return rc;      // (the plan is current behind it)
    double loss = 0.0;
    float* G = tr->G[0];
    float* Gn = tr->G[1];
    if ((rc = mse(tr, B, t.y, G, &loss))) return rc;
    if (loss_out) *loss_out = (float)loss;
    for (int i = L - 1; i >= 0; --i) {
        const int in = tr->dims[i], out = tr->dims[i + 1];
        const TrainLayerPlan& p = tr->plan[i];
        const TrainSplit sp = train_plan_split(B, in, out, tr->partial_floats);
        const float* H = tr->H[i];
        // dW = G^T . H_i: partials over the chunks of the batch, summed in order
        switch (p.wgrad) {
        case TRAIN_WGRAD_FIRST: omds_launch_train_wgrad_thin(s, p.wgrad_tt, G, out, out, H, in, in, 1, tr->partial, B, sp.splits, sp.kchunk, (size_t)out * in, in); break;
        case TRAIN_WGRAD_LAST: omds_launch_train_wgrad_thin(s, p.wgrad_tt, H, in, in, G, out, out, 0, tr->partial, B, sp.splits, sp.kchunk, (size_t)out * in, in); break;
        default: omds_launch_train_wgrad(s, G, out, H, in, tr->partial, B, sp.splits, sp.kchunk); break;
        }
        omds_launch_train_sum_partials(s, tr->partial, sp.splits, (size_t)out * in, tr->gW[i]);
        // db = column sums of G
        omds_launch_train_colsum(s, G, B, out, sp.rsplit, sp.rows_per, tr->partial);
        omds_launch_train_sum_partials(s, tr->partial, sp.rsplit, (size_t)out, tr->gb[i]);
        if (p.inputgrad == TRAIN_NONE) continue;
        // gradient at this layer's input, through the activation of the layer in front
        switch (p.inputgrad) {
        case TRAIN_THIN: omds_launch_train_thin(s, 2, G, out, tr->W[i], in, 1, Gn, in, B, in, out, H, tr->act); break;
        case TRAIN_TALL: omds_launch_train_tall(s, 2, tr->pack256, G, tr->W[i], in, 1, Gn, in, B, in, H, tr->act); break;
        default: omds_launch_linear_inputgrad(s, G, out, tr->W[i], in, Gn, B, H, tr->act); break;
        }
        std::swap(G, Gn);
    }
    tr->step++;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)tr->step), bc2 = 1.0 - std::pow((double)beta2, (double)tr->step);
    const float step_size = (float)((double)lr / bc1), bc2_sqrt = (float)std::sqrt(bc2);
    for (int i = 0; i < L; ++i) {
        const size_t nw = (size_t)tr->dims[i] * tr->dims[i + 1], nb = tr->dims[i + 1];
        omds_launch_train_adam(s, tr->W[i], tr->gW[i], tr->mW[i], tr->vW[i], nw, beta1, beta2, eps, step_size, bc2_sqrt);
        omds_launch_train_adam(s, tr->b[i], tr->gb[i], tr->mb[i], tr->vb[i], nb, beta1, beta2, eps, step_size, bc2_sqrt);
    }
    TCK(hipGetLastError());
    TCK(hipStreamSynchronize(s));
    return OMDS_OK;
}

}  // extern "C"
