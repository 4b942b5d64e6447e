// The trainer's ROUTE and SPLIT policy, stated once: which kernel of train_kernels.hip multiplies each of a layer's three products, and
// how the two contractions over the batch (the weight gradient, the bias gradient) are cut into partial sums.  train.hip computes the
// routes once per trainer and the split numbers per layer and step; the kernels include this for the constants; the stand-alone host
// build of tests/train_plan_host.cpp prints both for tests/test_train_plan_cpu.py.  Plain C++, integer arithmetic only, no HIP header.
#pragma once
#include <algorithm>
#include <cstddef>

constexpr int TM = 128, TN = 128, TK = 16;   // k_gemm: the output tile of a workgroup, the k step of its LDS staging
constexpr int THIN_KMAX = 32;                // k_gemm_thin: the contraction length a thread keeps in registers
constexpr int THINN_NMAX = 16;               // k_gemm_thin_out: output columns
constexpr int WG_TMAX = 32;                  // k_wgrad_thin: columns of the thin matrix

enum TrainRoute : int {
    TRAIN_NONE = 0,        // no product (the input gradient of layer 0)
    TRAIN_GENERAL,         // k_gemm
    TRAIN_TALL,            // k_pack256 + k_gemm_tall
    TRAIN_THIN,            // k_gemm_thin
    TRAIN_THIN_OUT,        // k_gemm_thin_out
    TRAIN_WGRAD_FIRST,     // k_wgrad_thin, first-layer form: the thin matrix is H_i [B x in] (dW's columns), the wide one G [B x out]
    TRAIN_WGRAD_LAST       // k_wgrad_thin, last-layer form: the thin matrix is G [B x out] (dW's rows), the wide one H_i [B x in]
};

// Layer i (in = dims[i] -> out = dims[i + 1]): Z [B x out] = H [B x in] . W^T, dW [out x in] = G^T . H, Gi [B x in] = G [B x out] . W
struct TrainLayerPlan {
    int forward;       // GENERAL | TALL | THIN | THIN_OUT
    int wgrad;         // GENERAL | WGRAD_FIRST | WGRAD_LAST
    int wgrad_tt;      // k_wgrad_thin's instantiation (4 | 12 | 16 | 32: the thin width rounded up), 0 on the general kernel
    int inputgrad;     // GENERAL | TALL | THIN, NONE for layer 0
};

// the tall kernels: a 256-long contraction (a row of A is one 1 KB DMA piece, A's row stride is K) into more than half of their 256 columns
inline bool train_tall_shape(int N, int K) { return N > 128 && N <= 256 && K == 256; }
// k_gemm_thin (N < 64: the thin-output products have a kernel of their own)
inline bool train_thin_shape(int N, int K) { return K <= THIN_KMAX && N >= 64 && N <= 256; }

inline int train_route_forward(int in, int out) {
    if (train_thin_shape(out, in)) return TRAIN_THIN;
    if (out <= THINN_NMAX && in <= 256 && in > THIN_KMAX) return TRAIN_THIN_OUT;
    if (train_tall_shape(out, in)) return TRAIN_TALL;
    return TRAIN_GENERAL;
}
inline int train_route_inputgrad(int in, int out) {
    if (train_thin_shape(in, out)) return TRAIN_THIN;
    if (train_tall_shape(in, out)) return TRAIN_TALL;
    return TRAIN_GENERAL;
}
inline int train_route_wgrad(int in, int out) {
    if (in <= WG_TMAX && out <= 4096 && out > WG_TMAX) return TRAIN_WGRAD_FIRST;
    if (out <= WG_TMAX && in <= 4096 && in > WG_TMAX) return TRAIN_WGRAD_LAST;
    return TRAIN_GENERAL;
}
inline int train_wgrad_tt(int T) { return T <= 4 ? 4 : T <= 12 ? 12 : T <= 16 ? 16 : 32; }

// plan [L] of the network dims [L + 1]; general: every product on k_gemm (the test hook omds_debug_trainer_general_gemm)
inline void train_plan_layers(const int* dims, int L, bool general, TrainLayerPlan* plan) {
    for (int i = 0; i < L; ++i) {
        const int in = dims[i], out = dims[i + 1];
        TrainLayerPlan& p = plan[i];
        p.forward = general ? TRAIN_GENERAL : train_route_forward(in, out);
        p.wgrad = general ? TRAIN_GENERAL : train_route_wgrad(in, out);
        p.wgrad_tt = p.wgrad == TRAIN_WGRAD_FIRST ? train_wgrad_tt(in) : p.wgrad == TRAIN_WGRAD_LAST ? train_wgrad_tt(out) : 0;
        p.inputgrad = i == 0 ? TRAIN_NONE : general ? TRAIN_GENERAL : train_route_inputgrad(in, out);
    }
}

// the floats of a trainer's partial-sum buffer: up to 256 split-K partials of the largest weight gradient
inline size_t train_partial_floats(const int* dims, int L) {
    size_t wmax = 0;
    for (int i = 0; i < L; ++i) wmax = std::max(wmax, (size_t)dims[i] * dims[i + 1]);
    return 256 * wmax;
}

// The batch-dependent numbers of layer in -> out at B rows, partial_floats = the floats of the trainer's partial-sum buffer.
// dW: the contraction over the batch is split so that ~1024 workgroups exist, at most 256 ways, never below 4 k steps a split, never
// past the buffer; chunk z is rows [z kchunk, min(B, (z + 1) kchunk)), kchunk a multiple of TK, and no chunk is empty.  Whichever
// kernel the weight gradient is routed to keeps these boundaries: the same partial sums, summed in the same order.
// db: the column sums of G over rsplit row ranges of rows_per rows.
struct TrainSplit {
    int splits, kchunk;
    int rsplit;
    size_t rows_per;
};
inline TrainSplit train_plan_split(int B, int in, int out, size_t partial_floats) {
    TrainSplit t;
    const int tiles = ((out + TM - 1) / TM) * ((in + TN - 1) / TN);
    int splits = std::max(1, std::min({256, 1024 / std::max(tiles, 1), (B + 4 * TK - 1) / (4 * TK)}));
    while ((size_t)splits * out * in > partial_floats) --splits;
    t.kchunk = ((B + splits - 1) / splits + TK - 1) / TK * TK;
    t.splits = (B + t.kchunk - 1) / t.kchunk;
    t.rsplit = std::max(1, std::min({2048, B / 256, (int)(partial_floats / (size_t)out)}));
    t.rows_per = ((size_t)B + t.rsplit - 1) / t.rsplit;
    return t;
}
