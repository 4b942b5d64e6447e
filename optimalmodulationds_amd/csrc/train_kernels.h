// What the trainer's host side (train.hip) needs of train_kernels.hip: one launcher per kernel family.  A launcher takes a stream,
// raw pointers and the numbers of train_plan_def.h, enqueues, and waits for nothing; which family multiplies a layer is the plan's
// decision, never a launcher's.  Matrices are row-major; W is a layer's [out x in] matrix with row stride ldw.
// (k_gemm's forward and input-gradient forms are omds_launch_linear_forward / _inputgrad of omds_internal.h, which wide_kernels.hip shares.)
#pragma once
#include "omds_internal.h"
#include "train_plan_def.h"

constexpr int TRAIN_MSE_BLOCKS = 1024;                              // k_mse writes at most this many partial sums
constexpr size_t TRAIN_PACK_BYTES = 8 * 32 * 64 * sizeof(float4);   // the fragment pack a tall product goes through

// k_gemm, weight-gradient form: P [z] [out x in] = the part of G^T . H over the rows of chunk z (TrainSplit), z < splits
void omds_launch_train_wgrad(hipStream_t s, const float* G, int out, const float* H, int in, float* P, int B, int splits, int kchunk);

// k_pack256 + k_gemm_tall (TRAIN_TALL): C [M x N] = A [M x 256] . B, B(k, n) = W[n][k] (trans = 0) or W[k][n] (trans = 1), 128 < N <= 256.
// epi 1 (forward): C = act(product + aux[n]), act < 0: none; epi 2 (input gradient): C = product * act'(aux[m][n]), aux = the stored activation.
// A's row stride is 256 and A is 16-byte aligned (any hipMalloc'ed matrix of a 256-wide layer); pack = TRAIN_PACK_BYTES of the caller's,
// re-packed on s by every call
void omds_launch_train_tall(hipStream_t s, int epi, float4* pack, const float* A, const float* W, int ldw, int trans, float* C, int ldc, int M, int N,
                            const float* aux, int act);
// k_gemm_thin (TRAIN_THIN): the same product and epilogues with K <= THIN_KMAX, 64 <= N <= 256
void omds_launch_train_thin(hipStream_t s, int epi, const float* A, int lda, const float* W, int ldw, int trans, float* C, int ldc, int M, int N, int K,
                            const float* aux, int act);
// k_gemm_thin_out (TRAIN_THIN_OUT): C [M x N] = act(A [M x K] . W^T + bias), N <= THINN_NMAX, K <= 256
void omds_launch_train_thin_out(hipStream_t s, const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K, const float* bias, int act);
// k_wgrad_thin<tt> (TRAIN_WGRAD_FIRST: thin_is_n = 1, X = G, Y = H; TRAIN_WGRAD_LAST: thin_is_n = 0, X = H, Y = G): X [B x Wd] wide, Y [B x T] thin,
// T <= tt; the partials of the general form above, chunk by chunk
void omds_launch_train_wgrad_thin(hipStream_t s, int tt, const float* X, int ldx, int Wd, const float* Y, int ldy, int T, int thin_is_n, float* P, int B,
                                  int splits, int kchunk, size_t cstride, int ldp);
// out [n] = P[0][.] + P[1][.] + ... + P[S - 1][.], in that order
void omds_launch_train_sum_partials(hipStream_t s, const float* P, int S, size_t n, float* out);
// H0 [B x 3 d] = [x, sin x, cos x]
void omds_launch_train_encode(hipStream_t s, const float* x, int B, int d, float* H0);
// G (if not null) = (2 / n) (pred - y); partial [blocks] = sums of (pred - y)^2 in double.  Returns blocks <= TRAIN_MSE_BLOCKS
int omds_launch_train_mse(hipStream_t s, const float* pred, const float* y, size_t n, float* G, double* partial);
// P [z] [N] = the column sums of G [B x N] over rows [z rows_per, min(B, (z + 1) rows_per)), z < rsplit
void omds_launch_train_colsum(hipStream_t s, const float* G, int B, int N, int rsplit, size_t rows_per, float* P);
// torch.optim.Adam's single-tensor step on n elements
void omds_launch_train_adam(hipStream_t s, float* p, const float* g, float* m, float* v, size_t n, float b1, float b2, float eps, float step_size, float bc2_sqrt);
