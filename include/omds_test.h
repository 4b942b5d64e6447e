/*
 * omds_test.h -- test hooks of the MI355X-native MPPI rollout path.  NOT part of the product ABI: libomds_hip.so does not export
 * them.  They exist in libomds_hip_test.so (`make test-lib`: the same objects except mlp_pack, screening, tail_kernel, propagate and train -- the
 * trainer's host side; its kernels are train_kernels.hip -- which are compiled with -DOMDS_TEST_HOOKS; the sin / cos hooks are csrc/trig_test.hip,
 * the raw Philox hook csrc/philox_test.hip, the top-k hook csrc/select_test.hip and the one-step modulation hook csrc/modulate_test.hip, files that only the test library links), which tests/ load explicitly (optimalmodulationds_amd._lib.load_test_hooks()).  Neither
 * library reads experiment environment variables.
 */
#ifndef OMDS_TEST_H
#define OMDS_TEST_H

#include "omds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Damages what the screening network sees so that the run-time checks of the screened step (omds.h, "Screening of pass 1") have
 * something to catch.  what = 0: zeroes fragment `index` (1 KiB) of the fp16 weight pack; what = 1: shifts obstacle `index` by
 * `value` along x in the screening kernel's input table only (until the next omds_set_obstacles).  The fp32 kernels are never
 * touched.                                                                                                               */
OMDS_API int omds_screen_debug_corrupt(omds_ctx* ctx, int what, int index, float value);
/* Process-wide: the tile shape of the step's tail kernels instead of the launcher's own choice -- tail_sel_rows in {0, 4, 16, 32}
 * for the screened step (4 = the backward on 4-row groups; ReLU networks without skip concatenations), tail_rows in {0, 4, 16, 32}
 * for the unscreened one (4 = forward and backward on 4-row groups); 0 = the launcher chooses again.  Every shape computes the same bits per row: the tests run them against
 * each other.                                                                                                             */
OMDS_API int omds_debug_force_tile_rows(int tail_sel_rows, int tail_rows);
/* Process-wide: every product of the trainer (omds_trainer_step / _eval) on the general GEMM kernel instead of the special-shape
 * kernels (tall 256-wide layers, thin first / last layers, thin weight gradients).  All of them sum in ascending k from zero, so
 * the runs must agree bit for bit: tests/test_gpu_train.py compares them on a batch that is not a multiple of the tile height. */
OMDS_API int omds_debug_trainer_general_gemm(int on);
/* The HOST half of omds_set_mlp_ex alone: argument validation, zero-padding to the kernels' width and every MFMA fragment pack
 * (fp32 forward / backward, 16-row, 4-row-group, fp16 screening slices), with no device and no context -- the sanitizer build
 * (`make asan`) runs it on the CPU (tests/test_asan_cpu.py).  *checksum = FNV-1a over ALL packs -- the screening pack, every pack
 * omds_set_mlp_ex uploads (one table serves both, MlpPacks::for_each_pack), and the screening pack again in a reversed unit order
 * -- *bytes = their total size (NULL = skip); the message of a failure through omds_last_error(NULL).                       */
OMDS_API int omds_test_pack_mlp(int n_dof, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W,
                                const float* const* b, int act, float out_div, int n_skips, const int32_t* skip_after,
                                uint64_t* checksum, int64_t* bytes);
/* The encoding's sin / cos (csrc/trig_device.h: omds_sinf / omds_cosf, what every feature kernel inlines) on the current device,
 * for tests/test_gpu_trig.py.  omds_test_trig: s[i] = sin x[i], c[i] = cos x[i] for n host floats (copied to the device and back).
 * omds_test_trig_sweep: every float whose bit pattern lies in [lo, hi) (hi <= 2^32); digests[0] / digests[1] = the sum mod 2^64
 * of splitmix64(bits(x) << 32 | bits(f(x))) for f = sin / cos -- order-independent, the sum oracle/chain_arith.c computes.   */
OMDS_API int omds_test_trig(const float* x, float* s, float* c, int64_t n);
OMDS_API int omds_test_trig_sweep(uint32_t lo, uint64_t hi, uint64_t* digests);
/* The generator behind both random kernels (csrc/philox_device.h: philox4x32_10, what k_sample and k_sdf_data inline) on the current
 * device, for tests/test_gpu_random_draws.py: out[i] = the four words of counter ctr[i] under key key[i], for n <= 2^28 host rows
 * (copied to the device and back).                                                                                             */
OMDS_API int omds_test_philox(const uint32_t* ctr /*[n][4]*/, const uint32_t* key /*[n][2]*/, uint32_t* out /*[n][4]*/, int64_t n);
/* The selection of the k closest obstacles (csrc/topk_device.h: topk_row, both of its paths) on the current device, for
 * tests/test_gpu_topk.py: the host rows are copied to the device, the production launcher (k_topk, one wave per row) runs on them
 * as it does on the pass-1 matrix, and idx_out[b][j] = the index of the j-th smallest entry of row b under the rule at the top of
 * topk_device.h.  1 <= k <= O.  (csrc/select_test.hip, a file that only the test library links.)                                */
OMDS_API int omds_test_topk(const float* rows /*[B][O]*/, int B, int O, int k, int32_t* idx_out /*[B][k]*/);
/* ONE horizon step `step` of the per-rollout modulation (csrc/step_device.h: modulate_core, everything of a step behind the distance
 * network) on caller-supplied inputs, with no network and no context, for tests/test_gpu_step_edges.py.  nsub = 1: the production
 * launcher omds_launch_modulate (k_modulate, n_dof = 1..7, the only caller with the SEDS branch); nsub = 16: a small kernel of
 * csrc/modulate_test.hip (a file that only the test library links) that calls modulate_core with 16 lanes per rollout the way the
 * fused step kernels do, n_dof = 2 or 7, no SEDS.  All arrays are host memory in the DEVICE's layouts (rollout index fastest).  Every
 * output buffer of the device is pre-filled with the byte 0xFF, so what the step did not write reads back as the bits 0xFFFFFFFF:
 * q_next is slab `step` of the rollouts (left alone at step == H), qdot is written at step 1 only.  maxact / phisum0 go in with
 * their previous contents and come back as the step left them.  OMDS_ERR_INVALID_ARG, before anything is launched: a size < 1,
 * n_dof > 7, nsub not 1 or 16, k > 32 (the fused tails' maximum), K > Kmax, d < n_dof or > 16, step outside 1..H, H > 64,
 * N > 2^16, Kmax > 2^10, rbf_p <= 0, a null array that the step reads or writes, seds_G outside 0..64 (or with A), nsub = 16 with
 * another n_dof or with SEDS, and with frame != 0: O outside 1..2^16, ldVel < d - n_dof or > 8, frame_max negative or NaN, a rowObs
 * entry outside [0, O).                                                                                                          */
typedef struct omds_test_modulate_args {
    int32_t n_dof, nsub, N, K, Kmax, k, d, step, H;
    int32_t frame, O, ldVel, seds_G;
    float frame_max, seds_lin_thr, seds_thr;
    omds_params prm;
    const float* qf;                 /* [n]                                                                        */
    const float* A;                  /* [n][n] matrix DS (velocity = (q - qf) @ A), NULL = linear                    */
    const float *seds_mu_in, *seds_b, *seds_sigma_inv, *seds_A, *seds_prior, *seds_den;   /* as omds_set_ds_seds takes them; seds_G > 0 */
    const float* vel;                /* [O][ldVel]; frame only                                                     */
    const int32_t* rowObs;           /* [N][k] obstacle of every gradient row; frame only                          */
    const float *q, *drow, *gradx;   /* [n][N], [N][k], [N][k][d]                                                  */
    const float *mu, *sigma, *alpha; /* [K][n][N], [K][N], [K][n][N]; K > 0                                        */
    float *maxact, *phisum0;         /* in / out: [Kmax][N], [Kmax]                                                */
    float *q_next, *qdot, *dist, *dot, *act, *normal, *kval;   /* out: [n][N], [n][N], [N], [N], [N], [n][N], [Kmax][N] */
} omds_test_modulate_args;
OMDS_API int omds_test_modulate(const omds_test_modulate_args* args);

#ifdef __cplusplus
}
#endif
#endif /* OMDS_TEST_H */
