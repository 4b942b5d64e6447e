/*
 * omds_test_tiles.h -- test hooks of the block-ordered pass 1 (csrc/tile_order.hip, k_pass1_dyn_blk).  Like the hooks of omds_test.h
 * they are NOT part of the product ABI: libomds_hip.so does not export them, libomds_hip_test.so does (propagate.hip compiled with
 * -DOMDS_TEST_HOOKS), and tests/test_gpu_coherent_tiles.py loads them through optimalmodulationds_amd._lib.load_test_hooks().
 */
#ifndef OMDS_TEST_TILES_H
#define OMDS_TEST_TILES_H

#include "omds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rollout order of the last block-ordered launch (rperm, n_traj entries) and the obstacle order of its propagate (operm, n_obs
 * entries); either may be NULL.  Fails with OMDS_ERR_NOT_INITIALISED when no block-ordered launch has run on the context.      */
OMDS_API int omds_test_tile_orders(omds_ctx* ctx, int32_t* rperm, int32_t* operm);
/* The [n_traj][n_obs] pass-1 matrix as the last horizon step of the last propagate left it on the Dense route (the caller's
 * obstacle index, whatever the order of the tiles).                                                                          */
OMDS_API int omds_test_read_dmin(omds_ctx* ctx, float* dmin);

#ifdef __cplusplus
}
#endif
#endif /* OMDS_TEST_TILES_H */
