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
/* What the ordering launches (csrc/tile_order.hip) left at the last block-ordered launch: the keys the orders rank (rkey [n_traj],
 * okey [n_obs]: sign bits << 20 | index), the orders WITH their padding (rperm [omds_test_order_pad(n_traj)], operm
 * [omds_test_order_pad(n_obs)]; the padding names the last-ranked row again), and the key units of the propagate: unit [12], their
 * layer-1 weights W [12][32] over the feature slots, and the constants a rollout's (cR [12]) and an obstacle's (cO [12]) share is
 * compared against.  No output may be NULL.  Fails with OMDS_ERR_NOT_INITIALISED when no block-ordered launch has run on the context. */
#define OMDS_TEST_KEY_UNITS 12
#define OMDS_TEST_KEY_SLOTS 32
static inline int omds_test_order_pad(int n) { return ((n + 15) & ~15) + 16; }
OMDS_API int omds_test_tile_state(omds_ctx* ctx, uint32_t* rkey, uint32_t* okey, int32_t* rperm, int32_t* operm, int32_t* unit, float* W,
                                  float* cR, float* cO);
/* The [n_traj][n_obs] pass-1 matrix as the last horizon step of the last propagate left it on the Dense route (the caller's
 * obstacle index, whatever the order of the tiles).                                                                          */
OMDS_API int omds_test_read_dmin(omds_ctx* ctx, float* dmin);

#ifdef __cplusplus
}
#endif
#endif /* OMDS_TEST_TILES_H */
