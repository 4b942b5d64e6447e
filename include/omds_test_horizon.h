/*
 * omds_test_horizon.h -- test hook of screening under an obstacle horizon (csrc/screening.hip, omds_set_screening_horizon).  Like the
 * hooks of omds_test.h it is NOT part of the product ABI: libomds_hip.so does not export it, libomds_hip_test.so does (screening.hip
 * compiled with -DOMDS_TEST_HOOKS), and tests/test_gpu_screen_horizon.py loads it through optimalmodulationds_amd._lib.load_test_hooks().
 */
#ifndef OMDS_TEST_HORIZON_H
#define OMDS_TEST_HORIZON_H

#include "omds.h"

#ifdef __cplusplus
extern "C" {
#endif

/* shifts obstacle `index` by dx along x in the fp16 SCREENING table of slab `slab` only (the fp32 tables stay); undone when the
 * tables are rebuilt.  OMDS_ERR_NOT_INITIALISED unless fp16 slab tables exist (build them first: omds_get_obstacle_horizon). */
OMDS_API int omds_test_screen_corrupt_slab(omds_ctx* ctx, int slab, int index, float dx);

#ifdef __cplusplus
}
#endif
#endif /* OMDS_TEST_HORIZON_H */
