// Test hook (include/omds_test.h, libomds_hip_test.so only: the Makefile links this file into no other library): the raw words of
// philox4x32_10 (philox_device.h) as k_sample and k_sdf_data inline it, for tests/test_gpu_random_draws.py.
#include "omds_internal.h"
#include "omds_test.h"
#include "philox_device.h"

namespace {
__global__ __launch_bounds__(256) void k_test_philox(const uint32_t* __restrict__ ctr, const uint32_t* __restrict__ key,
                                                     uint32_t* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    philox4x32_10(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], out + 4 * i);
}
}   // namespace

#define HCK(expr) do { if ((expr) != hipSuccess) { rc = OMDS_ERR_HIP; goto done; } } while (0)

extern "C" OMDS_API int omds_test_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out, int64_t n) {
    if (n < 0 || n > (int64_t)1 << 28 || (n > 0 && (!ctr || !key || !out))) return OMDS_ERR_INVALID_ARG;
    if (n == 0) return OMDS_OK;
    int rc = OMDS_OK;
    uint32_t *dc = nullptr, *dk = nullptr, *dout = nullptr;
    const size_t words = (size_t)n * sizeof(uint32_t);
    HCK(hipMalloc(&dc, 4 * words));
    HCK(hipMalloc(&dk, 2 * words));
    HCK(hipMalloc(&dout, 4 * words));
    HCK(hipMemcpy(dc, ctr, 4 * words, hipMemcpyHostToDevice));
    HCK(hipMemcpy(dk, key, 2 * words, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_philox, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dc, dk, dout, n);
    HCK(hipGetLastError());
    HCK(hipMemcpy(out, dout, 4 * words, hipMemcpyDeviceToHost));
done:
    for (uint32_t* p : {dc, dk, dout}) if (p) (void)hipFree(p);
    return rc;
}
#undef HCK
