// Test hooks (include/omds_test.h, libomds_hip_test.so only: the Makefile links this file into no other library): the encoding's
// sin / cos (trig_device.h) as k_encode and the feature kernels inline them, for tests/test_gpu_trig.py.
#include <algorithm>
#include <vector>

#include "omds_internal.h"
#include "omds_test.h"
#include "trig_device.h"

namespace {
__global__ void k_test_trig(const float* __restrict__ x, float* __restrict__ s, float* __restrict__ c, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    s[i] = omds_sinf(v);
    c[i] = omds_cosf(v);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// every bit pattern lo + i, i < count (lo + count <= 2^32): partial[2 b] / partial[2 b + 1] = workgroup b's sums mod 2^64 of
// splitmix64(bits(x) << 32 | bits(f(x))) for f = sin / cos; the host adds the partials (no atomics)
__global__ __launch_bounds__(256) void k_test_trig_sweep(uint32_t lo, uint64_t count, uint64_t* __restrict__ partial) {
    __shared__ uint64_t red[2][256];
    uint64_t ds = 0, dc = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (uint64_t)gridDim.x * 256) {
        const uint32_t b = lo + (uint32_t)i;
        const float x = __uint_as_float(b);
        ds += splitmix64((uint64_t)b << 32 | __float_as_uint(omds_sinf(x)));
        dc += splitmix64((uint64_t)b << 32 | __float_as_uint(omds_cosf(x)));
    }
    red[0][threadIdx.x] = ds;
    red[1][threadIdx.x] = dc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) {
            red[0][threadIdx.x] += red[0][threadIdx.x + off];
            red[1][threadIdx.x] += red[1][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = red[0][0];
        partial[2 * blockIdx.x + 1] = red[1][0];
    }
}
}   // namespace

#define HCK(expr) do { if ((expr) != hipSuccess) { rc = OMDS_ERR_HIP; goto done; } } while (0)

extern "C" OMDS_API int omds_test_trig(const float* x, float* s, float* c, int64_t n) {
    if (n < 0 || (n > 0 && (!x || !s || !c))) return OMDS_ERR_INVALID_ARG;
    if (n == 0) return OMDS_OK;
    int rc = OMDS_OK;
    float *dx = nullptr, *ds = nullptr, *dc = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    HCK(hipMalloc(&dx, bytes));
    HCK(hipMalloc(&ds, bytes));
    HCK(hipMalloc(&dc, bytes));
    HCK(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_test_trig, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, ds, dc, n);
    HCK(hipGetLastError());
    HCK(hipMemcpy(s, ds, bytes, hipMemcpyDeviceToHost));
    HCK(hipMemcpy(c, dc, bytes, hipMemcpyDeviceToHost));
done:
    for (float* p : {dx, ds, dc}) if (p) (void)hipFree(p);
    return rc;
}

extern "C" OMDS_API int omds_test_trig_sweep(uint32_t lo, uint64_t hi, uint64_t* digests) {
    if (!digests || hi < lo || hi > (1ull << 32)) return OMDS_ERR_INVALID_ARG;
    int rc = OMDS_OK;
    const uint64_t count = hi - lo;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(8 * (uint64_t)omds_cu_count(), (count + 255) / 256));
    uint64_t* dp = nullptr;
    std::vector<uint64_t> hp(2 * (size_t)blocks);
    HCK(hipMalloc(&dp, hp.size() * sizeof(uint64_t)));
    hipLaunchKernelGGL(k_test_trig_sweep, dim3(blocks), dim3(256), 0, 0, lo, count, dp);
    HCK(hipGetLastError());
    HCK(hipMemcpy(hp.data(), dp, hp.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    digests[0] = digests[1] = 0;
    for (unsigned b = 0; b < blocks; ++b) {
        digests[0] += hp[2 * (size_t)b];
        digests[1] += hp[2 * (size_t)b + 1];
    }
done:
    if (dp) (void)hipFree(dp);
    return rc;
}
#undef HCK
