// Host build of the encoding's sin / cos (optimalmodulationds_amd/csrc/trig_device.h) for tests/test_trig_cpu.py and
// tests/test_gpu_trig.py.  Compiled at test time by g++ -O2 -mfma -ffp-contract=off -fopenmp (tests/helpers.py: trig_host): the header's
// functions are the ones the kernels inline, only the compiler differs.
#include <cstdint>
#include <cstring>

#include "../optimalmodulationds_amd/csrc/trig_device.h"

namespace {
// the digest of one (input, output) pair: splitmix64 of bits(x) << 32 | bits(f(x)); a sweep sums them mod 2^64 (order-independent)
inline uint64_t mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
}   // namespace

extern "C" {

void omds_host_sin(const float* x, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = omds_sinf(x[i]); }
void omds_host_cos(const float* x, float* y, long n) { for (long i = 0; i < n; ++i) y[i] = omds_cosf(x[i]); }

// every float whose bit pattern lies in [lo, hi): out[0] = digest of omds_sinf, out[1] = digest of omds_cosf
void omds_host_trig_digest(uint32_t lo, uint64_t hi, uint64_t* out) {
    uint64_t ds = 0, dc = 0;
#pragma omp parallel for schedule(static) num_threads(8) reduction(+ : ds, dc)
    for (uint64_t u = lo; u < hi; ++u) {
        float x;
        const uint32_t b = (uint32_t)u;
        std::memcpy(&x, &b, 4);
        ds += mix((uint64_t)b << 32 | bits(omds_sinf(x)));
        dc += mix((uint64_t)b << 32 | bits(omds_cosf(x)));
    }
    out[0] = ds;
    out[1] = dc;
}
}
